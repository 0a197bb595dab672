"""Opt-in noise pre-whitening (baz_music_set_noise_covariance) on the MI355X.

The main pins: with Rn a diagonal of powers of four the transform is exact, so a whitened context fed x and a plain context on the
table W a fed W x must agree bit for bit on every scan path; the stage alone against the numpy restatement at its derived bound; the
table on the device against the host form of the kernel's own routine, image by image; a general Rn end to end against the fp64
oracle evaluated on the device's own R' and the host's whitened table, at each path's bound; the two coloured-noise scenes with Rn
measured on the device; composition, refusals, off == the context never set, and changes of Rn beside a submitting thread."""
import threading

import numpy as np
import pytest

import order_ref as oref
import power_ref as pr
import whiten_ref as wr
from helpers import assert_doa_within_bound, assert_spectrum_within_bound
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

IMAGES = range(0, 9)


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _path(ctx):
    return "int8" if ctx.stage_name(2).startswith("bazmusic::scan_i8_kernel") else "fp64"


def _scene(m, n, K, res, batch, seed, snr_db=20.0):
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    angles = (40.3, 121.7)[:n] if n <= 2 else tuple(np.linspace(23.0, 301.0, n))
    return table, mo.synth_items(batch, m, m * K, arr, mo.FREQUENCY, mo.SPACING, angles_deg=angles, snr_db=snr_db, seed=seed)


def _general_rn(m, seed):
    """A general complex noise covariance: unequal channel powers (+-6 dB) and correlation between neighbours."""
    rng = np.random.default_rng(seed)
    g = 10.0 ** (rng.uniform(-6.0, 6.0, m) / 20.0)
    C = np.eye(m, dtype=np.complex128)
    for i in range(m - 1):
        C[i + 1, i] = 0.3 * np.exp(2j * np.pi * rng.uniform())
        C[i, i + 1] = np.conj(C[i + 1, i])
    return (g[:, None] * C * g[None, :]) * 0.01


def _diag_case(m, seed):
    """Rn = diag(4^k), k in -3 .. 3: (Rn, w = 2^-k): W = diag(w), W x exact in complex64, W R W^H exact."""
    k = np.random.default_rng(seed).integers(-3, 4, m)
    return np.diag(4.0 ** k).astype(np.complex128), 2.0 ** (-k.astype(np.float64))


def _run_device(ctx, items, want_spec=True):
    import torch
    B = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    ang = torch.full((B, ctx.n), -1.0, dtype=torch.float32, device="cuda")
    lvl = torch.full((B, ctx.n), -1.0, dtype=torch.float32, device="cuda")
    spec = torch.full((B, ctx.res), -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    torch.cuda.synchronize()
    ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr() if want_spec else None)
    ctx.sync()
    return ang.cpu().numpy(), lvl.cpu().numpy(), spec.cpu().numpy() if want_spec else None


def _device_cov(ctx, items, m):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _device_whiten(ctx, R):
    import torch
    B = R.shape[0]
    per = R[0].size * 2
    rin = torch.from_numpy(np.ascontiguousarray(R).view(np.float64).reshape(B, per)).cuda()
    rout = torch.full((B + 1, per), np.nan, dtype=torch.float64, device="cuda")       # (one matrix of guard behind the batch)
    torch.cuda.synchronize()
    ctx.debug_whiten(rin.data_ptr(), B, rout.data_ptr())
    ctx.sync()
    out = rout.cpu().numpy()
    assert np.all(np.isnan(out[B])), "debug_whiten wrote behind its batch"
    return out[:B].view(np.complex128).reshape(R.shape)


def _assert_outputs_equal(a, b, what):
    for name, x, y in zip(("ang", "lvl", "spectrum"), a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(_f32bits(x), _f32bits(y)), "%s: %s differs" % (what, name)


def _assert_images(ctx, m, n, res, table, what):
    """Every image of the context that exists equals the host builders' image of `table`, byte for byte."""
    capi = _capi()
    seen = 0
    for which in IMAGES:
        got = ctx.debug_table_image(which)
        if got is None:
            continue
        want = capi.debug_host_table_image(m, n, res, table, which)
        assert want is not None and np.array_equal(got, want), "%s: table image %d differs from the host image" % (what, which)
        seen += 1
    assert seen >= 2, what


# name, m, n, K, res, spectrum port
SHAPES = [
    ("m3", 3, 2, 16, 361, True),
    ("m4", 4, 2, 64, 360, True),
    ("m5", 5, 2, 40, 121, True),
    ("m8_int8_port", 8, 2, 64, 3600, True),
    ("m8_coarse_gate_no_port", 8, 2, 64, 3600, False),
    ("m16", 16, 2, 64, 720, True),
    ("m24_wide", 24, 2, 8, 360, True),
    ("m33_wide_general_scan", 33, 9, 64, 90, True),
    ("m64_wide", 64, 3, 66, 256, True),
]
FUSED = ("m4_fused_shape", 4, 2, 256, 360, True)
BATCH = 23


# ---- 4. the exact case, bit for bit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,m,n,K,res,port", SHAPES, ids=[s[0] for s in SHAPES])
def test_power_of_four_diagonal_equals_a_plain_context_on_the_scaled_table_and_data(name, m, n, K, res, port, gpu_device):
    capi = _capi()
    table, items = _scene(m, n, K, res, BATCH, seed=900 + m)
    Rn, w = _diag_case(m, 40 + m)
    wtable = (table * w[None, :].astype(np.float32)).astype(np.complex64)                         # exact: powers of two
    witems = (items.reshape(BATCH, K, m) * w[None, None, :].astype(np.float32)).reshape(BATCH, K * m).astype(np.complex64)
    assert np.array_equal(capi.whiten_table(table, np.diag(w).astype(np.complex128)), wtable)     # (values: a -0 may come back as +0)
    with capi.Context(m, n, m * K, res, table) as a, capi.Context(m, n, m * K, res, wtable) as b:
        a.set_noise_covariance(Rn)
        assert np.array_equal(a.get_noise_covariance(), Rn) and b.get_noise_covariance() is None
        oa = _run_device(a, items, port)
        ob = _run_device(b, witems, port)
        _assert_outputs_equal(oa, ob, name)
        assert oa[1].any()
        assert a.stage_name(capi.STAGE_SCAN) == b.stage_name(capi.STAGE_SCAN), (a.stage_name(capi.STAGE_SCAN), b.stage_name(capi.STAGE_SCAN))
        if name == "m33_wide_general_scan":
            assert "topn_wide_kernel" in a.stage_name(capi.STAGE_MERGE), a.stage_name(capi.STAGE_MERGE)
        # the stage's own output is the plain context's covariance, bit for bit (upper triangle and diagonal included)
        Ra = _device_whiten(a, _device_cov(a, items, m))
        Rb = _device_cov(b, witems, m)
        assert np.array_equal(Ra, Rb)
        # the transform changes something unless W = I
        if not np.all(w == 1.0):
            with capi.Context(m, n, m * K, res, table) as plain:
                assert not np.array_equal(_f32bits(_run_device(plain, items, port)[1]), _f32bits(oa[1]))


# ---- 5. the stage alone ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [2, 4, 5, 8, 16, 17, 40, 64])
def test_whiten_stage_is_the_restatement_within_its_bound(m, gpu_device):
    capi = _capi()
    n, K, res = 1, 12, 64
    table, items = _scene(m, n, K, res, 23, seed=950 + m, snr_db=10.0)
    Rn = _general_rn(m, 60 + m)
    W = capi.whitening_factor(Rn)
    with capi.Context(m, n, m * K, res, table) as ctx:
        with pytest.raises(capi.MusicError):
            _device_whiten(ctx, np.zeros((1, m, m), np.complex128))               # off: the tap has no W
        ctx.set_noise_covariance(Rn)
        R = _device_cov(ctx, items, m)
        for B in (1, 23):
            got = _device_whiten(ctx, R[:B])
            ref = wr.whiten_cov(R[:B], W)
            tol = wr.whiten_cov_tol(R[:B], W)
            assert np.all(np.abs(got.real - ref.real) <= tol) and np.all(np.abs(got.imag - ref.imag) <= tol), \
                "m=%d B=%d: worst %.3g of the bound" % (m, B, max(np.max(np.abs(got.real - ref.real) / tol), np.max(np.abs(got.imag - ref.imag) / tol)))
            low = np.tril(got, -1)
            assert np.array_equal(np.triu(got, 1), np.conj(np.swapaxes(low, 1, 2)))                 # upper == conj(lower), exactly
            d = np.diagonal(got, axis1=1, axis2=2)
            assert np.array_equal(_bits(d.imag), _bits(np.zeros_like(d.imag)))                      # +0, not -0
        # only the lower triangle and the real diagonal of R are read
        junk = R.copy()
        junk[:, np.triu_indices(m, 1)[0], np.triu_indices(m, 1)[1]] = 3.0 - 2.0j
        junk[:, np.arange(m), np.arange(m)] += 7.0j
        full = _device_whiten(ctx, R)
        assert np.array_equal(_bits(_device_whiten(ctx, junk)), _bits(full))
        # a NaN item changes only its own output
        bad = R.copy()
        bad[7] = np.nan
        out = _device_whiten(ctx, bad)
        keep = np.arange(23) != 7
        assert np.array_equal(_bits(out[keep]), _bits(full[keep])) and np.all(np.isnan(out[7].real))


# ---- 6. the table on the device ------------------------------------------------------------------------------------------------------------

TABLE_SHAPES = [s for s in SHAPES if s[0] in ("m3", "m4", "m8_int8_port", "m16", "m24_wide", "m64_wide")]


@pytest.mark.parametrize("name,m,n,K,res,port", TABLE_SHAPES, ids=[s[0] for s in TABLE_SHAPES])
def test_device_table_is_the_host_routines_table(name, m, n, K, res, port, gpu_device):
    """Context A: general Rn.  Context B: plain, created on whiten_table's output, with Rn2 = I set, so that both run the stage.  Every
    table image of A equals the host builders' image of the host-whitened table byte for byte (debug_table_image is the table tap);
    B's whitened table is its own table (W = I returns the bytes).  The covariances differ (W against I), so the outputs are compared
    by test_general_rn_end_to_end's bounded comparison, not here."""
    capi = _capi()
    table, items = _scene(m, n, K, res, 4, seed=970 + m)
    Rn = _general_rn(m, 80 + m)
    wtable = capi.whiten_table(table, capi.whitening_factor(Rn))
    with capi.Context(m, n, m * K, res, table) as a, capi.Context(m, n, m * K, res, wtable) as b:
        a.set_noise_covariance(Rn)
        _assert_images(a, m, n, res, wtable, name)
        b.set_noise_covariance(np.eye(m))
        _assert_images(b, m, n, res, wtable, name + " (identity on the whitened table)")
        # with calibration on: gamma first, then W
        rng = np.random.default_rng(m)
        gamma = (rng.uniform(0.7, 1.3, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)
        a.set_calibration(gamma)
        both = capi.whiten_table(capi.calibration_apply(table, gamma), capi.whitening_factor(Rn))
        _assert_images(a, m, n, res, both, name + " (calibration + whitening)")


# ---- 7. end to end, a general Rn -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,m,n,K,res,port", SHAPES + [FUSED], ids=[s[0] for s in SHAPES + [FUSED]])
def test_general_rn_end_to_end(name, m, n, K, res, port, gpu_device):
    capi = _capi()
    table, items = _scene(m, n, K, res, BATCH, seed=990 + m)
    Rn = _general_rn(m, 90 + m)
    W = capi.whitening_factor(Rn)
    wtable = capi.whiten_table(table, W)
    with capi.Context(m, n, m * K, res, table) as ctx:
        off_name = ctx.stage_name(capi.STAGE_COV)
        assert (off_name == "bazmusic::cov4_evd_kernel") == (name == "m4_fused_shape")
        ctx.set_noise_covariance(Rn)
        on_name = ctx.stage_name(capi.STAGE_COV)
        assert on_name == ("bazmusic::cov4_x4_kernel" if name == "m4_fused_shape" else off_name), on_name
        ang, lvl, spec = _run_device(ctx, items, port)
        path = _path(ctx)
        Rp = _device_whiten(ctx, _device_cov(ctx, items, m))                       # the device's own R'
        host = ctx.process(items, want_spectrum=port)                               # the host-fed entry point: the same bits
        ctx.set_noise_covariance(None)
        assert ctx.stage_name(capi.STAGE_COV) == off_name and ctx.get_noise_covariance() is None
    a_ref, _, _, s64, w = wr.oracle_on_R(Rp, wtable, m, n)
    worst = 0.0
    if spec is not None:
        worst = assert_spectrum_within_bound(spec, s64, path, m, n, wtable, w, what=name)[0]
    worst = max(worst, assert_doa_within_bound(ang, lvl, a_ref, s64, path, m, n, wtable, w))
    print("%s (%s path): worst err / tol against the fp64 oracle on (R', W a): %.3g" % (name, path, worst))
    for d, h in zip((ang, lvl, spec), host):
        assert (d is None and h is None) or np.array_equal(_f32bits(d), _f32bits(h)), name


# ---- 8. known answers on the device ------------------------------------------------------------------------------------------------------------

def _to_device(items):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    torch.cuda.synchronize()
    return x


def test_scene_a_on_the_device_with_a_measured_noise_covariance(gpu_device):
    capi = _capi()
    items, noise, table, K = wr.scene_a()
    m, n = wr.M, 3                                  # (a context that may report up to three: the count has room to be wrong)
    with capi.Context(m, n, m * K, wr.RES, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.process(items)
        plain = int(np.sum(ctx.last_orders(wr.ITEMS) == wr.N_EMIT))
        xn = _to_device(noise)
        Rn = ctx.mean_covariance_device(xn.data_ptr(), len(noise))
        assert np.array_equal(_bits(Rn), _bits(ctx.mean_covariance(noise)))        # the host-fed form: the same bits
        ref = wr.mean_covariance(noise, m)
        assert np.all(np.abs(Rn - ref) <= 1e-12 * np.abs(ref).max())
        ctx.set_noise_covariance(Rn)
        ctx.process(items)
        white = int(np.sum(ctx.last_orders(wr.ITEMS) == wr.N_EMIT))
    print("scene A on the device, items with the right MDL count: plain %d, whitened %d" % (plain, white))
    assert white >= 60 and plain <= 8


def test_scene_b_on_the_device(gpu_device):
    capi = _capi()
    items, ang_true, Rn, table, K = wr.scene_b()
    m, n = wr.M, wr.N_EMIT
    with capi.Context(m, n, m * K, wr.RES, table) as ctx:
        ctx.set_peak_mode(1)
        e_plain = wr.bearing_errors(ctx.process(items)[0], ang_true)
        ctx.set_noise_covariance(Rn)
        e_white = wr.bearing_errors(ctx.process(items)[0], ang_true)
    print("scene B on the device, items with both emitters within 2 bins: plain %d, whitened %d; median worst-entry error %.1f / %.1f bins"
          % ((e_plain <= 2).sum(), (e_white <= 2).sum(), np.median(e_plain), np.median(e_white)))
    assert (e_white <= 2).sum() >= 60 and (e_plain <= 2).sum() <= 32


# ---- 9. composition and scope -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,K,res", [(4, 2, 64, 360), (8, 2, 32, 360), (24, 2, 8, 360)])
def test_averaging_first_whitening_second(m, n, K, res, gpu_device):
    """With a window of 3 the stage's input is debug_average's output: R' of a call == debug_whiten(debug_average(debug_cov))."""
    import torch
    capi = _capi()
    B = 12
    table, items = _scene(m, n, K, res, B, seed=1100 + m)
    Rn = _general_rn(m, 110 + m)
    wtable = capi.whiten_table(table, capi.whitening_factor(Rn))
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_averaging(3)
        ctx.set_noise_covariance(Rn)
        R = _device_cov(ctx, items, m)
        per = m * m * 2
        rin = torch.from_numpy(np.ascontiguousarray(R).view(np.float64).reshape(B, per)).cuda()
        ravg = torch.zeros((B, per), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.reset_averaging()
        ctx.debug_average(rin.data_ptr(), B, ravg.data_ptr())
        ctx.sync()
        Rp = _device_whiten(ctx, ravg.cpu().numpy().view(np.complex128).reshape(B, m, m))
        ctx.reset_averaging()
        ang, lvl, spec = _run_device(ctx, items)
        path = _path(ctx)
        ctx.set_noise_covariance(None)                      # switching the mode does not touch the history
        assert ctx.get_averaging() == (3, 1.0)
    a_ref, _, _, s64, w = wr.oracle_on_R(Rp, wtable, m, n)
    first = 2 if K < m else 0                               # (a window still filling at K < m: rank-deficient, the bound is not defined)
    assert_spectrum_within_bound(spec[first:], s64[first:], path, m, n, wtable, w[first:])
    assert_doa_within_bound(ang[first:], lvl[first:], a_ref[first:], s64[first:], path, m, n, wtable, w[first:])


@pytest.mark.parametrize("m,n,K,res", [(4, 2, 64, 360), (8, 2, 32, 360), (24, 2, 8, 360)])
def test_averaging_and_whitening_in_the_exact_case_bit_for_bit(m, n, K, res, gpu_device):
    """Rn a diagonal of powers of four: averaging commutes with the scaling exactly, so a context with both modes on fed x equals a
    context with averaging alone on the table W a fed W x, bit for bit -- across two calls (history) and through the host-fed path."""
    capi = _capi()
    B = 12
    table, items = _scene(m, n, K, res, B, seed=1150 + m)
    Rn, w = _diag_case(m, 5 + m)
    wtable = (table * w[None, :].astype(np.float32)).astype(np.complex64)
    witems = (items.reshape(B, K, m) * w[None, None, :].astype(np.float32)).reshape(B, K * m).astype(np.complex64)
    with capi.Context(m, n, m * K, res, table) as a, capi.Context(m, n, m * K, res, wtable) as b:
        a.set_averaging(3)
        b.set_averaging(3)
        a.set_noise_covariance(Rn)
        for lo, hi in ((0, 5), (5, B)):
            _assert_outputs_equal(_run_device(a, items[lo:hi]), _run_device(b, witems[lo:hi]), "items %d..%d" % (lo, hi))
        a.reset_averaging()
        b.reset_averaging()
        _assert_outputs_equal(a.process(items), b.process(witems), "host-fed")


@pytest.mark.parametrize("m,n,res", [(4, 2, 360), (8, 2, 360), (17, 2, 100)])
def test_calibration_and_whitening_stay_in_force_across_set_table(m, n, res, gpu_device):
    capi = _capi()
    K, B = 32, 16
    table, items = _scene(m, n, K, res, B, seed=1200 + m)
    t2 = mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY * 0.9, mo.SPACING)
    rng = np.random.default_rng(m)
    gamma = (rng.uniform(0.7, 1.3, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)
    Rn = _general_rn(m, 120 + m)
    W = capi.whitening_factor(Rn)
    both2 = capi.whiten_table(capi.calibration_apply(t2, gamma), W)
    with capi.Context(m, n, m * K, res, table) as ctx, capi.Context(m, n, m * K, res, t2) as plain2:
        ctx.set_noise_covariance(Rn)
        ctx.set_calibration(gamma)
        ctx.set_table(t2)
        assert np.array_equal(ctx.get_noise_covariance(), Rn) and np.array_equal(_bits(ctx.get_calibration()), _bits(gamma))
        _assert_images(ctx, m, n, res, both2, "after set_table")
        assert ctx.process(items)[1].any()
        ctx.set_calibration(None)
        _assert_images(ctx, m, n, res, capi.whiten_table(t2, W), "after set_calibration(None)")
        ctx.set_noise_covariance(None)
        _assert_images(ctx, m, n, res, t2, "after set_noise_covariance(None)")
        _assert_outputs_equal(ctx.process(items), plain2.process(items), "both off again")


@pytest.mark.parametrize("m", [4, 8])
def test_power_mode_reads_the_whitened_pair(m, gpu_device):
    capi = _capi()
    n, K, res, B = 2, 64, 360, 23
    table, items = _scene(m, n, K, res, B, seed=1300 + m)
    Rn = _general_rn(m, 130 + m)
    wtable = capi.whiten_table(table, capi.whitening_factor(Rn))
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_noise_covariance(Rn)
        ctx.set_peak_mode(1)
        ctx.set_power_mode(1)
        ang, lvl, _ = _run_device(ctx, items)
        tap = ctx.last_powers(B * n).reshape(B, n)
        Rp = _device_whiten(ctx, _device_cov(ctx, items, m))
    present = lvl != 0
    ref = pr.powers(Rp, wtable, pr.bins_of(ang, res), present)
    tol = pr.tolerance(Rp)[:, None]
    assert present.any() and np.count_nonzero(ref) == present.sum()
    assert np.all(np.abs(tap - ref) <= tol * ref) and not tap[~present].any()


def test_refinement_and_order_mode_run_on_the_whitened_pair(gpu_device):
    """Device-resident and host-fed calls agree bit for bit with every composing mode on (chunked host path included)."""
    capi = _capi()
    m, n, K, res, B = 8, 3, 64, 360, 40
    table, items = _scene(m, 2, K, res, B, seed=1400)
    Rn = _general_rn(m, 140)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_noise_covariance(Rn)
        ctx.set_peak_mode(1)
        ctx.set_order_mode("mdl")
        ctx.set_refine_mode(1)
        ctx.set_power_mode(1)
        od = _run_device(ctx, items)
        taps_d = (ctx.last_orders(B).copy(), ctx.last_refine_offsets(B * n).copy(), ctx.last_powers(B * n).copy())
        oh = ctx.process(items)
        taps_h = (ctx.last_orders(B), ctx.last_refine_offsets(B * n), ctx.last_powers(B * n))
        _assert_outputs_equal(od, oh, "every composing mode on")
        for x, y in zip(taps_d, taps_h):
            assert np.array_equal(_bits(x), _bits(y))
        # the count is the criterion on the eigenvalues of R' (the scene's own noise is white, so this Rn colours it: no "right" count)
        Rp = _device_whiten(ctx, _device_cov(ctx, items, m))
        want, gap = oref.estimate(np.linalg.eigvalsh(wr.hermitian_from_lower(Rp)), K, n, "mdl", with_gap=True)
        clear = gap > oref.GAP_RTOL
        assert clear.mean() >= 1.0 - oref.GAP_CAP and np.array_equal(taps_d[0][clear], want[clear]), (taps_d[0], want)


def test_refusals_hold_in_both_orders_and_leave_the_context_working(gpu_device):
    capi = _capi()
    m, n, K, res, B = 4, 2, 64, 360, 8
    table = mo.steering_table_c64([[i, 0] for i in range(m)], res, mo.FREQUENCY, mo.SPACING)       # a line array: smoothing applies
    items = mo.synth_items(B, m, m * K, [[i, 0] for i in range(m)], mo.FREQUENCY, mo.SPACING, snr_db=20.0, seed=1500)
    Rn = _general_rn(m, 150)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_noise_covariance(Rn)
        want = ctx.process(items)
        for call in (lambda: ctx.set_smoothing(3, True), lambda: ctx.set_beam_mode(1), lambda: ctx.set_estimator(capi.ESTIMATOR_CAPON),
                     lambda: ctx.set_estimator(capi.ESTIMATOR_BARTLETT)):
            with pytest.raises(capi.MusicError) as e:
                call()
            assert e.value.code == capi.E_UNSUPPORTED
        assert np.array_equal(ctx.get_noise_covariance(), Rn) and ctx.get_estimator() == 0 and ctx.get_beam_mode()[0] == 0
        _assert_outputs_equal(ctx.process(items), want, "after the refused setters")
        # invalid matrices: the setting in force stays
        for bad in (np.full((m, m), np.nan), np.zeros((m, m)), np.ones((m, m))):
            with pytest.raises(capi.MusicError) as e:
                ctx.set_noise_covariance(bad)
            assert e.value.code == capi.E_INVALID
        assert np.array_equal(ctx.get_noise_covariance(), Rn)
        _assert_outputs_equal(ctx.process(items), want, "after the refused matrices")
        ctx.set_noise_covariance(None)
        plain = ctx.process(items)
        # the other order
        for arm, disarm in ((lambda: ctx.set_smoothing(3, True), lambda: ctx.set_smoothing(m, False)),
                            (lambda: ctx.set_beam_mode(1), lambda: ctx.set_beam_mode(0)),
                            (lambda: ctx.set_estimator(capi.ESTIMATOR_CAPON), lambda: ctx.set_estimator(0)),
                            (lambda: ctx.set_estimator(capi.ESTIMATOR_BARTLETT), lambda: ctx.set_estimator(0))):
            arm()
            with pytest.raises(capi.MusicError) as e:
                ctx.set_noise_covariance(Rn)
            assert e.value.code == capi.E_UNSUPPORTED and ctx.get_noise_covariance() is None
            disarm()
        _assert_outputs_equal(ctx.process(items), plain, "after the refusals in the other order")
        ctx.set_noise_covariance(Rn)
        _assert_outputs_equal(ctx.process(items), want, "on again")


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    """A context never set, one set to None and one switched on and off again: identical bits on every port, identical launch counts
    of every stage, identical table images.  While on, the covariance stage counts one launch more per call."""
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=93)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    Rn = _general_rn(m, 160 + m)
    outs, launches, images = [], [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_noise_covariance(None)
            if how == "on_then_off":
                ctx.set_noise_covariance(Rn)
                ctx.profile(1)
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                on_launches = [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]
                ctx.set_noise_covariance(None)
            assert ctx.get_noise_covariance() is None
            ctx.profile(1)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            images.append([ctx.debug_table_image(w) for w in IMAGES])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b))
    assert launches[0] == launches[1] == launches[2], launches
    for im in images[1:]:
        for x, y in zip(images[0], im):
            assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))
    fused = m == 4 and (N // m) % 256 == 0
    off = launches[0]
    # on: the covariance and the whitening stage each count once under COV where the covariance (or the fused kernel) counted alone
    assert on_launches[capi.STAGE_COV] == 2 * off[capi.STAGE_COV] > 0, (on_launches, off)
    assert on_launches[capi.STAGE_EVD] == (off[capi.STAGE_COV] if fused else off[capi.STAGE_EVD]), (on_launches, off)
    assert on_launches[capi.STAGE_SCAN] == off[capi.STAGE_SCAN], (on_launches, off)


# ---- 10. no torn batch --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,K,res", [(4, 2, 64, 360), (24, 2, 8, 360)])
def test_toggling_beside_a_submitting_thread_never_tears_a_batch(m, n, K, res, gpu_device):
    capi = _capi()
    B = 16
    table, items = _scene(m, n, K, res, B, seed=1600 + m)
    Rn, w = _diag_case(m, 7 + m)
    assert not np.all(w == 1.0)
    with capi.Context(m, n, m * K, res, table) as ctx:
        off = ctx.process(items)
        ctx.set_noise_covariance(Rn)
        on = ctx.process(items)
        ctx.set_noise_covariance(None)
        assert not np.array_equal(_f32bits(off[2]), _f32bits(on[2]))
        known = [tuple(_f32bits(x).tobytes() for x in o) for o in (off, on)]
        stop = threading.Event()
        seen, errors = [0, 0], []

        def submit():
            try:
                while not stop.is_set():
                    got = tuple(_f32bits(x).tobytes() for x in ctx.process(items))
                    if got not in known:
                        errors.append("a batch is neither the off result nor the on result")
                        return
                    seen[known.index(got)] += 1
            except Exception as e:          # noqa: BLE001 (reported by the asserting thread)
                errors.append(repr(e))

        t = threading.Thread(target=submit)
        t.start()
        try:
            for i in range(200):
                ctx.set_noise_covariance(Rn if i % 2 == 0 else None)
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        assert sum(seen) > 0
        ctx.set_noise_covariance(None)
        _assert_outputs_equal(ctx.process(items), off, "off after the toggles")


# ---- 11. the host block, through the pybind work() -----------------------------------------------------------------------------------------

def test_host_block_whiten_next(gpu_device):
    from gr_baz_amd import baz
    capi = _capi()
    items, noise, table, K = wr.scene_a()
    m, n, res = wr.M, wr.N_EMIT, wr.RES
    rows = [list(map(complex, r)) for r in table]
    with capi.Context(m, n, m * K, res, table) as ctx:
        Rn = ctx.mean_covariance(noise[:48])
        plain_out = ctx.process(items[:8])
        ctx.set_noise_covariance(Rn)
        want = ctx.process(items[:8])
    assert not np.array_equal(_f32bits(want[1]), _f32bits(plain_out[1]))
    armed = baz.music_doa(m, n, m * K, rows, res)
    assert armed.last_whitening_status() == 0 and len(armed.noise_covariance()) == 0
    armed.whiten_next(48)
    for k in (0, 1):                                            # 32 + 32 items: the capture ends inside the second call
        assert armed.last_whitening_status() == -1 and len(armed.noise_covariance()) == 0
        produced, *_ = armed.work(noise[32 * k:32 * k + 32], 3)
        assert produced == 32
    assert armed.last_whitening_status() == 0
    got = np.asarray(armed.noise_covariance(), dtype=np.complex128).reshape(m, m)
    assert np.array_equal(_bits(got), _bits(Rn))
    pa, aa, la, sa = armed.work(items[:8], 3)
    _assert_outputs_equal((aa, la, sa), want, "after the measurement was applied")
    # a capture that cannot be an Rn (all zeros) is refused: the status carries the error, the setting in force stays
    armed.whiten_next(4)
    armed.work(np.zeros((4, m * K), np.complex64), 3)
    assert armed.last_whitening_status() == capi.E_INVALID
    assert np.array_equal(_bits(np.asarray(armed.noise_covariance(), dtype=np.complex128).reshape(m, m)), _bits(Rn))
    # by hand, and off
    other = baz.music_doa(m, n, m * K, rows, res)
    other.set_noise_covariance([complex(v) for v in Rn.reshape(-1)])
    po, ao, lo, so = other.work(items[:8], 3)
    _assert_outputs_equal((ao, lo, so), want, "set_noise_covariance by hand")
    other.set_noise_covariance([])
    assert len(other.noise_covariance()) == 0
    po, ao, lo, so = other.work(items[:8], 3)
    _assert_outputs_equal((ao, lo, so), plain_out, "off again")
    with pytest.raises(ValueError):
        other.set_noise_covariance([1 + 0j] * (m * m - 1))
    with pytest.raises(ValueError):
        other.set_noise_covariance([0j] * (m * m))
    with pytest.raises(ValueError):
        other.whiten_next(0)
