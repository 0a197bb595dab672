"""Opt-in Capon and Bartlett spectrum estimators (baz_music_set_estimator) on the MI355X: every float32 word of the spectrum against
spectrum_ref on the device's own covariance (debug_cov) and the table, for every group width up to 16 antennas, with and without the
spectrum port, under both pickers; ang / lvl against the oracle's pickers on the device's own float32 row; kind 0 == the reference
with the same launches; scaling; averaging; the power and beam modes; calibration and retune; host paths == device path; degenerate
items; scope; the known-answer scene.

Spectrum criterion: one float32 ulp of float32(P_ref).  Any fp64 evaluation is good to ~8 m cond_2(R) 2^-52 relative, so while that
stays at or below 2^-26 (asserted for every item) only a rounding boundary can separate the two float32 values."""
import numpy as np
import pytest

import averaging_ref as ar
import beam_ref as br
import calib_ref as cr
import order_ref as oref
import power_ref as pr
import spectrum_ref as sref
from oracle import music_oracle as mo
from test_estimator import KNOWN_BOUND, known_answer_error, known_scene

pytestmark = pytest.mark.gpu

KINDS = [1, 2]
KIND_IDS = ["capon", "bartlett"]


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _device_cov(ctx, items, m):
    """R of every item as the context's own covariance stage computes it (debug_cov), (B, m, m) complex128."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _run_device(ctx, items, want_spectrum=True):
    """One process_device call into buffers pre-filled with NaN: (ang, lvl, spectrum | None) as numpy arrays."""
    import torch
    B = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    d_ang = torch.full((B, ctx.n), float("nan"), dtype=torch.float32, device="cuda")
    d_lvl = torch.full((B, ctx.n), float("nan"), dtype=torch.float32, device="cuda")
    d_spec = torch.full((B, ctx.res), float("nan"), dtype=torch.float32, device="cuda") if want_spectrum else None
    ctx.process_device(x.data_ptr(), B, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr() if want_spectrum else None,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ang.cpu().numpy(), d_lvl.cpu().numpy(), d_spec.cpu().numpy() if want_spectrum else None


def _assert_spectrum(spec, ref, R, what):
    """Every float32 word of `spec` within one ulp of float32(ref); zeros exactly zero; every item conditioned well enough for the
    criterion.  Returns (words that differ by one ulp, words)."""
    tol = pr.tolerance(R)
    assert np.all(tol <= 2.0 ** -26), "%s: 8 m cond 2^-52 = %.3g > 2^-26: the criterion does not apply" % (what, float(np.max(tol)))
    assert not np.isnan(spec).any(), "%s: a word of the spectrum was not written (or is NaN)" % what
    with np.errstate(over="ignore"):
        ref32 = ref.astype(np.float32)
    assert np.array_equal(spec == 0, ref32 == 0), "%s: the zeros differ" % what
    assert not _f32bits(spec)[spec == 0].any(), "%s: a zero is not +0" % what
    assert np.all(spec >= 0) and np.all(np.isfinite(spec))
    dist = sref.ulp_distance_f32(spec, ref32)
    bad = dist > 1
    if bad.any():
        b, k = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError("%s item %d bin %d: %.9g against float32(P_ref) %.9g (P_ref %.17g): %d ulp"
                             % (what, b, k, spec[b, k], ref32[b, k], ref[b, k], dist[b, k]))
    return int(np.count_nonzero(dist)), dist.size


def _picks(spec, n, res, peak):
    """The oracle's picker on every float32 row: (ang, lvl) float32 (B, n)."""
    ang = np.zeros((len(spec), n), np.float32)
    lvl = np.zeros((len(spec), n), np.float32)
    for b, row in enumerate(spec):
        if peak:
            ang[b], lvl[b] = mo.peak_pick(row, n, res)
        else:
            a, l = mo.top_n_insertion(row, n, res)
            ang[b], lvl[b] = a.astype(np.float32), l.astype(np.float32)
    return ang, lvl


def _assert_entries(ang, lvl, spec, n, res, peak, what):
    want_a, want_l = _picks(spec, n, res, peak)
    assert np.array_equal(_f32bits(ang), _f32bits(want_a)), "%s: ang differs from the picker on the device's own row" % what
    assert np.array_equal(_f32bits(lvl), _f32bits(want_l)), "%s: lvl differs from the picker on the device's own row" % what
    bins = pr.bins_of(ang, res)
    rows = np.arange(len(spec))[:, None]
    real = lvl != 0
    assert np.array_equal(_f32bits(lvl)[real], _f32bits(spec[rows, bins])[real]), "%s: lvl != spectrum[bin]" % what


def _ties(spec, n):
    """Items whose n + 1 largest float32 values hold an exact tie."""
    top = -np.sort(-spec, axis=1)[:, :n + 1]
    return int(np.count_nonzero((np.diff(top, axis=1) == 0).any(axis=1)))


# name, m, n, K, res, batch, sigma.  Line arrays.  Batches of 23 leave item groups partly empty.
SHAPES = [
    ("m2_n1", 2, 1, 32, 90, 23, 0.1),
    ("m3_n2", 3, 2, 100, 357, 23, 0.1),
    ("m4_two_kernels", 4, 2, 64, 360, 48, 0.1),
    ("m4_fused_shape", 4, 2, 256, 360, 24, 0.1),       # kind 0 takes the fused covariance + EVD kernel here
    ("m5_n3", 5, 3, 200, 720, 23, 0.1),
    ("m8_K512", 8, 2, 512, 720, 6, 0.1),
    ("m9_n2", 9, 2, 64, 200, 23, 0.1),
    ("m12_n2", 12, 2, 64, 720, 23, 0.1),
    ("m16_n15", 16, 15, 64, 360, 23, 0.1),
    ("batch_of_1", 8, 2, 64, 360, 1, 0.1),
    ("res_67", 8, 2, 64, 67, 23, 0.1),                 # one partial pass of bins, rows not 16-byte aligned
    ("m8_40dB", 8, 2, 64, 720, 23, 0.01),
]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name,m,n,K,res,batch,sigma", SHAPES, ids=[s[0] for s in SHAPES])
def test_definition_parity(name, m, n, K, res, batch, sigma, kind, gpu_device):
    capi = _capi()
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(batch, m, K, min(n, 4), sigma, seed=500 + m, arr=arr)
    with capi.Context(m, n, m * K, res, table) as ctx:
        if name == "m4_fused_shape":
            assert ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"
        R = _device_cov(ctx, items, m)
        ref = sref.spectrum(kind, R, table)
        ctx.set_estimator(kind)
        assert ctx.get_estimator() == kind
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            what = "%s kind=%d peak=%d" % (name, kind, peak)
            ang, lvl, spec = _run_device(ctx, items, True)
            off, words = _assert_spectrum(spec, ref, R, what)
            _assert_entries(ang, lvl, spec, n, res, peak, what)
            ang2, lvl2, _ = _run_device(ctx, items, False)
            assert np.array_equal(_f32bits(ang2), _f32bits(ang)), "%s: ang differs without port 2" % what
            assert np.array_equal(_f32bits(lvl2), _f32bits(lvl)), "%s: lvl differs without port 2" % what
            assert ctx.refined_values() == 0
            print("%s: %d of %d words one ulp off, %d of %d items with a tie in the top n + 1, %d real entries, largest 8 m cond 2^-52 %.3g"
                  % (what, off, words, _ties(spec, n), batch, int(np.count_nonzero(lvl)), float(np.max(pr.tolerance(R)))))
            assert np.count_nonzero(lvl) > 0
            assert _ties(spec, n) > 0                                       # (mirror-symmetric rows of a line array: the tie rule is exercised)


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    """A context never set, one set to 0 and one switched on and off again: identical bits on every port and identical launch counts
    of every stage.  With kind 1 no EVD kernel is launched."""
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=92)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs, launches = [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_estimator(0)
            if how == "on_then_off":
                ctx.set_estimator(1)
                ctx.profile(1)
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                on_launches = [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]
                ctx.set_estimator(0)
            assert ctx.get_estimator() == 0
            ctx.profile(1)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b))
    assert launches[0] == launches[1] == launches[2], launches
    assert on_launches[capi.STAGE_EVD] == 0, on_launches
    assert on_launches[capi.STAGE_SCAN] == 2 and on_launches[capi.STAGE_MERGE] == 2 and on_launches[capi.STAGE_COV] == 2, on_launches


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("m,n,K", [(4, 2, 64), (8, 2, 64), (16, 3, 64)], ids=["m4", "m8", "m16"])
def test_scaling_by_two_is_exact(m, n, K, kind, gpu_device):
    capi = _capi()
    res, B = 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=70 + m)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_estimator(kind)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            a1, l1, s1 = _run_device(ctx, items)
            a2, l2, s2 = _run_device(ctx, (2.0 * items).astype(np.complex64))
            assert np.array_equal(_f32bits(s2), _f32bits(4.0 * s1)) and np.array_equal(_f32bits(l2), _f32bits(4.0 * l1))
            assert np.array_equal(_f32bits(a2), _f32bits(a1)) and np.count_nonzero(l1) > 0


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_averaging_window_3(kind, gpu_device):
    capi = _capi()
    m, n, K, res, B = 8, 2, 64, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=333 + m)
    Rbar = ar.average(ar.covariance(items, m), 3)
    ref = sref.spectrum(kind, Rbar, table)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_averaging(3)
        ctx.set_estimator(kind)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            for port2 in (True, False):
                ctx.reset_averaging()
                ang, lvl, spec = _run_device(ctx, items, port2)
                if port2:
                    off, words = _assert_spectrum(spec, ref, Rbar, "averaging W=3 kind=%d" % kind)
                    _assert_entries(ang, lvl, spec, n, res, peak, "averaging W=3 kind=%d peak=%d" % (kind, peak))
                    first = (ang, lvl)
                else:
                    assert np.array_equal(_f32bits(ang), _f32bits(first[0])) and np.array_equal(_f32bits(lvl), _f32bits(first[1]))
    print("averaging W=3 kind=%d: %d of %d words one ulp off" % (kind, off, words))


def test_power_mode_2_and_beam_mode_under_capon(gpu_device):
    """float32(last_powers) within one ulp of spectrum[bin] (both are the Capon power of that row); mode 2 puts float32(P) on lvl;
    the MVDR weights against beam_ref at the device's own bins."""
    capi = _capi()
    m, n, K, res, B = 8, 2, 64, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=61)
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_estimator(1)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            a0, l0, s0 = _run_device(ctx, items)
            ctx.set_power_mode(2)
            ctx.set_beam_mode(1, 0.0)
            for port2 in (True, False):
                a, l, s = _run_device(ctx, items, port2)
                P = ctx.last_powers(B * n).reshape(B, n)
                W = ctx.last_beam_weights(B)
                assert np.array_equal(_f32bits(a), _f32bits(a0))
                if port2:
                    assert np.array_equal(_f32bits(s), _f32bits(s0))
                assert np.array_equal(_f32bits(l), _f32bits(P.astype(np.float32))), "mode 2: lvl is not float32(P)"
                bins = pr.bins_of(a0, res)
                at_bin = s0[np.arange(B)[:, None], bins]
                assert np.all(l0 != 0) and np.all(P > 0)
                assert np.all(sref.ulp_distance_f32(P.astype(np.float32), at_bin) <= 1)
                ref_P = pr.powers(R, table, bins, l0 != 0)
                assert np.all(np.abs(P - ref_P) <= pr.tolerance(R)[:, None] * ref_P)
                ref_W = br.item_weights(R, table, bins, l0 != 0, 0.0)
                tol = br.tolerance(R, 0.0)
                for b in range(B):
                    for e in range(n):
                        rel = np.linalg.norm(W[b, e] - ref_W[b, e]) / np.linalg.norm(ref_W[b, e])
                        assert rel <= tol[b], "item %d slot %d: relative norm error of w %.3g > tol %.3g" % (b, e, rel, tol[b])
            ctx.set_power_mode(0)
            ctx.set_beam_mode(0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_calibration_and_retune(kind, gpu_device):
    capi = _capi()
    m, n, K, res, B = 8, 2, 64, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=88)
    gamma = np.asarray(cr.random_gains(np.random.default_rng(3), m)).astype(np.complex64)
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_estimator(kind)
        ctx.set_peak_mode(1)
        a0, l0, s0 = _run_device(ctx, items)
        # a non-trivial gamma: the spectrum of the table gamma (.) a
        ctx.set_calibration(gamma)
        ang, lvl, spec = _run_device(ctx, items)
        calibrated = capi.calibration_apply(table, gamma)
        assert not np.array_equal(calibrated, table)
        _assert_spectrum(spec, sref.spectrum(kind, R, calibrated), R, "calibrated kind=%d" % kind)
        _assert_entries(ang, lvl, spec, n, res, 1, "calibrated kind=%d" % kind)
        ctx.set_calibration(None)
        # retune to the table rolled by 37 bins: the spectrum rolls bit for bit
        ctx.set_table(np.ascontiguousarray(np.roll(table, 37, axis=0)))
        a1, l1, s1 = _run_device(ctx, items)
        assert np.array_equal(_f32bits(s1), _f32bits(np.roll(s0, 37, axis=1)))
        _assert_entries(a1, l1, s1, n, res, 1, "rolled kind=%d" % kind)
        assert np.array_equal(_f32bits(np.sort(l1, axis=1)), _f32bits(np.sort(l0, axis=1)))


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("cfg,batch", [("cfg1", 1000), ("cfg2", 300)])
def test_host_paths_equal_the_device_path(cfg, batch, kind, gpu_device, monkeypatch):
    """One device call, a host-fed call from pageable memory, one from page-locked memory (no copies) and one cut into chunks:
    identical ang / lvl / spectrum bits, with and without the spectrum port."""
    import torch
    capi = _capi()
    c = mo.make_config(cfg, batch, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    items = c["items"]
    outs = []
    for how in ("device", "pageable", "page_locked", "chunked"):
        if how == "chunked":
            monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            ctx.set_peak_mode(1)
            ctx.set_estimator(kind)
            if how == "device":
                out = _run_device(ctx, items) + _run_device(ctx, items, False)[:2]
            elif how == "page_locked":
                pinned = torch.from_numpy(items.view(np.float32)).pin_memory().numpy().view(np.complex64)
                o = tuple(torch.zeros((batch, k), dtype=torch.float32).pin_memory().numpy() for k in (n, n, res))
                ctx.process(pinned, out=o)
                o2 = tuple(torch.zeros((batch, k), dtype=torch.float32).pin_memory().numpy() for k in (n, n))
                ctx.process(pinned, out=o2 + (None,))
                out = tuple(np.array(v) for v in o + o2)
            else:
                out = ctx.process(items) + ctx.process(items, want_spectrum=False)[:2]
            outs.append(out)
    assert np.count_nonzero(outs[0][1]) > batch
    for how, o in zip(("pageable", "page_locked", "chunked"), outs[1:]):
        for name, a, b in zip(("ang", "lvl", "spectrum", "ang without port 2", "lvl without port 2"), outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b)), "%s: %s differs from the device path" % (how, name)


@pytest.mark.parametrize("m,n", [(4, 2), (8, 2), (16, 3)], ids=["m4", "m8", "m16"])
def test_degenerate_items_inside_a_wave(m, n, gpu_device):
    """All-zero items and items with fewer snapshots than antennas (every snapshot from the m-th on is zero: a singular R) between
    healthy ones: their Capon rows are all zero and their entries (0, 0); every other item is bit-identical to a run of healthy
    items only; Bartlett of an all-zero item is zeros, of a singular R the definition's value."""
    capi = _capi()
    res, B, K = 360, 23, 64
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    zero_at, short_at = [3, 17], [5, 6, 22]
    items, _ = oref.scene(B, m, K, n, 0.1, seed=40 + m)
    holed = items.copy()
    holed[zero_at] = 0
    holed[short_at, (m - 1) * m:] = 0                                        # m - 1 snapshots
    good = np.ones(B, bool)
    good[zero_at + short_at] = False
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, holed, m)
        for kind in KINDS:
            ctx.set_estimator(kind)
            for peak in (0, 1):
                ctx.set_peak_mode(peak)
                what = "degenerate m=%d kind=%d peak=%d" % (m, kind, peak)
                base = _run_device(ctx, items)
                got = _run_device(ctx, holed)
                nolvl = _run_device(ctx, holed, False)
                for a, b in zip(base, got):
                    assert np.array_equal(_f32bits(a[good]), _f32bits(b[good])), "%s: a healthy item changed" % what
                assert np.all(base[2] > 0) and np.all(base[1] > 0)
                dead = zero_at + short_at if kind == 1 else zero_at
                for v in got:
                    assert not _f32bits(v[dead]).any(), "%s: a degenerate item has a non-zero word" % what
                assert np.array_equal(_f32bits(nolvl[0]), _f32bits(got[0])) and np.array_equal(_f32bits(nolvl[1]), _f32bits(got[1]))
                _assert_entries(got[0], got[1], got[2], n, res, peak, what)
                if kind == 2:
                    ref32 = sref.spectrum(2, R[short_at], table).astype(np.float32)
                    assert np.all(got[2][short_at] > 0) and np.all(sref.ulp_distance_f32(got[2][short_at], ref32) <= 1), what


def test_scope(gpu_device):
    capi = _capi()
    L = capi.lib()
    m = 17
    table = mo.steering_table_c64(oref.ula(m), 360, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, 2, m * 32, 360, table) as ctx:
        for kind in KINDS:
            with pytest.raises(capi.MusicError) as e:
                ctx.set_estimator(kind)
            assert e.value.code == capi.E_UNSUPPORTED and ctx.get_estimator() == 0
        ctx.set_estimator(0)
        assert L.baz_music_set_estimator(ctx._h, 3) == capi.E_INVALID
    m, n, K, res = 8, 2, 64, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, n, m * K, res, table) as ctx:
        for keep in (0, 1, 2):
            ctx.set_estimator(keep)
            for bad in (3, -1):
                assert L.baz_music_set_estimator(ctx._h, bad) == capi.E_INVALID
                assert ctx.get_estimator() == keep                          # the previous kind stays in force
        ctx.set_estimator(0)
        # refused in both orders, both settings intact
        setters = [("order", lambda: ctx.set_order_mode("mdl"), lambda: ctx.set_order_mode(None), lambda: ctx.get_order_mode() is not None),
                   ("refine", lambda: ctx.set_refine_mode(1), lambda: ctx.set_refine_mode(0), lambda: ctx.get_refine_mode() != 0),
                   ("smoothing", lambda: ctx.set_smoothing(6, True), lambda: ctx.set_smoothing(m, False),
                    lambda: ctx.get_smoothing() != (m, False))]
        for name, on, off, is_on in setters:
            for kind in KINDS:
                on()                                                        # the other mode first: the estimator is refused
                assert is_on()
                with pytest.raises(capi.MusicError) as e:
                    ctx.set_estimator(kind)
                assert e.value.code == capi.E_UNSUPPORTED, name
                assert ctx.get_estimator() == 0 and is_on()
                ctx.set_estimator(0)                                        # always accepted
                off()
                assert not is_on()
                ctx.set_estimator(kind)                                     # the estimator first: the other mode is refused
                with pytest.raises(capi.MusicError) as e:
                    on()
                assert e.value.code == capi.E_UNSUPPORTED, name
                assert ctx.get_estimator() == kind and not is_on()
                ctx.set_estimator(0)
        # a refused setter leaves a context that still works
        ctx.set_estimator(1)
        items, _ = oref.scene(5, m, K, n, 0.1, seed=1)
        assert np.all(ctx.process(items)[1] > 0)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_known_answer_on_the_device(kind, gpu_device):
    capi = _capi()
    items, table, m, K, res, true_bins = known_scene()
    with capi.Context(m, 2, m * K, res, table) as ctx:
        ctx.set_estimator(kind)
        ctx.set_peak_mode(1)
        ang, lvl, spec = _run_device(ctx, items)
    worst = known_answer_error(spec, res, true_bins)
    print("kind %d on the device: strongest two local maxima within %d bins of the emitters (bound %d)" % (kind, worst, KNOWN_BOUND[kind]))
    assert worst <= KNOWN_BOUND[kind]
    # the device's own entries are those maxima
    bins = pr.bins_of(ang, res)
    for t in true_bins:
        dist = np.abs(bins - t)
        assert np.all(np.min(np.minimum(dist, res - dist), axis=1) <= KNOWN_BOUND[kind]) and np.all(lvl > 0)
