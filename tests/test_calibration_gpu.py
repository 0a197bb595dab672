"""Opt-in per-antenna gain / phase calibration (baz_music_set_calibration, baz_music_calibrate) on the MI355X.

The main pin is an equivalence: a context on a table T with set_calibration(gamma) and a context created on
calibration_apply(T, gamma) -- the host form of the table kernel's own routine -- agree bit for bit in every port, every side output
and every table image, on every scan path; for the table gamma (.) T the reference itself is then the oracle, through the existing
parity tests.  Further: persistence across set_table, off == the context that was never set, changes of gamma with batches in flight,
the estimator's R-bar against the exactly rounded mean (math.fsum) of the device's own covariances, within B 2^-53 mean_t |x_t| per
real component (the first-order bound of any summation order plus the final scaling), its repeatability and side effects, the host
block's calibrate_next and the helper."""
import math
import threading

import numpy as np
import pytest

import calib_ref as cr
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


def _gamma(seed, m):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.7, 1.3, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)


def _shape(m, n, res, K, B, seed=11):
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(B, m, m * K, arr, mo.FREQUENCY, mo.SPACING, snr_db=20.0, seed=seed)
    return table, items


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


# ---- 5. equivalence, on every scan path ----------------------------------------------------------------------------------------------
# name, m, n, res, spectrum port, K
PATHS = [
    ("m4_fp64_projector", 4, 2, 360, True, 64),
    ("m4_coarse_gate", 4, 2, 360, False, 64),
    ("m4_fused_frontend", 4, 2, 360, True, 256),
    ("m3_res357", 3, 2, 357, True, 32),
    ("m8_int8", 8, 2, 360, True, 32),
    ("m12_short_form", 12, 2, 360, True, 32),
    ("m17_wide", 17, 2, 100, True, 32),
    ("m32_wide_n3", 32, 3, 360, True, 32),
]


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_calibrated_context_equals_a_context_on_the_applied_table(gpu_device, path):
    capi = _capi()
    name, m, n, res, with_spec, K = path
    B = 24
    table, items = _shape(m, n, res, K, B)
    gamma = _gamma(500 + m, m)
    applied = capi.calibration_apply(table, gamma)
    assert np.array_equal(_bits(applied), _bits(cr.apply(table, gamma)))
    with capi.Context(m, n, m * K, res, table) as a, capi.Context(m, n, m * K, res, applied) as b:
        a.set_calibration(gamma)
        assert np.array_equal(_bits(a.get_calibration()), _bits(gamma)) and b.get_calibration() is None
        oa = a.process(items, want_spectrum=with_spec)
        ob = b.process(items, want_spectrum=with_spec)
        _assert_outputs_equal(oa, ob, name)
        assert oa[1].any()
        _assert_images(a, m, n, res, applied, name)
        _assert_images(b, m, n, res, applied, name + " (created on the applied table)")
        # the calibration changes something: the uncalibrated context reports another spectrum / other levels
        with capi.Context(m, n, m * K, res, table) as plain:
            op = plain.process(items, want_spectrum=with_spec)
            assert not np.array_equal(_f32bits(op[1]), _f32bits(oa[1]))


@pytest.mark.parametrize("m", [4, 8])
def test_equivalence_with_refinement_power_and_beam_on(gpu_device, m):
    capi = _capi()
    n, res, K, B = 2, 360, 64, 24
    table, items = _shape(m, n, res, K, B, seed=12)
    gamma = _gamma(600 + m, m)
    applied = capi.calibration_apply(table, gamma)
    taps = []
    for ctx_table, g in ((table, gamma), (applied, None)):
        with capi.Context(m, n, m * K, res, ctx_table) as ctx:
            ctx.set_peak_mode(1)
            ctx.set_refine_mode(1)
            ctx.set_power_mode(1)
            ctx.set_beam_mode(1)
            if g is not None:
                ctx.set_calibration(g)
            out = ctx.process(items)
            taps.append((out, ctx.last_refine_offsets(B * n), ctx.last_powers(B * n), ctx.last_beam_weights(B), ctx.last_beams(B)))
    _assert_outputs_equal(taps[0][0], taps[1][0], "m=%d" % m)
    for k, name in ((1, "last_refine_offsets"), (2, "last_powers"), (3, "last_beam_weights"), (4, "last_beams")):
        assert taps[0][k].shape == taps[1][k].shape and taps[0][k].any(), name
        assert np.array_equal(_bits(taps[0][k]), _bits(taps[1][k])), "m=%d: %s differs" % (m, name)


# ---- 6. persistence ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,res", [(4, 2, 360), (8, 2, 360), (17, 2, 100)])
def test_calibration_stays_in_force_across_set_table(gpu_device, m, n, res):
    capi = _capi()
    K, B = 32, 16
    table, items = _shape(m, n, res, K, B, seed=13)
    t2 = mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY * 0.9, mo.SPACING)
    gamma = _gamma(700 + m, m)
    applied2 = capi.calibration_apply(t2, gamma)
    with capi.Context(m, n, m * K, res, table) as ctx, capi.Context(m, n, m * K, res, applied2) as want, \
            capi.Context(m, n, m * K, res, t2) as plain2:
        ctx.set_calibration(gamma)
        ctx.set_table(t2)
        assert np.array_equal(_bits(ctx.get_calibration()), _bits(gamma))
        _assert_outputs_equal(ctx.process(items), want.process(items), "after set_table")
        _assert_images(ctx, m, n, res, applied2, "after set_table")
        ctx.set_calibration(None)
        assert ctx.get_calibration() is None
        _assert_outputs_equal(ctx.process(items), plain2.process(items), "after set_calibration(None)")
        _assert_images(ctx, m, n, res, t2, "after set_calibration(None)")


# ---- 7. off is the context that was never set ------------------------------------------------------------------------------------------

def _counts(ctx):
    capi = _capi()
    return [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]


@pytest.mark.parametrize("m,n,res,with_spec", [(4, 2, 360, True), (4, 2, 360, False), (8, 2, 360, True), (17, 2, 100, True)])
def test_off_is_the_context_never_set(gpu_device, m, n, res, with_spec):
    capi = _capi()
    K, B = 32, 16
    table, items = _shape(m, n, res, K, B, seed=14)
    gamma = _gamma(800 + m, m)
    results = []
    for how in ("never set", "set to None", "on and off again"):
        with capi.Context(m, n, m * K, res, table) as ctx:
            if how == "set to None":
                ctx.set_calibration(None)
            if how == "on and off again":
                ctx.set_calibration(gamma)
                ctx.set_calibration(None)
            assert ctx.get_calibration() is None
            ctx.profile(1)
            out = ctx.process(items, want_spectrum=with_spec)
            ctx.sync()
            counts = _counts(ctx)
            _assert_images(ctx, m, n, res, table, how)
            results.append((out, counts, [ctx.debug_table_image(w) for w in IMAGES]))
    for how, (out, counts, images) in zip(("set to None", "on and off again"), results[1:]):
        _assert_outputs_equal(results[0][0], out, how)
        assert counts == results[0][1] and sum(counts) > 0, (how, counts, results[0][1])
        for w, (x, y) in enumerate(zip(results[0][2], images)):
            assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (how, w)


def test_explicit_unit_gains_run_the_kernel_and_give_the_same_bytes(gpu_device):
    capi = _capi()
    m, n, res, K, B = 8, 2, 360, 32, 16
    table, items = _shape(m, n, res, K, B, seed=15)
    with capi.Context(m, n, m * K, res, table) as ctx:
        want = ctx.process(items)
        ctx.set_calibration(np.ones(m, np.complex64))
        assert ctx.get_calibration() is not None
        _assert_outputs_equal(ctx.process(items), want, "gamma = 1")
        _assert_images(ctx, m, n, res, table, "gamma = 1")


def test_invalid_gains_are_refused_and_the_setting_stays(gpu_device):
    capi = _capi()
    m, n, res, K, B = 4, 2, 360, 32, 8
    table, items = _shape(m, n, res, K, B, seed=16)
    gamma = _gamma(900, m)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_calibration(gamma)
        want = ctx.process(items)
        for bad in (0.0, np.nan, np.inf, complex(1.0, -np.inf)):
            g = gamma.copy()
            g[2] = bad
            with pytest.raises(capi.MusicError) as e:
                ctx.set_calibration(g)
            assert e.value.code == capi.E_INVALID
            assert np.array_equal(_bits(ctx.get_calibration()), _bits(gamma))
        _assert_outputs_equal(ctx.process(items), want, "after refused gains")
        t0 = ctx.last_retune_ms()[0]
        assert t0 > 0.0                                    # set_calibration is a retune: it reports its wall time like set_table


# ---- 8. changes of gamma with batches in flight ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,res,with_spec", [(4, 2, 360, True), (8, 2, 360, False), (17, 2, 100, True)])
def test_calibration_changes_with_batches_in_flight_never_tear(gpu_device, m, n, res, with_spec):
    """One thread submits device batches, four at a time without waiting; another alternates set_calibration between two gammas, a
    fixed 50 changes.  Every batch equals, bit for bit, the outputs of one gamma or of the other."""
    import torch
    capi = _capi()
    K, B, CHANGES, DEPTH = 32, 64, 50, 4
    table, items = _shape(m, n, res, K, B, seed=17)
    gammas = [_gamma(1000 + m, m), _gamma(2000 + m, m)]
    want = []
    for g in gammas:
        with capi.Context(m, n, m * K, res, capi.calibration_apply(table, g)) as ref:
            want.append(ref.process(items, want_spectrum=with_spec))
    assert not np.array_equal(_f32bits(want[0][1]), _f32bits(want[1][1]))
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).to(gpu_device)
    outs = [(torch.zeros(B, n, dtype=torch.float32, device=gpu_device), torch.zeros(B, n, dtype=torch.float32, device=gpu_device),
             torch.zeros(B, res, dtype=torch.float32, device=gpu_device) if with_spec else None) for _ in range(DEPTH)]
    torch.cuda.synchronize()
    failed = []
    seen = [0, 0]
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_calibration(gammas[0])
        ctx.reserve(B)
        done = threading.Event()

        def setter():
            try:
                for k in range(CHANGES):
                    ctx.set_calibration(gammas[(k + 1) % 2])
            except Exception as e:                        # noqa: BLE001 -- reported by the main thread
                failed.append(repr(e))
            finally:
                done.set()

        th = threading.Thread(target=setter)
        th.start()
        rounds = 0
        while True:
            last = done.is_set()                          # one more round after the last change
            for a, l, s in outs:
                ctx.process_device(x.data_ptr(), B, a.data_ptr(), l.data_ptr(), s.data_ptr() if with_spec else None)
            ctx.sync()
            for a, l, s in outs:
                got = (a.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy() if with_spec else None)
                which = [all(y is None or np.array_equal(_f32bits(y), _f32bits(w)) for y, w in zip(got, want[k])) for k in (0, 1)]
                if not any(which):
                    failed.append("round %d: a batch equals the outputs of neither gamma" % rounds)
                else:
                    seen[which.index(True)] += 1
            rounds += 1
            if last or failed or rounds >= 10000:
                break
        th.join()
    assert not failed, failed[:3]
    assert sum(seen) == rounds * DEPTH and rounds >= 1
    # (CHANGES is even: the last gamma in force is gammas[0])
    print("m=%d: %d rounds of %d batches; %d / %d batches on gamma A / B" % (m, rounds, DEPTH, seen[0], seen[1]))


# ---- 9. the estimator on the device ------------------------------------------------------------------------------------------------------

def _device_cov(ctx, x, B, m):
    import torch
    R = torch.zeros(B * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), B, R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().reshape(B, 2 * m * m)


def _pilot_items(m, K, B, seed):
    rng = np.random.default_rng(seed)
    p = np.exp(2j * np.pi * rng.uniform(0, 1, m)).astype(np.complex64)
    gamma = cr.random_gains(rng, m)
    return cr.scene(rng, p[None, :], gamma, [0], B, K, 0.1), p, gamma


_worst_mean = [0.0]
# m, K.  (4, 256): the fused covariance + EVD shape -- calibrate runs the two-kernel form there.  (64, 32) with B = 300: two chunks.
EST_SHAPES = [(2, 32), (4, 32), (4, 256), (5, 32), (8, 32), (16, 32), (17, 32), (32, 32)]
EST_CASES = [(m, K, B) for m, K in EST_SHAPES for B in (1, 8, 61)] + [(64, 32, 300)]


@pytest.mark.parametrize("m,K,B", EST_CASES, ids=["m%d_K%d_B%d" % c for c in EST_CASES])
def test_estimator_mean_covariance_repeatability_and_estimate(gpu_device, m, K, B):
    import torch
    capi = _capi()
    n, res = 1, 90
    items, p, gamma = _pilot_items(m, K, B, 3000 + 64 * m + B)
    table = mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY, mo.SPACING)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).to(gpu_device)
    torch.cuda.synchronize()
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, x, B, m)
        g1, q1, rbar1 = ctx.calibrate_device(x.data_ptr(), B, p, want_rbar=True)
        g2, q2, rbar2 = ctx.calibrate_device(x.data_ptr(), B, p, want_rbar=True)
        g3, q3, rbar3 = ctx.calibrate(items, p, want_rbar=True)
        g4, q4 = ctx.calibrate(items, p)
    # R-bar against the exactly rounded mean of the device's own covariances
    got = rbar1.view(np.float64).reshape(-1)
    exact = np.array([math.fsum(R[:, e]) / B for e in range(2 * m * m)])      # (the division rounds once more: below the bound)
    bound = B * 2.0 ** -53 * np.mean(np.abs(R), axis=0)
    err = np.abs(got - exact)
    assert np.all(err <= bound), "m=%d B=%d: |R-bar - mean| %.3g > %.3g" % (m, B, err.max(), bound[np.argmax(err - bound)])
    nz = bound > 0
    frac = float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0
    _worst_mean[0] = max(_worst_mean[0], frac)
    print("m=%d K=%d B=%d: largest |R-bar - exact mean| / bound %.3g (so far %.3g); quality %.6f" % (m, K, B, frac, _worst_mean[0], q1))
    # repeatability, and host-fed == device form
    assert np.array_equal(_bits(rbar1), _bits(rbar2)) and np.array_equal(_bits(rbar1), _bits(rbar3))
    for g, q in ((g2, q2), (g3, q3), (g4, q4)):
        assert np.array_equal(_bits(g), _bits(g1)) and q == q1
    # gamma-hat and quality are calibration_estimate on that R-bar: the same routine
    ge, qe = capi.calibration_estimate(rbar1, p)
    assert np.array_equal(_bits(ge), _bits(g1)) and qe == q1
    # ... and they find the gains (sigma 0.1: quality near 1 from a handful of items on)
    if B * K >= 256:
        assert q1 >= 0.9 and np.max(np.abs(g1 - gamma)) <= 0.1, (q1, np.max(np.abs(g1 - gamma)))


@pytest.mark.parametrize("m", [4, 8, 17])
def test_calibrate_has_no_side_effects(gpu_device, m):
    """Averaging W = 3 on: a process call after calibrate gives the bits it gives without it; the taps of the last call stay."""
    capi = _capi()
    n, res, K, B = 2, 100 if m > 16 else 360, 32, 16
    table, items = _shape(m, n, res, K, 2 * B, seed=18)
    pilot, p, _ = _pilot_items(m, K, 8, 4000 + m)
    first, second = items[:B], items[B:]
    runs = []
    for with_calibrate in (False, True):
        with capi.Context(m, n, m * K, res, table) as ctx:
            ctx.set_averaging(3)
            if m <= 16:
                ctx.set_power_mode(1)
            o1 = ctx.process(first)
            taps = ctx.last_powers(B * n) if m <= 16 else None
            if with_calibrate:
                g, q = ctx.calibrate(pilot, p)
                assert q > 0.9
                assert ctx.get_calibration() is None                   # the estimate is not applied
                if taps is not None:
                    assert np.array_equal(_bits(ctx.last_powers(B * n)), _bits(taps)) and taps.any()
                _assert_images(ctx, m, n, res, table, "after calibrate")
            o2 = ctx.process(second)
            runs.append((o1, o2))
    _assert_outputs_equal(runs[0][0], runs[1][0], "first call")
    _assert_outputs_equal(runs[0][1], runs[1][1], "the call after calibrate")


def test_smoothing_and_calibration_refuse_each_other(gpu_device):
    import torch
    capi = _capi()
    m, n, res, K, B = 4, 2, 360, 32, 8
    table, items = _shape(m, n, res, K, B, seed=19)
    gamma = _gamma(1100, m)
    p = np.ones(m, np.complex64)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).to(gpu_device)
    torch.cuda.synchronize()

    def refused(call, *args):
        with pytest.raises(capi.MusicError) as e:
            call(*args)
        assert e.value.code == capi.E_UNSUPPORTED

    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_smoothing(m, True)                         # forward-backward averaging on the centro-symmetric square
        assert ctx.get_smoothing() == (m, 1)
        want = ctx.process(items)
        refused(ctx.set_calibration, gamma)
        refused(ctx.calibrate, items, p)
        refused(ctx.calibrate_device, x.data_ptr(), B, p)
        assert ctx.get_calibration() is None and ctx.get_smoothing() == (m, 1)
        ctx.set_calibration(None)                          # off while off: allowed
        _assert_outputs_equal(ctx.process(items), want, "smoothing stays as it was")
        ctx.set_smoothing(m, False)
        ctx.set_calibration(gamma)
        want = ctx.process(items)
        refused(ctx.set_smoothing, m, True)
        assert ctx.get_smoothing() == (m, 0) and np.array_equal(_bits(ctx.get_calibration()), _bits(gamma))
        _assert_outputs_equal(ctx.process(items), want, "the calibration stays as it was")
        # argument errors of calibrate
        for bad in (0.0, np.nan):
            q = p.copy()
            q[1] = bad
            with pytest.raises(capi.MusicError) as e:
                ctx.calibrate(items, q)
            assert e.value.code == capi.E_INVALID
        with pytest.raises(capi.MusicError) as e:
            ctx.calibrate(items[:0].reshape(0, m * K), p)
        assert e.value.code == capi.E_INVALID


# ---- 10. the host block, through the pybind work() -----------------------------------------------------------------------------------

def test_host_block_calibrate_next(gpu_device):
    from gr_baz_amd import baz
    capi = _capi()
    m, n, res, K = 8, 2, 360, 32
    table = mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY, mo.SPACING)
    rng = np.random.default_rng(77)
    gamma = cr.random_gains(rng, m)
    pilot_bin = 200
    items = cr.scene(rng, table, gamma, [pilot_bin], 16, K, 0.1)
    probe = cr.scene(rng, table, gamma, [40, 122], 8, K, 0.1)
    ref = [complex(v) for v in table[pilot_bin]]
    rows = [list(map(complex, r)) for r in table]
    with capi.Context(m, n, m * K, res, table) as ctx:
        g12, q12 = ctx.calibrate(items[:12], table[pilot_bin])
    g12 = g12.astype(np.complex64)
    armed, plain = baz.music_doa(m, n, m * K, rows, res), baz.music_doa(m, n, m * K, rows, res)
    assert armed.last_calibration_quality() == -1.0 and len(armed.calibration()) == 0
    armed.calibrate_next(12, ref, 0.9)
    assert armed.last_calibration_quality() == -1.0
    for k in (0, 1):
        chunk = items[8 * k:8 * k + 8]
        pa, aa, la, sa = armed.work(chunk, 3)
        pp, ap, lp, sp = plain.work(chunk, 3)
        assert pa == pp == 8
        _assert_outputs_equal((aa, la, sa), (ap, lp, sp), "work() call %d while capturing" % k)
        if k == 0:
            assert armed.last_calibration_quality() == -1.0 and len(armed.calibration()) == 0
    assert armed.last_calibration_quality() == q12 and q12 >= 0.9
    applied = np.asarray(armed.calibration(), dtype=np.complex64)
    assert np.array_equal(_bits(applied), _bits(g12))
    # ... and it is in force: the block now equals a context on the applied table
    with capi.Context(m, n, m * K, res, capi.calibration_apply(table, g12)) as ctx:
        want = ctx.process(probe)
    pa, aa, la, sa = armed.work(probe, 3)
    _assert_outputs_equal((aa, la, sa), want, "after the estimate was applied")
    # a min_quality above the measured quality leaves the calibration unchanged
    armed.calibrate_next(4, ref, 1.0)
    armed.work(items[:4], 3)
    assert armed.last_calibration_quality() < 1.0 and armed.last_calibration_quality() > 0.9
    assert np.array_equal(_bits(np.asarray(armed.calibration(), dtype=np.complex64)), _bits(g12))
    plain.calibrate_next(4, ref, 1.0)
    plain.work(items[:4], 3)
    assert len(plain.calibration()) == 0
    # set_calibration / off by hand
    plain.set_calibration([complex(v) for v in g12])
    pp, ap, lp, sp = plain.work(probe, 3)
    _assert_outputs_equal((ap, lp, sp), want, "set_calibration by hand")
    plain.set_calibration([])
    assert len(plain.calibration()) == 0
    with pytest.raises(ValueError):
        plain.set_calibration([1 + 0j] * (m - 1))
    with pytest.raises(ValueError):
        plain.set_calibration([0j] * m)
    with pytest.raises(ValueError):
        plain.calibrate_next(0, ref, 0.9)
    with pytest.raises(ValueError):
        plain.calibrate_next(4, ref, 1.5)


# ---- 11. the helper ------------------------------------------------------------------------------------------------------------------

def test_helper_calibration_survives_set_frequency(gpu_device):
    from gr_baz_amd import baz
    capi = _capi()
    h = baz.music_doa_helper
    m, n, res, K = 4, 2, 360, 64
    arr = mo.array_geometry(m)
    hb = h.music_doa_helper(m=m, n=n, nsamples=m * K, angular_resolution=res, frequency=mo.FREQUENCY, array_spacing=mo.SPACING,
                            antenna_array=arr, output_spectrum=True)
    gamma = _gamma(1200, m)
    items = mo.synth_items(12, m, m * K, arr, mo.FREQUENCY, mo.SPACING, seed=6)
    assert hb.calibration() is None
    hb.set_calibration(gamma)
    assert np.array_equal(_bits(hb.calibration()), _bits(gamma))
    for f in (mo.FREQUENCY, 0.75 * mo.FREQUENCY):
        if f != mo.FREQUENCY:
            hb.set_frequency(f)
            assert np.array_equal(_bits(hb.calibration()), _bits(gamma))
        t = mo.steering_table_c64(arr, res, f, mo.SPACING)
        assert np.array_equal(np.asarray(hb.array_response, dtype=np.complex64), t)        # the helper's table stays uncalibrated
        with capi.Context(m, n, m * K, res, capi.calibration_apply(t, gamma)) as ctx:
            want = ctx.process(items)
        _assert_outputs_equal(hb.work(items), want, "helper at %.3g Hz" % f)
    # calibrate_next by pilot bin and by an explicit reference
    rng = np.random.default_rng(78)
    true = cr.random_gains(rng, m)
    table = mo.steering_table_c64(arr, res, 0.75 * mo.FREQUENCY, mo.SPACING)
    pilot = cr.scene(rng, table, true, [200], 8, K, 0.1)
    hb.set_calibration(None)
    hb.calibrate_next(8, pilot_bin=200)
    assert hb.last_calibration_quality() == -1.0
    hb.work(pilot)
    assert hb.last_calibration_quality() >= 0.9
    assert np.max(np.abs(hb.calibration() - true)) <= 0.05
    with capi.Context(m, n, m * K, res, table) as ctx:
        g, q = ctx.calibrate(pilot, table[200])
    assert np.array_equal(_bits(hb.calibration()), _bits(g.astype(np.complex64))) and q == hb.last_calibration_quality()
    with pytest.raises(ValueError):
        hb.calibrate_next(8)
    with pytest.raises(ValueError):
        hb.calibrate_next(8, pilot_bin=3, ref=[1] * m)
    hb.calibrate_next(8, ref=[1] * m, min_quality=0.5)
    assert hb.last_calibration_quality() == -1.0
