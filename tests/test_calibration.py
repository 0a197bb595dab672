"""Opt-in per-antenna gain / phase calibration (baz_music_set_calibration, baz_music_calibrate): what needs no device.  calib_ref.py
restates the two definitions of include/baz_music_hip.h in numpy; baz_music_calibration_apply is the table kernel's own routine on
the host (bit for bit against the restatement), baz_music_calibration_estimate the host Jacobi that calibrate() calls on its R-bar
(against numpy.linalg.eigh: the sine of the angle between the two gain vectors within 8 m 2^-52 |R-bar|_2 / (l1 - l2), Davis-Kahan
against a backward error of m 2^-52 |R-bar|_2 with a factor 8 of headroom; the quality within 8 m 2^-52 relative)."""
import ctypes

import numpy as np
import pytest

import calib_ref as cr
from gr_baz_amd import capi
from oracle import music_oracle as mo

F32_MAX = np.finfo(np.float32).max
F32_TINY = np.finfo(np.float32).tiny


def _bits64(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.uint32)


def _gains(rng, m):
    return (rng.uniform(0.5, 2.0, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)


def _table(rng, res, m, extremes=True):
    t = (rng.standard_normal((res, m)) + 1j * rng.standard_normal((res, m))).astype(np.complex64)
    if extremes:          # fp32 extremes: the largest and smallest normal numbers, subnormals, exact zeros, huge against tiny
        flat = t.reshape(-1)
        vals = [F32_MAX, -F32_MAX, F32_TINY, -F32_TINY, F32_TINY / 8, np.float32(1e-45), 0.0, 1.0, np.float32(2.0 ** 100), np.float32(2.0 ** -100)]
        for k in range(min(flat.size, 4 * len(vals))):
            re = vals[k % len(vals)]
            im = vals[(k * 7 + 3) % len(vals)]
            flat[(k * 13) % flat.size] = np.complex64(complex(re, im))
    return t


# ---- 1. applying -------------------------------------------------------------------------------------------------------------------

APPLY_M = list(range(1, 17)) + [17, 64]


@pytest.mark.parametrize("m", APPLY_M)
def test_apply_equals_the_restatement_bit_for_bit(m):
    rng = np.random.default_rng(8100 + m)
    res = 37 if m < 64 else 11
    t = _table(rng, res, m)
    for trial in range(2):
        g = _gains(rng, m)
        if trial:            # gains at extremes too
            g[0] = np.complex64(complex(F32_TINY, 0.0))
            g[m - 1] = np.complex64(complex(0.0, -3.0e38))
        got = capi.calibration_apply(t, g)
        want = cr.apply(t, g)
        same = (_bits64(got) == _bits64(want)) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))
        assert same.all(), "m=%d: %d words differ" % (m, int((~same).sum()))


@pytest.mark.parametrize("m", APPLY_M)
def test_apply_with_unit_gains_returns_the_input_bits(m):
    rng = np.random.default_rng(8200 + m)
    t = _table(rng, 29, m)
    t = np.where(np.isfinite(t), t, 1).astype(np.complex64)
    # (a component -0 may come back as +0: -0 - (-0) = +0; no other bit ever changes)
    assert not np.signbit(t.view(np.float32)[t.view(np.float32) == 0]).any()
    got = capi.calibration_apply(t, np.ones(m, np.complex64))
    assert np.array_equal(_bits64(got), _bits64(t))
    assert np.array_equal(_bits64(cr.apply(t, np.ones(m, np.complex64))), _bits64(t))


def test_apply_by_hand():
    t = np.array([[1 + 2j, 3 - 1j], [0.5j, -2.0]], np.complex64)
    g = np.array([2j, 0.5], np.complex64)
    want = np.array([[-4 + 2j, 1.5 - 0.5j], [-1.0, -1.0]], np.complex64)
    assert np.array_equal(capi.calibration_apply(t, g), want)
    assert np.array_equal(cr.apply(t, g), want)


# ---- 2. estimating -----------------------------------------------------------------------------------------------------------------

EST_M = list(range(2, 17)) + [32, 64]
EST_SNR_DB = (0.0, 10.0, 20.0, 40.0)
_worst = {"vector": 0.0, "quality": 0.0}


def _pilot_rbar(rng, m, snr_db, B=8, K=64):
    """(R-bar of B items of a pilot seen through random gains in white noise, the pilot's unit-modulus ideal response, the gains)."""
    p = np.exp(2j * np.pi * rng.uniform(0, 1, m)).astype(np.complex64)
    gamma = cr.random_gains(rng, m)
    sigma = 10.0 ** (-snr_db / 20.0)
    items = cr.scene(rng, p[None, :], gamma, [0], B, K, sigma)
    return cr.covariance(items, m).mean(axis=0), p, gamma


@pytest.mark.parametrize("m", EST_M)
def test_estimate_against_numpy_eigh(m):
    rng = np.random.default_rng(8300 + m)
    for snr_db in EST_SNR_DB:
        for trial in range(2):
            R, p, gamma = _pilot_rbar(rng, m, snr_db)
            g, q = capi.calibration_estimate(R, p)
            g_ref, q_ref, w = cr.estimate(R, p, with_spectrum=True)
            bound = cr.vector_bound(R, w)
            s = cr.sine(g, g_ref)
            _worst["vector"] = max(_worst["vector"], s / bound)
            print("m=%d snr=%g dB: sine %.3g, bound %.3g (%.3g of it); quality %.6f" % (m, snr_db, s, bound, s / bound, q))
            assert s <= bound, "m=%d snr=%g: sine %.3g > %.3g" % (m, snr_db, s, bound)
            dq = abs(q - q_ref) / q_ref
            _worst["quality"] = max(_worst["quality"], dq / (8.0 * m * cr.EPS))
            assert dq <= 8.0 * m * cr.EPS, "m=%d snr=%g: quality %.17g against %.17g" % (m, snr_db, q, q_ref)
            assert 1.0 / m - 1e-12 <= q <= 1.0 + 1e-12
            # normalisation
            assert g[0].imag == 0.0 and g[0].real > 0.0
            assert abs(np.mean(np.abs(g) ** 2) - 1.0) <= m * cr.EPS
            # the estimate finds the gains: within the noise of a finite sample at 40 dB
            if snr_db >= 40.0:
                assert np.max(np.abs(g - gamma)) <= 0.02, np.max(np.abs(g - gamma))
    print("m=%d: largest sine / bound so far %.3g, largest quality difference / bound %.3g" % (m, _worst["vector"], _worst["quality"]))


def test_estimate_pure_pilot_by_hand():
    # R-bar = (gamma p)(gamma p)^H exactly: quality 1, the gains themselves
    gamma = np.array([1.0, 0.5j, -2.0], np.complex128)
    p = np.array([1.0, 1j, -1.0], np.complex64)
    u = gamma * p.astype(np.complex128)
    R = np.outer(u, np.conj(u))
    g, q = capi.calibration_estimate(R, p)
    want = gamma / np.sqrt(np.mean(np.abs(gamma) ** 2))
    assert abs(q - 1.0) <= 8 * 3 * cr.EPS
    assert np.max(np.abs(g - want)) <= 64 * cr.EPS
    # the injected noise source: ref = all ones, the eigenvector is the gain vector
    g1, q1 = capi.calibration_estimate(np.outer(gamma, np.conj(gamma)), np.ones(3, np.complex64))
    assert np.max(np.abs(g1 - want)) <= 64 * cr.EPS and abs(q1 - 1.0) <= 8 * 3 * cr.EPS
    # white noise alone: quality 1 / m
    g2, q2 = capi.calibration_estimate(np.eye(4).astype(np.complex128) * 3.0, np.ones(4, np.complex64))
    assert abs(q2 - 0.25) <= 8 * 4 * cr.EPS


def test_only_the_upper_triangle_and_the_real_diagonal_are_read():
    rng = np.random.default_rng(5)
    R, p, _ = _pilot_rbar(rng, 6, 20.0)
    junk = R + np.tril(rng.standard_normal((6, 6)), -1) * 100.0 + 1j * np.eye(6) * 3.0
    g, q = capi.calibration_estimate(R, p)
    gj, qj = capi.calibration_estimate(junk, p)
    assert np.array_equal(g.view(np.uint64), gj.view(np.uint64)) and q == qj
    gr_, qr = cr.estimate(junk, p)
    assert cr.sine(gr_, g) <= 1e-12 and abs(qr - q) <= 1e-12


def test_scaling_by_a_power_of_two_changes_nothing():
    rng = np.random.default_rng(6)
    R, p, _ = _pilot_rbar(rng, 5, 10.0)
    g, q = capi.calibration_estimate(R, p)
    for k in (-600, -30, 17, 600):
        gk, qk = capi.calibration_estimate(R * 2.0 ** k, p)
        assert np.array_equal(g.view(np.uint64), gk.view(np.uint64)) and q == qk


# ---- 3. errors and degenerate cases --------------------------------------------------------------------------------------------------

def test_estimate_errors_and_degenerate_cases():
    rng = np.random.default_rng(7)
    m = 4
    R, p, _ = _pilot_rbar(rng, m, 20.0)
    for bad in (0.0, np.nan, np.inf, complex(1.0, np.nan)):
        q = p.copy()
        q[2] = bad
        with pytest.raises(ValueError):
            capi.calibration_estimate(R, q)
    ones = np.ones(m, np.complex128)
    cases = {"zero R-bar": np.zeros((m, m), np.complex128), "negative trace": -np.eye(m).astype(np.complex128)}
    for name, val, where in (("NaN entry", np.nan, (0, 2)), ("NaN on the diagonal", np.nan, (1, 1)), ("Inf entry", np.inf, (1, 3)),
                             ("NaN below the diagonal", np.nan, (3, 0)), ("Inf in an imaginary part", complex(0, np.inf), (0, 1))):
        X = R.copy()
        X[where] = val
        cases[name] = X
    v0 = np.zeros((m, m), np.complex128)          # the principal eigenvector has a zero first component
    v0[1, 1] = 2.0
    v0[2, 2] = 1.0
    cases["v_0 == 0"] = v0
    for name, X in cases.items():
        g, q = capi.calibration_estimate(X, p)
        assert q == 0.0 and np.array_equal(g, ones), name
        gr_, qr = cr.estimate(X, p)
        assert qr == 0.0 and np.array_equal(gr_, ones), name
    L = capi.lib()
    f64p, f32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    Rp = np.ascontiguousarray(R).view(np.float64).ctypes.data_as(f64p)
    pp = p.view(np.float32).ctypes.data_as(f32p)
    g, q = np.zeros(2 * m), ctypes.c_double(0.0)
    gp = g.ctypes.data_as(f64p)
    assert L.baz_music_calibration_estimate(m, Rp, pp, gp, ctypes.byref(q)) == capi.OK
    for mm in (0, 65):
        assert L.baz_music_calibration_estimate(mm, Rp, pp, gp, ctypes.byref(q)) == capi.E_INVALID
    assert L.baz_music_calibration_estimate(m, None, pp, gp, ctypes.byref(q)) == capi.E_INVALID
    assert L.baz_music_calibration_estimate(m, Rp, None, gp, ctypes.byref(q)) == capi.E_INVALID
    assert L.baz_music_calibration_estimate(m, Rp, pp, None, ctypes.byref(q)) == capi.E_INVALID
    assert L.baz_music_calibration_estimate(m, Rp, pp, gp, None) == capi.E_INVALID


def test_apply_errors():
    t = np.ones((3, 2), np.complex64)
    for bad in (0.0, np.nan, np.inf, -np.inf, complex(np.nan, 1.0), complex(0.0, np.inf)):
        with pytest.raises(ValueError):
            capi.calibration_apply(t, np.array([1.0, bad], np.complex64))
    with pytest.raises(ValueError):
        capi.calibration_apply(t, np.ones(3, np.complex64))
    L = capi.lib()
    f32p = ctypes.POINTER(ctypes.c_float)
    out = np.zeros((3, 2), np.complex64)
    g = np.ones(2, np.complex64)
    tp, gp, op = (x.view(np.float32).ctypes.data_as(f32p) for x in (t, g, out))
    assert L.baz_music_calibration_apply(2, 3, tp, gp, op) == capi.OK and np.array_equal(out, t)
    assert L.baz_music_calibration_apply(0, 3, tp, gp, op) == capi.E_INVALID
    assert L.baz_music_calibration_apply(65, 3, tp, gp, op) == capi.E_INVALID
    assert L.baz_music_calibration_apply(2, 0, tp, gp, op) == capi.E_INVALID
    assert L.baz_music_calibration_apply(2, 3, None, gp, op) == capi.E_INVALID
    assert L.baz_music_calibration_apply(2, 3, tp, None, op) == capi.E_INVALID
    assert L.baz_music_calibration_apply(2, 3, tp, gp, None) == capi.E_INVALID


def test_null_context_calls_are_refused():
    L = capi.lib()
    on, q = ctypes.c_int(7), ctypes.c_double(0.0)
    g32, g64 = np.ones(2, np.complex64), np.zeros(2, np.complex128)
    f64p, f32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    assert L.baz_music_set_calibration(None, None) == capi.E_INVALID
    assert L.baz_music_set_calibration(None, g32.view(np.float32).ctypes.data_as(f32p)) == capi.E_INVALID
    assert L.baz_music_get_calibration(None, None, ctypes.byref(on)) == capi.E_INVALID
    assert L.baz_music_calibrate(None, g32.view(np.float32).ctypes.data_as(f32p), 1, g32.view(np.float32).ctypes.data_as(f32p),
                                 g64.view(np.float64).ctypes.data_as(f64p), ctypes.byref(q), None) == capi.E_INVALID
    assert L.baz_music_calibrate_device(None, None, 1, g32.view(np.float32).ctypes.data_as(f32p),
                                        g64.view(np.float64).ctypes.data_as(f64p), ctypes.byref(q), None) == capi.E_INVALID


# ---- 4. the effect, through the restatement and the numpy oracle ----------------------------------------------------------------------
EFFECT_RES, EFFECT_K, EFFECT_SIGMA = 360, 64, 0.1
EFFECT_PILOT_BIN, EFFECT_PILOT_ITEMS = 200, 8
EFFECT_BINS, EFFECT_ITEMS = (40, 122), 8
EFFECT_SEEDS = (9101, 9102, 9103, 9104, 9105)


def effect_row(m, seed):
    """One row of the effect table: (hits with gamma-hat applied, hits with the uncalibrated table, max |gamma-hat - gamma|, quality)."""
    rng = np.random.default_rng(seed)
    table = mo.steering_table_c64(mo.array_geometry(m), EFFECT_RES, mo.FREQUENCY, mo.SPACING)
    gamma = cr.random_gains(rng, m)
    pilot = cr.scene(rng, table, gamma, [EFFECT_PILOT_BIN], EFFECT_PILOT_ITEMS, EFFECT_K, EFFECT_SIGMA)
    rbar = cr.covariance(pilot, m).mean(axis=0)
    g_hat, quality = cr.estimate(rbar, table[EFFECT_PILOT_BIN])
    g_lib, q_lib = capi.calibration_estimate(rbar, table[EFFECT_PILOT_BIN])
    assert cr.sine(g_lib, g_hat) <= 1e-12 and abs(q_lib - quality) <= 1e-12
    items = cr.scene(rng, table, gamma, EFFECT_BINS, EFFECT_ITEMS, EFFECT_K, EFFECT_SIGMA)
    calibrated = cr.apply(table, g_hat.astype(np.complex64))
    assert np.array_equal(_bits64(calibrated), _bits64(capi.calibration_apply(table, g_hat.astype(np.complex64))))
    with_cal = cr.hits(cr.music_peaks(items, calibrated, m, 2), EFFECT_BINS, EFFECT_RES)
    without = cr.hits(cr.music_peaks(items, table, m, 2), EFFECT_BINS, EFFECT_RES)
    return with_cal, without, float(np.max(np.abs(g_hat - gamma))), float(quality)


def test_effect_table():
    print("items of %d that report both bins %s within +-1 (gains 0.7 .. 1.3, random phases; %d pilot items at bin %d, K = %d, sigma = %g)"
          % (EFFECT_ITEMS, EFFECT_BINS, EFFECT_PILOT_ITEMS, EFFECT_PILOT_BIN, EFFECT_K, EFFECT_SIGMA))
    print("  array            seed   calibrated  uncalibrated  max|g^ - g|  quality")
    for m, name in ((8, "8-element circle"), (4, "4-element square")):
        for seed in EFFECT_SEEDS:
            with_cal, without, err, quality = effect_row(m, seed)
            print("  %-16s %5d  %4d of %d   %4d of %d     %.4f       %.4f" % (name, seed, with_cal, EFFECT_ITEMS, without, EFFECT_ITEMS, err, quality))
            if m == 8:        # (the square's figures are recorded, not asserted: at 4 antennas an occasional peak lands more than a bin off)
                assert with_cal == EFFECT_ITEMS, (seed, with_cal)
                assert without == 0, (seed, without)
                assert quality >= 0.9


# ---- ABI, host only ------------------------------------------------------------------------------------------------------------------

def test_symbols_and_upper_layers_expose_the_mode():
    import inspect
    import os
    import re
    L = capi.lib()
    names = ("baz_music_set_calibration", "baz_music_get_calibration", "baz_music_calibration_apply", "baz_music_calibrate",
             "baz_music_calibrate_device", "baz_music_calibration_estimate")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "baz_music_hip.h")).read()
    for name in names:
        assert name in capi.SYMBOLS and getattr(L, name)
        assert re.search(r"BAZ_MUSIC_API int %s\(" % name, header), name
    for name in ("set_calibration", "get_calibration", "calibrate", "calibrate_device"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.calibration_apply) and callable(capi.calibration_estimate)
    from gr_baz_amd.baz import music_doa_helper as helper_mod
    for name in ("set_calibration", "calibrate_next", "last_calibration_quality"):
        assert callable(getattr(helper_mod.music_doa_helper, name))
    params = inspect.signature(helper_mod.music_doa_helper.calibrate_next).parameters
    assert params["pilot_bin"].default is None and params["ref"].default is None and params["min_quality"].default == 0.9
    from gr_baz_amd import baz                              # (imports the pybind module)
    for name in ("set_calibration", "calibration", "calibrate_next", "last_calibration_quality"):
        assert hasattr(baz.baz_music_doa_sptr, name)
