"""Opt-in Capon and Bartlett spectrum estimators (baz_music_set_estimator): what needs no device.  spectrum_ref.py restates the
definitions of include/baz_music_hip.h in numpy; baz_music_spectrum_estimate runs them on the host -- kind 1 through the routine
behind baz_music_power_estimate (the same bits), kind 2 by the Bartlett loop.  Tolerance of kind 2 against the independent matmul
form: relative 8 m cond_2(R) 2^-52 (power_ref.tolerance)."""
import ctypes

import numpy as np
import pytest

import power_ref as pr
import spectrum_ref as sref
from gr_baz_amd import capi
from oracle import music_oracle as mo


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _hpd(rng, m, snapshots=None, sigma=0.1):
    K = snapshots or 4 * m
    X = rng.standard_normal((m, K)) + 1j * rng.standard_normal((m, K))
    X[: max(1, m // 3)] *= 30.0                                          # a few strong rows: cond ~ 1e3 .. 1e5
    return X @ X.conj().T / K + sigma ** 2 * np.eye(m)


def _rows(rng, count, m):
    return (rng.standard_normal((count, m)) + 1j * rng.standard_normal((count, m))).astype(np.complex64)


def test_constants_match_the_header():
    assert (capi.ESTIMATOR_MUSIC, capi.ESTIMATOR_CAPON, capi.ESTIMATOR_BARTLETT) == (0, 1, 2)
    assert (sref.MUSIC, sref.CAPON, sref.BARTLETT) == (0, 1, 2)


@pytest.mark.parametrize("m", list(range(1, 17)) + [64])
def test_capon_is_power_estimate_bit_for_bit(m):
    rng = np.random.default_rng(7000 + m)
    R = _hpd(rng, m)
    a = _rows(rng, 9, m)
    got = capi.spectrum_estimate(1, R, a)
    assert np.array_equal(_bits(got), _bits(capi.power_estimate(R, a)))
    assert np.all(got > 0)
    # the row-vectorised restatement is power_ref.power up to the rounding of numpy's vector loops (they may fuse a multiply-add)
    tol = float(pr.tolerance(R))
    assert np.max(np.abs(sref.capon(R, a) - pr.power(R, a)) / got) <= tol
    assert np.max(np.abs(got - sref.capon_solve(R, a)) / got) <= tol


def test_bartlett_by_hand():
    # R = diag(1, 2, 4), a = (1, 1, 1): q = 7, w = 3
    R = np.diag([1.0, 2.0, 4.0]).astype(np.complex128)
    a = np.ones((1, 3), np.complex64)
    assert capi.spectrum_estimate(2, R, a)[0] == 7.0 / 9.0
    assert sref.bartlett(R, a)[0] == 7.0 / 9.0
    # the imaginary part of the diagonal and the upper triangle are ignored; the lower triangle is read
    R2 = R.copy()
    R2[1, 1] = 2.0 + 5.0j
    R2[0, 2] = 77.0
    assert capi.spectrum_estimate(2, R2, a)[0] == 7.0 / 9.0 and sref.bartlett(R2, a)[0] == 7.0 / 9.0
    R3 = R.copy()
    R3[1, 0] = 0.5                                                        # y_0 += conj(R_10) a_1, y_1 += R_10 a_0: q = 8
    assert capi.spectrum_estimate(2, R3, a)[0] == 8.0 / 9.0 and sref.bartlett(R3, a)[0] == 8.0 / 9.0
    # m = 1
    assert capi.spectrum_estimate(2, np.array([[3.0 + 0j]]), np.array([[2.0 + 0j]], np.complex64))[0] == 12.0 / 16.0


@pytest.mark.parametrize("m", list(range(1, 17)) + [64])
def test_bartlett_against_the_independent_form(m):
    rng = np.random.default_rng(8000 + m)
    worst = 0.0
    for trial in range(3):
        R = _hpd(rng, m)
        a = _rows(rng, 7, m)
        got = capi.spectrum_estimate(2, R, a)
        ref = sref.bartlett(R, a)
        ind = sref.bartlett_matmul(R, a)
        tol = float(pr.tolerance(R))
        assert np.all(got > 0)
        for name, x, y in (("library vs restatement", got, ref), ("library vs matmul", got, ind), ("restatement vs matmul", ref, ind)):
            rel = np.max(np.abs(x - y) / np.abs(y))
            worst = max(worst, rel / tol)
            assert rel <= tol, "m=%d %s: relative %.3g > %.3g" % (m, name, rel, tol)
    print("m=%d: worst relative difference / tolerance %.3g" % (m, worst))


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("m", [3, 4, 8, 16])
def test_linear_in_R_exactly_for_a_power_of_two(kind, m):
    rng = np.random.default_rng(90 + m)
    R = _hpd(rng, m)
    a = _rows(rng, 6, m)
    base = capi.spectrum_estimate(kind, R, a)
    assert np.array_equal(_bits(capi.spectrum_estimate(kind, 4.0 * R, a)), _bits(4.0 * base))
    assert np.array_equal(_bits(capi.spectrum_estimate(kind, 0.25 * R, a)), _bits(0.25 * base))
    ref = {1: sref.capon, 2: sref.bartlett}[kind]
    assert np.array_equal(_bits(ref(4.0 * R, a)), _bits(4.0 * ref(R, a)))


def test_degenerate_and_nan_rules():
    rng = np.random.default_rng(17)
    m = 6
    a = _rows(rng, 4, m)
    zero = np.zeros((m, m), np.complex128)
    X = rng.standard_normal((m, 3)) + 1j * rng.standard_normal((m, 3))
    short = X @ X.conj().T / 3                                            # 3 snapshots, 6 antennas: rank 3
    nan = _hpd(rng, m)
    nan[2, 1] = np.nan
    for R in (zero, short, nan):
        assert not capi.spectrum_estimate(1, R, a).any() and not sref.capon(R, a).any()
    assert not capi.spectrum_estimate(2, zero, a).any() and not sref.bartlett(zero, a).any()
    assert not capi.spectrum_estimate(2, nan, a).any() and not sref.bartlett(nan, a).any()
    got = capi.spectrum_estimate(2, short, a)                             # Bartlett needs no inverse: a rank-deficient R is fine
    assert np.all(got > 0) and np.allclose(got, sref.bartlett_matmul(short, a), rtol=1e-12)
    # w == 0 (an all-zero row) and a row with a NaN
    R = _hpd(rng, m)
    bad = a.copy()
    bad[1] = 0
    bad[2, 3] = np.nan
    for kind, ref in ((1, sref.capon), (2, sref.bartlett)):
        got = capi.spectrum_estimate(kind, R, bad)
        assert got[1] == 0.0 and got[2] == 0.0 and got[0] > 0 and got[3] > 0
        assert np.array_equal(got == 0, ref(R, bad) == 0)


def test_invalid_arguments():
    L = capi.lib()
    m = 4
    R = np.ascontiguousarray(np.eye(m, dtype=np.complex128))
    a = np.ones((2, m), np.complex64)
    out = np.zeros(2)
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    Rp, ap, op = R.ctypes.data_as(dp), a.ctypes.data_as(fp), out.ctypes.data_as(dp)
    for kind in (1, 2):
        assert L.baz_music_spectrum_estimate(kind, m, Rp, ap, 2, op) == capi.OK
        assert L.baz_music_spectrum_estimate(kind, 0, Rp, ap, 2, op) == capi.E_INVALID
        assert L.baz_music_spectrum_estimate(kind, capi.MAX_M + 1, Rp, ap, 2, op) == capi.E_INVALID
        assert L.baz_music_spectrum_estimate(kind, m, None, ap, 2, op) == capi.E_INVALID
        assert L.baz_music_spectrum_estimate(kind, m, Rp, None, 2, op) == capi.E_INVALID
        assert L.baz_music_spectrum_estimate(kind, m, Rp, ap, 2, None) == capi.E_INVALID
        assert L.baz_music_spectrum_estimate(kind, m, None, None, 0, None) == capi.OK
    for kind in (0, 3, -1):
        assert L.baz_music_spectrum_estimate(kind, m, Rp, ap, 2, op) == capi.E_INVALID
    assert L.baz_music_set_estimator(None, 1) == capi.E_INVALID
    assert L.baz_music_get_estimator(None, None) == capi.E_INVALID
    with pytest.raises(ValueError):
        capi.spectrum_estimate(0, R, a)


def test_helper_name_mapping():
    from gr_baz_amd.baz import music_doa_helper as helper
    for kind, name in enumerate(("music", "capon", "bartlett")):
        assert helper.estimator_kind(kind) == kind
        assert helper.estimator_kind(name) == kind and helper.estimator_kind(name.upper()) == kind
    for bad in (3, -1, "mvdr", None, 1.5, True):
        with pytest.raises(ValueError):
            helper.estimator_kind(bad)
    for cls in (helper.music_doa_helper,):
        assert callable(getattr(cls, "set_estimator"))


# ---- known answer -------------------------------------------------------------------------------------------------------------------

KNOWN_ANGLES = (40.0, 122.0)
KNOWN_BOUND = {1: 1, 2: 3}        # bins: Capon resolves the pair; Bartlett is biased by the other emitter's sidelobe


def known_scene():
    """The 8-element circle, emitters at 40 and 122 degrees, 20 dB, K = 64, res = 360, 16 items, seed 5:
    (items, table, m, K, res, true bins)."""
    m, K, res = 8, 64, 360
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(16, m, m * K, arr, mo.FREQUENCY, mo.SPACING, angles_deg=KNOWN_ANGLES, snr_db=20.0, seed=5)
    return items, table, m, K, res, np.array([40, 122])


def known_answer_error(spec_rows, res, true_bins):
    """The largest circular distance in bins between a true bin and the nearer of the two strongest local maxima, over all rows."""
    worst = 0
    for row in spec_rows:
        ang, lvl = mo.peak_pick(np.asarray(row, dtype=np.float32), 2, res)
        assert np.all(lvl > 0), "fewer than two local maxima"
        bins = pr.bins_of(ang, res)
        for t in true_bins:
            dist = np.abs(bins - t)
            worst = max(worst, int(np.min(np.minimum(dist, res - dist))))
    return worst


@pytest.mark.parametrize("kind", [1, 2], ids=["capon", "bartlett"])
def test_known_answer(kind):
    import order_ref as oref
    items, table, m, K, res, true_bins = known_scene()
    R = oref.covariance(items, m)
    spec = sref.spectrum(kind, R, table)
    lib_spec = np.stack([capi.spectrum_estimate(kind, Rb, table) for Rb in R])
    assert np.allclose(lib_spec, spec, rtol=1e-9, atol=0.0)
    worst = known_answer_error(spec, res, true_bins)
    print("kind %d: strongest two local maxima within %d bins of the emitters (bound %d)" % (kind, worst, KNOWN_BOUND[kind]))
    assert worst <= KNOWN_BOUND[kind]
    assert known_answer_error(lib_spec, res, true_bins) <= KNOWN_BOUND[kind]
