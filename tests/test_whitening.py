"""Opt-in noise pre-whitening (baz_music_set_noise_covariance), the parts that need no device: the host factorisation against its
componentwise error bounds, the host form of the table kernel's routine against the numpy restatement, and the effect of the mode on
the two coloured-noise scenes, in numpy alone."""
import numpy as np
import pytest

import calib_ref as cr
import order_ref as oref
import whiten_ref as wr
from oracle import music_oracle as mo


def _capi():
    from gr_baz_amd import capi
    return capi


_hpd = wr.hpd


# ---- 1. the factor ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [2, 4, 7, 16, 33, 64])
def test_whitening_factor_is_within_the_triangular_solve_and_cholesky_bounds(m):
    capi = _capi()
    Rn = _hpd(m, 100 + m, cond=0.05)
    W = capi.whitening_factor(Rn)
    assert W.shape == (m, m) and W.dtype == np.complex128
    assert np.array_equal(np.triu(W, 1), np.zeros((m, m)))                       # lower triangular, exactly
    d = np.diagonal(W)
    assert np.all(d.real > 0) and np.array_equal(d.imag, np.zeros(m))             # a real positive diagonal, exactly
    # the factor L the library's W inverts is the fp64 Cholesky factor in the library's loop order (whiten_ref.factor)
    L, W_ref = wr.factor(Rn)
    g = wr.factor_bounds(m)
    res_l = np.abs(L @ L.conj().T - wr.hermitian_from_lower(Rn))
    assert np.all(res_l <= g * (np.abs(L) @ np.abs(L.conj().T))), "L L^H - Rn: worst %.3g of the bound" % np.max(
        res_l / (g * (np.abs(L) @ np.abs(L.conj().T))))
    res_w = np.abs(W @ L - np.eye(m))
    bound = g * (np.abs(W) @ np.abs(L))
    assert np.all(res_w <= bound), "W L - I: worst %.3g of the bound" % np.max(res_w / bound)
    # ... and the restatement's own W is the library's to a few units of the same bound (two codings of one recurrence)
    assert np.all(np.abs(W - W_ref) <= g * (np.abs(W) @ np.abs(L) @ np.abs(W)))
    # only the lower triangle and the real diagonal are read
    junk = Rn.copy()
    junk[np.triu_indices(m, 1)] = 7.0 - 3.0j
    junk[np.arange(m), np.arange(m)] += 5.0j
    assert np.array_equal(capi.whitening_factor(junk).view(np.uint8), W.view(np.uint8))


def test_whitening_factor_of_a_power_of_four_diagonal_is_exact():
    capi = _capi()
    k = np.array([-3, -2, -1, 0, 1, 2, 3])
    W = capi.whitening_factor(np.diag(4.0 ** k).astype(np.complex128))
    assert np.array_equal(W, np.diag(2.0 ** -k).astype(np.complex128))


@pytest.mark.parametrize("m", [2, 5, 17])
def test_whitening_factor_refusals(m):
    capi = _capi()
    good = _hpd(m, 200 + m)
    bad = good.copy()
    bad[m - 1, 0] = np.nan
    with pytest.raises(ValueError):
        capi.whitening_factor(bad)
    bad = good.copy()
    bad[0, m - 1] = np.inf                       # (an entry the factor does not read: still not a covariance)
    with pytest.raises(ValueError):
        capi.whitening_factor(bad)
    zero_pivot = good.copy()
    zero_pivot[0, 0] = 0.0
    with pytest.raises(ValueError):
        capi.whitening_factor(zero_pivot)
    v = np.random.default_rng(m).standard_normal((m, 1)) + 0j
    with pytest.raises(ValueError):
        capi.whitening_factor(v @ v.conj().T)     # rank one: the second pivot is rounding noise, far below 2^-40 of the mean diagonal
    with pytest.raises(ValueError):
        capi.whitening_factor(-good)              # not positive definite


# ---- 2. the table ------------------------------------------------------------------------------------------------------------------------

def _table(m, res):
    return mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY, mo.SPACING)


@pytest.mark.parametrize("m,res", [(2, 37), (4, 360), (7, 121), (16, 90), (33, 45), (64, 31)])
def test_whiten_table_is_the_restatement_within_its_bound(m, res):
    capi = _capi()
    table = _table(m, res)
    W = capi.whitening_factor(_hpd(m, 300 + m, cond=0.1))
    got = capi.whiten_table(table, W)
    ref = wr.whiten_table(table, W)
    tol_re, tol_im = wr.whiten_table_tol(table, W, ref)
    assert got.shape == (res, m) and got.dtype == np.complex64
    assert np.all(np.abs(got.real.astype(np.float64) - ref.real) <= tol_re)
    assert np.all(np.abs(got.imag.astype(np.float64) - ref.imag) <= tol_im)
    # the upper triangle of W is not read
    junk = W.copy()
    junk[np.triu_indices(m, 1)] = np.nan
    assert np.array_equal(capi.whiten_table(table, junk).view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("m,res", [(3, 50), (8, 360), (40, 17)])
def test_whiten_table_with_the_identity_returns_the_table(m, res):
    capi = _capi()
    table = _table(m, res)
    table[1, 0] = np.complex64(complex(-0.0, 0.25))
    got = capi.whiten_table(table, np.eye(m, dtype=np.complex128))
    assert np.array_equal(got, table)                                              # values (-0 == +0)
    nz = (table.view(np.float32) != 0)
    assert np.array_equal(got.view(np.uint32)[nz], table.view(np.uint32)[nz])      # bits, wherever the component is not a zero


def test_whiten_table_with_a_power_of_two_diagonal_is_exact():
    capi = _capi()
    m, res = 8, 360
    table = _table(m, res)
    d = 2.0 ** np.array([3, -1, 0, 2, -3, 1, -2, 0])
    got = capi.whiten_table(table, np.diag(d).astype(np.complex128))
    assert np.array_equal(got, (table * d[None, :]).astype(np.complex64))


@pytest.mark.parametrize("m,res", [(4, 360), (17, 33)])
def test_calibration_then_whitening_is_the_two_host_routines_in_turn(m, res):
    capi = _capi()
    table = _table(m, res)
    rng = np.random.default_rng(400 + m)
    gamma = (rng.uniform(0.7, 1.3, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))).astype(np.complex64)
    W = capi.whitening_factor(_hpd(m, 500 + m, cond=0.1))
    applied = capi.calibration_apply(table, gamma)
    assert np.array_equal(applied.view(np.uint8), cr.apply(table, gamma).view(np.uint8))
    got = capi.whiten_table(applied, W)
    ref = wr.whiten_table(table, W, gamma=gamma)
    tol_re, tol_im = wr.whiten_table_tol(applied, W, ref)
    assert np.all(np.abs(got.real.astype(np.float64) - ref.real) <= tol_re)
    assert np.all(np.abs(got.imag.astype(np.float64) - ref.imag) <= tol_im)


def test_whiten_table_argument_checks():
    capi = _capi()
    with pytest.raises(ValueError):
        capi.whiten_table(_table(4, 10), np.eye(5))
    with pytest.raises(ValueError):
        capi.whitening_factor(np.ones((3, 4)))


# ---- 3. known answers, numpy alone ---------------------------------------------------------------------------------------------------------

def test_scene_a_unequal_channel_noise_breaks_the_emitter_count_and_whitening_restores_it():
    items, noise, table, K = wr.scene_a()
    Rn = wr.mean_covariance(noise, wr.M)                      # measured from 4096 noise-only snapshots
    _, W = wr.factor(Rn)
    R = oref.covariance(items, wr.M)
    plain = {c: wr.right_counts(R, K, c) for c in ("mdl", "aic")}
    white = {c: wr.right_counts(wr.whiten_cov(R, W), K, c) for c in ("mdl", "aic")}
    print("scene A, items with the right count: plain %r, whitened %r" % (plain, white))
    assert white["mdl"] >= 60 and plain["mdl"] <= 8           # (AIC is printed only: it over-counts now and then by nature)


def test_scene_b_two_loud_channels_break_the_bearings_and_whitening_restores_them():
    items, ang, Rn, table, K = wr.scene_b()
    _, W = wr.factor(Rn)
    R = oref.covariance(items, wr.M)
    e_plain = wr.bearing_errors(wr.music_peaks(R, table), ang)
    e_white = wr.bearing_errors(wr.music_peaks(wr.whiten_cov(R, W), wr.whiten_table(table, W)), ang)
    print("scene B, items with both emitters within 2 bins: plain %d, whitened %d; median worst-entry error %.1f / %.1f bins"
          % ((e_plain <= 2).sum(), (e_white <= 2).sum(), np.median(e_plain), np.median(e_white)))
    assert (e_white <= 2).sum() >= 60 and (e_plain <= 2).sum() <= 32
