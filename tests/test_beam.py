"""Opt-in MVDR beamformer output (baz_music_set_beam_mode): what needs no device.  beam_ref.py restates the definition of
include/baz_music_hip.h in numpy loop for loop; baz_music_beam_weights runs the same definition on the host with the kernels' own
degeneracy rule and s -> w step.  Tolerance: relative (in norm) 8 m cond_2(R_l) 2^-52, the form of the backward-error bound of an
LDL^H solve, against the restatement and against np.linalg.solve."""
import ctypes

import numpy as np
import pytest

import beam_ref as br
import order_ref as oref
import power_ref as pr
from gr_baz_amd import capi
from oracle import music_oracle as mo


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.complex128).view(np.uint64)


def _hpd(rng, m, snapshots=None, sigma=0.1, strong=30.0):
    K = snapshots or 4 * m
    X = rng.standard_normal((m, K)) + 1j * rng.standard_normal((m, K))
    X[: max(1, m // 3)] *= strong                                        # a few strong rows: cond ~ 1e3 .. 1e5 (strong = 2000: ~ 1e7)
    return X @ X.conj().T / K + sigma ** 2 * np.eye(m)


def _rows(rng, count, m):
    return (rng.standard_normal((count, m)) + 1j * rng.standard_normal((count, m))).astype(np.complex64)


def _relnorm(x, y):
    return np.linalg.norm(x - y, axis=-1) / np.linalg.norm(y, axis=-1)


# ---- the library's routine against the restatement and numpy ----------------------------------------------------------------------

def test_diagonal_by_hand():
    # R = diag(1, 2, 4), a = (1, 1, 1): R^-1 a = (1, 1/2, 1/4), s = 1.75
    R = np.diag([1.0, 2.0, 4.0]).astype(np.complex128)
    a = np.ones((1, 3), np.complex64)
    want = np.array([1.0, 0.5, 0.25]) / 1.75
    assert np.array_equal(capi.beam_weights(R, a)[0], want)
    assert np.array_equal(br.weights(R, a)[0], want)
    # loading 1: the mean diagonal 7/3 on every pivot
    d = np.array([1.0, 2.0, 4.0]) + 7.0 / 3.0
    got = capi.beam_weights(R, a, loading=1.0)[0]
    assert np.allclose(got, (1.0 / d) / np.sum(1.0 / d), rtol=1e-15, atol=0)
    assert np.allclose(got, br.weights(R, a, 1.0)[0], rtol=1e-15, atol=0)
    # m = 1: w = 1 / conj(a)
    w1 = capi.beam_weights(np.array([[3.0 + 0j]]), np.array([[2.0 + 0j]], np.complex64))
    assert w1.shape == (1, 1) and w1[0, 0] == 0.5


CASES = [(m, loading, strong) for m in list(range(1, 17)) + [64] for loading in (0.0, 1e-2) for strong in (30.0, 2000.0)]


@pytest.mark.parametrize("m,loading,strong", CASES, ids=["m%d_l%g_s%g" % c for c in CASES])
def test_three_way_agreement_distortionless_and_capon(m, loading, strong):
    """capi.beam_weights, the restatement and np.linalg.solve agree in relative norm within 8 m cond_2(R_l) 2^-52; w^H a = 1 within
    the same; at loading 0 Re(w^H R w) is the Capon power."""
    rng = np.random.default_rng(6000 + 7 * m + int(strong))
    worst = 0.0
    for trial in range(3):
        R = _hpd(rng, m, strong=strong)
        a = _rows(rng, 5, m)
        got = capi.beam_weights(R, a, loading)
        ref = br.weights(R, a, loading)
        sol = br.solve_weights(R, a, loading)
        tol = float(br.tolerance(R, loading))
        assert np.all(np.abs(got).sum(axis=1) > 0) and np.all(np.abs(ref).sum(axis=1) > 0)
        for name, x, y in (("library vs restatement", got, ref), ("library vs solve", got, sol), ("restatement vs solve", ref, sol)):
            rel = float(np.max(_relnorm(x, y)))
            worst = max(worst, rel / tol)
            assert rel <= tol, "m=%d %s: relative norm error %.3g > %.3g" % (m, name, rel, tol)
        a128 = a.astype(np.complex128)
        for name, w in (("library", got), ("restatement", ref)):
            dist = np.abs(np.einsum("em,em->e", np.conj(w), a128) - 1.0)
            assert np.all(dist <= tol), "m=%d %s: |w^H a - 1| = %.3g > %.3g" % (m, name, dist.max(), tol)
        if loading == 0.0:
            H = pr.hermitian_from_lower(R)
            P = capi.power_estimate(R, a)
            out = np.real(np.einsum("ei,ij,ej->e", np.conj(got), H, got))
            assert np.all(np.abs(out - P) <= tol * P), "m=%d: Re(w^H R w) %s against Capon %s" % (m, out, P)
    cond = tol / (8.0 * m * br.EPS)
    print("m=%d loading=%g: cond %.3g, worst relative norm difference / tolerance %.3g" % (m, loading, cond, worst))


def test_the_conditioning_of_the_cases_reaches_1e7():
    rng = np.random.default_rng(6000 + 7 * 12 + 2000)
    cond = float(br.tolerance(_hpd(rng, 12, strong=2000.0))) / (8.0 * 12 * br.EPS)
    assert cond >= 5e6, cond


def test_only_the_lower_triangle_is_read():
    rng = np.random.default_rng(5)
    R = _hpd(rng, 6)
    a = _rows(rng, 3, 6)
    junk = R + np.triu(rng.standard_normal((6, 6)), 1) * 100.0 + 1j * np.eye(6) * 3.0
    for loading in (0.0, 1e-2):
        assert np.array_equal(_bits(capi.beam_weights(junk, a, loading)), _bits(capi.beam_weights(R, a, loading)))
        assert np.array_equal(_bits(br.weights(junk, a, loading)), _bits(br.weights(R, a, loading)))


# ---- scaling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [3, 4, 8, 16])
def test_power_of_two_scaling_leaves_the_weights_unchanged(m):
    rng = np.random.default_rng(70 + m)
    R = _hpd(rng, m)
    a = _rows(rng, 4, m)
    for loading in (0.0, 1e-2):
        w = capi.beam_weights(R, a, loading)
        q = br.weights(R, a, loading)
        for k in (-30, -1, 1, 17, 100):
            assert np.array_equal(_bits(capi.beam_weights(R * 2.0 ** k, a, loading)), _bits(w))
            assert np.array_equal(_bits(br.weights(R * 2.0 ** k, a, loading)), _bits(q))


def test_large_loading_is_the_conventional_beamformer():
    rng = np.random.default_rng(31)
    for m in (4, 8, 16):
        R = _hpd(rng, m)
        a = _rows(rng, 4, m)
        a128 = a.astype(np.complex128)
        conv = a128 / np.sum(np.abs(a128) ** 2, axis=1)[:, None]
        for w in (capi.beam_weights(R, a, 1e12), br.weights(R, a, 1e12)):
            err = np.linalg.norm(w - conv, axis=1) / np.linalg.norm(w, axis=1)
            assert np.all(err <= 1e-9), err


# ---- degeneracy -------------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs_give_zero_weights():
    rng = np.random.default_rng(8)
    m = 4
    a = _rows(rng, 3, m)
    cases = {"zero R": np.zeros((m, m), np.complex128), "minus identity": -np.eye(m).astype(np.complex128)}
    X = rng.standard_normal((m, 2)) + 1j * rng.standard_normal((m, 2))
    short = X @ X.conj().T / 2
    cases["K = 2 snapshots"] = short
    nan = _hpd(rng, m)
    nan[2, 1] = np.nan
    cases["NaN entry"] = nan
    nand = _hpd(rng, m)
    nand[0, 0] = np.nan
    cases["NaN on the diagonal"] = nand
    inf = _hpd(rng, m)
    inf[3, 3] = np.inf
    cases["Inf on the diagonal"] = inf
    for name, R in cases.items():
        assert not capi.beam_weights(R, a).any(), name
        assert not br.weights(R, a).any(), name
    # loading brings the K < m item back: finite weights that match the restatement and the solve
    got = capi.beam_weights(short, a, 1e-2)
    ref = br.weights(short, a, 1e-2)
    tol = float(br.tolerance(short, 1e-2))
    assert np.isfinite(got).all() and np.all(np.abs(got).sum(axis=1) > 0)
    assert np.all(_relnorm(got, ref) <= tol) and np.all(_relnorm(got, br.solve_weights(short, a, 1e-2)) <= tol)
    # ... but not the all-zero item (its trace is 0), nor NaN
    assert not capi.beam_weights(cases["zero R"], a, 1e-2).any() and not br.weights(cases["zero R"], a, 1e-2).any()
    assert not capi.beam_weights(nan, a, 1e-2).any() and not br.weights(nan, a, 1e-2).any()
    # an all-zero steering row: s = 0 -> w = 0; its neighbours get weights
    R = _hpd(rng, m)
    rows = a.copy()
    rows[1] = 0
    got = capi.beam_weights(R, rows)
    assert not got[1].any() and got[0].any() and got[2].any()
    assert not br.weights(R, rows)[1].any()


# ---- the effect on the restatement ------------------------------------------------------------------------------------------------
EFFECT_M, EFFECT_K, EFFECT_RES, EFFECT_ITEMS = 8, 512, 720, 64
EFFECT_ANGLES = (60.0, 100.0)        # wanted, interferer
EFFECT_AMP = (0.5, 1.0)
EFFECT_SIGMA = 0.1


def effect_scene():
    """(items (B, m K) complex64, wanted waveform s (B, K) complex128, a (m,) complex64: the table row of the wanted direction)."""
    m, K, B = EFFECT_M, EFFECT_K, EFFECT_ITEMS
    rng = np.random.default_rng(2026)
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, EFFECT_RES, mo.FREQUENCY, mo.SPACING)
    bins = [int(round(t * EFFECT_RES / 360.0)) for t in EFFECT_ANGLES]
    A = table[bins].astype(np.complex128)                                  # (2, m): the emitters sit on the grid
    cg = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    s = cg(B, K, 2) * np.asarray(EFFECT_AMP)[None, None, :]
    x = EFFECT_SIGMA * cg(B, K, m) + np.einsum("bke,em->bkm", s, A)
    return np.ascontiguousarray(x.reshape(B, K * m)).astype(np.complex64), s[:, :, 0], table[bins[0]]


def residual(y, s):
    return np.sum(np.abs(y - s) ** 2, axis=-1) / np.sum(np.abs(s) ** 2, axis=-1)


def test_effect_table():
    items, s, a = effect_scene()
    m, K = EFFECT_M, EFFECT_K
    R = oref.covariance(items, m)
    X = items.reshape(len(items), K, m)
    ant0 = residual(X[:, :, 0].astype(np.complex128), s)
    print("residual sum|y - s|^2 / sum|s|^2 over %d items (ideal sigma^2 / (m amp^2) = %.4g)"
          % (len(items), EFFECT_SIGMA ** 2 / (m * EFFECT_AMP[0] ** 2)))
    print("  antenna 0 alone       mean %.4g  largest %.4g" % (ant0.mean(), ant0.max()))
    for loading in (0.0, 1e-2):
        res = np.zeros(len(items))
        for b in range(len(items)):
            w = capi.beam_weights(R[b], a[None, :], loading)
            assert float(_relnorm(w, br.weights(R[b], a[None, :], loading))[0]) <= float(br.tolerance(R[b], loading))
            res[b] = residual(br.beams(X[b], w)[0], s[b])
        print("  MVDR, loading %-6g  mean %.4g  largest %.4g  (antenna 0 / beam: %.0fx)" % (loading, res.mean(), res.max(), ant0.mean() / res.mean()))
        assert res.mean() * 20.0 <= ant0.mean(), (loading, res.mean(), ant0.mean())


# ---- ABI, host only ---------------------------------------------------------------------------------------------------------------

def test_beam_weights_argument_errors():
    L = capi.lib()
    R = np.eye(2).astype(np.complex128)
    a = np.ones(2, np.complex64)
    out = np.zeros(4)
    Rp = R.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ap = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.baz_music_beam_weights(2, Rp, ap, 1, 0.0, op) == capi.OK and np.array_equal(out, [0.5, 0.0, 0.5, 0.0])
    assert L.baz_music_beam_weights(0, Rp, ap, 1, 0.0, op) == capi.E_INVALID
    assert L.baz_music_beam_weights(65, Rp, ap, 1, 0.0, op) == capi.E_INVALID
    assert L.baz_music_beam_weights(2, None, ap, 1, 0.0, op) == capi.E_INVALID
    assert L.baz_music_beam_weights(2, Rp, None, 1, 0.0, op) == capi.E_INVALID
    assert L.baz_music_beam_weights(2, Rp, ap, 1, 0.0, None) == capi.E_INVALID
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        assert L.baz_music_beam_weights(2, Rp, ap, 1, bad, op) == capi.E_INVALID
        with pytest.raises(ValueError):
            capi.beam_weights(R, a, bad)
    assert L.baz_music_beam_weights(2, None, None, 0, 0.0, None) == capi.OK
    with pytest.raises(ValueError):
        capi.beam_weights(np.zeros((2, 3)), a)


def test_null_context_calls_are_refused():
    L = capi.lib()
    mode, loading = ctypes.c_int(7), ctypes.c_double(7.0)
    items, p = ctypes.c_uint32(7), ctypes.c_void_p(None)
    for m in (0, 1, 2):
        assert L.baz_music_set_beam_mode(None, m, 0.0) == capi.E_INVALID
    assert L.baz_music_get_beam_mode(None, ctypes.byref(mode), ctypes.byref(loading)) == capi.E_INVALID
    assert L.baz_music_last_beams(None, None, 0) == capi.E_INVALID
    assert L.baz_music_last_beam_weights(None, None, 0) == capi.E_INVALID
    assert L.baz_music_last_beams_device(None, ctypes.byref(p), ctypes.byref(items)) == capi.E_INVALID


def test_symbols_and_upper_layers_expose_the_mode():
    import inspect
    import os
    import re
    L = capi.lib()
    names = ("baz_music_set_beam_mode", "baz_music_get_beam_mode", "baz_music_last_beams", "baz_music_last_beams_device",
             "baz_music_last_beam_weights", "baz_music_beam_weights")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "baz_music_hip.h")).read()
    for name in names:
        assert name in capi.SYMBOLS and getattr(L, name)
        assert re.search(r"BAZ_MUSIC_API int %s\(" % name, header), name
    for name in ("set_beam_mode", "get_beam_mode", "last_beams", "last_beam_weights", "last_beams_device"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.beam_weights)
    from gr_baz_amd.baz import music_doa_helper as helper_mod
    assert callable(helper_mod.music_doa_helper.set_beam_mode) and callable(helper_mod.music_doa_helper.last_beams)
    params = inspect.signature(helper_mod.music_doa_helper.set_beam_mode).parameters
    assert "beam_mode" in params and params["loading"].default == 0.0
    from gr_baz_amd import baz                              # (imports the pybind module)
    assert hasattr(baz.baz_music_doa_sptr, "set_beam_mode") and hasattr(baz.baz_music_doa_sptr, "last_beams")
