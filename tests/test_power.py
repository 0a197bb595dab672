"""Opt-in per-emitter Capon power estimate (baz_music_set_power_mode): what needs no device.  power_ref.py restates the definition
of include/baz_music_hip.h in numpy loop for loop; baz_music_power_estimate runs the same definition on the host with the kernel's
own degeneracy rule and s -> P step.  Tolerance: relative 8 m cond_2(R) 2^-52 (the form of the backward-error bound of an LDL^H
solve), against the restatement and against np.linalg.solve."""
import ctypes

import numpy as np
import pytest

import order_ref as oref
import power_ref as pr
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


# ---- the library's routine against the restatement and numpy ----------------------------------------------------------------------

def test_diagonal_by_hand():
    # R = diag(1, 2, 4), a = (1, 1, 1): a^H R^-1 a = 1 + 1/2 + 1/4
    R = np.diag([1.0, 2.0, 4.0]).astype(np.complex128)
    a = np.ones((1, 3), np.complex64)
    assert capi.power_estimate(R, a)[0] == 1.0 / 1.75
    assert pr.power(R, a)[0] == 1.0 / 1.75
    # a = e_1 picks the second pivot; the imaginary part of the diagonal and the upper triangle are ignored
    R2 = R.copy()
    R2[1, 1] = 2.0 + 5.0j
    R2[0, 2] = 77.0
    e1 = np.array([[0, 1, 0]], np.complex64)
    assert capi.power_estimate(R2, e1)[0] == 2.0 and pr.power(R2, e1)[0] == 2.0
    # m = 1
    assert capi.power_estimate(np.array([[3.0 + 0j]]), np.array([[2.0 + 0j]], np.complex64))[0] == 0.75


@pytest.mark.parametrize("m", list(range(1, 17)) + [64])
def test_random_hermitian_positive_definite(m):
    rng = np.random.default_rng(4000 + m)
    worst = 0.0
    for trial in range(3):
        R = _hpd(rng, m)
        a = _rows(rng, 5, m)
        got = capi.power_estimate(R, a)
        ref = pr.power(R, a)
        sol = pr.solve(R, a)
        tol = float(pr.tolerance(R))
        assert np.all(ref > 0) and np.all(got > 0)
        for name, x, y in (("library vs restatement", got, ref), ("library vs solve", got, sol), ("restatement vs solve", ref, sol)):
            rel = np.max(np.abs(x - y) / np.abs(y))
            worst = max(worst, rel / tol)
            assert rel <= tol, "m=%d %s: relative %.3g > %.3g" % (m, name, rel, tol)
    print("m=%d: worst relative difference / tolerance %.3g" % (m, worst))


def test_only_the_lower_triangle_is_read():
    rng = np.random.default_rng(5)
    R = _hpd(rng, 6)
    a = _rows(rng, 3, 6)
    want = capi.power_estimate(R, a)
    junk = R + np.triu(rng.standard_normal((6, 6)), 1) * 100.0 + 1j * np.eye(6) * 3.0
    assert np.array_equal(_bits(capi.power_estimate(junk, a)), _bits(want))
    assert np.array_equal(_bits(pr.power(junk, a)), _bits(pr.power(R, a)))


# ---- scaling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [3, 4, 8, 16])
def test_power_of_two_scaling_is_exact(m):
    rng = np.random.default_rng(70 + m)
    R = _hpd(rng, m)
    a = _rows(rng, 4, m)
    p = capi.power_estimate(R, a)
    q = pr.power(R, a)
    for k in (-30, -1, 1, 17, 100):
        assert np.array_equal(_bits(capi.power_estimate(R * 2.0 ** k, a)), _bits(p * 2.0 ** k))
        assert np.array_equal(_bits(pr.power(R * 2.0 ** k, a)), _bits(q * 2.0 ** k))


# ---- degeneracy: all give 0 -------------------------------------------------------------------------------------------------------

def test_degenerate_inputs_give_zero():
    rng = np.random.default_rng(8)
    m = 4
    a = _rows(rng, 3, m)
    cases = {"zero R": np.zeros((m, m), np.complex128), "minus identity": -np.eye(m).astype(np.complex128)}
    X = rng.standard_normal((m, 2)) + 1j * rng.standard_normal((m, 2))
    cases["K = 2 snapshots"] = X @ X.conj().T / 2
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
        assert not capi.power_estimate(R, a).any(), name
        assert not pr.power(R, a).any(), name
    # an all-zero steering row: s = 0 -> P = 0; its neighbours are estimated
    R = _hpd(rng, m)
    rows = a.copy()
    rows[1] = 0
    got = capi.power_estimate(R, rows)
    assert got[1] == 0.0 and got[0] > 0 and got[2] > 0
    assert pr.power(R, rows)[1] == 0.0


# ---- the effect on the restatement ------------------------------------------------------------------------------------------------
EFFECT_AMP = (1.0, 0.5)
EFFECT_RANGE = (0.95, 1.02)          # (K - m + 1) / K = 0.986 at K = 512, m = 8; measured 0.988 and 0.981


def effect_scene():
    m, K, res = 8, 512, 720
    items, ang = oref.scene(64, m, K, 2, 0.1, seed=508, amp=EFFECT_AMP, grid=0.5)
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    return items, ang, table, m, K, res


def test_effect_table():
    items, ang, table, m, K, res = effect_scene()
    R = oref.covariance(items, m)
    bins = np.rint(ang * res / 360.0).astype(np.int64)
    assert np.array_equal(bins * 360.0 / res, ang)                       # the emitters sit on the grid
    P = pr.powers(R, table, bins, np.ones(bins.shape, bool))
    lib = np.stack([capi.power_estimate(R[b], table[bins[b]]) for b in range(len(R))])
    tol = pr.tolerance(R)[:, None]
    assert np.all(np.abs(lib - P) <= tol * P)
    ratio = P / np.asarray(EFFECT_AMP)[None, :] ** 2
    means = ratio.mean(axis=0)
    print("P / amp^2: means %.4g %.4g, per-item range %.3g .. %.3g; (K - m + 1) / K = %.4g"
          % (means[0], means[1], ratio.min(), ratio.max(), (K - m + 1) / K))
    assert np.all((means >= EFFECT_RANGE[0]) & (means <= EFFECT_RANGE[1])), means


# ---- ABI, host only ---------------------------------------------------------------------------------------------------------------

def test_power_estimate_argument_errors():
    L = capi.lib()
    R = np.eye(2).astype(np.complex128)
    a = np.ones(2, np.complex64)
    out = np.zeros(1)
    Rp = R.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ap = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.baz_music_power_estimate(2, Rp, ap, 1, op) == capi.OK and out[0] == 0.5
    assert L.baz_music_power_estimate(0, Rp, ap, 1, op) == capi.E_INVALID
    assert L.baz_music_power_estimate(65, Rp, ap, 1, op) == capi.E_INVALID
    assert L.baz_music_power_estimate(2, None, ap, 1, op) == capi.E_INVALID
    assert L.baz_music_power_estimate(2, Rp, None, 1, op) == capi.E_INVALID
    assert L.baz_music_power_estimate(2, Rp, ap, 1, None) == capi.E_INVALID
    assert L.baz_music_power_estimate(2, None, None, 0, None) == capi.OK
    with pytest.raises(ValueError):
        capi.power_estimate(np.zeros((2, 3)), a)


def test_null_context_calls_are_refused():
    L = capi.lib()
    mode = ctypes.c_int(7)
    for m in (0, 1, 2, 3):
        assert L.baz_music_set_power_mode(None, m) == capi.E_INVALID
    assert L.baz_music_get_power_mode(None, ctypes.byref(mode)) == capi.E_INVALID
    assert L.baz_music_last_powers(None, None, 0) == capi.E_INVALID


def test_symbols_and_upper_layers_expose_the_mode():
    import os
    import re
    L = capi.lib()
    names = ("baz_music_set_power_mode", "baz_music_get_power_mode", "baz_music_last_powers", "baz_music_power_estimate")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "baz_music_hip.h")).read()
    for name in names:
        assert name in capi.SYMBOLS and getattr(L, name)
        assert re.search(r"BAZ_MUSIC_API int %s\(" % name, header), name
    assert "BAZ_MUSIC_POWER_PIVOT_FLOOR" in header
    for name in ("set_power_mode", "get_power_mode", "last_powers"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.power_estimate)
    from gr_baz_amd.baz import music_doa_helper as helper_mod
    assert callable(helper_mod.music_doa_helper.set_power_mode) and callable(helper_mod.music_doa_helper.last_powers)
    import inspect
    assert "power_mode" in inspect.signature(helper_mod.music_doa_helper.set_power_mode).parameters
    from gr_baz_amd import baz                              # (imports the pybind module)
    assert hasattr(baz.baz_music_doa_sptr, "set_power_mode") and hasattr(baz.baz_music_doa_sptr, "last_powers")


# ---- one degeneracy rule behind the power and the beam entries ---------------------------------------------------------------------

def _dead_sets(R, a):
    """(entries baz_music_power_estimate declares dead, entries baz_music_beam_weights(loading = 0) declares dead)."""
    with np.errstate(all="ignore"):
        P = capi.power_estimate(R, a)
        w = capi.beam_weights(R, a, 0.0)
    return P == 0.0, ~(w != 0).any(axis=1)


def _floor(diag):
    """The pivot floor as the library forms it: the trace summed in index order, 2^-40 (trace / m)."""
    trace = 0.0
    for v in diag:
        trace += float(v)
    return 2.0 ** -40 * (trace / len(diag))


def _diag_at_floor(m, step):
    """diag(1 .. 1, x) with x `step` ulps from the floor the matrix itself gives (step = 0: on it)."""
    diag = np.ones(m)
    diag[-1] = 0.0
    for _ in range(8):                                                   # (the floor moves by 2^-40 / m of what x moves)
        x = _floor(diag)
        for _ in range(abs(step)):
            x = np.nextafter(x, np.inf if step > 0 else -np.inf)
        if diag[-1] == x:
            break
        diag[-1] = x
    f = _floor(diag)
    want = f
    for _ in range(abs(step)):
        want = np.nextafter(want, np.inf if step > 0 else -np.inf)
    assert diag[-1] == want
    return np.diag(diag).astype(np.complex128)


@pytest.mark.parametrize("m", list(range(1, 17)) + [64])
def test_power_and_beam_entries_declare_the_same_entries_dead(m):
    """For the same R and rows, P == 0 exactly where w (loading 0) is all zero: random positive-definite matrices (none dead, and
    one all-zero row: that entry alone), the degenerate inputs of test_degenerate_inputs_give_zero, and diagonal matrices whose last
    pivot sits one ulp above, on and one ulp below the floor 2^-40 trace / m."""
    rng = np.random.default_rng(6100 + m)
    for trial in range(3):
        R = _hpd(rng, m)
        a = _rows(rng, 5, m)
        a[3] = 0
        dead_p, dead_w = _dead_sets(R, a)
        assert np.array_equal(dead_p, dead_w)
        assert np.array_equal(dead_p, np.arange(5) == 3)
    if m == 4:
        a = _rows(rng, 3, m)
        cases = {"zero R": np.zeros((m, m), np.complex128), "minus identity": -np.eye(m).astype(np.complex128)}
        X = rng.standard_normal((m, 2)) + 1j * rng.standard_normal((m, 2))
        cases["K = 2 snapshots"] = X @ X.conj().T / 2
        for name, (i, j, v) in {"NaN entry": (2, 1, np.nan), "NaN on the diagonal": (0, 0, np.nan), "Inf on the diagonal": (3, 3, np.inf),
                                "minus zero on the diagonal": (1, 1, -0.0)}.items():
            cases[name] = _hpd(rng, m)
            cases[name][i, j] = v
        for name, R in cases.items():
            dead_p, dead_w = _dead_sets(R, a)
            assert dead_p.all() and dead_w.all(), name
    if m >= 2:
        a = _rows(rng, 3, m)
        for step, alive in ((1, True), (0, False), (-1, False)):
            dead_p, dead_w = _dead_sets(_diag_at_floor(m, step), a)
            assert np.array_equal(dead_p, dead_w), "m=%d, last pivot %+d ulp from the floor" % (m, step)
            assert (not dead_p.any()) if alive else dead_p.all(), "m=%d, last pivot %+d ulp from the floor" % (m, step)
