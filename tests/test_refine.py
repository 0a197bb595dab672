"""Opt-in sub-bin angle refinement (baz_music_set_refine_mode): what needs no device.  refine_ref.py restates the definition of
include/baz_music_hip.h in numpy; baz_music_refine_estimate compiles the decision routine the kernel calls for the host, so the
rule itself is checked here against the restatement bit for bit, and the effect table of DESIGN.md 8d is reproduced from the
fp64 oracle."""
import ctypes

import numpy as np
import pytest

import refine_ref as rr
from gr_baz_amd import capi
from helpers import oracle_fp64
from oracle import music_oracle as mo


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _same(y):
    got, want = capi.refine_estimate(y), rr.delta(y)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert np.all(np.abs(got) <= 0.5)
    return got


# ---- the restatement against cases worked by hand -------------------------------------------------------------------------------

def test_parabola_by_hand():
    # d = 2 + 3 (x - 0.25)^2 sampled at x = -1, 0, 1: the vertex is recovered exactly
    y = [[2 + 3 * 1.25 ** 2, 2 + 3 * 0.25 ** 2, 2 + 3 * 0.75 ** 2]]
    assert rr.delta(y)[0] == 0.25
    assert rr.delta([[1.0, 0.0, 1.0]])[0] == 0.0                   # symmetric: stays
    assert rr.delta([[1.0, 0.0, 0.0]])[0] == 0.5 and rr.delta([[0.0, 0.0, 1.0]])[0] == -0.5
    assert rr.angle([10], [0.25], 360)[0] == np.float32(10.25)
    assert rr.angle([0], [-0.3], 360)[0] == np.float32(359.7)      # below bin 0: one turn is added
    assert rr.angle([7], [0.0], 3600)[0] == np.float32(7 * 360.0 / 3600)
    assert rr.angle([359], [0.4999999999], 360)[0] < np.float32(360.0)
    assert rr.angle([0], [-1e-12], 360)[0] == np.float32(0.0)      # rounds to 360.0f: stored as 0


# ---- the library's routine against the restatement, bit for bit -----------------------------------------------------------------

def test_random_triples():
    rng = np.random.default_rng(11)
    y = np.exp(rng.uniform(-40.0, 40.0, (20000, 3)))
    d = _same(y)
    assert np.count_nonzero(d) > 1000                               # (a third of random triples have their minimum in the middle)
    y0 = rng.uniform(1e-9, 1.0, (20000, 1))
    near = y0 * (1.0 + np.abs(rng.standard_normal((20000, 3))) * 10.0 ** rng.uniform(-16, 0, (20000, 3)))
    near[:, 1] = y0[:, 0]
    d = _same(near)
    assert np.count_nonzero(d) > 15000


def test_boundaries_of_the_rule():
    cases = [
        [1.0, 1.0, 2.0],        # p = 0
        [2.0, 1.0, 1.0],        # q = 0
        [1.0, 1.0, 1.0],        # p + q = 0: a plateau
        [0.0, 0.0, 0.0],
        [0.5, 1.0, 2.0],        # p < 0: a flank
        [2.0, 1.0, 0.5],        # q < 0
        [0.5, 1.0, 0.5],        # a maximum
        [1.0, 0.0, 3.0],        # y0 = 0
        [0.0, 0.0, 1.0],
        [5e-324, 0.0, 5e-324],  # denormal p, q
        [1e308, 0.0, 1.7e308],  # p + q overflows
        [1.0 + 2.0 ** -52, 1.0, 1.0 + 2.0 ** -51],
    ]
    d = _same(cases)
    assert d[0] == -0.5 and d[1] == 0.5
    assert np.all(d[2:7] == 0.0)
    assert d[7] == -0.25 and d[8] == -0.5
    assert d[9] == 0.0
    assert d[10] == 0.0
    assert d[11] == (1.0 - 2.0) / (2.0 * 3.0)


def test_nonfinite_values_stay_put():
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(3):
            y = [3.0, 1.0, 2.0]
            y[pos] = bad
            rows.append(y)
    rows.append([np.nan, np.nan, np.nan])
    rows.append([np.inf, np.inf, np.inf])
    assert np.all(_same(rows) == 0.0)
    assert _same([[3.0, 1.0, 2.0]])[0] != 0.0


# ---- the effect table of DESIGN.md 8d on the fp64 oracle ------------------------------------------------------------------------
# mo.make_config(cfg, batch, snr_db, seed=77); entries from mo.peak_pick with n = 2 on the oracle's float32 spectrum; every entry
# scored against the nearer true angle, RMS in degrees over all entries.  (cfg, snr_db, batch, emitters): (grid, refined) as measured.
EFFECT = {
    ("cfg1", 40.0, 200, (40.3, 121.7)): (0.300, 0.0286),
    ("cfg1", 40.0, 200, (40.5, 121.5)): (0.500, 0.0285),
    ("cfg1", 20.0, 200, (40.3, 121.7)): (0.431, 0.283),
    ("cfg1", 10.0, 200, (40.3, 121.7)): (0.920, 0.902),
    ("cfg2", 20.0, 100, (40.3, 121.7)): (0.133, 0.130),
    ("cfg2", 10.0, 100, (40.3, 121.7)): (0.423, 0.420),
}


def effect_rms(ang_grid, ang_refined, present, truth):
    e0 = rr.angle_error_deg(ang_grid, truth)[present]
    e1 = rr.angle_error_deg(ang_refined, truth)[present]
    return float(np.sqrt(np.mean(e0 ** 2))), float(np.sqrt(np.mean(e1 ** 2)))


def oracle_effect(cfg, snr, batch, truth):
    c = mo.make_config(cfg, batch, snr_db=snr, seed=77, angles_deg=truth)
    m, n, res = c["m"], c["n"], c["res"]
    _, _, s32, s64, _ = oracle_fp64(c["items"], c["table"], m, n)
    picks = [mo.peak_pick(s32[b], n, res) for b in range(batch)]
    ang = np.array([p[0] for p in picks])
    present = np.array([p[1] for p in picks]) != 0
    ang1, dl = rr.refine(1.0 / s64, ang, present, res)
    # the routine of the library gives the same offsets, hence the same angles
    lib = capi.refine_estimate(rr.triples(1.0 / s64, rr.bins_of(ang, res))).reshape(dl.shape)
    assert np.array_equal(_bits(np.where(present, lib, 0.0)), _bits(dl))
    return effect_rms(ang, ang1, present, truth) + (int(present.sum()), int(np.count_nonzero(dl)))


@pytest.mark.parametrize("case", sorted(EFFECT), ids=lambda c: "%s_%gdB_%g" % (c[0], c[1], c[3][0]))
def test_effect_table(case):
    cfg, snr, batch, truth = case
    grid, refined, entries, moved = oracle_effect(cfg, snr, batch, truth)
    print("%s %g dB emitters %s: %d entries, %d moved, grid %.4g deg, refined %.4g deg, ratio %.3g"
          % (cfg, snr, truth, entries, moved, grid, refined, grid / refined))
    want_grid, want_refined = EFFECT[case]
    assert abs(grid - want_grid) <= 6e-4 and abs(refined - want_refined) <= 6e-4       # (the table's rounding)
    if snr == 40.0:
        # the grid is the limit: refinement removes it (reference 10.5 and 17.6; a factor of two below the smaller covers the
        # seed-to-seed spread over 400 entries)
        assert refined <= grid / 5.0
    else:
        # noise is the limit: refinement does no harm (reference ratios refined / grid 0.65 .. 0.99)
        assert refined <= 1.05 * grid


# ---- ABI, host only -------------------------------------------------------------------------------------------------------------

def test_refine_estimate_argument_errors():
    L = capi.lib()
    y = np.array([3.0, 1.0, 2.0])
    yp = y.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(1)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.baz_music_refine_estimate(yp, 1, op) == capi.OK and out[0] == rr.delta(y)[0]
    assert L.baz_music_refine_estimate(None, 1, op) == capi.E_INVALID
    assert L.baz_music_refine_estimate(yp, 1, None) == capi.E_INVALID
    assert L.baz_music_refine_estimate(None, 0, None) == capi.OK


def test_null_context_calls_are_refused():
    L = capi.lib()
    mode = ctypes.c_int(7)
    assert L.baz_music_set_refine_mode(None, 1) == capi.E_INVALID
    assert L.baz_music_set_refine_mode(None, 2) == capi.E_INVALID
    assert L.baz_music_get_refine_mode(None, ctypes.byref(mode)) == capi.E_INVALID
    assert L.baz_music_last_refine_offsets(None, None, 0) == capi.E_INVALID
    assert L.baz_music_strerror(capi.E_INVALID) and L.baz_music_strerror(capi.E_UNSUPPORTED)


def test_symbols_and_upper_layers_expose_the_mode():
    L = capi.lib()
    for name in ("baz_music_set_refine_mode", "baz_music_get_refine_mode", "baz_music_last_refine_offsets",
                 "baz_music_refine_estimate"):
        assert name in capi.SYMBOLS and getattr(L, name)
    for name in ("set_refine_mode", "get_refine_mode", "last_refine_offsets"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.refine_estimate)
    from gr_baz_amd.baz import music_doa_helper as helper_mod
    assert callable(helper_mod.music_doa_helper.set_refine_mode)
    from gr_baz_amd import baz                              # (imports the pybind module)
    assert hasattr(baz.baz_music_doa_sptr, "set_refine_mode")
