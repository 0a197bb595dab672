"""Opt-in per-item emitter-count estimate (baz_music_set_order_mode): what needs no device.  order_ref.py restates the
definition of include/baz_music_hip.h in numpy; baz_music_order_estimate compiles the decision routine the kernels call for
the host, so the rule itself is checked here against the restatement on seeded scenes."""
import ctypes

import numpy as np
import pytest

import order_ref as oref
from gr_baz_amd import capi

# (m, K, n_max, emitters, sigma, seed): the shapes of the comparison, 4,000 items each
ULA8 = [(8, 64, 4, e, 0.1, 100 + e) for e in range(4)]
SQUARE4 = [(4, 256, 2, e, 0.1, 200 + e) for e in range(3)]
WIDE16 = [(16, 256, 4, 3, 0.3, 300)]
ITEMS = 4000


# ---- the restatement against cases worked by hand -------------------------------------------------------------------------------

def test_equal_eigenvalues_count_zero():
    # every mean(ln l) - ln(mean l) is 0: L(k) = 0 for all k, the penalty decides, the smallest k wins
    for crit in ("mdl", "aic"):
        assert oref.estimate([[2.0] * 6], 64, 4, crit)[0] == 0
        v = oref.criterion_values([[2.0] * 6], 64, 4, crit)[0]
        pen = [k * (12 - k) * (0.5 * np.log(64) if crit == "mdl" else 2.0) for k in range(5)]
        np.testing.assert_allclose(v, pen, rtol=0, atol=1e-9)


def test_one_dominant_eigenvalue_counts_one():
    w = [[1.0, 1.0, 1.0, 100.0]]
    for crit in ("mdl", "aic"):
        assert oref.estimate(w, 64, 2, crit)[0] == 1
    # by hand, m = 4, N = 64, k = 0: mean ln = ln(100)/4, ln mean = ln(25.75): L(0) = -256 (1.151293 - 3.248435) = 536.868
    v = oref.criterion_values(w, 64, 2, "mdl")[0]
    assert abs(v[0] - 536.868) < 1e-2
    assert abs(v[1] - 0.5 * 7 * np.log(64)) < 1e-9            # the three equal ones: L(1) = 0
    assert abs(oref.criterion_values(w, 64, 2, "aic")[0][1] - 14.0) < 1e-9


def test_scale_invariance():
    rng = np.random.default_rng(1)
    w = np.sort(np.concatenate([rng.uniform(0.9, 1.1, (50, 5)), rng.uniform(5.0, 50.0, (50, 3))], axis=1), axis=1)
    w[25:, 5] = w[25:, 4] * 1.01                                # some rows with two, some with three above the noise
    for crit in ("mdl", "aic"):
        k0, gap = oref.estimate(w, 64, 4, crit, with_gap=True)
        assert gap.min() > 1e-6 and len(set(k0.tolist())) >= 2
        for s in (2.0 ** -300, 2.0 ** 300):
            assert np.array_equal(oref.estimate(w * s, 64, 4, crit), k0)
            assert np.array_equal(capi.order_estimate(8, 64, 4, crit, w * s), k0)


def test_clamp_engages_for_a_zero_eigenvalue():
    w = np.array([[0.0, 1.0, 1.0, 1.0, 30.0]])
    v = oref.criterion_values(w, 32, 3, "mdl")
    assert np.all(np.isfinite(v))                              # ln 0 never appears: the zero became 2^-40 * 30
    wc = w.copy(); wc[0, 0] = 30.0 * 2.0 ** -40
    assert np.array_equal(v, oref.criterion_values(wc, 32, 3, "mdl"))
    assert np.array_equal(v, oref.criterion_values([[-1e-3, 1.0, 1.0, 1.0, 30.0]], 32, 3, "mdl"))
    for crit in ("mdl", "aic"):
        assert capi.order_estimate(5, 32, 3, crit, w)[0] == oref.estimate(w, 32, 3, crit)[0]


def test_zero_and_nonfinite_rows_count_zero():
    rows = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, np.inf], [1.0, 1.0, 1.0, np.nan], [-3.0, -2.0, -1.0, 0.0]])
    for crit in ("mdl", "aic"):
        assert np.array_equal(oref.estimate(rows, 64, 3, crit), [0, 0, 0, 0])
        assert np.array_equal(capi.order_estimate(4, 64, 3, crit, rows), [0, 0, 0, 0])


# ---- the library's routine against the restatement ----------------------------------------------------------------------------

def _compare(m, K, n_max, emitters, sigma, seed, crit):
    items, _ = oref.scene(ITEMS, m, K, emitters, sigma, seed)
    w = oref.eigvals(items, m)
    k_ref, gap = oref.estimate(w, K, n_max, crit, with_gap=True)
    k_lib = capi.order_estimate(m, K, n_max, crit, w)
    close = gap < oref.GAP_RTOL
    assert close.sum() <= oref.GAP_CAP * ITEMS, "%d items at a criterion gap below %.0e" % (close.sum(), oref.GAP_RTOL)
    bad = np.nonzero((k_lib != k_ref) & ~close)[0]
    assert bad.size == 0, "item %d: library %d, restatement %d (gap %.3g)" % (bad[0], k_lib[bad[0]], k_ref[bad[0]], gap[bad[0]])
    return k_ref, float(gap.min())


@pytest.mark.parametrize("crit", ["mdl", "aic"])
@pytest.mark.parametrize("shape", ULA8 + SQUARE4 + WIDE16, ids=lambda s: "m%d_K%d_nmax%d_e%d_sig%g" % s[:5])
def test_library_routine_equals_restatement(shape, crit):
    k_ref, gmin = _compare(*shape, crit)
    print("m=%d K=%d n_max=%d emitters=%d sigma=%g %s: counts %s, smallest gap %.3g"
          % (shape[:5] + (crit, np.bincount(k_ref, minlength=shape[2] + 1).tolist(), gmin)))


# ---- detection rates (the table of DESIGN.md 8c) -------------------------------------------------------------------------------
# rate = share of items whose count equals the number of emitters in the scene; 8-element lambda/2 line array, K = 64,
# n_max = 4, 4,000 items per case, emitters at seeded random angles in [20, 160] degrees at least 20 degrees apart.  The fixed-n
# block reports 4 pairs whatever is in the air: its rate is 0 for 0 .. 3 emitters.
RATES = {   # (sigma, emitters): (MDL, AIC) measured on order_ref (this file's seeds); asserted to +-0.03, MDL at 0.1 to 1.00
    (0.1, 0): (1.000, 0.942), (0.1, 1): (1.000, 0.923), (0.1, 2): (1.000, 0.914), (0.1, 3): (1.000, 0.900),
    (2.0, 0): (1.000, 0.942), (2.0, 1): (0.969, 0.930), (2.0, 2): (0.851, 0.918), (2.0, 3): (0.642, 0.896),
}


@pytest.mark.parametrize("sigma,emitters", sorted(RATES))
def test_detection_rates(sigma, emitters):
    """MDL finds 0 .. 3 emitters at sigma = 0.1 in every item but one of the 16,000 (3,999 of 4,000 at three emitters: one
    over-estimate): asserted as 1.00 to the two decimals the table states, i.e. >= 0.995.  The other rates are recorded and
    held to +-0.03; the library's routine must give the restatement's rates."""
    items, _ = oref.scene(ITEMS, 8, 64, emitters, sigma, 100 + emitters)
    w = oref.eigvals(items, 8)
    for crit, want in zip(("mdl", "aic"), RATES[(sigma, emitters)]):
        r_ref = float(np.mean(oref.estimate(w, 64, 4, crit) == emitters))
        r_lib = float(np.mean(capi.order_estimate(8, 64, 4, crit, w) == emitters))
        print("sigma=%g emitters=%d %s: restatement %.5f, library %.5f, fixed n: %.2f" % (sigma, emitters, crit, r_ref, r_lib, float(emitters == 4)))
        assert abs(r_ref - want) <= 0.03 and abs(r_lib - r_ref) <= 0.03
        if crit == "mdl" and sigma == 0.1:
            assert r_ref >= 0.995 and r_lib >= 0.995


# ---- argument errors, host only -----------------------------------------------------------------------------------------------

def test_order_estimate_argument_errors():
    L = capi.lib()
    w = np.ones(4)
    wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(1, np.uint8)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.baz_music_order_estimate(4, 64, 2, 1, wp, 1, op) == capi.OK
    for args in ((0, 64, 0, 1), (65, 64, 2, 1), (4, 64, 4, 1), (4, 0, 2, 1), (4, 64, 2, 0), (4, 64, 2, 3), (4, 64, 2, -1)):
        assert L.baz_music_order_estimate(*args, wp, 1, op) == capi.E_INVALID, args
    assert L.baz_music_order_estimate(4, 64, 2, 1, None, 1, op) == capi.E_INVALID
    assert L.baz_music_order_estimate(4, 64, 2, 1, wp, 1, None) == capi.E_INVALID
    assert L.baz_music_order_estimate(4, 64, 2, 1, None, 0, None) == capi.OK
    with pytest.raises(ValueError):
        capi.order_estimate(4, 64, 2, "bic", w)


def test_null_context_calls_are_refused():
    L = capi.lib()
    crit = ctypes.c_int(7)
    assert L.baz_music_set_order_mode(None, 1) == capi.E_INVALID
    assert L.baz_music_get_order_mode(None, ctypes.byref(crit)) == capi.E_INVALID
    assert L.baz_music_last_orders(None, None, 0) == capi.E_INVALID
    assert not L.baz_music_last_orders_device(None)


def test_upper_layers_expose_the_mode():
    from gr_baz_amd.baz import music_doa_helper as helper_mod
    assert capi.ORDER_MODES == {None: 0, "mdl": 1, "aic": 2}
    for name in ("set_order_mode", "get_order_mode", "last_orders", "last_orders_device"):
        assert callable(getattr(capi.Context, name))
    assert callable(helper_mod.music_doa_helper.set_order_mode)
    from gr_baz_amd import baz                              # (imports the pybind module)
    assert hasattr(baz.baz_music_doa_sptr, "set_order_mode") and hasattr(baz.baz_music_doa_sptr, "last_orders")


# ---- downstream: the compass controller reads lvl == 0 as "no estimate" ---------------------------------------------------------

def test_compass_controller_on_order_mode_rows():
    from gr_baz_amd.baz import doa_compass_control as dcc
    # count 0: every pair is (0, 0) -> no direction; count 1 of n = 2: the one real pair is taken, the (0, 0) pad is not
    assert dcc.strongest_direction([0.0, 0.0], [0.0, 0.0]) is None
    got = dcc.strongest_direction([123.5, 0.0], [41.0, 0.0])
    assert got == 123.5
