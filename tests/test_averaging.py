"""CPU tests of the opt-in covariance averaging across stream items (baz_music_set_averaging, include/baz_music_hip.h;
DESIGN.md 8e): the library's weight routine against the numpy restatement bit for bit, argument validation without a device,
the boxcar identity that holds the mode to the existing oracle, and the effect table DESIGN.md quotes."""
import ctypes

import numpy as np
import pytest

import averaging_ref as aref
from gr_baz_amd import capi
from oracle import music_oracle as mo

WEIGHT_CASES = [(1, 1.0), (2, 1.0), (8, 1.0), (64, 1.0), (5, 0.5), (64, 0.9), (3, 1e-3)]


@pytest.mark.parametrize("W,beta", WEIGHT_CASES)
def test_weights_match_the_restatement_bit_for_bit(W, beta):
    w, inv, ne = capi.averaging_weights(W, beta)
    w_ref, inv_ref, ne_ref = aref.weights(W, beta)
    assert w.shape == (W,) and inv.shape == (W + 1,)
    assert w.tobytes() == w_ref.tobytes()
    assert inv.tobytes() == inv_ref.tobytes()
    assert np.float64(ne).tobytes() == np.float64(ne_ref).tobytes()
    assert w[0] == 1.0 and inv[0] == 0.0 and inv[1] == 1.0
    if beta == 1.0:
        assert ne == float(W) and np.all(w == 1.0) and np.array_equal(inv[1:], 1.0 / np.arange(1, W + 1))
    else:
        assert 1.0 <= ne < W or W == 1


def test_weights_accept_null_outputs():
    L = capi.lib()
    ne = ctypes.c_double(0.0)
    assert L.baz_music_averaging_weights(8, 1.0, None, None, ctypes.byref(ne)) == capi.OK and ne.value == 8.0
    assert L.baz_music_averaging_weights(8, 0.5, None, None, None) == capi.OK


@pytest.mark.parametrize("W,beta", [(0, 1.0), (65, 1.0), (4, 0.0), (4, -0.5), (4, 1.5), (4, float("nan")), (4, float("inf"))])
def test_arguments_are_validated_without_a_device(W, beta):
    L = capi.lib()
    assert capi.MAX_AVG_WINDOW == 64
    w = (ctypes.c_double * 66)()
    assert L.baz_music_averaging_weights(W, beta, w, w, None) == capi.E_INVALID
    assert L.baz_music_set_averaging(None, W, beta) == capi.E_INVALID
    with pytest.raises(ValueError):
        capi.averaging_weights(W, beta)


def test_null_context():
    L = capi.lib()
    W, b = ctypes.c_uint32(0), ctypes.c_double(0.0)
    assert L.baz_music_set_averaging(None, 4, 1.0) == capi.E_INVALID
    assert L.baz_music_get_averaging(None, ctypes.byref(W), ctypes.byref(b)) == capi.E_INVALID
    assert L.baz_music_reset_averaging(None) == capi.E_INVALID
    assert L.baz_music_debug_average(None, None, 1, None) == capi.E_INVALID


@pytest.mark.parametrize("m,n,nsamples,W", [(4, 2, 64, 4), (8, 2, 128, 3), (5, 2, 50, 8)])
def test_boxcar_is_the_covariance_of_the_concatenated_item(m, n, nsamples, W):
    """Rbar_t of the restatement equals, up to scale, the plain covariance of [X_{t-c+1} .. X_t]; the oracle's own work() on
    that item gives the spectrum of MUSIC from Rbar_t."""
    res = 180
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(2 * W + 3, m, nsamples, arr, mo.FREQUENCY, mo.SPACING, snr_db=15.0, seed=5 + m)
    Rbar = aref.average(aref.covariance(items, m), W, 1.0)
    _, _, _, s64, _ = aref.music_from_R(Rbar, table, n)
    for t in range(len(items)):
        cat = aref.concatenated(items, t, W)
        assert cat.shape[0] == aref.taps(t, W) * nsamples
        Rc = aref.covariance(cat[None, :], m)[0]
        scale = np.vdot(Rc, Rbar[t]).real / np.vdot(Rc, Rc).real
        assert np.max(np.abs(scale * Rc - Rbar[t])) <= 1e-13 * np.max(np.abs(Rbar[t]))
        assert abs(scale - 1.0) <= 1e-13                  # (the boxcar's normalisation makes the scale 1)
        _, _, _, internals = mo.music_doa_work(cat, table, m, n, return_internals=True)
        assert np.max(np.abs(internals["strength"] - s64[t]) / s64[t]) <= 1e-10


def test_exponential_weights_favour_recent_items():
    """beta < 1: Rbar is a convex combination with decreasing weights; a constant stream is a fixed point."""
    rng = np.random.default_rng(3)
    R = rng.standard_normal((12, 3, 3)) + 1j * rng.standard_normal((12, 3, 3))
    out = aref.average(R, 5, 0.5)
    w, inv, _ = aref.weights(5, 0.5)
    t = 9
    want = sum(w[j] * R[t - j] for j in range(5)) * inv[5]
    assert np.allclose(out[t], want, rtol=1e-14, atol=0)
    assert np.array_equal(out[0], R[0])
    const = np.repeat(R[:1], 12, axis=0)
    assert np.allclose(aref.average(const, 5, 0.5), const, rtol=1e-15, atol=0)


def _effect_row(table, items, W, n):
    Rbar = aref.average(aref.covariance(items, aref.EFFECT["m"]), W, 1.0)
    _, _, spec32, _, _ = aref.music_from_R(Rbar, table, n)
    return aref.effect_stats(*aref.pick_peaks(spec32, n))


def test_effect_table():
    """The table of DESIGN.md 8e, regenerated: unit square, two emitters, 64 samples per item, the local-maximum picker
    (mo.peak_pick), both emitters to be reported within 3 degrees."""
    n = aref.EFFECT["n"]
    rows = {}
    print("\n| SNR | window W | both found | RMS error of reported peaks |\n|---|---|---|---|")
    for snr, Ws in ((10.0, (1, 4, 8)), (0.0, (1, 8, 32))):
        table, items = aref.effect_scene(snr)
        for W in Ws:
            rows[(snr, W)] = _effect_row(table, items, W, n)
            print("| %g dB | %d%s | %.3f | %.2f deg |" % (snr, W, " (off)" if W == 1 else "", *rows[(snr, W)]))
    assert rows[(10.0, 1)][0] <= 0.85
    assert rows[(10.0, 8)][0] >= 0.99
    assert rows[(10.0, 8)][1] <= 0.5 * rows[(10.0, 1)][1]
