"""The exact covariance reference (tests/cov_exact_ref.py) is checked here before it judges a kernel (tests/test_cov_exact_gpu.py).
CPU only."""
from fractions import Fraction

import numpy as np
import pytest

import cov_exact_ref as cx

# scene families: the graded default, equal gains, few bits, many bits, the subnormal and the large scale (graded as well)
FAMILIES = {
    "graded": dict(),
    "flat": dict(gain_exp="flat"),
    "bits2": dict(bits=2),
    "bits20": dict(bits=20),
    "subnormal": dict(gain_exp="subnormal", scale_exp=cx.SUBNORMAL_SCALE),
    "large": dict(scale_exp=cx.LARGE_SCALE),
}
SHAPES = [(3, 5, 33), (2, 8, 37), (3, 13, 50), (2, 4, 256), (2, 33, 37)]       # (B, m, K)


def scene(family, B, m, K, seed):
    kw = dict(FAMILIES[family])
    if kw.get("gain_exp") == "flat":
        kw["gain_exp"] = np.zeros(m, np.int64)
    elif kw.get("gain_exp") == "subnormal":
        kw["gain_exp"] = cx.subnormal_gains(m, seed)
    return cx.make(B, m, K, seed=seed, **kw)


def all_scenes():
    for f, fam in enumerate(sorted(FAMILIES)):
        for s, (B, m, K) in enumerate(SHAPES):
            yield fam, scene(fam, B, m, K, seed=100 * f + s)


def fraction_entry(sc, b, a, c):
    """R[b][a][c] from the complex64 samples themselves in rational arithmetic, each part rounded to float64 once"""
    x = sc["items"][b].reshape(sc["K"], sc["m"])
    sr, si = Fraction(0), Fraction(0)
    for k in range(sc["K"]):
        ar, ai = Fraction(float(x[k, a].real)), Fraction(float(x[k, a].imag))
        br, bi = Fraction(float(x[k, c].real)), Fraction(float(x[k, c].imag))
        sr += ar * br + ai * bi
        si += ai * br - ar * bi
    return float(sr / sc["K"]), float(si / sc["K"])         # Fraction -> float is int / int: correctly rounded


def test_int64_route_equals_rational_arithmetic_rounded_once():
    rng = np.random.default_rng(5)
    for fam, sc in all_scenes():
        m = sc["m"]
        picks = [(0, 0, 0), (sc["B"] - 1, m - 1, m - 1), (0, 0, m - 1), (0, m - 1, 0)]
        weak = int(np.argmin(sc["exp"]))
        picks += [(0, weak, weak), (0, weak, int(np.argmax(sc["exp"])))]
        picks += [tuple(int(v) for v in (rng.integers(sc["B"]), rng.integers(m), rng.integers(m))) for _ in range(6)]
        for b, a, c in picks:
            re, im = fraction_entry(sc, b, a, c)
            assert sc["re"][b, a, c] == re and sc["im"][b, a, c] == im, (fam, sc["K"], b, a, c)


def test_fp64_gram_in_any_column_order_has_the_same_bits():
    """the order-independence the GPU test relies on: fp64 sums of the widened samples' products, three column orders, and a
    plain left-to-right loop with two accumulators for one entry"""
    for f, (fam, sc) in enumerate(all_scenes()):
        B, K, m = sc["B"], sc["K"], sc["m"]
        x = sc["items"].reshape(B, K, m)
        for o in range(3):
            p = np.random.default_rng(10 * f + o).permutation(K)
            xr, xi = x.real.astype(np.float64)[:, p, :], x.imag.astype(np.float64)[:, p, :]
            rT, iT = xr.transpose(0, 2, 1), xi.transpose(0, 2, 1)
            re = (rT @ xr + iT @ xi) / float(K)
            im = (iT @ xr - rT @ xi) / float(K)
            assert np.array_equal(re, sc["re"]) and np.array_equal(im, sc["im"]), (fam, K, o)
        a, c = int(np.argmin(sc["exp"])), m - 1
        xr, xi = x.real.astype(np.float64)[0], x.imag.astype(np.float64)[0]
        acc = [0.0, 0.0]
        for k in range(K):
            acc[k & 1] += xr[k, a] * xr[k, c]
            acc[k & 1] += xi[k, a] * xi[k, c]
        assert (acc[0] + acc[1]) / float(K) == sc["re"][0, a, c]


def test_scales_keep_their_bookkeeping():
    for m, K in ((5, 128), (13, 64), (4, 256), (17, 33), (33, 37)):
        base = cx.make(2, m, K, gain_exp=cx.subnormal_gains(m, 9), seed=9)
        for scale in (cx.SUBNORMAL_SCALE, cx.LARGE_SCALE):
            sc = cx.make(2, m, K, gain_exp=cx.subnormal_gains(m, 9), scale_exp=scale, seed=9)
            assert np.array_equal(sc["ints_re"], base["ints_re"]) and np.array_equal(sc["S_im"], base["S_im"])
            # the same integers: R moves by exactly 2^(2 scale), no entry lost to underflow or overflow
            assert np.array_equal(sc["re"], np.ldexp(base["re"], 2 * scale)) and np.array_equal(sc["im"], np.ldexp(base["im"], 2 * scale))
            assert np.all(np.isfinite(sc["re"])) and np.all((sc["re"] != 0) == (base["re"] != 0))
            assert np.all(np.isfinite(sc["items"].view(np.float32)))
        sub = cx.make(2, m, K, gain_exp=cx.subnormal_gains(m, 9), scale_exp=cx.SUBNORMAL_SCALE, seed=9)
        assert cx.subnormal_fraction(sub) > 0.5
        assert 0.0 < cx.subnormal_fraction(sub) < 1.0           # some samples of the strong antennas are normal numbers
        assert cx.subnormal_fraction(base) == 0.0


def test_every_item_widens_back_to_its_integers():
    for fam, sc in all_scenes():
        assert cx.widens_back(sc), fam
        x = sc["items"].reshape(sc["B"], sc["K"], sc["m"])
        assert np.abs(sc["ints_re"]).max() <= 1 << sc["bits"] and np.abs(sc["ints_im"]).max() <= 1 << sc["bits"]
        # the port's layout: sample (antenna r, column c) of an item at c m + r
        assert sc["items"][0, 3 * sc["m"] + 1] == x[0, 3, 1]
    with pytest.raises(AssertionError):
        cx.make(1, 4, 8, scale_exp=cx.SUBNORMAL_SCALE)            # gains down to -20 below the subnormal grid
    with pytest.raises(AssertionError):
        cx.make(1, 4, 8, bits=27)                                 # more bits than a float32 holds


def test_graded_gains_hide_the_weak_rows_from_a_relative_check():
    for m in (2, 3, 8, 16, 33):
        sc = cx.make(2, m, 37, seed=m)
        assert sc["exp"].max() - sc["exp"].min() == 20
        big = np.abs(sc["re"]).max()
        weak = int(np.argmin(sc["exp"]))
        assert 0 < sc["re"][0, weak, weak] < 2.0 ** -36 * big      # wrong by 100 % and still inside 1e-11 max|R|


def test_tiling_by_an_index_vector():
    sc = cx.make(5, 3, 7, seed=1)
    idx = cx.tile_index(5, 23, seed=2)
    assert idx.shape == (23,) and set(idx.tolist()) == set(range(5))
    re, im = cx.tiled(sc, idx)
    assert re.shape == (23, 3, 3) and np.array_equal(re[7], sc["re"][idx[7]]) and np.array_equal(im[22], sc["im"][idx[22]])
    assert not np.array_equal(idx[:5], idx[5:10]) or not np.array_equal(idx[:5], idx[10:15])
