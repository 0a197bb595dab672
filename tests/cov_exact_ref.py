"""Covariance scenes with an exact answer.

Every covariance kernel forms R = x x^H / K as sums of fp32 x fp32 products held in fp64 and ONE division by (double)K per
real and imaginary part.  Where every sample is an integer times a power of two that depends on its
antenna only, every product entering R[a][b] is an integer multiple of the same power of two `unit[a][b]`, every partial sum
of them is too, and as long as that integer stays below 2^53 no addition rounds: the result does not depend on the order of
summation, the tile shape or the number of accumulators.  The only rounding is the division, and IEEE division is correctly
rounded.  A kernel's R can therefore be compared with `np.array_equal`, entry by entry, however weak the antenna.

make() draws such scenes: real and imaginary parts are integers in [-2^bits, 2^bits] times 2^(gain_exp[antenna] + scale_exp).
The Gram is formed in int64 (real and imaginary part apart), then R = S * unit / K in float64, the two parts divided
separately (numpy's complex-by-real division takes another route and rounds differently).  The graded gains spread the
entries of one R over 2^-40 .. 2^0 of its largest: a check relative to max|R| does not see the weak rows.

What fp32 can hold bounds the exponents: a sample needs gain_exp + scale_exp >= -149 (integers on the subnormal grid) and
bits + gain_exp + scale_exp <= 127.  The subnormal scenes (scale_exp = -139) therefore take their graded gains from
-10 .. +10 (SUBNORMAL_GAINS), the same 2^20 spread as the default -20 .. 0; make() refuses what does not widen back."""
import numpy as np

GAIN_LO, GAIN_HI = -20, 0
SUBNORMAL_SCALE, LARGE_SCALE = -139, 40
F32_TINY = 2.0 ** -126            # smallest normal float32


def graded_gains(m, lo=GAIN_LO, hi=GAIN_HI, seed=0):
    """m exponents from hi down to lo in even steps (both ends taken from two antennas on), dealt to the antennas in a seeded order"""
    g = np.round(np.linspace(hi, lo, m)).astype(np.int64)
    return g[np.random.default_rng(1000 + seed).permutation(m)]


def subnormal_gains(m, seed=0):
    return graded_gains(m, -10, 10, seed)


def make(B, m, K, bits=10, gain_exp=None, scale_exp=0, seed=0):
    """B items of K time columns of m antennas.  Returns a dict:
    items (B, K m) complex64 in the port's layout in[c m + r]; re, im (B, m, m) float64: the expected R;
    ints_re, ints_im (B, K, m) int64 and exp (m,): the integers and the per-antenna exponent the samples were made from;
    S_re, S_im (B, m, m) int64 and unit_exp (m, m): the Gram in units of 2^unit_exp."""
    rng = np.random.default_rng(seed)
    lim = 1 << bits
    ir = rng.integers(-lim, lim + 1, size=(B, K, m), dtype=np.int64)
    ii = rng.integers(-lim, lim + 1, size=(B, K, m), dtype=np.int64)
    ge = graded_gains(m, seed=seed) if gain_exp is None else np.asarray(gain_exp, dtype=np.int64)
    assert ge.shape == (m,)
    e = ge + int(scale_exp)
    assert e.min() >= -149 and bits + e.max() <= 127, "float32 cannot hold these samples"
    xr = np.ldexp(ir.astype(np.float64), e).astype(np.float32)
    xi = np.ldexp(ii.astype(np.float64), e).astype(np.float32)
    items = np.empty((B, K, m), np.complex64)
    items.real, items.imag = xr, xi
    items = items.reshape(B, K * m)
    sc = {"items": items, "ints_re": ir, "ints_im": ii, "exp": e, "B": B, "m": m, "K": K, "bits": bits}
    assert widens_back(sc), "a sample changed on its way into float32"
    # Gram in int64: S[a][b] = sum_k x_a conj(x_b) = (re_a re_b + im_a im_b) + i (im_a re_b - re_a im_b)
    rT, iT = ir.transpose(0, 2, 1), ii.transpose(0, 2, 1)
    S_re = rT @ ir + iT @ ii
    S_im = iT @ ir - rT @ ii
    # exactness: every partial sum of the 2 K products of one part, in any order, is below 2^53 units
    assert 2 * K * lim * lim < 2 ** 53
    assert max(int(np.abs(S_re).max()), int(np.abs(S_im).max())) < 2 ** 53
    U = e[:, None] + e[None, :]
    assert U.min() > -1022 + 53 and U.max() + 53 < 1023, "the Gram leaves the normal range of float64"
    sc.update(S_re=S_re, S_im=S_im, unit_exp=U,
              re=np.ldexp(S_re.astype(np.float64), U) / float(K),
              im=np.ldexp(S_im.astype(np.float64), U) / float(K))
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


def widens_back(sc):
    """every complex64 sample, widened, is the integer it was made from times its antenna's power of two"""
    x = sc["items"].reshape(sc["B"], sc["K"], sc["m"])
    return (np.array_equal(np.ldexp(x.real.astype(np.float64), -sc["exp"]), sc["ints_re"].astype(np.float64))
            and np.array_equal(np.ldexp(x.imag.astype(np.float64), -sc["exp"]), sc["ints_im"].astype(np.float64)))


def subnormal_fraction(sc):
    """share of the non-zero real and imaginary parts that are float32 subnormals"""
    v = np.abs(sc["items"].view(np.float32))
    nz = v > 0
    return float(np.mean(v[nz] < F32_TINY))


def tile_index(D, B, seed=0):
    """index vector of a batch of B items drawn from D distinct ones: every distinct item occurs (B >= D), in no period"""
    rng = np.random.default_rng(7000 + seed)
    idx = rng.integers(0, D, size=B)
    if B >= D:
        idx[rng.permutation(B)[:D]] = np.arange(D)
    return idx


def tiled(sc, idx):
    """(re, im) of the batch items[idx]: large batches cost nothing on the host (the items are gathered on the device)"""
    return sc["re"][idx], sc["im"][idx]
