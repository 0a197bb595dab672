"""numpy restatement of the opt-in per-antenna gain / phase calibration (baz_music_set_calibration, baz_music_calibrate,
include/baz_music_hip.h), loop for loop.

Applying:   a'_r(bin) = gamma_r a_r(bin): both operands widened exactly to fp64 (the four products are exact there),
            re = g.re a.re - g.im a.im,  im = g.re a.im + g.im a.re   (one fp64 rounding each), then one conversion to fp32.

Estimating: v = the unit eigenvector of the largest eigenvalue l1 of R-bar (here: numpy.linalg.eigh on the Hermitian matrix of the
            upper triangle and the real diagonal);  g_r = v_r / p_r;  g times conj(g_0) / |g_0|, Im g_0 = 0 exactly;  g scaled so that
            mean |g_r|^2 = 1;  quality = l1 / Re tr(R-bar).  Degenerate (a NaN / Inf in R-bar, trace not > 0, v_0 == 0): quality 0
            and g = all (1, 0).
"""
import numpy as np

EPS = 2.0 ** -52


def apply(table, gamma):
    """(res, m) complex64 calibrated table for the table (res, m) complex64 and gamma (m,) complex64."""
    t = np.asarray(table, dtype=np.complex64)
    g = np.asarray(gamma, dtype=np.complex64).reshape(-1)
    res, m = t.shape
    out = np.zeros((res, m), np.complex64)
    with np.errstate(all="ignore"):
        for r in range(m):
            gr, gi = np.float64(g[r].real), np.float64(g[r].imag)
            for b in range(res):
                ar, ai = np.float64(t[b, r].real), np.float64(t[b, r].imag)
                re = gr * ar - gi * ai
                im = gr * ai + gi * ar
                out[b, r] = np.complex64(complex(np.float32(re), np.float32(im)))
    return out


def hermitian_from_upper(R):
    R = np.asarray(R, dtype=np.complex128)
    U = np.triu(R, 1)
    return U + U.conj().T + np.diag(np.real(np.diag(R))).astype(np.complex128)


def estimate(rbar, ref, with_spectrum=False):
    """(gamma (m,) complex128, quality) of the definition; with_spectrum: additionally the ascending eigenvalues of R-bar."""
    R = np.asarray(rbar, dtype=np.complex128)
    m = R.shape[0]
    p = np.asarray(ref, dtype=np.complex64).astype(np.complex128).reshape(-1)
    ones = np.ones(m, np.complex128)
    degenerate = (ones, 0.0, np.zeros(m)) if with_spectrum else (ones, 0.0)
    if not np.all(np.isfinite(R.view(np.float64))):
        return degenerate
    trace = 0.0
    for i in range(m):
        trace = trace + R[i, i].real
    if not trace > 0.0:
        return degenerate
    w, V = np.linalg.eigh(hermitian_from_upper(R), UPLO="U")
    v = V[:, m - 1]
    v = v / np.linalg.norm(v)
    if v[0] == 0:
        return degenerate
    g = v / p
    g = g * (np.conj(g[0]) / abs(g[0]))
    g[0] = complex(abs(g[0]), 0.0)
    g = g / np.sqrt(np.mean(np.abs(g) ** 2))
    g[0] = complex(g[0].real, 0.0)
    quality = w[m - 1] / trace
    return (g, quality, w) if with_spectrum else (g, quality)


def sine(x, y):
    """The sine of the angle between two complex vectors."""
    x = np.asarray(x, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128)
    c = abs(np.vdot(x, y)) / (np.linalg.norm(x) * np.linalg.norm(y))
    # (1 - c^2 cancels near 0: the norm of the component of x orthogonal to y instead)
    yn = y / np.linalg.norm(y)
    perp = x - yn * np.vdot(yn, x)
    return float(np.linalg.norm(perp) / np.linalg.norm(x)) if c > 0 else 1.0


def vector_bound(rbar, w):
    """8 m 2^-52 |R-bar|_2 / (l1 - l2): Davis-Kahan against a backward error of m 2^-52 |R-bar|_2, eight times over."""
    m = len(w)
    norm2 = max(abs(w[0]), abs(w[-1]))
    gap = w[-1] - w[-2] if m > 1 else norm2
    return 8.0 * m * EPS * norm2 / gap


# ---- scenes and the MUSIC estimate on a table, for the effect table ----------------------------------------------------------------

def cgauss(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def random_gains(rng, m, lo=0.7, hi=1.3):
    """Gains lo .. hi, phases uniform on the circle; normalised like the estimate (g_0 > 0, mean |g|^2 = 1) so the two compare."""
    g = rng.uniform(lo, hi, m) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, m))
    g = g * (np.conj(g[0]) / abs(g[0]))
    g[0] = complex(abs(g[0]), 0.0)
    return g / np.sqrt(np.mean(np.abs(g) ** 2))


def scene(rng, table, gamma, bins, items, K, sigma, amp=1.0):
    """(items, K m) complex64: emitters of amplitude `amp` on the table's rows `bins`, seen through diag(gamma), plus white noise of
    standard deviation sigma AT THE CHANNEL OUTPUTS."""
    t = np.asarray(table).astype(np.complex128)
    m = t.shape[1]
    A = t[list(bins)] * np.asarray(gamma, dtype=np.complex128)[None, :]
    s = amp * cgauss(rng, items, K, len(bins))
    x = np.einsum("bke,em->bkm", s, A) + sigma * cgauss(rng, items, K, m)
    return np.ascontiguousarray(x.reshape(items, K * m)).astype(np.complex64)


def covariance(items, m):
    x = np.asarray(items, dtype=np.complex64).astype(np.complex128)
    B, N = x.shape
    K = N // m
    x = x.reshape(B, K, m).transpose(0, 2, 1)
    return (x @ x.conj().transpose(0, 2, 1)) / float(K)


def music_peaks(items, table, m, n):
    """Per item the bins of the n strongest circular local maxima of the MUSIC spectrum on `table` (the oracle's arithmetic and
    picker), -1 where fewer exist."""
    from oracle import music_oracle as mo
    res = np.asarray(table).shape[0]
    _, _, spec, _ = mo.music_doa_work_batch(items, table, m, n)
    out = np.full((len(items), n), -1, np.int64)
    for b in range(len(items)):
        ang, lvl = mo.peak_pick(spec[b], n, res)
        for k in range(n):
            if lvl[k] > 0:
                out[b, k] = int(round(float(ang[k]) * res / 360.0)) % res
    return out


def hits(peaks, bins, res, within=1):
    """How many items report every bin of `bins` within +- `within` bins (circular)."""
    count = 0
    for row in peaks:
        ok = True
        for b in bins:
            d = [min((int(p) - b) % res, (b - int(p)) % res) for p in row if p >= 0]
            ok = ok and len(d) > 0 and min(d) <= within
        count += bool(ok)
    return count
