"""numpy restatement of the opt-in noise pre-whitening (baz_music_set_noise_covariance, include/baz_music_hip.h), the
error bounds its tests hold the library to, and the two seeded scenes with coloured noise.

    Rn = L L^H (unpivoted Cholesky, from the lower triangle and the real diagonal), W = L^-1 (row by row of W L = I)
    table in force   a'_r(b) = fl32(sum_{k<=r} W_rk a~_k(b))            (a~: after the calibration where that is on)
    covariance       R' = W R W^H, R read from its lower triangle; upper = conj(lower), Im diag = +0

The library fixes an operation order (fused multiply-adds, k ascending); numpy does not offer one, so the restatement here is in
plain complex128 arithmetic and the comparisons carry the standard componentwise bounds of a length-(r+1) inner product
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 8.1 / 10.1), with the factor for complex arithmetic.
"""
import numpy as np

import order_ref as oref
from oracle import music_oracle as mo

U64 = 2.0 ** -53


def hpd(m, seed, cond=1.0):
    """A random Hermitian positive-definite matrix: A A^H / m + cond I."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    return A @ A.conj().T / m + cond * np.eye(m)


def hermitian_from_lower(R):
    """(.., m, m): the Hermitian matrix the lower triangle and the real diagonal describe."""
    R = np.asarray(R, dtype=np.complex128)
    low = np.tril(R, -1)
    d = np.real(np.diagonal(R, axis1=-2, axis2=-1))
    out = low + np.conj(np.swapaxes(low, -1, -2))
    idx = np.arange(R.shape[-1])
    out[..., idx, idx] = d
    return out


def factor(Rn):
    """(L, W) in fp64 with the library's loop order: column-by-column Cholesky, then W L = I row by row."""
    Rn = np.asarray(Rn, dtype=np.complex128)
    m = Rn.shape[0]
    L = np.zeros((m, m), np.complex128)
    for j in range(m):
        d = Rn[j, j].real
        for k in range(j):
            d = d - (L[j, k].real ** 2 + L[j, k].imag ** 2)
        if not np.isfinite(d) or d <= 0.0:
            raise ValueError("pivot %d is %r" % (j, d))
        ljj = np.sqrt(d)
        L[j, j] = ljj
        for i in range(j + 1, m):
            s = Rn[i, j]
            for k in range(j):
                s = s - L[i, k] * np.conj(L[j, k])
            L[i, j] = s / ljj
    W = np.zeros((m, m), np.complex128)
    for i in range(m):
        W[i, i] = 1.0 / L[i, i].real
        for j in range(i - 1, -1, -1):
            s = 0.0 + 0.0j
            for k in range(j + 1, i + 1):
                s = s + W[i, k] * L[k, j]
            W[i, j] = -s / L[j, j].real
    return L, W


def factor_bounds(m):
    """gamma of the two componentwise bounds |W L - I| <= g |W| |L| and |L L^H - Rn| <= g |L| |L^H|."""
    return 8.0 * (m + 1) * U64


def whiten_table(table, W, gamma=None):
    """(res, m) complex64 -> complex64; gamma (m complex64): the calibration, applied first and rounded to complex64 as calib_mul does."""
    t = np.asarray(table, dtype=np.complex64)
    if gamma is not None:
        import calib_ref as cr
        t = cr.apply(t, gamma)
    Wl = np.tril(np.asarray(W, dtype=np.complex128))
    out = t.astype(np.complex128) @ Wl.T
    return out.astype(np.complex64)


def whiten_table_tol(table, W, ref):
    """Per real component: 2^-24 |ref| + (m + 1) 2^-52 sum_k |W_rk| |a_k|  (one fp32 rounding + the fp64 inner product)."""
    t = np.abs(np.asarray(table, dtype=np.complex64).astype(np.complex128))
    m = t.shape[1]
    acc = (m + 1) * 2.0 ** -52 * (t @ np.abs(np.tril(np.asarray(W, dtype=np.complex128))).T)
    r = np.asarray(ref, dtype=np.complex64)
    return 2.0 ** -24 * np.abs(r.real) + acc, 2.0 ** -24 * np.abs(r.imag) + acc


def whiten_cov(R, W):
    """(.., m, m) -> R' = W R W^H of the Hermitian matrix R's lower triangle describes."""
    Wl = np.tril(np.asarray(W, dtype=np.complex128))
    return Wl @ hermitian_from_lower(R) @ Wl.conj().T


def whiten_cov_tol(R, W):
    """Per real component: 8 (2m + 2) 2^-53 (|W| |R| |W|^T)."""
    Wa = np.abs(np.tril(np.asarray(W, dtype=np.complex128)))
    m = Wa.shape[0]
    return 8.0 * (2 * m + 2) * U64 * (Wa @ np.abs(hermitian_from_lower(R)) @ Wa.T)


def oracle_on_R(R, table, m, n):
    """helpers.oracle_fp64 from given covariances (B, m, m) instead of items: (ang32, lvl32, spec32, strength64, w)."""
    R = np.asarray(R, dtype=np.complex128)
    B = R.shape[0]
    w, V = np.linalg.eigh(R)
    G = V[:, :, :m - n]
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    c = np.einsum("st,btk->bsk", A, G.conj())
    nrm2 = np.sum(c.real ** 2 + c.imag ** 2, axis=2)
    with np.errstate(divide="ignore"):
        strength = 1.0 / nrm2
    res = A.shape[0]
    ang = np.zeros((B, n), np.float32)
    lvl = np.zeros((B, n), np.float32)
    for b in range(B):
        ang[b], lvl[b] = mo.top_n_fast(strength[b], n, res) if np.all(np.isfinite(strength[b])) else mo.top_n_insertion(strength[b], n, res)
    return ang, lvl, strength.astype(np.float32), strength, w


# ---- the two scenes with coloured noise ----------------------------------------------------------------------------------------------
M, N_EMIT, RES, ITEMS = 8, 2, 360, 64
GAINS_A_DB = (0, 10, 0, -6, 3, 8, -3, 0)
GAINS_B_DB = (0, 20, 0, -6, 3, 20, -3, 0)


def _cg(rng, *sh):
    return (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)


def _coloured(seed, K, base, gains_db, grid=None):
    arr = mo.array_geometry(M)
    clean, ang = oref.scene(ITEMS, M, K, N_EMIT, 0.0, seed=seed, arr=arr, grid=grid)
    std = base * 10.0 ** (np.asarray(gains_db, dtype=np.float64) / 20.0)
    rng = np.random.default_rng(seed + 7)
    x = clean.astype(np.complex128).reshape(ITEMS, K, M) + std[None, None, :] * _cg(rng, ITEMS, K, M)
    table = mo.steering_table_c64(arr, RES, mo.FREQUENCY, mo.SPACING)
    return np.ascontiguousarray(x.reshape(ITEMS, K * M)).astype(np.complex64), ang, std, rng, table


def scene_a():
    """Unequal channel noise against the emitter count: (items (64, 8*64) complex64, noise-only items of the same shape, table, K)."""
    K = 64
    items, _, std, rng, table = _coloured(11, K, 0.1, GAINS_A_DB)
    noise = (std[None, None, :] * _cg(rng, ITEMS, K, M)).reshape(ITEMS, K * M).astype(np.complex64)      # 4096 further snapshots
    return items, noise, table, K


def scene_b():
    """Two loud channels against the bearings: (items (64, 8*32) complex64, emitter angles (64, 2) on the 1-degree grid, Rn = the
    diagonal of the true noise variances, table, K)."""
    K = 32
    items, ang, std, _, table = _coloured(22, K, 0.3, GAINS_B_DB, grid=1.0)
    return items, ang, np.diag(std ** 2).astype(np.complex128), table, K


def mean_covariance(items, m):
    return oref.covariance(items, m).mean(axis=0)


def right_counts(R, K, criterion, n_max=M - 1):
    """Items whose MDL / AIC count on the eigenvalues of R (B, m, m) is the true N_EMIT."""
    k = oref.estimate(np.linalg.eigvalsh(R), K, n_max, criterion)
    return int(np.sum(k == N_EMIT))


def bearing_errors(ang_found, ang_true, res=RES):
    """Per item: the worst circular distance in bins from a true emitter to the nearest reported entry."""
    f = np.asarray(ang_found, dtype=np.float64) * res / 360.0
    t = np.asarray(ang_true, dtype=np.float64) * res / 360.0
    d = np.abs(t[:, :, None] - f[:, None, :])
    d = np.minimum(d, res - d)
    return d.min(axis=2).max(axis=1)


def music_peaks(R, table, n=N_EMIT):
    """The reference MUSIC spectrum of R in fp64, rounded to float32, through the local-maximum picker: ang (B, n)."""
    _, _, spec32, _, _ = oracle_on_R(R, table, R.shape[-1], n)
    return np.stack([mo.peak_pick(s, n)[0] for s in spec32])
