"""numpy restatement of the opt-in per-emitter Capon power estimate (baz_music_set_power_mode, include/baz_music_hip.h;
DESIGN.md 8f), loop for loop:

    d_j  = Re R_jj - sum_{k<j} |L_jk|^2 d_k
    L_ij = (R_ij - sum_{k<j} L_ik conj(L_jk) d_k) / d_j        (i > j)
    z_i  = a_i - sum_{k<i} L_ik z_k
    s    = sum_i |z_i|^2 / d_i
    P    = 1 / s

from the lower triangle of R as stored, the imaginary part of the diagonal ignored.  An item is degenerate when some d_j is not
finite or d_j <= 2^-40 (sum_i Re R_ii) / m: all its entries get 0.  An entry whose s is 0 or not finite gets 0.
"""
import numpy as np

PIVOT_FLOOR = 2.0 ** -40        # BAZ_MUSIC_POWER_PIVOT_FLOOR
EPS = 2.0 ** -52


def ldl(R):
    """(L (m, m) complex128 unit lower triangular, d (m,) float64) of one R, or None for a degenerate item."""
    R = np.asarray(R, dtype=np.complex128)
    m = R.shape[0]
    with np.errstate(all="ignore"):
        trace = 0.0
        for i in range(m):
            trace = trace + R[i, i].real
        floor = PIVOT_FLOOR * (trace / m)
        L = np.zeros((m, m), np.complex128)
        d = np.zeros(m, np.float64)
        for j in range(m):
            dj = R[j, j].real
            for k in range(j):
                dj = dj - (L[j, k].real * L[j, k].real + L[j, k].imag * L[j, k].imag) * d[k]
            if not np.isfinite(dj) or not dj > floor:
                return None
            d[j] = dj
            L[j, j] = 1.0
            for i in range(j + 1, m):
                v = R[i, j]
                for k in range(j):
                    v = v - L[i, k] * np.conj(L[j, k]) * d[k]
                L[i, j] = v / dj
    return L, d


def power(R, rows):
    """P (count,) float64 for one R (m, m) and steering rows (count, m) complex64."""
    rows = np.asarray(rows, dtype=np.complex64).reshape(-1, np.asarray(R).shape[0])
    out = np.zeros(rows.shape[0], np.float64)
    f = ldl(R)
    if f is None:
        return out
    L, d = f
    m = len(d)
    with np.errstate(all="ignore"):
        for e in range(rows.shape[0]):
            a = rows[e].astype(np.complex128)
            z = np.zeros(m, np.complex128)
            s = 0.0
            for i in range(m):
                zi = a[i]
                for k in range(i):
                    zi = zi - L[i, k] * z[k]
                z[i] = zi
                s = s + (zi.real * zi.real + zi.imag * zi.imag) / d[i]
            out[e] = 1.0 / s if (np.isfinite(s) and s != 0.0) else 0.0
    return out


def bins_of(ang, res):
    """The grid bin of every reported angle, as refine_kernel recovers it."""
    b = np.rint(np.asarray(ang, dtype=np.float64) * res / 360.0).astype(np.int64)
    return np.minimum(b, res - 1)


def powers(R, table, bins, present):
    """(B, n) powers for covariances R (B, m, m), the table (res, >= m) complex64 (its first m columns are used), the entries'
    bins (B, n) and which entries are real."""
    R = np.asarray(R)
    B, m = R.shape[0], R.shape[1]
    out = np.zeros(bins.shape, np.float64)
    for b in range(B):
        if present[b].any():
            p = power(R[b], np.asarray(table)[bins[b], :m])
            out[b] = np.where(present[b], p, 0.0)
    return out


def hermitian_from_lower(R):
    """The Hermitian matrix the definition sees: the lower triangle as stored, the diagonal's imaginary part dropped."""
    R = np.asarray(R, dtype=np.complex128)
    low = np.tril(R, -1)
    return low + np.conj(np.swapaxes(low, -1, -2)) + np.real(np.diagonal(R, axis1=-2, axis2=-1))[..., None] * np.eye(R.shape[-1])


def tolerance(R):
    """Relative tolerance per item, 8 m cond_2(R) 2^-52: the form of the backward-error bound of an LDL^H solve (inf for an item
    numpy cannot condition)."""
    H = hermitian_from_lower(R)
    m = H.shape[-1]
    flat = H.reshape(-1, m, m)
    c = np.full(flat.shape[0], np.inf)
    for b in range(flat.shape[0]):
        if np.isfinite(flat[b]).all():
            with np.errstate(all="ignore"):
                cb = np.linalg.cond(flat[b])
            c[b] = cb if np.isfinite(cb) else np.inf
    return (8.0 * m * c * EPS).reshape(H.shape[:-2])


def solve(R, rows):
    """The same powers by np.linalg.solve (no degeneracy rule): the independent reference of the restatement."""
    H = hermitian_from_lower(R)
    rows = np.asarray(rows, dtype=np.complex64).astype(np.complex128).reshape(-1, H.shape[0])
    x = np.linalg.solve(H, rows.T)
    return 1.0 / np.real(np.einsum("em,me->e", np.conj(rows), x))
