"""numpy restatement of the opt-in MVDR beamformer output (baz_music_set_beam_mode, include/baz_music_hip.h), loop for
loop, on top of power_ref.ldl:

    R_l  = R with loading (sum_i Re R_ii) / m added to the real diagonal
    z_i  = a_i - sum_{k<i} L_ik z_k                 (L, d: the unpivoted LDL^H of R_l, the pivot rule on R_l's mean diagonal)
    s    = sum_i |z_i|^2 / d_i
    u_i  = z_i / d_i - sum_{k>i} conj(L_ki) u_k     (k = m-1 down to i+1)
    w    = u / s
    y[c] = sum_{r<m} conj(w_r) x[c m + r]

A degenerate item gets w = 0; an entry whose s is 0 or not finite gets w = 0.
"""
import numpy as np

import power_ref as pr

EPS = pr.EPS


def loaded(R, loading):
    """R_l: loading * (trace summed in index order) / m added to the real diagonal of R as stored."""
    R = np.array(R, dtype=np.complex128)
    m = R.shape[0]
    with np.errstate(all="ignore"):
        trace = 0.0
        for i in range(m):
            trace = trace + R[i, i].real
        delta = loading * (trace / m)
        for i in range(m):
            R[i, i] = complex(R[i, i].real + delta, R[i, i].imag)
    return R


def weights(R, rows, loading=0.0):
    """w (count, m) complex128 for one R (m, m) and steering rows (count, m) complex64."""
    m = np.asarray(R).shape[0]
    rows = np.asarray(rows, dtype=np.complex64).reshape(-1, m)
    out = np.zeros((rows.shape[0], m), np.complex128)
    f = pr.ldl(loaded(R, loading))
    if f is None:
        return out
    L, d = f
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
            u = np.zeros(m, np.complex128)
            for i in range(m - 1, -1, -1):
                ui = z[i] / d[i]
                for k in range(m - 1, i, -1):
                    ui = ui - np.conj(L[k, i]) * u[k]
                u[i] = ui
            if np.isfinite(s) and s != 0.0:
                out[e] = u / s
    return out


def beams(X, w):
    """y (count, K) complex128 for one item's snapshots X (K, m) and weights w (count, m): y[e, c] = sum_r conj(w[e, r]) X[c, r],
    accumulated in the order r = 0 .. m-1."""
    X = np.asarray(X).astype(np.complex128)
    w = np.asarray(w, dtype=np.complex128)
    y = np.zeros((w.shape[0], X.shape[0]), np.complex128)
    for r in range(X.shape[1]):
        y = y + np.conj(w[:, r])[:, None] * X[None, :, r]
    return y


def beam_bound(X, w):
    """The bound of a stored beam against beams(X, w): (sum_r |w_r| |x_r|) per (entry, snapshot), the factor of the fp64
    accumulation term 8 m 2^-52."""
    return np.abs(np.asarray(w, dtype=np.complex128)) @ np.abs(np.asarray(X).astype(np.complex128)).T


def solve_weights(R, rows, loading=0.0):
    """The same weights by np.linalg.solve (no degeneracy rule): the independent reference of the restatement."""
    H = pr.hermitian_from_lower(loaded(R, loading))
    rows = np.asarray(rows, dtype=np.complex64).astype(np.complex128).reshape(-1, H.shape[0])
    x = np.linalg.solve(H, rows.T)                      # (m, count)
    s = np.einsum("em,me->e", np.conj(rows), x)
    return (x / s[None, :]).T


def tolerance(R, loading=0.0):
    """Relative tolerance (in norm) per item, 8 m cond_2(R_l) 2^-52."""
    R = np.asarray(R)
    if R.ndim == 2:
        return pr.tolerance(loaded(R, loading))
    return np.array([pr.tolerance(loaded(r, loading)) for r in R.reshape(-1, R.shape[-2], R.shape[-1])]).reshape(R.shape[:-2])


def item_weights(R, table, bins, present, loading=0.0):
    """(B, n, m) weights for covariances R (B, m, m), the table (res, >= m) complex64, the entries' bins (B, n) and which are real."""
    R = np.asarray(R)
    B, m = R.shape[0], R.shape[1]
    out = np.zeros(bins.shape + (m,), np.complex128)
    for b in range(B):
        if present[b].any():
            w = weights(R[b], np.asarray(table)[bins[b], :m], loading)
            out[b] = np.where(present[b][:, None], w, 0.0)
    return out
