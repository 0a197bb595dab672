"""numpy restatement of the opt-in per-item emitter-count estimate (baz_music_set_order_mode, include/baz_music_hip.h;
DESIGN.md 8c): the MDL / AIC criteria of Wax & Kailath on the eigenvalues of an item's covariance, plus seeded test scenes.

    N snapshots, l_1 <= ... <= l_m, clamped l_i <- max(l_i, 2^-40 l_m); for k = 0 .. n_max over the m - k smallest
        L(k)   = -N (m - k) (mean(ln l) - ln(mean l))
        MDL(k) = L(k) + 1/2 k (2m - k) ln N           AIC(k) = 2 L(k) + 2 k (2m - k)
    count = the smallest k that minimises the criterion; l_m <= 0 or non-finite -> 0.
"""
import numpy as np

from oracle import music_oracle as mo

CRITERIA = {"mdl": 1, "aic": 2}
GAP_RTOL = 1e-8          # an item whose best and runner-up criterion values are this close (relative) may be skipped ...
GAP_CAP = 1e-3           # ... by the comparing tests, up to this share of the items


def criterion_values(eigvals_ascending, nsnap, n_max, criterion):
    """(B, n_max + 1) criterion values of rows of m ascending eigenvalues (NaN rows where l_m is not a positive finite number)."""
    assert criterion in CRITERIA, criterion
    w = np.atleast_2d(np.asarray(eigvals_ascending, dtype=np.float64))
    B, m = w.shape
    assert 0 <= n_max < m
    N = float(nsnap)
    lmax = w[:, -1]
    ok = np.isfinite(lmax) & (lmax > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        floor = np.where(ok, lmax, 1.0) * 2.0 ** -40
        l = np.where(w > floor[:, None], w, floor[:, None])     # (a NaN below a finite l_m is clamped too)
        ln = np.log(l)
    out = np.full((B, n_max + 1), np.nan)
    for k in range(n_max + 1):
        p = m - k
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ll = -N * p * (ln[:, :p].sum(axis=1) / p - np.log(l[:, :p].sum(axis=1) / p))
        dof = k * (2 * m - k)
        out[:, k] = 2.0 * ll + 2.0 * dof if criterion == "aic" else ll + 0.5 * dof * np.log(N)
    out[~ok] = np.nan
    return out


def estimate(eigvals_ascending, nsnap, n_max, criterion, with_gap=False):
    """Counts (uint8) per row; with_gap: also the relative gap between the best and the runner-up criterion value (inf where
    there is no runner-up or the row counts 0 by rule)."""
    v = criterion_values(eigvals_ascending, nsnap, n_max, criterion)
    bad = np.isnan(v).any(axis=1)
    vv = np.where(bad[:, None], 0.0, v)
    k = np.argmin(vv, axis=1).astype(np.uint8)                    # (argmin returns the first = smallest k of a tie)
    k[bad] = 0
    if not with_gap:
        return k
    if v.shape[1] == 1:
        return k, np.full(v.shape[0], np.inf)
    s = np.sort(vv, axis=1)
    gap = (s[:, 1] - s[:, 0]) / np.maximum(np.abs(s[:, 0]), np.abs(s[:, 1]))
    gap[bad] = np.inf
    return k, gap


def covariance(items, m):
    x = np.asarray(items).astype(np.complex128)
    B = x.shape[0]
    K = x.shape[1] // m
    X = x.reshape(B, K, m).transpose(0, 2, 1)
    return X @ X.conj().transpose(0, 2, 1) / K


def eigvals(items, m):
    return np.linalg.eigvalsh(covariance(items, m))


def estimate_items(items, m, n_max, criterion, with_gap=False):
    K = np.asarray(items).shape[1] // m
    return estimate(eigvals(items, m), K, n_max, criterion, with_gap)


def ula(m):
    return [[i, 0] for i in range(m)]


def scene(B, m, K, emitters, sigma, seed, arr=None, amp=None, grid=None):
    """B items of `emitters` independent unit-power (or amp[i]-scaled) complex-Gaussian emitters at seeded random angles in
    [20, 160] degrees, at least 20 degrees apart, plus complex white noise of standard deviation sigma per antenna:
    (items (B, m*K) complex64, angles (B, emitters) degrees).  arr: element positions in units of the spacing (default: the
    m-element lambda/2 line array); steering vectors as oracle.music_oracle.steer.  grid: round the angles to multiples of
    this many degrees (emitters exactly on the table's bins: the deepest nulls)."""
    rng = np.random.default_rng(seed)
    arr = ula(m) if arr is None else arr
    lam = mo.C_LIGHT / mo.FREQUENCY
    pos = np.asarray(mo.scaled_array(arr, mo.SPACING), dtype=np.float64)          # (m, 2)
    ang = np.zeros((B, emitters))
    for b in range(B):
        while emitters:
            a = rng.uniform(20.0, 160.0, emitters)
            if grid:
                a = np.round(a / grid) * grid
            if emitters < 2 or np.min(np.diff(np.sort(a))) >= 20.0:
                ang[b] = a
                break
    cg = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    x = sigma * cg(B, K, m)
    if emitters:
        th = np.deg2rad(ang)
        u = np.stack([np.cos(th), np.sin(th)], axis=2)                             # (B, emitters, 2)
        A = np.exp(-1j * 2.0 * np.pi * (u @ pos.T) / lam)                          # (B, emitters, m), as mo.steer
        s = cg(B, K, emitters)
        if amp is not None:
            s = s * np.asarray(amp, dtype=np.float64)[None, None, :]
        x = x + np.einsum("bke,bem->bkm", s, A)
    return np.ascontiguousarray(x.reshape(B, K * m)).astype(np.complex64), ang
