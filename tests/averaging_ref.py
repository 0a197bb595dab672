"""numpy restatement of the opt-in covariance averaging across the items of a stream (baz_music_set_averaging,
include/baz_music_hip.h), plus the seeded scene of the effect table.

    w_0 = 1, w_j = w_{j-1} beta (fp64);   c(t) = min(W, t + 1)
    Rbar_t = (sum_{j = c(t)-1 .. 0} w_j R_{t-j}) inv_norm[c(t)],   inv_norm[c] = 1 / sum_{j < c} w_j   (summed j ascending)

weights() is one IEEE fp64 operation per step in the order written, so the library's routine (baz_music_averaging_weights, the
text the kernels' table is filled with) must agree bit for bit.  average() accumulates oldest tap first like the kernel, but
with a multiply and an add where the kernel has one FMA: the two agree to rounding, not bit for bit.
"""
import numpy as np

from oracle import music_oracle as mo

MAX_WINDOW = 64


def weights(W, beta):
    """(w[W], inv_norm[W + 1], n_eff): inv_norm[0] = 0 (no item has no tap), n_eff = (sum w)^2 / sum w^2 of the full window."""
    W = int(W)
    assert 1 <= W <= MAX_WINDOW and 0.0 < beta <= 1.0
    beta = float(beta)
    w = np.zeros(W, np.float64)
    inv = np.zeros(W + 1, np.float64)
    s, s2, cur = 0.0, 0.0, 1.0
    for j in range(W):
        if j:
            cur = cur * beta
        w[j] = cur
        s = s + cur
        s2 = s2 + cur * cur
        inv[j + 1] = 1.0 / s
    return w, inv, (s * s) / s2


def taps(t, W):
    return min(int(W), int(t) + 1)


def average(R, W, beta=1.0, dtype=np.complex128):
    """R: (T, ...) plain covariances of stream items 0 .. T-1 -> Rbar of the same shape (complex128).  dtype: the accumulator
    (np.clongdouble makes this restatement's own rounding negligible beside the kernel's)."""
    R = np.asarray(R)
    w, inv, _ = weights(W, beta)
    real = np.float64 if dtype == np.complex128 else np.longdouble
    out = np.zeros(R.shape, np.complex128)
    for t in range(R.shape[0]):
        c = taps(t, W)
        acc = np.zeros(R.shape[1:], dtype)
        for j in range(c - 1, -1, -1):                     # oldest tap first
            acc = acc + real(w[j]) * R[t - j].astype(dtype)
        out[t] = (acc * real(inv[c])).astype(np.complex128)
    return out


def covariance(items, m):
    """Plain fp64 covariance of every item, (B, m, m): x(r, c) = in[c*m + r], R = x x^H / K."""
    x = np.asarray(items).astype(np.complex128)
    B = x.shape[0]
    K = x.shape[1] // m
    X = x.reshape(B, K, m).transpose(0, 2, 1)
    return X @ X.conj().transpose(0, 2, 1) / K


def music_from_R(R, table, n):
    """MUSIC of given covariances (B, m, m) in fp64 -- the arithmetic of helpers.oracle_fp64 from R on:
    (ang32, lvl32, spec32, strength64, w) with w the ascending eigenvalues, so that helpers.spectrum_tol and the other bound
    functions apply."""
    R = np.asarray(R, dtype=np.complex128)
    B, m, _ = R.shape
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
        if np.all(np.isfinite(strength[b])):
            ang[b], lvl[b] = mo.top_n_fast(strength[b], n, res)
        else:
            ang[b], lvl[b] = mo.top_n_insertion(strength[b], n, res)
    return ang, lvl, strength.astype(np.float32), strength, w


def concatenated(items, t, W):
    """The item [X_{t-c+1} .. X_t] of c(t) nsamples samples: for beta = 1 its plain covariance is Rbar_t up to scale."""
    c = taps(t, W)
    return np.concatenate([np.asarray(items[k]) for k in range(t - c + 1, t + 1)])


def windows(items, W):
    """The concatenated items of a whole stream grouped by tap count: [(c, stream indices, (len, c nsamples) items)], the
    start-up items first."""
    items = np.asarray(items)
    T = items.shape[0]
    groups = []
    for t in range(min(W - 1, T)):
        groups.append((t + 1, np.array([t]), concatenated(items, t, W)[None, :]))
    if T >= W:
        idx = np.arange(W - 1, T)
        groups.append((W, idx, np.stack([concatenated(items, t, W) for t in idx])))
    return groups


# ---- the effect table: unit square, two emitters, short items --------------------------------------------------
EFFECT = dict(m=4, n=2, nsamples=64, res=360, seed=77, items=2000, angles=(40.3, 121.7), within=3.0)


def effect_scene(snr_db, items=None):
    E = EFFECT
    arr = mo.array_geometry(E["m"])
    table = mo.steering_table_c64(arr, E["res"], mo.FREQUENCY, mo.SPACING)
    x = mo.synth_items(items or E["items"], E["m"], E["nsamples"], arr, mo.FREQUENCY, mo.SPACING, angles_deg=E["angles"],
                       snr_db=snr_db, seed=E["seed"])
    return table, x


def peak_errors(ang, lvl):
    """Circular distance in degrees of every reported entry to the nearer true angle; NaN where the entry is missing (lvl 0)."""
    a = np.asarray(ang, dtype=np.float64)[..., None]
    e = np.abs((a - np.asarray(EFFECT["angles"]) + 180.0) % 360.0 - 180.0)
    return np.where(np.asarray(lvl) > 0, e.min(axis=-1), np.nan)


def effect_stats(ang, lvl):
    """(share of items with both emitters reported within EFFECT['within'] degrees, RMS error of the reported peaks)."""
    a = np.asarray(ang, dtype=np.float64)[..., None]
    e = np.abs((a - np.asarray(EFFECT["angles"]) + 180.0) % 360.0 - 180.0)            # (B, n, 2)
    hit = (e <= EFFECT["within"]) & (np.asarray(lvl) > 0)[..., None]
    both = hit.any(axis=1).all(axis=1)
    err = peak_errors(ang, lvl)
    return float(np.mean(both)), float(np.sqrt(np.nanmean(err ** 2)))


def pick_peaks(spec32, n):
    """mo.peak_pick of every float32 spectrum row: (ang (B, n), lvl (B, n))."""
    rows = [mo.peak_pick(s, n) for s in np.asarray(spec32, dtype=np.float32)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
