"""numpy restatement of the opt-in forward-backward averaging / spatial smoothing mode (baz_music_set_smoothing,
include/baz_music_hip.h): the re-stacking, the table's structure checks, and coherent-emitter test signals.  The device runs
the inner context on restack(items) and table[:, :ms]; tests compare it with helpers.oracle_fp64 of exactly that."""
import numpy as np

from oracle import music_oracle as mo

TOL = 1e-5          # relative tolerance of the structure checks (the library's SMOOTH_TOL)


def restack(items, m, ms, fb=False, perm=None):
    """(B, m*K) complex64 items, x(r, c) = in[c*m + r] -> (B, ms*K') re-stacked items, K' = L K (fb ? 2 : 1):
    Y = [X_0 .. X_{L-1} (, P conj(X_0) .. P conj(X_{L-1}))], X_l = rows l .. l+ms-1, P the involution perm."""
    x = np.asarray(items, dtype=np.complex64)
    B = x.shape[0]
    K = x.shape[1] // m
    X = x.reshape(B, K, m)                                  # [item][column][row]
    L = m - ms + 1
    blocks = [X[:, :, l:l + ms] for l in range(L)]
    if fb:
        p = np.asarray(perm if perm is not None else np.arange(ms)[::-1], dtype=np.intp)
        blocks += [np.conj(X[:, :, l:l + ms][:, :, p]) for l in range(L)]
    return np.ascontiguousarray(np.concatenate(blocks, axis=1)).reshape(B, -1).astype(np.complex64)


def covariance(items, m):
    x = np.asarray(items).astype(np.complex128)
    B = x.shape[0]
    K = x.shape[1] // m
    X = x.reshape(B, K, m).transpose(0, 2, 1)
    return X @ X.conj().transpose(0, 2, 1) / K


def _scale(A):
    return np.max(np.abs(A) ** 2, axis=1)


def shift_invariant(table, ms):
    """a_{i+l} a_0 == a_i a_l for i < ms, l < L on every bin, to TOL * max_k |a_k|^2."""
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    m = A.shape[1]
    s = _scale(A)
    for l in range(1, m - ms + 1):
        d = A[:, l:l + ms] * A[:, :1] - A[:, :ms] * A[:, l:l + 1]
        if np.any(np.abs(d) > TOL * s[:, None]):
            return False
    return True


def fb_holds(table, ms, perm):
    """conj(a_i) = c(theta) a_perm(i) on every bin, stated through the bin's largest element k: conj(a_i) a_perm(k) ==
    conj(a_k) a_perm(i), to TOL * |a_k|^2."""
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)[:, :ms]
    p = np.asarray(perm, dtype=np.intp)
    if not np.array_equal(p[p], np.arange(ms)):
        return False
    rows = np.arange(A.shape[0])
    k = np.argmax(np.abs(A) ** 2, axis=1)
    ak, apk = A[rows, k], A[rows, p[k]]
    d = np.conj(A) * apk[:, None] - np.conj(ak)[:, None] * A[:, p]
    return bool(np.all(np.abs(d) <= TOL * (np.abs(ak) ** 2)[:, None]))


def derive_perm(table, ms):
    """The involution by brute force (small tables only): every candidate perm(0) = j0 fixes perm(i) as the j with
    conj(a_i) a_j0 == conj(a_0) a_j on every bin."""
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)[:, :ms]
    s = _scale(A)
    for j0 in range(ms):
        p = []
        for i in range(ms):
            d = np.conj(A[:, i:i + 1]) * A[:, j0:j0 + 1] - np.conj(A[:, :1]) * A      # (res, j)
            ok = np.all(np.abs(d) <= TOL * s[:, None], axis=0)
            if not ok.any():
                break
            p.append(int(np.argmax(ok)))
        if len(p) == ms and fb_holds(table, ms, p):
            return np.array(p, np.uint8)
    return None


def check(table, ms, fb):
    """The mode's outcome on a table: the involution (identity without fb) or None."""
    m = np.asarray(table).shape[1]
    if ms < m and not shift_invariant(table, ms):
        return None
    if not fb:
        return np.arange(ms, dtype=np.uint8)
    return derive_perm(table, ms)


def ula(m):
    return [[i, 0] for i in range(m)]


def table_of(arr, res, freq=mo.FREQUENCY):
    return mo.steering_table_c64(arr, res, freq, mo.SPACING)


def two_emitters(batch, arr, K, angles=(40.3, 121.7), sigma=0.1, coherent=True, seed=0, freq=mo.FREQUENCY):
    """(batch, m*K) complex64 items: two unit-power emitters, the second a phase-rotated copy of the first when coherent
    (a random phase per item), else independent; complex white noise of standard deviation sigma."""
    rng = np.random.default_rng(seed)
    m = len(arr)
    lam = mo.C_LIGHT / freq
    scaled = mo.scaled_array(arr, mo.SPACING)
    a1, a2 = mo.steer(angles[0], scaled, lam), mo.steer(angles[1], scaled, lam)
    cg = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2.0)
    s1 = cg(batch, K)
    s2 = s1 * np.exp(1j * rng.uniform(0, 2 * np.pi, (batch, 1))) if coherent else cg(batch, K)
    x = s1[:, :, None] * a1[None, None, :] + s2[:, :, None] * a2[None, None, :] + sigma * cg(batch, K, m)
    return x.reshape(batch, K * m).astype(np.complex64)


def fold(deg):
    """A ULA's spectrum is mirrored about 0/180 degrees."""
    d = np.mod(deg, 360.0)
    return np.minimum(d, 360.0 - d)


def both_found(ang_row, angles=(40.3, 121.7), tol=2.0):
    f = fold(np.asarray(ang_row, dtype=np.float64))
    return all(np.any(np.abs(f - fold(a)) <= tol) for a in angles)


def success_rate(ang, angles=(40.3, 121.7)):
    return float(np.mean([both_found(a, angles) for a in ang]))


def picked(spec, npeaks=4):
    """mo.peak_pick of every spectrum row: (B, npeaks) angles."""
    return np.array([mo.peak_pick(s, npeaks)[0] for s in np.asarray(spec, dtype=np.float32)])
