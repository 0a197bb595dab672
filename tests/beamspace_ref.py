"""numpy restatement of the opt-in beamspace mode (baz_music_set_beamspace, include/baz_music_hip.h): the projection
y = T^H x, the sector design, beamspace MUSIC through the oracle, and the known-answer scenes.  Test infrastructure, not the product.

The projection here is numpy's complex128 product rounded once to complex64: the library fixes the order of its fused multiply-adds,
numpy does not, so the two agree to one float32 ulp and exactly away from rounding boundaries (bound(): tests/test_beamspace.py)."""
import numpy as np

from oracle import music_oracle as mo

RES, K, ITEMS, SNR_DB, SEED = 360, 64, 16, 20.0, 5

# (m, B, first bin of the sector, bins, emitter angles in degrees): uniform circles of array_geometry, resolution 360
SCENES = [
    dict(m=32, B=16, lo=20, cnt=120, angles=(40.0, 122.0)),
    dict(m=32, B=8, lo=30, cnt=40, angles=(40.0, 62.0)),
    dict(m=24, B=8, lo=20, cnt=60, angles=(40.0, 62.0)),
    dict(m=17, B=8, lo=20, cnt=90, angles=(40.0, 62.0)),
    dict(m=64, B=16, lo=20, cnt=60, angles=(40.0, 62.0)),
]


def table_of(m, res=RES):
    return mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY, mo.SPACING)


def scene(k):
    """(table, items (ITEMS, m K) complex64, scene record) of known-answer scene k."""
    s = SCENES[k]
    m = s["m"]
    items = mo.synth_items(ITEMS, m, m * K, mo.array_geometry(m), mo.FREQUENCY, mo.SPACING, angles_deg=s["angles"], snr_db=SNR_DB,
                           seed=SEED)
    return table_of(m), items, s


def project64(T, x):
    """T^H x in complex128 for rows of m entries (x: (..., m)) -> (..., B), unrounded."""
    T = np.asarray(T, np.complex128)
    v = np.asarray(x, np.complex64).astype(np.complex128)
    return v @ T.conj()


def bound(T, x):
    """m 2^-52 sum_r |T_rb| |x_r| per output word: what any order of the 2 m products' fp64 sum stays within."""
    T = np.asarray(T, np.complex128)
    v = np.asarray(x, np.complex64).astype(np.complex128)
    return T.shape[0] * 2.0 ** -52 * (np.abs(v) @ np.abs(T))


def project(T, x, normalise=False):
    """float32(T^H x), rows optionally scaled to unit norm first: (..., B) complex64."""
    y = project64(T, x)
    if normalise:
        nu = np.sqrt(np.sum(y.real ** 2 + y.imag ** 2, axis=-1, keepdims=True))
        ok = (nu > 0) & np.isfinite(nu)
        y = np.where(ok, y / np.where(ok, nu, 1.0), 0.0)
    with np.errstate(over="ignore"):
        return y.astype(np.complex64)


def sector_covariance(table, lo, cnt):
    a = np.asarray(table, np.complex64).astype(np.complex128)[(lo + np.arange(cnt)) % len(table)]
    return a.T @ a.conj()          # sum_b a_b a_b^H


def design(table, lo, cnt, B):
    """(T (m, B) complex128, captured, eigenvalues descending) by numpy's eigh; each column's largest-modulus component (lowest index
    on ties) real and positive."""
    C = sector_covariance(table, lo, cnt)
    w, V = np.linalg.eigh(C)
    w, V = w[::-1], V[:, ::-1]
    T = V[:, :B].copy()
    for b in range(B):
        k = int(np.argmax(np.abs(T[:, b])))
        T[:, b] *= np.conj(T[k, b]) / abs(T[k, b])
    return T, float(np.sum(w[:B]) / np.sum(w)), w


def music(y, tab, B, n, peak=True):
    """The oracle on projected items y ((items, K, B) or (items, K B)) and the projected table: (ang, lvl, spectrum)."""
    y = np.asarray(y, np.complex64).reshape(len(y), -1)
    ang = np.zeros((len(y), n), np.float32)
    lvl = np.zeros((len(y), n), np.float32)
    spec = np.zeros((len(y), len(tab)), np.float32)
    for i, item in enumerate(y):
        a, l, s = mo.music_doa_work(item, tab, B, n)
        spec[i] = s
        ang[i], lvl[i] = mo.peak_pick(s, n, len(tab)) if peak else (a, l)
    return ang, lvl, spec


def beamspace_music(T, table, items, m, n, peak=True):
    """Beamspace MUSIC of items ((items, m K) complex64) by numpy alone."""
    B = np.asarray(T).shape[1]
    y = project(T, np.asarray(items, np.complex64).reshape(len(items), -1, m))
    return music(y, project(T, table), B, n, peak)


def bin_errors(ang, angles, res=RES):
    """(items,) worst circular distance in bins between the reported angles and the true ones, matched the cheaper way round."""
    b = np.asarray(ang, np.float64) * res / 360.0
    t = np.asarray(angles, np.float64) * res / 360.0

    def d(u, v):
        e = np.abs(u - v) % res
        return np.minimum(e, res - e)
    straight = np.maximum(d(b[:, 0], t[0]), d(b[:, 1], t[1]))
    crossed = np.maximum(d(b[:, 0], t[1]), d(b[:, 1], t[0]))
    return np.minimum(straight, crossed)


def mdl_orders(y, B, n_max):
    """MDL emitter counts of projected items y ((items, K B) or (items, K, B)) by order_ref (N of the criterion is K)."""
    import order_ref
    return order_ref.estimate_items(np.asarray(y, np.complex64).reshape(len(y), -1), B, n_max, "mdl")
