"""numpy restatement of the opt-in sub-bin angle refinement (baz_music_set_refine_mode, include/baz_music_hip.h):
a parabola through the MUSIC denominator d = ||G^H a||^2 at a reported bin b and its two neighbours on the circle.

    y-, y0, y+ = d at bins b - 1, b, b + 1 (mod res), fp64;   p = y- - y0,  q = y+ - y0
    delta = (p - q) / (2 (p + q))   if p >= 0, q >= 0, p + q > 0 and the three values are finite,   else 0
    ang   = (float)(((b + delta) mod res) * 360 / res) in fp64, a result that rounds to 360.0f stored as 0.0f

Every operation is one IEEE fp64 operation in the order written (nothing can contract into an FMA), so the library's routine
(baz_music_refine_estimate, the text the kernel calls) must agree bit for bit.
"""
import numpy as np

from helpers import RCP_ULPS, ULP32, spectrum_bound


def delta(y3):
    """Offsets in bins for rows (d(b-1), d(b), d(b+1)); float64 array, |delta| <= 1/2."""
    y = np.asarray(y3, dtype=np.float64).reshape(-1, 3)
    ym, y0, yp = y[:, 0], y[:, 1], y[:, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = ym - y0
        q = yp - y0
        s = p + q
        r = (p - q) / (2.0 * s)
        ok = np.isfinite(y).all(axis=1) & (p >= 0.0) & (q >= 0.0) & (s > 0.0) & np.isfinite(r)
    return np.where(ok, r, 0.0)


def angle(bins, deltas, res):
    """float32 angles of bins moved by deltas: fp64 throughout, one turn added below 0, 360.0f -> 0.0f."""
    t = np.asarray(bins, dtype=np.float64) + np.asarray(deltas, dtype=np.float64)
    t = np.where(t < 0.0, t + float(res), t)
    a = (t * 360.0 / float(res)).astype(np.float32)
    return np.where(a >= np.float32(360.0), np.float32(0.0), a)


def bins_of(ang, res):
    """The bins behind grid angles (float)(b * 360 / res): exact up to 2^20 bins."""
    return np.rint(np.asarray(ang, dtype=np.float64) * res / 360.0).astype(np.int64) % res


def triples(d, bins):
    """d: (B, res) fp64 denominators, bins: (B, n) -> (B, n, 3) values at b - 1, b, b + 1 on the circle."""
    d = np.asarray(d, dtype=np.float64)
    B, res = d.shape
    bins = np.asarray(bins, dtype=np.int64)
    rows = np.arange(B)[:, None]
    return np.stack([d[rows, (bins - 1) % res], d[rows, bins], d[rows, (bins + 1) % res]], axis=2)


def refine(d, ang, present, res):
    """Mode 1 applied to mode-0 outputs: d (B, res) fp64, ang (B, n) grid angles, present (B, n) bool (a missing entry is
    (0, 0) and stays).  Returns (ang32 (B, n), delta (B, n))."""
    ang = np.asarray(ang, dtype=np.float32)
    bins = bins_of(ang, res)
    dl = delta(triples(d, bins)).reshape(bins.shape)
    dl = np.where(present, dl, 0.0)
    out = np.where(dl != 0.0, angle(bins, dl, res), ang)
    return out.astype(np.float32), dl


def tolerance(path_m, n, table, strength64, w, bins):
    """Per-entry allowance on delta against this restatement applied to the oracle's fp64 d (derivation: DESIGN.md 8d).
    t = the fp64 path's relative bound on d without the float32 reciprocal term (nothing here is rounded to float);
    E = t- y- + t+ y+ + 2 t0 y0 bounds the error of p + q and of p - q; first-order propagation through delta with
    |delta| <= 1/2 gives |d delta| <= E / (p + q), doubled for the second order.  Returns (tol (B, n), either (B, n) bool: entries
    whose p or q is within E of 0, which may take either branch)."""
    m = path_m
    s64 = np.asarray(strength64, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / s64
        t = spectrum_bound("fp64", m, n, table, s64, w) - RCP_ULPS * ULP32
        y = triples(d, bins)
        tt = triples(t, bins)
        E = tt[..., 0] * y[..., 0] + tt[..., 2] * y[..., 2] + 2.0 * tt[..., 1] * y[..., 1]
        p = y[..., 0] - y[..., 1]
        q = y[..., 2] - y[..., 1]
        tol = 2.0 * E / (p + q)
    either = np.minimum(np.abs(p), np.abs(q)) <= E
    return tol, either


def angle_error_deg(ang, truth_deg):
    """Signed error of each angle against the nearer of the true angles, in (-180, 180]."""
    a = np.asarray(ang, dtype=np.float64)[..., None]
    e = (a - np.asarray(truth_deg, dtype=np.float64) + 180.0) % 360.0 - 180.0
    k = np.argmin(np.abs(e), axis=-1)
    return np.take_along_axis(e, k[..., None], axis=-1)[..., 0]
