"""numpy restatement of the opt-in wideband (subband) mode (baz_music_set_subbands, include/baz_music_hip.h): the twiddles,
the channeliser, the two combine rules, the pickers on the combined row, the helper's bin selection, and the wideband known-answer
scenes.  Test infrastructure, not the product.

The channeliser here runs the header's chain word for word (math.fma where the interpreter has it, exact rational arithmetic rounded
once per step otherwise), on the twiddles the library reports: the definition is in terms of the W in force."""
import math
from fractions import Fraction

import numpy as np

from oracle import music_oracle as mo

C_LIGHT = mo.C_LIGHT
RES, ITEMS, SNR_DB, SEED, OCC = 360, 16, 20.0, 5, 0.375
FS_OVER_FC = 0.4

# the known-answer scenes: uniform circles of array_geometry at half-wavelength spacing, two or three uncorrelated emitters that fill
# 75 % of the sampled band, sample rate 0.4 x carrier
SCENES = [
    dict(m=8, n=2, K=256, F=8, angles=(40.0, 62.0)),
    dict(m=4, n=2, K=512, F=8, angles=(40.0, 122.0)),
    dict(m=16, n=3, K=512, F=16, angles=(40.0, 52.0, 200.0)),
]


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def twiddles(F, bins):
    """W (S, F) complex128 in extended precision, rounded once: exp(-2 pi i ((k_s t) mod F) / F) / sqrt(F), the quarter points exact."""
    ld = np.longdouble
    W = np.zeros((len(bins), F), np.complex128)
    scale = ld(1) / np.sqrt(ld(F))
    two_pi = 2 * np.arctan2(ld(0), ld(-1))
    for s, k in enumerate(bins):
        for t in range(F):
            j = (int(k) * t) % F
            if (4 * j) % F == 0:
                re, im = [(1, 0), (0, -1), (-1, 0), (0, 1)][4 * j // F]
                re, im = ld(re) * scale, ld(im) * scale
            else:
                ph = two_pi * ld(j) / ld(F)
                re, im = np.cos(ph) * scale, -np.sin(ph) * scale
            W[s, t] = complex(float(re), float(im))
    return W


if hasattr(math, "fma"):
    _fma = math.fma
else:
    def _fma(a, b, c):
        """fl64(a b + c) with one rounding, for finite operands (anything else: IEEE's plain result, which is the fused one's too)."""
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
            return a * b + c
        v = Fraction(a) * Fraction(b) + Fraction(c)
        if v == 0:
            return a * b + c                     # (the sign of an exact zero: the unfused form gives the same)
        return float(v)


def channelise(W, x):
    """The channeliser of the header, word for word.  W: (S, F) complex128; x: (..., F, m) complex64 -> (S, ..., m) complex64."""
    W = np.asarray(W, np.complex128)
    x = np.asarray(x, np.complex64)
    S, F = W.shape
    lead, m = x.shape[:-2], x.shape[-1]
    xb = x.reshape(-1, F, m)
    out = np.zeros((S, len(xb), m), np.complex64)
    with np.errstate(over="ignore"):
        for s in range(S):
            for b in range(len(xb)):
                for r in range(m):
                    re = im = 0.0
                    for t in range(F):
                        wr, wi = float(W[s, t].real), float(W[s, t].imag)
                        xr, xi = float(xb[b, t, r].real), float(xb[b, t, r].imag)
                        re = _fma(wr, xr, re)
                        re = _fma(-wi, xi, re)
                        im = _fma(wr, xi, im)
                        im = _fma(wi, xr, im)
                    out[s, b, r] = np.complex64(complex(np.float32(re), np.float32(im)))
    return out.reshape((S,) + lead + (m,))


def channelise_items(W, items, m):
    """items (batch, m K) complex64 -> (S, batch, m Q) complex64, the device layout [s][item][q][r], by the LIBRARY's host routine."""
    from gr_baz_amd import capi
    F = np.asarray(W).shape[1]
    items = np.asarray(items, np.complex64)
    y = capi.subband_apply(W, items.reshape(len(items), -1, F, m))        # (S, batch, Q, m)
    return y.reshape(y.shape[0], len(items), -1)


def combine(P, arithmetic=False):
    """P (S, ...) float32 -> float32: S / sum_s 1 / P_s, or (sum_s P_s) / S; fp64 sums from +0 with s ascending, one division."""
    P = np.asarray(P, np.float32).astype(np.float64)
    acc = np.zeros(P.shape[1:], np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(len(P)):
            acc = acc + (P[s] if arithmetic else 1.0 / P[s])
        out = acc / float(len(P)) if arithmetic else float(len(P)) / acc
        return out.astype(np.float32)


def top_n(row, n, res=None):
    """The reference's top-n rule on one float32 row: (ang, lvl) float32, lvl the stored word itself."""
    row = np.asarray(row, np.float32)
    res = len(row) if res is None else res
    ang, lvl = mo.top_n_insertion(row.astype(np.float64), n, res)
    return ang.astype(np.float32), lvl.astype(np.float32)


def pick(rows, n, peak):
    """(ang, lvl) (items, n) float32 of combined rows (items, res) under peak mode `peak`."""
    rows = np.asarray(rows, np.float32)
    ang = np.zeros((len(rows), n), np.float32)
    lvl = np.zeros((len(rows), n), np.float32)
    for i, row in enumerate(rows):
        ang[i], lvl[i] = mo.peak_pick(row, n) if peak else top_n(row, n)
    return ang, lvl


# ---- the helper's rule ----------------------------------------------------------------------------------------------------------------

def offset(k, F):
    """o(k): k below ceil(F / 2), k - F from there on."""
    return k if k < (F + 1) // 2 else k - F


def used_bins(F, occupied=0.75):
    """All k with |o(k)| / F <= occupied / 2, ascending."""
    return [k for k in range(F) if abs(offset(k, F)) / F <= occupied / 2]


def wavelengths(frequency, sample_rate, F, bins):
    return [C_LIGHT / (frequency + offset(k, F) * sample_rate / F) for k in bins]


def tables(m, frequency, sample_rate, F, bins, res=RES, spacing=mo.SPACING):
    """(S, res, m) complex64: the helper formula at each used subband's own wavelength."""
    arr = mo.scaled_array(mo.array_geometry(m), spacing)
    return np.stack([np.array(mo.calculate_antenna_array_response(arr, res, l), np.complex128).astype(np.complex64)
                     for l in wavelengths(frequency, sample_rate, F, bins)])


# ---- known answers --------------------------------------------------------------------------------------------------------------------

def synth_wideband(batch, m, K, arr_scaled, fc, fs, angles, snr_db, seed, occ):
    rng = np.random.default_rng(seed)
    p = np.asarray(arr_scaled)
    nu = np.fft.fftfreq(K) * fs
    band = np.abs(nu) <= occ * fs
    x = np.zeros((batch, K, m), complex)
    for th in angles:
        u = np.array([np.cos(np.deg2rad(th)), np.sin(np.deg2rad(th))])
        tau = (p @ u) / C_LIGHT
        s = (rng.standard_normal((batch, K)) + 1j * rng.standard_normal((batch, K))) / np.sqrt(2)
        S = np.fft.fft(s, axis=1) * band[None, :] / np.sqrt(band.mean())
        x += np.fft.ifft(S[:, :, None] * np.exp(-2j * np.pi * (fc + nu)[None, :, None] * tau[None, None, :]), axis=1)
    x += 10 ** (-snr_db / 20) * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) / np.sqrt(2)
    return x.reshape(batch, K * m).astype(np.complex64)


_SCENES = {}


def scene(k):
    """(items (ITEMS, m K) complex64, centre table, bins, subband tables (S, RES, m), scene record) of known-answer scene k; computed
    once, not to be written to."""
    if k not in _SCENES:
        s = SCENES[k]
        m, F = s["m"], s["F"]
        fc = mo.FREQUENCY
        fs = FS_OVER_FC * fc
        arr = mo.scaled_array(mo.array_geometry(m), mo.SPACING)
        items = synth_wideband(ITEMS, m, s["K"], arr, fc, fs, s["angles"], SNR_DB, SEED, OCC)
        bins = used_bins(F, 2 * OCC)
        centre = mo.steering_table_c64(mo.array_geometry(m), RES, fc, mo.SPACING)
        tabs = tables(m, fc, fs, F, bins)
        for a in (items, centre, tabs):
            a.setflags(write=False)
        _SCENES[k] = (items, centre, bins, tabs, s)
    return _SCENES[k]


def music_rows(items, table, m, n):
    """The oracle's float32 MUSIC spectrum of every item: (items, res)."""
    return np.stack([mo.music_doa_work(it, table, m, n)[2] for it in items])


def exact_hits(ang, angles, res=RES):
    """How many items report exactly the emitters' bins (as a set)."""
    want = sorted(int(round(a * res / 360.0)) for a in angles)
    got = np.rint(np.asarray(ang, np.float64) * res / 360.0).astype(int)
    return int(sum(sorted(row.tolist()) == want for row in got))
