"""Scenes whose spectrum holds EXACT ties, infinities, fewer bins than list entries or plateaus, each with a known answer under the
reference's insertion rule (lib/baz_music_doa.cc:95,129-141: strict '>' over ascending bins), for the top-n tests (numpy only).

A tied table is a base steering table of P bins repeated c times: res = P c and every strength occurs at b, b + P, ...  The copies
are the same table row, so they tie bit for bit in the oracle (tests/test_topn_scenes.py asserts it) and in any kernel whose value
depends on the row alone.  The expected list is oracle.music_oracle.top_n_insertion of the oracle's fp64 strengths, and it is compared
EXACTLY: which bin wins is the point.  So that the answer cannot depend on rounding, every scene satisfies a separation condition on
EVERY item (no item is skipped; the seeds below were found by a one-off search on the CPU and are committed, not searched again):

    sort the strengths of one period in descending order; among the first ceil(n / c) + 1 of them (all that can reach the list, and
    the first that cannot) neighbours differ by at least SEPARATION = 1e-3 relative.

1e-3 is 50 times the suite's tie tolerance (helpers.TIE_RTOL = 2e-5) and about 700 times the int8 scan's 1.5e-6.  The other scene
kinds state their own form of the same condition (gap() below).  Arrays have m >= 3: a two-element array is a line whose mirror bins
tie in the oracle itself.

Scene kinds (make(name) returns a Scene; NAMES lists what exists):
    tied-m<m>-n<n>        TIED: (m, n) -> (K, P, c, seed)
    widekey               res = 69,632: [base(4096) | one dull row 61,440 times | base(4096)]; the list is [b, b + 65,536], so the
                          second bin has bit 16 set (the 20-bit bin field of the key); the long stretch is a plateau of equal values
    zero-m<m>[-r<rows>]   res = 64 with all-zero table rows: d = 0 there, the reference inserts +inf (tests/test_oracle.py)
    allzero-m<m>          an all-zero table: every strength is +inf, the list is bins 0 .. n-1
    short-m<m>-n<n>       fewer bins than list entries: all res bins in descending strength, then (0, 0) pairs
    plateau-<kind>-m<m>   for the local-maximum picker: `pairs` (np.repeat(base, 2): every value a two-bin plateau), `wrapped` (the
                          same rolled by one row: the plateau of base bin 0 occupies bins res-1 and 0) and `constant` (one row
                          repeated: no peak at all)
"""
import functools

import numpy as np

from oracle import music_oracle as mo

SEPARATION = 1e-3
BATCH = 33                      # more than one 16-item row group, ragged

# (m, n) -> (K, P, c, seed)
TIED = {
    (4, 3): (64, 16, 4, 7),
    (4, 2): (64, 80, 4, 6),
    (3, 1): (32, 48, 3, 7),
    (8, 2): (32, 80, 4, 6),
    (6, 4): (32, 48, 3, 7),
    (16, 2): (32, 80, 4, 6),
    (11, 3): (32, 48, 3, 3),
    (9, 1): (32, 48, 3, 7),
    (6, 5): (32, 48, 4, 1),
    (8, 7): (20, 24, 4, 4),
    (13, 12): (32, 32, 4, 8),
    (16, 15): (32, 24, 5, 8),
    (20, 9): (24, 40, 3, 5),
    (18, 3): (32, 60, 2, 6),
}
WIDEKEY = dict(m=3, n=2, K=32, P=4096, res=69632, batch=3, seed=4)
# name -> (m, n, K, zero rows, seed); res = 64
ZERO_RES = 64
ZERO = {
    "zero-m4": (4, 3, 64, (5, 40), 7),
    "zero-m8": (8, 2, 32, (5, 40), 1),
    "zero-m8-r40": (8, 2, 32, (40,), 6),
    "zero-m18": (18, 3, 32, (5, 40), 6),
}
ALLZERO = {"allzero-m4": (4, 3, 64), "allzero-m8": (8, 2, 32), "allzero-m18": (18, 3, 32)}      # (m, n, K)
# (m, n) -> (res, K, seed)
SHORT = {(8, 7): (3, 32, 11), (16, 15): (7, 32, 9), (4, 3): (2, 32, 1), (6, 4): (3, 32, 2), (20, 19): (5, 32, 8)}
# m -> (n, K, P, seed); the first emitter stands at 0 degrees, base bin 0.  (m = 4: an odd P, so that no bin stands at 180 degrees --
# on the unit square that row equals the row of 0 degrees and the two peaks would tie.)
PLATEAU = {4: (2, 64, 41, 3), 8: (3, 32, 40, 8)}
PLATEAU_KINDS = ("pairs", "wrapped", "constant")


class Scene:
    """table (res, m) complex64, items (B, m K) complex64, strength (B, res) fp64 of the oracle, ang / lvl (B, n): the expected
    list (ang float32 as every path reports it, lvl fp64), period / copies of a tied table (else res / 1)"""

    def __init__(self, name, m, n, K, table, items, period=None):
        self.name, self.m, self.n, self.K = name, m, n, K
        self.table, self.items = table, items
        self.res = table.shape[0]
        self.period = self.res if period is None else period
        self.copies = self.res // self.period
        _, _, self.spec32, self.strength = mo.music_doa_work_batch(items, table, m, n)
        ang = np.zeros((items.shape[0], n), np.float64)
        self.lvl = np.zeros((items.shape[0], n), np.float64)
        for b in range(items.shape[0]):
            ang[b], self.lvl[b] = mo.top_n_insertion(self.strength[b], n, self.res)
        self.ang = ang.astype(np.float32)
        self.bins = np.rint(ang * self.res / 360.0).astype(np.int64)
        for a in (self.table, self.items, self.strength, self.spec32, self.ang, self.lvl, self.bins):
            a.setflags(write=False)

    @property
    def nsamples(self):
        return self.m * self.K


def base_table(m, P):
    return mo.steering_table_c64(mo.array_geometry(m), P, mo.FREQUENCY, mo.SPACING)


def short_table(m, res):
    """The first res rows of the (2 res + 1)-bin table.  Not the res-bin table: bins 180 degrees apart hold conjugate rows, and on the
    unit square the rows of 0 and 180 degrees are one real vector, so the two-bin table of m = 4 ties in the oracle itself."""
    return base_table(m, 2 * res + 1)[:res].copy()


def seeded_items(m, n, K, seed, batch=BATCH, angles=None):
    if angles is None:
        angles = np.random.default_rng(seed).uniform(0, 360, n)
    return mo.synth_items(batch, m, m * K, mo.array_geometry(m), mo.FREQUENCY, mo.SPACING, angles_deg=tuple(float(a) for a in angles),
                          snr_db=20.0, seed=seed)


def descending_gaps(values, count):
    """(B,) the smallest relative difference between neighbours among the `count` largest values of every row (inf where count < 2)"""
    v = np.sort(np.asarray(values, dtype=np.float64), axis=1)[:, ::-1][:, :count]
    if v.shape[1] < 2:
        return np.full(v.shape[0], np.inf)
    return ((v[:, :-1] - v[:, 1:]) / v[:, :-1]).min(axis=1)


def tied_names():
    return ["tied-m%d-n%d" % s for s in TIED]


def short_names():
    return ["short-m%d-n%d" % s for s in SHORT]


def plateau_names():
    return ["plateau-%s-m%d" % (k, m) for m in PLATEAU for k in PLATEAU_KINDS]


NAMES = tied_names() + ["widekey"] + list(ZERO) + list(ALLZERO) + short_names() + plateau_names()


def _shape(name):
    p = name.split("-")
    return int(p[1][1:]), int(p[2][1:])


def plateau_base(m):
    """(base table (P, m), items) of the plateau scenes of an antenna count"""
    n, K, P, seed = PLATEAU[m]
    angles = np.concatenate([[0.0], np.random.default_rng(seed).uniform(40.0, 320.0, n - 1)])
    return base_table(m, P), seeded_items(m, n, K, seed, angles=angles)


@functools.lru_cache(maxsize=None)
def make(name):
    """The scene of a name, computed once and shared: nothing may write to it (its arrays are read-only)."""
    kind = name.split("-")[0]
    if kind == "tied":
        m, n = _shape(name)
        K, P, c, seed = TIED[(m, n)]
        return Scene(name, m, n, K, np.tile(base_table(m, P), (c, 1)), seeded_items(m, n, K, seed), period=P)
    if kind == "widekey":
        w = WIDEKEY
        base = base_table(w["m"], w["P"])
        items = seeded_items(w["m"], w["n"], w["K"], w["seed"], batch=w["batch"])
        s0 = mo.music_doa_work_batch(items, base, w["m"], w["n"])[3]
        dull = int(np.argmin(s0.max(axis=0)))                       # the base bin with the lowest maximum strength over the batch
        table = np.concatenate([base, np.repeat(base[dull:dull + 1], 65536 - w["P"], axis=0), base])
        assert table.shape[0] == w["res"]
        return Scene(name, w["m"], w["n"], w["K"], table, items)
    if kind == "zero":
        m, n, K, rows, seed = ZERO[name]
        table = base_table(m, ZERO_RES)
        table[list(rows)] = 0
        return Scene(name, m, n, K, table, seeded_items(m, n, K, seed))
    if kind == "allzero":
        m, n, K = ALLZERO[name]
        return Scene(name, m, n, K, np.zeros((ZERO_RES, m), np.complex64), seeded_items(m, n, K, 1))
    if kind == "short":
        m, n = _shape(name)
        res, K, seed = SHORT[(m, n)]
        return Scene(name, m, n, K, short_table(m, res), seeded_items(m, n, K, seed))
    if kind == "plateau":
        m = int(name.split("-")[2][1:])
        base, items = plateau_base(m)
        which = name.split("-")[1]
        if which == "constant":
            table = np.repeat(base[:1], 2 * base.shape[0], axis=0)
        else:
            table = np.repeat(base, 2, axis=0)
            if which == "wrapped":
                table = np.roll(table, -1, axis=0)                  # base bin 0 now occupies bins res-1 and 0
        n, K, _, _ = PLATEAU[m]
        return Scene(name, m, n, K, table, items)
    raise KeyError(name)


def zero_rows(name):
    return ZERO[name][3]


def gap(scene):
    """(B,) the separation of every item of a scene, in the form its kind needs (to be >= SEPARATION; inf: nothing to separate)"""
    kind = scene.name.split("-")[0]
    s = scene.strength
    if kind == "tied":
        return descending_gaps(s[:, :scene.period], -(-scene.n // scene.copies) + 1)
    if kind == "widekey":                                           # the first base copy: its two largest values (the list holds the larger twice)
        return descending_gaps(s[:, :WIDEKEY["P"]], 2)
    if kind == "zero":                                              # the finite values that follow the infinities in the list, and the next one
        rows = zero_rows(scene.name)
        return descending_gaps(np.delete(s, rows, axis=1), max(scene.n - len(rows), 0) + 1)
    if kind == "allzero":
        return np.full(s.shape[0], np.inf)
    if kind == "short":                                             # all res values
        return descending_gaps(s, scene.res)
    raise KeyError(scene.name)


# ---- the local-maximum picker on the plateau tables ----------------------------------------------------------------------------------
def base_peaks(spec_row, n):
    """The n strongest STRICT circular local maxima of a row in which no two neighbours are equal (asserted): bins in descending
    strength.  Written independently of music_oracle.peak_pick."""
    s = np.asarray(spec_row)
    prev, nxt = np.roll(s, 1), np.roll(s, -1)
    assert np.all(s != prev)
    peaks = np.nonzero((s > prev) & (s > nxt))[0]
    return peaks[np.argsort(-s[peaks], kind="stable")][:n]


def plateau_answer(which, base_spec, n):
    """(B, n) expected bins and (B, n) whether the entry exists, from the BASE spectrum (B, P) alone: a peak of the base at bin p is the
    plateau (2p, 2p + 1) of `pairs`, reported at its first bin 2p; `wrapped` moves every bin down by one on the circle, so the
    plateau of base bin 0 is reported at bin res-1; `constant` has no peak."""
    B, P = base_spec.shape
    res = 2 * P
    bins = np.zeros((B, n), np.int64)
    used = np.zeros((B, n), bool)
    if which == "constant":
        return bins, used
    for b in range(B):
        p = base_peaks(base_spec[b], n)
        bins[b, :len(p)] = 2 * p if which == "pairs" else (2 * p - 1) % res
        used[b, :len(p)] = True
    return bins, used


def plateau_gap(base_spec, n):
    """(B,) separation among the n + 1 strongest peaks of the base spectrum"""
    out = np.full(base_spec.shape[0], np.inf)
    for b in range(base_spec.shape[0]):
        p = base_peaks(base_spec[b], n + 1)
        v = base_spec[b, p].astype(np.float64)
        if len(v) > 1:
            out[b] = ((v[:-1] - v[1:]) / v[:-1]).min()
    return out


def angles_of(bins, used, res):
    """float32 angles as every path reports them: (float)(bin 360 / res), 0 for a missing entry"""
    return np.where(used, bins.astype(np.float64) * 360.0 / float(res), 0.0).astype(np.float32)
