"""The top-n scenes (tests/topn_scenes.py) are what they promise, for every item of every committed scene, so that the exact
comparisons of tests/test_topn_rule_gpu.py neither pass vacuously nor fail because of the oracle: the copies of a tied table tie bit
for bit, the separation condition holds with no item excluded, the insertion rule and its vectorised form agree (infinities
included), the wide-key scene selects a bin with bit 16 set, and the local-maximum picker's definition gives the pinned answers on
the plateau tables.  CPU only."""
import numpy as np
import pytest

import topn_scenes as ts
from oracle import music_oracle as mo

LIST_SCENES = [n for n in ts.NAMES if not n.startswith("plateau")]


def _fast(scene):
    ang = np.zeros_like(scene.lvl)
    lvl = np.zeros_like(scene.lvl)
    for b in range(scene.items.shape[0]):
        ang[b], lvl[b] = mo.top_n_fast(scene.strength[b], scene.n, scene.res)
    return ang.astype(np.float32), lvl


@pytest.mark.parametrize("name", LIST_SCENES)
def test_scene_is_separated_and_both_forms_of_the_rule_agree(name):
    s = ts.make(name)
    assert s.m >= 3 and s.table.dtype == np.complex64 and s.items.dtype == np.complex64
    assert s.items.shape == ((ts.WIDEKEY["batch"] if name == "widekey" else ts.BATCH), s.m * s.K) and s.table.shape == (s.res, s.m)
    assert not np.isnan(s.strength).any() and np.all(s.strength > 0)
    g = ts.gap(s)
    assert g.shape == (s.items.shape[0],)                           # every item, none skipped
    assert np.all(g >= ts.SEPARATION), (name, float(g.min()))
    fa, fl = _fast(s)
    assert np.array_equal(fa, s.ang) and np.array_equal(fl, s.lvl)  # (inf == inf)
    assert np.all(s.lvl[:, :-1] >= s.lvl[:, 1:])
    for b in range(s.items.shape[0]):                               # lvl is the strength at the bin; (0, 0) where nothing was inserted
        used = s.lvl[b] > 0
        assert np.array_equal(s.lvl[b][used], s.strength[b][s.bins[b][used]])
        assert np.all(s.ang[b][~used] == 0.0)


@pytest.mark.parametrize("name", ts.tied_names())
def test_copies_of_a_period_tie_bit_for_bit(name):
    s = ts.make(name)
    P, c = s.period, s.copies
    assert c >= 2 and s.res == P * c
    for k in range(1, c):
        assert np.array_equal(s.strength[:, :P].view(np.uint64), s.strength[:, k * P:(k + 1) * P].view(np.uint64))
        assert np.array_equal(s.table[:P], s.table[k * P:(k + 1) * P])
    # the list: whole groups of copies in bin order, then the first copies of the next value
    order = np.argsort(-s.strength[:, :P], axis=1, kind="stable")
    for b in range(s.items.shape[0]):
        want = [order[b, i // c] + P * (i % c) for i in range(s.n)]
        assert s.bins[b].tolist() == want, (name, b)
    assert np.all(s.lvl > 0)


def test_wide_key_scene_selects_a_bin_with_bit_16_set():
    s = ts.make("widekey")
    w = ts.WIDEKEY
    assert s.res == w["res"] > 65536
    assert np.all(s.bins[:, 0] < w["P"]) and np.array_equal(s.bins[:, 1], s.bins[:, 0] + 65536)
    assert np.all(s.bins[:, 1] >= 65536) and np.all((s.bins[:, 1] >> 16) & 1 == 1)
    assert np.array_equal(s.strength[:, :w["P"]], s.strength[:, 65536:])
    plateau = s.strength[:, w["P"]:65536]
    assert np.all(plateau == plateau[:, :1])                         # 61,440 equal values ...
    assert np.all(plateau[:, 0] < 1e-3 * s.lvl[:, 0])                # ... far below the peak


@pytest.mark.parametrize("name", list(ts.ZERO))
def test_zero_rows_give_infinite_strengths_that_lead_the_list(name):
    s = ts.make(name)
    rows = list(ts.zero_rows(name))
    assert np.all(np.isinf(s.strength[:, rows])) and np.all(np.isfinite(np.delete(s.strength, rows, axis=1)))
    k = min(len(rows), s.n)
    assert np.all(s.bins[:, :k] == np.asarray(rows[:k])[None, :]) and np.all(np.isinf(s.lvl[:, :k]))
    assert np.all(np.isfinite(s.lvl[:, k:])) and np.all(s.lvl[:, k:] > 0)
    rest = np.delete(np.arange(s.res), rows)
    if s.n > k:
        assert np.array_equal(s.bins[:, k], rest[np.argmax(s.strength[:, rest], axis=1)])


@pytest.mark.parametrize("name", list(ts.ALLZERO))
def test_all_zero_table_gives_the_first_n_bins(name):
    s = ts.make(name)
    assert not s.table.any() and np.all(np.isinf(s.strength))
    assert np.all(s.bins == np.arange(s.n)[None, :]) and np.all(np.isinf(s.lvl))


@pytest.mark.parametrize("name", ts.short_names())
def test_short_tables_fill_the_list_with_zero_pairs(name):
    s = ts.make(name)
    assert s.res < s.n
    order = np.argsort(-s.strength, axis=1, kind="stable")
    assert np.array_equal(s.bins[:, :s.res], order)
    assert np.all(s.ang[:, s.res:] == 0.0) and np.all(s.lvl[:, s.res:] == 0.0) and np.all(s.lvl[:, :s.res] > 0)


@pytest.mark.parametrize("m", sorted(ts.PLATEAU))
def test_peak_picker_definition_on_the_plateau_tables(m):
    """first bin of a plateau, bin res-1 for the plateau that wraps, (0, 0) throughout for the constant row"""
    n, K, P, _ = ts.PLATEAU[m]
    base, items = ts.plateau_base(m)
    base_spec = mo.music_doa_work_batch(items, base, m, n)[2]
    assert np.all(ts.plateau_gap(base_spec, n) >= ts.SEPARATION)
    first = np.array([ts.base_peaks(row, n)[0] for row in base_spec])
    assert np.all(first == 0)                                        # the emitter at 0 degrees is every item's strongest peak
    for which in ts.PLATEAU_KINDS:
        s = ts.make("plateau-%s-m%d" % (which, m))
        res = s.res
        assert res == 2 * P and np.array_equal(s.items, items)
        bins, used = ts.plateau_answer(which, base_spec, n)
        want_ang = ts.angles_of(bins, used, res)
        if which == "constant":
            assert np.all(s.spec32 == s.spec32[:, :1]) and not used.any()
        else:
            pairs = s.spec32 if which == "pairs" else np.roll(s.spec32, 1, axis=1)
            assert np.array_equal(pairs[:, 0::2], base_spec) and np.array_equal(pairs[:, 1::2], base_spec)
            assert used.all()                                        # n peaks in every item
            assert np.all(bins[:, 0] == (0 if which == "pairs" else res - 1))
            if which == "pairs":
                assert np.all(bins % 2 == 0)
        for b in range(items.shape[0]):
            a, l = mo.peak_pick(s.spec32[b], n)
            assert np.array_equal(a, want_ang[b]), (which, b)
            assert np.array_equal(l, np.where(used[b], s.spec32[b][bins[b]], np.float32(0.0)))
