"""The structured scenes (tests/structured_scenes.py) are what they promise, at every shape the GPU tests use, so that those
tests neither pass vacuously nor fail because of the oracle; and the scenes of the wrong-subspace class are pinned to the
mechanism they exist to catch by a numpy restatement of the kernels' iteration.  CPU only."""
import numpy as np
import pytest

import structured_scenes as ss
from helpers import SPECTRUM_RTOL, oracle_fp64, spectrum_bound

# the solver table's shapes plus those only the wrong-subspace scenes and their controls use
ALL_SHAPES = ss.SHAPES + sorted({(m, n) for _, m, n in ss.WRONG_SUBSPACE + ss.CONTROL} - set(ss.SHAPES))


FUSED = [(4, 1, True), (4, 2, True), (4, 3, True)]


@pytest.mark.parametrize("m,n,fused", [s + (False,) for s in ALL_SHAPES] + FUSED,
                         ids=["m%d-n%d" % s for s in ALL_SHAPES] + ["m%d-n%d-K256" % s[:2] for s in FUSED])
def test_every_scene_of_a_shape_is_what_it_promises(m, n, fused):
    names = ss.scene_names(m, n)
    assert "diagonal" in names and "block_diagonal" in names and "graded" in names
    for name in names:
        table, items, K, zeros = ss.make(name, m, n, K=ss.K_FUSED, common_K=True) if fused else ss.make(name, m, n)
        assert table.dtype == np.complex64 and items.dtype == np.complex64
        assert table.shape == (ss.res_of(m), m) and items.shape == (ss.B_DEFAULT, m * K) and (K <= 80 or fused)
        R = ss.covariance(items, m)
        if zeros is not None:                                     # the promised zeros are exact, both parts
            assert zeros.any()
            assert np.all(R[:, zeros] == 0.0), name
        if name in ("real_only", "imag_only"):
            assert np.all(R.imag == 0.0), name
            assert np.all((items.imag if name == "real_only" else items.real) == 0.0)
        allow, w = ss.allowance(items, m, n)
        assert np.all(allow < 1e-6), (name, float(allow.max()))
        lam = w[:, ::-1]
        with np.errstate(divide="ignore"):
            ratio = lam[:, n - 1] / np.maximum(lam[:, n], 0.0)
        if not name.startswith("graded"):
            assert np.all(ratio >= 100.0), (name, float(ratio.min()))
        if name.startswith("diagonal"):
            d = np.sort(R[0].diagonal().real)[::-1]
            assert np.array_equal(np.sort(lam[0])[::-1], d)
            if name == "diagonal":
                assert len(set(d)) == m
            else:
                assert (n < 2 or d[0] == d[1]) and (m - n < 2 or d[n] == d[n + 1]) and d[n - 1] > d[n]
        if name == "repeated_signal":
            tol = m * 2.0 ** -52 * lam[:, :1]                       # (eigvalsh's own error)
            assert np.all(np.abs(lam[:, 0] - lam[:, 1]) <= tol[:, 0]) and np.all(np.abs(lam[:, 2:]) <= tol)
            if m & (m - 1) == 0:                                  # K = m a power of two: nothing rounds
                u, c = np.unique(np.abs(R[0]), return_counts=True)
                assert len(u) <= 2
        if name.startswith("rank_deficient"):
            Kd = n if name.endswith("noise_free") else int(name.split("K")[-1])
            assert Kd < m and np.all(np.abs(lam[:, Kd:]) <= 1e-14 * lam[:, :1])
        _, _, _, s64, _ = oracle_fp64(items, table, m, n)
        assert np.all(np.isfinite(s64)) and np.all(s64 > 0), name


@pytest.mark.parametrize("m,n", ss.MIXED, ids=["m%d-n%d" % s for s in ss.MIXED])
def test_mixed_batch_items_are_well_posed(m, n):
    table, items, kinds, K = ss.mixed_batch(m, n)
    assert items.shape[0] <= 40 and K <= 80 and {"ordinary", "structured", "zero", "nan"} == set(kinds)
    good = [i for i, k in enumerate(kinds) if k in ("ordinary", "structured")]
    allow, w = ss.allowance(items[good], m, n)
    assert np.all(allow < 1e-6)
    _, _, _, s64, _ = oracle_fp64(items[good], table, m, n)
    assert np.all(np.isfinite(s64)) and np.all(s64 > 0)


def test_decoupled_strengths_sit_where_they_say():
    for (m, n) in [(8, 2), (16, 4), (40, 2)]:
        for pos in ("first", "middle", "last"):
            j = ss.where_of(pos, m, n)[0]
            rest = [r for r in range(m) if r != j]
            for strength in ("weak", "between", "strong"):
                _, items, K, _ = ss.make("decoupled-%s-%s" % (pos, strength), m, n)
                R = ss.covariance(items, m)
                for b in range(R.shape[0]):
                    lam = np.linalg.eigvalsh(R[b][np.ix_(rest, rest)])[::-1]
                    k = len(ss.decoupled_plan(m, n, strength)[0])
                    rjj = R[b, j, j].real
                    if strength == "weak":
                        assert rjj < lam[k:].mean() / 4.0         # under the rest's noise floor (its mean noise eigenvalue)
                    elif strength == "between":
                        assert lam[k] < rjj < lam[k - 1]
                    else:
                        assert rjj > lam[0]


def test_graded_g_is_the_largest_grade_within_the_allowance():
    for (m, n) in [(4, 2), (8, 2), (16, 4), (32, 2), (64, 8)]:
        g = ss.graded_g(m, n, ss.K_DEFAULT, ss.res_of(m), ss.B_DEFAULT)
        i = ss.GRADES.index(g)
        _, items = ss.graded(m, n, ss.K_DEFAULT, ss.res_of(m), ss.B_DEFAULT, g)
        assert np.all(ss.allowance(items, m, n)[0] < 1e-6)
        if i > 0:
            _, items = ss.graded(m, n, ss.K_DEFAULT, ss.res_of(m), ss.B_DEFAULT, ss.GRADES[i - 1])
            assert not np.all(ss.allowance(items, m, n)[0] < 1e-6)


def _iteration_verdicts(name, m, n):
    """per item: (converged by the stopping rule alone, subspace error of that basis, handed back by the dominance check)"""
    _, items, K, _ = ss.make(name, m, n)
    out = []
    for R in ss.covariance(items, m):
        conv, Y, steps = ss.iterate(R, n)
        out.append((conv, ss.subspace_error(R, n, Y) if conv else None, ss.dominance_check(R, Y) if conv else None, steps))
    return out


@pytest.mark.parametrize("name,m,n", ss.WRONG_SUBSPACE, ids=["%s-m%d-n%d" % c for c in ss.WRONG_SUBSPACE])
def test_stopping_rule_alone_accepts_a_wrong_subspace(name, m, n):
    """the iteration, restated: on these scenes the basis stops moving on an invariant subspace that is not the dominant
    one (projector error 1.0), and the dominance check hands every such item back"""
    for conv, err, back, steps in _iteration_verdicts(name, m, n):
        assert conv and steps <= 8, (conv, steps)
        assert err > 0.99, err
        assert back


@pytest.mark.parametrize("name,m,n", ss.CONTROL, ids=["%s-m%d-n%d" % c for c in ss.CONTROL])
def test_control_scenes_converge_to_the_dominant_subspace(name, m, n):
    for conv, err, back, steps in _iteration_verdicts(name, m, n):
        assert conv and err <= 1e-14 and not back, (conv, err, back)


def test_wrong_subspace_scenes_are_exactly_the_ones_the_table_names():
    """over every scene of every iteration shape: the stopping rule alone accepts a wrong subspace only where exact zeros keep
    the start columns away from a dominant eigenvector (a decoupled antenna; a diagonal R; a block the first n columns do not touch), the
    dominance check hands back every such item and none that converged to the right subspace; every scene of the table is
    among them and no control is"""
    wrong = set()
    for (m, n) in ss.LDS_ITER + [s for s in ss.WIDE if s[1] <= 4]:
        for name in ss.scene_names(m, n):
            for conv, err, back, steps in _iteration_verdicts(name, m, n):
                if not conv:
                    continue
                if err > 1e-9:
                    assert err > 0.5 and back, (name, m, n, err, back)
                    wrong.add((name, m, n))
                else:
                    assert not back, (name, m, n, err)
    assert wrong and all(name.startswith(("decoupled", "diagonal", "block_diagonal")) for name, _, _ in wrong), sorted(wrong)
    for c in ss.WRONG_SUBSPACE:
        if (c[1], c[2]) in ss.SHAPES and c[0] in ss.scene_names(c[1], c[2]):
            assert c in wrong, c
    for c in ss.CONTROL:
        assert c not in wrong
