"""The fractional resampler's phase walk held to two integer models (tests/resamp_phase_ref.py).

X87Walk is the reference's recurrence with every long double operation rounded to a 64-bit significand; FixedWalk is the
library's 64.64 closed form with its `exact` flag.  On the CPU: X87Walk == oracle/resamp_ref.c == the reference-source build on
every family below (output bits, consumed, mu); `exact` implies the two models are the same walk; where it is 0 their distance
stays inside the bound derived in the model's docstring.  On the GPU: the one-input kernel reads exactly FixedWalk's (ii, imu)
-- whatever the flag says -- which a probe tap table makes visible; with the default table its outputs are the oracle's wherever
the flag is 1; the two-input walk is X87Walk.

Phase exactly 1.0: the library reads row 0 at ii + 1 where the reference reads row 128 at ii.  The probe's rows carry their own
index, so it does NOT have row 128 = row 0 shifted: the probe tests hold the GPU to FixedWalk's raw (ii, imu) = (1, 0), and the
agreement with the reference at phase 1.0 is tested with the default table only (whose rows 0 and 128 are both pure delays);
model-to-model comparisons use resamp_phase_ref.canonical, which is valid for such tables.

Families (sizes are per GPU case):
  F1  double phase with a fine bit against the step width (<= 300 outputs where the ratio is >= 1024)
  F2  quotient ratios: rational pairs and ppb pairs
  F3  events between calls on a double-ratio stream
  F4  the supported edge, ratio 2^-11
  F5  the two-input walk with a float ratio per sample
"""
import ctypes
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np
import pytest

import resamp_phase_ref as pr
from oracle import resamp_ref as rr

TIE = 81 / 256 + 2.0 ** -26 + 2.0 ** -54          # (float)TIE is above the tie 40.5/128; without the 2^-54 bit it IS the tie
TIE64 = 2.5 / 128 + 2.0 ** -30 + 2.0 ** -58       # the same construction against a ratio of 64 (57 fraction bits kept)
CALLS = (1, 255, 1023, 1024, 1025, 1671)
SHORT = (1, 49, 250)                              # 300 outputs: the F1 cases with a ratio >= 1024 (<= 0.5 M input samples)
MID = (1, 255, 1023, 721)                         # 2000 outputs
EDGE53 = 2.0 ** -11 * (1 + 0x5A5A5A5A5A5A5 / 2.0 ** 52)     # 53 significant bits in [2^-11, 2^-10): last bit 2^-63

Case = namedtuple("Case", "name family phase ratio num denom calls events")


def C(name, family, phase, ratio, calls, events=(), num=0, denom=0):
    return Case(name, family, phase, ratio, num, denom, tuple(calls), tuple(events))


# events: (index of the call they precede, kind, a, b)
CASES = [
    C("f1_0.001_17.3", "F1", 0.001, 17.3, MID),
    C("f1_0.37+2^-54_1024.5", "F1", 0.37 + 2.0 ** -54, 1024.5, SHORT),
    C("f1_tie_1024", "F1", TIE, 1024.0, SHORT),
    C("f1_tie_1536", "F1", TIE, 1536.0, SHORT),
    C("f1_0.3_1023.7", "F1", 0.3, 1023.7, SHORT),             # s alternates between 10 and 11 integer bits
    C("f1_0.001_4.25", "F1", 0.001, 4.25, MID),               # stays exact
    C("f1_1.0_2.5", "F1", 1.0, 2.5, MID),
    C("f1_0.0_3.999999", "F1", 0.0, 3.999999, MID),
    C("f1_0.0_17.3", "F1", 0.0, 17.3, MID),
    C("f1_0.37_17.3", "F1", 0.37, 17.3, MID),
    C("f1_0.37_0.0123", "F1", 0.37, 0.0123, MID),
    C("f2_1/3", "F2", 0.2, 0.0, CALLS, num=1, denom=3),
    C("f2_147/160", "F2", 0.2, 0.0, CALLS, num=147, denom=160),
    C("f2_160/147", "F2", 0.2, 0.0, CALLS, num=160, denom=147),
    C("f2_1000000007/1e9", "F2", 0.0, 0.0, CALLS, num=1000000007, denom=1000000000),
    C("f2_ppb_1e9+0.5", "F2", 0.2, 1.0, CALLS, [(0, "ppb", 1000000000, 0.5)]),
    C("f2_ppb_999999985.25", "F2", 0.0, 1.0, CALLS, [(0, "ppb", 999999985, 0.25)]),
    C("f3_setmu_adjust", "F3", 0.25, 1.3, CALLS, [(1, "mu", 0.001, 0), (2, "adjust", 0.3, 0), (3, "adjust", -0.3, 0)]),
    C("f3_ratio_up", "F3", 0.25, 1.3, CALLS, [(1, "adjust", 3.7, 0), (2, "ratio", 17.3, 0), (3, "adjust", 3.7, 0),
                                              (3, "mu", 0.001, 0)]),
    C("f3_tie64", "F3", 0.0, 64.0, CALLS, [(2, "mu", TIE64, 0)]),
    C("f3_rational", "F3", 0.25, 1.3, CALLS, [(2, "rational", 147, 160), (3, "mu", 0.001, 0), (3, "adjust", 0.3, 0)]),
    C("f3_all_at_once", "F3", 0.5, 1.3, CALLS, [(1, "mu", 0.75, 0), (1, "ratio", 2.5, 0), (1, "adjust", -0.3, 0)]),
    C("f3_mu_then_ratio", "F3", 0.25, 1.3, CALLS, [(1, "mu", 0.001, 0), (3, "ratio", 2.5, 0)]),
    C("f4_1/2048", "F4", 0.37, 2.0 ** -11, CALLS),
    C("f4_53bits", "F4", 0.37, EDGE53, CALLS),
    C("f3_tie_1024", "F3", 0.0, 1024.0, CALLS, [(2, "mu", TIE, 0)]),      # 5.1 M input samples; one stream in the probe test
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
PAD = 4096                                        # input samples past the last one the walk reads


def apply_events(blk, case, i):
    for (ci, kind, a, b) in case.events:
        if ci != i:
            continue
        if kind == "mu": blk.set_mu(float(a))
        elif kind == "ratio": blk.set_resamp_ratio(float(a))
        elif kind == "adjust": blk.adjust(float(a))
        elif kind == "rational": blk.set_resamp_ratio_rational(int(a), int(b))
        elif kind == "ppb": blk.set_resamp_ratio_ppb(int(a), float(b))
        else: raise ValueError(kind)


def make(cls, case, **kw):
    return cls(case.phase, case.ratio, case.num, case.denom, **kw)


Run = namedtuple("Run", "L x87 fixed bound")     # x87 / fixed: per call (ii, imu, consumed, mu float, mu Fraction, exact, exact_old)


@functools.lru_cache(maxsize=None)
def model_run(name):
    """Both models through the case's calls and events, once per session; read-only afterwards."""
    case = BY_NAME[name]
    a = make(pr.X87Walk, case)
    xs = []
    for i, n in enumerate(case.calls):
        apply_events(a, case, i)
        ii, imu, k = a.work(n)
        xs.append((ii, imu, k, a.mu(), a.d_mu, None, None))
    L = sum(c[2] for c in xs) + PAD
    a, b = make(pr.X87Walk, case), make(pr.FixedWalk, case)
    bound = pr.PhaseBound(a, b)
    fs, bs, pos = [], [], 0
    for i, n in enumerate(case.calls):
        apply_events(a, case, i)
        apply_events(b, case, i)
        bs.append(bound.call(n))
        a.work(n)
        ii, imu, k = b.work(L - pos, n)
        assert len(ii) == n                       # the input never runs out here
        fs.append((ii, imu, k, b.mu(), b.mu_exact, b.exact, b.exact_conversion_only))
        pos += k
    for arr in xs + fs:
        arr[0].setflags(write=False), arr[1].setflags(write=False)
    return Run(L, tuple(xs), tuple(fs), tuple(bs))


def signal(L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)


def differing(x, f):
    (ia, ma), (ib, mb) = pr.canonical(x[0], x[1]), pr.canonical(f[0], f[1])
    return int(((ia != ib) | (ma != mb)).sum())


def same_walk(x, f):
    return differing(x, f) == 0 and x[2] == f[2] and x[4] == f[4]


# ------------------------------------------------------------------ CPU: X87Walk is the reference
def assert_x87_equals(cls, case):
    run = model_run(case.name)
    x = signal(run.L, 1234)
    taps = rr.taps()
    blk = make(cls, case)
    pos = 0
    for i, n in enumerate(case.calls):
        apply_events(blk, case, i)
        out, k = blk.work(x[pos:], n)
        ii, imu, kx, mu, _, _, _ = run.x87[i]
        assert k == kx and blk.mu() == mu, (case.name, i)
        want = pr.interp_f32(x[pos:], ii, imu, taps)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (case.name, i)
        pos += k


@pytest.mark.parametrize("name", IDS)
def test_x87walk_equals_the_c_restatement(name):
    """consumed, mu() and the output bits on a random input with the default table: a wrong (ii, imu) changes output bits."""
    assert_x87_equals(rr.Resampler, BY_NAME[name])


@pytest.mark.skipif(not rr.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", IDS)
def test_x87walk_equals_the_reference_source_build(name):
    assert_x87_equals(rr.RefResampler, BY_NAME[name])


def f5_ratios(L):
    """Float ratios mixing 0.75, 1.5, 9000.25 and 2^-20: pairs of 9000.25 every 1500 samples (steps of at most 1.5 visit one of
    every two samples, so each pair is hit), and 2^-20 from sample 30000 on, where the walk then stays for the rest of the run."""
    rng = np.random.default_rng(91)
    r = rng.choice(np.array([0.75, 1.5], np.float32), L)
    for j in range(700, 30000, 1500):
        r[j:j + 2] = 9000.25
    r[30000:] = 2.0 ** -20
    return r


F5_PHASE, F5_CALLS, F5_L = 0.3, (1, 255, 1023, 1024, 697), 40000


@functools.lru_cache(maxsize=None)
def f5_run():
    a = pr.X87Walk(F5_PHASE, 1.0)
    ratios = f5_ratios(F5_L)
    calls, pos = [], 0
    for n in F5_CALLS:
        ii, imu, k = a.work(n, rr=ratios[pos:])
        ii.setflags(write=False), imu.setflags(write=False)
        calls.append((ii, imu, k, a.mu(), a.resamp_ratio()))
        pos += k
    assert 30000 <= pos and pos + 8 <= F5_L       # long jumps were taken, the 2^-20 stretch was reached, the input did not run out
    assert a.sums_rounded > 0                     # mu + 9000.25 pushed bits of the phase out
    return tuple(calls)


def test_x87walk_two_input_branch_equals_the_oracles():
    ratios, x, taps = f5_ratios(F5_L), signal(F5_L, 92), rr.taps()
    blocks = [rr.Resampler(F5_PHASE, 1.0)] + ([rr.RefResampler(F5_PHASE, 1.0)] if rr.have_ref() else [])
    for blk in blocks:
        pos = 0
        for n, (ii, imu, kx, mu, ratio) in zip(F5_CALLS, f5_run()):
            out, k = blk.work(x[pos:], n, rr=ratios[pos:])
            assert k == kx and blk.mu() == mu and blk.resamp_ratio() == ratio
            assert np.array_equal(out.view(np.uint32), pr.interp_f32(x[pos:], ii, imu, taps).view(np.uint32))
            pos += k


# ------------------------------------------------------------------ CPU: the flag and the bound
def test_exact_flag_is_sound():
    """`exact` after a call implies that call (and all before it: the flag never comes back) is the reference's walk: same
    (ii, imu) up to the phase-1.0 equivalence, same consumed count, same mu as a rational number."""
    for case in CASES:
        run = model_run(case.name)
        for i, (x, f) in enumerate(zip(run.x87, run.fixed)):
            if f[5]:
                assert same_walk(x, f), (case.name, i)


def test_the_conversion_only_rule_was_not_sound():
    """The rule the library had -- exact unless a conversion to 64.64 dropped bits -- says 1 on walks that are not the reference's."""
    broken = [c.name for c in CASES
              if any(f[6] and not same_walk(x, f) for x, f in zip(model_run(c.name).x87, model_run(c.name).fixed))]
    print("conversion-only rule says exact on a different walk:", broken)
    assert set(broken) >= {"f1_0.001_17.3", "f1_0.37+2^-54_1024.5", "f1_tie_1024", "f1_tie_1536", "f1_0.3_1023.7"}


# exact == 1 at the end of the run, per family, with the corrected rule (F1: 6 of 11, F2: 0 of 6, F3: 1 of 7, F4: 2 of 2)
MIN_EXACT = {"F1": 6, "F2": 0, "F3": 1, "F4": 2}


def test_exact_flag_is_not_vacuous():
    count = {f: 0 for f in MIN_EXACT}
    for case in CASES:
        final = model_run(case.name).fixed[-1][5]
        count[case.family] += bool(final)
        if case.family == "F2":
            assert not final, case.name
    print("exact cases per family:", count)
    for fam, n in MIN_EXACT.items():
        assert count[fam] >= n, (fam, count)
    for name in ("f1_0.0_17.3", "f1_0.37_17.3", "f1_1.0_2.5", "f1_0.001_4.25", "f1_0.0_3.999999", "f1_0.37_0.0123", "f4_1/2048", "f4_53bits"):
        assert model_run(name).fixed[-1][5], name
    for name in ("f1_0.001_17.3", "f1_tie_1024"):
        assert not model_run(name).fixed[0][5], name      # already 0 after the constructor's own check and the first call
    assert not pr.FixedWalk(TIE, 1024.0).exact and not pr.FixedWalk(0.001, 17.3).exact
    assert pr.FixedWalk(0.0, 17.3).exact and pr.FixedWalk(0.37, 0.0123).exact


def test_inexact_walks_stay_inside_the_derived_bound():
    """|T_x87 - T_fixed| (T = samples consumed + mu; equal to the mu difference when the counts agree) at every call boundary
    against PhaseBound; constant double ratios also against the bound that no longer grows.  The number of outputs whose
    (ii, imu) differ is printed, not capped: the GPU is held to FixedWalk, the relation to the reference is this bound."""
    worst = {}
    for case in CASES:
        run = model_run(case.name)
        tx = tf = Fraction(0)
        ndiff, w = 0, 0.0
        for i, (x, f) in enumerate(zip(run.x87, run.fixed)):
            tx, tf = tx + x[2], tf + f[2]
            d = abs((tx + x[4]) - (tf + f[4]))
            assert d <= run.bound[i], (case.name, i, float(d), float(run.bound[i]))
            if case.family == "F1":
                assert d <= pr.constant_double_bound(case.phase, case.ratio), (case.name, i)
            w = max(w, float(d / run.bound[i]))
            ndiff += differing(x, f)
        if not run.fixed[-1][5]:
            print("%-24s outputs with another (ii, imu): %4d of %d, worst |dT| / bound %.3f" % (case.name, ndiff, sum(case.calls), w))
            worst[case.family] = max(worst.get(case.family, 0.0), w)
        else:
            assert w == 0.0 and ndiff == 0
    print("worst |dT| / bound per family:", worst)
    assert differing(model_run("f1_tie_1024").x87[2], model_run("f1_tie_1024").fixed[2]) == 250     # the issue's counterexample


def test_ratio_below_the_supported_edge_is_refused_by_both_models():
    r = 2.0 ** -11 - 2.0 ** -40
    for cls in (pr.X87Walk, pr.FixedWalk):
        with pytest.raises(pr.Unsupported):
            cls(0.0, r)
        blk = cls(0.0, 1.0)
        with pytest.raises(pr.Unsupported):
            blk.set_resamp_ratio(r)
        cls(0.0, 2.0 ** -11)


# ------------------------------------------------------------------ GPU: the kernel reads FixedWalk's (ii, imu)
def probe_table(second_pass):
    """Only tap [r][7] is non-zero -- the tap that multiplies in[ii] -- so out = in[ii] * t[r][7]: 1.0 in the first pass (out.re
    is the input index), r + 1 in the second (out.im is the row).  All finite, which is all baz_resamp_set_taps checks."""
    t = np.zeros((pr.NSTEPS + 1, pr.NTAPS), np.float32)
    t[:, 7] = np.arange(1, pr.NSTEPS + 2, dtype=np.float32) if second_pass else 1.0
    return t


def probe_input(S, L, stride):
    """x[s][i] = (s + 1) * (i, 1): exact in float32 while (s + 1) * i < 2^24; NaN beyond the L samples of each row."""
    assert S * L < 2 ** 24
    x = np.full((S, stride, 2), np.nan, np.float32)
    for s in range(S):
        x[s, :L, 0] = np.arange(L, dtype=np.float32) * (s + 1)
        x[s, :L, 1] = s + 1
    return x


def decode(out, S, pos, second_pass, ii_known=None):
    """out: (S, n, 2) float32 -> the int64[n] every stream agrees on (ii relative to `pos`, or imu); asserts exactness."""
    vals = []
    for s in range(S):
        re, im = out[s, :, 0].astype(np.float64), out[s, :, 1].astype(np.float64)
        if not second_pass:
            assert np.all(im == s + 1)
            v = re / (s + 1)
        else:
            v = im / (s + 1) - 1
            assert np.array_equal(out[s, :, 0], (np.float32(s + 1) * (ii_known + pos).astype(np.float32)) * (v + 1).astype(np.float32))
        assert np.all(v == np.rint(v))
        vals.append(v.astype(np.int64))
        assert np.array_equal(vals[s], vals[0])
    v = vals[0] - (0 if second_pass else pos)
    assert np.all(v >= 0) and (not second_pass or np.all(v <= pr.NSTEPS))
    return v


SENTINEL = np.float32(-7.0)


def hip_probe_pass(case, S, second_pass, gpu_device):
    """One fresh context through the case: first pass on the host path, second on device buffers, both with row strides larger
    than the windows.  consumed, mu() and phase_exact() against FixedWalk at every call.  -> decoded values per call."""
    import torch
    from gr_baz_amd import resamp
    run = model_run(case.name)
    L, stride = run.L, run.L + 37
    x = probe_input(S, L, stride)
    f32p = ctypes.POINTER(ctypes.c_float)
    got = []
    with make(resamp.Resampler, case, nstreams=S) as blk:
        blk.set_taps(probe_table(second_pass))
        if second_pass:
            xd = torch.from_numpy(x).to(gpu_device)
        pos = 0
        for i, n in enumerate(case.calls):
            apply_events(blk, case, i)
            ii, imu, k, mu, _, exact, _ = run.fixed[i]
            ostride = n + 5
            if not second_pass:
                out = np.full((S, ostride, 2), SENTINEL, np.float32)
                consumed = ctypes.c_uint64(0)
                r = resamp.lib().baz_resamp_process(blk._h, ctypes.cast(x[:, pos:].ctypes.data, f32p), stride, L - pos,
                                                    out.ctypes.data_as(f32p), ostride, n, ctypes.byref(consumed))
                kk = consumed.value
            else:
                od = torch.full((S, ostride, 2), float(SENTINEL), dtype=torch.float32, device=gpu_device)
                torch.cuda.synchronize()                     # the engine runs on its own stream: fills first
                r, kk = blk.process_device(xd.data_ptr() + 8 * pos, stride, L - pos, od.data_ptr(), ostride, n)
                blk.sync()
                out = od.cpu().numpy()
            assert r == n and kk == k, (case.name, i, r, kk, k)
            assert blk.mu() == mu and blk.phase_exact() == exact, (case.name, i)
            assert np.all(out[:, n:] == SENTINEL)            # nothing written past the outputs produced
            got.append(decode(out[:, :n], S, pos, second_pass, ii))
            pos += k
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_hip_reads_the_fixed_walks_rows_and_samples(name, gpu_device):
    """(ii, imu) of resamp_kernel, read out through a probe table, equal FixedWalk's bit for bit, flag or no flag."""
    case = BY_NAME[name]
    run = model_run(name)
    S = 1 if run.L > 2 ** 21 else 1 + IDS.index(name) % 3
    for second_pass in (False, True):
        got = hip_probe_pass(case, S, second_pass, gpu_device)
        for i, v in enumerate(got):
            want = run.fixed[i][1 if second_pass else 0]
            assert np.array_equal(v, want), (name, i, "imu" if second_pass else "ii", int((v != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_hip_default_table_equals_the_oracle_where_the_flag_is_set(name, gpu_device):
    """2 streams, the first 2000 outputs of the case (all its events lie there): output bits equal the C restatement's while
    phase_exact() is 1, and always equal the float32 interpolation at FixedWalk's (ii, imu).  Phase 1.0 is covered here."""
    from gr_baz_amd import resamp
    case = BY_NAME[name]
    run = model_run(name)
    calls = case.calls if sum(case.calls) <= 2000 else MID
    assert all(ci < len(calls) for (ci, _, _, _) in case.events)
    x = np.stack([signal(run.L, 55), signal(run.L, 56)])
    taps = rr.taps()
    with make(resamp.Resampler, case, nstreams=2) as blk:
        oracles = [make(rr.Resampler, case) for _ in range(2)]
        fixed = make(pr.FixedWalk, case)
        pos, seen_exact = 0, 0
        for i, n in enumerate(calls):
            for b in [blk, fixed] + oracles:
                apply_events(b, case, i)
            out, k = blk.work(x[:, pos:], n)
            ii, imu, kf = fixed.work(run.L - pos, n)
            assert out.shape == (2, n) and k == kf and blk.mu() == fixed.mu() and blk.phase_exact() == fixed.exact
            for s in range(2):
                assert np.array_equal(out[s].view(np.uint32), pr.interp_f32(x[s, pos:], ii, imu, taps).view(np.uint32))
                if blk.phase_exact():
                    o, ko = oracles[s].work(x[s, pos:], n)
                    assert ko == k and np.array_equal(out[s].view(np.uint32), o.view(np.uint32)) and blk.mu() == oracles[s].mu()
                    seen_exact += 1
            pos += k
        assert bool(seen_exact) == bool(run.fixed[0][5])


@pytest.mark.gpu
@pytest.mark.parametrize("phase,ratio,num,denom,adjust,windows", [
    (0.0, 1.5, 0, 0, None, (100, 7, 8, 9, 300)),                # 62 outputs fit in 100 samples; none in 7; one in 8
    (0.2, 0.0, 160, 147, None, (1000, 7, 1001, 50)),
    (0.37, 17.3, 0, 0, 3.7, (100, 500, 7, 72, 73, 2000)),         # the adjusted first step jumps past short windows
    (1.0, 2.5, 0, 0, None, (8, 9, 10, 200)),                    # phase 1.0: P_0 = 1, the first window of 8 holds no output
    (0.5, 2.0 ** -11, 0, 0, None, (8, 9, 7, 3000)),
])
def test_hip_end_of_input_rule_is_the_fixed_walks(phase, ratio, num, denom, adjust, windows, gpu_device):
    """Short windows: the number of outputs that fit, consumed, mu and the output bits equal FixedWalk's end-of-input rule
    (every output's 8 samples lie inside the window), call after call on the advancing input, 2 streams."""
    from gr_baz_amd import resamp
    L = sum(windows) + 64
    x = np.stack([signal(L, 61), signal(L, 62)])
    taps = rr.taps()
    with resamp.Resampler(phase, ratio, num, denom, nstreams=2) as blk:
        fixed = pr.FixedWalk(phase, ratio, num, denom)
        pos, produced = 0, []
        for w in windows:
            if adjust is not None:
                blk.adjust(adjust), fixed.adjust(adjust)
            out, k = blk.work(x[:, pos:pos + w], 5000)
            ii, imu, kf = fixed.work(w, 5000)
            assert out.shape == (2, len(ii)) and k == kf and blk.mu() == fixed.mu() and blk.phase_exact() == fixed.exact
            for s in range(2):
                assert np.array_equal(out[s].view(np.uint32), pr.interp_f32(x[s, pos:], ii, imu, taps).view(np.uint32))
            assert len(ii) == 0 or ii[-1] + 8 <= w
            pos += k
            produced.append(len(ii))
        assert 0 in produced and any(1 < p < 5000 for p in produced), produced


@pytest.mark.gpu
def test_hip_flag_for_the_named_pairs(gpu_device):
    from gr_baz_amd import resamp
    for phase, ratio, want in ((TIE, 1024.0, False), (0.001, 17.3, False), (0.0, 17.3, True), (0.37, 0.0123, True)):
        with resamp.Resampler(phase, ratio) as blk:
            assert blk.phase_exact() == want, (phase, ratio)
    with pytest.raises(resamp.ResampError) as e:
        resamp.Resampler(0.0, 2.0 ** -11 - 2.0 ** -40)
    assert e.value.code == -4                                  # BAZ_RESAMP_E_UNSUPPORTED
    with resamp.Resampler(0.0, 2.0 ** -11) as blk:
        assert blk.phase_exact()
        with pytest.raises(resamp.ResampError) as e:
            blk.set_resamp_ratio(2.0 ** -11 - 2.0 ** -40)
        assert e.value.code == -4


@pytest.mark.gpu
def test_hip_two_input_walk_is_the_x87_walk(gpu_device):
    """F5: outputs with the default table equal the C restatement's; (ii, imu) through the probe equal X87Walk's (the walk
    kernel rounds the sum like the x87 does), on 2 streams."""
    from gr_baz_amd import resamp
    ratios, taps = f5_ratios(F5_L), rr.taps()
    x = np.stack([signal(F5_L, 92), signal(F5_L, 93)])
    with resamp.Resampler(F5_PHASE, 1.0, nstreams=2) as blk:
        oracles = [rr.Resampler(F5_PHASE, 1.0) for _ in range(2)]
        pos = 0
        for n, (ii, imu, kx, mu, ratio) in zip(F5_CALLS, f5_run()):
            out, k = blk.work(x[:, pos:], n, rr=ratios[pos:])
            assert out.shape == (2, n) and k == kx and blk.mu() == mu and blk.resamp_ratio() == ratio
            for s in range(2):
                o, ko = oracles[s].work(x[s, pos:], n, rr=ratios[pos:])
                assert ko == k and np.array_equal(out[s].view(np.uint32), o.view(np.uint32))
            pos += k
    S = 2
    px = probe_input(S, F5_L, F5_L).view(np.complex64)[:, :, 0]
    for second_pass in (False, True):
        with resamp.Resampler(F5_PHASE, 1.0, nstreams=S) as blk:
            blk.set_taps(probe_table(second_pass))
            pos = 0
            for n, (ii, imu, kx, mu, ratio) in zip(F5_CALLS, f5_run()):
                out, k = blk.work(px[:, pos:], n, rr=ratios[pos:])
                assert out.shape == (S, n) and k == kx
                v = decode(np.ascontiguousarray(out).view(np.float32).reshape(S, n, 2), S, pos, second_pass, ii)
                assert np.array_equal(v, imu if second_pass else ii)
                pos += k
