"""baz_agc_cc: oracle pins on CPU, HIP parity on the GPU.  Tolerance: the parallel scan
re-associates an fp64 recurrence (~1e-15), the outputs are float32 -> 1e-5 relative like the main path;
measured differences are at most 1 ulp_f32."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from oracle import agc_ref as ar


def agc_golden():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "agc_*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def close(a, b, rtol=1e-5):
    a = np.asarray(a); b = np.asarray(b)
    if np.iscomplexobj(a):
        return close(a.real, b.real, rtol) and close(a.imag, b.imag, rtol)
    fin = np.isfinite(b)
    if not np.array_equal(np.isfinite(a), fin):
        return False
    # components of out near a zero crossing are small: bound by the magnitude scale of the pair
    return bool(np.all(np.abs(a[fin] - b[fin]) <= rtol * np.maximum(np.abs(b[fin]), 1e-30) + 1e-37))


def close_strict(a, b, rtol=1e-5):
    """close() and, beyond it, what its isfinite masks cannot tell apart: the same NaN, +inf and -inf positions, and the
    reference's sign bit wherever the reference is +0 or -0."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if np.iscomplexobj(a):
        a = a.view(np.float32); b = b.view(np.float32)
    if not close(a, b, rtol):
        return False
    zero = b == 0
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
                and np.array_equal(np.isneginf(a), np.isneginf(b))
                and np.array_equal(a[zero] == 0, b[zero] == 0) and np.array_equal(np.signbit(a[zero]), np.signbit(b[zero])))


def ulp_flips(got, ref):
    """(largest difference of the float32 bit patterns, number of differing floats, floats compared) where ref is finite."""
    got = np.ascontiguousarray(got); ref = np.ascontiguousarray(ref)
    if np.iscomplexobj(ref):
        got = got.view(np.float32); ref = ref.view(np.float32)
    fin = np.isfinite(ref)
    u = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))[fin]
    return (int(u.max()) if u.size else 0), int(np.count_nonzero(u)), int(u.size)


def run_calls(blk, x, calls):
    outs, envs, muls = [], [], []
    pos = 0
    for c in calls:
        o, e, m = blk.work(x[pos:pos + c])
        outs.append(o); envs.append(e); muls.append(m)
        pos += c
    return np.concatenate(outs), np.concatenate(envs), np.concatenate(muls)


@pytest.mark.parametrize("name", agc_golden())
def test_c_oracle_matches_reference_source_vectors(name):
    g = load(name)
    out, env, mul = run_calls(ar.Agc(float(g["rate"]), float(g["reference"])), g["x"], g["calls"])
    assert np.array_equal(out, g["out"]) and np.array_equal(env, g["env"]) and np.array_equal(mul, g["mul"])


@pytest.mark.skipif(not ar.have_ref(), reason="oracle/_ref not built")
def test_reference_source_build_is_stateful_like_the_restatement():
    x = (np.arange(1, 3001) * (0.01 + 0.01j)).astype(np.complex64)
    a = ar.Agc(1e-3, 1.0)
    b = ar.Agc(1e-3, 1.0, use_reference_source=True)
    for lo, hi in ((0, 1), (1, 2000), (2000, 3000)):
        ra, rb = a.work(x[lo:hi]), b.work(x[lo:hi])
        assert all(np.array_equal(p, q) for p, q in zip(ra, rb))
    o, e, m = ar.Agc(1e-3, 1.0).work(x[:5])
    assert e[0] == np.float32(abs(x[0]))          # count == 0: env = |x0|  (lib/baz_agc_cc.cc:79-80)
    assert m[0] == np.float32(1.0 / np.float64(np.float32(abs(np.complex128(x[0])))) ) or abs(m[0] * e[0] - 1) < 1e-6


def test_abi_symbols_and_loud_failure():
    from gr_baz_amd import agc
    src = open(os.path.join(ROOT, "include", "baz_agc_hip.h")).read()
    declared = sorted(set(re.findall(r"BAZ_AGC_API\s+[\w\s\*]+?\b(baz_agc_\w+)\s*\(", src)))
    assert declared == sorted(agc.SYMBOLS)
    raw = ctypes.CDLL(agc.LIB_PATH)
    for s in declared:
        assert getattr(raw, s) is not None
    assert "lib/baz_agc_cc.cc:64-102" in src
    L = agc.lib()
    h = ctypes.c_void_p()
    assert L.baz_agc_create(ctypes.byref(h), 0, 1e-4, 1.0, 1.0, 0.0, -1) == -1     # nstreams == 0
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(agc.AgcError):
            agc.Agc()


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", agc_golden())
def test_hip_agc_matches_golden(name, gpu_device):
    from gr_baz_amd import agc
    g = load(name)
    with agc.Agc(float(g["rate"]), float(g["reference"])) as blk:
        out, env, mul = run_calls(blk, g["x"], g["calls"])
        assert blk.count == int(g["calls"].sum())
    assert close(env, g["env"]) and close(mul, g["mul"]) and close(out, g["out"])
    # The per-sample arithmetic is the reference's operation for operation; only a tile's entry state comes out of the
    # re-associated scan (a few ulp_f64 off): float32 outputs are the sequential loop's bit for bit, except a 1-ulp flip
    # in < 1e-5 of the samples (measured 8e-7 at rate 1e-4, 6e-8 at 1e-3: profiles/r02_agc_exactness.txt)
    for got, ref in ((np.ascontiguousarray(out).view(np.float32), np.ascontiguousarray(g["out"]).view(np.float32)),
                     (env, g["env"]), (mul, g["mul"])):
        fin = np.isfinite(ref)
        u = np.abs(np.ascontiguousarray(got).view(np.int32).astype(np.int64) - np.ascontiguousarray(ref).view(np.int32).astype(np.int64))[fin]
        assert u.size == 0 or (u.max() <= 1 and np.count_nonzero(u) <= max(1, 1e-5 * u.size))


@pytest.mark.gpu
def test_hip_agc_multi_stream_device_path_and_tail_alignment(gpu_device):
    import torch
    from gr_baz_amd import agc
    S, n, stride = 5, 10007, 10240           # odd length: scalar tail; stride keeps stream starts 16-B aligned
    rng = np.random.default_rng(5)
    x = ((rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))) * np.linspace(0.2, 4.0, n)).astype(np.complex64)
    xin = np.zeros((S, stride), np.complex64); xin[:, :n] = x
    with agc.Agc(3e-3, 1.5, nstreams=S) as blk:
        d_in = torch.from_numpy(xin.view(np.float32)).to(gpu_device)
        d_out = torch.zeros_like(d_in)
        d_env = torch.zeros(S, stride, dtype=torch.float32, device=gpu_device)
        d_mul = torch.zeros_like(d_env)
        torch.cuda.synchronize()                       # the engine runs on its own stream: fills first
        for lo, hi in ((0, 4097), (4097, n)):          # second call starts at an odd offset (unaligned float2 pairs)
            blk.process_device(d_in.data_ptr() + lo * 8, hi - lo, stride, d_out.data_ptr() + lo * 8,
                               d_env.data_ptr() + lo * 4, d_mul.data_ptr() + lo * 4)
        blk.sync()
        out = d_out.cpu().numpy().view(np.complex64)[:, :n]
        env = d_env.cpu().numpy()[:, :n]
        mul = d_mul.cpu().numpy()[:, :n]
    for s in range(S):
        o, e, m = ar.Agc(3e-3, 1.5).work(x[s])
        assert close(env[s], e) and close(mul[s], m) and close(out[s], o)


@pytest.mark.gpu
def test_agc_host_block_and_python_surface(gpu_device):
    """baz.agc_cc -> C++ host block -> C-ABI: ports of lib/baz_agc_cc.cc:52-54, optional outputs (:68-69)."""
    from gr_baz_amd import baz
    g = load("agc_stateful_rate1e-2")
    blk = baz.agc_cc(float(g["rate"]), float(g["reference"]))
    assert blk.name() == "gr_agc_cc" and blk.input_item_sizes() == [8] and blk.output_item_sizes() == [8, 4]
    assert blk.output_streams() == (1, 3)
    # requests for large work() calls that cost no sample of a finite capture: look-back, not an output multiple
    assert blk.output_multiple() == 1 and blk.history() == 16385 and blk.min_output_buffer() == 2 * 16384
    outs, envs, muls = [], [], []
    pos = 0
    for c in g["calls"]:
        produced, o, e, m = blk.work(g["x"][pos:pos + c], 3)
        assert produced == c
        outs.append(o); envs.append(e); muls.append(m)
        pos += c
    assert close(np.concatenate(outs), g["out"]) and close(np.concatenate(envs), g["env"]) and close(np.concatenate(muls), g["mul"])
    p1, o1, e1, m1 = baz.agc_cc().work(g["x"][:100], 1)
    assert p1 == 100 and e1 is None and m1 is None


@pytest.mark.gpu
def test_agc_zero_first_sample_and_reset(gpu_device):
    """|x0| = 0 makes env = 0 and gain = inf in the reference (reference/0, lib/baz_agc_cc.cc:89): same here."""
    from gr_baz_amd import agc
    x = np.zeros(300, np.complex64); x[5:] = (1 + 1j)
    o, e, m = ar.Agc(0.1, 1.0).work(x)
    with agc.Agc(0.1, 1.0) as blk:
        o2, e2, m2 = blk.work(x)
        assert close(e2, e) and close(m2, m)
        assert np.array_equal(np.isnan(o2.real), np.isnan(o.real))
        blk.reset()
        assert blk.count == 0
        o3, e3, m3 = blk.work(x[5:])
    assert close(e3, ar.Agc(0.1, 1.0).work(x[5:])[1])


@pytest.mark.gpu
def test_fast_sqrt_and_division_are_the_rounded_ones(gpu_device):
    """Full tiles of ordinary values run lean sqrt / division sequences (agc_kernels.hip.h): the Newton cores of the rounded
    library functions without their range scaling.  Bit for bit the same as __dsqrt_rn / __ddiv_rn on |x|^2 of random float
    samples, on envelope-like divisors, and log-uniformly over the whole range the fast path accepts."""
    import torch
    from gr_baz_amd import agc
    rng = np.random.default_rng(11)
    n = 1 << 22
    xs = (rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-18, 18, size=(n, 1))).astype(np.float32).astype(np.float64)
    a1 = xs[:, 0] * xs[:, 0] + xs[:, 1] * xs[:, 1]                                  # |x|^2 as the kernel forms it
    b1 = np.sqrt(a1) * rng.uniform(0.5, 2.0, size=n)                                 # envelope-like
    a2 = np.ldexp(rng.uniform(1.0, 2.0, size=n), rng.integers(-399, 399, size=n))    # the whole accepted range
    b2 = np.ldexp(rng.uniform(1.0, 2.0, size=n), rng.integers(-399, 399, size=n))
    a3 = np.full(n, 1.0); b3 = np.ldexp(rng.uniform(1.0, 2.0, size=n), rng.integers(-60, 60, size=n))   # reference / env
    a4 = np.nextafter(np.ldexp(1.0, rng.integers(-300, 300, size=n)), rng.choice([0.0, np.inf], size=n))  # around powers of two
    with agc.Agc(1e-4, 1.0) as blk:
        for a, b in ((a1, b1), (a2, b2), (a3, b3), (a4, b2), (a2, a4)):
            da = torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
            db = torch.from_numpy(np.ascontiguousarray(b)).to(gpu_device)
            torch.cuda.synchronize()
            assert blk.debug_selfcheck(da.data_ptr(), db.data_ptr(), n) == (0, 0)


@pytest.mark.gpu
def test_fast_and_general_tile_paths_agree(gpu_device, monkeypatch):
    """BAZ_AGC_FAST=0 keeps every tile on the general path.  The two builds differ only in how a tile's ENTRY state is
    re-associated (DPP scan with host-computed powers against the (A, S) pair scan): float32 outputs identical except a
    1-ulp flip in < 1e-5 of the samples, like either against the sequential loop; zeros in the stream (general path for
    those tiles) and a ragged tail included."""
    import torch
    from gr_baz_amd import agc
    S, n = 3, 256 * 40 + 77
    rng = np.random.default_rng(3)
    x = ((rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))) * np.linspace(0.1, 5.0, n)).astype(np.complex64)
    x[1, 1000:1300] = 0                                   # a zero run: |x|^2 = 0 is not "ordinary"
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("BAZ_AGC_FAST", mode)
        with agc.Agc(1e-3, 2.0, nstreams=S) as blk:
            d_in = torch.from_numpy(x.view(np.float32)).to(gpu_device)
            d_out = torch.zeros_like(d_in)
            d_env = torch.zeros(S, n, dtype=torch.float32, device=gpu_device)
            d_mul = torch.zeros_like(d_env)
            d_items = torch.zeros(n, S, 2, dtype=torch.float32, device=gpu_device)
            torch.cuda.synchronize()
            blk.process_device(d_in.data_ptr(), n, n, d_out.data_ptr(), d_env.data_ptr(), d_mul.data_ptr())
            blk.sync()
            blk.reset()
            blk.process_device_interleaved(d_in.data_ptr(), n, n, d_items.data_ptr())
            blk.sync()
            outs[mode] = [t.cpu().numpy() for t in (d_out, d_env, d_mul, d_items)]
    for got, ref in zip(outs["1"], outs["0"]):
        fin = np.isfinite(ref)
        u = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))[fin]
        assert u.max() <= 1 and np.count_nonzero(u) <= max(1, 1e-5 * u.size)
    assert np.array_equal(outs["1"][3].reshape(n, S, 2).transpose(1, 0, 2).reshape(S, -1), outs["1"][0].reshape(S, -1))   # both output forms agree
    for s in range(S):
        o, e, m = ar.Agc(1e-3, 2.0).work(x[s])
        assert close(outs["1"][1][s], e) and close(outs["1"][0][s].view(np.complex64), o)


# --------------------------------------------------------------------------- the carry scan past its first level
# agc_carry_kernel: 1,024 threads per stream; thread t composes a slice of per = ceil(ntiles / 1024) tile maps, a 64-lane
# wave scan, then the 16 wave totals.  Shapes at the thresholds: one wave exactly, a second wave, several waves, per = 1
# with every thread busy, per = 2, per = 3 with a ragged tail.
SCAN_SHAPES = [256 * 64, 256 * 64 + 1, 256 * 200 + 77, 256 * 1024, 256 * 1024 + 1, 256 * 2049 + 77]
SCAN_REFERENCE = 1.5
_scan_cache = {}


def scan_input(S, n):
    """Noise whose amplitude changes from tile to tile (2^0 .. 2^6, cycling, shifted per stream) on a slow ramp: a carry
    taken from the wrong tile, wave or slice moves the envelope by percent.  Tiles 70-72 and 1023-1025 are zero (general-path
    tiles between fast-path ones; short enough for the envelope to stay an ordinary number)."""
    key = ("x", S, n)
    if key not in _scan_cache:
        rng = np.random.default_rng(1000 + S)
        t = np.arange(n)
        x = np.empty((S, n), np.complex64)
        for s in range(S):
            amp = np.ldexp(0.5 + t / n, ((t // 256 + s) % 7).astype(np.int32))
            x[s] = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp).astype(np.complex64)
        x[:, 256 * 70:256 * 73] = 0
        x[:, 256 * 1023:256 * 1026] = 0
        x.setflags(write=False)
        _scan_cache[key] = x
    return _scan_cache[key]


def scan_oracle(S, n, rate):
    """(out, env, mul) of the sequential loop, one oracle instance per stream; computed once per shape."""
    key = ("ref", S, n, rate)
    if key not in _scan_cache:
        x = scan_input(S, n)
        r = [ar.Agc(rate, SCAN_REFERENCE).work(x[s]) for s in range(S)]
        ref = tuple(np.stack([q[i] for q in r]) for i in range(3))
        for a in ref:
            a.setflags(write=False)
        _scan_cache[key] = ref
    return _scan_cache[key]


def hip_planar(blk, x, dev, calls=None):
    """process_device with the env and mul ports over the call lengths `calls` (default: one call); row stride = n."""
    import torch
    S, n = x.shape
    d_in = torch.from_numpy(np.array(x).view(np.float32)).to(dev)        # (a copy: the cached inputs are read-only)
    d_out = torch.zeros_like(d_in)
    d_env = torch.zeros(S, n, dtype=torch.float32, device=dev)
    d_mul = torch.zeros_like(d_env)
    torch.cuda.synchronize()                       # the engine runs on its own stream: fills first
    lo = 0
    for c in (calls or (n,)):
        blk.process_device(d_in.data_ptr() + lo * 8, c, n, d_out.data_ptr() + lo * 8, d_env.data_ptr() + lo * 4,
                           d_mul.data_ptr() + lo * 4)
        lo += c
    assert lo == n
    blk.sync()
    return d_out.cpu().numpy().view(np.complex64), d_env.cpu().numpy(), d_mul.cpu().numpy()


def hip_interleaved(blk, x, dev):
    """process_device_interleaved: items[t * S + s] -> (S, n) complex64."""
    import torch
    S, n = x.shape
    d_in = torch.from_numpy(np.array(x).view(np.float32)).to(dev)        # (a copy: the cached inputs are read-only)
    d_items = torch.zeros(n, S, 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    blk.process_device_interleaved(d_in.data_ptr(), n, n, d_items.data_ptr())
    blk.sync()
    return np.ascontiguousarray(d_items.cpu().numpy().transpose(1, 0, 2)).view(np.complex64).reshape(S, n)


def assert_agc_parity(what, got, ref):
    """The project's bounds (test_hip_agc_matches_golden): 1e-5 relative, and on the float32 bit patterns at most 1 ulp in
    at most 1e-5 of the floats.  Prints the measured flip share first."""
    for name, g, r in zip(("out", "env", "mul"), got, ref):
        if g is None:
            continue
        worst, flips, size = ulp_flips(g, r)
        print("agc flips %s %s: %d of %d floats (share %.2e), largest %d ulp" % (what, name, flips, size, flips / max(size, 1), worst))
        assert close(g, r, rtol=1e-5), (what, name)
        assert worst <= 1 and flips <= max(1, 1e-5 * size), (what, name, worst, flips, size)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [1e-4, 1e-2])
@pytest.mark.parametrize("n", SCAN_SHAPES)
def test_hip_agc_carry_scan_levels_planar(n, rate, gpu_device):
    """process_device with env and mul, S = 2, against the sequential loop.  At rate 1e-2 the map coefficient A = a^(256 k)
    underflows to 0 on finite data within the 2,050-tile shape: legitimate, and without effect on the result."""
    from gr_baz_amd import agc
    S = 2
    x = scan_input(S, n)
    with agc.Agc(rate, SCAN_REFERENCE, nstreams=S) as blk:
        got = hip_planar(blk, x, gpu_device)
        assert blk.count == n
    assert_agc_parity("planar S=%d n=%d rate=%g" % (S, n, rate), got, scan_oracle(S, n, rate))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [1e-4, 1e-2])
@pytest.mark.parametrize("n", [256 * 64 + 1, 256 * 1024 + 1])
@pytest.mark.parametrize("S", [16, 5])
def test_hip_agc_carry_scan_levels_interleaved(S, n, rate, gpu_device):
    """process_device_interleaved (the form the benchmark's chain runs): S = 16 takes the float4 write-out, S = 5 the
    scalar one; 65 tiles (a second wave) and 1,025 tiles (per = 2)."""
    from gr_baz_amd import agc
    x = scan_input(S, n)
    with agc.Agc(rate, SCAN_REFERENCE, nstreams=S) as blk:
        out = hip_interleaved(blk, x, gpu_device)
        assert blk.count == n
    assert_agc_parity("interleaved S=%d n=%d rate=%g" % (S, n, rate), (out, None, None), scan_oracle(S, n, rate))


@pytest.mark.gpu
def test_hip_agc_carry_scan_levels_general_tile_path(gpu_device, monkeypatch):
    """BAZ_AGC_FAST=0: every tile map comes from the general path's (A, S) pair scan and feeds the same carry kernel
    (1,025 tiles: waves and per = 2), both output forms."""
    from gr_baz_amd import agc
    monkeypatch.setenv("BAZ_AGC_FAST", "0")
    S, n, rate = 2, 256 * 1024 + 1, 1e-4
    x = scan_input(S, n)
    with agc.Agc(rate, SCAN_REFERENCE, nstreams=S) as blk:
        got = hip_planar(blk, x, gpu_device)
        blk.reset()
        items = hip_interleaved(blk, x, gpu_device)
    ref = scan_oracle(S, n, rate)
    assert_agc_parity("general path planar n=%d" % n, got, ref)
    assert_agc_parity("general path interleaved n=%d" % n, (items, None, None), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_hip_agc_stateful_calls_across_scan_levels(path, gpu_device):
    """One context, calls of 300, 256*1100 + 5, 17,000 and 1 samples: the second call regrows the per-tile tables while the
    first call's launches may still be in flight and runs per = 2; the third enters with the state a multi-level call left."""
    from gr_baz_amd import agc
    calls = (300, 256 * 1100 + 5, 17000, 1)
    n, rate = sum(calls), 1e-4
    S = 1 if path == "host" else 2
    x = scan_input(S, n)
    ref = [run_calls(ar.Agc(rate, SCAN_REFERENCE), x[s], calls) for s in range(S)]
    ref = tuple(np.stack([q[i] for q in ref]) for i in range(3))
    with agc.Agc(rate, SCAN_REFERENCE, nstreams=S) as blk:
        if path == "host":
            got = tuple(a[None, :] for a in run_calls(blk, x[0], calls))
        else:
            got = hip_planar(blk, x, gpu_device, calls)
        assert blk.count == n
    assert_agc_parity("stateful %s path" % path, got, ref)


# --------------------------------------------------------------------------- non-finite samples
# The reference (oracle/agc_ref.c, .cc:79-100): an inf sample makes env = inf for good, so gain = 0 and every later
# finite sample comes out as (signed) 0; a NaN sample makes everything after it NaN.  Stream 0 carries the special
# sample, stream 1 is finite throughout (nothing may leak across streams).
def nonfinite_case(case):
    """-> (rate, [x of call 0, x of call 1, ...]) each x of shape (2, n)."""
    rng = np.random.default_rng(77)
    noise = lambda n: ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * 0.7).astype(np.complex64)
    if case == "a_inf_rate0.5":
        x = noise(256 * 12); x[0, 10] = np.inf
        return 0.5, [x]
    if case == "b_neg_inf_imag_rate1e-2":
        x = noise(256 * 400); x[0, 256 * 3 + 9] = complex(0, -np.inf)
        return 1e-2, [x]
    if case == "c_inf_state_enters_call":
        x0 = noise(600); x0[0, 5] = np.inf
        return 0.5, [x0, noise(256 * 70)]
    if case == "d_inf_first_sample":
        x = noise(256 * 12); x[0, 0] = np.inf
        return 0.5, [x]
    if case == "e_nan":
        x = noise(256 * 12); x[0, 256 * 2 + 100] = complex(np.nan, 0.25)
        return 0.5, [x]
    raise KeyError(case)


def nonfinite_run(blk, form, xs, dev):
    """-> per call (out, env | None, mul | None), each (2, n)."""
    if form == "planar":
        return [blk.work(x) for x in xs]
    return [(hip_interleaved(blk, x, dev), None, None) for x in xs]


def nonfinite_oracle(rate, xs):
    orc = [ar.Agc(rate, 1.0) for _ in range(2)]
    res = []
    for x in xs:
        r = [orc[s].work(x[s]) for s in range(2)]
        res.append(tuple(np.stack([q[i] for q in r]) for i in range(3)))
    return res


def assert_strict(what, got, ref):
    for name, g, r in zip(("out", "env", "mul"), got, ref):
        if g is not None:
            for s in range(r.shape[0]):
                assert close_strict(g[s], r[s]), (what, name, "stream %d" % s)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["planar", "interleaved"])
@pytest.mark.parametrize("case", ["a_inf_rate0.5", "b_neg_inf_imag_rate1e-2", "c_inf_state_enters_call",
                                  "d_inf_first_sample", "e_nan"])
def test_hip_agc_non_finite_samples_behave_like_the_reference(case, form, gpu_device):
    from gr_baz_amd import agc
    rate, xs = nonfinite_case(case)
    ref = nonfinite_oracle(rate, xs)
    if case == "a_inf_rate0.5":       # what the oracle itself says: env = inf, mul = 0, outputs exactly 0, one NaN float
        o, e, m = ref[0]
        assert np.all(np.isposinf(e[0, 10:])) and np.all(m[0, 10:] == 0) and np.all(o[0, 11:] == 0)
        assert np.count_nonzero(np.isnan(o[0].view(np.float32))) == 1 and np.isnan(o[0, 10].real)
    with agc.Agc(rate, 1.0, nstreams=2) as blk:
        got = nonfinite_run(blk, form, xs, gpu_device)
        assert blk.count == sum(x.shape[1] for x in xs)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_strict("%s %s call %d" % (case, form, i), g, r)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["planar", "interleaved"])
def test_hip_agc_reset_revives_a_stream_after_an_inf_sample(form, gpu_device):
    from gr_baz_amd import agc
    rate, xs = nonfinite_case("a_inf_rate0.5")
    fresh = np.ascontiguousarray(xs[0][:, 1000:])            # finite
    with agc.Agc(rate, 1.0, nstreams=2) as blk:
        got = nonfinite_run(blk, form, xs, gpu_device)
        assert_strict("before reset, " + form, got[0], nonfinite_oracle(rate, xs)[0])
        blk.reset()
        assert blk.count == 0
        got = nonfinite_run(blk, form, [fresh], gpu_device)
    ref = nonfinite_oracle(rate, [fresh])                    # fresh oracle instances
    assert np.all(np.isfinite(ref[0][1])) and np.all(ref[0][2] > 0)
    assert_strict("after reset, " + form, got[0], ref[0])
