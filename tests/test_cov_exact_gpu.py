"""Every covariance kernel against exact integer arithmetic, bit for bit (tests/cov_exact_ref.py; the reference itself is
checked in tests/test_cov_exact.py).  With integer-valued samples R = x x^H / K does not depend on the order of summation,
so each case demands np.array_equal on the real and on the imaginary parts of the R tap (debug_cov), R == R^H exactly, and
that nothing is written past the batch -- at every kernel, at every branch of it that another shape takes:

  cov_mfma_kernel<M>      slow path (column tail, tile tails, PAD rows), fast path (one, two, three and four 32-step buffers), the
                          m = 4 instantiation (lab: BAZ_MUSIC_COV_OLD=1), the tile loop past its first round (> 32,768 tiles)
  cov_mfma2_kernel<M>     slow and fast path with and without rows past 2 m, the grid-stride loop (> 32,768 items)
  cov4_x4_kernel          (lab: BAZ_MUSIC_FUSE=0) one to three 8-chunk groups, the load ring across two and three items of a wave
  cov4_evd_kernel         the shipped grid; one workgroup (lab: BAZ_MUSIC_COVEVD_BLOCKS=1) with 16 / 32 / 64-item tasks under both
                          rotation schedules; the order-mode twin
  cov_wide_mfma_kernel    no chunk, one and two chunks of the ring, k-step tails; the ring across items (> 8 CUs items)
  cov_wide_pairs_kernel   3 and 4 antenna blocks with and without a partial one, tails; the task walk (> 64 CUs tasks)
  cov_wide_kernel         (lab: BAZ_MUSIC_WIDE_COV_MFMA=0) one to three LDS passes, K % 32 tails

The scenes carry graded per-antenna gains (2^-20 .. 2^0), so the entries of one R span 2^-40 .. 2^0 of its largest: the tap
tests of test_gpu_parity.py and test_path_accuracy.py (1e-14 / 1e-13 of max|R|) cannot see the weak rows, these can.
Further: fp32 subnormal samples (scale 2^-139) and large ones (2^40), and NaN / Inf samples in items that share a tile or a
load ring with healthy ones.  All through the lab library: the kernels are the release library's."""
import functools

import numpy as np
import pytest

import cov_exact_ref as cx
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

RES = 32
PAD = 3               # rows past the batch in the R buffer
SENT = -7.0
LAB_VARS = ("BAZ_MUSIC_FUSE", "BAZ_MUSIC_COV_OLD", "BAZ_MUSIC_WIDE_COV_MFMA", "BAZ_MUSIC_COVEVD_BLOCKS",
            "BAZ_MUSIC_COVEVD_TASK_ITEMS", "BAZ_MUSIC_COVEVD_DEFER", "BAZ_MUSIC_COV_BLOCKS_PER_CU")

TWO_KERNELS = {"BAZ_MUSIC_FUSE": "0"}
OLD4 = {"BAZ_MUSIC_COV_OLD": "1"}
SCALAR_WIDE = {"BAZ_MUSIC_WIDE_COV_MFMA": "0"}
ONE_BLOCK = {"BAZ_MUSIC_COVEVD_BLOCKS": "1"}


def kernel_name(m, K, env):
    """the covariance kernel a context of this shape launches under `env` (baz_music_create)"""
    if m > 32:
        return "bazwide::cov_wide_kernel" if env.get("BAZ_MUSIC_WIDE_COV_MFMA") == "0" else "bazwide::cov_wide_pairs_kernel"
    if m > 16:
        return "bazwide::cov_wide_kernel" if env.get("BAZ_MUSIC_WIDE_COV_MFMA") == "0" else "bazwide::cov_wide_mfma_kernel"
    if m > 8:
        return "bazmusic::cov_mfma2_kernel<%d>" % m
    if m == 4 and K % 256 == 0 and env.get("BAZ_MUSIC_COV_OLD") != "1":
        return "bazmusic::cov4_x4_kernel" if env.get("BAZ_MUSIC_FUSE") == "0" else "bazmusic::cov4_evd_kernel"
    return "bazmusic::cov_mfma_kernel<%d>" % m


@functools.lru_cache(maxsize=None)
def table_of(m):
    return mo.steering_table_c64(mo.array_geometry(m), RES, mo.FREQUENCY, mo.SPACING)


def cus(gpu_device):
    import torch
    return int(torch.cuda.get_device_properties(gpu_device).multi_processor_count)


class Tap:
    """a lab context of (m, K) under `env`, checked to launch `kernel`; tap(x, B) returns the R buffer with its PAD sentinel rows"""

    def __init__(self, monkeypatch, gpu_device, m, K, env=None, kernel=None, order=None):
        from gr_baz_amd import capi
        env = env or {}
        for k in LAB_VARS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.m, self.K, self.dev = m, K, gpu_device
        self.ctx = capi.Context(m, 2 if order else 1, m * K, RES, table_of(m), lab=True)
        try:
            want = kernel or kernel_name(m, K, env)
            assert self.ctx.stage_name(0) == want, "the context launches %s, the case is about %s" % (self.ctx.stage_name(0), want)
            if order:
                self.ctx.set_order_mode(order)
                assert self.ctx.stage_name(0) == want
        except BaseException:
            self.ctx.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def upload(self, items, idx=None):
        """(B, 2 K m) float32 on the device; idx: the batch items[idx], gathered there"""
        import torch
        x = torch.from_numpy(np.array(items, dtype=np.complex64, order="C").view(np.float32)).to(self.dev)   # (a writable copy)
        if idx is not None:
            x = x[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.dev)].contiguous()
        return x

    def tap(self, x, B):
        import torch
        assert x.shape == (B, 2 * self.K * self.m) and x.is_contiguous()
        R = torch.full((B + PAD, self.m * self.m, 2), SENT, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize()                     # (the tap runs on the context's own stream)
        self.ctx.debug_cov(x.data_ptr(), B, R.data_ptr())
        self.ctx.sync()
        return R.cpu().numpy()


def _first_mismatch(got, ref):
    bad = np.argwhere(~(got == ref))
    b, a, c = (int(v) for v in bad[0])
    return "%d of %d entries differ; first: item %d entry (%d, %d): got %r (%s), expected %r (%s)" % (
        len(bad), got.size, b, a, c, float(got[b, a, c]), float(got[b, a, c]).hex(), float(ref[b, a, c]), float(ref[b, a, c]).hex())


def check_exact(Rbuf, ref_re, ref_im, what, poisoned=()):
    """the whole contract of one tap: sentinel rows untouched, every written part equal to the reference (values: the sign of a
    zero is free), R == R^H exactly.  poisoned: {item: antenna} -- there, entries off row and column `antenna` are exact and
    every entry on them is non-finite in both parts."""
    B, m = ref_re.shape[0], ref_re.shape[1]
    assert Rbuf.shape == (B + PAD, m * m, 2)
    assert np.all(Rbuf[B:] == SENT), "%s: rows past the batch were written" % what
    re = Rbuf[:B, :, 0].reshape(B, m, m)
    im = Rbuf[:B, :, 1].reshape(B, m, m)
    poisoned = dict(poisoned)
    ok = np.ones(B, bool)
    for item in poisoned:
        ok[item] = False
    assert np.array_equal(re[ok], ref_re[ok]), "%s: Re R: %s" % (what, _first_mismatch(re[ok], ref_re[ok]))
    assert np.array_equal(im[ok], ref_im[ok]), "%s: Im R: %s" % (what, _first_mismatch(im[ok], ref_im[ok]))
    assert np.array_equal(re[ok], re[ok].transpose(0, 2, 1)) and np.array_equal(im[ok], -im[ok].transpose(0, 2, 1)), \
        "%s: R is not exactly Hermitian" % what
    for item, a in poisoned.items():
        off = np.ones((m, m), bool)
        off[a, :] = False
        off[:, a] = False
        assert np.array_equal(re[item][off], ref_re[item][off]) and np.array_equal(im[item][off], ref_im[item][off]), \
            "%s: poisoned item %d (antenna %d): an entry off its row and column changed" % (what, item, a)
        assert not np.any(np.isfinite(re[item][~off])) and not np.any(np.isfinite(im[item][~off])), \
            "%s: poisoned item %d (antenna %d): a finite entry on its row or column" % (what, item, a)


def run_small(monkeypatch, gpu_device, m, Ks, batches, env=None, order=None, **scene_kw):
    """one context per K; the batches are the leading items of one scene"""
    env = env or {}
    for K in Ks:
        sc = cx.make(max(batches), m, K, seed=31 * m + K, **scene_kw)
        with Tap(monkeypatch, gpu_device, m, K, env, order=order) as t:
            x = t.upload(sc["items"])
            for B in batches:
                got = t.tap(x[:B].contiguous(), B)
                check_exact(got, sc["re"][:B], sc["im"][:B], "m %d K %d batch %d %s" % (m, K, B, env))


def run_tiled(monkeypatch, gpu_device, m, K, B, env=None, D=64, poison=None):
    """a batch of B items gathered on the device from D distinct ones.  poison: [(item, antenna, column, value)] written into the batch"""
    env = env or {}
    sc = cx.make(D, m, K, seed=77 * m + K)
    idx = cx.tile_index(D, B, seed=m + K)
    ref_re, ref_im = cx.tiled(sc, idx)
    with Tap(monkeypatch, gpu_device, m, K, env) as t:
        x = t.upload(sc["items"], idx)
        for item, a, col, val in (poison or ()):
            x[item, 2 * (col * m + a)] = val
            x[item, 2 * (col * m + a) + 1] = val
        got = t.tap(x, B)
    check_exact(got, ref_re, ref_im, "m %d K %d batch %d %s" % (m, K, B, env), poisoned={p[0]: p[1] for p in (poison or ())})


# ---- cov_mfma_kernel<M> ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 4, 5, 6, 7, 8])
def test_cov_mfma_slow_path(m, gpu_device, monkeypatch):
    """K % 128 != 0: one k-step per iteration with the 4 t + kk < K tail (K = 1: three of four lanes idle; K = 3, 5: a partial
    only or last step; K = 37: nine full steps and one column).  Batches 1, 5, 17 end inside a tile at m = 2 (four items per
    tile), m = 3 and m = 4 (two); m = 3, 5, 6, 7 carry PAD rows.  (m = 4 takes this kernel wherever K % 256 != 0.)"""
    run_small(monkeypatch, gpu_device, m, (1, 3, 5, 37), (1, 5, 17))


@pytest.mark.parametrize("m", [2, 3, 5, 8])
def test_cov_mfma_fast_path(m, gpu_device, monkeypatch):
    """K % 128 == 0, two 32-step register buffers: K = 128 never arms the second, 256 runs both once, 384 re-arms the first and
    ends on more_b == false, 512 goes round twice.  m = 3, 5: the PAD rows' fp32 multiply by `keep`."""
    run_small(monkeypatch, gpu_device, m, (128, 256, 384, 512), (5, 17))


def test_cov_mfma_m4_instantiation(gpu_device, monkeypatch):
    """cov_mfma_kernel<4> at K % 256 == 0, where the product runs the dwordx4 kernels (lab: BAZ_MUSIC_COV_OLD=1)"""
    run_small(monkeypatch, gpu_device, 4, (256, 768), (5, 17), env=OLD4)


@pytest.mark.parametrize("K", [3, 128])
def test_cov_mfma_tile_loop_past_the_first_round(K, gpu_device, monkeypatch):
    """the grid stops at 8,192 workgroups = 32,768 waves: from tile 32,768 on a wave takes a second tile, through both
    wave_lds_fence() hand-overs of the Gram tile"""
    run_tiled(monkeypatch, gpu_device, 8, K, 32768 + 37)


# ---- cov_mfma2_kernel<M> -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [9, 13, 16])
def test_cov_mfma2(m, gpu_device, monkeypatch):
    """slow path (K = 1, 3, 50) and fast path (K % 64 == 0: one, two, three 16-step chunks); m < 16 zeroes the rows past 2 m of
    the second tile (slow: a select; fast: the fp32 multiply by keep1)"""
    run_small(monkeypatch, gpu_device, m, (1, 3, 50, 64, 128, 192), (1, 9))


def test_cov_mfma2_grid_stride(gpu_device, monkeypatch):
    run_tiled(monkeypatch, gpu_device, 9, 3, 32768 + 5)


# ---- cov4_x4_kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512, 768])
def test_cov4_x4(K, gpu_device, monkeypatch):
    run_small(monkeypatch, gpu_device, 4, (K,), (1, 5), env=TWO_KERNELS)


def test_cov4_x4_ring_across_items(gpu_device, monkeypatch):
    """one workgroup per CU: 4 CUs waves.  8 CUs + 5 items: five waves take three items, the others two -- every slot of the load
    ring is re-armed from the wave's NEXT item (nsrc) while the current one is still being consumed"""
    run_tiled(monkeypatch, gpu_device, 4, 256, 8 * cus(gpu_device) + 5, env=TWO_KERNELS)


# ---- cov4_evd_kernel and its order twin --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512])
def test_cov4_evd_shipped_grid(K, gpu_device, monkeypatch):
    run_small(monkeypatch, gpu_device, 4, (K,), (70,))


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("task_items", ["16", "32", "64"])
def test_cov4_evd_one_workgroup(task_items, defer, gpu_device, monkeypatch):
    """one workgroup of four waves walks every task (131 and 197 items: short last tasks, waves with several tasks), the R of a
    task waiting in the LDS table or (deferred rotation) in registers: the tap's bits depend on neither"""
    env = dict(ONE_BLOCK, BAZ_MUSIC_COVEVD_TASK_ITEMS=task_items, BAZ_MUSIC_COVEVD_DEFER=defer)
    run_small(monkeypatch, gpu_device, 4, (256,), (131, 197), env=env)


@pytest.mark.parametrize("env", [{}, dict(ONE_BLOCK, BAZ_MUSIC_COVEVD_TASK_ITEMS="16")], ids=["shipped", "one-workgroup"])
def test_cov4_evd_order_twin(env, gpu_device, monkeypatch):
    run_small(monkeypatch, gpu_device, 4, (256,), (131,), env=env, order="mdl")


# ---- cov_wide_mfma_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 24, 32])
def test_cov_wide_mfma(m, gpu_device, monkeypatch):
    """K < 32: no chunk of the ring, k-steps one by one; 32: one chunk, no tail; 33, 40: a chunk and a partial / two tail steps;
    66: two chunks and a partial step.  m = 17, 24: antennas past m re-read antenna m - 1"""
    run_small(monkeypatch, gpu_device, m, (1, 3, 32, 33, 40, 66), (5,))


def test_cov_wide_mfma_ring_across_items(gpu_device, monkeypatch):
    """two workgroups per CU: 8 CUs waves; with 8 CUs + 5 items five waves re-arm their ring from a second item"""
    run_tiled(monkeypatch, gpu_device, 17, 33, 8 * cus(gpu_device) + 5)


# ---- cov_wide_pairs_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [33, 37, 49, 64])
def test_cov_wide_pairs(m, gpu_device, monkeypatch):
    run_small(monkeypatch, gpu_device, m, (1, 5, 32, 33, 37), (3,))


def test_cov_wide_pairs_task_walk(gpu_device, monkeypatch):
    """the grid stops at 16 CUs workgroups = 64 CUs waves; m = 33 has 6 block pairs per item: past 64 CUs / 6 items a wave walks on
    to a second (item, pair) task"""
    run_tiled(monkeypatch, gpu_device, 33, 5, -(-64 * cus(gpu_device) // 6) + 7)


# ---- cov_wide_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [17, 40, 64])
def test_cov_wide_scalar(m, gpu_device, monkeypatch):
    """one workgroup per item, 32 time columns per LDS pass: K = 1 and 32 (one pass), 33 (a pass of one column), 70 (three passes)"""
    run_small(monkeypatch, gpu_device, m, (1, 32, 33, 70), (3,), env=SCALAR_WIDE)


# ---- dynamic range -----------------------------------------------------------------------------------------------------------
# a fast-path and a slow-path shape of every kernel family (the dwordx4 kernels have one path); (5, 128) and (13, 64) are the
# fast PAD paths, whose fp32 multiply by keep / keep1 runs BEFORE the widening
RANGE_CASES = [(5, 128, {}), (5, 37, {}), (2, 128, {}), (8, 128, {}), (13, 64, {}), (13, 50, {}), (16, 64, {}),
               (4, 256, OLD4), (4, 37, {}), (4, 256, TWO_KERNELS), (4, 256, {}),
               (17, 33, {}), (17, 3, {}), (33, 37, {}), (33, 5, {}), (17, 33, SCALAR_WIDE), (40, 70, SCALAR_WIDE)]


@pytest.mark.parametrize("scale", [cx.SUBNORMAL_SCALE, cx.LARGE_SCALE], ids=["subnormal", "large"])
@pytest.mark.parametrize("m,K,env", RANGE_CASES, ids=["m%d-K%d%s" % (m, K, "".join("-" + k[10:] + v for k, v in e.items())) for m, K, e in RANGE_CASES])
def test_dynamic_range(m, K, env, scale, gpu_device, monkeypatch):
    """samples scaled by 2^-139 (most are fp32 subnormals, R lives near 2^-270) and by 2^40, with graded gains: the widening keeps
    subnormals (static_cast<gr_complexd> of the reference does), and so must whatever a kernel does before it widens"""
    gains = cx.subnormal_gains(m, seed=m + K) if scale == cx.SUBNORMAL_SCALE else None
    run_small(monkeypatch, gpu_device, m, (K,), (5,), env=env, gain_exp=gains, scale_exp=scale)


# ---- non-finite neighbours ---------------------------------------------------------------------------------------------------
def _poison(B, m, K, spots):
    """[(item, antenna, column, value)]: NaN and Inf alternate; the antennas include the last one (the one that rows past m
    re-read), the columns the last one (a tail's)"""
    out = []
    for j, item in enumerate(spots):
        out.append((item % B, (m - 1, 1 % m, 0)[j % 3], (K - 1) if j % 2 == 0 else (5 * j) % K, float("nan") if j % 2 == 0 else float("inf")))
    return out


@pytest.mark.parametrize("m,K,env", [(2, 37, {}), (2, 128, {}), (3, 37, {}), (3, 128, {}), (4, 256, OLD4), (4, 37, {})],
                         ids=["m2-slow", "m2-fast", "m3-slow", "m3-fast", "m4-old-fast", "m4-slow"])
def test_poisoned_items_in_a_shared_tile(m, K, env, gpu_device, monkeypatch):
    """several items share a 16 x 16 Gram tile (block diagonal): a NaN or Inf of one must stay in its block.  Item 16 of 17 is alone
    in the last tile, whose other slots re-read it (batch tail)"""
    B = 17
    run_tiled(monkeypatch, gpu_device, m, K, B, env=env, D=17, poison=_poison(B, m, K, (1, 6, 16)))


def test_poisoned_items_in_a_load_ring_cov4_x4(gpu_device, monkeypatch):
    """4 CUs + 9 items: waves 0 .. 8 take two.  Item 3 is a wave's first (its ring moves on to healthy item 4 CUs + 3), item 4 CUs + 2 a
    wave's second (loaded while healthy item 2 is consumed), the last item is re-read past the end"""
    n = 4 * cus(gpu_device)
    B = n + 9
    run_tiled(monkeypatch, gpu_device, 4, 256, B, env=TWO_KERNELS, poison=_poison(B, 4, 256, (3, n + 2, B - 1)))


@pytest.mark.parametrize("defer", ["0", "1"])
def test_poisoned_items_in_a_load_ring_cov4_evd(defer, gpu_device, monkeypatch):
    """16-item tasks of one workgroup: the ring runs across the items of a task; item 130 is the only one of the last task"""
    env = dict(ONE_BLOCK, BAZ_MUSIC_COVEVD_TASK_ITEMS="16", BAZ_MUSIC_COVEVD_DEFER=defer)
    run_tiled(monkeypatch, gpu_device, 4, 256, 131, env=env, poison=_poison(131, 4, 256, (3, 70, 130)))


def test_poisoned_items_in_a_load_ring_cov_wide_mfma(gpu_device, monkeypatch):
    n = 8 * cus(gpu_device)
    B = n + 5
    run_tiled(monkeypatch, gpu_device, 17, 33, B, poison=_poison(B, 17, 33, (2, n + 3, B - 1)))
