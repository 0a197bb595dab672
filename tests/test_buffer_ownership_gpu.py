"""Every device and page-locked buffer of the three host libraries has an owner (gr_baz_amd/csrc/device_buffer.hip.h): whatever a
context allocated while it lived -- workspaces that regrew, both table sets, every opt-in mode's buffers, the host-fed path's slots --
is back when it is closed (the baz_*_debug_live_buffers taps count the live allocations), and a workspace that regrew between two
calls changes no bit of the second one."""
import gc
import os
import re

import numpy as np
import pytest

import smoothing_ref as sr
from conftest import ROOT
from oracle import agc_ref as ar
from oracle import music_oracle as mo
from oracle import resamp_ref as rr
from test_agc import SCAN_REFERENCE, assert_agc_parity, run_calls, scan_input

pytestmark = pytest.mark.gpu

# m, n, nsamples, res -- the smallest shapes that reach each family of buffers
SHAPES = {
    "m4_fused_covevd_row_classes_coarse": (4, 2, 1024, 360),
    "m8_coarse_and_int8_images": (8, 2, 64, 200),
    "m16_short_form": (16, 2, 64, 128),
    "m17_wide_matrix_core_scan": (17, 2, 136, 90),
}


def _kernel_constant(header, name):
    """An integer constant of a kernel header, products of integers and earlier constants resolved."""
    text = open(os.path.join(ROOT, "gr_baz_amd", "csrc", header)).read()
    expr = re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)
    value = 1
    for factor in expr.split("*"):
        factor = factor.strip()
        value *= int(factor) if factor.isdigit() else _kernel_constant(header, factor)
    return value


def _scene(m, nsamples, res, items):
    arr = mo.array_geometry(m) if m > 16 else sr.ula(m)       # (a uniform line where smoothing will run: its table passes smoothing_check)
    table = sr.table_of(arr, res) if m <= 16 else mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    x = mo.synth_items(items, m, nsamples, arr, mo.FREQUENCY, mo.SPACING, snr_db=20.0, seed=5200 + m)
    return table, x


class _Device:
    """process_device on the first `nb` items of one resident input; returns host copies of (ang, lvl, spectrum | None)."""

    def __init__(self, torch, dev, x, n, res):
        self.torch, self.n, self.res = torch, n, res
        self.x = torch.from_numpy(x.view(np.float32)).to(dev)
        self.ang = torch.zeros(x.shape[0], n, dtype=torch.float32, device=dev)
        self.lvl = torch.zeros_like(self.ang)
        self.spec = torch.zeros(x.shape[0], res, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()                    # the context launches on its own stream: fills first

    def __call__(self, ctx, nb, spectrum=True):
        ctx.process_device(self.x.data_ptr(), nb, self.ang.data_ptr(), self.lvl.data_ptr(), self.spec.data_ptr() if spectrum else None)
        ctx.sync()
        return (self.ang[:nb].cpu().numpy(), self.lvl[:nb].cpu().numpy(), self.spec[:nb].cpu().numpy() if spectrum else None)


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_every_buffer_comes_back(shape, gpu_device, monkeypatch):
    import torch
    from gr_baz_amd import capi
    m, n, N, res = SHAPES[shape]
    narrow, hostfed = m <= 16, m == 4
    table, x = _scene(m, N, res, 600 if hostfed else 300)
    if hostfed:
        monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")        # read at create: 600-item host-fed calls run in about six chunks
    gc.collect()                                               # (a context another test dropped without closing goes now, not midway)
    base = capi.live_buffers()
    ctx = capi.Context(m, n, N, res, table)
    try:
        run = _Device(torch, gpu_device, x, n, res)
        run(ctx, 70)
        run(ctx, 200)                                          # crosses the rounded capacity: every workspace regrows
        ctx.reserve(300)
        ctx.set_table(table)
        ctx.set_table(table)                                   # both table sets have been the one in force
        mid = capi.live_buffers()
        assert mid[0] > base[0] and mid[1] > base[1], "the tap does not count: %r at the start, %r with a context at work" % (base, mid)
        if narrow:
            ctx.set_order_mode("mdl")
            ctx.set_refine_mode(1)
            ctx.set_power_mode(2)
            ctx.set_beam_mode(1)
            ctx.set_peak_mode(1)
            ctx.set_averaging(3, 0.9)
            run(ctx, 200, spectrum=True)
            run(ctx, 200, spectrum=False)
            ctx.set_beam_mode(0)
            ctx.set_calibration(np.exp(0.1j * np.arange(m)).astype(np.complex64))
            ctx.set_noise_covariance(np.diag(1.0 + 0.1 * np.arange(m)).astype(np.complex128))
            ctx.calibrate(x[:70], table[res // 3])
            run(ctx, 200)
            ctx.set_calibration(None)
            ctx.set_noise_covariance(None)
            ctx.set_order_mode(None)
            ctx.set_refine_mode(0)
            ctx.set_estimator(capi.ESTIMATOR_CAPON)
            run(ctx, 200, spectrum=False)                      # the private spectrum
            ctx.set_estimator(capi.ESTIMATOR_MUSIC)
            ctx.set_power_mode(0)
            ctx.set_peak_mode(0)
            ctx.set_averaging(1, 1.0)
            ms = m - 1 if m <= 4 else (6 if m == 8 else 13)
            assert capi.smoothing_check(m, res, table, ms, False) is not None
            ctx.set_smoothing(ms, False)
            run(ctx, 200)
            ctx.process(x[:200])
            ctx.set_smoothing(m, False)
        if hostfed:
            ctx.process(x, want_spectrum=False)                # pageable: the two-slot path
            pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()
            xp = pin(x.view(np.float32)).view(np.complex64)
            out = tuple(pin(np.zeros((x.shape[0], k), np.float32)) for k in (n, n, res))
            ctx.process(xp, out=out)                           # page-locked with the spectrum port: four slots and the whole call's ang / lvl image
            ctx.process(xp[:64], out=tuple(a[:64] for a in out))     # one chunk on page-locked memory: the zero-copy path
        grown = capi.live_buffers()
        assert grown[0] >= mid[0] and grown[1] >= mid[1]      # (nothing the calls above allocated went before the context)
    finally:
        ctx.close()
    assert capi.live_buffers() == base


@pytest.mark.parametrize("shape", ["m4_fused_covevd_row_classes_coarse", "m17_wide_matrix_core_scan"])
def test_regrow_between_calls_changes_no_bit(shape, gpu_device):
    import torch
    from gr_baz_amd import capi
    m, n, N, res = SHAPES[shape]
    table, x = _scene(m, N, res, 200)
    with capi.Context(m, n, N, res, table) as ctx:
        run = _Device(torch, gpu_device, x, n, res)
        first = run(ctx, 64)
        run(ctx, 200)                                          # every workspace regrows
        third = run(ctx, 64)
    for a, b, what in zip(first, third, ("ang", "lvl", "spectrum")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s of the same 64 items differs behind a regrow" % what


def test_agc_buffers_come_back(gpu_device):
    """Two host-path calls; the second has more tiles (the per-tile tables regrow) and more samples (the staging regrows)."""
    from gr_baz_amd import agc
    tile = _kernel_constant("agc_kernels.hip.h", "AGC_IT")
    calls = (tile + 44, 3 * tile + 1)                          # 2 tiles, then 4
    rate = 1e-4
    x = scan_input(1, sum(calls))[0]
    ref = run_calls(ar.Agc(rate, SCAN_REFERENCE), x, calls)
    gc.collect()
    base = agc.debug_live_buffers()
    blk = agc.Agc(rate, SCAN_REFERENCE)
    try:
        got = run_calls(blk, x, calls)
        assert agc.debug_live_buffers()[0] > base[0]
    finally:
        blk.close()
    assert agc.debug_live_buffers() == base
    assert_agc_parity("two host-path calls", tuple(a[None, :] for a in got), tuple(a[None, :] for a in ref))


def test_resampler_buffers_come_back(gpu_device):
    """Two host-path calls of the two-input branch (it uses every buffer of a context); the second asks for more than two blocks
    of outputs and reads past the walk's first window, so the staging buffers and the phase tables regrow."""
    from gr_baz_amd import resamp
    per_block = _kernel_constant("resamp_kernels.hip.h", "RS_BLOCK") * _kernel_constant("resamp_kernels.hip.h", "RS_PER_THREAD")
    window = _kernel_constant("resamp_kernels.hip.h", "RS_WALK_WIN")
    lo, hi, S = 3.0, 5.0, 2
    calls = (300, 2 * per_block + 1)
    windows = tuple(int(c * hi) + 64 for c in calls)
    assert windows[1] > window > windows[0]
    rng = np.random.default_rng(78)
    L = sum(windows)
    x = (rng.standard_normal((S, L)) + 1j * rng.standard_normal((S, L))).astype(np.complex64)
    ratio = rng.uniform(lo, hi, L).astype(np.float32)
    gc.collect()
    base = resamp.debug_live_buffers()
    blk = resamp.Resampler(0.37, 1.0, nstreams=S)
    outs = []
    try:
        pos = 0
        for c, w in zip(calls, windows):
            out, k = blk.work(x[:, pos:pos + w], c, rr=ratio[pos:pos + w])
            outs.append((pos, w, c, out, k))
            pos += k
        assert resamp.debug_live_buffers()[0] > base[0]
    finally:
        blk.close()
    assert resamp.debug_live_buffers() == base
    oracles = [rr.Resampler(0.37, 1.0) for _ in range(S)]
    for pos, w, c, out, k in outs:
        assert out.shape == (S, c)
        for s in range(S):
            o, ks = oracles[s].work(x[s, pos:pos + w], c, rr=ratio[pos:pos + w])
            assert ks == k and np.array_equal(out[s].view(np.uint32), o.view(np.uint32))
