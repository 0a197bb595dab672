"""Rotation schedules of the fused m = 4 covariance + EVD kernel (cov4_evd_kernel / cov4_evd_order_kernel, section 2a of
music_kernels.hip.h).  The product rotates after every task.  The deferred form (lab: BAZ_MUSIC_COVEVD_DEFER=1) lets a wave
with more tasks to stream hold the R of up to COVEVD_PARK finished tasks in registers and run the rotation passes back to
back where its work ends; it gained nothing that clears a step's run-to-run spread (profiles/r06_covevd_deferred.txt) and
stays a lab switch.  Same function on the same values: every output must keep its bits under either schedule, whichever
of the two places (registers, the LDS table) an item's R waited in.

At the production grid a wave takes a second task only from 131,073 items on, so these tests use the lab library with
BAZ_MUSIC_COVEVD_BLOCKS=1 and BAZ_MUSIC_COVEVD_TASK_ITEMS=16: one workgroup of four waves walks every 16-item task, wave w
the tasks w, w + 4, w + 8, ...  The release library at the production grid (two tasks per wave at 262,144 items) is
exercised by `bench.py --full`'s own oracle check, not here.

The noise eigenvectors G go to a buffer of the context that no tap hands out: the out-of-batch test covers Q, the R tap and
the three outputs; a misplaced G store would show in the literal-form bins of the spectra the other tests compare."""
import os
import re

import numpy as np
import pytest

from helpers import assert_doa_match, assert_spectrum_close
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

M, NSAMPLES, RES = 4, 1024, 360
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _park():
    """COVEVD_PARK, the compile-time size of the held set"""
    with open(os.path.join(ROOT, "gr_baz_amd", "csrc", "music_kernels.hip.h")) as f:
        return int(re.search(r"constexpr int COVEVD_PARK = (\d+);", f.read()).group(1))


PARK = _park()
# one task per wave; two per wave; two plus a short task on one wave; 4/3/3/3 tasks with a short last one; five per wave; one more
# than a full held set plus the LDS-held task (a rotation of held tasks in the middle of the wave's work)
BATCHES = (64, 128, 131, 197, 320, 16 * 4 * (PARK + 2) + 5)
MAXB = max(BATCHES)

SHIPPED, DEFER, NODEFER, TWO_KERNELS = {}, {"BAZ_MUSIC_COVEVD_DEFER": "1"}, {"BAZ_MUSIC_COVEVD_DEFER": "0"}, {"BAZ_MUSIC_FUSE": "0"}
SCHEDULES = pytest.mark.parametrize("sched", [SHIPPED, DEFER], ids=["shipped", "deferred"])


@pytest.fixture(scope="module")
def scene():
    arr = mo.array_geometry(M)
    table = mo.steering_table_c64(arr, RES, mo.FREQUENCY, mo.SPACING)
    parts = [mo.synth_items((MAXB + 2) // 3, M, NSAMPLES, arr, mo.FREQUENCY, mo.SPACING, snr_db=snr, seed=6100 + i)
             for i, snr in enumerate((25.0, 10.0, 0.0))]
    items = np.stack(parts, axis=1).reshape(-1, NSAMPLES)[:MAXB]     # SNRs interleaved: every task has all three
    items.setflags(write=False)
    return {"table": table, "items": items}


def run(monkeypatch, gpu_device, table, items, n, env, order=None, pad=0):
    """One call of a fresh lab context under `env`: ang, lvl, spectrum, the R tap and (order mode) the per-item counts.
    pad: rows past the batch in every buffer, pre-filled with a sentinel and returned with the rest."""
    import torch
    from gr_baz_amd import capi
    for k in ("BAZ_MUSIC_COVEVD_DEFER", "BAZ_MUSIC_FUSE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BAZ_MUSIC_COVEVD_BLOCKS", "1")
    monkeypatch.setenv("BAZ_MUSIC_COVEVD_TASK_ITEMS", "16")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = items.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).to(gpu_device)
    ang = torch.full((B + pad, n), -7.0, dtype=torch.float32, device=gpu_device)
    lvl = torch.full((B + pad, n), -7.0, dtype=torch.float32, device=gpu_device)
    spec = torch.full((B + pad, RES), -7.0, dtype=torch.float32, device=gpu_device)
    R = torch.full((B + pad, 16, 2), -7.0, dtype=torch.float64, device=gpu_device)
    out = {}
    with capi.Context(M, n, NSAMPLES, RES, table, lab=True) as ctx:
        assert ("cov4_evd_kernel" in ctx.stage_name(0)) == (env is not TWO_KERNELS)
        if order:
            ctx.set_order_mode(order)
        ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
        ctx.sync()
        if order:
            out["orders"] = ctx.last_orders(B)
        ctx.debug_cov(x.data_ptr(), B, R.data_ptr())
        ctx.sync()
        if pad:
            qs = capi.q_stride(B)
            Q = torch.full((16 * qs + pad,), -7.0, dtype=torch.float64, device=gpu_device)
            ctx.debug_q(x.data_ptr(), B, Q.data_ptr())
            ctx.sync()
            out["Q"], out["qstride"] = Q.cpu().numpy(), qs
    out.update(ang=ang.cpu().numpy(), lvl=lvl.cpu().numpy(), spectrum=spec.cpu().numpy(), R=R.cpu().numpy())
    return out


def assert_same_bits(a, b, keys=("ang", "lvl", "spectrum", "R"), what=""):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_both_schedules_keep_the_bits_of_the_two_kernel_form(n, scene, gpu_device, monkeypatch):
    for B in BATCHES:
        items = scene["items"][:B]
        got = run(monkeypatch, gpu_device, scene["table"], items, n, DEFER)
        assert_same_bits(got, run(monkeypatch, gpu_device, scene["table"], items, n, TWO_KERNELS), what="batch %d vs two kernels" % B)
        assert_same_bits(got, run(monkeypatch, gpu_device, scene["table"], items, n, NODEFER), what="batch %d vs a phase per task" % B)
        assert_same_bits(got, run(monkeypatch, gpu_device, scene["table"], items, n, SHIPPED), what="batch %d vs the shipped schedule" % B)
        assert np.all(np.isfinite(got["spectrum"]))
        if B == 197:
            ao, lo, so, st = mo.music_doa_work_batch(items, scene["table"], M, n)
            assert_spectrum_close(got["spectrum"], so)
            assert_doa_match(got["ang"], got["lvl"], ao, lo, RES, st)


@SCHEDULES
@pytest.mark.parametrize("B", [131, 197])
def test_order_mode_twin_keeps_the_bits_and_the_counts(B, sched, scene, gpu_device, monkeypatch):
    items = scene["items"][:B]
    got = run(monkeypatch, gpu_device, scene["table"], items, 2, sched, order="mdl")
    ref = run(monkeypatch, gpu_device, scene["table"], items, 2, TWO_KERNELS, order="mdl")
    assert_same_bits(got, ref, keys=("ang", "lvl", "spectrum", "R", "orders"))
    assert got["orders"].shape == (B,) and got["orders"].max() <= 2


@SCHEDULES
def test_outputs_do_not_depend_on_where_an_item_waits(sched, scene, gpu_device, monkeypatch):
    """rolled by one and by three tasks, items change between a register-held task and the LDS-held one (wave w walks the
    tasks w, w + 4, ...: in the deferred form the tasks 0 .. 3 and 8 are held, 4 .. 7 and 9 .. 12 are not, at COVEVD_PARK = 1)"""
    items = scene["items"][:197]
    base = run(monkeypatch, gpu_device, scene["table"], items, 2, sched)
    for shift in (16, 48):
        got = run(monkeypatch, gpu_device, scene["table"], np.roll(items, shift, axis=0), 2, sched)
        for k in ("ang", "lvl", "spectrum", "R"):
            assert np.array_equal(np.roll(got[k], -shift, axis=0), base[k]), "rolled by %d: %s differs" % (shift, k)


@SCHEDULES
def test_poisoned_items_in_a_held_and_in_a_last_task(sched, scene, gpu_device, monkeypatch):
    """batch 128: wave 0 streams task 0 (items 0 .. 15; deferred: held in registers) and ends on task 4 (items 64 .. 79)"""
    clean_items = scene["items"][:128]
    items = clean_items.copy()
    items[3, 517] = np.nan
    items[70, 12] = np.inf
    clean = run(monkeypatch, gpu_device, scene["table"], clean_items, 2, sched)
    got = run(monkeypatch, gpu_device, scene["table"], items, 2, sched)
    bad = np.zeros(128, bool)
    bad[[3, 70]] = True
    assert np.all(np.isnan(got["spectrum"][bad]))
    assert np.all(got["ang"][bad] == 0.0) and np.all(got["lvl"][bad] == 0.0)
    for k in ("ang", "lvl", "spectrum", "R"):
        assert np.array_equal(got[k][~bad], clean[k][~bad]), k


@SCHEDULES
def test_nothing_is_written_past_the_batch(sched, scene, gpu_device, monkeypatch):
    B, pad = 131, 77
    got = run(monkeypatch, gpu_device, scene["table"], scene["items"][:B], 2, sched, pad=pad)
    for k in ("ang", "lvl", "spectrum", "R"):
        assert np.all(got[k][B:] == -7.0), k
        assert not np.any(got[k][:B] == -7.0), k
    qs = got["qstride"]
    Q = got["Q"]
    rows = Q[:16 * qs].reshape(16, qs)
    assert np.all(rows[:, B:] == -7.0) and np.all(Q[16 * qs:] == -7.0)
    assert not np.any(rows[:, :B] == -7.0)
