"""The 17 .. 64 antenna sequence across more than one pass (GPU): wide_pass_items caps a pass at 8,192 items, so a call of 8,197 items
runs as two passes, the second of 5 items.  One call must equal the same context run as two calls of 8,192 and 5 items, bit for bit,
on either wide scan and with the averaging history and the whitening stage running across the pass boundary."""
import functools

import numpy as np
import pytest

from helpers import assert_doa_match, assert_doa_within_bound, assert_spectrum_close, assert_spectrum_within_bound, oracle_fp64
from oracle import music_oracle as mo
from whiten_ref import hpd

pytestmark = pytest.mark.gpu

M, N_EMIT, K, RES = 17, 2, 8, 90
NSAMPLES = M * K
PASS, TAIL = 8192, 5
BATCH = PASS + TAIL
HEAD = 64                 # items held to the oracle: the first HEAD and the last TAIL (both sides of the pass boundary)
SHARP = slice(4096, 4128)


@functools.lru_cache(maxsize=None)
def _scene():
    """items (BATCH, NSAMPLES) complex64 as in test_wide_arrays_match_the_oracle, the table, and the oracle of the items it is asked on"""
    arr = mo.array_geometry(M)
    table = mo.steering_table_c64(arr, RES, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(BATCH, M, NSAMPLES, arr, mo.FREQUENCY, mo.SPACING, angles_deg=tuple(np.linspace(17.0, 311.0, N_EMIT)),
                           snr_db=20.0, seed=100 * M + N_EMIT)
    # ... and in the middle of the first pass, away from the items held to the oracle, emitters exactly on bins at 80 dB as in
    # test_wide_arrays_matrix_core_scan: nulls so deep that the matrix-core scan recomputes values (a non-zero statistic)
    sharp = tuple(np.round(np.linspace(0.13, 0.71, N_EMIT) * RES) * 360.0 / RES)
    items[SHARP] = mo.synth_items(SHARP.stop - SHARP.start, M, NSAMPLES, arr, mo.FREQUENCY, mo.SPACING, angles_deg=sharp, snr_db=80.0,
                                  seed=9 * M + N_EMIT)
    asked = np.r_[0:HEAD, BATCH - TAIL:BATCH]
    sub = items[asked]
    return items, table, asked, mo.music_doa_work_batch(sub, table, M, N_EMIT), oracle_fp64(sub, table, M, N_EMIT)


def _run(ctx, x, calls, want_spec, gpu_device):
    """`calls` (item counts) process_device calls over consecutive slices of x: (ang, lvl, spec | None, refined values of each call)"""
    import torch
    ang = torch.full((BATCH, N_EMIT), -1.0, dtype=torch.float32, device=gpu_device)
    lvl = torch.full((BATCH, N_EMIT), -1.0, dtype=torch.float32, device=gpu_device)
    spec = torch.full((BATCH, RES), -1.0, dtype=torch.float32, device=gpu_device) if want_spec else None
    stream = torch.cuda.current_stream().cuda_stream
    refined, off = [], 0
    for nb in calls:
        ctx.process_device(x[off].data_ptr(), nb, ang[off].data_ptr(), lvl[off].data_ptr(), spec[off].data_ptr() if want_spec else None,
                           stream=stream)
        ctx.sync()
        refined.append(ctx.refined_values())
        off += nb
    assert off == BATCH
    return ang.cpu().numpy(), lvl.cpu().numpy(), spec.cpu().numpy() if want_spec else None, refined


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _one_call_against_two(gpu_device, want_spec, lab=False, averaging=None, rn=None):
    import torch
    from gr_baz_amd import capi
    items, table, _, _, _ = _scene()
    x = torch.from_numpy(items.view(np.float32)).to(gpu_device)
    with capi.Context(M, N_EMIT, NSAMPLES, RES, table, lab=lab) as ctx:
        if rn is not None:
            ctx.set_noise_covariance(rn)
        if averaging:
            ctx.set_averaging(*averaging)
        one = _run(ctx, x, (BATCH,), want_spec, gpu_device)
        if averaging:
            ctx.reset_averaging()        # both runs start at the first item of a stream
        two = _run(ctx, x, (PASS, TAIL), want_spec, gpu_device)
        scan = ctx.stage_name(2)
    assert _same_bits(one[0], two[0]) and _same_bits(one[1], two[1])
    assert (one[2] is None and two[2] is None) or _same_bits(one[2], two[2])
    print("refined values: one call %s, two calls %s" % (one[3], two[3]))
    assert one[3][0] == sum(two[3])
    return one, scan


def _assert_meets_the_oracle(ang, lvl, spec):
    """what test_wide_arrays_match_the_oracle asserts at this shape, on the items the oracle was asked on"""
    _, table, asked, (ao, lo, so, st), (ao64, _, _, s64, w) = _scene()
    if spec is not None:
        assert_spectrum_close(spec[asked], so)
        _, tight, _ = assert_spectrum_within_bound(spec[asked], s64, "fp64", M, N_EMIT, table, w)
        assert tight >= 0.9, tight
    assert_doa_match(ang[asked], lvl[asked], ao, lo, RES, st)
    assert_doa_within_bound(ang[asked], lvl[asked], ao64, s64, "fp64", M, N_EMIT, table, w)


@pytest.mark.parametrize("want_spec", [True, False], ids=["spectrum_wired", "spectrum_not_wired"])
def test_two_passes_equal_two_calls_and_meet_the_oracle(want_spec, gpu_device):
    (ang, lvl, spec, refined), scan = _one_call_against_two(gpu_device, want_spec)
    assert scan.endswith("scan_wide_mfma_kernel")
    assert refined[0] > 0         # (the sum over the calls asserted above is not 0 = 0 + 0)
    _assert_meets_the_oracle(ang, lvl, spec)


@pytest.mark.parametrize("want_spec", [True, False], ids=["spectrum_wired", "spectrum_not_wired"])
def test_two_passes_of_the_plain_scan_equal_two_calls_and_meet_the_oracle(want_spec, gpu_device, monkeypatch):
    monkeypatch.setenv("BAZ_MUSIC_WIDE_MFMA", "0")
    (ang, lvl, spec, _), scan = _one_call_against_two(gpu_device, want_spec, lab=True)
    assert scan.endswith("scan_wide_kernel")
    _assert_meets_the_oracle(ang, lvl, spec)


@pytest.mark.parametrize("want_spec", [True, False], ids=["spectrum_wired", "spectrum_not_wired"])
@pytest.mark.parametrize("averaging,whiten", [((4, 0.7), False), (None, True), ((4, 0.7), True)],
                         ids=["averaging", "whitening", "averaging_and_whitening"])
def test_the_stages_between_covariance_and_evd_run_across_the_pass_boundary(averaging, whiten, want_spec, gpu_device):
    """averaging: item 8,192 of the one call averages over the last three items of the first pass"""
    _one_call_against_two(gpu_device, want_spec, averaging=averaging, rn=hpd(M, 1234) if whiten else None)
