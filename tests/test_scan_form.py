"""The scan's decision table (scan_form in gr_baz_amd/csrc/baz_music_hip.hip), pinned through the ABI's own
introspection: which of scan_mfma_kernel / scan_i8_kernel / scan_coarse_kernel a launch takes for a shape, a port wiring and a
setting -- stage_name(2) after a process_device call, uses_i8_scan() -- and that the call's angles are the fp64 oracle's.

Shapes are the smallest that reach every branch: 17 items (a partial 16-item row group), 16 snapshots, 360 bins (vectorised
spectrum stores; one row at 361 for the scalar-store instantiation).

Two rows do not pick the reference's n strongest bins, by their mode's definition, and are compared with what the mode
defines instead (same helper, same bound):
  set_peak_mode(1)   the n strongest circular local maxima (oracle.music_oracle.peak_pick) of the oracle's spectrum;
  set_order_mode(1)  the per-item count decides how many entries are kept: the scene is one where every count is n (MDL's
                     runner-up lies > 80 % away in tests/order_ref.py), which the row asserts before it compares."""
import functools

import numpy as np
import pytest

from helpers import assert_doa_within_bound, oracle_fp64
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

BATCH, K = 17, 16


@functools.lru_cache(maxsize=None)
def _scene(m, n, res):
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(BATCH, m, m * K, arr, mo.FREQUENCY, mo.SPACING, angles_deg=tuple(np.linspace(23.0, 301.0, n)),
                           snr_db=20.0, seed=4000 + 17 * m + n)
    for a in (table, items):
        a.setflags(write=False)
    return table, items, oracle_fp64(items, table, m, n)


# (m, n, spectrum port wired, setting, kernel)
ROWS = [
    (4, 2, True, None, "scan_mfma_kernel<4,"),
    (4, 2, True, "res361", "scan_mfma_kernel<4,"),
    (4, 2, False, None, "scan_coarse_kernel<4,"),
    (4, 2, False, "BAZ_MUSIC_COARSE=0", "scan_mfma_kernel<4,"),
    (4, 2, False, "order", "scan_mfma_kernel<4,"),
    (4, 2, False, "peak", "scan_mfma_kernel<4,"),
    (5, 2, True, None, "scan_mfma_kernel<5,"),
    (5, 2, False, None, "scan_coarse_kernel<5,"),
    (8, 2, True, None, "scan_i8_kernel<8,"),
    (8, 2, False, None, "scan_coarse_kernel<8,"),
    (8, 2, False, "BAZ_MUSIC_COARSE=0", "scan_mfma_kernel<8,"),
    (8, 2, True, "BAZ_MUSIC_EXACT=1", "scan_mfma_kernel<8,"),
    (6, 1, False, None, "scan_i8_kernel<6,"),
    (6, 1, False, "BAZ_MUSIC_EXACT=1", "scan_mfma_kernel<6,"),
    (8, 5, False, None, "scan_mfma_kernel<8,"),
    (12, 2, False, None, "scan_i8_kernel<12,"),
    (12, 2, False, "BAZ_MUSIC_EXACT=1", "scan_mfma_kernel<12,"),
]


def _row_id(r):
    return "m%d-n%d-%s%s" % (r[0], r[1], "spec" if r[2] else "nospec", "-" + r[3] if r[3] else "")


@pytest.mark.parametrize("m,n,spec,setting,kernel", ROWS, ids=[_row_id(r) for r in ROWS])
def test_scan_kernel_by_shape_wiring_and_setting(m, n, spec, setting, kernel, gpu_device, monkeypatch):
    import torch
    from gr_baz_amd import capi
    for name in ("BAZ_MUSIC_COARSE", "BAZ_MUSIC_EXACT"):
        monkeypatch.delenv(name, raising=False)
    if setting and "=" in setting:
        monkeypatch.setenv(*setting.split("="))
    res = 361 if setting == "res361" else 360
    table, items, (ao, lo, so, s64, w) = _scene(m, n, res)
    x = torch.from_numpy(items.view(np.float32).copy()).to(gpu_device)
    ang = torch.full((BATCH, n), -1.0, dtype=torch.float32, device=gpu_device)
    lvl = torch.full((BATCH, n), -1.0, dtype=torch.float32, device=gpu_device)
    sp = torch.full((BATCH, res), -1.0, dtype=torch.float32, device=gpu_device) if spec else None
    with capi.Context(m, n, m * K, res, table) as ctx:
        if setting == "order":
            ctx.set_order_mode("mdl")
        if setting == "peak":
            ctx.set_peak_mode(1)
        ctx.process_device(x.data_ptr(), BATCH, ang.data_ptr(), lvl.data_ptr(), sp.data_ptr() if spec else None,
                           stream=torch.cuda.current_stream().cuda_stream)
        ctx.sync()
        name = ctx.stage_name(2)
        uses_i8 = ctx.uses_i8_scan()
        orders = ctx.last_orders(BATCH) if setting == "order" else None
    assert name == "bazmusic::" + kernel, name
    assert uses_i8 == (setting != "BAZ_MUSIC_EXACT=1" and 6 <= m and n <= 4)
    ref = ao
    if setting == "peak":
        ref = np.stack([mo.peak_pick(so[b], n)[0] for b in range(BATCH)])
    if setting == "order":
        assert np.all(np.asarray(orders) == n), orders
    path = "int8" if kernel.startswith("scan_i8_kernel") else "fp64"
    assert_doa_within_bound(ang.cpu().numpy(), lvl.cpu().numpy(), ref, s64, path, m, n, table, w)


@pytest.mark.parametrize("m,n,kernel", [(8, 2, "scan_i8_kernel<8,"), (4, 2, "scan_mfma_kernel<4,")])
def test_scan_kernel_named_before_the_first_launch(m, n, kernel, gpu_device, monkeypatch):
    """A fresh context answers with what a call WITH the spectrum port would take."""
    from gr_baz_amd import capi
    for name in ("BAZ_MUSIC_COARSE", "BAZ_MUSIC_EXACT"):
        monkeypatch.delenv(name, raising=False)
    table = _scene(m, n, 360)[0]
    with capi.Context(m, n, m * K, 360, table) as ctx:
        assert ctx.stage_name(2) == "bazmusic::" + kernel
