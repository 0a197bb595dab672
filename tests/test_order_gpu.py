"""Opt-in per-item emitter-count estimate (baz_music_set_order_mode) on the MI355X: the counts against order_ref on the
device's own covariance for every Jacobi home, spectrum / DoA of every item against the fp64 oracle at that item's count on
every scan the mode can reach, mixed batches, mode off == the reference bit for bit, composition with peak mode and
smoothing, poisoned items, and mode changes beside a submitting thread."""
import threading

import numpy as np
import pytest

import order_ref as oref
import smoothing_ref as sr
from helpers import (EPS64, I8_EPS, RCP_ULPS, ULP32, assert_doa_within_bound, assert_spectrum_within_bound, oracle_fp64)
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _mixed(m, K, counts, per, sigma, seed, arr=None, grid=None):
    """`per` items of every emitter count in `counts`, in seeded random order: (items, emitters per item)."""
    parts = [oref.scene(per, m, K, e, sigma, seed + 17 * e, arr=arr, grid=grid)[0] for e in counts]
    truth = np.repeat(np.asarray(counts), per)
    order = np.random.default_rng(seed).permutation(len(truth))
    return np.concatenate(parts)[order], truth[order]


def _device_cov(ctx, items, m):
    """R of every item as the context's own covariance stage computes it (debug_cov), (B, m, m) complex128."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _assert_counts(orders, R, K, n_max, crit, what=""):
    """orders == order_ref on the eigenvalues of R, except items whose criterion gap is below GAP_RTOL (at most GAP_CAP of
    them, at least one allowed in a small batch never: the cap is floor(GAP_CAP * B))."""
    Rh = 0.5 * (R + R.conj().transpose(0, 2, 1))
    k_ref, gap = oref.estimate(np.linalg.eigvalsh(Rh), K, n_max, crit, with_gap=True)
    close = gap < oref.GAP_RTOL
    assert close.sum() <= int(oref.GAP_CAP * len(orders)), "%s: %d items at a gap below %.0e" % (what, close.sum(), oref.GAP_RTOL)
    bad = np.nonzero((orders != k_ref) & ~close)[0]
    assert bad.size == 0, "%s item %d: device %d, order_ref %d (gap %.3g)" % (what, bad[0], orders[bad[0]], k_ref[bad[0]], gap[bad[0]])
    return k_ref


def _assert_outputs(items, table, m, n_max, orders, ang, lvl, spec, path):
    """Every item against the fp64 oracle at ITS count: spectrum and DoA within the path's own bound, (0, 0) at and beyond the
    count, 1 / ||a||^2 for count 0."""
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    a2 = np.sum(A.real ** 2 + A.imag ** 2, axis=1)
    for k in np.unique(orders):
        idx = np.nonzero(orders == k)[0]
        assert np.all(ang[idx, k:] == 0.0) and (lvl is None or np.all(lvl[idx, k:] == 0.0)), "entries beyond count %d" % k
        if k == 0:
            if spec is not None:
                # Q = I: d = sum_i |a_i|^2 in the projector form (m^2 eps ||a||^2), one float reciprocal; + the int8 form's eps
                tol = RCP_ULPS * ULP32 + m * m * EPS64 + (I8_EPS if path == "int8" else 0.0)
                err = np.abs(spec[idx].astype(np.float64) * a2[None, :] - 1.0)
                assert err.max() <= tol, "count 0: spectrum vs 1/||a||^2: %.3g > %.3g" % (err.max(), tol)
            continue
        a_ref, _, _, s64, w = oracle_fp64(items[idx], table, m, int(k))
        if spec is not None:
            assert_spectrum_within_bound(spec[idx], s64, path, m, int(k), table, w, ill_posed_ok=True, what="count %d" % k)
        assert_doa_within_bound(ang[idx, :k], None if lvl is None else lvl[idx, :k], a_ref, s64, path, m, int(k), table, w,
                                ill_posed_ok=True)
        if lvl is not None:
            assert np.all(lvl[idx, :k] > 0.0)


# name, m, K, n_max, emitter counts in the batch, array (None: line array), environment, expected scan with the spectrum port
HOMES = [
    ("m2_unfused", 2, 64, 1, (0, 1), None, {}, "fp64"),
    ("m3_unfused", 3, 64, 2, (0, 1, 2), None, {}, "fp64"),
    ("m4_unfused", 4, 64, 3, (0, 1, 2, 3), mo.array_geometry(4), {}, "fp64"),
    ("m4_fused", 4, 256, 2, (0, 1, 2), mo.array_geometry(4), {}, "fp64"),
    ("m5_lds", 5, 64, 2, (0, 1, 2), None, {}, "fp64"),
    ("m8_lds_i8", 8, 64, 4, (0, 1, 2, 3), None, {}, "int8"),                   # n = 4 of 8: orthogonal iteration with the mode off
    ("m8_lds_fp64", 8, 64, 4, (0, 1, 2, 3), None, {"BAZ_MUSIC_EXACT": "1"}, "fp64"),
    ("m12_lds_short_form", 12, 64, 2, (0, 1, 2), None, {"BAZ_MUSIC_EXACT": "1"}, "fp64"),   # n = 2, m >= 9: the short form
    ("m6_lds_short_form_n1", 6, 64, 1, (0, 1), None, {"BAZ_MUSIC_EXACT": "1"}, "fp64"),
    ("m16_lds_i8", 16, 256, 3, (0, 1, 2, 3), None, {}, "int8"),                # n = 3 of 16: orthogonal iteration with the mode off
]


@pytest.mark.parametrize("crit", ["mdl", "aic"])
@pytest.mark.parametrize("name,m,K,n_max,counts,arr,env,path", HOMES, ids=[h[0] for h in HOMES])
def test_counts_and_outputs_per_evd_home(name, m, K, n_max, counts, arr, env, path, crit, gpu_device, monkeypatch):
    """A mixed batch (0 .. n_max emitters in seeded random order: nothing wave-uniform may be assumed) through the host-fed
    entry point with and without the spectrum port (without it, up to 8 antennas would take the coarse-gated scan: the mode
    routes them to the full scan) and through the device entry point."""
    import torch
    capi = _capi()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = 360
    arr = oref.ula(m) if arr is None else arr
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = _mixed(m, K, counts, 23, 0.1, seed=1000 + m + K, arr=arr)           # 23 per count: ragged waves
    B = len(items)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        assert ctx.get_order_mode() is None
        ctx.set_order_mode(crit)
        assert ctx.get_order_mode() == crit
        assert ctx.uses_i8_scan() == (path == "int8")
        ang, lvl, spec = ctx.process(items)
        orders = ctx.last_orders(B)
        assert len(orders) == B
        R = _device_cov(ctx, items, m)
        assert np.array_equal(ctx.last_orders(B), orders)                          # (the tap's EVD keeps its counts elsewhere)
        _assert_counts(orders, R, K, n_max, crit, name)
        assert len(np.unique(orders)) >= 2
        _assert_outputs(items, table, m, n_max, orders, ang, lvl, spec, path)
        # without the spectrum port
        ang0, lvl0, _ = ctx.process(items, want_spectrum=False)
        assert np.array_equal(ctx.last_orders(B), orders)
        nospec_path = path if (m > 8 or path == "fp64") else "fp64"                # 6 .. 8 antennas without port 2: the fp64 scan
        _assert_outputs(items, table, m, n_max, orders, ang0, lvl0, None, nospec_path)
        # device entry point, last_orders_device
        x = torch.from_numpy(items.view(np.float32)).cuda()
        d_ang = torch.full((B, n_max), 7.0, dtype=torch.float32, device="cuda")
        d_lvl = torch.full((B, n_max), 7.0, dtype=torch.float32, device="cuda")
        d_spec = torch.zeros(B, res, dtype=torch.float32, device="cuda")
        ctx.process_device(x.data_ptr(), B, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
        ptr = ctx.last_orders_device()
        assert ptr != 0

        class _Bytes:
            __cuda_array_interface__ = {"shape": (B,), "typestr": "|u1", "data": (ptr, False), "version": 2}

        dev_orders = torch.as_tensor(_Bytes(), device="cuda").cpu().numpy()
        ctx.sync()
        assert np.array_equal(ctx.last_orders(B), orders) and np.array_equal(dev_orders, orders)
        assert np.array_equal(d_ang.cpu().numpy(), ang) and np.array_equal(d_lvl.cpu().numpy(), lvl)
        assert np.array_equal(d_spec.cpu().numpy(), spec)
        # the projector tap returns the variable-rank projector: trace = m - count
        Q = torch.zeros(m * m * capi.q_stride(B), dtype=torch.float64, device="cuda")
        ctx.debug_q(x.data_ptr(), B, Q.data_ptr())
        ctx.sync()
        q = Q.cpu().numpy().reshape(m * m, -1)[:, :B]
        trace = sum(q[i * m + i] for i in range(m))
        assert np.allclose(trace, m - orders.astype(np.float64), atol=1e-9)


def test_chunked_host_call_reports_every_item(gpu_device, monkeypatch):
    capi = _capi()
    monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")                                 # ~300 items per chunk at this shape
    m, K, n_max, res = 4, 64, 3, 360
    arr = mo.array_geometry(4)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = _mixed(m, K, (0, 1, 2, 3), 250, 0.1, seed=77, arr=arr)               # 1,000 items: four chunks
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ang, lvl, spec = ctx.process(items)
        orders = ctx.last_orders(len(items))
        assert len(orders) == len(items)
        assert np.array_equal(ctx.last_orders(10), orders[:10])
        _assert_counts(orders, _device_cov(ctx, items, m), K, n_max, "mdl", "chunked")
        _assert_outputs(items, table, m, n_max, orders, ang, lvl, spec, "fp64")
    monkeypatch.delenv("BAZ_MUSIC_CHUNK_MIB")
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        one = ctx.process(items)
        assert np.array_equal(ctx.last_orders(len(items)), orders)
        for a, b in zip(one, (ang, lvl, spec)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name,m,K,n_max,env,path", [("m4_fp64", 4, 256, 2, {}, "fp64"), ("m8_i8", 8, 64, 3, {}, "int8"),
                                                     ("m12_short", 12, 64, 2, {"BAZ_MUSIC_EXACT": "1"}, "fp64")])
def test_literal_refinement_at_60_db(name, m, K, n_max, env, path, gpu_device, monkeypatch):
    """sigma = 1e-3, emitters on the table's bins: the nulls fall below the projector form's threshold and the scans recompute
    them in the literal form over the zero-padded noise vectors; still the oracle's values at every item's own count."""
    capi = _capi()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = 720
    arr = mo.array_geometry(4) if m == 4 else oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = _mixed(m, K, tuple(range(n_max + 1)), 20, 1e-3, seed=60 + m, arr=arr, grid=360.0 / res)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ang, lvl, spec = ctx.process(items)
        refined = ctx.refined_values()
        orders = ctx.last_orders(len(items))
        _assert_counts(orders, _device_cov(ctx, items, m), K, n_max, "mdl", name)
        assert refined > 0, "no value took the literal form"
        _assert_outputs(items, table, m, n_max, orders, ang, lvl, spec, path)
        ang0, lvl0, _ = ctx.process(items, want_spectrum=False)
        _assert_outputs(items, table, m, n_max, orders, ang0, lvl0, None, path if m > 8 else "fp64")


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=92)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs = []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_order_mode(None)
            if how == "on_then_off":
                ctx.set_order_mode("mdl")
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                ctx.set_order_mode(None)
            assert ctx.get_order_mode() is None
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            assert np.array_equal(ctx.last_orders(batch), np.full(batch, n, np.uint8))    # off: every item used n
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_peak_mode_gives_the_strongest_local_maxima(gpu_device):
    capi = _capi()
    m, K, n_max, res = 8, 64, 4, 720
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = _mixed(m, K, (0, 1, 2, 3), 16, 0.1, seed=5)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.set_peak_mode(1)
        ang, lvl, spec = ctx.process(items)
        orders = ctx.last_orders(len(items))
        ang0, lvl0, _ = ctx.process(items, want_spectrum=False)
    assert set(np.unique(orders)) == {0, 1, 2, 3}
    for b in range(len(items)):
        k = int(orders[b])
        pa, pl = mo.peak_pick(spec[b], n_max, res)
        assert np.array_equal(ang[b, :k], pa[:k]) and np.array_equal(lvl[b, :k], pl[:k]), b
        assert np.all(ang[b, k:] == 0) and np.all(lvl[b, k:] == 0), b
    assert np.array_equal(ang0, ang) and np.array_equal(lvl0, lvl)


def test_smoothing_recovers_the_count_of_a_coherent_pair(gpu_device):
    """The coherent pair of test_smoothing_gpu.py (8-element line array, K = 64, sigma = 0.1).  Plain: the pair's signal
    covariance has rank 1 and the count is 1 (recorded: order_ref gives 1 in 200 of 200 items).  FB + SS(6): 2, with N = the
    outer K = 64 in the criterion -- equal to order_ref on the re-stacked items' covariance with that N."""
    capi = _capi()
    res, m, n_max, K, ms = 720, 8, 3, 64, 6
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = sr.two_emitters(200, arr, K, coherent=True, seed=2024)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.process(items, want_spectrum=False)
        plain = ctx.last_orders(len(items))
        ctx.set_smoothing(ms, True)
        assert ctx.get_order_mode() == "mdl"
        path = "int8" if ctx.uses_i8_scan() else "fp64"
        ang, lvl, spec = ctx.process(items)
        smooth = ctx.last_orders(len(items))
        # (switching the criterion while smoothing is on reaches the inner context)
        ctx.set_order_mode("aic")
        ctx.process(items[:8])
        aic = ctx.last_orders(8)
    print("coherent pair: share of count 2 plain %.3f, FB+SS(6) %.3f" % (np.mean(plain == 2), np.mean(smooth == 2)))
    assert np.all(smooth == 2), np.bincount(smooth)
    assert np.mean(plain == 1) > 0.9
    y = sr.restack(items, m, ms, True, capi.smoothing_check(m, res, table, ms, True))
    k_ref, gap = oref.estimate(oref.eigvals(y, ms), K, n_max, "mdl", with_gap=True)
    assert gap.min() > 1e-3 and np.array_equal(smooth, k_ref)
    assert np.array_equal(aic, oref.estimate(oref.eigvals(y[:8], ms), K, n_max, "aic"))
    sub = table[:, :ms]
    a_ref, _, _, s64, w = oracle_fp64(y, sub, ms, 2)
    assert_spectrum_within_bound(spec, s64, path, ms, 2, sub, w, ill_posed_ok=True)
    assert_doa_within_bound(ang[:, :2], lvl[:, :2], a_ref, s64, path, ms, 2, sub, w, ill_posed_ok=True)
    assert np.all(ang[:, 2:] == 0) and np.all(lvl[:, 2:] == 0)


@pytest.mark.parametrize("m,K,n_max", [(4, 256, 2), (4, 64, 2), (8, 64, 3)])
def test_poisoned_and_zero_items(m, K, n_max, gpu_device):
    capi = _capi()
    res = 360
    arr = mo.array_geometry(4) if m == 4 else oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(70, m, K, 1, 0.1, seed=3, arr=arr)
    items[5] = 0
    items[17, 3] = np.nan
    items[40, 9] = np.inf
    items[69] = 0
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ang, lvl, spec = ctx.process(items)
        orders = ctx.last_orders(70)
        ang0, lvl0, _ = ctx.process(items, want_spectrum=False)
    special = [5, 17, 40, 69]
    assert np.all(orders[special] == 0)
    assert np.all(np.delete(orders, special) == 1)
    for a, l in ((ang, lvl), (ang0, lvl0)):
        assert np.all(a[special] == 0) and np.all(l[special] == 0)
        assert np.all(np.delete(l, special, axis=0)[:, 0] > 0)
    assert np.all(np.isnan(spec[[17, 40]]))
    a2 = np.sum(np.abs(table.astype(np.complex128)) ** 2, axis=1)
    assert np.allclose(spec[[5, 69]] * a2[None, :], 1.0, rtol=0, atol=1e-5)
    assert np.all(np.isfinite(np.delete(spec, [17, 40], axis=0)))


def test_wide_arrays_are_refused(gpu_device):
    capi = _capi()
    m = 24
    table = mo.steering_table_c64(oref.ula(m), 360, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, 2, m * 32, 360, table) as ctx:
        with pytest.raises(capi.MusicError) as e:
            ctx.set_order_mode("mdl")
        assert e.value.code == capi.E_UNSUPPORTED
        assert ctx.get_order_mode() is None
        ctx.set_order_mode(None)
        with pytest.raises(ValueError):
            ctx.set_order_mode("bic")
        assert capi.lib().baz_music_set_order_mode(ctx._h, 3) == capi.E_INVALID


def test_profile_and_stage_names_keep_working(gpu_device):
    capi = _capi()
    m, K, res = 8, 64, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(64, m, K, 2, 0.1, seed=8)
    with capi.Context(m, 3, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.profile(1)
        ctx.process(items)
        for stage in range(4):
            ms_, launches = ctx.stage_ms(stage)
            assert launches >= 1 and ms_ > 0.0, stage
            assert ctx.stage_name(stage)


def test_mode_changes_beside_a_submitting_thread(gpu_device):
    """One emitter, n = 2: with the mode off every item reports two bins (lvl > 0 twice), with MDL on one pair and (0, 0).  A
    second thread flips the mode while this one submits: every batch is all of one kind."""
    capi = _capi()
    m, K, res = 4, 256, 360
    arr = mo.array_geometry(4)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(256, m, K, 1, 0.1, seed=12, arr=arr)
    stop = threading.Event()
    errors = []

    def flip(ctx):
        i = 0
        try:
            while not stop.is_set():
                ctx.set_order_mode("mdl" if i % 2 == 0 else None)
                i += 1
        except Exception as e:       # noqa: BLE001
            errors.append(e)

    kinds = set()
    with capi.Context(m, 2, m * K, res, table) as ctx:
        t = threading.Thread(target=flip, args=(ctx,))
        t.start()
        try:
            for _ in range(60):
                ang, lvl, _ = ctx.process(items, want_spectrum=False)
                orders = ctx.last_orders(len(items))
                second = lvl[:, 1] > 0
                assert second.all() or not second.any(), "a batch mixes the two modes"
                # (the mode may have flipped again before last_orders; its answer is still all of one kind)
                assert np.all(orders == (2 if second.all() else 1))
                kinds.add(bool(second.all()))
        finally:
            stop.set()
            t.join()
    assert not errors, errors
    print("batches seen with the mode off / on:", kinds)
