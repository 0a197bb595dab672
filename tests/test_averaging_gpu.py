"""Opt-in covariance averaging across stream items (baz_music_set_averaging) on the MI355X: the boxcar against the reference's own
arithmetic on the concatenated items for every frontend, the averaging stage alone against the restatement at a derived tolerance,
exponential weights end to end, bitwise independence of how the stream is cut, history semantics, off == the reference bit for
bit, composition with the other opt-in modes, the effect table on the device, and mode changes beside a submitting thread."""
import threading

import numpy as np
import pytest

import averaging_ref as aref
import order_ref as oref
import refine_ref as rr
import smoothing_ref as sr
from helpers import assert_doa_within_bound, assert_spectrum_within_bound, oracle_fp64
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _stream(ctx, items, cuts=None, want_lvl=True, want_spec=True):
    """The items through device-resident calls of the given sizes (None: one call): (ang, lvl | None, spec | None)."""
    import torch
    B = len(items)
    cuts = [B] if cuts is None else list(cuts)
    assert sum(cuts) == B
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    ang = torch.full((B, ctx.n), -1.0, dtype=torch.float32, device="cuda")
    lvl = torch.full((B, ctx.n), -1.0, dtype=torch.float32, device="cuda") if want_lvl else None
    spec = torch.full((B, ctx.res), -1.0, dtype=torch.float32, device="cuda") if want_spec else None
    torch.cuda.synchronize()
    done = 0
    for nb in cuts:
        ctx.process_device(x[done].data_ptr(), nb, ang[done].data_ptr(), lvl[done].data_ptr() if want_lvl else None,
                           spec[done].data_ptr() if want_spec else None)
        done += nb
    ctx.sync()
    return ang.cpu().numpy(), lvl.cpu().numpy() if want_lvl else None, spec.cpu().numpy() if want_spec else None


def _path(ctx):
    return "int8" if ctx.stage_name(2).startswith("bazmusic::scan_i8_kernel") else "fp64"


def _assert_concat_oracle(items, table, m, n, W, ang, lvl, spec, path, first=0):
    """Every item t >= first against the fp64 oracle of the concatenated item [X_{t-c+1} .. X_t], with the comparison and the
    per-path bound tests/test_path_accuracy.py applies (K < m: where the bound is defined).  Returns the worst err / tol."""
    worst = 0.0
    K = items.shape[1] // m
    for c, idx, cat in aref.windows(items, W):
        keep = idx >= first
        if not keep.any():
            continue
        idx, cat = idx[keep], cat[keep]
        a_ref, _, _, s64, w = oracle_fp64(cat, table, m, n)
        ill = c * K < m
        if spec is not None:
            worst = max(worst, assert_spectrum_within_bound(spec[idx], s64, path, m, n, table, w, ill_posed_ok=ill,
                                                            what="items with %d taps" % c)[0])
        worst = max(worst, assert_doa_within_bound(ang[idx], None if lvl is None else lvl[idx], a_ref, s64, path, m, n, table, w,
                                                   ill_posed_ok=ill))
    return worst


def _scene(m, n, nsamples, res, batch, seed, snr_db=20.0):
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    angles = (40.3, 121.7)[:n] if n <= 2 else tuple(np.linspace(23.0, 301.0, n))
    return table, mo.synth_items(batch, m, nsamples, arr, mo.FREQUENCY, mo.SPACING, angles_deg=angles, snr_db=snr_db, seed=seed)


# ---- 1. the boxcar against the reference's own arithmetic -------------------------------------------------------------------------
BOXCAR = [
    # name, m, n, nsamples, res, W, items, spectrum port, expected covariance / scan kernel while the mode is on
    ("m4_two_kernels", 4, 2, 64, 360, 4, 40, True, "bazmusic::cov_mfma_kernel<4>", "bazmusic::scan_mfma_kernel<4,"),
    ("m4_fused_shape", 4, 2, 1024, 360, 3, 20, True, "bazmusic::cov4_x4_kernel", "bazmusic::scan_mfma_kernel<4,"),
    ("m3", 3, 2, 48, 361, 2, 21, True, "bazmusic::cov_mfma_kernel<3>", "bazmusic::scan_mfma_kernel<3,"),
    ("m5_orthogonal_iteration", 5, 2, 200, 121, 4, 23, True, "bazmusic::cov_mfma_kernel<5>", "bazmusic::scan_mfma_kernel<5,"),
    ("m8_int8_port", 8, 2, 512, 3600, 4, 19, True, "bazmusic::cov_mfma_kernel<8>", "bazmusic::scan_i8_kernel<8,"),
    ("m8_coarse_gate_no_port", 8, 2, 512, 3600, 4, 19, False, "bazmusic::cov_mfma_kernel<8>", "bazmusic::scan_coarse_kernel<8,"),
    ("m16", 16, 2, 1024, 720, 2, 13, True, "bazmusic::cov_mfma2_kernel<16>", "bazmusic::scan_i8_kernel<16,"),
    ("m24_wide", 24, 2, 192, 360, 3, 12, True, "bazwide::cov_wide_", "bazwide::scan_wide_mfma_kernel"),
]


@pytest.mark.parametrize("name,m,n,nsamples,res,W,batch,port,cov,scan", BOXCAR, ids=[b[0] for b in BOXCAR])
def test_boxcar_is_the_reference_on_the_concatenated_items(name, m, n, nsamples, res, W, batch, port, cov, scan, gpu_device):
    capi = _capi()
    table, items = _scene(m, n, nsamples, res, batch, seed=300 + m + W)
    with capi.Context(m, n, nsamples, res, table) as ctx:
        assert ctx.get_averaging() == (1, 1.0)
        fused = ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"
        assert fused == (name == "m4_fused_shape")
        ctx.set_averaging(W)
        assert ctx.get_averaging() == (W, 1.0)
        assert ctx.stage_name(capi.STAGE_COV).startswith(cov), ctx.stage_name(capi.STAGE_COV)
        # two calls: the second one's first W - 1 items take taps from the history
        ang, lvl, spec = _stream(ctx, items, cuts=(5, batch - 5), want_spec=port)
        assert ctx.stage_name(capi.STAGE_SCAN) == scan, ctx.stage_name(capi.STAGE_SCAN)
        path = _path(ctx)
        host = None
        if name in ("m4_two_kernels", "m24_wide"):                      # the host-fed entry point: the same bits
            ctx.reset_averaging()
            host = ctx.process(items, want_spectrum=port)
    worst = _assert_concat_oracle(items, table, m, n, W, ang, lvl, spec, path)
    print("%s: worst err / tol against the concatenation oracle %.3g" % (name, worst))
    if host is not None:
        for d, h in zip((ang, lvl, spec), host):
            assert (d is None and h is None) or np.array_equal(d, h, equal_nan=True)


# ---- 2. the averaging stage alone ----------------------------------------------------------------------------------------------
def _device_cov(ctx, items, m):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _device_average(ctx, R, cuts):
    import torch
    B = R.shape[0]
    per = R[0].size * 2
    rin = torch.from_numpy(np.ascontiguousarray(R).view(np.float64).reshape(B, per)).cuda()
    rout = torch.full((B, per), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    done = 0
    for nb in cuts:
        ctx.debug_average(rin[done].data_ptr(), nb, rout[done].data_ptr())
        done += nb
    assert done == B
    ctx.sync()
    return rout.cpu().numpy().view(np.complex128).reshape(R.shape)


def _tap_tolerance(R, W):
    """(W + 2) 2^-53 max_j |R_{t-j}[e]| per component: W FMAs, one multiply and the rounding of inv_norm (derived, not chosen)."""
    comp = np.abs(np.stack([R.real, R.imag], axis=-1))
    mx = np.zeros_like(comp)
    for t in range(R.shape[0]):
        mx[t] = comp[t - aref.taps(t, W) + 1:t + 1].max(axis=0)
    return (W + 2) * 2.0 ** -53 * mx


TAPS = [
    # m, nsamples, items, W, beta, sizes of the debug_average calls
    (4, 64, 100, 2, 1.0, (100,)),
    (4, 64, 100, 8, 0.7, (3, 1, 40, 56)),
    (4, 64, 100, 64, 1.0, (100,)),
    (4, 64, 100, 64, 0.95, (1, 5, 70, 24)),          # calls shorter than W - 1: the new history is part old history, part batch
    (4, 64, 76, 64, 1.0, (1, 5, 70)),
    (5, 40, 37, 8, 0.7, (9, 28)),                    # E = 25
    (17, 136, 21, 8, 0.7, (2, 19)),                  # E = 289, the run-time-m path's covariance
    (17, 136, 21, 64, 1.0, (1, 5, 15)),
]


@pytest.mark.parametrize("m,nsamples,batch,W,beta,cuts", TAPS, ids=["m%d-W%d-b%g-%dcalls" % (t[0], t[3], t[4], len(t[5])) for t in TAPS])
def test_the_tap_matches_the_restatement(m, nsamples, batch, W, beta, cuts, gpu_device):
    capi = _capi()
    table, items = _scene(m, 2, nsamples, 90, batch, seed=700 + m + W)
    with capi.Context(m, 2, nsamples, 90, table) as ctx:
        R = _device_cov(ctx, items, m)                                   # the device's own plain covariances
        import torch
        r1 = torch.zeros(m * m * 2, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.MusicError) as e:                        # mode off: there is no stage to run
            ctx.debug_average(r1.data_ptr(), 1, r1.data_ptr() + 8)
        assert e.value.code == capi.E_UNSUPPORTED
        ctx.set_averaging(W, beta)
        got = _device_average(ctx, R, cuts)
        again = _device_average(ctx, R, cuts)                            # the history runs on: only the first W - 1 items differ
        ctx.reset_averaging()
        whole = _device_average(ctx, R, (batch,))
        assert np.array_equal(_device_cov(ctx, items, m), R)             # debug_cov keeps returning the plain R
    want = aref.average(R, W, beta, dtype=np.clongdouble)
    tol = _tap_tolerance(R, W)
    err = np.abs(np.stack([(got - want).real, (got - want).imag], axis=-1))
    print("m=%d W=%d beta=%g: worst err / tol %.3g" % (m, W, beta, float(np.max(err / np.maximum(tol, 1e-300)))))
    assert np.all(err <= tol)
    assert np.array_equal(got.view(np.float64), whole.view(np.float64)), "the cut changed bits"
    assert np.array_equal(again[W - 1:].view(np.float64), got[W - 1:].view(np.float64))
    both = np.concatenate([R, R])
    cont = aref.average(both, W, beta, dtype=np.clongdouble)[batch:]
    tol2 = _tap_tolerance(both, W)[batch:]
    err2 = np.abs(np.stack([(again - cont).real, (again - cont).imag], axis=-1))
    assert np.all(err2 <= tol2), "the second pass does not continue the stream"


# ---- 3. exponential weights end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,nsamples,res", [(4, 64, 360), (8, 256, 1000)])
def test_exponential_weights_end_to_end(m, nsamples, res, gpu_device):
    capi = _capi()
    n, W, beta, batch = 2, 16, 0.8, 45
    table, items = _scene(m, n, nsamples, res, batch, seed=900 + m)
    a_ref, _, _, s64, w = aref.music_from_R(aref.average(aref.covariance(items, m), W, beta), table, n)
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W, beta)
        assert ctx.get_averaging() == (W, beta)
        ang, lvl, spec = _stream(ctx, items, cuts=(7, 38))
        path = _path(ctx)
    worst = assert_spectrum_within_bound(spec, s64, path, m, n, table, w)[0]
    worst = max(worst, assert_doa_within_bound(ang, lvl, a_ref, s64, path, m, n, table, w))
    print("m=%d beta=%g W=%d (%s): worst err / tol %.3g" % (m, beta, W, path, worst))


# ---- 4. cut invariance, bitwise -----------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    for x, y, part in zip(a, b, ("ang", "lvl", "spectrum")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), "%s: %s differs" % (what, part)


def test_cut_invariance_is_bitwise(gpu_device, monkeypatch):
    """64 items in one device call, in calls of (1, 7, 3, 53), host-fed, and host-fed under BAZ_MUSIC_CHUNK_MIB=1.  The host-fed
    path never cuts below 1 MiB of traffic per chunk (532 items of this shape), so a 1,300-item stream is what shows three host
    chunks against one device call."""
    capi = _capi()
    m, n, nsamples, res, W = 4, 2, 64, 360, 8
    table, items = _scene(m, n, nsamples, res, 1300, seed=41, snr_db=10.0)
    short = items[:64]
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W)
        one = _stream(ctx, short)
        ctx.reset_averaging()
        _same_bits(one, _stream(ctx, short, cuts=(1, 7, 3, 53)), "calls of (1, 7, 3, 53)")
        ctx.reset_averaging()
        _same_bits(one, ctx.process(short), "host-fed")
        ctx.reset_averaging()
        long_one = _stream(ctx, items)
    _same_bits(one, tuple(v[:64] for v in long_one), "the head of a longer call")
    monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W)
        _same_bits(one, ctx.process(short), "host-fed, BAZ_MUSIC_CHUNK_MIB=1")
        ctx.reset_averaging()
        _same_bits(long_one, ctx.process(items), "host-fed in three chunks")


def test_cut_invariance_on_the_wide_path(gpu_device):
    capi = _capi()
    m, n, nsamples, res, W = 24, 2, 192, 360, 3
    table, items = _scene(m, n, nsamples, res, 14, seed=43)
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W)
        one = _stream(ctx, items)
        ctx.reset_averaging()
        _same_bits(one, _stream(ctx, items, cuts=(1, 13)), "calls of (1, 13)")
        ctx.reset_averaging()
        _same_bits(one, _stream(ctx, items, cuts=(6, 8)), "calls of (6, 8)")


# ---- 5. history semantics --------------------------------------------------------------------------------------------------------
def test_history_semantics(gpu_device):
    capi = _capi()
    m, n, nsamples, res, W = 4, 2, 64, 360, 4
    table, items = _scene(m, n, nsamples, res, 24, seed=51)
    arr = mo.array_geometry(m)
    table2 = mo.steering_table_c64(arr, res, mo.FREQUENCY * 1.07, mo.SPACING)
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W)
        fresh = _stream(ctx, items)
        carried = _stream(ctx, items)                           # the history of the first pass is in force
        assert not np.array_equal(carried[2][:W - 1], fresh[2][:W - 1])
        _same_bits(tuple(v[W - 1:] for v in carried), tuple(v[W - 1:] for v in fresh), "items past the history")
        ctx.reset_averaging()
        _same_bits(fresh, _stream(ctx, items), "after reset_averaging")
        # set_table keeps the history: the next items still match the concatenation oracle, with the new table
        ctx.reset_averaging()
        head = _stream(ctx, items[:10])
        ctx.set_table(table2)
        tail = _stream(ctx, items[10:])
        path = _path(ctx)
        _same_bits(head, tuple(v[:10] for v in fresh), "before the retune")
        both = tuple(np.concatenate([np.zeros_like(h), t]) for h, t in zip(head, tail))
        _assert_concat_oracle(items, table2, m, n, W, both[0], both[1], both[2], path, first=10)
        # a set_averaging that changes nothing keeps the history; changing W or beta resets it
        ctx.set_table(table)
        ctx.reset_averaging()
        _stream(ctx, items[:10])
        ctx.set_averaging(W, 1.0)
        _same_bits(tuple(v[10:] for v in fresh), _stream(ctx, items[10:]), "set_averaging with the values in force")
        ctx.set_averaging(W + 1)
        ctx.set_averaging(W)
        _same_bits(fresh, _stream(ctx, items), "after W changed and changed back")
        ctx.set_averaging(W, 0.5)
        ctx.set_averaging(W, 1.0)
        _same_bits(fresh, _stream(ctx, items), "after beta changed and changed back")
        # errors keep the mode and the history
        _stream(ctx, items[:10])
        for bad in ((0, 1.0), (65, 1.0), (W, 0.0), (W, 1.5), (W, float("nan"))):
            with pytest.raises(capi.MusicError) as e:
                ctx.set_averaging(*bad)
            assert e.value.code == capi.E_INVALID
        assert ctx.get_averaging() == (W, 1.0)
        _same_bits(tuple(v[10:] for v in fresh), _stream(ctx, items[10:]), "after refused calls")
        # the taps that would consume history are refused while the mode is on
        import torch
        x = torch.from_numpy(np.ascontiguousarray(items[:2]).view(np.float32)).cuda()
        q = torch.zeros(64 * m * m, dtype=torch.float64, device="cuda")
        for tap in (lambda: ctx.debug_q(x.data_ptr(), 2, q.data_ptr()), lambda: ctx.debug_coarse_margin(x.data_ptr(), 2)):
            with pytest.raises(capi.MusicError) as e:
                tap()
            assert e.value.code == capi.E_UNSUPPORTED


def test_a_nan_item_poisons_exactly_its_windows(gpu_device):
    capi = _capi()
    m, n, nsamples, res, W = 4, 2, 64, 360, 4
    table, items = _scene(m, n, nsamples, res, 20, seed=53)
    bad = items.copy()
    bad[7, 5] = np.nan
    with capi.Context(m, n, nsamples, res, table) as ctx:
        ctx.set_averaging(W)
        clean = _stream(ctx, items)
        ctx.reset_averaging()
        ang, lvl, spec = _stream(ctx, bad, cuts=(9, 11))        # the poisoned window runs across two calls
        ctx.reset_averaging()
        zero = items.copy()
        zero[7] = 0                                             # a zero item is just a zero tap
        z = _stream(ctx, zero)
    hit = np.arange(7, 7 + W)
    ok = np.setdiff1d(np.arange(20), hit)
    assert np.all(np.isnan(spec[hit])) and np.all(ang[hit] == 0.0) and np.all(lvl[hit] == 0.0)
    _same_bits(tuple(v[ok] for v in clean), (ang[ok], lvl[ok], spec[ok]), "items whose window does not hold the NaN")
    assert np.all(np.isfinite(z[2])) and np.all(z[1] > 0)
    _same_bits(tuple(v[ok] for v in clean), tuple(v[ok] for v in z), "items whose window does not hold the zero item")


# ---- 6. off is the reference bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=91)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs, names = [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_averaging(1, 0.5)
            if how == "on_then_off":
                ctx.set_averaging(4)
                ctx.process(c["items"])
                ctx.set_averaging(1)
            assert ctx.get_averaging()[0] == 1
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2] + _stream(ctx, c["items"]))
            names.append(ctx.stage_name(capi.STAGE_COV))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(set(names)) == 1
    if cfg == "cfg2":
        assert names[0] == "bazmusic::cov4_evd_kernel"


# ---- 7. composition ---------------------------------------------------------------------------------------------------------------
def test_emitter_count_uses_the_effective_snapshots(gpu_device):
    """MDL at 8 antennas, n_max = 3, W = 4: the counts are order_ref on the eigenvalues of Rbar (the device's own plain
    covariances, averaged by the restatement) with N = 4 K -- for the start-up items too."""
    capi = _capi()
    m, K, n_max, W, res = 8, 64, 3, 4, 360
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    parts = [oref.scene(12, m, K, e, 0.1, 60 + e, arr=arr)[0] for e in (1, 2, 3, 0, 2)]      # the count changes along the stream
    items = np.concatenate(parts)
    B = len(items)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_order_mode("mdl")
        ctx.set_averaging(W)
        ang, lvl, spec = ctx.process(items)
        orders = ctx.last_orders(B)
    _, _, ne = capi.averaging_weights(W, 1.0)
    assert ne == W
    Rbar = aref.average(R, W, 1.0)
    Rh = 0.5 * (Rbar + Rbar.conj().transpose(0, 2, 1))
    k_ref, gap = oref.estimate(np.linalg.eigvalsh(Rh), K * W, n_max, "mdl", with_gap=True)
    close = gap < oref.GAP_RTOL
    assert close.sum() <= int(oref.GAP_CAP * B)
    assert np.array_equal(orders[~close], k_ref[~close]), (orders, k_ref)
    assert len(np.unique(orders)) >= 3
    k_single = oref.estimate(np.linalg.eigvalsh(Rh), K, n_max, "mdl")
    print("counts that N = K would have given differently: %d of %d" % (int(np.sum(k_single != k_ref)), B))
    for b in range(B):
        assert np.all(ang[b, orders[b]:] == 0.0) and np.all(lvl[b, orders[b]:] == 0.0) and np.all(lvl[b, :orders[b]] > 0.0)


def test_smoothing_forwards_the_mode_to_the_inner_context(gpu_device):
    """FB + SS(6) on an 8-element line array, the coherent pair of DESIGN.md 8b, W = 4: the inner context averages the re-stacked
    covariances, which is the smoothed covariance of the concatenated items."""
    capi = _capi()
    res, m, n, ms, W, K = 720, 8, 2, 6, 4, 64
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = sr.two_emitters(21, arr, K, coherent=True, seed=2025)
    perm = capi.smoothing_check(m, res, table, ms, True)
    sub = table[:, :ms]
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_averaging(W)
        ctx.set_smoothing(ms, True)
        assert ctx.get_averaging() == (W, 1.0) and ctx.get_smoothing() == (ms, True)
        path = "int8" if ctx.uses_i8_scan() else "fp64"
        ang, lvl, spec = ctx.process(items)
        ctx.reset_averaging()                                   # (forwarded: the inner context keeps the history)
        dev = _stream(ctx, items, cuts=(4, 17))
        ctx.set_smoothing(m, False)                             # smoothing off: this context averages itself, from an empty history
        assert ctx.get_averaging() == (W, 1.0)
        plain = _stream(ctx, items)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_averaging(W)
        _same_bits(plain, _stream(ctx, items), "after smoothing went off against a context that never smoothed")
    _same_bits((ang, lvl, spec), dev, "host-fed against device-resident")
    for c, idx, cat in aref.windows(items, W):
        a_ref, _, _, s64, w = oracle_fp64(sr.restack(cat, m, ms, True, perm), sub, ms, n)
        assert_spectrum_within_bound(spec[idx], s64, path, ms, n, sub, w, ill_posed_ok=True)
        assert_doa_within_bound(ang[idx], lvl[idx], a_ref, s64, path, ms, n, sub, w, ill_posed_ok=True)


def test_peak_mode_and_refinement_read_the_averaged_problem(gpu_device):
    """cfg1's shape, peak mode 1 + refinement, W = 4: offsets against refine_ref on the oracle's d of the concatenated items at the
    device's own bins, with tests/test_refine_gpu.py's tolerance function."""
    capi = _capi()
    c = mo.make_config("cfg1", 40, snr_db=20.0, seed=77)
    m, n, N, res, W = c["m"], c["n"], c["nsamples"], c["res"], 4
    items, table = c["items"], c["table"]
    with capi.Context(m, n, N, res, table) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_averaging(W)
        a0, l0, s0 = ctx.process(items)
        ctx.reset_averaging()
        ctx.set_refine_mode(1)
        a1, l1, s1 = ctx.process(items)
        off = ctx.last_refine_offsets(len(items) * n).reshape(len(items), n)
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    for b in range(len(items)):
        pa, pl = mo.peak_pick(s0[b], n, res)
        assert np.array_equal(a0[b], pa) and np.array_equal(l0[b], pl)
    present = l0 != 0
    bins = rr.bins_of(a0, res)
    worst, moved = 0.0, 0
    for cc, idx, cat in aref.windows(items, W):
        _, _, _, s64, w = oracle_fp64(cat, table, m, n)
        with np.errstate(divide="ignore"):
            d = 1.0 / s64
        tol, either = rr.tolerance(m, n, table, s64, w, bins[idx])
        ref = np.where(present[idx], rr.delta(rr.triples(d, bins[idx])).reshape(bins[idx].shape), 0.0)
        err = np.abs(off[idx] - ref)
        y = rr.triples(d, bins[idx])
        with np.errstate(invalid="ignore", divide="ignore"):
            raw = ((y[..., 0] - y[..., 1]) - (y[..., 2] - y[..., 1])) / (2.0 * ((y[..., 0] - y[..., 1]) + (y[..., 2] - y[..., 1])))
        alt = either & ((off[idx] == 0.0) | (np.abs(off[idx] - raw) <= np.abs(tol)))       # (p or q within E of 0: either branch)
        bad = present[idx] & ~(err <= tol) & ~alt
        assert not bad.any(), "items with %d taps: offset error %.3g above its tolerance" % (cc, float(err[bad].max()))
        cmpd = present[idx] & np.isfinite(tol) & (tol > 0)
        worst = max(worst, float(np.max(err[cmpd] / tol[cmpd])) if cmpd.any() else 0.0)
        moved += int(np.count_nonzero(off[idx]))
        mv = present[idx] & (off[idx] != 0.0)
        assert np.array_equal(a1[idx][mv].view(np.uint32), rr.angle(bins[idx][mv], off[idx][mv], res).view(np.uint32))
    assert moved > len(items)
    print("refinement on the averaged problem: %d entries moved, worst err / tol %.3g" % (moved, worst))


# ---- 8. the effect on the device -----------------------------------------------------------------------------------------------
def test_effect_on_the_device(gpu_device):
    """The 2,000 items of the CPU effect test (10 dB) through a context at W = 1 and W = 8, peak mode on: the found-both rates
    within 0.005 of the oracle's (spectra differ by ~1e-7; 0.005 allows ten near-tie items of 2,000)."""
    capi = _capi()
    E = aref.EFFECT
    table, items = aref.effect_scene(10.0)
    got, want = {}, {}
    with capi.Context(E["m"], E["n"], E["nsamples"], E["res"], table) as ctx:
        ctx.set_peak_mode(1)
        for W in (1, 8):
            ctx.set_averaging(W)
            ang, lvl, _ = ctx.process(items)
            got[W] = aref.effect_stats(ang, lvl)
            Rbar = aref.average(aref.covariance(items, E["m"]), W, 1.0)
            want[W] = aref.effect_stats(*aref.pick_peaks(aref.music_from_R(Rbar, table, E["n"])[2], E["n"]))
            print("W = %d: device found-both %.4f RMS %.3f deg; oracle %.4f / %.3f deg; difference %.4f"
                  % (W, got[W][0], got[W][1], want[W][0], want[W][1], abs(got[W][0] - want[W][0])))
    for W in (1, 8):
        assert abs(got[W][0] - want[W][0]) <= 0.005
    assert got[1][0] <= 0.85 and got[8][0] >= 0.99 and got[8][1] <= 0.5 * got[1][1]


# ---- 9. a mode change beside a submitting thread -----------------------------------------------------------------------------------
def test_mode_changes_beside_a_submitting_thread(gpu_device):
    """A second thread flips the mode while this one submits.  Every batch starts from an empty history (reset_averaging before
    it; a flip resets too), so a batch computed under ONE mode equals the mode-off outputs or the mode-on outputs of a fresh
    stream bit for bit -- a batch that mixed the two would equal neither."""
    capi = _capi()
    m, n, nsamples, res, W = 4, 2, 64, 360, 8
    table, items = _scene(m, n, nsamples, res, 64, seed=97, snr_db=10.0)
    stop = threading.Event()
    errors = []

    def flip(ctx):
        i = 0
        try:
            while not stop.is_set():
                ctx.set_averaging(W if i % 2 == 0 else 1)
                i += 1
        except Exception as e:       # noqa: BLE001
            errors.append(e)

    kinds = set()
    with capi.Context(m, n, nsamples, res, table) as ctx:
        off = ctx.process(items, want_spectrum=False)
        ctx.set_averaging(W)
        on = ctx.process(items, want_spectrum=False)
        assert not np.array_equal(off[1], on[1])
        t = threading.Thread(target=flip, args=(ctx,))
        t.start()
        try:
            for _ in range(60):
                ctx.reset_averaging()
                ang, lvl, _ = ctx.process(items, want_spectrum=False)
                is_off = np.array_equal(ang, off[0]) and np.array_equal(lvl, off[1])
                is_on = np.array_equal(ang, on[0]) and np.array_equal(lvl, on[1])
                assert is_off or is_on, "a batch mixes the two modes"
                kinds.add(is_on)
        finally:
            stop.set()
            t.join()
    assert not errors, errors
    print("batches seen with the mode off / on:", kinds)
