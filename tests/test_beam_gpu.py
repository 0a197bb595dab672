"""Opt-in MVDR beamformer output (baz_music_set_beam_mode) on the MI355X: the weights tap (last_beam_weights) of every reported
entry against beam_ref on the device's own covariance (debug_cov) and the device's own bins, and the beams (last_beams) against
beam_ref.beams applied to the device's own weights, for every group width, frontend and scan form up to 16 antennas, with and without
the spectrum port, under both pickers, with and without loading; every port bit for bit that of mode 0; the Capon identity on the
device; the emitter-count mode, refinement, the power mode and averaging; scope; host paths == device path; mode off == the reference
with no extra launch; degenerate items; retune.

Tolerances: weights, relative in norm, 8 m cond_2(R_l) 2^-52 per item (beam_ref.tolerance); beams
|y - y_ref| <= 2^-24 |y_ref| + 8 m 2^-52 sum_r |w_r| |x_r| (the half-ulp complex64 rounding and the fp64 accumulation)."""
import numpy as np
import pytest

import averaging_ref as ar
import beam_ref as br
import order_ref as oref
import power_ref as pr
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _c64bits(x):
    return np.ascontiguousarray(x, dtype=np.complex64).view(np.uint64)


def _c128bits(x):
    return np.ascontiguousarray(x, dtype=np.complex128).view(np.uint64)


def _device_cov(ctx, items, m):
    """R of every item as the context's own covariance stage computes it (debug_cov), (B, m, m) complex128."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _taps(ctx, B):
    W = ctx.last_beam_weights(B)
    Y = ctx.last_beams(B)
    assert W.shape == (B, ctx.n, ctx.m) and Y.shape == (B, ctx.n, ctx.nsamples // ctx.m)
    return W, Y


def _off_and_on(ctx, items, loading=0.0, want_spectrum=True, before=None):
    """Mode 0, then mode 1 on the same items: (ports of mode 0, ports of mode 1, weights (B, n, m), beams (B, n, K)).  before: called
    in front of every process call (averaging: reset the stream)."""
    B = len(items)
    ctx.set_beam_mode(0)
    if before:
        before()
    o0 = ctx.process(items, want_spectrum=want_spectrum)
    W0, Y0 = _taps(ctx, B)
    assert not W0.any() and not Y0.any()                                   # a call with the mode off reports zeros
    ctx.set_beam_mode(1, loading)
    assert ctx.get_beam_mode() == (1, loading)
    if before:
        before()
    o1 = ctx.process(items, want_spectrum=want_spectrum)
    W, Y = _taps(ctx, B)
    ctx.set_beam_mode(0)
    return o0, o1, W, Y


def _assert_ports_equal(o0, o1, what):
    for name, a, b in zip(("ang", "lvl", "spectrum"), o0, o1):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(_f32bits(a), _f32bits(b)), "%s: %s changed under the beam mode" % (what, name)


def _assert_beams(items, W, Y, m, what):
    """Y against beam_ref.beams on the device's own weights W; entries without weights have all-zero beams (bit for bit).  Returns
    the worst ratio |y - y_ref| / bound."""
    B = len(items)
    K = items.shape[1] // m
    X = np.asarray(items).reshape(B, K, m)
    worst = 0.0
    for b in range(B):
        dead = ~np.abs(W[b]).astype(bool).any(axis=1)
        assert not _c64bits(Y[b][dead]).any(), "%s item %d: an entry without weights has a beam" % (what, b)
        if dead.all():
            continue
        with np.errstate(all="ignore"):
            ref = br.beams(X[b], W[b])
            bound = 2.0 ** -24 * np.abs(ref) + 8.0 * m * br.EPS * br.beam_bound(X[b], W[b])
            err = np.abs(Y[b].astype(np.complex128) - ref)
        live = ~dead
        bad = ~(err[live] <= bound[live])
        assert not bad.any(), "%s item %d: |y - y_ref| %.3g > bound %.3g" % (what, b, err[live][bad][0], bound[live][bad][0])
        nz = bound[live] > 0
        if nz.any():
            worst = max(worst, float(np.max(err[live][nz] / bound[live][nz])))
    return worst


def _assert_definition(o0, o1, W, Y, R, table, res, items, loading, what="", present=None):
    """Ports of mode 1 == mode 0 bit for bit; the weights within tolerance (relative norm) of beam_ref on R at the device's own bins;
    zero and non-zero entries coincide; the beams within their bound of beam_ref.beams on the device's weights.
    Returns (worst weight error / (m cond 2^-52), worst beam error / bound, live entries)."""
    _assert_ports_equal(o0, o1, what)
    a0, l0 = o0[0], o0[1]
    present = (l0 != 0) if present is None else present
    m = R.shape[1]
    bins = pr.bins_of(a0, res)
    ref = br.item_weights(R, table, bins, present, loading)
    tol = br.tolerance(R, loading)
    got_live = np.abs(W).astype(bool).any(axis=2)
    ref_live = np.abs(ref).astype(bool).any(axis=2)
    assert np.array_equal(got_live, ref_live), "%s: the degenerate / missing entries differ" % what
    assert not W[~present].any(), "%s: a missing entry has weights" % what
    worst_w = 0.0
    for b, e in zip(*np.nonzero(ref_live)):
        rel = np.linalg.norm(W[b, e] - ref[b, e]) / np.linalg.norm(ref[b, e])
        assert rel <= tol[b], ("%s item %d slot %d (bin %d): relative norm error of w %.3g > tol %.3g" % (what, b, e, bins[b, e], rel, tol[b]))
        worst_w = max(worst_w, rel / (tol[b] / 8.0))
    worst_y = _assert_beams(items, W, Y, m, what)
    return worst_w, worst_y, int(ref_live.sum())


# name, m, n, K, res, batch, sigma, loadings.  Line arrays.  Batches of 23 leave wave groups partly empty.
SHAPES = [
    ("m2_n1", 2, 1, 32, 90, 23, 0.1, (0.0, 1e-2)),
    ("m3_n2_K100", 3, 2, 100, 357, 23, 0.1, (0.0, 1e-2)),
    ("m4_two_kernels", 4, 2, 64, 360, 48, 0.1, (0.0, 1e-2)),
    ("m4_fused", 4, 2, 256, 360, 24, 0.1, (0.0, 1e-2)),
    ("m5_n3", 5, 3, 200, 720, 23, 0.1, (0.0, 1e-2)),
    ("m7_n4", 7, 4, 64, 720, 23, 0.1, (0.0, 1e-2)),
    ("m8_int8_coarse", 8, 2, 512, 720, 6, 0.1, (0.0, 1e-2)),
    ("m12_n2", 12, 2, 64, 720, 23, 0.1, (0.0, 1e-2)),
    ("m16_n15", 16, 15, 64, 360, 23, 0.1, (0.0, 1e-2)),
    ("batch_of_1", 8, 2, 64, 360, 1, 0.1, (0.0, 1e-2)),
    ("m8_60dB", 8, 2, 64, 720, 23, 1e-3, (0.0, 1e-2)),
    ("m4_K3_loaded", 4, 2, 3, 360, 23, 0.1, (0.0, 1e-2)),         # (K < m: every item degenerate at loading 0, none at 1e-2)
]


@pytest.mark.parametrize("name,m,n,K,res,batch,sigma,loadings", SHAPES, ids=[s[0] for s in SHAPES])
def test_definition_parity(name, m, n, K, res, batch, sigma, loadings, gpu_device):
    capi = _capi()
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    # (at most 4 emitters: the scene keeps them 20 degrees apart inside [20, 160]; the slots beyond them hold whatever the picker finds)
    items, _ = oref.scene(batch, m, K, min(n, 4), sigma, seed=700 + m, arr=arr, grid=360.0 / res if sigma < 0.01 else None)
    worst_w_all = worst_y_all = 0.0
    with capi.Context(m, n, m * K, res, table) as ctx:
        if name == "m4_fused":
            assert ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"
        R = _device_cov(ctx, items, m)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            for spectrum in (True, False):
                for loading in loadings:
                    what = "%s peak=%d spectrum=%d loading=%g" % (name, peak, spectrum, loading)
                    o0, o1, W, Y = _off_and_on(ctx, items, loading, want_spectrum=spectrum)
                    worst_w, worst_y, entries = _assert_definition(o0, o1, W, Y, R, table, res, items, loading, what)
                    worst_w_all, worst_y_all = max(worst_w_all, worst_w), max(worst_y_all, worst_y)
                    print("%s: %d entries, worst w err / (m cond 2^-52) %.3g (bound 8), worst |y - y_ref| / bound %.3g, largest cond %.3g"
                          % (what, entries, worst_w, worst_y, float(np.max(br.tolerance(R, loading))) / (8.0 * m * br.EPS)))
                    assert (entries > 0) if (K >= m or loading > 0) else (entries == 0 and (o0[1] != 0).any())
        if name == "m4_fused":
            ctx.set_beam_mode(1)
            assert ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"   # the fused kernel keeps running (with its R tap)
    print("%s: worst over the wirings: w %.3g of m cond 2^-52, y %.3g of its bound" % (name, worst_w_all, worst_y_all))


@pytest.mark.parametrize("m,n,K", [(4, 2, 256), (8, 2, 64), (16, 3, 64)], ids=["m4_fused_shape", "m8", "m16"])
def test_capon_identity_on_the_device(m, n, K, gpu_device):
    """mean_c |y[c]|^2 == last_powers within tolerance + 2^-22 (power mode 1, loading 0): y^H y / K = w^H R w = 1 / (a^H R^-1 a)."""
    capi = _capi()
    res, B = 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=810 + m)
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_peak_mode(1)
        ctx.set_power_mode(1)
        ctx.set_beam_mode(1, 0.0)
        _, lvl, _ = ctx.process(items)
        P = ctx.last_powers(B * n).reshape(B, n)
        _, Y = _taps(ctx, B)
    out = np.mean(np.abs(Y.astype(np.complex128)) ** 2, axis=2)
    tol = br.tolerance(R)[:, None] + 2.0 ** -22
    live = lvl != 0
    assert live.sum() >= B and np.all(P[live] > 0)
    rel = np.abs(out[live] - P[live]) / P[live]
    print("Capon identity m=%d: worst relative %.3g, worst / tolerance %.3g" % (m, rel.max(), np.max(rel / np.broadcast_to(tol, P.shape)[live])))
    assert np.all(rel <= np.broadcast_to(tol, P.shape)[live])
    assert not out[~live].any()


def test_order_mode_mixed_counts(gpu_device):
    capi = _capi()
    m, K, n_max, res = 8, 64, 3, 720
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    parts = [oref.scene(16, m, K, e, 0.1, 900 + 17 * e, arr=arr)[0] for e in range(n_max + 1)]
    items = np.concatenate(parts)[np.random.default_rng(9).permutation(16 * (n_max + 1))]
    B = len(items)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_order_mode("mdl")
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            o0, o1, W, Y = _off_and_on(ctx, items)
            orders = ctx.last_orders(B)
            assert set(np.unique(orders)) == set(range(n_max + 1))
            want = oref.estimate_items(items, m, n_max, "mdl")
            assert np.mean(orders == want) >= 0.9                          # (the counts are the emitter-count mode's own)
            for b in range(B):
                assert not W[b, orders[b]:].any() and not _c64bits(Y[b, orders[b]:]).any()
            worst_w, worst_y, entries = _assert_definition(o0, o1, W, Y, R, table, res, items, 0.0, "order mode peak=%d" % peak)
            print("order mode peak=%d: %d entries, worst w %.3g, worst y %.3g" % (peak, entries, worst_w, worst_y))
            if not peak:
                assert entries == int(orders.sum())


def test_refinement_and_power_mode_2_together(gpu_device):
    """The grid bin is used and ang is refined as before; with power mode 2 + refinement + beam every caller-visible word is written
    once (buffers prefilled with a sentinel on the device path), lvl is float32(P), the beams are those of beam alone."""
    import torch
    capi = _capi()
    m, n, K, res, B = 8, 2, 64, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.03, seed=77)
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_peak_mode(1)
        grid = ctx.process(items)
        ctx.set_beam_mode(1, 1e-2)
        alone = ctx.process(items)
        W_alone, Y_alone = _taps(ctx, B)
        _assert_ports_equal(grid, alone, "beam alone")
        ctx.set_beam_mode(0)
        ctx.set_refine_mode(1)
        refined = ctx.process(items)
        ctx.set_beam_mode(1, 1e-2)
        both = ctx.process(items)
        W_ref, Y_ref = _taps(ctx, B)
        _assert_ports_equal(refined, both, "refinement + beam")
        assert not np.array_equal(_f32bits(grid[0]), _f32bits(refined[0]))
        assert np.array_equal(_c128bits(W_ref), _c128bits(W_alone)) and np.array_equal(_c64bits(Y_ref), _c64bits(Y_alone))
        ctx.set_power_mode(2)
        x = torch.from_numpy(items.view(np.float32)).cuda()
        d_ang = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda")
        d_lvl = torch.full((B, n), 7.0, dtype=torch.float32, device="cuda")
        d_spec = torch.full((B, res), 7.0, dtype=torch.float32, device="cuda")
        ctx.process_device(x.data_ptr(), B, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        P = ctx.last_powers(B * n).reshape(B, n)
        W3, Y3 = _taps(ctx, B)
        assert np.array_equal(_f32bits(d_ang.cpu().numpy()), _f32bits(refined[0]))
        assert np.array_equal(_f32bits(d_lvl.cpu().numpy()), _f32bits(P.astype(np.float32)))
        assert np.array_equal(_f32bits(d_spec.cpu().numpy()), _f32bits(refined[2]))
        assert np.array_equal(_c128bits(W3), _c128bits(W_alone)) and np.array_equal(_c64bits(Y3), _c64bits(Y_alone))
        # power mode 1 + beam, neither refinement: power_kernel writes the ports, the taps of both modes are their own
        ctx.set_refine_mode(0)
        ctx.set_power_mode(1)
        pb = ctx.process(items)
        _assert_ports_equal(grid, pb, "power mode 1 + beam")
        assert np.array_equal(ctx.last_powers(B * n).reshape(B, n), P)
        W4, Y4 = _taps(ctx, B)
        assert np.array_equal(_c128bits(W4), _c128bits(W_alone)) and np.array_equal(_c64bits(Y4), _c64bits(Y_alone))
    worst_w, worst_y, entries = _assert_definition(grid, alone, W_alone, Y_alone, R, table, res, items, 1e-2, "grid bins")
    assert entries == int((grid[1] != 0).sum())
    ref_P = pr.powers(R, table, pr.bins_of(grid[0], res), grid[1] != 0)     # the power mode keeps its definition on the unloaded R
    assert np.all(np.abs(P - ref_P) <= pr.tolerance(R)[:, None] * ref_P)


@pytest.mark.parametrize("m,K", [(4, 256), (8, 64)], ids=["m4_fused_shape", "m8"])
def test_averaging_window_3(m, K, gpu_device):
    capi = _capi()
    n, res, B = 2, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=333 + m)
    Rbar = ar.average(ar.covariance(items, m), 3)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_averaging(3)
        ctx.set_peak_mode(1)
        o0, o1, W, Y = _off_and_on(ctx, items, 1e-2, before=ctx.reset_averaging)
    # (R-bar_t from numpy covariances, x the item's own: _assert_beams applies W to `items`)
    worst_w, worst_y, entries = _assert_definition(o0, o1, W, Y, Rbar, table, res, items, 1e-2, "averaging W=3 m=%d" % m)
    assert W[:2].any()                                                     # the first two items of the stream average fewer taps
    print("averaging W=3 m=%d: %d entries, worst w %.3g, worst y %.3g" % (m, entries, worst_w, worst_y))


def test_scope(gpu_device):
    capi = _capi()
    m = 17
    table = mo.steering_table_c64(oref.ula(m), 360, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, 2, m * 32, 360, table) as ctx:
        with pytest.raises(capi.MusicError) as e:
            ctx.set_beam_mode(1)
        assert e.value.code == capi.E_UNSUPPORTED and ctx.get_beam_mode() == (0, 0.0)
        ctx.set_beam_mode(0)
    m, n, K, res = 8, 2, 64, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(8, m, K, n, 0.1, seed=5)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_beam_mode(1, 0.25)
        for mode, loading in ((2, 0.0), (-1, 0.0), (1, -1e-3), (1, float("nan")), (1, float("inf")), (0, -1.0)):
            assert capi.lib().baz_music_set_beam_mode(ctx._h, mode, loading) == capi.E_INVALID
            assert ctx.get_beam_mode() == (1, 0.25)                        # the previous setting stays in force
        # smoothing refuses while the beam mode is on ...
        with pytest.raises(capi.MusicError) as e:
            ctx.set_smoothing(6, True)
        assert e.value.code == capi.E_UNSUPPORTED
        assert ctx.get_smoothing() == (m, False) and ctx.get_beam_mode() == (1, 0.25)
        ctx.process(items)
        assert ctx.last_beam_weights(8).any()
        # ... and the beam mode while smoothing is on
        ctx.set_beam_mode(0)
        ctx.set_smoothing(6, True)
        with pytest.raises(capi.MusicError) as e:
            ctx.set_beam_mode(1, 0.5)
        assert e.value.code == capi.E_UNSUPPORTED
        assert ctx.get_smoothing() == (6, True) and ctx.get_beam_mode() == (0, 0.0)
        ctx.set_beam_mode(0)                                               # (switching it off is always accepted)
        ctx.process(items)
        assert not ctx.last_beams(8).any()
        ctx.set_smoothing(m, False)
        ctx.set_beam_mode(1, 0.5)
        assert ctx.get_beam_mode() == (1, 0.5)


def test_host_paths_equal_the_device_path(gpu_device, monkeypatch):
    """process_device, a host-fed call in one chunk, a host-fed zero-copy call on page-locked memory and a host-fed call cut into
    chunks: identical ang / lvl / spectrum / weights / beams bits, the chunks' beams in call order."""
    import torch
    capi = _capi()
    batch = 300
    c = mo.make_config("cfg2", batch, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    items = c["items"]
    K = N // m
    outs = []
    for how in ("device", "host", "zero_copy", "chunked"):
        if how == "chunked":
            monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            ctx.set_peak_mode(1)
            ctx.set_beam_mode(1, 1e-2)
            if how == "device":
                x = torch.from_numpy(items.view(np.float32)).cuda()
                d_ang = torch.full((batch, n), 7.0, dtype=torch.float32, device="cuda")
                d_lvl = torch.full((batch, n), 7.0, dtype=torch.float32, device="cuda")
                d_spec = torch.zeros(batch, res, dtype=torch.float32, device="cuda")
                ctx.process_device(x.data_ptr(), batch, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                out = (d_ang.cpu().numpy(), d_lvl.cpu().numpy(), d_spec.cpu().numpy())
            elif how == "zero_copy":
                pinned = torch.from_numpy(items.view(np.float32)).pin_memory().numpy().view(np.complex64)
                o = tuple(torch.zeros((batch, k), dtype=torch.float32).pin_memory().numpy() for k in (n, n, res))
                out = ctx.process(pinned, out=o)
            else:
                out = ctx.process(items)
            if how == "chunked":
                assert batch > 2 * max(64, (1 << 20) // (N * 8 + res * 4 + n * 8))   # (more than two chunks)
            W, Y = _taps(ctx, batch)
            assert np.array_equal(_c64bits(ctx.last_beams(10)), _c64bits(Y[:10]))
            assert np.array_equal(_c128bits(ctx.last_beam_weights(10)), _c128bits(W[:10]))
            ptr, cnt = ctx.last_beams_device()
            assert cnt == batch and ptr
            ctx.sync()                                                     # (the buffer is ordered on the context's stream)

            class _Floats:
                __cuda_array_interface__ = {"shape": (batch * n * K * 2,), "typestr": "<f4", "data": (ptr, False), "version": 2}

            back = torch.as_tensor(_Floats(), device="cuda").cpu().numpy().view(np.complex64).reshape(batch, n, K)
            outs.append(tuple(np.array(a) for a in out) + (W, Y, back))
    assert np.abs(outs[0][3]).astype(bool).any(axis=2).sum() > batch
    for o in outs:
        assert np.array_equal(_c64bits(o[5]), _c64bits(o[4])), "last_beams_device holds other bytes than last_beams"
    for o in outs[1:]:
        for a, b in zip(outs[0][:3], o[:3]):
            assert np.array_equal(_f32bits(a), _f32bits(b))
        assert np.array_equal(_c128bits(outs[0][3]), _c128bits(o[3]))
        assert np.array_equal(_c64bits(outs[0][4]), _c64bits(o[4]))


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    """A context never set, one set to 0 and one switched on and off again: identical bits, and identical launch counts of every
    stage (mode 1 adds exactly two launches per sequence, both under the merge stage)."""
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=92)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs, launches = [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_beam_mode(0)
            if how == "on_then_off":
                ctx.set_beam_mode(1, 1e-2)
                ctx.profile(1)
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                on_launches = [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]
                assert ctx.last_beams(batch).any()
                ctx.set_beam_mode(0)
            assert ctx.get_beam_mode()[0] == 0
            ctx.profile(1)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            assert not ctx.last_beams(batch).any() and not ctx.last_beam_weights(batch).any()
            assert ctx.last_beams_device() == (0, 0)
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b))
    assert launches[0] == launches[1] == launches[2], launches
    want = list(launches[0])
    want[capi.STAGE_MERGE] += 4                                            # two calls, beam_weights_kernel and beam_apply_kernel each
    assert on_launches == want, (on_launches, launches[0])


@pytest.mark.parametrize("m,n,K", [(4, 2, 64), (12, 2, 64)], ids=["m4", "m12"])
def test_degenerate_items_in_the_middle_of_a_wave(m, n, K, gpu_device):
    """All-zero items (and one holding NaN) interleaved with live ones: zeros for them, the neighbours bit for bit those of a batch
    without them."""
    capi = _capi()
    res, B = 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    clean, _ = oref.scene(B, m, K, n, 0.1, seed=40 + m)
    zeroed = [3, 4, 9, 17]
    items = clean.copy()
    items[zeroed] = 0
    items[11, 7] = np.nan
    dead = zeroed + [11]
    good = np.ones(B, bool)
    good[dead] = False
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            for loading in (0.0, 1e-2):
                what = "degenerate m=%d peak=%d loading=%g" % (m, peak, loading)
                o0, o1, W, Y = _off_and_on(ctx, items, loading)
                assert not W[dead].any() and not _c64bits(Y[dead]).any(), what
                assert np.abs(W[good]).astype(bool).any(axis=2)[o0[1][good] != 0].all(), what
                ok = np.isfinite(R.reshape(B, -1)).all(axis=1)             # (numpy cannot condition the NaN item: checked above)
                _assert_ports_equal(o0, o1, what)
                _assert_definition(tuple(None if a is None else a[ok] for a in o0), tuple(None if a is None else a[ok] for a in o1),
                                   W[ok], Y[ok], R[ok], table, res, items[ok], loading, what)
                _, _, Wc, Yc = _off_and_on(ctx, clean[good], loading)
                assert np.array_equal(_c128bits(W[good]), _c128bits(Wc)), what + ": a neighbour's weights changed"
                assert np.array_equal(_c64bits(Y[good]), _c64bits(Yc)), what + ": a neighbour's beams changed"


def test_fewer_snapshots_than_antennas(gpu_device):
    """K < m: zeros at loading 0 (a failing pivot), the restatement's weights at loading 1e-2."""
    capi = _capi()
    m, n, N, res, B = 4, 2, 8, 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, N // m, n, 0.1, seed=12)
    with capi.Context(m, n, N, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        o0, o1, W, Y = _off_and_on(ctx, items, 0.0)
        assert (o0[1] != 0).any()
        _assert_ports_equal(o0, o1, "K < m")
        assert not W.any() and not _c64bits(Y).any()
        o0, o1, W, Y = _off_and_on(ctx, items, 1e-2)
        worst_w, worst_y, entries = _assert_definition(o0, o1, W, Y, R, table, res, items, 1e-2, "K < m, loaded")
        assert entries == int((o0[1] != 0).sum()) and entries >= B


def test_retune_to_a_rotated_table(gpu_device):
    capi = _capi()
    c = mo.make_config("cfg1", 64, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    rotated = np.ascontiguousarray(np.roll(c["table"], 37, axis=0))
    with capi.Context(m, n, N, res, c["table"]) as ctx:
        R = _device_cov(ctx, c["items"], m)
        ctx.set_peak_mode(1)
        ctx.set_beam_mode(1)
        a_old, _, _ = ctx.process(c["items"])
        W_old, _ = _taps(ctx, 64)
        ctx.set_table(rotated)
        o0, o1, W, Y = _off_and_on(ctx, c["items"])
    worst_w, worst_y, entries = _assert_definition(o0, o1, W, Y, R, rotated, res, c["items"], 0.0, "rotated table")
    assert entries == 64 * n
    # the same rows 37 bins further round the circle: the same weights
    b_old, b_new = pr.bins_of(a_old, res), (pr.bins_of(o0[0], res) - 37) % res
    io, inw = np.argsort(b_old, axis=1), np.argsort(b_new, axis=1)
    assert np.array_equal(np.take_along_axis(b_old, io, 1), np.take_along_axis(b_new, inw, 1))
    assert np.array_equal(_c128bits(np.take_along_axis(W_old, io[:, :, None], 1)), _c128bits(np.take_along_axis(W, inw[:, :, None], 1)))
