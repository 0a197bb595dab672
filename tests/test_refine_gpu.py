"""Opt-in sub-bin angle refinement (baz_music_set_refine_mode) on the MI355X: the offsets of every reported entry against
refine_ref applied to the fp64 oracle's d at the device's own bins, on every frontend / scan up to 16 antennas, with and without
the spectrum port, under both pickers, the emitter-count mode and smoothing; host path == device path; mode off == the reference
bit for bit with no extra launch; the effect table of DESIGN.md 8d produced by the device; retune; scope."""
import numpy as np
import pytest

import order_ref as oref
import refine_ref as rr
import smoothing_ref as sr
from helpers import oracle_fp64
from oracle import music_oracle as mo
from test_refine import EFFECT, effect_rms

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _both_modes(ctx, items, want_spectrum=True, want_lvl=True):
    """Mode 0 then mode 1 on the same items: ((ang, lvl, spec) of mode 0, the same of mode 1, offsets (B, n))."""
    B = len(items)
    ctx.set_refine_mode(0)
    off_out = ctx.process(items, want_lvl=want_lvl, want_spectrum=want_spectrum)
    zeros = ctx.last_refine_offsets(B * ctx.n)
    assert len(zeros) == B * ctx.n and not zeros.any()                     # a call with the mode off reports zeros
    ctx.set_refine_mode(1)
    assert ctx.get_refine_mode() == 1
    on_out = ctx.process(items, want_lvl=want_lvl, want_spectrum=want_spectrum)
    off = ctx.last_refine_offsets(B * ctx.n)
    assert len(off) == B * ctx.n
    ctx.set_refine_mode(0)
    return off_out, on_out, off.reshape(B, ctx.n)


def _assert_definition(off_out, on_out, off, d, tol, either, present, res, what=""):
    """The parity procedure: lvl / spectrum bitwise equal between the two modes; every entry's offset within the derived
    tolerance of refine_ref on the oracle's d at the device's own bins (an entry whose p or q is within E of 0 may take either
    branch); ang consistent with the offset.  Returns (worst |err| / tol, entries compared, either-branch entries)."""
    a0, l0, s0 = off_out
    a1, l1, s1 = on_out
    if l0 is not None:
        assert np.array_equal(_f32bits(l0), _f32bits(l1)), "%s: lvl changed" % what
    if s0 is not None:
        assert np.array_equal(_f32bits(s0), _f32bits(s1)), "%s: the spectrum changed" % what
    bins = rr.bins_of(a0, res)
    y = rr.triples(d, bins)
    ref = np.where(present, rr.delta(y).reshape(bins.shape), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        raw = ((y[..., 0] - y[..., 1]) - (y[..., 2] - y[..., 1])) / (2.0 * ((y[..., 0] - y[..., 1]) + (y[..., 2] - y[..., 1])))
    assert np.all(np.abs(off) <= 0.5)
    assert not off[~present].any(), "%s: a missing entry moved" % what
    assert np.array_equal(_f32bits(a1[~present]), _f32bits(a0[~present]))
    err = np.abs(off - ref)
    ok = err <= tol
    alt = either & ((off == 0.0) | (np.abs(off - raw) <= np.abs(tol)))
    bad = present & ~ok & ~alt
    if bad.any():
        b, i = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError("%s item %d slot %d (bin %d): offset %.12g, refine_ref %.12g, |err| %.3g > tol %.3g"
                             % (what, b, i, bins[b, i], off[b, i], ref[b, i], err[b, i], tol[b, i]))
    # ang: exactly the restated cast of the device's own offset; an unmoved entry keeps the bits of mode 0
    moved = present & (off != 0.0)
    assert np.array_equal(_f32bits(a1[moved]), _f32bits(rr.angle(bins[moved], off[moved], res))), "%s: ang is not the cast of b + delta" % what
    assert np.array_equal(_f32bits(a1[~moved]), _f32bits(a0[~moved])), "%s: an entry with delta = 0 changed its ang bits" % what
    # ... and against the restatement: 1 ulp_f32 of the reference angle plus 360 / res times the offset's tolerance
    aref = rr.angle(bins, ref, res).astype(np.float64)
    diff = np.abs((a1.astype(np.float64) - aref + 180.0) % 360.0 - 180.0)
    cmp = present & ok
    assert np.all(diff[cmp] <= np.spacing(aref.astype(np.float32))[cmp] + 360.0 / res * tol[cmp]), "%s: ang against the restatement" % what
    cmpd = present & ok & np.isfinite(tol) & (tol > 0)
    worst = float(np.max(err[cmpd] / tol[cmpd])) if cmpd.any() else 0.0
    return worst, int(present.sum()), int((present & either).sum())


def _oracle(items, table, m, n):
    _, _, _, s64, w = oracle_fp64(items, table, m, n)
    with np.errstate(divide="ignore"):
        return 1.0 / s64, s64, w


# name, m, n, K, res, batch, array (None: line array), environment; "60dB": sigma = 1e-3 and emitters on the table's bins -- the
# nulls fall below the projector form's threshold and the three values take the literal form
SHAPES = [
    ("cfg1", 4, 2, 64, 360, 48, mo.array_geometry(4), {}),                     # m = 4, two kernels
    ("cfg2", 4, 2, 256, 3600, 24, mo.array_geometry(4), {}),                   # m = 4, fused covariance + EVD
    ("cfg3", 8, 2, 512, 36000, 6, mo.array_geometry(8), {}),                   # int8 with the port, coarse-gated without
    ("m7_n4_lds_jacobi", 7, 4, 64, 720, 23, None, {}),
    ("m12_n2_short_form", 12, 2, 64, 720, 23, None, {"BAZ_MUSIC_EXACT": "1"}),  # no projector coefficients: literal form
    ("m12_n2_int8", 12, 2, 64, 720, 23, None, {}),
    ("m16_n3", 16, 3, 256, 360, 23, None, {}),
    ("m4_60dB_literal", 4, 2, 256, 720, 23, mo.array_geometry(4), {}),
    ("m8_n3_60dB_literal", 8, 3, 64, 720, 23, None, {}),
]


@pytest.mark.parametrize("name,m,n,K,res,batch,arr,env", SHAPES, ids=[s[0] for s in SHAPES])
def test_definition_parity(name, m, n, K, res, batch, arr, env, gpu_device, monkeypatch):
    capi = _capi()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name.startswith("cfg"):
        c = mo.make_config(name, batch, snr_db=20.0, seed=77)
        items, table = c["items"], c["table"]
        assert (c["m"], c["n"], c["nsamples"], c["res"]) == (m, n, m * K, res)
    else:
        arr = oref.ula(m) if arr is None else arr
        table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
        hot = "60dB" in name
        items, _ = oref.scene(batch, m, K, n, 1e-3 if hot else 0.1, seed=500 + m, arr=arr, grid=360.0 / res if hot else None)
    d, s64, w = _oracle(items, table, m, n)
    with capi.Context(m, n, m * K, res, table) as ctx:
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            for spectrum in (True, False):
                what = "%s peak=%d spectrum=%d" % (name, peak, spectrum)
                off_out, on_out, off = _both_modes(ctx, items, want_spectrum=spectrum)
                present = off_out[1] != 0
                tol, either = rr.tolerance(m, n, table, s64, w, rr.bins_of(off_out[0], res))
                worst, entries, loose = _assert_definition(off_out, on_out, off, d, tol, either, present, res, what)
                print("%s: %d entries, %d moved, %d either-branch, worst err/tol %.3g, largest tol %.3g bins"
                      % (what, entries, np.count_nonzero(off), loose, worst, float(np.max(tol[present & np.isfinite(tol)]))))
                assert entries > 0
                if peak:
                    assert np.count_nonzero(off) >= entries // 2


def test_order_mode_mixed_counts(gpu_device):
    capi = _capi()
    m, K, n_max, res = 8, 64, 3, 720
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    parts = [oref.scene(16, m, K, e, 0.1, 900 + 17 * e, arr=arr)[0] for e in range(n_max + 1)]
    items = np.concatenate(parts)[np.random.default_rng(9).permutation(16 * (n_max + 1))]
    B = len(items)
    with capi.Context(m, n_max, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.set_peak_mode(1)
        off_out, on_out, off = _both_modes(ctx, items)
        orders = ctx.last_orders(B)
    assert set(np.unique(orders)) == set(range(n_max + 1))
    present = off_out[1] != 0
    d = np.full((B, res), np.nan)
    tol = np.full((B, n_max), np.inf)
    either = np.zeros((B, n_max), bool)
    bins = rr.bins_of(off_out[0], res)
    for k in range(1, n_max + 1):
        idx = np.nonzero(orders == k)[0]
        dk, s64, w = _oracle(items[idx], table, m, k)
        d[idx] = dk
        tol[idx], either[idx] = rr.tolerance(m, k, table, s64, w, bins[idx])
    for b in range(B):
        assert not present[b, orders[b]:].any() and not off[b, orders[b]:].any()
    d[orders == 0] = 1.0                                                   # (count 0: no entry, nothing is read)
    worst, entries, loose = _assert_definition(off_out, on_out, off, d, tol, either, present, res, "order mode")
    print("order mode: %d entries, %d moved, %d either-branch, worst err/tol %.3g" % (entries, np.count_nonzero(off), loose, worst))
    assert np.count_nonzero(off) >= entries // 2


def test_smoothing_fb_ss6(gpu_device):
    capi = _capi()
    res, m, n, K, ms = 720, 8, 2, 64, 6
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = sr.two_emitters(40, arr, K, coherent=True, seed=2024)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_refine_mode(1)
        ctx.set_smoothing(ms, True)
        assert ctx.get_refine_mode() == 1                                  # set_smoothing forwards the mode ...
        a_fwd, _, _ = ctx.process(items)
        off_fwd = ctx.last_refine_offsets(len(items) * n).reshape(-1, n)
        assert np.count_nonzero(off_fwd)
        off_out, on_out, off = _both_modes(ctx, items)                     # ... and set_refine_mode reaches the inner context
        assert np.array_equal(off, off_fwd) and np.array_equal(_f32bits(on_out[0]), _f32bits(a_fwd))
    y = sr.restack(items, m, ms, True, capi.smoothing_check(m, res, table, ms, True))
    sub = table[:, :ms]
    d, s64, w = _oracle(y, sub, ms, n)
    present = off_out[1] != 0
    tol, either = rr.tolerance(ms, n, sub, s64, w, rr.bins_of(off_out[0], res))
    worst, entries, loose = _assert_definition(off_out, on_out, off, d, tol, either, present, res, "FB + SS(6)")
    print("FB + SS(6): %d entries, %d moved, %d either-branch, worst err/tol %.3g" % (entries, np.count_nonzero(off), loose, worst))


@pytest.mark.parametrize("cfg,batch", [("cfg1", 1000), ("cfg2", 300)])
def test_host_paths_equal_the_device_path(cfg, batch, gpu_device, monkeypatch):
    """One device call, one host-fed call and a host-fed call cut into chunks: identical ang / lvl / spectrum / offset bits."""
    import torch
    capi = _capi()
    c = mo.make_config(cfg, batch, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    items = c["items"]
    outs = []
    for how in ("device", "host", "chunked"):
        if how == "chunked":
            monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            ctx.set_peak_mode(1)
            ctx.set_refine_mode(1)
            if how == "device":
                x = torch.from_numpy(items.view(np.float32)).cuda()
                d_ang = torch.full((batch, n), 7.0, dtype=torch.float32, device="cuda")
                d_lvl = torch.full((batch, n), 7.0, dtype=torch.float32, device="cuda")
                d_spec = torch.zeros(batch, res, dtype=torch.float32, device="cuda")
                ctx.process_device(x.data_ptr(), batch, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                out = (d_ang.cpu().numpy(), d_lvl.cpu().numpy(), d_spec.cpu().numpy())
            else:
                out = ctx.process(items)
            off = ctx.last_refine_offsets(batch * n)
            assert len(off) == batch * n
            assert np.array_equal(ctx.last_refine_offsets(10), off[:10])
            outs.append(out + (off,))
    assert np.count_nonzero(outs[0][3]) > batch
    for o in outs[1:]:
        for a, b in zip(outs[0][:3], o[:3]):
            assert np.array_equal(_f32bits(a), _f32bits(b))
        assert np.array_equal(outs[0][3].view(np.uint64), o[3].view(np.uint64))


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    """A context never set, one set to 0 and one switched on and off again: identical bits, and identical launch counts of the
    stage the refinement belongs to (mode 1 adds exactly one launch per call)."""
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=92)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs, launches = [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_refine_mode(0)
            if how == "on_then_off":
                ctx.set_refine_mode(1)
                ctx.profile(1)
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                on_launches = [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]
                ctx.set_refine_mode(0)
            assert ctx.get_refine_mode() == 0
            ctx.profile(1)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            assert not ctx.last_refine_offsets(batch * n).any()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b))
    assert launches[0] == launches[1] == launches[2], launches
    want = list(launches[0])
    want[capi.STAGE_MERGE] += 2                                            # two calls, one refine_kernel each
    assert on_launches == want, (on_launches, launches[0])


@pytest.mark.parametrize("case", [k for k in sorted(EFFECT) if k[0] == "cfg1" and k[1] in (40.0, 10.0)],
                         ids=lambda c: "%s_%gdB_%g" % (c[0], c[1], c[3][0]))
def test_device_effect(case, gpu_device):
    """The cfg1 rows of the effect table, produced by the device with peak mode 1; the assertions of the CPU table."""
    capi = _capi()
    cfg, snr, batch, truth = case
    c = mo.make_config(cfg, batch, snr_db=snr, seed=77, angles_deg=truth)
    with capi.Context(c["m"], c["n"], c["nsamples"], c["res"], c["table"]) as ctx:
        ctx.set_peak_mode(1)
        off_out, on_out, off = _both_modes(ctx, c["items"], want_spectrum=False)
    present = off_out[1] != 0
    grid, refined = effect_rms(off_out[0], on_out[0], present, truth)
    print("device %s %g dB emitters %s: %d entries, %d moved, grid %.4g deg, refined %.4g deg, ratio %.3g (oracle: %.4g, %.4g)"
          % ((cfg, snr, truth, int(present.sum()), np.count_nonzero(off), grid, refined, grid / refined) + EFFECT[case]))
    if snr == 40.0:
        assert refined <= grid / 5.0
    else:
        assert refined <= 1.05 * grid


def test_retune_to_a_rotated_table(gpu_device):
    capi = _capi()
    c = mo.make_config("cfg1", 64, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    rotated = np.ascontiguousarray(np.roll(c["table"], 37, axis=0))
    with capi.Context(m, n, N, res, c["table"]) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_refine_mode(1)
        a_old, _, _ = ctx.process(c["items"])
        ctx.set_table(rotated)
        off_out, on_out, off = _both_modes(ctx, c["items"])
    d, s64, w = _oracle(c["items"], rotated, m, n)
    present = off_out[1] != 0
    tol, either = rr.tolerance(m, n, rotated, s64, w, rr.bins_of(off_out[0], res))
    worst, entries, _ = _assert_definition(off_out, on_out, off, d, tol, either, present, res, "rotated table")
    assert np.count_nonzero(off) == entries
    # the same items 37 bins further round the circle
    shift = (on_out[0].astype(np.float64) - a_old.astype(np.float64)) % 360.0
    assert np.all(np.abs(shift - 37.0) <= 1e-3), shift


def test_scope_wide_arrays_and_invalid_modes(gpu_device):
    capi = _capi()
    m = 24
    table = mo.steering_table_c64(oref.ula(m), 360, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, 2, m * 32, 360, table) as ctx:
        with pytest.raises(capi.MusicError) as e:
            ctx.set_refine_mode(1)
        assert e.value.code == capi.E_UNSUPPORTED
        assert ctx.get_refine_mode() == 0
        ctx.set_refine_mode(0)
        assert capi.lib().baz_music_set_refine_mode(ctx._h, 2) == capi.E_INVALID
    c = mo.make_config("cfg1", 8, seed=3)
    with capi.Context(c["m"], c["n"], c["nsamples"], c["res"], c["table"]) as ctx:
        ctx.set_refine_mode(1)
        for bad in (2, -1, 7):
            assert capi.lib().baz_music_set_refine_mode(ctx._h, bad) == capi.E_INVALID
            assert ctx.get_refine_mode() == 1                              # the previous mode stays in force


def test_missing_entries_stay_zero_without_lvl(gpu_device):
    """lvl not wired.  Peak mode: an item with fewer local maxima than n (a NaN item has none; one emitter against n = 3 leaves
    fewer than three).  Emitter-count mode: a count-0 item."""
    capi = _capi()
    m, K, n, res = 4, 64, 3, 360
    arr = mo.array_geometry(4)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(40, m, K, 1, 0.01, seed=31, arr=arr)
    items[7, 5] = np.nan
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_peak_mode(1)
        (a0, l0, _), _, _ = _both_modes(ctx, items)                         # (with lvl: which entries exist)
        missing = l0 == 0
        off_out, on_out, off = _both_modes(ctx, items, want_spectrum=False, want_lvl=False)
        assert on_out[1] is None
        assert missing[7].all() and missing.sum() > n, "no item with fewer local maxima than n"
        assert not on_out[0][missing].any() and not off[missing].any()
        assert np.count_nonzero(off[~missing]) >= (~missing).sum() // 2
        assert np.array_equal(_f32bits(off_out[0]), _f32bits(a0))
    noise, _ = oref.scene(8, m, K, 0, 0.1, seed=32, arr=arr)
    mixed = np.concatenate([items[:8], noise])
    with capi.Context(m, 2, m * K, res, table) as ctx:
        ctx.set_order_mode("mdl")
        ctx.set_refine_mode(1)
        ang, lvl, _ = ctx.process(mixed, want_lvl=False, want_spectrum=False)
        orders = ctx.last_orders(len(mixed))
        off = ctx.last_refine_offsets(len(mixed) * 2).reshape(-1, 2)
        assert lvl is None and (orders[8:] == 0).all() and (orders[:7] == 1).all()
        assert not ang[8:].any() and not off[8:].any()
        assert not ang[:8, 1].any() and not off[:8, 1].any()
        assert np.count_nonzero(off[:7, 0]) >= 4


def test_bin_zero_wraps_below_360(gpu_device):
    """An emitter at 359.7 degrees on the cfg1 grid: the entry at bin 0 moves down and is reported just under 360."""
    capi = _capi()
    truth = (359.7, 121.7)
    c = mo.make_config("cfg1", 64, snr_db=40.0, seed=77, angles_deg=truth)
    with capi.Context(c["m"], c["n"], c["nsamples"], c["res"], c["table"]) as ctx:
        ctx.set_peak_mode(1)
        off_out, on_out, off = _both_modes(ctx, c["items"])
    at0 = (off_out[1] != 0) & (off_out[0] == 0.0)
    assert at0.sum() >= 32, "the emitter is not reported at bin 0"
    assert np.all(off[at0] < 0.0)
    assert np.all((on_out[0][at0] > 359.5) & (on_out[0][at0] < 360.0))
    assert np.array_equal(_f32bits(on_out[0][at0]), _f32bits(rr.angle(np.zeros(at0.sum(), np.int64), off[at0], c["res"])))
    err = rr.angle_error_deg(on_out[0][at0], truth)
    print("emitter at 359.7: %d entries at bin 0, refined RMS error %.4g deg" % (at0.sum(), float(np.sqrt(np.mean(err ** 2)))))
