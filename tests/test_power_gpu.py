"""Opt-in per-emitter Capon power estimate (baz_music_set_power_mode) on the MI355X: the fp64 tap (last_powers) of every reported
entry against power_ref on the device's own covariance (debug_cov) and the device's own bins, for every group width, frontend and
scan form up to 16 antennas, with and without the spectrum port, under both pickers; mode 1 == mode 0 bit for bit on every port;
mode 2 puts float32(P) on lvl; the emitter-count mode, refinement, averaging and smoothing; host path == device path; mode off ==
the reference with no extra launch; degenerate items; retune; scope; the effect table of DESIGN.md 8f produced by the device.

Tolerance: relative 8 m cond_2(R) 2^-52 per item (power_ref.tolerance)."""
import numpy as np
import pytest

import averaging_ref as ar
import order_ref as oref
import power_ref as pr
import smoothing_ref as sr
from oracle import music_oracle as mo
from test_power import EFFECT_AMP, EFFECT_RANGE, effect_scene

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _f64bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _device_cov(ctx, items, m):
    """R of every item as the context's own covariance stage computes it (debug_cov), (B, m, m) complex128."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    R = torch.zeros(len(items) * m * m * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_cov(x.data_ptr(), len(items), R.data_ptr())
    ctx.sync()
    return R.cpu().numpy().view(np.complex128).reshape(len(items), m, m)


def _three_modes(ctx, items, want_spectrum=True, before=None):
    """Modes 0, 1, 2 on the same items: (ports of mode 0, of mode 1, of mode 2, tap of mode 1 (B, n)).  before: called in front of
    every process call (averaging: reset the stream)."""
    B, n = len(items), ctx.n
    outs, taps = [], []
    for mode in (0, 1, 2):
        ctx.set_power_mode(mode)
        assert ctx.get_power_mode() == mode
        if before:
            before()
        outs.append(ctx.process(items, want_spectrum=want_spectrum))
        tap = ctx.last_powers(B * n)
        assert len(tap) == B * n
        taps.append(tap.reshape(B, n))
    ctx.set_power_mode(0)
    assert not taps[0].any()                                               # a call with the mode off reports zeros
    assert np.array_equal(_f64bits(taps[1]), _f64bits(taps[2]))
    return outs[0], outs[1], outs[2], taps[1]


def _assert_definition(o0, o1, o2, tap, R, table, res, what="", present=None):
    """Mode 1 ports == mode 0 bit for bit; the tap within tolerance of power_ref on R at the device's own bins; missing entries 0;
    mode 2: lvl bits == float32(tap), ang and spectrum unchanged.  Returns (worst |err| / (m cond 2^-52 P), entries)."""
    a0, l0, s0 = o0
    for name, o in (("mode 1", o1), ("mode 2", o2)):
        assert np.array_equal(_f32bits(a0), _f32bits(o[0])), "%s %s: ang changed" % (what, name)
        if s0 is not None:
            assert np.array_equal(_f32bits(s0), _f32bits(o[2])), "%s %s: the spectrum changed" % (what, name)
    assert np.array_equal(_f32bits(l0), _f32bits(o1[1])), "%s mode 1: lvl changed" % what
    with np.errstate(over="ignore"):
        assert np.array_equal(_f32bits(o2[1]), _f32bits(tap.astype(np.float32))), "%s mode 2: lvl is not float32(P)" % what
    present = (l0 != 0) if present is None else present
    assert not tap[~present].any(), "%s: a missing entry has a power" % what
    m = R.shape[1]
    bins = pr.bins_of(a0, res)
    ref = pr.powers(R, table, bins, present)
    tol = pr.tolerance(R)[:, None] * np.ones(bins.shape)
    live = present & (ref != 0)
    assert np.array_equal(tap == 0, ref == 0), "%s: the degenerate / missing entries differ" % what
    rel = np.zeros(bins.shape)
    rel[live] = np.abs(tap[live] - ref[live]) / ref[live]
    bad = live & ~(rel <= tol)
    if bad.any():
        b, i = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError("%s item %d slot %d (bin %d): P %.17g, power_ref %.17g, relative %.3g > tol %.3g"
                             % (what, b, i, bins[b, i], tap[b, i], ref[b, i], rel[b, i], tol[b, i]))
    worst = float(np.max(rel[live] / (tol[live] / 8.0))) if live.any() else 0.0
    return worst, int(live.sum())


# name, m, n, K, res, batch, sigma, environment.  Line arrays.  Batches of 23 leave wave groups partly empty.
SHAPES = [
    ("m2_n1", 2, 1, 32, 90, 23, 0.1, {}),
    ("m3_n2", 3, 2, 100, 357, 23, 0.1, {}),
    ("m4_two_kernels", 4, 2, 64, 360, 48, 0.1, {}),
    ("m4_fused", 4, 2, 256, 360, 24, 0.1, {}),
    ("m5_n3", 5, 3, 200, 720, 23, 0.1, {}),
    ("m7_n4", 7, 4, 64, 720, 23, 0.1, {}),
    ("m8_int8_coarse", 8, 2, 512, 720, 6, 0.1, {}),
    ("m12_n2", 12, 2, 64, 720, 23, 0.1, {}),
    ("m12_n2_short_form", 12, 2, 64, 720, 23, 0.1, {"BAZ_MUSIC_EXACT": "1"}),
    ("m16_n15", 16, 15, 64, 360, 23, 0.1, {}),
    ("batch_of_1", 8, 2, 64, 360, 1, 0.1, {}),
    ("m8_60dB", 8, 2, 64, 720, 23, 1e-3, {}),
]


@pytest.mark.parametrize("name,m,n,K,res,batch,sigma,env", SHAPES, ids=[s[0] for s in SHAPES])
def test_definition_parity(name, m, n, K, res, batch, sigma, env, gpu_device, monkeypatch):
    capi = _capi()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    arr = oref.ula(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    # (at most 4 emitters: the scene keeps them 20 degrees apart inside [20, 160]; the slots beyond them hold whatever the picker finds)
    items, _ = oref.scene(batch, m, K, min(n, 4), sigma, seed=500 + m, arr=arr, grid=360.0 / res if sigma < 0.01 else None)
    worst_all = 0.0
    with capi.Context(m, n, m * K, res, table) as ctx:
        if name == "m4_fused":
            assert ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"
        R = _device_cov(ctx, items, m)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            for spectrum in (True, False):
                what = "%s peak=%d spectrum=%d" % (name, peak, spectrum)
                o0, o1, o2, tap = _three_modes(ctx, items, want_spectrum=spectrum)
                worst, entries = _assert_definition(o0, o1, o2, tap, R, table, res, what)
                worst_all = max(worst_all, worst)
                print("%s: %d entries, worst err / (m cond 2^-52) %.3g (bound 8), largest cond %.3g"
                      % (what, entries, worst, float(np.max(pr.tolerance(R))) / (8.0 * m * pr.EPS)))
                assert entries > 0
        if name == "m4_fused":
            ctx.set_power_mode(1)
            assert ctx.stage_name(capi.STAGE_COV) == "bazmusic::cov4_evd_kernel"   # the fused kernel keeps running (with its R tap)
    print("%s: worst over the four wirings %.3g" % (name, worst_all))


def test_mode_2_without_lvl_behaves_as_mode_1(gpu_device):
    capi = _capi()
    m, n, K, res = 8, 2, 64, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(23, m, K, n, 0.1, seed=61)
    with capi.Context(m, n, m * K, res, table) as ctx:
        a0, _, s0 = ctx.process(items, want_lvl=False)
        ctx.set_power_mode(1)
        ctx.process(items)
        want = ctx.last_powers(23 * n)
        ctx.set_power_mode(2)
        a2, l2, s2 = ctx.process(items, want_lvl=False)
        got = ctx.last_powers(23 * n)
    assert l2 is None and np.count_nonzero(want) == 23 * n
    assert np.array_equal(_f64bits(got), _f64bits(want))
    assert np.array_equal(_f32bits(a0), _f32bits(a2)) and np.array_equal(_f32bits(s0), _f32bits(s2))


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
            o0, o1, o2, tap = _three_modes(ctx, items)
            orders = ctx.last_orders(B)
            assert set(np.unique(orders)) == set(range(n_max + 1))
            for b in range(B):
                assert not tap[b, orders[b]:].any() and not o2[1][b, orders[b]:].any() and not o2[0][b, orders[b]:].any()
            worst, entries = _assert_definition(o0, o1, o2, tap, R, table, res, "order mode peak=%d" % peak)
            print("order mode peak=%d: %d entries, worst err / (m cond 2^-52) %.3g" % (peak, entries, worst))
            if not peak:
                assert entries == int(orders.sum())


def test_refine_with_power_mode_2(gpu_device):
    """ang == refine-only ang bit for bit; lvl == the power at the GRID bin (recovered from the unrefined ang)."""
    capi = _capi()
    m, n, K, res = 8, 2, 64, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(23, m, K, n, 0.03, seed=77)
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        ctx.set_peak_mode(1)
        grid = ctx.process(items)
        ctx.set_refine_mode(1)
        refined = ctx.process(items)
        off = ctx.last_refine_offsets(23 * n)
        for mode in (1, 2):
            ctx.set_power_mode(mode)
            both = ctx.process(items)
            tap = ctx.last_powers(23 * n).reshape(23, n)
            assert np.array_equal(_f64bits(ctx.last_refine_offsets(23 * n)), _f64bits(off))
            assert np.array_equal(_f32bits(both[0]), _f32bits(refined[0])), "mode %d: ang differs from refine-only" % mode
            assert np.array_equal(_f32bits(both[2]), _f32bits(refined[2]))
            want_lvl = refined[1] if mode == 1 else tap.astype(np.float32)
            assert np.array_equal(_f32bits(both[1]), _f32bits(want_lvl)), "mode %d: lvl" % mode
            both_nolvl = ctx.process(items, want_lvl=False, want_spectrum=False)
            assert np.array_equal(_f32bits(both_nolvl[0]), _f32bits(refined[0]))
            assert np.array_equal(_f64bits(ctx.last_powers(23 * n).reshape(23, n)), _f64bits(tap))
    assert np.count_nonzero(off) >= 23 and not np.array_equal(_f32bits(grid[0]), _f32bits(refined[0]))
    present = grid[1] != 0
    ref = pr.powers(R, table, pr.bins_of(grid[0], res), present)
    tol = pr.tolerance(R)[:, None]
    assert np.all(np.abs(tap - ref) <= tol * ref) and np.count_nonzero(ref) == present.sum()


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
        o0, o1, o2, tap = _three_modes(ctx, items, before=ctx.reset_averaging)
    worst, entries = _assert_definition(o0, o1, o2, tap, Rbar, table, res, "averaging W=3 m=%d" % m)
    assert (o0[1][:2] != 0).any() and tap[:2].any()                        # the first two items of the stream average fewer taps
    print("averaging W=3 m=%d: %d entries, worst err / (m cond 2^-52) %.3g" % (m, entries, worst))


def test_smoothing_fb_ss6(gpu_device):
    capi = _capi()
    res, m, n, K, ms = 720, 8, 2, 64, 6
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = sr.two_emitters(40, arr, K, coherent=True, seed=2024)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_power_mode(1)
        ctx.set_smoothing(ms, True)
        assert ctx.get_power_mode() == 1                                   # set_smoothing forwards the mode ...
        ctx.process(items)
        tap_fwd = ctx.last_powers(len(items) * n).reshape(-1, n)
        assert np.count_nonzero(tap_fwd)
        o0, o1, o2, tap = _three_modes(ctx, items)                         # ... and set_power_mode reaches the inner context
        assert np.array_equal(_f64bits(tap), _f64bits(tap_fwd))
    y = sr.restack(items, m, ms, True, capi.smoothing_check(m, res, table, ms, True))
    R = sr.covariance(y, ms)
    worst, entries = _assert_definition(o0, o1, o2, tap, R, table[:, :ms], res, "FB + SS(6)")
    print("FB + SS(6): %d entries, worst err / (m cond 2^-52) %.3g" % (entries, worst))


@pytest.mark.parametrize("cfg,batch", [("cfg1", 1000), ("cfg2", 300)])
def test_host_paths_equal_the_device_path(cfg, batch, gpu_device, monkeypatch):
    """One device call, one host-fed call and a host-fed call cut into chunks: identical ang / lvl / spectrum / power bits."""
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
            ctx.set_power_mode(2)
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
            tap = ctx.last_powers(batch * n)
            assert len(tap) == batch * n
            assert np.array_equal(ctx.last_powers(10), tap[:10])
            outs.append(out + (tap,))
    assert np.count_nonzero(outs[0][3]) > batch
    assert np.array_equal(_f32bits(outs[0][1]).ravel(), _f32bits(outs[0][3].astype(np.float32)))
    for o in outs[1:]:
        for a, b in zip(outs[0][:3], o[:3]):
            assert np.array_equal(_f32bits(a), _f32bits(b))
        assert np.array_equal(_f64bits(outs[0][3]), _f64bits(o[3]))


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg2", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    """A context never set, one set to 0 and one switched on and off again: identical bits, and identical launch counts of every
    stage (mode 1 adds exactly one launch per call, under the merge stage)."""
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=92)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs, launches = [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_power_mode(0)
            if how == "on_then_off":
                ctx.set_power_mode(1)
                ctx.profile(1)
                ctx.process(c["items"])
                ctx.process(c["items"], want_spectrum=False)
                on_launches = [ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)]
                ctx.set_power_mode(0)
            assert ctx.get_power_mode() == 0
            ctx.profile(1)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            assert not ctx.last_powers(batch * n).any()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(_f32bits(a), _f32bits(b))
    assert launches[0] == launches[1] == launches[2], launches
    want = list(launches[0])
    want[capi.STAGE_MERGE] += 2                                            # two calls, one power_kernel each
    assert on_launches == want, (on_launches, launches[0])


@pytest.mark.parametrize("m,n,K", [(4, 2, 64), (8, 2, 64), (16, 3, 64)], ids=["m4", "m8", "m16"])
def test_degenerate_items_in_the_middle_of_a_wave(m, n, K, gpu_device):
    capi = _capi()
    res, B = 360, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(B, m, K, n, 0.1, seed=40 + m)
    items[3] = 0
    items[5, 7] = np.nan
    with capi.Context(m, n, m * K, res, table) as ctx:
        R = _device_cov(ctx, items, m)
        for peak in (0, 1):
            ctx.set_peak_mode(peak)
            o0, o1, o2, tap = _three_modes(ctx, items)
            assert not tap[3].any() and not tap[5].any()
            assert not o2[1][3].any() and not o2[1][5].any()
            good = np.ones(B, bool)
            good[[3, 5]] = False
            assert np.all(tap[good][o0[1][good] != 0] > 0)
            worst, entries = _assert_definition(o0, o1, o2, tap, R, table, res, "degenerate m=%d peak=%d" % (m, peak))
            assert entries >= (B - 2)


def test_fewer_snapshots_than_antennas(gpu_device):
    capi = _capi()
    m, n, N, res = 4, 2, 8, 360
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items, _ = oref.scene(23, m, N // m, n, 0.1, seed=12)
    with capi.Context(m, n, N, res, table) as ctx:
        o0, o1, o2, tap = _three_modes(ctx, items)
    assert (o0[1] != 0).any()
    assert not tap.any() and not o2[1].any()
    assert np.array_equal(_f32bits(o2[0]), _f32bits(o0[0])) and np.array_equal(_f32bits(o1[1]), _f32bits(o0[1]))


def test_retune_to_a_rotated_table(gpu_device):
    capi = _capi()
    c = mo.make_config("cfg1", 64, snr_db=30.0, seed=77)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    rotated = np.ascontiguousarray(np.roll(c["table"], 37, axis=0))
    with capi.Context(m, n, N, res, c["table"]) as ctx:
        R = _device_cov(ctx, c["items"], m)
        ctx.set_peak_mode(1)
        ctx.set_power_mode(1)
        a_old, l_old, _ = ctx.process(c["items"])
        tap_old = ctx.last_powers(64 * n).reshape(64, n)
        ctx.set_table(rotated)
        o0, o1, o2, tap = _three_modes(ctx, c["items"])
    worst, entries = _assert_definition(o0, o1, o2, tap, R, rotated, res, "rotated table")
    assert entries == 64 * n
    # the same rows 37 bins further round the circle: the same powers
    b_old, b_new = pr.bins_of(a_old, res), (pr.bins_of(o0[0], res) - 37) % res
    io, inw = np.argsort(b_old, axis=1), np.argsort(b_new, axis=1)
    assert np.array_equal(np.take_along_axis(b_old, io, 1), np.take_along_axis(b_new, inw, 1))
    assert np.array_equal(_f64bits(np.take_along_axis(tap_old, io, 1)), _f64bits(np.take_along_axis(tap, inw, 1)))


def test_scope_wide_arrays_and_invalid_modes(gpu_device):
    capi = _capi()
    m = 17
    table = mo.steering_table_c64(oref.ula(m), 360, mo.FREQUENCY, mo.SPACING)
    with capi.Context(m, 2, m * 32, 360, table) as ctx:
        for mode in (1, 2):
            with pytest.raises(capi.MusicError) as e:
                ctx.set_power_mode(mode)
            assert e.value.code == capi.E_UNSUPPORTED
            assert ctx.get_power_mode() == 0
        ctx.set_power_mode(0)
        assert capi.lib().baz_music_set_power_mode(ctx._h, 3) == capi.E_INVALID
    c = mo.make_config("cfg1", 8, seed=3)
    with capi.Context(c["m"], c["n"], c["nsamples"], c["res"], c["table"]) as ctx:
        for keep in (1, 2):
            ctx.set_power_mode(keep)
            for bad in (3, -1, 7):
                assert capi.lib().baz_music_set_power_mode(ctx._h, bad) == capi.E_INVALID
                assert ctx.get_power_mode() == keep                        # the previous mode stays in force


def test_device_effect(gpu_device):
    """The scene of test_power.test_effect_table on the device under peak mode 1: entries within one bin of a true angle.
    The context asks for n = 4 entries per item: a line array cannot tell theta from 360 - theta, every emitter has a mirror
    peak of the same height, and with two entries the picker reports the stronger emitter and its mirror (the fp64 oracle's
    peak_pick does the same: 64 of 128 matched at n = 2, all 128 at n = 4).  R and P do not depend on n."""
    capi = _capi()
    items, ang, table, m, K, res = effect_scene()
    n = 4
    true_bins = np.rint(ang * res / 360.0).astype(np.int64)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_power_mode(1)
        a, l, _ = ctx.process(items)
        tap = ctx.last_powers(len(items) * n).reshape(-1, n)
    bins = pr.bins_of(a, res)
    ratios = [[], []]
    for b in range(len(items)):
        for e in range(2):
            hit = (l[b] != 0) & (np.abs(bins[b] - true_bins[b, e]) <= 1)
            if hit.any():
                ratios[e].append(tap[b][hit][0] / EFFECT_AMP[e] ** 2)
    matched = len(ratios[0]) + len(ratios[1])
    print("device effect: %d of %d emitters matched" % (matched, 2 * len(items)))
    assert matched >= 0.9 * 2 * len(items)
    means = [float(np.mean(r)) for r in ratios]
    print("device effect: mean P / amp^2 %.4g %.4g" % (means[0], means[1]))
    assert all(EFFECT_RANGE[0] <= v <= EFFECT_RANGE[1] for v in means), means
