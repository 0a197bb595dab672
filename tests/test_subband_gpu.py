"""The opt-in wideband (subband) mode (baz_music_set_subbands) on the MI355X: the channeliser kernel against the host
routine bit for bit; a context with the mode on against S plain contexts on the channelised items, their spectra through the numpy
combine and pickers, bit for bit on every port; the estimators with the arithmetic rule; covariance averaging; the known answer;
chunking; refusals; off == the context never set; a setter beside a submitting thread."""
import threading

import numpy as np
import pytest

import subband_ref as sr
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

RES = 360


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x).view(np.float32).view(np.uint32)


def _table(m, res=RES):
    return mo.steering_table_c64(mo.array_geometry(m), res, mo.FREQUENCY, mo.SPACING)


def _items(m, batch, k, seed, angles=(40.0, 62.0)):
    return mo.synth_items(batch, m, m * k, mo.array_geometry(m), mo.FREQUENCY, mo.SPACING, angles_deg=angles, snr_db=20.0, seed=seed)


def _tables(m, F, bins, res=RES):
    return sr.tables(m, mo.FREQUENCY, sr.FS_OVER_FC * mo.FREQUENCY, F, bins, res)


def _run_device(ctx, items, want_spectrum=True, want_lvl=True):
    """One process_device call into buffers pre-filled with NaN: (ang, lvl | None, spectrum | None)."""
    import torch
    nb = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    d_ang = torch.full((nb, ctx.n), float("nan"), dtype=torch.float32, device="cuda")
    d_lvl = torch.full((nb, ctx.n), float("nan"), dtype=torch.float32, device="cuda") if want_lvl else None
    d_spec = torch.full((nb, ctx.res), float("nan"), dtype=torch.float32, device="cuda") if want_spectrum else None
    ctx.process_device(x.data_ptr(), nb, d_ang.data_ptr(), d_lvl.data_ptr() if want_lvl else None,
                       d_spec.data_ptr() if want_spectrum else None, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ang.cpu().numpy(), d_lvl.cpu().numpy() if want_lvl else None, d_spec.cpu().numpy() if want_spectrum else None


def _same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        if u is None or v is None:
            continue
        assert np.array_equal(_f32bits(u), _f32bits(v)), "%s: port %d differs" % (what, k)


def _channelise_device(ctx, items, S, guard_words=64):
    """debug_subbands on items (batch, m K) -> (S, batch, m Q) complex64, and the guard row behind the output."""
    import torch
    nb = len(items)
    F = ctx.get_subbands()[0]
    per = items.shape[1] // F                      # complex64 of one subband's item: m Q
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    out = torch.full((S * nb * per * 2 + guard_words,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_subbands(x.data_ptr(), nb, out.data_ptr())
    ctx.sync()
    o = out.cpu().numpy()
    return o[:S * nb * per * 2].view(np.complex64).reshape(S, nb, per), o[S * nb * per * 2:]


def _reference(capi, m, n, q, tabs, y, peak, estimator=0, arithmetic=False, averaging=None, calls=1):
    """S plain contexts of shape (m, n, m q, RES), context s on table s and subband s's items y[s]; their spectra through the numpy
    combine and pickers: `calls` results (ang, lvl, spectrum), the same items submitted again each time."""
    spectra = [[] for _ in range(calls)]
    for s in range(len(tabs)):
        with capi.Context(m, n, m * q, RES, tabs[s]) as plain:
            if estimator:
                plain.set_estimator(estimator)
            if averaging:
                plain.set_averaging(averaging)
            for c in range(calls):
                spectra[c].append(_run_device(plain, y[s])[2])
    out = []
    for c in range(calls):
        row = sr.combine(np.stack(spectra[c]), arithmetic=arithmetic)
        ang, lvl = sr.pick(row, n, peak)
        out.append((ang, lvl, row))
    return out


# ---- 1. the channeliser, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,F,S,blocks,batch", [(2, 2, 1, 1, 5), (3, 3, 3, 5, 3), (4, 8, 7, 16, 4), (16, 64, 32, 2, 2), (7, 16, 13, 9, 3)])
def test_channeliser_equals_the_host_routine(m, F, S, blocks, batch, gpu_device):
    capi = _capi()
    rng = np.random.default_rng(m * 100 + F)
    k = F * blocks
    bins = sorted(rng.choice(F, S, replace=False).tolist(), key=lambda b: (b * 7) % F + b / 100.0)      # (distinct, not ascending)
    items = (rng.standard_normal((batch, m * k)) + 1j * rng.standard_normal((batch, m * k))).astype(np.complex64)
    t_nan = (blocks // 2) * F + F - 1
    items[1, t_nan * m + m - 1] = np.nan                      # one sample of item 1: block blocks // 2, the last antenna
    table = (rng.standard_normal((RES, m)) + 1j * rng.standard_normal((RES, m))).astype(np.complex64)
    tabs = (rng.standard_normal((S, RES, m)) + 1j * rng.standard_normal((S, RES, m))).astype(np.complex64)
    with capi.Context(m, 1, m * k, RES, table) as ctx:
        with pytest.raises(capi.MusicError) as e:
            ctx.debug_subbands(1, 1, 2)                      # (refused before anything is touched: the mode is off)
        assert e.value.code == capi.E_UNSUPPORTED
        ctx.set_subbands(F, bins, tabs)
        assert ctx.get_subbands() == (F, bins, capi.SUBBAND_HARMONIC)
        got, guard = _channelise_device(ctx, items, S)
    W = capi.subband_twiddles(F, bins)
    want = capi.subband_apply(W, items.reshape(batch, blocks, F, m)).reshape(S, batch, blocks * m)
    assert np.array_equal(_f32bits(got), _f32bits(want))
    assert np.isnan(guard).all(), "the kernel wrote behind the batch"
    bad = np.isnan(got.view(np.float32).reshape(S, batch, blocks, m, 2)).any(axis=4)
    assert bad[:, 1, blocks // 2, m - 1].all() and bad.sum() == S, "the NaN sample poisoned %d outputs" % bad.sum()


@pytest.mark.parametrize("arithmetic", [False, True])
def test_combine_kernel_equals_the_restatement(arithmetic, gpu_device):
    """The combine alone on rows that hold zeros, infinities, NaNs, denormals and the largest float32: IEEE does the special cases.
    Every word of every item's row is written, nothing behind them."""
    import torch
    capi = _capi()
    m, k, F, S, batch, res = 4, 8, 4, 3, 5, 97
    rng = np.random.default_rng(11)
    P = np.exp(rng.uniform(-30, 30, (S, batch, res))).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4028235e38, -1.0], np.float32)
    for i, v in enumerate(special):
        P[i % S, i % batch, 3 + 5 * i] = v
        P[:, (i + 1) % batch, 50 + 5 * i] = v                    # (... and in every subband at once)
    table = (rng.standard_normal((res, m)) + 1j * rng.standard_normal((res, m))).astype(np.complex64)
    with capi.Context(m, 1, m * k, res, table) as ctx:
        ctx.set_subbands(F, [0, 1, 3], np.stack([table] * S), combine=int(arithmetic))
        d_p = torch.from_numpy(P).cuda()
        out = torch.full((batch * res + 64,), float("nan"), dtype=torch.float32, device="cuda")
        out[:batch * res] = 7.0
        torch.cuda.synchronize()
        ctx.debug_subband_combine(d_p.data_ptr(), batch, out.data_ptr())
        ctx.sync()
        o = out.cpu().numpy()
    got, want = o[:batch * res].reshape(batch, res), sr.combine(P, arithmetic=arithmetic)
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(got), nan)       # (IEEE leaves a NaN's sign and payload open: they are not compared)
    assert np.array_equal(_f32bits(got)[~nan], _f32bits(want)[~nan])
    assert np.isnan(o[batch * res:]).all(), "the kernel wrote behind the rows"


# ---- 2. the main pin -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("peak", [0, 1])
@pytest.mark.parametrize("m,k,F,occ", [(4, 64, 8, 0.75), (8, 48, 4, 1.0), (16, 32, 16, 0.75)])
def test_equals_plain_contexts_and_the_numpy_pipeline(m, k, F, occ, peak, gpu_device):
    capi = _capi()
    n, batch = 2, 9
    bins = sr.used_bins(F, occ)
    tabs, items = _tables(m, F, bins), _items(m, batch, k, seed=200 + m + F)
    y = sr.channelise_items(capi.subband_twiddles(F, bins), items, m)
    want = _reference(capi, m, n, k // F, tabs, y, peak)[0]
    with capi.Context(m, n, m * k, RES, _table(m)) as ctx:
        ctx.set_peak_mode(peak)
        ctx.set_subbands(F, bins, tabs)
        assert ctx.get_subbands() == (F, bins, capi.SUBBAND_HARMONIC)
        for port2 in (True, False):
            _same(_run_device(ctx, items, port2), want, "device path, port 2 %s" % port2)
            _same(ctx.process(items, want_spectrum=port2), want, "host-fed path, port 2 %s" % port2)
            got = _run_device(ctx, items, port2, want_lvl=False)
            assert got[1] is None
            _same(got, want, "device path, lvl not wired, port 2 %s" % port2)
            _same(ctx.process(items, want_lvl=False, want_spectrum=port2), want, "host-fed path, lvl not wired, port 2 %s" % port2)
        assert ctx.stage_name(capi.STAGE_SCAN) == ""
    assert np.count_nonzero(want[1]) == want[1].size


# ---- 3. the estimators with the arithmetic rule --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("m,k,F", [(4, 64, 8), (8, 48, 4)])
def test_estimators_with_the_arithmetic_rule(m, k, F, kind, gpu_device):
    capi = _capi()
    n, batch = 2, 7
    bins = sr.used_bins(F, 0.75)
    tabs, items = _tables(m, F, bins), _items(m, batch, k, seed=300 + m)
    y = sr.channelise_items(capi.subband_twiddles(F, bins), items, m)
    with capi.Context(m, n, m * k, RES, _table(m)) as ctx:
        ctx.set_subbands(F, bins, tabs, combine=capi.SUBBAND_ARITHMETIC)
        ctx.set_estimator(kind)                                       # (forwarded to every inner context)
        assert ctx.get_subbands()[2] == capi.SUBBAND_ARITHMETIC
        for peak in (0, 1):
            want = _reference(capi, m, n, k // F, tabs, y, peak, estimator=kind, arithmetic=True)[0]
            ctx.set_peak_mode(peak)
            _same(_run_device(ctx, items), want, "estimator %d, peak mode %d" % (kind, peak))
            _same(ctx.process(items, want_spectrum=False), want, "estimator %d, peak mode %d, host-fed" % (kind, peak))
    with capi.Context(m, n, m * k, RES, _table(m)) as ctx:
        ctx.set_estimator(kind)                                       # ... and in the other order
        ctx.set_peak_mode(1)
        ctx.set_subbands(F, bins, tabs, combine=capi.SUBBAND_ARITHMETIC)
        _same(_run_device(ctx, items), want, "estimator %d set first" % kind)


# ---- 4. covariance averaging ---------------------------------------------------------------------------------------------------------------

def test_averaging_is_forwarded(gpu_device):
    capi = _capi()
    m, n, k, F, batch = 8, 2, 64, 8, 6
    bins = sr.used_bins(F, 0.75)
    tabs, items = _tables(m, F, bins), _items(m, batch, k, seed=400)
    y = sr.channelise_items(capi.subband_twiddles(F, bins), items, m)
    want = _reference(capi, m, n, k // F, tabs, y, 1, averaging=4, calls=2)
    plain = _reference(capi, m, n, k // F, tabs, y, 1)[0]
    assert not np.array_equal(_f32bits(want[0][2]), _f32bits(plain[2]))
    for order in ("averaging first", "subbands first"):
        with capi.Context(m, n, m * k, RES, _table(m)) as ctx:
            ctx.set_peak_mode(1)
            if order == "averaging first":
                ctx.set_averaging(4)
            ctx.set_subbands(F, bins, tabs)
            if order == "subbands first":
                ctx.set_averaging(4)
            _same(_run_device(ctx, items), want[0], order + ", first call")
            _same(ctx.process(items), want[1], order + ", second call: the history carries on")
            ctx.reset_averaging()
            _same(_run_device(ctx, items), want[0], order + ", after the reset")
            ctx.set_averaging(1)
            _same(_run_device(ctx, items), plain, order + ", averaging off again")


# ---- 5. what the feature is for ----------------------------------------------------------------------------------------------------------------

def test_known_answer_on_the_device(gpu_device):
    capi = _capi()
    items, centre, bins, tabs, s = sr.scene(0)
    m, n, k, F = s["m"], s["n"], s["K"], s["F"]
    with capi.Context(m, n, m * k, RES, centre) as ctx:
        ctx.set_peak_mode(1)
        narrow = ctx.process(items)[0]
        ctx.set_subbands(F, bins, tabs)
        wide, lvl, _ = ctx.process(items)
    hits_n, hits_w = sr.exact_hits(narrow, s["angles"]), sr.exact_hits(wide, s["angles"])
    print("scene 0 on the device: narrowband %d / 16, subband %d / 16" % (hits_n, hits_w))
    assert hits_w == 16 and np.all(lvl > 0)
    assert hits_n <= 8


# ---- 6. chunking ---------------------------------------------------------------------------------------------------------------------------

def test_chunks_of_the_workspace_constant(gpu_device):
    capi = _capi()
    m, n, k, F = 8, 2, 2048, 2
    bins = [1, 0]
    batch = capi.SMOOTH_WORKSPACE_BYTES // (len(bins) * (k // F) * m * 8) + 5
    tabs = _tables(m, F, bins)
    base = _items(m, 32, k, seed=500)
    items = np.ascontiguousarray(base[np.arange(batch) % 32])
    items[1::2] = items[1::2][:, ::-1]                               # (every other item reversed in time and across antennas)
    with capi.Context(m, n, m * k, RES, _table(m)) as ctx:
        ctx.set_subbands(F, bins, tabs)
        y, guard = _channelise_device(ctx, items, len(bins))
        assert np.isnan(guard).all()
        dev = _run_device(ctx, items)
        host = ctx.process(items)
    y3 = sr.channelise_items(capi.subband_twiddles(F, bins), items[:3], m)
    assert np.array_equal(_f32bits(y[:, :3]), _f32bits(y3))
    want = _reference(capi, m, n, k // F, tabs, y, 0)[0]
    _same(dev, want, "device path")
    _same(host, want, "host-fed path")


# ---- 7. refusals, retunes ------------------------------------------------------------------------------------------------------------------

def test_refusals_in_both_orders(gpu_device):
    capi = _capi()
    m, n, k, F = 8, 2, 64, 8
    line = [[i, 0] for i in range(m)]
    table = mo.steering_table_c64(line, RES, mo.FREQUENCY, mo.SPACING)      # (a line array: smoothing applies)
    items = mo.synth_items(8, m, m * k, line, mo.FREQUENCY, mo.SPACING, seed=600)
    bins = sr.used_bins(F, 0.75)
    tabs = np.stack([mo.steering_table_c64(line, RES, mo.C_LIGHT / l, mo.SPACING)
                     for l in sr.wavelengths(mo.FREQUENCY, 0.4 * mo.FREQUENCY, F, bins)])
    T = capi.beamspace_design(table, 20, 60, 4)[0]

    def refused(call, code):
        with pytest.raises(capi.MusicError) as e:
            call()
        assert e.value.code == code, e.value

    others = [(lambda c: c.set_smoothing(6, True), lambda c: c.set_smoothing(m, False), lambda c: c.get_smoothing() == (6, True)),
              (lambda c: c.set_beamspace(T), lambda c: c.set_beamspace(None), lambda c: c.get_beamspace() is not None),
              (lambda c: c.set_calibration(np.full(m, 1 + 0.1j, np.complex64)), lambda c: c.set_calibration(None),
               lambda c: c.get_calibration() is not None),
              (lambda c: c.set_noise_covariance(np.diag(np.arange(1.0, m + 1))), lambda c: c.set_noise_covariance(None),
               lambda c: c.get_noise_covariance() is not None),
              (lambda c: c.set_order_mode("mdl"), lambda c: c.set_order_mode(None), lambda c: c.get_order_mode() == "mdl"),
              (lambda c: c.set_refine_mode(1), lambda c: c.set_refine_mode(0), lambda c: c.get_refine_mode() == 1),
              (lambda c: c.set_power_mode(1), lambda c: c.set_power_mode(0), lambda c: c.get_power_mode() == 1),
              (lambda c: c.set_beam_mode(1), lambda c: c.set_beam_mode(0), lambda c: c.get_beam_mode()[0] == 1)]
    with capi.Context(m, n, m * k, RES, table) as ctx:
        refused(lambda: ctx.set_subband_tables(tabs), capi.E_UNSUPPORTED)          # (while off)
        # the other setting first: set_subbands is refused and the setting in force stays
        for on, off, probe in others:
            on(ctx)
            before = ctx.process(items)
            refused(lambda: ctx.set_subbands(F, bins, tabs), capi.E_UNSUPPORTED)
            assert ctx.get_subbands() is None and probe(ctx)
            _same(ctx.process(items), before, "after the refused set_subbands")
            off(ctx)
        # subbands first: the others are refused and the setting stays
        ctx.set_subbands(F, bins, tabs)
        before = ctx.process(items)
        for on, off, probe in others:
            refused(lambda: on(ctx), capi.E_UNSUPPORTED)
            assert ctx.get_subbands() == (F, bins, 0) and not probe(ctx)
            off(ctx)                                                      # (another mode's "off" is not this mode's to end)
            assert ctx.get_subbands() == (F, bins, 0)
        # invalid settings: F, S, bins, tables, combine
        bad_nan = tabs.copy()
        bad_nan[2, 7, 1] = np.nan
        for call in (lambda: ctx.set_subbands(1, [0], tabs[:1]), lambda: ctx.set_subbands(65, [0], tabs[:1]),
                     lambda: ctx.set_subbands(7, [0], tabs[:1]),                           # (7 does not divide K = 64)
                     lambda: ctx.set_subbands(8, [0, 8], tabs[:2]), lambda: ctx.set_subbands(8, [3, 3], tabs[:2]),
                     lambda: ctx.set_subbands(64, list(range(33)), np.zeros((33, RES, m), np.complex64)),
                     lambda: ctx.set_subbands(F, bins, bad_nan), lambda: ctx.set_subbands(F, bins, tabs, combine=2),
                     lambda: ctx.set_subband_tables(bad_nan)):
            refused(call, capi.E_INVALID)
            assert ctx.get_subbands() == (F, bins, 0)
        _same(ctx.process(items), before, "after the refusals")
        for call in (lambda: ctx.profile(1), lambda: ctx.stage_ms(0)):
            refused(call, capi.E_UNSUPPORTED)
        assert ctx.refined_values() == capi.E_UNSUPPORTED
        # set_table while on replaces only the table "off" returns to
        second = (table * np.exp(1j * np.linspace(0, 0.3, m))[None, :]).astype(np.complex64)
        ctx.set_table(second)
        _same(ctx.process(items), before, "set_table while on")
        # set_subband_tables == a fresh set_subbands with those tables
        tabs2 = (tabs * np.exp(1j * np.linspace(0, 0.2, m))[None, None, :]).astype(np.complex64)
        ctx.set_subband_tables(tabs2)
        retuned = ctx.process(items)
        assert ctx.get_subbands() == (F, bins, 0)
        ctx.set_subbands(0)
        off_out = ctx.process(items)
    with capi.Context(m, n, m * k, RES, table) as fresh:
        fresh.set_subbands(F, bins, tabs2)
        _same(retuned, fresh.process(items), "set_subband_tables")
        assert not np.array_equal(_f32bits(retuned[2]), _f32bits(before[2]))
    with capi.Context(m, n, m * k, RES, second) as fresh:
        _same(off_out, fresh.process(items), "off after set_table while on")
    with capi.Context(32, n, 32 * k, RES, _table(32)) as wide:
        refused(lambda: wide.set_subbands(F, bins, np.zeros((len(bins), RES, 32), np.complex64)), capi.E_UNSUPPORTED)    # 17 .. 64 antennas
        assert wide.get_subbands() is None


def test_host_block_and_helper_surface(gpu_device):
    """The helper's set_subbands through the pybind module and the host block: the bins and tables it derives, on the device, equal a
    capi context set with the same; the setting follows set_frequency(); None returns to the plain block."""
    from gr_baz_amd import baz
    capi = _capi()
    m, n, k, F = 4, 2, 64, 8
    arr = mo.array_geometry(m)
    fs = sr.FS_OVER_FC * mo.FREQUENCY
    items = _items(m, 10, k, seed=900)
    hb = baz.music_doa_helper.music_doa_helper(m, n, m * k, RES, mo.FREQUENCY, mo.SPACING, arr, output_spectrum=True)
    assert hb.subbands() is None
    plain = hb.work(items)
    hb.set_subbands(fs, F)
    bins = sr.used_bins(F, 0.75)
    assert hb.subbands() == (F, 0, bins)
    for f in (mo.FREQUENCY, 0.8 * mo.FREQUENCY):
        if f != mo.FREQUENCY:
            hb.set_frequency(f)
            assert hb.subbands() == (F, 0, bins)
        with capi.Context(m, n, m * k, RES, mo.steering_table_c64(arr, RES, f, mo.SPACING)) as ctx:
            ctx.set_subbands(F, bins, sr.tables(m, f, fs, F, bins))
            _same(hb.work(items), ctx.process(items), "helper at %.3g Hz" % f)
    with pytest.raises(ValueError):
        hb.impl.set_subbands(7, [0], [hb.array_response], 0)            # (7 does not divide K: std::invalid_argument)
    with pytest.raises(ValueError):
        hb.impl.set_subbands(F, [0, 1], [hb.array_response], 0)         # (one table per bin)
    assert hb.subbands() == (F, 0, bins)
    hb.set_subbands(None, 0)
    assert hb.subbands() is None
    hb.set_frequency(mo.FREQUENCY)
    _same(hb.work(items), plain, "off again")


# ---- 8. off is the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [4, 8, 16])
def test_off_is_the_reference_bit_for_bit(m, gpu_device):
    """A context never set, one set to off and one switched on and off again: identical bits on every port, identical launch counts of
    every stage, and no allocation left behind."""
    capi = _capi()
    n, k, F = 2, 64, 8
    bins = sr.used_bins(F, 0.75)
    table, tabs, items = _table(m), _tables(m, F, bins), _items(m, 24, k, seed=700 + m)
    outs, launches, live = [], [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, m * k, RES, table) as ctx:
            if how == "set_off":
                ctx.set_subbands(0)
            if how == "on_then_off":
                ctx.set_subbands(F, bins, tabs)
                ctx.process(items)
                ctx.process(items, want_spectrum=False)
                ctx.set_subbands(None)
            assert ctx.get_subbands() is None
            ctx.profile(1)
            outs.append(ctx.process(items) + ctx.process(items, want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            live.append(capi.live_buffers())
    for o in outs[1:]:
        _same(o, outs[0], "off")
    assert launches[0] == launches[1] == launches[2], launches
    assert live[0] == live[1] == live[2], live


# ---- 9. no torn batch ----------------------------------------------------------------------------------------------------------------------

def test_setters_beside_a_submitting_thread_never_tear_a_batch(gpu_device):
    capi = _capi()
    m, n, k, F = 4, 2, 64, 4
    bins = [0, 1, 3]
    table, items = _table(m), _items(m, 16, k, seed=800)
    tabs1 = _tables(m, F, bins)
    tabs2 = (tabs1 * np.exp(1j * np.linspace(0, 0.4, m))[None, None, :]).astype(np.complex64)
    with capi.Context(m, n, m * k, RES, table) as ctx:
        known = []
        for tabs in (tabs1, tabs2):
            ctx.set_subbands(F, bins, tabs)
            known.append(tuple(_f32bits(x).tobytes() for x in ctx.process(items)))
        assert known[0] != known[1]
        stop = threading.Event()
        seen, errors = [0, 0], []

        def submit():
            try:
                while not stop.is_set() and sum(seen) < 200:
                    got = tuple(_f32bits(x).tobytes() for x in ctx.process(items))
                    if got not in known:
                        errors.append("a batch is neither setting's result")
                        return
                    seen[known.index(got)] += 1
            except Exception as e:          # noqa: BLE001 (reported by the asserting thread)
                errors.append(repr(e))

        t = threading.Thread(target=submit)
        t.start()
        try:
            i = 0
            while t.is_alive() and i < 60:
                if i % 4 < 2:
                    ctx.set_subband_tables(tabs1 if i % 2 else tabs2)
                else:
                    ctx.set_subbands(F, bins, tabs1 if i % 2 else tabs2)
                i += 1
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        assert sum(seen) > 0
        print("batches beside %d setter calls: %s" % (i, seen))
