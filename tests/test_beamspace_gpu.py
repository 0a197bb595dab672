"""The opt-in beamspace mode (baz_music_set_beamspace) on the MI355X: the projection kernel against the host routine bit
for bit; a context with T set against a plain B-antenna context on the projected table and items, bit for bit on every port; the
inner context's table images; the opt-in modes at 17 .. 64 antennas, which the plain path refuses; chunking; refusals; off == the
context never set; a setter beside a submitting thread."""
import threading

import numpy as np
import pytest

import beamspace_ref as br
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

RES, K = 360, 64


def _capi():
    from gr_baz_amd import capi
    return capi


def _f32bits(x):
    return np.ascontiguousarray(x).view(np.float32).view(np.uint32)


def _items(m, batch, seed, k=K, angles=(40.0, 62.0)):
    return mo.synth_items(batch, m, m * k, mo.array_geometry(m), mo.FREQUENCY, mo.SPACING, angles_deg=angles, snr_db=20.0, seed=seed)


def _design(capi, m, B, lo=20, cnt=60):
    return capi.beamspace_design(br.table_of(m), lo, cnt, B)[0]


def _run_device(ctx, items, want_spectrum=True):
    """One process_device call into buffers pre-filled with NaN: (ang, lvl, spectrum | None)."""
    import torch
    nb = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    d_ang = torch.full((nb, ctx.n), float("nan"), dtype=torch.float32, device="cuda")
    d_lvl = torch.full((nb, ctx.n), float("nan"), dtype=torch.float32, device="cuda")
    d_spec = torch.full((nb, ctx.res), float("nan"), dtype=torch.float32, device="cuda") if want_spectrum else None
    ctx.process_device(x.data_ptr(), nb, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr() if want_spectrum else None,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ang.cpu().numpy(), d_lvl.cpu().numpy(), d_spec.cpu().numpy() if want_spectrum else None


def _same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        if u is None and v is None:
            continue
        assert np.array_equal(_f32bits(u), _f32bits(v)), "%s: port %d differs" % (what, k)


def _project_device(ctx, items, B):
    """debug_beamspace on items (batch, m K) -> (batch, K B) complex64, and the guard row behind the output."""
    import torch
    nb = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    cols = items.shape[1] // ctx.m
    out = torch.full((nb * cols * B * 2 + 2 * B,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.debug_beamspace(x.data_ptr(), nb, out.data_ptr())
    ctx.sync()
    o = out.cpu().numpy()
    return o[:nb * cols * B * 2].view(np.complex64).reshape(nb, cols * B), o[nb * cols * B * 2:]


# ---- 1. the projection, bit for bit --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,B,k,batch", [(3, 2, 5, 3), (17, 5, 37, 3), (33, 16, 64, 2), (64, 16, 37, 3), (16, 8, 64, 4)])
def test_projection_equals_the_host_routine(m, B, k, batch, gpu_device):
    capi = _capi()
    rng = np.random.default_rng(m * 100 + B)
    T = (rng.standard_normal((m, B)) + 1j * rng.standard_normal((m, B))) / np.sqrt(m)
    items = (rng.standard_normal((batch, m * k)) + 1j * rng.standard_normal((batch, m * k))).astype(np.complex64)
    items[1, (k // 2) * m + 1] = np.nan                      # one sample of item 1
    table = (rng.standard_normal((RES, m)) + 1j * rng.standard_normal((RES, m))).astype(np.complex64)
    with capi.Context(m, 1, m * k, RES, table) as ctx:
        with pytest.raises(capi.MusicError):
            ctx.debug_beamspace(1, 1, 2)                     # (refused before anything is touched: the mode is off)
        ctx.set_beamspace(T)
        got, guard = _project_device(ctx, items, B)
    want = capi.beamspace_apply(T, items.reshape(batch, k, m)).reshape(batch, k * B)
    assert np.array_equal(_f32bits(got), _f32bits(want))
    assert np.isnan(guard).all(), "the kernel wrote behind the batch"
    bad = np.isnan(got.view(np.float32)).reshape(batch, k, 2 * B).any(axis=2)
    assert bad[1, k // 2] and bad.sum() == 1, "the NaN sample poisoned %d columns" % bad.sum()


# ---- 2. the main pin ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,B", [(17, 3), (33, 4), (17, 5), (64, 8), (33, 16), (16, 8)])
def test_equals_the_plain_context_on_projected_data(m, B, gpu_device):
    capi = _capi()
    n = 2
    table, items = br.table_of(m), _items(m, 8, seed=200 + m + B)
    T = _design(capi, m, B)
    tab_p = capi.beamspace_apply(T, table)
    y = capi.beamspace_apply(T, items.reshape(8, K, m)).reshape(8, K * B)
    kernels = set()
    with capi.Context(m, n, m * K, RES, table) as ctx, capi.Context(B, n, B * K, RES, tab_p) as plain:
        ctx.set_beamspace(T)
        got_T, nrm = ctx.get_beamspace()
        assert np.array_equal(got_T, T) and nrm is False
        for port2 in (True, False):
            want = _run_device(plain, y, port2)
            kernels.add(plain.stage_name(capi.STAGE_SCAN))
            _same(_run_device(ctx, items, port2), want, "device path, port 2 %s" % port2)
            host = ctx.process(items, want_spectrum=port2)
            _same(host, want, "host-fed path, port 2 %s" % port2)
            assert ctx.stage_name(capi.STAGE_SCAN) == ""
        assert ctx.uses_i8_scan() == plain.uses_i8_scan()
    kernels = " ".join(sorted(kernels))
    if B <= 5:
        assert "scan_mfma_kernel" in kernels and "scan_coarse_kernel" in kernels, kernels      # (m <= 4 / fp64, and the f16-gated scan)
    elif B == 8:
        assert "scan_i8_kernel" in kernels and "scan_coarse_kernel" in kernels, kernels
    else:
        assert "scan_i8_kernel" in kernels, kernels


# ---- 3. the table on the device ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,B", [(33, 8), (17, 16), (24, 4)])
def test_inner_table_images(m, B, gpu_device):
    capi = _capi()
    n = 2
    table = br.table_of(m)
    rng = np.random.default_rng(5)
    second = (table * np.exp(1j * rng.uniform(0, 0.3, (1, m)))).astype(np.complex64)
    T = _design(capi, m, B)

    def check(ctx, tab, normalise, what):
        proj = capi.beamspace_apply(T, tab, normalise=normalise)
        seen = 0
        for which in capi.TABLE_IMAGES:
            want = capi.debug_host_table_image(B, n, RES, proj, which)
            got = ctx.debug_table_image(which + 256)
            assert (want is None) == (got is None), (what, which)
            if want is not None:
                seen += 1
                assert np.array_equal(got, want), "%s: image %d (%s) differs" % (what, which, capi.TABLE_IMAGES[which])
        assert seen >= 2

    with capi.Context(m, n, m * K, RES, table) as ctx:
        assert ctx.debug_table_image(256) is None
        ctx.set_beamspace(T)
        check(ctx, table, False, "set_beamspace")
        ctx.set_table(second)
        check(ctx, second, False, "set_table with T in force")
        assert np.array_equal(ctx.get_beamspace()[0], T)
        ctx.set_beamspace(T, normalise=True)
        check(ctx, second, True, "normalise")
        assert ctx.get_beamspace()[1] is True


# ---- 4. what the feature is for ----------------------------------------------------------------------------------------------------

MODES = [("peak", lambda c: c.set_peak_mode(1)), ("order", lambda c: c.set_order_mode("mdl")), ("refine", lambda c: c.set_refine_mode(1)),
         ("power", lambda c: c.set_power_mode(2)), ("capon", lambda c: c.set_estimator(1))]


@pytest.mark.parametrize("name,setter", MODES, ids=[m[0] for m in MODES])
def test_modes_open_at_32_antennas(name, setter, gpu_device):
    capi = _capi()
    m, B, n = 32, 16, 2
    table, items = br.table_of(m), _items(m, 8, seed=400)
    T = _design(capi, m, B)
    tab_p = capi.beamspace_apply(T, table)
    y = capi.beamspace_apply(T, items.reshape(8, K, m)).reshape(8, K * B)
    with capi.Context(m, n, m * K, RES, table) as ctx, capi.Context(B, n, B * K, RES, tab_p) as plain:
        with pytest.raises(capi.MusicError) as e:
            setter(ctx)                                          # today's behaviour at 17 .. 64 antennas
        assert e.value.code == capi.E_UNSUPPORTED
        ctx.set_beamspace(T)
        setter(ctx)
        setter(plain)
        if name == "refine":
            ctx.set_peak_mode(1)
            plain.set_peak_mode(1)
        for port2 in (True, False):
            want = _run_device(plain, y, port2)
            _same(_run_device(ctx, items, port2), want, "%s, port 2 %s" % (name, port2))
            assert np.array_equal(ctx.last_orders(8), plain.last_orders(8))
            assert np.array_equal(ctx.last_refine_offsets(16).view(np.uint64), plain.last_refine_offsets(16).view(np.uint64))
            assert np.array_equal(ctx.last_powers(16).view(np.uint64), plain.last_powers(16).view(np.uint64))
        if name == "power":
            assert np.count_nonzero(ctx.last_powers(16)) == 16
        if name == "refine":
            assert np.count_nonzero(ctx.last_refine_offsets(16)) > 0
        # switching the front-end off on a wide context takes the modes the run-time-m kernels do not have with it
        ctx.set_beamspace(None)
        assert ctx.get_beamspace() is None
        out = _run_device(ctx, items)
    with capi.Context(m, n, m * K, RES, table) as fresh:
        _same(out, _run_device(fresh, items), "off again")


@pytest.mark.parametrize("k", [0, 4])
def test_known_answer_on_the_device(k, gpu_device):
    capi = _capi()
    table, items, s = br.scene(k)
    m, B, n = s["m"], s["B"], 2
    with capi.Context(m, n, m * K, RES, table) as ctx:
        captured = None
        T, captured = capi.beamspace_design(table, s["lo"], s["cnt"], B)
        ctx.set_beamspace(T)
        ctx.set_peak_mode(1)
        ang, lvl, _ = ctx.process(items)
        err = br.bin_errors(ang, s["angles"])
        print("scene %d on the device: captured %.5f, bin errors %s" % (k, captured, err.tolist()))
        assert np.all(lvl > 0) and np.all(err <= 1.0)
        ctx.set_order_mode("mdl")
        ctx.process(items)
        orders = ctx.last_orders(len(items))
    ref = br.mdl_orders(capi.beamspace_apply(T, items.reshape(len(items), K, m)), B, n)
    print("   MDL: 2 emitters in %d items on the device, %d by numpy" % (np.count_nonzero(orders == 2), np.count_nonzero(ref == 2)))
    assert np.count_nonzero(orders == 2) >= np.count_nonzero(ref == 2)


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------

def test_chunks_of_the_workspace_constant(gpu_device):
    capi = _capi()
    m, B, n, kk = 17, 16, 2, 1024
    batch = capi.SMOOTH_WORKSPACE_BYTES // (kk * B * 8) + 7
    table = br.table_of(m)
    base = _items(m, 32, seed=500, k=kk)
    items = np.ascontiguousarray(base[np.arange(batch) % 32])
    items[1::2] = items[1::2][:, ::-1]                               # (every other item reversed in time... and across antennas)
    T = _design(capi, m, B, 20, 90)
    with capi.Context(m, n, m * kk, RES, table) as ctx:
        ctx.set_beamspace(T)
        y, _ = _project_device(ctx, items, B)
        dev = _run_device(ctx, items)
        host = ctx.process(items)
    with capi.Context(B, n, B * kk, RES, capi.beamspace_apply(T, table)) as plain:
        want = _run_device(plain, y)
    y32 = capi.beamspace_apply(T, items[:3].reshape(3, kk, m)).reshape(3, kk * B)
    assert np.array_equal(_f32bits(y[:3]), _f32bits(y32))
    _same(dev, want, "device path")
    _same(host, want, "host-fed path")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_in_both_orders(gpu_device):
    capi = _capi()
    m, n = 8, 2
    table = mo.steering_table_c64([[i, 0] for i in range(m)], RES, mo.FREQUENCY, mo.SPACING)      # (a line array: smoothing applies)
    items = mo.synth_items(8, m, m * K, [[i, 0] for i in range(m)], mo.FREQUENCY, mo.SPACING, seed=600)
    T = capi.beamspace_design(table, 20, 60, 4)[0]

    def refused(call, code):
        with pytest.raises(capi.MusicError) as e:
            call()
        assert e.value.code == code, e.value

    with capi.Context(m, n, m * K, RES, table) as ctx:
        # the other setting first: set_beamspace is refused and the setting in force stays
        for on, off, probe in [(lambda: ctx.set_smoothing(6, True), lambda: ctx.set_smoothing(m, False), lambda: ctx.get_smoothing() == (6, True)),
                               (lambda: ctx.set_calibration(np.full(m, 1 + 0.1j, np.complex64)), lambda: ctx.set_calibration(None),
                                lambda: ctx.get_calibration() is not None),
                               (lambda: ctx.set_noise_covariance(np.diag(np.arange(1.0, m + 1))), lambda: ctx.set_noise_covariance(None),
                                lambda: ctx.get_noise_covariance() is not None),
                               (lambda: ctx.set_beam_mode(1), lambda: ctx.set_beam_mode(0), lambda: ctx.get_beam_mode()[0] == 1)]:
            on()
            before = ctx.process(items)
            refused(lambda: ctx.set_beamspace(T), capi.E_UNSUPPORTED)
            assert ctx.get_beamspace() is None and probe()
            _same(ctx.process(items), before, "after the refused set_beamspace")
            off()
        # beamspace first: the others are refused and T stays
        ctx.set_beamspace(T)
        before = ctx.process(items)
        for call in (lambda: ctx.set_smoothing(6, True), lambda: ctx.set_calibration(np.full(m, 1 + 0.1j, np.complex64)),
                     lambda: ctx.set_noise_covariance(np.diag(np.arange(1.0, m + 1))), lambda: ctx.set_beam_mode(1)):
            refused(call, capi.E_UNSUPPORTED)
            assert np.array_equal(ctx.get_beamspace()[0], T)
        ctx.set_smoothing(m, False)                                   # (smoothing's "off" is not this mode's to end)
        assert ctx.get_smoothing() == (m, False) and ctx.get_beamspace() is not None
        # invalid T: B <= n, B > m, a NaN, an all-zero column
        bad_nan, bad_zero = T.copy(), T.copy()
        bad_nan[3, 1] = np.nan
        bad_zero[:, 2] = 0
        for bad in (T[:, :2], np.zeros((m, 9), np.complex128) + 1, bad_nan, bad_zero):
            refused(lambda: ctx.set_beamspace(bad), capi.E_INVALID)
            assert np.array_equal(ctx.get_beamspace()[0], T)
        _same(ctx.process(items), before, "after the refusals")
    m = 32
    table = br.table_of(m)
    with capi.Context(m, n, m * K, RES, table) as ctx:
        rng = np.random.default_rng(1)
        refused(lambda: ctx.set_beamspace(rng.standard_normal((m, 17)) + 0j), capi.E_INVALID)       # B > 16
        assert ctx.get_beamspace() is None
        for call in (lambda: ctx.profile(1), lambda: ctx.stage_ms(0)):
            call()
        ctx.set_beamspace(_design(capi, m, 8))
        refused(lambda: ctx.profile(1), capi.E_UNSUPPORTED)
        refused(lambda: ctx.stage_ms(0), capi.E_UNSUPPORTED)
        assert ctx.refined_values() == capi.E_UNSUPPORTED


# ---- 7. off is the reference -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,B", [(4, 3), (8, 4), (32, 8)])
def test_off_is_the_reference_bit_for_bit(m, B, gpu_device):
    """A context never set, one set to off and one switched on and off again: identical bits on every port, identical launch counts of
    every stage, and no allocation left behind."""
    capi = _capi()
    n = 2
    table, items = br.table_of(m), _items(m, 24, seed=700 + m)
    T = _design(capi, m, B)
    outs, launches, live = [], [], []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, m * K, RES, table) as ctx:
            if how == "set_off":
                ctx.set_beamspace(None)
            if how == "on_then_off":
                ctx.set_beamspace(T)
                ctx.process(items)
                ctx.process(items, want_spectrum=False)
                ctx.set_beamspace(None)
            assert ctx.get_beamspace() is None
            ctx.profile(1)
            outs.append(ctx.process(items) + ctx.process(items, want_spectrum=False)[:2])
            launches.append([ctx.stage_ms(s)[1] for s in range(capi.NUM_STAGES)])
            live.append(capi.live_buffers())
    for o in outs[1:]:
        _same(o, outs[0], "off")
    assert launches[0] == launches[1] == launches[2], launches
    assert live[0] == live[1] == live[2], live


# ---- 8. no torn batch ------------------------------------------------------------------------------------------------------------------

def test_set_beamspace_beside_a_submitting_thread_never_tears_a_batch(gpu_device):
    capi = _capi()
    m, B, n = 24, 8, 2
    table, items = br.table_of(m), _items(m, 16, seed=800)
    T1, T2 = _design(capi, m, B, 20, 60), _design(capi, m, B, 10, 90)
    with capi.Context(m, n, m * K, RES, table) as ctx:
        known = []
        for T in (T1, T2):
            ctx.set_beamspace(T)
            known.append(tuple(_f32bits(x).tobytes() for x in ctx.process(items)))
        assert known[0] != known[1]
        stop = threading.Event()
        seen, errors = [0, 0], []

        def submit():
            try:
                while not stop.is_set() and sum(seen) < 400:
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
            while t.is_alive() and i < 400:
                ctx.set_beamspace(T1 if i % 2 else T2)
                i += 1
        finally:
            stop.set()
            t.join()
        assert not errors, errors
        assert sum(seen) > 0
        print("batches beside %d set_beamspace calls: %s" % (i, seen))
