"""Opt-in forward-backward averaging / spatial smoothing (baz_music_set_smoothing) on the MI355X: parity of every inner path
with the fp64 oracle of the re-stacked items, off == the reference bit for bit, the coherent-emitter property, set_table and
mode changes while on, host path == device path, and the host block / helper surface."""
import threading

import numpy as np
import pytest

import smoothing_ref as sr
from helpers import assert_doa_within_bound, assert_spectrum_within_bound, oracle_fp64
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _items(arr, K, batch, seed, snr_db=20.0):
    m = len(arr)
    return mo.synth_items(batch, m, m * K, arr, mo.FREQUENCY, mo.SPACING, snr_db=snr_db, seed=seed)


PARITY = [
    # name, array, subarray, forward-backward, n, K, res -- the inner context's path in the name
    ("fused_ula6_ss4", sr.ula(6), 4, False, 2, 256, 360),            # K' = 768: cov4_evd_kernel
    ("fused_square_fb", mo.array_geometry(4), 4, True, 1, 128, 360),  # K' = 256
    ("gated_i8_ula8_ss6", sr.ula(8), 6, False, 2, 64, 720),
    ("gated_i8_ula8_fb_ss6", sr.ula(8), 6, True, 3, 64, 720),
    ("i8_ula16_ss13", sr.ula(16), 13, False, 4, 32, 1000),
    ("wide_ula24_ss20", sr.ula(24), 20, False, 2, 32, 720),
    ("wide_circle32_fb", mo.array_geometry(32), 32, True, 1, 64, 720),
]


@pytest.mark.parametrize("name,arr,ms,fb,n,K,res", PARITY, ids=[p[0] for p in PARITY])
def test_parity_with_the_oracle_of_the_restacked_items(name, arr, ms, fb, n, K, res, gpu_device):
    capi = _capi()
    m = len(arr)
    table = sr.table_of(arr, res)
    items = _items(arr, K, 37, seed=len(name))                  # a ragged batch
    perm = capi.smoothing_check(m, res, table, ms, fb)
    assert perm is not None
    sub = table[:, :ms]
    a_ref, _, _, s64, w = oracle_fp64(sr.restack(items, m, ms, fb, perm), sub, ms, n)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_smoothing(ms, fb)
        assert ctx.get_smoothing() == (ms, bool(fb))
        if name.startswith("gated_i8") or name.startswith("i8"):
            assert ctx.uses_i8_scan()
        path = "int8" if ctx.uses_i8_scan() else "fp64"
        ang, lvl, spec = ctx.process(items)
        ang0, lvl0, _ = ctx.process(items, want_spectrum=False)
    assert_spectrum_within_bound(spec, s64, path, ms, n, sub, w, ill_posed_ok=True)
    assert_doa_within_bound(ang, lvl, a_ref, s64, path, ms, n, sub, w, ill_posed_ok=True)
    assert_doa_within_bound(ang0, lvl0, a_ref, s64, path, ms, n, sub, w, ill_posed_ok=True)


@pytest.mark.parametrize("cfg,batch", [("cfg1", 64), ("cfg3", 24)])
def test_off_is_the_reference_bit_for_bit(cfg, batch, gpu_device):
    capi = _capi()
    c = mo.make_config(cfg, batch, seed=91)
    m, n, N, res = c["m"], c["n"], c["nsamples"], c["res"]
    outs = []
    for how in ("fresh", "set_off", "on_then_off"):
        with capi.Context(m, n, N, res, c["table"]) as ctx:
            if how == "set_off":
                ctx.set_smoothing(m, False)
            if how == "on_then_off":
                ctx.set_smoothing(m, True)                     # the square and the even circle are centro-symmetric
                ctx.process(c["items"])
                ctx.set_smoothing(m, False)
            assert ctx.get_smoothing() == (m, False)
            outs.append(ctx.process(c["items"]) + ctx.process(c["items"], want_spectrum=False)[:2])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_coherent_emitters_and_peak_mode_on_the_device(gpu_device):
    """The CPU test's setup (tests/test_smoothing.py) with device outputs, peak mode on, spectrum port wired: the 4 strongest
    peaks of the device's spectrum find both coherent emitters at the CPU test's rates, and the peak-mode ang / lvl are
    oracle.music_oracle.peak_pick of the device's own spectrum."""
    capi = _capi()
    res, m, n = 720, 8, 2
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    rates = {}
    with capi.Context(m, n, m * 64, res, table) as ctx:
        ctx.set_peak_mode(1)
        for coherent in (True, False):
            items = sr.two_emitters(200, arr, 64, coherent=coherent, seed=2024)
            for name, ms, fb in (("plain", 8, False), ("fb", 8, True), ("ss6", 6, False), ("fb_ss6", 6, True)):
                ctx.set_smoothing(ms, fb)
                ang, lvl, spec = ctx.process(items)
                rates[(coherent, name)] = sr.success_rate(sr.picked(spec))
                for b in range(len(items)):
                    pa, pl = mo.peak_pick(spec[b], n, res)
                    assert np.array_equal(ang[b], pa) and np.array_equal(lvl[b], pl), (name, b)
    assert rates[(True, "plain")] < 0.5, rates
    assert rates[(True, "fb")] > 0.9 and rates[(True, "ss6")] > 0.95 and rates[(True, "fb_ss6")] > 0.95, rates
    assert all(rates[(False, k)] > 0.95 for k in ("plain", "fb", "ss6", "fb_ss6")), rates


def test_set_table_while_on(gpu_device):
    capi = _capi()
    res, m, n, ms = 720, 8, 2, 6
    arr = sr.ula(m)
    items = _items(arr, 64, 24, seed=5)
    with capi.Context(m, n, m * 64, res, sr.table_of(arr, res)) as ctx:
        ctx.set_smoothing(ms, True)
        t2 = sr.table_of(arr, res, freq=mo.FREQUENCY * 0.9)      # the ULA retuned stays a ULA
        ctx.set_table(t2)
        path = "int8" if ctx.uses_i8_scan() else "fp64"
        ang, lvl, spec = ctx.process(items)
        a_ref, _, _, s64, w = oracle_fp64(sr.restack(items, m, ms, True), t2[:, :ms], ms, n)
        assert_spectrum_within_bound(spec, s64, path, ms, n, t2[:, :ms], w, ill_posed_ok=True)
        assert_doa_within_bound(ang, lvl, a_ref, s64, path, ms, n, t2[:, :ms], w, ill_posed_ok=True)
        with pytest.raises(capi.MusicError) as e:
            ctx.set_table(sr.table_of(mo.array_geometry(8), res))  # a circle is not shift invariant
        assert e.value.code == capi.E_INVALID
        assert ctx.get_smoothing() == (ms, True)
        again = ctx.process(items)
        for a, b in zip((ang, lvl, spec), again):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("wired", [True, False])
def test_host_path_equals_device_path_across_chunks(wired, gpu_device):
    import torch
    capi = _capi()
    res, m, n, ms, K = 360, 8, 2, 6, 64
    arr = sr.ula(m)
    per_item = ms * (m - ms + 1) * K * 2 * 8
    B = capi.SMOOTH_WORKSPACE_BYTES // per_item + 180          # more than one chunk
    items = _items(arr, K, B, seed=11)
    with capi.Context(m, n, m * K, res, sr.table_of(arr, res)) as ctx:
        ctx.set_smoothing(ms, True)
        ctx.reserve(B)
        h_ang, h_lvl, h_spec = ctx.process(items, want_spectrum=wired)
        x = torch.from_numpy(items.view(np.float32)).to(gpu_device)
        ang = torch.zeros(B, n, dtype=torch.float32, device=gpu_device)
        lvl = torch.zeros_like(ang)
        spec = torch.zeros(B, res, dtype=torch.float32, device=gpu_device) if wired else None
        ctx.process_device(x.data_ptr(), B, ang.data_ptr(), lvl.data_ptr(), spec.data_ptr() if wired else None,
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert np.array_equal(ang.cpu().numpy(), h_ang) and np.array_equal(lvl.cpu().numpy(), h_lvl)
    if wired:
        assert np.array_equal(spec.cpu().numpy(), h_spec)


def test_mode_changes_from_a_second_thread_never_tear(gpu_device):
    """Modelled on tests/test_retune.py: thread B switches between FB + SS(6) and off while thread A runs batches; every
    batch equals one mode's outputs."""
    capi = _capi()
    res, m, n = 360, 8, 2
    arr = sr.ula(m)
    items = _items(arr, 64, 64, seed=13)
    with capi.Context(m, n, m * 64, res, sr.table_of(arr, res)) as ctx:
        off = ctx.process(items)
        ctx.set_smoothing(6, True)
        on = ctx.process(items)
        ctx.set_smoothing(m, False)
        assert not np.array_equal(on[2], off[2])
        stop, err = threading.Event(), []

        def switcher():
            try:
                k = 0
                while not stop.is_set() and k < 40:
                    ctx.set_smoothing(*((6, True) if k % 2 == 0 else (m, False)))
                    k += 1
            except Exception as e:   # noqa: BLE001
                err.append(e)

        th = threading.Thread(target=switcher)
        th.start()
        seen = set()
        try:
            for _ in range(40):
                got = ctx.process(items)
                match = [name for name, want in (("off", off), ("on", on)) if all(np.array_equal(a, b) for a, b in zip(got, want))]
                assert match, "a batch matched neither mode"
                seen.add(match[0])
        finally:
            stop.set()
            th.join()
        assert not err, err


def test_host_block_and_helper_surface(gpu_device):
    from gr_baz_amd import baz
    capi = _capi()
    res, m, n, K = 720, 8, 2, 64
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = _items(arr, K, 20, seed=17)
    with capi.Context(m, n, m * K, res, table) as ctx:
        ctx.set_smoothing(6, True)
        want = ctx.process(items)
    blk = baz.music_doa(m, n, m * K, [list(map(complex, r)) for r in table], res)
    blk.set_smoothing(6, True)
    produced, ang, lvl, spec = blk.work(items, 3)
    assert produced == len(items)
    for a, b in zip((ang, lvl, spec), want):
        assert np.array_equal(a, b)
    for bad in ((2, True), (9, False), (1, False)):               # n < subarray <= m
        with pytest.raises(ValueError):
            blk.set_smoothing(*bad)
    circ = baz.music_doa(7, 2, 7 * K, [list(map(complex, r)) for r in sr.table_of(mo.array_geometry(7), res)], res)
    with pytest.raises(ValueError):
        circ.set_smoothing(7, True)                               # an odd circle has no centro-symmetry

    h = baz.music_doa_helper.music_doa_helper(m, n, m * K, res, mo.FREQUENCY, mo.SPACING, arr, output_spectrum=True)
    h.set_smoothing(6, True)
    ht = np.asarray(h.array_response, dtype=np.complex64)
    with capi.Context(m, n, m * K, res, ht) as ctx:
        ctx.set_smoothing(6, True)
        want = ctx.process(items)
        for a, b in zip(h.work(items), want):
            assert np.array_equal(a, b)
        h.set_frequency(mo.FREQUENCY * 1.1)                      # the mode survives a retune
        ctx.set_table(np.asarray(h.array_response, dtype=np.complex64))
        for a, b in zip(h.work(items), ctx.process(items)):
            assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        h.set_smoothing(2)
