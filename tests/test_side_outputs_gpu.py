"""The per-call side outputs of the opt-in modes, all four modes on together (emitter count MDL, refinement, power mode 2, beam mode
with loading 1e-2, peak mode 1), seen through their accessors alone: last_orders, last_refine_offsets, last_powers,
last_beam_weights, last_beams and last_beams_device.

A characterisation of the bookkeeping, not of the numbers (those are held to their bounds by the modes' own tests): a host-fed call
cut into chunks reports what one device call over the same items reports, bit for bit and in call order; every reader returns
exactly min(count, what exists) units and leaves the rest of the caller's buffer alone; a following call with every mode off
reports its own size, n for every count and zeros elsewhere; switching the modes back on reproduces the first call; under
smoothing the counts are those of the outer call and the beams are zeros."""
import ctypes

import numpy as np
import pytest

import order_ref as oref
from oracle import music_oracle as mo

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
LOADING = 1e-2


def _capi():
    from gr_baz_amd import capi
    return capi


def _scene(B, m, K, seed):
    """Items of one and of two emitters, interleaved: the emitter-count mode reports both counts."""
    arr = oref.ula(m)
    one, _ = oref.scene(B, m, K, 1, 0.1, seed, arr=arr)
    two, _ = oref.scene(B, m, K, 2, 0.1, seed + 1, arr=arr)
    items = two.copy()
    items[::3] = one[::3]
    return items


def _modes_on(ctx):
    ctx.set_peak_mode(1)
    ctx.set_order_mode("mdl")
    ctx.set_refine_mode(1)
    ctx.set_power_mode(2)
    ctx.set_beam_mode(1, LOADING)


def _modes_off(ctx):
    ctx.set_order_mode(None)
    ctx.set_refine_mode(0)
    ctx.set_power_mode(0)
    ctx.set_beam_mode(0)


def _readers(ctx):
    """name -> (C entry, pointer type, bytes per unit of `count`, units per item)."""
    n, m, K = ctx.n, ctx.m, ctx.nsamples // ctx.m
    return {
        "orders": ("baz_music_last_orders", ctypes.c_uint8, 1, 1),
        "offsets": ("baz_music_last_refine_offsets", ctypes.c_double, 8, n),
        "powers": ("baz_music_last_powers", ctypes.c_double, 8, n),
        "weights": ("baz_music_last_beam_weights", ctypes.c_double, n * m * 16, 1),
        "beams": ("baz_music_last_beams", ctypes.c_float, n * K * 8, 1),
    }


def _read(ctx, name, count, room):
    """Calls the reader with `count` on a sentinel-filled buffer of `room` units: (return value, the buffer's bytes)."""
    entry, ctype, unit, _ = _readers(ctx)[name]
    buf = np.full(max(room * unit, 1), SENTINEL, np.uint8)
    r = getattr(_capi().lib(), entry)(ctx._h, ctypes.cast(buf.ctypes.data, ctypes.POINTER(ctype)), int(count))
    return r, buf


def _all(ctx, items):
    """Every side output of the last call, read with a count larger than what exists: name -> bytes of exactly what exists."""
    out = {}
    for name, (_, _, unit, per_item) in _readers(ctx).items():
        total = items * per_item
        r, buf = _read(ctx, name, total + 7, total + 7)
        assert r == total, "%s: %d units for a call of %d items" % (name, r, items)
        assert (buf[total * unit:] == SENTINEL).all(), "%s wrote past what exists" % name
        out[name] = buf[:total * unit].copy()
    return out


def _device_call(ctx, items):
    import torch
    B = len(items)
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).cuda()
    d_ang = torch.full((B, ctx.n), 7.0, dtype=torch.float32, device="cuda")
    d_lvl = torch.full((B, ctx.n), 7.0, dtype=torch.float32, device="cuda")
    d_spec = torch.full((B, ctx.res), 7.0, dtype=torch.float32, device="cuda")
    ctx.process_device(x.data_ptr(), B, d_ang.data_ptr(), d_lvl.data_ptr(), d_spec.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(np.uint32) for t in (d_ang, d_lvl, d_spec))


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s: %s differs" % (what, name)


# name, m, n, nsamples, res, items.  m = 4: the W = 4 group (23 items leave a wave's groups partly empty; 200 host-fed items are
# more than two chunks of 1 MiB); m = 6: the W = 8 group, with as many items as make more than two chunks of its smaller items.
CASES = [
    ("m4_23_items", 4, 2, 1024, 3600, 23),
    ("m4_200_items_chunked", 4, 2, 1024, 3600, 200),
    ("m6_W8_chunked", 6, 2, 384, 360, 485),
]


@pytest.mark.parametrize("name,m,n,N,res,B", CASES, ids=[c[0] for c in CASES])
def test_side_outputs_through_their_accessors(name, m, n, N, res, B, gpu_device, monkeypatch):
    capi = _capi()
    K = N // m
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items = _scene(B, m, K, seed=1300 + m)
    with capi.Context(m, n, N, res, table) as ctx:
        _modes_on(ctx)
        ports = _device_call(ctx, items)
        first = _all(ctx, B)
        orders = first["orders"]
        assert len(np.unique(orders)) > 1 and orders.max() <= n, "the scene should give more than one count"
        assert first["offsets"].view(np.float64).any() and (first["powers"].view(np.float64) > 0).any()
        assert first["weights"].view(np.float64).any() and first["beams"].view(np.float32).any()
        ptr, cnt = ctx.last_beams_device()
        assert ptr and cnt == B

        # every reader: fewer than, exactly and more than what exists
        for rname, (_, _, unit, per_item) in _readers(ctx).items():
            total = B * per_item
            for count in (0, 1, total - 1, total, total + 1, 3 * total):
                room = max(count, total) + 2
                r, buf = _read(ctx, rname, count, room)
                have = min(count, total)
                assert r == have, "%s count=%d: returned %d, %d exist" % (rname, count, r, total)
                assert np.array_equal(buf[:have * unit], first[rname][:have * unit]), "%s count=%d: other bytes" % (rname, count)
                assert (buf[have * unit:] == SENTINEL).all(), "%s count=%d: wrote behind the %d units it returned" % (rname, count, have)

        # a following call with every mode off, of another size
        B2 = 17
        _modes_off(ctx)
        _device_call(ctx, items[:B2])
        off = _all(ctx, B2)
        assert (off["orders"] == n).all()
        for rname in ("offsets", "powers", "weights", "beams"):
            assert not off[rname].any(), "%s after a call with the mode off" % rname
        assert ctx.last_beams_device() == (0, 0)

        # the modes back on: the first call again
        _modes_on(ctx)
        ports3 = _device_call(ctx, items)
        _assert_same(first, _all(ctx, B), "third call")
        for a, b in zip(ports, ports3):
            assert np.array_equal(a, b)

    # the same items host-fed and cut into chunks: the same bytes in call order
    monkeypatch.setenv("BAZ_MUSIC_CHUNK_MIB", "1")
    chunk = max(64, (1 << 20) // (N * 8 + res * 4 + n * 8))
    if B >= 200:
        assert B > 2 * chunk                                                   # (more than two chunks)
    with capi.Context(m, n, N, res, table) as ctx:
        _modes_on(ctx)
        out = ctx.process(items)
        _assert_same(first, _all(ctx, B), "chunked host-fed call")
        for a, b in zip(ports, out):
            assert np.array_equal(a, np.ascontiguousarray(b).view(np.uint32))
        ptr, cnt = ctx.last_beams_device()
        assert ptr and cnt == B


def test_side_outputs_under_smoothing(gpu_device):
    """Subarrays of 3 with forward-backward averaging on the m = 4 shape (the beam mode is refused there): counts, offsets and powers
    come back with the outer call's counts, last_beams / last_beam_weights give zeros for that many items."""
    capi = _capi()
    m, n, N, res, B = 4, 2, 1024, 3600, 23
    table = mo.steering_table_c64(oref.ula(m), res, mo.FREQUENCY, mo.SPACING)
    items = _scene(B, m, N // m, seed=1304)
    with capi.Context(m, n, N, res, table) as ctx:
        ctx.set_peak_mode(1)
        ctx.set_order_mode("mdl")
        ctx.set_refine_mode(1)
        ctx.set_power_mode(2)
        ctx.set_smoothing(3, True)
        with pytest.raises(capi.MusicError) as e:
            ctx.set_beam_mode(1, LOADING)
        assert e.value.code == capi.E_UNSUPPORTED
        ctx.process(items)
        got = _all(ctx, B)
        assert got["orders"].max() <= n and got["orders"].any()
        assert (got["powers"].view(np.float64) > 0).any() and got["offsets"].view(np.float64).any()
        assert not got["weights"].any() and not got["beams"].any()
        assert ctx.last_beams_device() == (0, 0)
        # a second, shorter call: the readers follow it
        ctx.process(items[:5])
        _all(ctx, 5)
