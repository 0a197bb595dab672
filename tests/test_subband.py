"""The host side of the opt-in wideband (subband) mode (include/baz_music_hip.h): the twiddles against an extended-precision
restatement, baz_music_subband_apply against the header's chain word for word, argument validation, the helper's bin selection and
wavelengths, and the wideband known-answer scenes (the library's channeliser, the numpy oracle per subband, the combine, the peak
picker).  No device is needed."""
import ctypes

import numpy as np
import pytest

import subband_ref as sr
from gr_baz_amd import capi
from oracle import music_oracle as mo


def _f32bits(x):
    return np.ascontiguousarray(x).view(np.float32).view(np.uint32)


# ---- twiddles ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [2, 3, 8, 12, 64])
def test_twiddles(F):
    """Every component within 2 ulp of exp(-2 pi i ((k t) mod F) / F) / sqrt(F) evaluated in extended precision, and exactly 0 or
    +-fl64(1 / sqrt(F)) where (k t) mod F is a multiple of F / 4."""
    bins = list(range(F))[:capi.MAX_SUBBANDS]
    if F == 64:
        bins = list(range(0, 64, 2))[:16] + list(range(33, 64, 2))
    W = capi.subband_twiddles(F, bins)
    assert W.shape == (len(bins), F) and W.dtype == np.complex128
    ref = sr.twiddles(F, bins)
    got2, ref2 = W.view(np.float64), ref.view(np.float64)
    ulp = np.spacing(np.abs(ref2))
    assert np.all(np.abs(got2 - ref2) <= 2 * ulp), (np.abs(got2 - ref2) / ulp).max()
    unit = float(np.longdouble(1) / np.sqrt(np.longdouble(F)))
    quarter = 0
    for s, k in enumerate(bins):
        for t in range(F):
            j = (k * t) % F
            if (4 * j) % F == 0:
                want = [(unit, 0.0), (0.0, -unit), (-unit, 0.0), (0.0, unit)][4 * j // F]
                assert (W[s, t].real, W[s, t].imag) == want, (F, k, t)
                quarter += 1
    assert quarter >= len(bins)                     # (t = 0 of every subband at the least)
    # one subband is a row of the unitary DFT matrix: unit norm
    assert np.allclose(np.sum(np.abs(W) ** 2, axis=1), 1.0, rtol=0, atol=1e-14)


# ---- the channeliser ----------------------------------------------------------------------------------------------------------------------

def _bins_for(rng, F, S):
    return sorted(rng.choice(F, S, replace=False).tolist(), key=lambda k: (k * 7) % F + k / 100.0)     # (distinct, not ascending)


@pytest.mark.parametrize("m,F,S,blocks", [(2, 2, 1, 1), (3, 3, 3, 5), (4, 8, 7, 16), (16, 64, 32, 2), (7, 16, 13, 9)])
def test_apply_equals_the_definition_word_for_word(m, F, S, blocks):
    rng = np.random.default_rng(1000 * m + F)
    bins = _bins_for(rng, F, S)
    W = capi.subband_twiddles(F, bins)
    x = (rng.standard_normal((blocks, F, m)) + 1j * rng.standard_normal((blocks, F, m))).astype(np.complex64)
    got = capi.subband_apply(W, x)
    assert got.shape == (S, blocks, m) and got.dtype == np.complex64
    assert np.array_equal(_f32bits(got), _f32bits(sr.channelise(W, x)))
    # ... which is the unitary DFT of every block, to float32 rounding
    dft = np.fft.fft(x.astype(np.complex128), axis=1)[:, bins, :].transpose(1, 0, 2) / np.sqrt(F)
    assert np.abs(got - dft).max() <= 4 * 2.0 ** -24 * np.abs(dft).max()
    # a NaN sample turns exactly the S outputs of its own (block, antenna) to NaN
    b0, t0, r0 = blocks // 2, F - 1, m - 1
    x[b0, t0, r0] = np.nan
    bad = capi.subband_apply(W, x)
    nan = np.isnan(bad.view(np.float32).reshape(S, blocks, m, 2)).any(axis=3)
    assert nan[:, b0, r0].all() and nan.sum() == S
    keep = ~nan
    assert np.array_equal(_f32bits(bad)[np.repeat(keep[..., None], 2, axis=3).reshape(S, blocks, 2 * m)],
                          _f32bits(got)[np.repeat(keep[..., None], 2, axis=3).reshape(S, blocks, 2 * m)])


def test_apply_takes_any_w():
    """The routine is defined on the W it is given (a block window is a change of W): W = one 1 per row copies samples."""
    m, F = 3, 4
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((5, F, m)) + 1j * rng.standard_normal((5, F, m))).astype(np.complex64)
    W = np.zeros((2, F), np.complex128)
    W[0, 1], W[1, 3] = 1.0, -1j
    got = capi.subband_apply(W, x)
    assert np.array_equal(_f32bits(got[0]), _f32bits(x[:, 1, :]))
    assert np.array_equal(got[1], (-1j * x[:, 3, :].astype(np.complex128)).astype(np.complex64))


# ---- validity -----------------------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    L = capi.lib()
    u32p, f64p, f32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)

    def bins(*k):
        return (ctypes.c_uint32 * len(k))(*k)

    W = np.zeros((33, 64), np.complex128)
    wp = W.view(np.float64).ctypes.data_as(f64p)
    assert L.baz_music_subband_twiddles(8, 3, bins(0, 1, 7), wp) == capi.OK
    assert L.baz_music_subband_twiddles(64, 32, bins(*range(32)), wp) == capi.OK
    for args in [(1, 1, bins(0), wp), (65, 1, bins(0), wp), (0, 1, bins(0), wp),                 # F out of range
                 (8, 0, bins(0), wp), (64, 33, bins(*range(33)), wp),                           # S out of range
                 (8, 2, bins(0, 8), wp), (8, 3, bins(1, 2, 1), wp),                             # a bin at F, a repeated bin
                 (8, 1, None, wp), (8, 1, bins(0), None)]:
        assert L.baz_music_subband_twiddles(*args) == capi.E_INVALID, args[:2]
    x = np.zeros((3, 8, 4), np.complex64)
    out = np.zeros((2, 3, 4), np.complex64)
    xp, op = x.view(np.float32).ctypes.data_as(f32p), out.view(np.float32).ctypes.data_as(f32p)
    assert L.baz_music_subband_apply(4, 8, 2, wp, xp, 3, op) == capi.OK
    assert L.baz_music_subband_apply(4, 8, 2, wp, None, 0, None) == capi.OK
    for args in [(1, 8, 2, wp, xp, 3, op), (17, 8, 2, wp, xp, 3, op), (4, 1, 2, wp, xp, 3, op), (4, 65, 2, wp, xp, 3, op),
                 (4, 8, 0, wp, xp, 3, op), (4, 8, 33, wp, xp, 3, op), (4, 8, 2, None, xp, 3, op), (4, 8, 2, wp, None, 3, op),
                 (4, 8, 2, wp, xp, 3, None)]:
        assert L.baz_music_subband_apply(*args) == capi.E_INVALID, args[:3]
    # ... and through capi
    for call in (lambda: capi.subband_twiddles(8, [0, 8]), lambda: capi.subband_twiddles(8, [1, 1]), lambda: capi.subband_twiddles(1, [0]),
                 lambda: capi.subband_twiddles(65, [0]), lambda: capi.subband_twiddles(8, []), lambda: capi.subband_twiddles(64, range(33)),
                 lambda: capi.subband_twiddles(8, [-1]),
                 lambda: capi.subband_apply(np.zeros((2, 8)), np.zeros((3, 7, 4))),              # F of x is not W's
                 lambda: capi.subband_apply(np.zeros(8), np.zeros((3, 8, 4))),
                 lambda: capi.subband_apply(np.zeros((2, 8)), np.zeros((3, 8, 17))),             # m > 16
                 lambda: capi.subband_apply(np.zeros((33, 8)), np.zeros((3, 8, 4)))):
        with pytest.raises(ValueError):
            call()


def test_symbols_are_listed():
    for s in ("set_subbands", "set_subband_tables", "get_subbands", "debug_subbands", "debug_subband_combine", "subband_twiddles", "subband_apply"):
        assert "baz_music_" + s in capi.SYMBOLS
    assert capi.MAX_SUBBANDS == 32 and (capi.SUBBAND_HARMONIC, capi.SUBBAND_ARITHMETIC) == (0, 1)


# ---- the combine rules ----------------------------------------------------------------------------------------------------------------------

def test_combine_restatement_special_values():
    """IEEE does the special cases: a zero in a subband makes the harmonic mean 0, an infinity drops out of it, a NaN stays a NaN."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    P = np.array([[1.0, 0.0, inf, nan, 2.0], [3.0, 5.0, 4.0, 1.0, 2.0]], np.float32)
    h = sr.combine(P)
    assert h[0] == np.float32(2 / (1 + 1 / 3)) and h[1] == 0.0 and h[2] == np.float32(8.0) and np.isnan(h[3]) and h[4] == 2.0
    a = sr.combine(P, arithmetic=True)
    assert a[0] == 2.0 and a[1] == 2.5 and a[2] == inf and np.isnan(a[3]) and a[4] == 2.0


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------

def test_helper_bins_and_wavelengths():
    from gr_baz_amd.baz import music_doa_helper as helper
    for F, occ, want in [(8, 0.75, [0, 1, 2, 3, 5, 6, 7]), (16, 0.75, [0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15]), (8, 1.0, list(range(8))),
                         (7, 0.5, [0, 1, 6]), (2, 0.75, [0]), (5, 0.9, [0, 1, 2, 3, 4])]:
        assert helper.subband_bins(F, occ) == want == sr.used_bins(F, occ), (F, occ)
    assert [helper.subband_offset(k, 8) for k in range(8)] == [0, 1, 2, 3, -4, -3, -2, -1]
    assert [helper.subband_offset(k, 5) for k in range(5)] == [0, 1, 2, -2, -1]
    fc, fs, F = mo.FREQUENCY, 0.4 * mo.FREQUENCY, 8
    bins = helper.subband_bins(F, 0.75)
    ls = helper.subband_wavelengths(fc, fs, F, bins)
    assert ls == sr.wavelengths(fc, fs, F, bins)
    assert ls[0] == mo.C_LIGHT / fc and ls[3] == mo.C_LIGHT / (fc + 3 * fs / 8) and ls[4] == mo.C_LIGHT / (fc - 3 * fs / 8)
    with pytest.raises(ValueError):
        helper.subband_bins(8, 0.0 - 0.1)
    with pytest.raises(ValueError):
        helper.subband_bins(1, 0.75)


class _Impl(object):
    """A recorder in the place of the wrapped block."""

    def __init__(self, *args):
        self.args, self.calls = args, []

    def set_array_response(self, table):
        self.calls.append(("set_array_response", table))

    def set_estimator(self, kind):
        self.calls.append(("set_estimator", kind))

    def set_subbands(self, F, bins, tables, combine):
        self.calls.append(("set_subbands", F, list(bins), tables, combine))

    def set_subband_tables(self, tables):
        self.calls.append(("set_subband_tables", tables))


def _helper_modules(monkeypatch):
    """The helper module as it stands here (the GNU-Radio-less class) and loaded against a stand-in gnuradio.gr (the hier block)."""
    import importlib.util
    import os
    import sys
    import types
    import gr_baz_amd.baz as baz
    from gr_baz_amd.baz import music_doa_helper as plain
    monkeypatch.setattr(baz, "music_doa", _Impl)
    gr = types.ModuleType("gnuradio.gr")
    gr.sizeof_float, gr.sizeof_gr_complex = 4, 8
    gr.io_signature = gr.io_signature2 = gr.io_signature3 = lambda *a: a

    class hier_block2(object):
        def __init__(self, *a):
            pass

        def connect(self, *a):
            pass

    gr.hier_block2 = hier_block2
    pkg = types.ModuleType("gnuradio")
    pkg.gr = gr
    monkeypatch.setitem(sys.modules, "gnuradio", pkg)
    monkeypatch.setitem(sys.modules, "gnuradio.gr", gr)
    spec = importlib.util.spec_from_file_location("gr_baz_amd.baz._music_doa_helper_under_gr_subband", plain.__file__)
    under_gr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(under_gr)
    assert under_gr._HAVE_GR
    return [plain, under_gr] if not plain._HAVE_GR else [under_gr]


def test_both_helper_classes_derive_and_keep_the_setting(monkeypatch, capsys):
    """set_subbands(sample_rate, block, occupied, combine): the bins, one table per bin at its own wavelength, the default rule by
    estimator; set_frequency() retunes the centre table and all S subband tables; None switches off."""
    arr = mo.array_geometry(4)
    fc, fs, F, res = mo.FREQUENCY, 0.4 * mo.FREQUENCY, 8, 90
    for mod in _helper_modules(monkeypatch):
        h = mod.music_doa_helper(4, 2, 4 * 64, res, fc, mo.SPACING, arr)
        scaled = mo.scaled_array(arr, mo.SPACING)

        def want_tables(f):
            return [mo.calculate_antenna_array_response(scaled, res, l) for l in sr.wavelengths(f, fs, F, sr.used_bins(F, 0.75))]

        h.set_subbands(fs, F)
        call = h.impl.calls[-1]
        assert call[:3] == ("set_subbands", F, [0, 1, 2, 3, 5, 6, 7]) and call[4] == 0          # harmonic under MUSIC
        assert np.array_equal(np.array(call[3]), np.array(want_tables(fc)))
        h.set_frequency(0.8 * fc)                                                                # stays in force: all S tables follow
        assert [c[0] for c in h.impl.calls[-2:]] == ["set_array_response", "set_subband_tables"]
        assert np.array_equal(np.array(h.impl.calls[-1][1]), np.array(want_tables(0.8 * fc)))
        assert np.array_equal(np.array(h.array_response), np.array(mo.calculate_antenna_array_response(scaled, res, mo.C_LIGHT / (0.8 * fc))))
        h.set_estimator("capon")
        h.set_subbands(fs, 16, occupied=0.5)
        call = h.impl.calls[-1]
        assert call[1:3] == (16, sr.used_bins(16, 0.5)) and call[4] == 1                         # arithmetic for the powers
        h.set_subbands(fs, F, combine="harmonic")
        assert h.impl.calls[-1][4] == 0
        with pytest.raises(ValueError):
            h.set_subbands(fs, F, combine=2)
        with pytest.raises(ValueError):
            h.set_subbands(fs, 1)
        h.set_subbands(None, 0)
        assert h.impl.calls[-1] == ("set_subbands", 0, [], [], 0)
        h.set_frequency(fc)
        assert h.impl.calls[-1][0] == "set_array_response"                                       # off: nothing else is retuned
    capsys.readouterr()


# ---- known answers ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(sr.SCENES)))
def test_known_answer_on_the_host(k):
    """Two or three emitters that fill 75 % of a band 0.4 x the carrier wide: subband MUSIC (the library's channeliser, the oracle per
    subband on that subband's table, the harmonic combine, the peak picker) puts every emitter in its exact bin in 16 of 16 items;
    narrowband MUSIC on the centre table does so in at most 8 of 16."""
    items, centre, bins, tabs, s = sr.scene(k)
    m, n, F = s["m"], s["n"], s["F"]
    assert [sr.offset(b, F) for b in bins] == list(range(0, len(bins) // 2 + 1)) + list(range(-(len(bins) // 2), 0))
    narrow = sr.pick(sr.music_rows(items, centre, m, n), n, peak=True)[0]
    W = capi.subband_twiddles(F, bins)
    y = sr.channelise_items(W, items, m)                                     # (S, items, m Q)
    P = np.stack([sr.music_rows(y[i], tabs[i], m, n) for i in range(len(bins))])
    wide = sr.pick(sr.combine(P), n, peak=True)[0]
    hits_n, hits_w = sr.exact_hits(narrow, s["angles"]), sr.exact_hits(wide, s["angles"])
    print("scene %d (m %d, F %d, %d subbands): narrowband %d / 16, subband %d / 16" % (k, m, F, len(bins), hits_n, hits_w))
    assert hits_w == 16
    assert hits_n <= 8
