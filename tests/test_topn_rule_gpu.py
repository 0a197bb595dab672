"""Every kernel that builds an (angle, strength) list, held to the reference's insertion rule (lib/baz_music_doa.cc:95,129-141: strict
'>' over ascending bins) on scenes with EXACT ties, infinities, fewer bins than list entries and plateaus (tests/topn_scenes.py;
tests/test_topn_scenes.py proves their conditions on the CPU).  The angles are compared EXACTLY with the insertion rule applied to the
oracle's fp64 strengths: every scene separates the values that compete for the list by >= 1e-3 relative, so which BIN wins never
depends on rounding, only on the rule -- the earliest bin of a tie first, +inf for d = 0, (0, 0) once the bins run out.

Each case names the kernel it is meant to run (ctx.stage_name(2) after the call), so that a change of the scan's decision table
cannot silently move it elsewhere:
    scan_mfma_kernel      the packed-key min/max network, list widths 2 / 4 / 8 / 16 and the two short forms, + topn_merge_kernel
    scan_coarse_kernel    the gated scan (no spectrum port, m <= 8, n <= 4): its gate |d| <= (K_n | low bits) must let ties through
    scan_i8_kernel        the int8 scan (6 .. 16 antennas, n <= 4)
    scan_wide_mfma_kernel / scan_wide_kernel + topn_wide_kernel (17 .. 64 antennas)
    peak_pick_kernel, topn_spec_kernel on the float32 row
"""
import numpy as np
import pytest

import topn_scenes as ts
from helpers import assert_spectrum_close
from oracle import music_oracle as mo
from test_gpu_parity import device_run

pytestmark = pytest.mark.gpu

SWITCHES = ("BAZ_MUSIC_COARSE", "BAZ_MUSIC_EXACT", "BAZ_MUSIC_NSPLIT", "BAZ_MUSIC_WIDE_MFMA")


def _capi():
    from gr_baz_amd import capi
    return capi


def fp64(m):
    return "bazmusic::scan_mfma_kernel<%d," % m


def i8(m):
    return "bazmusic::scan_i8_kernel<%d," % m


def gated(m):
    return "bazmusic::scan_coarse_kernel<%d," % m


WIDE_MFMA = "bazwide::scan_wide_mfma_kernel"
WIDE_SCALAR = "bazwide::scan_wide_kernel"


def merge_kernel(scene, scan):
    """the kernel that folds the scan's output into ang / lvl (stage 3): topn_wide_kernel behind the wide scalar scan, else
    topn_merge_kernel at the list width of n (the wide matrix-core scan keeps at most 8 keys)"""
    if scan == WIDE_SCALAR:
        return "bazwide::topn_wide_kernel"
    return "bazmusic::topn_merge_kernel<%d>" % next(w for w in (2, 4, 8, 16) if scene.n <= w)


def assert_infinities(got, want, what):
    """+inf, bit for bit (0x7F800000), exactly where the oracle has +inf -- not NaN, not -inf -- and nowhere else"""
    want_inf = np.isposinf(np.asarray(want, dtype=np.float64))
    assert np.array_equal(_bits(got) == 0x7F800000, want_inf), "%s: +inf not exactly where the oracle has it" % what
    assert not np.isnan(got).any() and not np.isneginf(got).any(), "%s: NaN or -inf" % what


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _writable(items):
    """a scene's arrays are shared and read-only; torch wants a writable array to wrap"""
    return items.copy()


def _context(scene, monkeypatch, env=None, lab=False):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return _capi().Context(scene.m, scene.n, scene.nsamples, scene.res, scene.table, lab=True if lab else None)


def run_case(scene, gpu_device, monkeypatch, with_spec, without_spec, env=None, lab=False):
    """One context, the scene's items through every wiring; the checks of the module's docstring.  with_spec / without_spec: the scan
    kernel of a launch with / without the spectrum port.  Returns {"spec": (ang, lvl, spectrum), "nospec": (ang, lvl)}."""
    s = scene
    with _context(s, monkeypatch, env, lab) as ctx:
        a3, l3, s3 = device_run(ctx, _writable(s.items), gpu_device)
        k3, g3 = ctx.stage_name(2), ctx.stage_name(_capi().STAGE_MERGE)
        a2, l2, _ = device_run(ctx, _writable(s.items), gpu_device, want_spec=False)
        k2, g2 = ctx.stage_name(2), ctx.stage_name(_capi().STAGE_MERGE)
        a1, _, _ = device_run(ctx, _writable(s.items), gpu_device, want_lvl=False, want_spec=False)
        k1 = ctx.stage_name(2)
        h3 = ctx.process(s.items)
        h2 = ctx.process(s.items, want_spectrum=False)
    what = "%s %s" % (s.name, env or "")
    # 1. the kernels: the scan, and what folds its output into the list
    assert k3 == with_spec, (what, k3)
    assert k2 == without_spec and k1 == without_spec, (what, k2, k1)
    assert g3 == merge_kernel(s, with_spec) and g2 == merge_kernel(s, without_spec), (what, g3, g2)
    # 2. the angles, exactly
    assert np.array_equal(a3, s.ang), "%s: ang with the spectrum port\n%s\nexpected\n%s" % (what, _rows(a3, s), _rows(s.ang, s))
    # 3. spectrum port wired: lvl is the stored word, the copies of a period are the same bits, the spectrum is the oracle's
    used = s.lvl > 0
    rows = np.arange(s.items.shape[0])[:, None]
    assert np.array_equal(_bits(l3), _bits(np.where(used, s3[rows, s.bins], np.float32(0.0)))), "%s: lvl != spectrum[bin]" % what
    for k in range(1, s.copies):
        assert np.array_equal(_bits(s3[:, :s.period]), _bits(s3[:, k * s.period:(k + 1) * s.period])), "%s: copy %d differs" % (what, k)
    assert_spectrum_close(s3, s.strength, what=what + " spectrum")
    assert_infinities(s3, s.strength, what + " spectrum")
    assert_infinities(l3, s.lvl, what + " lvl with the spectrum port")
    # 4. without the spectrum port, and without the strength port
    assert np.array_equal(a2, s.ang), "%s: ang without the spectrum port\n%s\nexpected\n%s" % (what, _rows(a2, s), _rows(s.ang, s))
    assert np.array_equal(a1, s.ang), "%s: ang with the angle port alone" % what
    assert_spectrum_close(l2, s.lvl, what=what + " lvl without the spectrum port")
    assert_infinities(l2, s.lvl, what + " lvl without the spectrum port")
    assert not _bits(l2)[~used].any() and not _bits(l3)[~used].any()          # a missing entry is (+0, +0)
    # 5. the host path
    for x, y in zip(h3, (a3, l3, s3)):
        assert np.array_equal(_bits(x), _bits(y)), "%s: host path differs from the device path" % what
    assert np.array_equal(_bits(h2[0]), _bits(a2)) and np.array_equal(_bits(h2[1]), _bits(l2)) and h2[2] is None
    return {"spec": (a3, l3, s3), "nospec": (a2, l2)}


def _rows(ang, scene, limit=4):
    """the bins of the first rows that differ from the expected ones (for the failure message)"""
    bad = np.nonzero(np.any(np.asarray(ang) != scene.ang, axis=1))[0][:limit]
    return "\n".join("  item %d: bins %s" % (b, np.rint(np.asarray(ang, np.float64)[b] * scene.res / 360.0).astype(int).tolist()) for b in bad)


# ------------------------------------------------------------------ tied tables, the default path of every shape
# name -> (kernel with the spectrum port, kernel without)
DEFAULT = {
    "tied-m3-n1": (fp64(3), gated(3)),
    "tied-m4-n2": (fp64(4), gated(4)),
    "tied-m4-n3": (fp64(4), gated(4)),
    "tied-m8-n2": (i8(8), gated(8)),
    "tied-m6-n4": (i8(6), gated(6)),
    "tied-m16-n2": (i8(16), i8(16)),
    "tied-m11-n3": (i8(11), i8(11)),
    "tied-m9-n1": (i8(9), i8(9)),
    "tied-m6-n5": (fp64(6), fp64(6)),           # n > 4: the fp64 scan in every wiring; list widths 8, 8, 16, 16
    "tied-m8-n7": (fp64(8), fp64(8)),
    "tied-m13-n12": (fp64(13), fp64(13)),
    "tied-m16-n15": (fp64(16), fp64(16)),
    "tied-m18-n3": (WIDE_MFMA, WIDE_MFMA),
    "tied-m20-n9": (WIDE_SCALAR, WIDE_SCALAR),  # n > 8: the scalar scan and topn_wide_kernel
}
assert sorted(DEFAULT) == sorted(ts.tied_names())


@pytest.mark.parametrize("name", list(DEFAULT))
def test_tied_table_on_the_default_path(name, gpu_device, monkeypatch):
    run_case(ts.make(name), gpu_device, monkeypatch, *DEFAULT[name])


# ------------------------------------------------------------------ the fp64 scan where the int8 scan is the default
EXACT = {
    "tied-m16-n2": (fp64(16), fp64(16)),        # short form, two emitters
    "tied-m9-n1": (fp64(9), fp64(9)),           # short form, one emitter
    "tied-m11-n3": (fp64(11), fp64(11)),        # projector form, list width 4, two tiles of antennas
    "tied-m8-n2": (fp64(8), gated(8)),
    "tied-m6-n4": (fp64(6), gated(6)),
}


@pytest.mark.parametrize("name", list(EXACT))
def test_tied_table_on_the_fp64_scan(name, gpu_device, monkeypatch):
    run_case(ts.make(name), gpu_device, monkeypatch, *EXACT[name], env={"BAZ_MUSIC_EXACT": "1"})


# ------------------------------------------------------------------ the gated scan against the full scan
UNGATED = {
    "tied-m3-n1": (fp64(3), fp64(3)),
    "tied-m4-n2": (fp64(4), fp64(4)),
    "tied-m4-n3": (fp64(4), fp64(4)),
    "tied-m8-n2": (i8(8), fp64(8)),
    "tied-m6-n4": (i8(6), fp64(6)),
}


@pytest.mark.parametrize("name", list(UNGATED))
def test_gated_scan_lets_every_tie_through(name, gpu_device, monkeypatch):
    """scan_coarse_kernel evaluates a tile exactly when its coarse bound can reach the n-th key; a tie WITH the n-th key must pass
    (the later copies of a value belong in the list).  With BAZ_MUSIC_COARSE=0 the full scan runs: the same bits."""
    s = ts.make(name)
    on = run_case(s, gpu_device, monkeypatch, *DEFAULT[name])
    off = run_case(s, gpu_device, monkeypatch, *UNGATED[name], env={"BAZ_MUSIC_COARSE": "0"})
    assert np.array_equal(_bits(on["nospec"][0]), _bits(off["nospec"][0]))
    assert np.array_equal(_bits(on["nospec"][1]), _bits(off["nospec"][1]))


# ------------------------------------------------------------------ bin ranges: tied copies in different ranges
@pytest.mark.parametrize("name", ["tied-m4-n2", "tied-m8-n2"])
def test_ties_across_bin_ranges(name, gpu_device, monkeypatch):
    """res = 320 is five 64-bin steps and the period is 80 bins: the copies of a value sit in different steps, so with more than one
    bin range per row topn_merge_kernel decides between them.  One, two and the most ranges (64 is clamped to what the kernel
    takes): the fp64 / int8 scan with the spectrum port and the gated scan without, bit-identical throughout.
    (The library offers no read-back of the split it used, so that BAZ_MUSIC_NSPLIT was honoured is NOT verified here: were the
    switch ignored, the three runs would be one run.  Every run is still held to the expected list, and at 33 items the default
    geometry already cuts a row into several ranges, so ties are merged across ranges either way.)"""
    s = ts.make(name)
    assert s.res == 320 and s.period == 80
    outs = [run_case(s, gpu_device, monkeypatch, *DEFAULT[name], env={"BAZ_MUSIC_NSPLIT": split}, lab=True) for split in ("1", "2", "64")]
    for o in outs[1:]:
        for key in ("spec", "nospec"):
            for x, y in zip(outs[0][key], o[key]):
                assert np.array_equal(_bits(x), _bits(y)), (name, key)


# ------------------------------------------------------------------ the wide path's scalar scan at a shape the matrix core takes by default
def test_wide_scalar_scan_on_the_matrix_core_shape(gpu_device, monkeypatch):
    run_case(ts.make("tied-m18-n3"), gpu_device, monkeypatch, WIDE_SCALAR, WIDE_SCALAR, env={"BAZ_MUSIC_WIDE_MFMA": "0"}, lab=True)


# ------------------------------------------------------------------ more than 65,536 bins: the 20-bit bin field
def test_wide_key_keeps_bit_16_of_the_bin(gpu_device, monkeypatch):
    """the list is [b, b + 65,536]: a 16-bit bin field would report b twice (or b + 65,536 as b); the 61,440-bin plateau between
    the two copies of the table must not reach the list"""
    s = ts.make("widekey")
    assert np.all(s.bins[:, 1] == s.bins[:, 0] + 65536)
    run_case(s, gpu_device, monkeypatch, fp64(3), gated(3))


# ------------------------------------------------------------------ d = 0: +inf, ordered by bin
ZEROS = {
    "zero-m4": (fp64(4), gated(4)),
    "zero-m8": (i8(8), gated(8)),
    "zero-m8-r40": (i8(8), gated(8)),
    "zero-m18": (WIDE_MFMA, WIDE_MFMA),
    # an all-zero table has no scale: neither approximate scan can form its image, the fp64 scan runs in every wiring
    "allzero-m4": (fp64(4), fp64(4)),
    "allzero-m8": (fp64(8), fp64(8)),
    "allzero-m18": (WIDE_MFMA, WIDE_MFMA),
}
assert sorted(ZEROS) == sorted(list(ts.ZERO) + list(ts.ALLZERO))


@pytest.mark.parametrize("name", list(ZEROS))
def test_zero_table_rows_insert_infinity(name, gpu_device, monkeypatch):
    """an all-zero table row has d = 0 exactly: the reference inserts a strength of +inf, the earlier bin first; on the device the key
    of such a bin is a denormal double (its bits are the bin index alone)"""
    s = ts.make(name)
    assert np.isinf(s.lvl[:, 0]).all()
    run_case(s, gpu_device, monkeypatch, *ZEROS[name])


# ------------------------------------------------------------------ fewer bins than list entries
SHORT = {
    "short-m8-n7": (fp64(8), fp64(8)),
    "short-m16-n15": (fp64(16), fp64(16)),
    "short-m4-n3": (fp64(4), gated(4)),
    "short-m6-n4": (i8(6), gated(6)),
    "short-m20-n19": (WIDE_SCALAR, WIDE_SCALAR),
}
assert sorted(SHORT) == sorted(ts.short_names())


@pytest.mark.parametrize("name", list(SHORT))
def test_short_table_ends_in_zero_pairs(name, gpu_device, monkeypatch):
    s = ts.make(name)
    assert s.res < s.n and np.all(s.lvl[:, s.res:] == 0.0)
    run_case(s, gpu_device, monkeypatch, *SHORT[name])


# ------------------------------------------------------------------ the local-maximum picker on plateaus
@pytest.mark.parametrize("name", ts.plateau_names())
def test_peak_mode_on_plateaus(name, gpu_device, monkeypatch):
    """peak_pick_kernel: a plateau counts once, at its first bin -- bin res-1 for the plateau that wraps from res-1 to 0 --, and a
    constant row has no peak: (0, 0) throughout.  ang / lvl are the definition (music_oracle.peak_pick) applied to the spectrum the
    device itself wrote, and ang is the answer pinned on the CPU."""
    s = ts.make(name)
    which, m = name.split("-")[1], s.m
    n = s.n
    base, items = ts.plateau_base(m)
    base_spec = mo.music_doa_work_batch(items, base, m, n)[2]
    bins, used = ts.plateau_answer(which, base_spec, n)
    want_ang = ts.angles_of(bins, used, s.res)
    with _context(s, monkeypatch) as ctx:
        ctx.set_peak_mode(1)
        a3, l3, s3 = device_run(ctx, _writable(s.items), gpu_device)
        k3 = ctx.stage_name(2)
        a2, l2, _ = device_run(ctx, _writable(s.items), gpu_device, want_spec=False)          # (the picker reads a private spectrum)
        k2 = ctx.stage_name(2)
        a1, _, _ = device_run(ctx, _writable(s.items), gpu_device, want_lvl=False, want_spec=False)
        h3 = ctx.process(s.items)
    assert k3 == k2 == (fp64(m) if m <= 4 else i8(m)), (k3, k2)
    assert_spectrum_close(s3, s.strength)
    if which == "constant":
        assert np.all(_bits(s3) == _bits(s3[:, :1]))
    else:
        pairs = s3 if which == "pairs" else np.roll(s3, 1, axis=1)
        assert np.array_equal(_bits(pairs[:, 0::2]), _bits(pairs[:, 1::2]))       # every value a two-bin plateau, bit for bit
    for b in range(s.items.shape[0]):
        ea, el = mo.peak_pick(s3[b], n)
        assert np.array_equal(_bits(a3[b]), _bits(ea)) and np.array_equal(_bits(l3[b]), _bits(el)), (name, b)
    assert np.array_equal(_bits(a3), _bits(want_ang)), name
    assert np.array_equal(_bits(a2), _bits(a3)) and np.array_equal(_bits(l2), _bits(l3)) and np.array_equal(_bits(a1), _bits(a3))
    for x, y in zip(h3, (a3, l3, s3)):
        assert np.array_equal(_bits(x), _bits(y))
    # (stage_name has no entry for the picker: stage 3 names the merge kernel of the default mode.  That peak_pick_kernel wrote these
    # lists shows in the lists: the reference's rule reports BOTH bins of the strongest plateau, the picker only its first.)
    if which != "constant":
        plain = np.stack([mo.top_n_insertion(row, n, s.res)[0] for row in s3])
        both = np.sort(np.stack([bins[:, 0], (bins[:, 0] + 1) % s.res], axis=1), axis=1)
        assert np.array_equal(np.sort(np.rint(plain[:, :2] * s.res / 360.0).astype(int), axis=1), both)
        assert np.all(a3[:, 1] != plain[:, 1].astype(np.float32))


# ------------------------------------------------------------------ the opt-in estimators' list
@pytest.mark.parametrize("kind", [1, 2], ids=["capon", "bartlett"])
@pytest.mark.parametrize("name", ["tied-m4-n3", "tied-m8-n2"])
def test_estimator_lists_follow_the_insertion_rule(name, kind, gpu_device, monkeypatch):
    """topn_spec_kernel on a float32 row whose every value occurs `copies` times: ang / lvl are the insertion rule applied to the
    device's own row, exactly"""
    s = ts.make(name)
    with _context(s, monkeypatch) as ctx:
        ctx.set_estimator(kind)
        a3, l3, s3 = device_run(ctx, _writable(s.items), gpu_device)
        assert ctx.stage_name(2) == "bazspectrum::spectrum_scan_kernel"      # (its picker, topn_spec_kernel, has no name in stage_name;
        #                                                                      with this scan and peak mode 0 no other kernel writes ang / lvl)
        a2, l2, _ = device_run(ctx, _writable(s.items), gpu_device, want_spec=False)
    assert np.all(np.isfinite(s3)) and np.all(s3 > 0)
    for k in range(1, s.copies):
        assert np.array_equal(_bits(s3[:, :s.period]), _bits(s3[:, k * s.period:(k + 1) * s.period]))
    for b in range(s.items.shape[0]):
        ea, el = mo.top_n_insertion(s3[b], s.n, s.res)
        assert np.array_equal(_bits(a3[b]), _bits(ea.astype(np.float32))), (name, b)
        assert np.array_equal(_bits(l3[b]), _bits(el.astype(np.float32))), (name, b)
    bins = np.rint(a3.astype(np.float64) * s.res / 360.0).astype(int)
    top = np.argmax(s3[:, :s.period], axis=1)
    assert np.array_equal(bins[:, 0], top) and np.array_equal(bins[:, 1], top + s.period)      # the tie: the earlier copy first
    assert np.array_equal(_bits(a2), _bits(a3)) and np.array_equal(_bits(l2), _bits(l3))
