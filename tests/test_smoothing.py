"""Opt-in forward-backward averaging / spatial smoothing (baz_music_set_smoothing): CPU part -- the numpy restatement, the
library's host-only structure check, the coherent-emitter property on the oracle, and argument checks that need no device."""
import time

import numpy as np
import pytest

import smoothing_ref as sr
from helpers import oracle_fp64
from oracle import music_oracle as mo


def _capi():
    from gr_baz_amd import capi
    return capi


def _random_table(res, m, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((res, m)) + 1j * rng.standard_normal((res, m))).astype(np.complex64)


@pytest.mark.parametrize("m,ms,fb", [(8, 6, False), (8, 6, True), (8, 8, True), (5, 2, True), (6, 4, False)])
def test_restacked_covariance_is_the_smoothed_covariance(m, ms, fb):
    rng = np.random.default_rng(m * 100 + ms)
    K = 16
    x = (rng.standard_normal((3, m * K)) + 1j * rng.standard_normal((3, m * K))).astype(np.complex64)
    perm = np.arange(ms)[::-1]
    R = sr.covariance(x, m)
    L = m - ms + 1
    want = sum(R[:, l:l + ms, l:l + ms] for l in range(L)) / L
    if fb:
        P = np.eye(ms)[perm]
        want = (want + P @ np.conj(want) @ P.T) / 2
    got = sr.covariance(sr.restack(x, m, ms, fb, perm), ms)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


GEOMETRIES = [
    # name, array, subarray for the SS check, passes SS, passes FB (at subarray = m)
    ("ula8", sr.ula(8), 6, True, True),
    ("square", mo.array_geometry(4), 3, False, True),
    ("circle8", mo.array_geometry(8), 6, False, True),
    ("circle7", mo.array_geometry(7), 5, False, False),
    ("random8", None, 6, False, False),
]


@pytest.mark.parametrize("name,arr,ms,ss_ok,fb_ok", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_structure_check_outcomes(name, arr, ms, ss_ok, fb_ok):
    capi = _capi()
    res = 720
    table = _random_table(res, 8) if arr is None else sr.table_of(arr, res)
    m = table.shape[1]
    for sub, fb, want in ((ms, False, ss_ok), (m, True, fb_ok), (ms, True, ss_ok and fb_ok)):
        lib_perm = capi.smoothing_check(m, res, table, sub, fb)
        ref_perm = sr.check(table, sub, fb)
        assert (lib_perm is not None) == want, (name, sub, fb)
        assert (ref_perm is not None) == want, (name, sub, fb)
        if want:
            assert np.array_equal(lib_perm, ref_perm), (lib_perm, ref_perm)
            assert np.array_equal(lib_perm[lib_perm], np.arange(sub))          # an involution
    if name == "square":
        assert np.array_equal(capi.smoothing_check(4, res, table, 4, True), [2, 3, 0, 1])


def test_structure_check_is_fast_on_the_largest_array():
    """m = 64, 36,000 bins: the FB involution is screened on a few bins and verified once per bin, not searched per bin."""
    capi = _capi()
    m, res = 64, 36000
    table = sr.table_of(sr.ula(m), res)
    capi.smoothing_check(m, res, table, m, True)            # warm the page cache / library
    t0 = time.perf_counter()
    perm = capi.smoothing_check(m, res, table, m, True)
    dt = time.perf_counter() - t0
    assert perm is not None and np.array_equal(perm, np.arange(m)[::-1])
    assert sr.fb_holds(table, m, perm)
    assert dt < 0.05, "FB check took %.1f ms" % (dt * 1e3)
    # an even circle of 32 elements: P pairs opposite elements
    t32 = sr.table_of(mo.array_geometry(32), 3600)
    p32 = capi.smoothing_check(32, 3600, t32, 32, True)
    assert np.array_equal(p32, (np.arange(32) + 16) % 32) and sr.fb_holds(t32, 32, p32)


def test_structure_check_rejects_bad_arguments():
    capi = _capi()
    t = sr.table_of(sr.ula(8), 360)
    for sub in (0, 1, 9):
        assert capi.smoothing_check(8, 360, t, sub, True) is None
    L = capi.lib()
    assert L.baz_music_smoothing_check(8, 360, None, 6, 1, None) == capi.E_INVALID


def test_null_context_is_invalid():
    capi = _capi()
    import ctypes
    L = capi.lib()
    assert L.baz_music_set_smoothing(None, 6, 1) == capi.E_INVALID
    ms, fb = ctypes.c_uint32(0), ctypes.c_int(0)
    assert L.baz_music_get_smoothing(None, ctypes.byref(ms), ctypes.byref(fb)) == capi.E_INVALID


MODES = [("plain", 8, False), ("fb", 8, True), ("ss6", 6, False), ("fb_ss6", 6, True)]


def coherent_rates(coherent, seed=2024, batch=200):
    """Share of items whose 4 strongest peaks hold both emitters (mirror-folded, +-2 degrees), per mode, on the fp64 oracle."""
    res, m, n = 720, 8, 2
    arr = sr.ula(m)
    table = sr.table_of(arr, res)
    items = sr.two_emitters(batch, arr, 64, coherent=coherent, seed=seed)
    out = {}
    for name, ms, fb in MODES:
        y = sr.restack(items, m, ms, fb) if (ms < m or fb) else items
        spec = oracle_fp64(y, table[:, :ms], ms, n)[2]
        out[name] = sr.success_rate(sr.picked(spec))
    return out


def test_smoothing_recovers_coherent_emitters_on_the_oracle():
    """8-element ULA, emitters at 40.3 and 121.7 degrees, K = 64, noise 0.1, 200 items, seed 2024.  This seed gives, coherent:
    plain 0.28, FB 0.99, SS(6) 1.00, FB + SS(6) 1.00; incoherent: 1.00 in every mode."""
    coh = coherent_rates(True)
    assert coh["plain"] < 0.5 and coh["fb"] > 0.9 and coh["ss6"] > 0.95 and coh["fb_ss6"] > 0.95, coh
    inc = coherent_rates(False)
    assert all(v > 0.95 for v in inc.values()), inc
