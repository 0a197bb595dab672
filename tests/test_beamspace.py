"""The host side of the opt-in beamspace mode (include/baz_music_hip.h): baz_music_beamspace_apply against numpy with a
derived bound per word, the cases in which no order of summation matters, the normalised table rows, baz_music_beamspace_design
against numpy's eigh, the known-answer scenes by numpy alone, and argument validation.  No device is needed."""
import numpy as np
import pytest

import beamspace_ref as br
from gr_baz_amd import capi


def _f32bits(x):
    return np.ascontiguousarray(x).view(np.float32).view(np.uint32)


def _ulp_distance(a, b):
    """Distance in float32 steps between words of equal shape (finite values)."""
    def key(u):
        u = u.astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7fffffff), u)
    return np.abs(key(_f32bits(a)) - key(_f32bits(b)))


def _boundary_distance(v):
    """Distance of every fp64 value from the nearest float32 rounding boundary (a midpoint of two neighbouring float32 values)."""
    f = v.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return np.minimum(np.abs(v - (f + up) / 2), np.abs(v - (f + dn) / 2))


def _random_T(rng, m, B):
    return (rng.standard_normal((m, B)) + 1j * rng.standard_normal((m, B))) / np.sqrt(m)


@pytest.mark.parametrize("m,B", [(3, 2), (17, 5), (33, 16), (64, 16)])
def test_apply_against_numpy(m, B):
    """Every word within one float32 ulp of float32(T^H x), and equal wherever numpy's fp64 value is further than
    m 2^-52 sum_r |T_rb| |x_r| from a rounding boundary: each of the two fp64 sums of 2 m products (numpy's in its order, the library's
    r ascending by fma) stays within that of the exact value."""
    rng = np.random.default_rng(100 + m)
    T = _random_T(rng, m, B)
    x = (rng.standard_normal((37, m)) + 1j * rng.standard_normal((37, m))).astype(np.complex64)
    got = capi.beamspace_apply(T, x)
    assert got.shape == (37, B) and got.dtype == np.complex64
    v = br.project64(T, x)
    ref = v.astype(np.complex64)
    bnd = np.repeat(br.bound(T, x)[..., None], 2, axis=-1).reshape(37, 2 * B)
    v2 = np.ascontiguousarray(v).view(np.float64).reshape(37, 2 * B)
    dist = _ulp_distance(got, ref).reshape(37, 2 * B)
    assert dist.max() <= 1, "a word is %d float32 steps from float32(T^H x)" % dist.max()
    clear = _boundary_distance(v2) > bnd
    assert clear.mean() > 0.99                       # (the bound is ~1e-8 of an ulp's width: almost every word is decided)
    assert not dist[clear].any(), "%d words differ away from every rounding boundary" % np.count_nonzero(dist[clear])


def test_exact_cases_no_order_matters():
    """Columns 2^k e_i, 2^k (e_i +- e_j), 2^k (e_i +- i e_j) on small integers: every product and sum is exact, so the words are the
    hand-formed float32 values."""
    rng = np.random.default_rng(7)
    m = 19
    x = (rng.integers(1, 1000, (37, m)) * rng.choice([-1, 1], (37, m))
         + 1j * rng.integers(1, 1000, (37, m)) * rng.choice([-1, 1], (37, m))).astype(np.complex64)
    xd = x.astype(np.complex128)
    for k in range(-3, 4):
        s = 2.0 ** k
        cols, want = [], []
        for (i, j) in [(0, 5), (18, 3), (7, 8)]:
            e_i, e_j = np.zeros(m, np.complex128), np.zeros(m, np.complex128)
            e_i[i], e_j[j] = 1, 1
            for c_j in (0, 1, -1, 1j, -1j):
                cols.append(s * (e_i + c_j * e_j))
                want.append(s * (xd[:, i] + np.conj(c_j) * xd[:, j]))       # conj(T)^T x
        T = np.stack(cols, axis=1)
        ref = np.stack(want, axis=1).astype(np.complex64)
        for b0 in range(0, T.shape[1], 15):
            got = capi.beamspace_apply(T[:, b0:b0 + 15], x)
            assert np.array_equal(_f32bits(got), _f32bits(ref[:, b0:b0 + 15])), "k = %d" % k


def test_normalise_rows():
    """normalise = 1: every row has unit norm to 2 ulp (each component carries one rounding of 2^-24 relative), equals the plain row
    divided by its norm to an ulp, and an all-zero input row gives zeros."""
    rng = np.random.default_rng(11)
    m, B = 33, 8
    T = _random_T(rng, m, B)
    x = (rng.standard_normal((37, m)) + 1j * rng.standard_normal((37, m))).astype(np.complex64)
    x[5] = 0
    got = capi.beamspace_apply(T, x, normalise=True)
    nrm = np.sqrt(np.sum(np.abs(got.astype(np.complex128)) ** 2, axis=1))
    live = np.arange(37) != 5
    assert np.all(np.abs(nrm[live] - 1.0) <= 2 * 2.0 ** -24), np.abs(nrm[live] - 1.0).max()
    assert not _f32bits(got[5]).any()
    assert _ulp_distance(got[live], br.project(T, x, normalise=True)[live]).max() <= 1
    assert np.array_equal(_f32bits(capi.beamspace_apply(T, x)[5]), np.zeros(2 * B, np.uint32))


# the scenes of beamspace_ref whose B-th eigenvalue is separated well enough for the projector criterion (bound <= 1e-9; the others
# sit at 2.0e-9 .. 2.4e-9 and are held to orthonormality and the captured fraction below), and one sector that wraps
DESIGN_CASES = [(32, 16, 20, 120), (24, 8, 20, 60), (17, 8, 20, 90), (24, 8, 340, 60)]


@pytest.mark.parametrize("k", range(len(br.SCENES)))
def test_design_is_orthonormal_on_every_scene(k):
    s = br.SCENES[k]
    table = br.table_of(s["m"])
    T, captured = capi.beamspace_design(table, s["lo"], s["cnt"], s["B"])
    assert np.abs(T.conj().T @ T - np.eye(s["B"])).max() <= 64 * s["m"] * 2.0 ** -52
    assert abs(captured - br.design(table, s["lo"], s["cnt"], s["B"])[1]) <= 1e-12
    k_big = np.argmax(np.abs(T), axis=0)
    big = T[k_big, np.arange(s["B"])]
    assert np.all(big.imag == 0.0) and np.all(big.real > 0.0)


@pytest.mark.parametrize("m,B,lo,cnt", DESIGN_CASES)
def test_design_against_eigh(m, B, lo, cnt):
    table = br.table_of(m)
    T, captured = capi.beamspace_design(table, lo, cnt, B)
    Tn, cap_n, w = br.design(table, lo, cnt, B)
    u = m * 2.0 ** -52
    sep = 64 * u * w[0] / (w[B - 1] - w[B])
    print("design m=%d B=%d sector [%d, +%d): bound %.3g" % (m, B, lo, cnt, sep))
    assert sep <= 1e-9, "the case does not separate the B-th eigenvalue well enough for the criterion: %.3g" % sep
    P, Pn = T @ T.conj().T, Tn @ Tn.conj().T
    err = np.linalg.norm(P - Pn, 2)
    print("   |T T^H - eigh's| = %.3g, |T^H T - I| = %.3g, captured %.12f" % (err, np.abs(T.conj().T @ T - np.eye(B)).max(), captured))
    assert err <= sep
    assert np.abs(T.conj().T @ T - np.eye(B)).max() <= 64 * u
    assert abs(captured - cap_n) <= 1e-12
    # phase convention: the largest-modulus component of every column is real and positive
    for b in range(B):
        k = int(np.argmax(np.abs(T[:, b])))
        assert T[k, b].imag == 0.0 and T[k, b].real > 0.0
    # eigenvalues in descending order: the Rayleigh quotients of the columns
    C = br.sector_covariance(table, lo, cnt)
    ray = np.real(np.einsum("rb,rs,sb->b", T.conj(), C, T))
    assert np.all(np.diff(ray) <= 1e-9 * w[0])
    assert np.allclose(ray, w[:B], rtol=0, atol=1e-9 * w[0])


def test_design_wrapping_sector_is_the_rotated_sector():
    """A sector that wraps past bin res - 1 is the sum over the same bins as two plain sectors' sum."""
    table = br.table_of(24)
    rolled = np.roll(table, 40, axis=0)                 # bin b of `rolled` is bin b - 40 of `table`
    T1, c1 = capi.beamspace_design(table, 340, 60, 8)
    T2, c2 = capi.beamspace_design(rolled, 20, 60, 8)
    assert np.array_equal(T1, T2) and c1 == c2


@pytest.mark.parametrize("k", range(len(br.SCENES)))
def test_known_answer_on_the_host(k):
    """The five scenes: the library's design and projection, the oracle's MUSIC and peak picker: both emitters within one bin in all
    16 items."""
    table, items, s = br.scene(k)
    m, B = s["m"], s["B"]
    T, captured = capi.beamspace_design(table, s["lo"], s["cnt"], B)
    y = capi.beamspace_apply(T, items.reshape(len(items), -1, m))
    ang, lvl, spec = br.music(y, capi.beamspace_apply(T, table), B, 2)
    err = br.bin_errors(ang, s["angles"])
    print("scene %d: captured %.5f, bin errors %s" % (k, captured, err.tolist()))
    assert np.all(lvl > 0) and np.all(err <= 1.0)
    # ... and by numpy alone (design included): the same
    Tn, _, _ = br.design(table, s["lo"], s["cnt"], B)
    ang_n, lvl_n, _ = br.beamspace_music(Tn, table, items, m, 2)
    assert np.all(br.bin_errors(ang_n, s["angles"]) <= 1.0)


def test_argument_validation():
    rng = np.random.default_rng(3)
    L = capi.lib()
    T = np.ascontiguousarray(_random_T(rng, 8, 4))
    x = np.zeros((3, 8), np.complex64)
    out = np.zeros((3, 4), np.complex64)
    import ctypes
    f64p, f32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    tp, xp, op = T.view(np.float64).ctypes.data_as(f64p), x.view(np.float32).ctypes.data_as(f32p), out.view(np.float32).ctypes.data_as(f32p)
    assert L.baz_music_beamspace_apply(8, 4, tp, 0, xp, 3, op) == capi.OK
    assert L.baz_music_beamspace_apply(8, 4, tp, 0, xp, 0, None) == capi.OK
    for args in [(1, 1, tp, 0, xp, 3, op), (65, 4, tp, 0, xp, 3, op), (8, 0, tp, 0, xp, 3, op), (8, 9, tp, 0, xp, 3, op),
                 (32, 17, tp, 0, xp, 3, op), (8, 4, None, 0, xp, 3, op), (8, 4, tp, 0, None, 3, op), (8, 4, tp, 0, xp, 3, None)]:
        assert L.baz_music_beamspace_apply(*args) == capi.E_INVALID, args[:2]
    table = br.table_of(8)
    tb = table.view(np.float32).ctypes.data_as(f32p)
    To, cap = np.zeros((8, 4), np.complex128), ctypes.c_double(0)
    top = To.view(np.float64).ctypes.data_as(f64p)
    assert L.baz_music_beamspace_design(8, 360, tb, 350, 360, 4, top, ctypes.byref(cap)) == capi.OK
    assert L.baz_music_beamspace_design(8, 360, tb, 0, 10, 4, top, None) == capi.OK
    for args in [(8, 360, tb, 0, 0, 4, top), (8, 360, tb, 0, 361, 4, top), (8, 360, tb, 0, 10, 0, top), (8, 360, tb, 0, 10, 9, top),
                 (8, 0, tb, 0, 10, 4, top), (8, 360, None, 0, 10, 4, top), (8, 360, tb, 0, 10, 4, None), (1, 360, tb, 0, 10, 1, top),
                 (65, 360, tb, 0, 10, 4, top)]:
        assert L.baz_music_beamspace_design(*(args + (None,))) == capi.E_INVALID, args
    with pytest.raises(ValueError):
        capi.beamspace_design(table, 0, 0, 4)
    with pytest.raises(ValueError):
        capi.beamspace_apply(T, np.zeros((3, 7), np.complex64))
    bad = table.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        capi.beamspace_design(bad, 0, 10, 4)


def test_symbols_are_listed():
    for s in ("set_beamspace", "get_beamspace", "debug_beamspace", "beamspace_apply", "beamspace_design"):
        assert "baz_music_" + s in capi.SYMBOLS
