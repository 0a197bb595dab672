"""Scenes whose covariance R = X X^H / K has STRUCTURE, for the eigensolver tests (numpy only).

The synthetic scenes of the other tests (emitters plus dense complex white noise) give generic matrices: full rank, no zero
entry, distinct eigenvalues, every start vector in general position.  The generators below give exact zeros in R, diagonal and
block-diagonal R, exactly repeated eigenvalues, rank-deficient R, real symmetric R and graded R.  The structure comes out of
the SAMPLES: an antenna that is 0 in a snapshot contributes 0 x = 0 to every product with it, amplitudes of the slots are
powers of two, so the promised zeros are exactly 0.0 in any fp64 accumulation of the products, in any order.

Every generator returns (table, items): the steering table (res, m) complex64 and the items (B, m K) complex64, antenna-
interleaved (items[b, k m + r] = antenna r in snapshot k), for m in 2..64 and B <= 40.

The module also restates, in numpy, the orthogonal iteration of evd_sub_kernel / sub_wide_kernel (start columns, scaling,
two-pass modified Gram-Schmidt, stopping rule, bail-out rule) and the dominance check that follows it, so that the CPU test
can pin each scene to the mechanism it exists to catch.
"""
import math

import numpy as np

SLOT = 4                        # snapshots of a decoupled antenna's own slot
UNITS = np.array([1.0, 1.0j, -1.0, -1.0j])


# ---- array and table (the circle of oracle.music_oracle.array_geometry at half a wavelength between neighbours) -----------------
def _positions(m):
    if m == 4:
        p = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    else:
        r = 0.5 / math.sin(math.pi / m)
        p = [[r * math.cos(2 * math.pi * k / m), r * math.sin(2 * math.pi * k / m)] for k in range(m)]
    return 0.5 * np.asarray(p, dtype=np.float64)


def steer(theta_deg, m):
    th = np.deg2rad(theta_deg)
    return np.exp(-2j * np.pi * (_positions(m) @ np.array([np.cos(th), np.sin(th)])))


def steering_table(m, res):
    return np.stack([steer(s * 360.0 / res, m) for s in range(res)]).astype(np.complex64)


def emitter_angles(n, res):
    """n angles spread over the circle, each 0.37 bin off the grid (>= 1/4 bin: no null is exactly zero)."""
    return [(round(res * (0.11 + 0.8 * i / max(n, 1))) + 0.37) * 360.0 / res for i in range(n)]


def _cgauss(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def _ordinary(rng, m, K, res, amps, sigma, rows=None, angles=None):
    """(K, m) complex128: emitters of amplitudes `amps` at `angles` (emitter_angles by default) plus white noise sigma, on the
    antennas `rows` (all by default); the other antennas are 0."""
    rows = np.arange(m) if rows is None else np.asarray(rows)
    x = np.zeros((K, m), np.complex128)
    for a, th in zip(amps, emitter_angles(len(amps), res) if angles is None else angles):
        x[:, rows] += a * _cgauss(rng, (K, 1)) * steer(th, m)[None, rows]
    x[:, rows] += sigma * _cgauss(rng, (K, len(rows)))
    return x


def _pack(xs):
    x = np.stack(xs)
    return x.reshape(x.shape[0], -1).astype(np.complex64)


def covariance(items, m):
    """(B, m, m) complex128, R = X X^H / K of the complex64 samples (the oracle's arithmetic)."""
    items = np.asarray(items, dtype=np.complex64)
    B, N = items.shape
    K = N // m
    x = items.astype(np.complex128).reshape(B, K, m).transpose(0, 2, 1)
    return (x @ x.conj().transpose(0, 2, 1)) / float(K)


# ---- the scenes -------------------------------------------------------------------------------------------------------------------
def where_of(position, m, n):
    """the decoupled antennas of a named position"""
    return {"first": [0], "first_n": list(range(n)), "middle": [m // 2], "last": [m - 1]}[position]


def decoupled_plan(m, n, strength, apart30=False):
    """(emitter amplitudes, sigma) of the coupled rest.  weak / between: n emitters, the decoupled antennas are noise
    eigenvectors.  strong: every decoupled antenna is a signal eigenvector; one emitter at n = 1 (the iteration finds it
    and misses the antenna), n - 1 emitters otherwise."""
    if apart30:
        assert n == 2 and strength != "strong"
        return [1.0, 2.0 ** -5], 2.0 ** -12              # 30.1 dB apart, noise 42 dB below the weaker one
    k = n if strength != "strong" else max(1, n - 1)
    return [1.0] * k, 2.0 ** -7


def decoupled(m, n, K, res, B, where, strength, apart30=False, seed=0):
    """The antennas in `where` are non-zero only in their own SLOT-snapshot slots (the first SLOT len(where) snapshots), where
    every other antenna is 0; the rest carry an ordinary scene in the remaining snapshots.  R[j, k] = R[k, j] = 0 exactly for
    j in where, k != j.  strength: R_jj is 'weak' (1/16 .. 1/64 of the rest's noise power), 'between' (1/128 .. 1/512 of the
    rest's lambda_n, above its lambda_(n+1)) or 'strong' (128 .. 512 times the rest's lambda_1)."""
    where = list(where)
    rest = [r for r in range(m) if r not in where]
    K0 = SLOT * len(where)
    assert K > K0 and rest
    amps, sigma = decoupled_plan(m, n, strength, apart30)
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b])
        x = np.zeros((K, m), np.complex128)
        x[K0:] = _ordinary(rng, m, K - K0, res, amps, sigma, rows=rest)
        lam = np.linalg.eigvalsh(x[K0:, rest].T @ x[K0:, rest].conj() / K)[::-1]
        if strength == "weak":
            target = sigma * sigma * (K - K0) / K / 16.0
        elif strength == "between":
            target = lam[len(amps) - 1] / 128.0
        else:
            target = lam[0] * 512.0
        for i, j in enumerate(where):
            a = 2.0 ** math.floor(0.5 * math.log2(target * K / SLOT))     # a power of two: R_jj = SLOT a^2 / K in (target / 4, target]
            a *= 2.0 ** (i if strength == "strong" else -i)               # (distinct per antenna, away from the rest's eigenvalues)
            x[SLOT * i:SLOT * (i + 1), j] = a * UNITS[rng.integers(0, 4, SLOT)]
        xs.append(x)
    return steering_table(m, res), _pack(xs)


def decoupled_zero_mask(m, where):
    z = np.zeros((m, m), bool)
    for j in where:
        z[j, :] = True
        z[:, j] = True
        z[j, j] = False
    return z


def diagonal(m, n, res, B, ties=False, K=None, seed=0):
    """K = m snapshots (more: zero snapshots follow), antenna pi(k) alone in snapshot k with amplitude 2^e: R is exactly diagonal, R_jj = 4^e_j / K, in a
    shuffled order per item.  Signal exponents 8 .. 8+n-1, noise exponents 0, -1, ..: distinct, lambda_n / lambda_(n+1) = 4^8.
    ties: the two largest signal exponents are equal (n >= 2) and the two largest noise exponents are equal (m - n >= 2):
    exactly repeated eigenvalues, never across the n-th."""
    e = np.concatenate([8.0 + np.arange(n), -np.arange(m - n)])
    if ties:
        if n >= 2:
            e[n - 1] = e[n - 2]
        if m - n >= 2:
            e[n + 1] = e[n]
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b, 1])
        ant = rng.permutation(m)                                  # exponent i sits on antenna ant[i] ...
        snap = rng.permutation(m)                                 # ... in snapshot snap[i]
        x = np.zeros((max(m, K or m), m), np.complex128)
        x[snap, ant] = 2.0 ** e * UNITS[rng.integers(0, 4, m)]
        xs.append(x)
    return steering_table(m, res), _pack(xs)


def diagonal_zero_mask(m):
    return ~np.eye(m, dtype=bool)


def blocks_of(m):
    h = (m + 1) // 2
    return list(range(h)), list(range(h, m))


def block_diagonal(m, n, K, res, B, seed=0):
    """Sub-arrays A (the first ceil(m/2) antennas) and B (the rest) are active in alternating SLOT-snapshot slots, the other
    one is 0: R = blockdiag(R_A, R_B) exactly.  ceil(n/2) emitters of amplitude 1 in A, floor(n/2) of amplitude 1/2 in B."""
    A, Bk = blocks_of(m)
    nA = (n + 1) // 2
    nB = n - nA
    assert K % (2 * SLOT) == 0
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b, 2])
        angles = emitter_angles(n, res)                           # (B's emitters at their own angles, not A's)
        xa = _ordinary(rng, m, K // 2, res, [1.0] * nA, 2.0 ** -7, rows=A, angles=angles[:nA])
        xb = _ordinary(rng, m, K // 2, res, [0.5] * nB, 2.0 ** -7, rows=Bk, angles=angles[nA:])
        x = np.zeros((K, m), np.complex128)
        for s in range(K // (2 * SLOT)):
            x[2 * SLOT * s:2 * SLOT * s + SLOT] = xa[SLOT * s:SLOT * (s + 1)]
            x[2 * SLOT * s + SLOT:2 * SLOT * (s + 1)] = xb[SLOT * s:SLOT * (s + 1)]
        xs.append(x)
    return steering_table(m, res), _pack(xs)


def block_zero_mask(m):
    A, Bk = blocks_of(m)
    z = np.zeros((m, m), bool)
    z[np.ix_(A, Bk)] = True
    z[np.ix_(Bk, A)] = True
    return z


RANK_DEFICIENT = [(3, 2, 2), (4, 1, 1), (4, 2, 2), (8, 2, 3), (13, 4, 5), (16, 2, 2), (16, 4, 5)]      # (m, n, K), K < m


def rank_deficient(m, n, K, res, B, noise_free=False, pad_to=None, seed=0):
    """K < m snapshots of n emitters plus noise (42 dB down): rank K.  noise_free: K = n snapshots of the emitters alone,
    rank n, lambda_(n+1) = 0 up to rounding.  pad_to: zero snapshots appended up to that K (the same R up to a factor)."""
    if noise_free:
        K = n
    assert K < m and K >= n
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b, 3])
        x = _ordinary(rng, m, K, res, [1.0] * n, 0.0 if noise_free else 2.0 ** -7)
        if pad_to:
            x = np.concatenate([x, np.zeros((pad_to - K, m), np.complex128)])
        xs.append(x)
    return steering_table(m, res), _pack(xs)


def repeated_signal(m, res, B, K=None, seed=0):
    """n = 2, noise-free, K = m snapshots (or K given): x_k = a u_1 in even snapshots, a u_2 in odd ones, a a power of two,
    u_1 and u_2 orthogonal vectors of entries +-1 / +-i (0 on the last antenna when m is odd, which then is dead:
    a zero row and column in R).  R = c (u_1 u_1^H + u_2 u_2^H): lambda_1 = lambda_2, the other m - 2 are 0.  Exactly so
    when K is a power of two (the division by K then rounds nothing)."""
    K = m if K is None else K
    me = m - (m & 1)
    assert me >= 2 and K >= 2
    A = steering_table(m, res).astype(np.complex128)
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, b, 4])
        while True:
            u1 = np.zeros(m, np.complex128)
            u2 = np.zeros(m, np.complex128)
            u1[:me] = UNITS[rng.integers(0, 4, me)]
            sgn = np.where(np.arange(me) % 2 == 0, 1.0, -1.0)[rng.permutation(me)]    # half +1, half -1: u_1^H u_2 = 0
            u2[:me] = u1[:me] * sgn
            # no steering vector of the grid may lie in span(u_1, u_2) (on the unit square some do): the nulls stay finite
            d = m - (np.abs(A @ u1.conj()) ** 2 + np.abs(A @ u2.conj()) ** 2) / me
            if d.min() >= 1e-3 * m:
                break
        a = 2.0 ** float(rng.integers(-3, 4))
        x = np.zeros((K, m), np.complex128)
        ke = K - (K & 1)
        x[0:ke:2] = a * u1[None, :] * UNITS[rng.integers(0, 4, ke // 2)][:, None]
        x[1:ke:2] = a * u2[None, :] * UNITS[rng.integers(0, 4, ke // 2)][:, None]
        xs.append(x)
    return steering_table(m, res), _pack(xs)


def real_only(m, n, K, res, B, imag=False, seed=0):
    """All samples real (imag: all purely imaginary): n real emitters along orthogonal real vectors of norm sqrt(m) plus real
    noise; R is real symmetric, every imaginary part of it exactly 0."""
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b, 5])
        V = np.linalg.qr(rng.standard_normal((m, n)))[0] * math.sqrt(m)
        x = rng.standard_normal((K, n)) @ V.T
        x += 2.0 ** -7 * rng.standard_normal((K, m))
        xs.append(x * (1j if imag else 1.0))
    return steering_table(m, res), _pack(xs)


def imag_only(m, n, K, res, B, seed=0):
    return real_only(m, n, K, res, B, imag=True, seed=seed)


GRADES = [4.0, 3.0, 2.0, 1.5, 1.0, 0.75, 0.5, 0.375, 0.25, 0.1875, 0.125, 0.09375, 0.0625, 0.03125]


def graded(m, n, K, res, B, g, seed=0):
    """An ordinary 42 dB scene with per-antenna gains 2^-round(g k): R = D R_0 D, graded by 4^-g per antenna."""
    gain = 2.0 ** -np.round(g * np.arange(m))
    xs = []
    for b in range(B):
        rng = np.random.default_rng([seed, m, n, b, 6])
        xs.append(_ordinary(rng, m, K, res, [1.0] * n, 2.0 ** -7) * gain[None, :])
    return steering_table(m, res), _pack(xs)


def allowance(items, m, n):
    """(B,) the Davis-Kahan allowance 2 delta + delta^2 of helpers.basis_delta, and the eigenvalues (B, m) ascending"""
    from helpers import basis_delta
    w = np.linalg.eigvalsh(covariance(items, m))
    dl = basis_delta(w, m, n)
    return 2.0 * dl + dl * dl, w


def graded_g(m, n, K, res, B, seed=0):
    """the largest g of GRADES at which every item's allowance stays below 1e-6 (computed, not assumed)"""
    for g in GRADES:
        _, items = graded(m, n, K, res, B, g, seed=seed)
        if np.all(allowance(items, m, n)[0] < 1e-6):
            return g
    raise AssertionError("no grade of GRADES keeps the allowance below 1e-6 at m = %d, n = %d" % (m, n))


# ---- which scenes a shape gets ------------------------------------------------------------------------------------------------------
REGISTER = [(2, 1), (3, 2), (4, 1), (4, 2), (4, 3)]
LDS_ITER = [(5, 1), (5, 2), (6, 3), (8, 2), (8, 4), (9, 1), (13, 4), (16, 2), (16, 4)]
LDS_ONLY = [(6, 5), (16, 9)]
WIDE = [(17, 1), (24, 1), (32, 2), (40, 2), (49, 3), (50, 1), (64, 2), (64, 8)]
SHAPES = REGISTER + LDS_ITER + LDS_ONLY + WIDE
K_DEFAULT, B_DEFAULT = 48, 5
K_FUSED = 256                   # m = 4, K % 256 == 0: covariance and EVD in one kernel (cov4_evd_kernel)


def res_of(m):
    return (90, 180, 360)[m % 3]


def scene_names(m, n):
    """The scenes of a shape.  A decoupled position is left out where it cannot be built: `where` must leave at least n
    coupled antennas (the rest holds up to n emitters), and SLOT len(where) snapshots must leave room in K_DEFAULT."""
    names = []
    for pos in ("first", "first_n", "middle", "last"):
        w = where_of(pos, m, n)
        if pos == "first_n" and n == 1:
            continue                                              # the same scene as "first"
        if m - len(w) < max(n, 2) or SLOT * len(w) > K_DEFAULT // 2:
            continue
        for strength in ("weak", "between", "strong"):
            names.append("decoupled-%s-%s" % (pos, strength))
        if n == 2:
            names.append("decoupled-%s-weak-apart30" % pos)
    names += ["diagonal", "diagonal-ties", "block_diagonal", "real_only", "imag_only", "graded"]
    if n == 2:
        names.append("repeated_signal")
    if n < m - 1 and m <= 16:
        names.append("rank_deficient-noise_free")
    for (mm, nn, K) in RANK_DEFICIENT:
        if (mm, nn) == (m, n):
            names.append("rank_deficient-K%d" % K)
    return names


def make(name, m, n, res=None, B=B_DEFAULT, K=K_DEFAULT, seed=0, common_K=False):
    """(table, items, K, zero mask or None) of a named scene at a shape.  common_K: the scenes with a K of their own (diagonal,
    rank_deficient, repeated_signal) are filled up to K with zero snapshots, which leaves their structure as it is (needs K >= m)."""
    res = res_of(m) if res is None else res
    p = name.split("-")
    if common_K:
        assert K >= m
        if p[0] == "diagonal":
            t, it = diagonal(m, n, res, B, ties=(len(p) > 1), K=K, seed=seed)
            return t, it, K, diagonal_zero_mask(m)
        if p[0] == "rank_deficient":
            nf = p[1] == "noise_free"
            t, it = rank_deficient(m, n, n if nf else int(p[1][1:]), res, B, noise_free=nf, pad_to=K, seed=seed)
            return t, it, K, None
        if p[0] == "repeated_signal":
            t, it = repeated_signal(m, res, B, K=K, seed=seed)
            return t, it, K, None
    if p[0] == "decoupled":
        w = where_of(p[1], m, n)
        t, it = decoupled(m, n, K, res, B, w, p[2], apart30=(p[-1] == "apart30"), seed=seed)
        return t, it, K, decoupled_zero_mask(m, w)
    if p[0] == "diagonal":
        t, it = diagonal(m, n, res, B, ties=(len(p) > 1), seed=seed)
        return t, it, m, diagonal_zero_mask(m)
    if p[0] == "block_diagonal":
        t, it = block_diagonal(m, n, K, res, B, seed=seed)
        return t, it, K, block_zero_mask(m)
    if p[0] == "rank_deficient":
        if p[1] == "noise_free":
            t, it = rank_deficient(m, n, n, res, B, noise_free=True, seed=seed)
            return t, it, n, None
        Kd = int(p[1][1:])
        t, it = rank_deficient(m, n, Kd, res, B, seed=seed)
        return t, it, Kd, None
    if p[0] == "repeated_signal":
        assert n == 2
        t, it = repeated_signal(m, res, B, seed=seed)
        return t, it, m, None
    if p[0] in ("real_only", "imag_only"):
        t, it = real_only(m, n, K, res, B, imag=(p[0] == "imag_only"), seed=seed)
        return t, it, K, None
    if p[0] == "graded":
        g = graded_g(m, n, K, res, B, seed=seed)
        t, it = graded(m, n, K, res, B, g, seed=seed)
        return t, it, K, None
    raise KeyError(name)


MIXED = [(4, 2), (8, 2), (13, 4), (16, 2), (32, 2), (64, 2)]


def mixed_batch(m, n):
    """(table, items, kinds, K): one batch (<= 40 items) of one structured item of every kind at a common K, five ordinary
    20 dB items, a zero item and a NaN item, kinds interleaved"""
    K = 48 if m <= 48 else 64
    parts, table = [], None
    for name in scene_names(m, n):
        table, items, _, _ = make(name, m, n, B=1, K=K, common_K=True, seed=3)
        parts.append(items)
    ordinary = _pack([_ordinary(np.random.default_rng([9, m, b]), m, K, table.shape[0], [1.0] * n, 0.1) for b in range(5)])
    nan = ordinary[:1].copy()
    nan[0, 7] = complex(np.nan, 1.0)
    items = np.concatenate([ordinary] + parts + [np.zeros((1, m * K), np.complex64), nan])
    kinds = ["ordinary"] * 5 + ["structured"] * len(parts) + ["zero", "nan"]
    assert len(kinds) <= 40
    order = np.random.default_rng(m * 100 + n).permutation(len(kinds))
    return table, items[order], [kinds[i] for i in order], K


# the scenes of the wrong-subspace table: where the parent's stopping rule accepts a wrong subspace, and the control where it does not
WRONG_SUBSPACE = ([("decoupled-first-weak", m, 1) for m in (5, 9, 16, 17, 50, 64)]
                  + [("decoupled-first-weak-apart30", m, 2) for m in (8, 16, 32, 64)]
                  + [("decoupled-first_n-weak", m, 2) for m in (16, 40)]
                  + [("decoupled-last-strong", m, 1) for m in (5, 8, 16, 24)])
CONTROL = [("decoupled-last-weak", m, 1) for m in (8, 16, 32)]


# ---- the iteration of evd_sub_kernel (m <= 16) / sub_wide_kernel (m >= 17), restated --------------------------------------------------
def _mgs2(Z):
    """two-pass modified Gram-Schmidt of the columns; ok = every norm was a positive finite number"""
    Z = Z.copy()
    Y = np.zeros_like(Z)
    ok = True
    for c in range(Z.shape[1]):
        for _ in range(2):
            for c2 in range(c):
                Z[:, c] -= np.vdot(Y[:, c2], Z[:, c]) * Y[:, c2]
        n2 = float(np.sum(Z[:, c].real ** 2 + Z[:, c].imag ** 2))
        good = n2 > 0.0 and n2 < np.inf
        ok = ok and good
        Y[:, c] = Z[:, c] * (1.0 / math.sqrt(n2)) if good else 0.0
    return Y, ok


def iterate(R, n):
    """(conv, Y, steps): the kernels' orthogonal iteration on one R, from the first n columns of the scaled R."""
    R = np.array(R, dtype=np.complex128)
    m = R.shape[0]
    max_it, bail2 = (28, 0.09) if m <= 8 else (64, 0.36)
    tol2 = 1.6e-29 * n
    if not np.all(np.isfinite(R.view(np.float64))):
        return False, None, 0
    np.fill_diagonal(R, R.diagonal().real)
    dmax = float(np.abs(R.diagonal().real).max())
    if 0.0 < dmax < np.inf:
        R = R * 2.0 ** -math.frexp(dmax)[1]
    Y, ok = _mgs2(R[:, :n])
    d2prev = np.inf
    for it in range(max_it):
        if not ok:
            return False, Y, it
        Yn, ok2 = _mgs2(R @ Y)
        D = Yn - Y @ (Y.conj().T @ Yn)
        d2 = float(np.sum(D.real ** 2 + D.imag ** 2))
        ok = ok2 and d2 == d2
        Y = Yn
        if ok and d2 <= tol2:
            return True, Y, it + 1
        if it >= 2 and d2 > 100.0 * tol2 and d2 > bail2 * d2prev:
            ok = False
        d2prev = d2
    return False, Y, max_it


def dominance_check(R, Y):
    """the check after convergence: True = handed back.  max_j r_j of the deflated diagonal against min_c Theta_cc.  (The
    kernels take R Y from the step that converged, whose basis equals Y to 4e-15; here it is formed from Y itself.)"""
    R = np.array(R, dtype=np.complex128)
    dmax = float(np.abs(R.diagonal().real).max())
    if 0.0 < dmax < np.inf:
        R = R * 2.0 ** -math.frexp(dmax)[1]
    Z = R @ Y
    t = (Z * Y.conj()).real                                       # (m, n)
    return float((R.diagonal().real - t.sum(axis=1)).max()) > float(t.sum(axis=0).min())


def eigh_projector(R, n):
    w, V = np.linalg.eigh(R)
    G = V[:, :R.shape[0] - n]
    return G @ G.conj().T


def subspace_error(R, n, Y):
    """max |I - Y Y^H - P_eigh| entry-wise"""
    return float(np.abs(np.eye(R.shape[0]) - Y @ Y.conj().T - eigh_projector(R, n)).max())
