"""Every eigensolver kernel on covariances with STRUCTURE (tests/structured_scenes.py): exact zeros, diagonal and block-diagonal
R, exactly repeated eigenvalues, rank-deficient, real symmetric and graded R -- against the fp64 oracle within the project's
bounds (tests/helpers.py: min(1e-5, path term + conditioning term) for spectra, 2 delta + delta^2 for projector coefficients),
the two solvers of a shape against each other, bits independent of an item's neighbours, and crafted R through debug_evd.

The scenes with exact zeros are the ones where an orthogonal iteration started from columns of R stops on an invariant subspace
that is not the dominant one (tests/test_structured_scenes.py shows which, with the iteration restated in numpy): without the
dominance check of evd_sub_kernel / sub_wide_kernel, test_both_solvers_find_the_same_subspace fails on them with
BAZ_MUSIC_SUB_EVD=1 and passes with 0, and the oracle tests fail on the same scenes.
"""
import functools

import numpy as np
import pytest

import structured_scenes as ss
from helpers import assert_doa_within_bound, assert_spectrum_within_bound, basis_delta, oracle_fp64
from test_gpu_parity import device_run, scan_path

pytestmark = pytest.mark.gpu


def _capi():
    from gr_baz_amd import capi
    return capi


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _scene(name, m, n, fused=False):
    """(table, items, K, oracle) of a scene, computed once and shared (nothing below writes to it)"""
    table, items, K, _ = ss.make(name, m, n, K=ss.K_FUSED, common_K=True) if fused else ss.make(name, m, n)
    return table, items, K, oracle_fp64(items, table, m, n)


def _tap_q(ctx, items, m, gpu_device):
    """debug_q of a batch: (B, m, m) coefficients Q_ii, 2 Re Q_ij (i < j), -2 Im Q_ij (at [j, i])"""
    torch, capi = _torch(), _capi()
    B = items.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(items).view(np.float32)).to(gpu_device)
    Q = torch.zeros(m * m, capi.q_stride(B), dtype=torch.float64, device=gpu_device)
    torch.cuda.synchronize()
    ctx.debug_q(x.data_ptr(), B, Q.data_ptr())
    ctx.sync()
    return Q.cpu().numpy()[:, :B].T.reshape(B, m, m)


def _coefficients(P):
    """the same layout from (B, m, m) complex projectors"""
    m = P.shape[-1]
    iu = np.triu_indices(m, 1)
    C = np.zeros(P.shape, np.float64)
    C[:, np.arange(m), np.arange(m)] = P[:, np.arange(m), np.arange(m)].real
    C[:, iu[0], iu[1]] = 2.0 * P[:, iu[0], iu[1]].real
    C[:, iu[1], iu[0]] = -2.0 * P[:, iu[0], iu[1]].imag
    return C


def _coefficient_weights(m):
    w = np.full((m, m), 2.0)
    w[np.arange(m), np.arange(m)] = 1.0
    return w


# ------------------------------------------------------------------ every solver, every scene, against the oracle
def _against_the_oracle(m, n, fused, gpu_device):
    for name in ss.scene_names(m, n):
        table, items, K, (ao, lo, so, s64, w) = _scene(name, m, n, fused)
        res = table.shape[0]
        with _capi().Context(m, n, m * K, res, table) as ctx:
            if fused:
                assert "cov4_evd_kernel" in ctx.stage_name(0)
            dev = device_run(ctx, items, gpu_device)
            path = scan_path(ctx)
            host = ctx.process(items)
        for what, (ang, lvl, spec) in (("device", dev), ("host", host)):
            try:
                assert_spectrum_within_bound(spec, s64, path, m, n, table, w, what="%s %s spectrum" % (name, what))
                assert_doa_within_bound(ang, lvl, ao, s64, path, m, n, table, w)
            except AssertionError as e:
                raise AssertionError("%s, m = %d, n = %d, %s path: %s" % (name, m, n, what, e)) from None


@pytest.mark.parametrize("m,n", ss.SHAPES, ids=["m%d-n%d" % s for s in ss.SHAPES])
def test_every_solver_on_every_scene(m, n, gpu_device):
    """register Jacobi (m <= 4), LDS Jacobi with and without the iteration before it (m = 5 .. 16), the wide Jacobi and the wide
    iteration in its full and its triangular form (m >= 50): device path and host path within the bound on every scene"""
    _against_the_oracle(m, n, False, gpu_device)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fused_covariance_evd_kernel_on_every_scene(n, gpu_device):
    """m = 4 with K = 256: cov4_evd_kernel, the register Jacobi's fused twin"""
    _against_the_oracle(4, n, True, gpu_device)


# ------------------------------------------------------------------ the projector tap
TAP_SHAPES = [s for s in ss.SHAPES if s[0] <= 16]


@pytest.mark.parametrize("m,n", TAP_SHAPES, ids=["m%d-n%d" % s for s in TAP_SHAPES])
def test_projector_tap_on_every_scene(m, n, gpu_device):
    """debug_q against the eigh projector, entry by entry, within the Davis-Kahan allowance 2 delta + delta^2 of each item
    (the layout and the bound of test_stage_taps_on_every_eigensolver_branch)"""
    wts = _coefficient_weights(m)
    for name in ss.scene_names(m, n):
        table, items, K, (_, _, _, _, w) = _scene(name, m, n)
        with _capi().Context(m, n, m * K, table.shape[0], table) as ctx:
            Qg = _tap_q(ctx, items, m, gpu_device)
        R = ss.covariance(items, m)
        C = _coefficients(np.stack([ss.eigh_projector(r, n) for r in R]))
        dl = basis_delta(w, m, n)
        allow = 2.0 * dl + dl * dl
        assert np.all(allow < 1e-6)
        worst = float((np.abs(Qg - C) / (allow[:, None, None] * wts[None])).max())
        assert worst <= 1.0, "%s, m = %d, n = %d: projector error / allowance %.3g" % (name, m, n, worst)


# ------------------------------------------------------------------ both solvers of a shape, same subspace
BOTH = sorted(set(ss.LDS_ITER + ss.WIDE) | {(m, n) for _, m, n in ss.WRONG_SUBSPACE + ss.CONTROL})


@pytest.mark.parametrize("m,n", BOTH, ids=["m%d-n%d" % s for s in BOTH])
def test_both_solvers_find_the_same_subspace(m, n, gpu_device, monkeypatch):
    """the iteration with its hand-back (BAZ_MUSIC_SUB_EVD=1) and the Jacobi alone (=0): projectors to 1e-12 (m <= 16), spectra to
    2e-6 relative -- the numbers of test_signal_subspace_iteration_and_its_hand_back and its wide twin.  Every scene of the shape
    in ONE batch per K, so that the iteration's items sit between handed-back ones."""
    names = ss.scene_names(m, n)
    byK = {}
    for name in names:
        table, items, K, _ = _scene(name, m, n)
        byK.setdefault(K, []).append((name, items))
    for K, group in sorted(byK.items()):
        items = np.concatenate([it for _, it in group])
        label = [nm for nm, it in group for _ in range(it.shape[0])]
        outs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("BAZ_MUSIC_SUB_EVD", mode)
            with _capi().Context(m, n, m * K, table.shape[0], table, lab=True) as ctx:
                outs[mode] = (device_run(ctx, items, gpu_device), _tap_q(ctx, items, m, gpu_device) if m <= 16 else None)
        s1, s0 = outs["1"][0][2].astype(np.float64), outs["0"][0][2].astype(np.float64)
        bad = np.nonzero(~np.all(np.abs(s1 - s0) <= 2e-6 * np.abs(s0), axis=1))[0]
        assert bad.size == 0, "m = %d, n = %d: spectra of the two solvers differ on %s" % (m, n, sorted({label[b] for b in bad}))
        if m <= 16:
            dq = np.abs(outs["1"][1] - outs["0"][1]).reshape(items.shape[0], -1).max(axis=1)
            bad = np.nonzero(~(dq < 1e-12))[0]
            assert bad.size == 0, "m = %d, n = %d: projectors of the two solvers differ on %s (max %.3g)" % (
                m, n, sorted({label[b] for b in bad}), dq.max())


# ------------------------------------------------------------------ item independence
@pytest.mark.parametrize("m,n", ss.MIXED, ids=["m%d-n%d" % s for s in ss.MIXED])
def test_item_bits_do_not_depend_on_the_batch(m, n, gpu_device):
    """whole, permuted and one item at a time: the same bits for every item"""
    table, items, kinds, K = ss.mixed_batch(m, n)
    B = items.shape[0]
    assert B <= 40
    perm = np.random.default_rng(5).permutation(B)
    with _capi().Context(m, n, m * K, table.shape[0], table) as ctx:
        whole = device_run(ctx, items, gpu_device)
        path = scan_path(ctx)
        permuted = device_run(ctx, items[perm], gpu_device)
        single = [device_run(ctx, items[i:i + 1], gpu_device) for i in range(B)]
    for x, y in zip(whole, permuted):
        assert np.array_equal(x[perm], y, equal_nan=True)
    for i in range(B):
        for x, y in zip(whole, single[i]):
            assert np.array_equal(x[i:i + 1], y, equal_nan=True), (i, kinds[i])
    i_nan = kinds.index("nan")
    assert np.all(np.isnan(whole[2][i_nan])) and np.all(np.isfinite(np.delete(whole[2], i_nan, axis=0)))
    good = [i for i, k in enumerate(kinds) if k in ("ordinary", "structured")]
    ao, lo, so, s64, w = oracle_fp64(items[good], table, m, n)
    assert_spectrum_within_bound(whole[2][good], s64, path, m, n, table, w)
    assert_doa_within_bound(whole[0][good], whole[1][good], ao, s64, path, m, n, table, w)


# ------------------------------------------------------------------ crafted R through debug_evd (m <= 16)
CRAFTED = [(3, 2), (4, 1), (4, 2), (5, 2), (6, 5), (8, 2), (13, 4), (16, 2), (16, 9)]
SCALES = (-300, -60, 60, 300)


def _crafted(m, n):
    """[(kind, R (m, m) complex128, well posed)]: exactly diagonal in several orders (ties never across the n-th), rank one from a
    dyadic vector, block diagonal, dense (the covariance of an ordinary item), a NaN in the strict lower triangle only, +Inf on one
    diagonal entry"""
    rng = np.random.default_rng(1000 * m + n)
    e = np.concatenate([8.0 + np.arange(n), -np.arange(m - n)])
    et = e.copy()
    if n >= 2:
        et[n - 1] = et[n - 2]
    if m - n >= 2:
        et[n + 1] = et[n]
    out = []
    for ee in (e, e[::-1], rng.permutation(e), et, rng.permutation(et)):
        out.append(("diagonal", np.diag(4.0 ** ee).astype(np.complex128), True))
    v = 2.0 ** rng.integers(-3, 4, m) * ss.UNITS[rng.integers(0, 4, m)]
    out.append(("rank one", np.outer(v, v.conj()), n == 1))
    _, items, K, _ = ss.make("block_diagonal", m, n, B=2)
    for R in ss.covariance(items, m):
        out.append(("block diagonal", R, True))
    for b in range(3):
        x = ss._ordinary(np.random.default_rng([77, m, n, b]), m, 40, 90, [1.0] * n, 2.0 ** -5)
        out.append(("dense", x.T @ x.conj() / 40.0, True))
    # Hermitian bit for bit with a real diagonal, as the covariance kernels write it
    out = [(k, np.triu(R, 1) + np.triu(R, 1).conj().T + np.diag(R.diagonal().real), p) for k, R, p in out]
    dense = out[-1][1]
    low = dense.copy()
    low[m - 1, 0] = complex(np.nan, 0.0)
    out.append(("nan below the diagonal", low, False))
    inf = dense.copy()
    inf[m // 2, m // 2] = np.inf
    out.append(("inf on the diagonal", inf, False))
    return out


def _debug_evd(ctx, R, m, gpu_device):
    torch, capi = _torch(), _capi()
    B = R.shape[0]
    Rt = torch.from_numpy(np.ascontiguousarray(R.reshape(B, m * m)).view(np.float64).reshape(B, m * m, 2)).to(gpu_device)
    Q = torch.zeros(m * m, capi.q_stride(B), dtype=torch.float64, device=gpu_device)
    torch.cuda.synchronize()
    ctx.debug_evd(Rt.data_ptr(), B, Q.data_ptr())
    ctx.sync()
    return Q.cpu().numpy()[:, :B].T.reshape(B, m, m)


def _same_bits(a, b):
    """bit for bit, any NaN equal to any NaN (a poisoned item's NaN carries no promise about its payload)"""
    return np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64)) \
        and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("m,n", CRAFTED, ids=["m%d-n%d" % s for s in CRAFTED])
def test_crafted_covariances_through_the_evd_tap(m, n, gpu_device, monkeypatch):
    crafted = _crafted(m, n)
    Rs = np.stack([r for _, r, _ in crafted])
    nc = Rs.shape[0]
    ipw_jacobi = 64 if m <= 4 else 64 // m
    ipw_iter = 8 if m <= 8 else 4
    sizes = sorted({s for ipw in (ipw_jacobi, ipw_iter) for s in (1, ipw - 1, ipw, ipw + 1, 2 * ipw + 1) if s >= 1})
    big = max(max(sizes), nc)
    table = ss.steering_table(m, 90)
    warm = ss._pack([ss._ordinary(np.random.default_rng([5, b]), m, 8, 90, [1.0] * n, 0.1) for b in range(big)])
    iteration = m >= 5 and n <= 4 and 2 * n <= m
    outs = {}
    for mode in (("1", "0") if iteration else ("1",)):
        monkeypatch.setenv("BAZ_MUSIC_SUB_EVD", mode)
        with _capi().Context(m, n, m * 8, 90, table, lab=True) as ctx:
            _tap_q(ctx, warm, m, gpu_device)                       # the iteration needs the context's workspace (launch_evd_t)
            full = _debug_evd(ctx, Rs[np.arange(big) % nc], m, gpu_device)
            # an item's bits do not depend on the batch size or its place in the wave
            for i in range(nc, big):
                assert _same_bits(full[i], full[i % nc]), (mode, crafted[i % nc][0])
            for s in sizes:
                part = _debug_evd(ctx, Rs[np.arange(s) % nc], m, gpu_device)
                for i in range(s):
                    assert _same_bits(part[i], full[i % nc]), (mode, s, crafted[i % nc][0])
            # the kernels scale by an exact power of two: R 2^k gives the same bits
            for k in SCALES:
                with np.errstate(invalid="ignore"):               # (the NaN and Inf entries of the poisoned inputs)
                    scaled = Rs * 2.0 ** k
                sc = _debug_evd(ctx, scaled, m, gpu_device)
                for i in range(nc):
                    if crafted[i][0] == "inf on the diagonal":     # (no finite scale: every solver poisons the item)
                        assert np.array_equal(np.isnan(sc[i]), np.isnan(full[i]))
                    else:
                        assert _same_bits(sc[i], full[i]), (mode, k, crafted[i][0])
            outs[mode] = full[:nc]
    q1 = outs["1"]
    # well-posed inputs: the eigh projector within the allowance
    wts = _coefficient_weights(m)
    for i, (kind, R, posed) in enumerate(crafted):
        if not posed:
            continue
        Rh = R
        w = np.linalg.eigvalsh(Rh)
        dl = basis_delta(w, m, n)[0]
        allow = 2.0 * dl + dl * dl
        C = _coefficients(ss.eigh_projector(Rh, n)[None])[0]
        assert allow < 1e-6 and np.all(np.abs(q1[i] - C) <= allow * wts), (kind, float(np.abs(q1[i] - C).max()), allow)
    i_inf = [k for k, _, _ in crafted].index("inf on the diagonal")
    assert np.all(np.isnan(q1[i_inf]))
    if iteration:
        q0 = outs["0"]
        assert np.array_equal(np.isfinite(q1), np.isfinite(q0))
        posed = [i for i, c in enumerate(crafted) if c[2]]
        assert np.abs(q1[posed] - q0[posed]).max() < 1e-12
        assert not np.array_equal(q1[posed], q0[posed])            # both solvers ran: the same subspace, not the same rounding
