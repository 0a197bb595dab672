"""The per-path, condition-aware bound of tests/helpers.py (assert_spectrum_within_bound) on the CPU: the oracles pass it, and
it catches what the 1e-5 budget lets through -- a lost digit in d, a Jacobi stopped one sweep early, the int8 scan with one
digit fewer.  No device: the oracle and the numpy restatements of the tree only."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from helpers import (SPECTRUM_RTOL, TIGHT_TOL, assert_doa_within_bound, assert_spectrum_close, assert_spectrum_within_bound,
                     oracle_fp64, spectrum_tol)
from oracle import music_oracle as mo
from oracle import music_ref as mr


def _eigvals(items, m):
    B, N = items.shape
    x = items.astype(np.complex128).reshape(B, N // m, m).transpose(0, 2, 1)
    return np.linalg.eigvalsh(x @ x.conj().transpose(0, 2, 1) / (N // m))


def _seeded(cfg, snr, batch=24):
    c = mo.make_config(cfg, batch, snr_db=snr, seed=4242 + int(snr))
    return c["m"], c["n"], c["table"], c["items"]


# ---- the oracles pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_oracles_pass_the_bound_on_the_goldens(name):
    g = load_golden(name)
    m, n = g["m"], g["n"]
    w = _eigvals(g["items"], m)
    worst, tight, _ = assert_spectrum_within_bound(g["spectrum"], g["strength64"], "fp64", m, n, g["table"], w)
    assert tight >= 0.9
    _, _, so, s64, _ = oracle_fp64(g["items"], g["table"], m, n)
    assert_spectrum_within_bound(so, g["strength64"], "fp64", m, n, g["table"], w)
    ac, lc, sc = mr.work_batch(g["items"], g["table"], m, n)
    assert_spectrum_within_bound(sc, g["strength64"], "fp64", m, n, g["table"], w)
    assert_doa_within_bound(ac, lc, g["ang"], g["strength64"], "fp64", m, n, g["table"], w)


@pytest.mark.parametrize("snr", [10.0, 20.0, 40.0])
@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3"])
def test_oracles_pass_the_bound_on_seeded_configs(cfg, snr):
    m, n, table, items = _seeded(cfg, snr, batch=24 if cfg != "cfg3" else 6)
    ao, lo, so, s64, w = oracle_fp64(items, table, m, n)
    _, tight, _ = assert_spectrum_within_bound(so, s64, "fp64", m, n, table, w)
    assert tight >= 0.9
    ac, lc, sc = mr.work_batch(items, table, m, n)                    # the plain-C restatement, its own Jacobi
    assert_spectrum_within_bound(sc, s64, "fp64", m, n, table, w)
    assert_doa_within_bound(ac, lc, ao, s64, "fp64", m, n, table, w)


def test_the_bound_is_never_looser_than_the_budget():
    m, n, table, items = _seeded("cfg1", 0.0)
    items[:, ::3] = 0                                                 # rank-poor items too: large cond_term
    _, _, _, s64, w = oracle_fp64(items, table, m, n)
    tol = spectrum_tol("int8", m, n, table, s64, w)
    assert np.all(tol <= SPECTRUM_RTOL)


# ---- it has teeth ----------------------------------------------------------------------------------------------------------
def test_a_lost_digit_in_d_fails_the_bound_but_not_the_budget():
    """d (1 + 4e-6) on the well-conditioned bins: a regression of one digit, inside the 1e-5 budget."""
    m, n, table, items = _seeded("cfg2", 20.0)
    _, _, so, s64, w = oracle_fp64(items, table, m, n)
    tol = spectrum_tol("fp64", m, n, table, s64, w)
    well = tol <= TIGHT_TOL
    assert well.mean() > 0.9
    bad = np.where(well, s64 / (1.0 + 4e-6), s64).astype(np.float32)
    assert_spectrum_close(bad, s64)                                   # the budget does not notice
    with pytest.raises(AssertionError, match="relative error"):
        assert_spectrum_within_bound(bad, s64, "fp64", m, n, table, w)
    assert_spectrum_within_bound(so, s64, "fp64", m, n, table, w)     # (the unperturbed values pass)


def _jacobi(R, max_sweeps=64):
    """Cyclic complex Jacobi with the kernels' stopping rule (music_kernels.hip.h:479-490: stop when off^2 <= 1e-33 dia^2,
    off^2 = sum_{i<j} |A_ij|^2, dia^2 = sum_i A_ii^2); ascending eigenvalues, eigenvectors and the sweeps it took."""
    m = R.shape[0]
    A = R.copy()
    V = np.eye(m, dtype=np.complex128)
    sweeps = 0
    while sweeps < max_sweeps:
        iu = np.triu_indices(m, 1)
        off = float(np.sum(np.abs(A[iu]) ** 2))
        dia = float(np.sum(A.diagonal().real ** 2))
        if not off > 1e-33 * dia:
            break
        for p in range(m - 1):
            for q in range(p + 1, m):
                g = abs(A[p, q])
                if g == 0.0:
                    continue
                theta = (A[q, q].real - A[p, p].real) / (2.0 * g)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                ph = A[p, q] / g
                J = np.eye(m, dtype=np.complex128)
                J[p, p] = J[q, q] = c
                J[p, q] = s * ph
                J[q, p] = -s * np.conj(ph)
                A = J.conj().T @ A @ J
                V = V @ J
        sweeps += 1
    w = A.diagonal().real
    o = np.argsort(w, kind="stable")
    return w[o], V[:, o], sweeps


def _jacobi_spectra(items, table, m, n, early):
    B, N = items.shape
    K = N // m
    x = items.astype(np.complex128).reshape(B, K, m).transpose(0, 2, 1)
    A = table.astype(np.complex128)
    out = []
    for b in range(B):
        R = x[b] @ x[b].conj().T / K
        _, V, S = _jacobi(R)
        if early:
            _, V, _ = _jacobi(R, S - 1)
        c = A @ V[:, :m - n].conj()
        out.append((1.0 / np.sum(c.real ** 2 + c.imag ** 2, axis=1)).astype(np.float32))
    return np.array(out)


@pytest.mark.parametrize("m,n,snr", [(4, 2, 20.0), (6, 3, 10.0)])
def test_a_jacobi_stopped_one_sweep_early_fails(m, n, snr):
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, 360, mo.FREQUENCY, mo.SPACING)
    items = mo.synth_items(8, m, m * 64, arr, mo.FREQUENCY, mo.SPACING, angles_deg=tuple(np.linspace(30, 250, n)),
                           snr_db=snr, seed=5)
    _, _, _, s64, w = oracle_fp64(items, table, m, n)
    assert_spectrum_within_bound(_jacobi_spectra(items, table, m, n, early=False), s64, "fp64", m, n, table, w)
    early = _jacobi_spectra(items, table, m, n, early=True)
    with pytest.raises(AssertionError, match="relative error"):
        assert_spectrum_within_bound(early, s64, "fp64", m, n, table, w)
    if m == 6:
        assert_spectrum_close(early, s64)                             # ... a miss the budget does not see


def test_the_int8_scan_with_four_leading_digits_fails_the_int8_bound():
    """tests/test_i8_scan.py's restatement of the integer forms on the library's own digit images: the kernel's rule (d5 where
    it exceeds T, else the seven-digit d7) passes the int8 bound; four leading digits in place of five do not."""
    import test_i8_scan as i8
    from gr_baz_amd import capi
    m, n, K, res, B = 8, 2, 64, 200, 24
    arr = mo.array_geometry(m)
    table = mo.steering_table_c64(arr, res, mo.FREQUENCY, mo.SPACING)
    img, par = capi.debug_i8_image(m, res, table)
    Fd = i8.image_digits(img, m, res)
    items = mo.synth_items(B, m, m * K, arr, mo.FREQUENCY, mo.SPACING, snr_db=25.0, seed=39)
    _, _, _, s64, w = oracle_fp64(items, table, m, n)
    x = items.astype(np.complex128).reshape(B, K, m).transpose(0, 2, 1)
    _, V = np.linalg.eigh(x @ x.conj().transpose(0, 2, 1) / K)
    G = V[:, :, :m - n]
    q = i8.q_image(G @ G.conj().transpose(0, 2, 1))
    d5, d7, d4 = i8._integer_forms(i8.digits(i8.fixed(q, par["sq"])), Fd, par["wt"])
    kernel = np.where(d5 > par["t_acc"], d5, d7)
    assert_spectrum_within_bound((1.0 / kernel).astype(np.float32), s64, "int8", m, n, table, w)
    four = np.where(d4 > par["t_acc"], d4, d7)
    with pytest.raises(AssertionError, match="relative error"):
        assert_spectrum_within_bound((1.0 / four).astype(np.float32), s64, "int8", m, n, table, w)
