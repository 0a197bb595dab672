"""Shared assertions for the parity tests (tolerances are the ones BASELINE.json / SURVEY.md 8d state)."""
import numpy as np

SPECTRUM_RTOL = 1e-5   # north_star: "within 1e-5 relative float tolerance"
TIE_RTOL = 2e-5        # ang may differ only where the reference's own competing
                       # strengths differ by less than this


def assert_spectrum_close(spec, spec_ref, rtol=SPECTRUM_RTOL, what="spectrum"):
    spec = np.asarray(spec, dtype=np.float64)
    ref = np.asarray(spec_ref, dtype=np.float64)
    assert spec.shape == ref.shape, (spec.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(spec), fin), "%s: finite/non-finite pattern differs" % what
    err = np.abs(spec[fin] - ref[fin])
    bound = rtol * np.abs(ref[fin])
    worst = float(np.max(err / np.maximum(np.abs(ref[fin]), 1e-300))) if err.size else 0.0
    assert np.all(err <= bound), "%s: max relative error %.3g > %.1g" % (what, worst, rtol)
    return worst


def assert_doa_match(ang, lvl, ang_ref, lvl_ref, res, strength64=None):
    """ang/lvl: (B,n).  Bins must be identical, except where the reference's own strengths at the two
    competing bins are within TIE_RTOL of each other (then either order/bin is acceptable)."""
    ang = np.asarray(ang); ang_ref = np.asarray(ang_ref)
    assert ang.shape == ang_ref.shape
    if lvl is not None:
        assert_spectrum_close(lvl, lvl_ref, what="lvl")
    if np.array_equal(ang, ang_ref):
        return
    assert strength64 is not None, "ang differs and no fp64 strengths were supplied for tie analysis"
    B, n = ang.shape
    for b in range(B):
        for i in range(n):
            if ang[b, i] == ang_ref[b, i]:
                continue
            bin_a = int(round(float(ang[b, i]) * res / 360.0)) % res
            bin_r = int(round(float(ang_ref[b, i]) * res / 360.0)) % res
            sa, sr = strength64[b, bin_a], strength64[b, bin_r]
            assert abs(sa - sr) <= TIE_RTOL * max(abs(sa), abs(sr)), \
                "item %d slot %d: bin %d (%.6g) vs reference bin %d (%.6g) is not a tie" % (b, i, bin_a, sa, bin_r, sr)


# ---- per-path, condition-aware error bound ----------------------------------------------------------------------------------
# The helpers above hold every path to the 1e-5 project budget.  The kernels are far better than that; the bound below is what
# each of them promises, so a regression that costs a digit fails even where the budget would not notice it.
#
#   tol(item, bin) = min(SPECTRUM_RTOL, path_term + cond_term)
#
# path_term: how the path forms d = a^H P a and the float32 spectrum value 1 / d.
#   * f32 result.  Every scan stores rcp_f32((float) d) (strength_f32, music_kernels.hip.h:1329-1334; the int8 scan
#     scan_i8_kernels.hip.h:437, 465, 568): 0.5 ulp for the conversion + <= 2 ulp for v_rcp_f32.  The wide scalar scan
#     stores (float)(1 / d) (music_wide_kernels.hip.h:707-709), less.  RCP_ULPS = 3 ulp_f32, ulp_f32 = 2^-23 relative.
#   * projector and short forms in fp64 (scan_mfma_kernel; the SIG short form ||a||^2 - ||S^H a||^2; the wide scans; the
#     coarse-gated scan, whose outputs are those of scan_mfma_kernel bit for bit): absolute error ~ m^2 eps ||a||^2
#     (music_kernels.hip.h:1375-1379, baz_music_hip.hip: build_tables_device), kept only where d > refine_below = m 1e-8 max||a||^2
#     (baz_music_hip.hip: build_tables_device, baz_music_debug_host_table_image; music_wide_kernels.hip.h:697-703, 859).
#     Below it the scan recomputes the value in the reference's literal form ||G^H a||^2 (literal_tile,
#     music_kernels.hip.h:1378-1384): its rounding is that of an fp64 basis perturbed by LIT_DELTA = 4 m eps, propagated like cond_term below.
#   * int8 scan (6 <= m <= 16, n <= 4): the kept five-digit form is within 7.5e-7 of the projector form by construction
#     (scan_i8_kernels.hip.h:14-51; the seven-digit refined form is of the fp64 form's class): I8_EPS on top.
#
# cond_term: the GPU and the oracle both solve an fp64 eigenproblem of (almost) the same R.  Davis-Kahan bounds the noise
# basis' perturbation by delta = EVD_C m 2^-53 lambda_max / (lambda_{m-n} - lambda_{m-n-1}) (ascending, 0-based: the gap
# between the smallest signal and the largest noise eigenvalue).  EVD_C m units of 2^-53 lambda_max cover
#   - the covariance: two fp64 accumulations of the same K products (tap tests: <= 1e-14 max|R| entry-wise),
#   - the Jacobi stopping rule off^2 <= 1e-33 dia^2 (music_kernels.hip.h:488): < 1 unit,
#   - orthogonal iteration: an item stops when its basis moves by <= 4e-15 sqrt(n) (music_kernels.hip.h:1050,
#     music_wide_kernels.hip.h:469), i.e. <= 36 sqrt(n) units times lambda_n / gap; slower items go to the Jacobi,
#   - LAPACK's zheevd on the oracle's side (a few m units).
# The literal form d = ||G^H a||^2 then moves by |dd| <= 2 ||a|| sqrt(d) delta + ||a||^2 delta^2; relative to d that is
# cond_term (the strength 1 / d moves by the same relative amount to first order).  The looser projector-form bound
# ||a||^2 ||dP|| / d is NOT used: it is the size of the cancellation the literal-form refinement exists to remove.
ULP32 = 2.0 ** -23
EPS64 = 2.0 ** -53
RCP_ULPS = 3.0
I8_EPS = 7.5e-7                # scan_i8_kernels.hip.h:22-27 (eps of the kept bulk form)
EVD_C = 64.0                   # units of m 2^-53 lambda_max, see above
REFINE_REL = 1e-8              # refine_below = m REFINE_REL max||a||^2 (baz_music_hip.hip: build_tables_device)
TIGHT_TOL = 2e-6               # the fraction of values with tol <= this is reported (and asserted by the GPU tests)
PATHS = ("fp64", "int8")


def oracle_fp64(items, table, m, n):
    """fp64 oracle of a batch (music_oracle.music_doa_work_batch's arithmetic) plus what the bound needs:
    (ang32, lvl32, spec32, strength64, w) with w the ascending eigenvalues of each item's fp64 R."""
    items = np.asarray(items, dtype=np.complex64)
    B, N = items.shape
    K = N // m
    x = items.astype(np.complex128).reshape(B, K, m).transpose(0, 2, 1)
    R = (x @ x.conj().transpose(0, 2, 1)) / float(K)
    w, V = np.linalg.eigh(R)
    G = V[:, :, :m - n]
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    c = np.einsum("st,btk->bsk", A, G.conj())
    nrm2 = np.sum(c.real ** 2 + c.imag ** 2, axis=2)
    with np.errstate(divide="ignore"):
        strength = 1.0 / nrm2
    from oracle import music_oracle as mo
    res = A.shape[0]
    ang = np.zeros((B, n), np.float32)
    lvl = np.zeros((B, n), np.float32)
    for b in range(B):
        if np.all(np.isfinite(strength[b])):
            ang[b], lvl[b] = mo.top_n_fast(strength[b], n, res)
        else:
            a_, l_ = mo.top_n_insertion(strength[b], n, res)
            ang[b], lvl[b] = a_, l_
    return ang, lvl, strength.astype(np.float32), strength, w


def _table_norms(table):
    A = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    a2 = np.sum(A.real ** 2 + A.imag ** 2, axis=1)
    fin = a2 < 1e300
    return a2, (float(a2[fin].max()) if fin.any() else 0.0)


def basis_delta(w, m, n):
    """Davis-Kahan bound on the noise basis' fp64 perturbation, per item (inf where the gap is not positive)."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    lam_max = np.maximum(np.abs(w).max(axis=1), 0.0)
    gap = w[:, m - n] - w[:, m - n - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(gap > 0, EVD_C * m * EPS64 * lam_max / np.where(gap > 0, gap, 1.0), np.inf)
    return np.where(lam_max > 0, delta, 0.0)


def _propagate(delta, a2, d):
    """relative change of d = ||G^H a||^2 when the basis moves by delta (per value; inf where it reaches d)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        na = np.sqrt(a2)
        rel = (2.0 * na * np.sqrt(d) * delta + a2 * delta * delta) / d
        return np.where(rel < 1.0, rel / (1.0 - rel), np.inf)


def path_term(path, m, table, strength64):
    """(B, res) relative allowance of the path's own arithmetic (see the notes above)."""
    assert path in PATHS, path
    a2, amax2 = _table_norms(table)
    s = np.asarray(strength64, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / s
        below = m * REFINE_REL * amax2
        proj = m * m * EPS64 * a2[None, :] / d                                   # projector / short form, d > below
        lit = _propagate(4.0 * m * EPS64, a2[None, :], d)                        # literal form
        form = np.where(d > below, np.maximum(proj, lit), lit)
    t = RCP_ULPS * ULP32 + form
    if path == "int8":
        t = t + I8_EPS
    return t


def cond_term(m, n, table, strength64, w):
    a2, _ = _table_norms(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / np.asarray(strength64, dtype=np.float64)
    return _propagate(basis_delta(w, m, n)[:, None], a2[None, :], d)


def spectrum_bound(path, m, n, table, strength64, w):
    """(B, res) unclamped bound path_term + cond_term (compare with min(SPECTRUM_RTOL, .))."""
    return path_term(path, m, table, strength64) + cond_term(m, n, table, strength64, w)


def spectrum_tol(path, m, n, table, strength64, w):
    return np.minimum(SPECTRUM_RTOL, spectrum_bound(path, m, n, table, strength64, w))


def assert_spectrum_within_bound(spec32, strength64, path, m, n, table, w, ill_posed_ok=False, what="spectrum"):
    """spec32 (B, res) float32 against the fp64 strengths at min(SPECTRUM_RTOL, path_term + cond_term) per value.
    ill_posed_ok: values whose bound exceeds SPECTRUM_RTOL are only checked for finiteness (the oracle's own answer is not
    defined to 1e-5 there: rank-deficient R, noise eigenvalues picked as signal).
    Returns (worst err / tol, fraction of compared values with tol <= TIGHT_TOL, compared values)."""
    spec = np.asarray(spec32, dtype=np.float64)
    ref = np.asarray(strength64, dtype=np.float64)
    assert spec.shape == ref.shape, (spec.shape, ref.shape)
    fin = np.isfinite(ref)
    bound = spectrum_bound(path, m, n, table, ref, w)
    if ill_posed_ok:
        assert np.all(np.isfinite(spec) | ~fin), "%s: non-finite value where the oracle's is finite" % what
        cmp = fin & (bound <= SPECTRUM_RTOL)
    else:
        assert np.array_equal(np.isfinite(spec), fin), "%s: finite/non-finite pattern differs" % what
        cmp = fin
    tol = np.minimum(SPECTRUM_RTOL, bound)[cmp]
    err = np.abs(spec[cmp] - ref[cmp]) / np.abs(ref[cmp])
    ratio = err / tol
    worst = float(ratio.max()) if ratio.size else 0.0
    tight = float(np.mean(tol <= TIGHT_TOL)) if tol.size else 1.0
    if worst > 1.0:
        k = int(np.argmax(ratio))
        b, s = [int(v[k]) for v in np.nonzero(cmp)]
        raise AssertionError("%s (%s path): item %d bin %d: relative error %.3g > tol %.3g (err/tol %.3g; bound %.3g)"
                             % (what, path, b, s, err[k], tol[k], worst, bound[b, s]))
    return worst, tight, int(cmp.sum())


def assert_doa_within_bound(ang, lvl, ang_ref, strength64, path, m, n, table, w, ill_posed_ok=False):
    """ang/lvl (B, n) of the device against the fp64 oracle: bins identical, or a tie whose fp64 strengths differ by at most
    2 tol; lvl[i] within tol of the fp64 strength at the device's own bin.  Returns worst lvl err / tol."""
    ang = np.asarray(ang); ang_ref = np.asarray(ang_ref)
    assert ang.shape == ang_ref.shape
    s64 = np.asarray(strength64, dtype=np.float64)
    B, res = s64.shape
    bound = spectrum_bound(path, m, n, table, s64, w)
    tol = np.minimum(SPECTRUM_RTOL, bound)
    worst = 0.0
    for b in range(B):
        if not np.all(np.isfinite(s64[b])):
            continue
        if ill_posed_ok and np.any(bound[b] > SPECTRUM_RTOL):
            if lvl is not None:
                assert np.all(np.isfinite(lvl[b]))
            continue
        filled = min(n, int(np.sum(s64[b] > 0)))      # slots past the bins that beat 0.0 keep the (0, 0) of .cc:95
        for i in range(filled, n):
            assert ang[b, i] == 0.0 and ang_ref[b, i] == 0.0 and (lvl is None or lvl[b, i] == 0.0), \
                "item %d slot %d: no bin is left for it, expected (0, 0)" % (b, i)
        for i in range(filled):
            bin_a = int(round(float(ang[b, i]) * res / 360.0)) % res
            if ang[b, i] != ang_ref[b, i]:
                bin_r = int(round(float(ang_ref[b, i]) * res / 360.0)) % res
                sa, sr = s64[b, bin_a], s64[b, bin_r]
                t = max(tol[b, bin_a], tol[b, bin_r])
                assert abs(sa - sr) <= 2.0 * t * max(abs(sa), abs(sr)), \
                    "item %d slot %d: bin %d (%.9g) vs oracle bin %d (%.9g) is not a tie at tol %.3g" % (b, i, bin_a, sa, bin_r, sr, t)
            if lvl is not None and s64[b, bin_a] > 0:
                r = abs(float(lvl[b, i]) - s64[b, bin_a]) / s64[b, bin_a] / tol[b, bin_a]
                assert r <= 1.0, "lvl item %d slot %d (bin %d): err/tol %.3g" % (b, i, bin_a, r)
                worst = max(worst, r)
    return worst
