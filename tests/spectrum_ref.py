"""numpy restatement of the opt-in Capon and Bartlett spectrum estimators (baz_music_set_estimator, include/baz_music_hip.h;
DESIGN.md 8i).  R is read as the power mode reads it: the lower triangle as stored, the imaginary part of the diagonal ignored.

    Capon     P_C(b) = power_ref.power(R, row b): the unpivoted LDL^H, the pivot-floor degeneracy rule (a degenerate item's whole
              row is 0), s -> P with 0 for an s that is 0 or not finite.
    Bartlett  P_B(b) = q / (w w),  w = sum_i |a_i|^2,
              y_i = sum_{j<i} R_ij a_j + Re(R_ii) a_i + sum_{j>i} conj(R_ji) a_j,  q = sum_i Re(conj(a_i) y_i),
              all sums in index order; 0 when w == 0 or when q or w is not finite.

capon / bartlett run the loops of the definition over i, j, k with the table's rows as the vector axis: the same operations per row
in the same order (numpy's vector loops may fuse a multiply-add where its scalar path does not, so capon agrees with
power_ref.power to an ulp or so of fp64, not bit for bit); capon_solve / bartlett_matmul are the independent np.linalg forms.
"""
import numpy as np

import power_ref as pr

MUSIC, CAPON, BARTLETT = 0, 1, 2


def capon(R, rows):
    """P_C (count,) float64 for one R (m, m) and steering rows (count, m) complex64: power_ref.power with the rows as the vector axis."""
    R = np.asarray(R, dtype=np.complex128)
    m = R.shape[0]
    rows = np.asarray(rows, dtype=np.complex64).reshape(-1, m)
    out = np.zeros(rows.shape[0], np.float64)
    f = pr.ldl(R)
    if f is None:
        return out
    L, d = f
    a = rows.astype(np.complex128)
    with np.errstate(all="ignore"):
        z = np.zeros_like(a)
        s = np.zeros(rows.shape[0], np.float64)
        for i in range(m):
            zi = a[:, i].copy()
            for k in range(i):
                zi = zi - L[i, k] * z[:, k]
            z[:, i] = zi
            s = s + (zi.real * zi.real + zi.imag * zi.imag) / d[i]
        good = np.isfinite(s) & (s != 0.0)
        out[good] = 1.0 / s[good]
    return out


def bartlett(R, rows):
    """P_B (count,) float64 for one R (m, m) and steering rows (count, m) complex64, by the loop of the definition."""
    R = np.asarray(R, dtype=np.complex128)
    m = R.shape[0]
    rows = np.asarray(rows, dtype=np.complex64).reshape(-1, m)
    a = rows.astype(np.complex128)
    with np.errstate(all="ignore"):
        w = np.zeros(rows.shape[0], np.float64)
        for i in range(m):
            w = w + (a[:, i].real * a[:, i].real + a[:, i].imag * a[:, i].imag)
        q = np.zeros(rows.shape[0], np.float64)
        for i in range(m):
            y = np.zeros(rows.shape[0], np.complex128)
            for j in range(m):
                if j < i:
                    y = y + R[i, j] * a[:, j]
                elif j == i:
                    y = y + R[i, i].real * a[:, j]
                else:
                    y = y + np.conj(R[j, i]) * a[:, j]
            q = q + (a[:, i].real * y.real + a[:, i].imag * y.imag)
        good = np.isfinite(q) & np.isfinite(w) & (w != 0.0)
        out = np.zeros(rows.shape[0], np.float64)
        out[good] = q[good] / (w[good] * w[good])
    return out


def spectrum(kind, R, table):
    """(B, res) float64 spectra for covariances R (B, m, m) and the table (res, >= m) complex64 (its first m columns are used)."""
    R = np.asarray(R)
    m = R.shape[-1]
    rows = np.asarray(table)[:, :m]
    fn = {CAPON: capon, BARTLETT: bartlett}[kind]
    return np.stack([fn(Rb, rows) for Rb in R.reshape(-1, m, m)])


def capon_solve(R, rows):
    """The independent form of Capon: np.linalg.solve (no degeneracy rule)."""
    return pr.solve(R, rows)


def bartlett_matmul(R, rows):
    """The independent form of Bartlett: Re(a^H H a) / (a^H a)^2 with H the Hermitian matrix the definition sees."""
    H = pr.hermitian_from_lower(R)
    a = np.asarray(rows, dtype=np.complex64).astype(np.complex128).reshape(-1, H.shape[0])
    q = np.real(np.einsum("em,mk,ek->e", np.conj(a), H, a))
    w = np.real(np.einsum("em,em->e", np.conj(a), a))
    return q / (w * w)


def ulp_distance_f32(x, y):
    """Distance in float32 units in the last place between two float32 arrays of equal sign and finite values (as ordered ints)."""
    xi = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    yi = np.ascontiguousarray(y, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(xi - yi)
