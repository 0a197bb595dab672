// order_kernels.hip.h -- the opt-in per-item emitter-count estimate (baz_music_set_order_mode, include/baz_music_hip.h;
// DESIGN.md 8c): the information-theoretic criteria of Wax & Kailath (MDL, AIC) on the eigenvalues of an item's covariance.
//
//   order_decide          the decision routine, __host__ __device__: the Jacobi epilogues of music_kernels.hip.h call it with the
//                         eigenvalues they hold (registers at m <= 4, the LDS diagonal from 5 antennas on), and
//                         baz_music_order_estimate() compiles the same text for the host, so the rule is testable without a device.
//   order_truncate_kernel (0, 0) in the output pairs at or beyond an item's count, after the top-n merge / the peak picker.
//
// DEFINITION.  N snapshots, eigenvalues l_1 <= ... <= l_m, clamped l_i <- max(l_i, 2^-40 l_m).  For k = 0 .. n_max over the
// m - k smallest:   L(k) = -N (m - k) (mean(ln l) - ln(mean l))
//     MDL(k) = L(k) + 1/2 k (2m - k) ln N          AIC(k) = 2 L(k) + 2 k (2m - k)
// and the count is the smallest k that minimises the criterion.  All in fp64.  l_m <= 0, NaN or Inf (a zero or non-finite
// covariance) gives 0.  The criterion is invariant under l -> s l, so the power-of-two scaling of the Jacobi kernels does not
// matter.  Cost: m logarithms, two running sums, n_max + 1 criterion values with one logarithm each.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bazorder {

constexpr int CRIT_MDL = 1, CRIT_AIC = 2;

// MT > 0: m known at compile time -- every loop unrolls and `lam` is only ever called with constants (register-resident
// eigenvalues, m <= 4); MT == 0: run-time m.  lam(i) = the i-th eigenvalue in ASCENDING order.
template <int MT, class Lam>
__host__ __device__ inline int order_decide(const int m_rt, const int nmax, const double nsnap, const int crit, Lam lam)
{
    const int m = MT > 0 ? MT : m_rt;
    const double lmax = lam(m - 1);
    if (!(lmax > 0.0) || !(lmax < __builtin_huge_val())) return 0;
    const double floor_l = lmax * 0x1p-40;
    const double lnN = log(nsnap);
    double s_ln = 0.0, s_l = 0.0, best = 0.0;
    int khat = 0;
    bool have = false;
    // the m - k smallest eigenvalues are a prefix: walking i upwards visits k = m - 1 - i downwards, and `<=` lets the smaller
    // k win a tie
#pragma unroll
    for (int i = 0; i < (MT > 0 ? MT : m); ++i) {
        double l = lam(i);
        l = l > floor_l ? l : floor_l;           // (also replaces a NaN below a finite l_m)
        s_ln += log(l);
        s_l += l;
        const int k = m - 1 - i;
        if (k <= nmax) {
            const double p = (double)(i + 1);
            const double ll = -nsnap * p * (s_ln / p - log(s_l / p));
            const double dof = (double)(k * (2 * m - k));
            const double v = (crit == CRIT_AIC) ? 2.0 * ll + 2.0 * dof : ll + 0.5 * dof * lnN;
            if (!have || v <= best) { best = v; khat = k; have = true; }
        }
    }
    return khat;
}

// ang / lvl entries at or beyond the item's count become (0, 0).  One thread per (item, entry); plain vector stores.
__global__ __launch_bounds__(256) void order_truncate_kernel(float* __restrict__ ang, float* __restrict__ lvl,
                                                             const uint8_t* __restrict__ ord, uint32_t batch, uint32_t n)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch * n) return;
    const uint32_t it = t / n, i = t - it * n;
    if (i >= (uint32_t)ord[it]) {
        ang[t] = 0.0f;
        if (lvl) lvl[t] = 0.0f;
    }
}

}  // namespace bazorder
