// refine_kernels.hip.h -- the opt-in sub-bin angle refinement (baz_music_set_refine_mode, include/baz_music_hip.h):
// a parabola through the MUSIC denominator d = ||G^H a||^2 at a reported bin and its two neighbours on the circle.
//
//   refine_decide     the decision rule (p, q, delta), __host__ __device__: refine_kernel calls it with the three fp64 values it has
//                     just formed, baz_music_refine_estimate() compiles the same text for the host, so the rule is testable
//                     without a device.
//   refine_angle      (bin, delta) -> the float angle, the wrap and the cast included; __host__ __device__ as well.
//   refine_kernel     one thread per reported (item, slot) entry, after the top-n merge / the peak picker / the count truncation.
//
// DEFINITION.  y-, y0, y+ = d at bins b - 1, b, b + 1 (mod res), fp64.  p = y- - y0, q = y+ - y0,
//     delta = (p - q) / (2 (p + q))   if p >= 0, q >= 0, p + q > 0 and the three values are finite,   else 0
// (|delta| <= 1/2), ang = (float)(((b + delta) mod res) 360 / res) in fp64, a result that rounds to 360.0f stored as 0.0f.  delta = 0
// reproduces the bits of the unrefined ang.  The fit is on d, not on the spectrum 1 / d (a Lorentzian near a null).
//
// THE THREE VALUES are formed as the exact fp64 scan forms a value: the projector form a^H Q a from the item's coefficients
// (Qs[e*qstride + item], the layout of evd_finish), and the reference's literal form ||G^H a||^2 from the item's noise vectors where
// the projector form is at or below `below` (ScanRefine of music_kernels.hip.h).  Where the context's scan runs its short form no
// projector coefficients are written (Qs == nullptr): the literal form is then taken for all three.  Steering rows come from the
// plain raw image of the TableSet in force (L2 resident), never from the upload staging buffer.
//
// ACCESS PATTERN.  Threads are entry-minor: the n threads of an item sit next to each other, consecutive items follow, so a
// coefficient load Qs[e*qstride + item] of a wave touches 64 / n consecutive doubles (one or two 128-B lines) and the ang / lvl /
// offset stores are unit-stride.  A thread's three steering rows are m contiguous complex64 each, held in registers;
// every coefficient is loaded once and feeds the three accumulators.  Entries are read from a device-side
// staging copy the pickers wrote and the results go to the caller's buffers with plain stores -- nothing is read back from the
// caller's (possibly host-mapped) memory.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capon_solve.hip.h"

namespace bazrefine {

// the rule: y[0] = d(b - 1), y[1] = d(b), y[2] = d(b + 1)
__host__ __device__ inline double refine_decide(const double ym, const double y0, const double yp)
{
    const double inf = __builtin_huge_val();
    const bool finite = (ym - ym == 0.0) && (y0 - y0 == 0.0) && (yp - yp == 0.0) && ym < inf && y0 < inf && yp < inf;
    if (!finite) return 0.0;
    const double p = ym - y0, q = yp - y0;
    const double s = p + q;
    if (!(p >= 0.0 && q >= 0.0 && s > 0.0)) return 0.0;      // a flank or a plateau
    const double r = (p - q) / (2.0 * s);
    return (r - r == 0.0) ? r : 0.0;                         // (p + q overflowed: p, q ~ 1e308)
}

// ang of bin b moved by delta bins, in fp64; (b + delta) < 0 only at b = 0: one turn is added
__host__ __device__ inline float refine_angle(const uint32_t b, const double delta, const uint32_t res)
{
    double t = (double)b + delta;
    if (t < 0.0) t = t + (double)res;
    const float a = (float)(t * 360.0 / (double)res);
    return a >= 360.0f ? 0.0f : a;
}

struct RefineArgs {
    const float* ang_in;       // [batch * n] what the merge / picker / truncation left (device staging)
    const float* lvl_in;       // [batch * n] ... lvl != 0 marks a real entry (1 / d > 0; a missing one is (0, 0))
    float* ang_out;            // [batch * n] the caller's ang
    float* lvl_out;            // [batch * n] the caller's lvl, or nullptr (port 1 not wired): the staged bits, untouched
    double* off_out;           // [batch * n] delta per entry (baz_music_last_refine_offsets)
    const double* Qs;          // projector coefficients, item-minor; nullptr: literal form throughout
    const double* Gs;          // noise vectors, [((k*M + i)*2 + re/im) * qstride + item], `rows` of them per item
    const float2* raw;         // the raw table in force, [res][m] complex64
    double below;              // projector value at or below this -> literal form (negative: never)
    uint32_t batch, n, res, qstride, rows;
};

template <int M>
__global__ __launch_bounds__(256) void refine_kernel(const RefineArgs A)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)A.batch * A.n) return;
    const uint32_t it = (uint32_t)(t / A.n);
    const float a_in = A.ang_in[t], l_in = A.lvl_in[t];
    if (A.lvl_out) A.lvl_out[t] = l_in;
    if (l_in == 0.0f) {                                      // a missing entry stays (0, 0)
        A.ang_out[t] = a_in;
        A.off_out[t] = 0.0;
        return;
    }
    const uint32_t b = bazcapon::staged_bin(a_in, A.res);
    const uint32_t bm = b == 0u ? A.res - 1u : b - 1u, bp = b + 1u == A.res ? 0u : b + 1u;
    // the three steering rows (kept as the table's floats; widened exactly where used, .cc:110-112)
    float2 a[3][M];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float2* __restrict__ row = A.raw + (size_t)(k == 0 ? bm : (k == 1 ? b : bp)) * M;
#pragma unroll
        for (int i = 0; i < M; ++i) a[k][i] = row[i];
    }
    double y[3] = {0.0, 0.0, 0.0};
    bool literal = A.Qs == nullptr;
    if (!literal) {
        // a^H Q a = sum_e q[e] F[e]:  e = i*M+i: |a_i|^2;  e = i*M+j (i < j): Re conj(a_i) a_j;  e = j*M+i: Im conj(a_i) a_j
        // (every coefficient is loaded once and feeds the three accumulators)
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const double qii = A.Qs[(size_t)(i * M + i) * A.qstride + it];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double xr = (double)a[k][i].x, xi = (double)a[k][i].y;
                y[k] += qii * (xr * xr + xi * xi);
            }
#pragma unroll
            for (int j = i + 1; j < M; ++j) {
                const double qre = A.Qs[(size_t)(i * M + j) * A.qstride + it];
                const double qim = A.Qs[(size_t)(j * M + i) * A.qstride + it];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double xr = (double)a[k][i].x, xi = (double)a[k][i].y, zr = (double)a[k][j].x, zi = (double)a[k][j].y;
                    y[k] += qre * (xr * zr + xi * zi);
                    y[k] += qim * (xr * zi - xi * zr);
                }
            }
        }
        literal = fabs(y[0]) <= A.below || fabs(y[1]) <= A.below || fabs(y[2]) <= A.below;
    }
    if (literal) {                                           // ||G^H a||^2, c_r = sum_i conj(G_ir) a_i (.cc:110-121)
        double l[3] = {0.0, 0.0, 0.0};
        for (uint32_t r = 0; r < A.rows; ++r) {
            double cr[3] = {0.0, 0.0, 0.0}, ci[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const double gr = A.Gs[(size_t)((r * M + i) * 2) * A.qstride + it];
                const double gi = A.Gs[(size_t)((r * M + i) * 2 + 1) * A.qstride + it];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double xr = (double)a[k][i].x, xi = (double)a[k][i].y;
                    cr[k] += gr * xr + gi * xi;
                    ci[k] += gr * xi - gi * xr;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) l[k] += cr[k] * cr[k] + ci[k] * ci[k];
        }
        // per VALUE, like the scan: only a value at or below the threshold is replaced
#pragma unroll
        for (int k = 0; k < 3; ++k) y[k] = (A.Qs == nullptr || fabs(y[k]) <= A.below) ? l[k] : y[k];
    }
    const double delta = refine_decide(y[0], y[1], y[2]);
    A.ang_out[t] = delta == 0.0 ? a_in : refine_angle(b, delta, A.res);
    A.off_out[t] = delta;
}

}  // namespace bazrefine
