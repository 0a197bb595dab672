// whiten_kernels.hip.h -- the opt-in noise pre-whitening (baz_music_set_noise_covariance, include/baz_music_hip.h): with a
// known or measured noise covariance Rn = L L^H and W = L^-1 (lower triangular, real positive diagonal, factored on the host) the EVD
// decomposes R' = W R W^H and the table in force becomes a' = W a.
//
//   whiten_fma           acc += w x of two complex numbers as four fused multiply-adds in one order, __host__ __device__: the one
//                        piece of arithmetic every routine below is made of.
//   whiten_entry         one entry of the whitened table, __host__ __device__: table_whiten_kernel and baz_music_whiten_table() run the
//                        same text, so the rule is testable without a device (as calib_mul is).
//   table_whiten_kernel  the raw table from the page-locked staging copy, times gamma where a calibration is on, times W, into dRaw:
//                        takes the place of the first copy_words_kernel / table_calib_kernel launch of build_tables_device.
//   whiten_kernel<M>     R' of a batch at 2 <= M <= 16 antennas, one item per group of 4 / 8 / 16 lanes.
//   whiten_wide_kernel   one "left-multiply by W" pass at a run-time m (17 .. 64), launched twice: R' = W (W R)^H.
//
// DEFINITION (table).  a'_r(b) = fl32(sum_{k <= r} W_rk a~_k(b)), a~ the table entry after calibration (calib_mul), widened exactly;
// the sum starts from (+0, +0) and takes k ascending, each term by whiten_fma; one round-to-nearest conversion per component.
//
// DEFINITION (covariance).  R is read as the Hermitian matrix its lower triangle describes: R_kj = the stored (k, j) for k > j,
// conj of the stored (j, k) for k < j, (Re of the stored (j, j), 0) on the diagonal.  T_rj = sum_{k <= r} W_rk R_kj and then, for r >= j,
// R'_rj = sum_{k <= r} W_rk conj(T_jk) (= (T W^H)_rj of a Hermitian R'), both from (+0, +0) with k ascending by whiten_fma.
// The upper triangle is written as the conjugate of the lower one and the diagonal's imaginary part as +0.  Every kernel evaluates
// these same two chains, so the bits of R' do not depend on which of them ran; an item touches no other item's data.
//
// LAYOUT (whiten_kernel).  Lane j of an item's group first holds COLUMN j of R (lower part: a strided gather; upper part: its own
// row, conjugated), so column j of T needs nothing from another lane; W sits in LDS and is read at workgroup-uniform addresses (a
// broadcast).  The group then turns T over through LDS (column in, row out; rows padded by one entry) and lane j computes column j of
// the lower triangle of R'.  Everything is unrolled at compile time: registers, no scratch.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "calib_kernels.hip.h"

namespace bazwhiten {

__host__ __device__ inline void whiten_fma(const double wr, const double wi, const double xr, const double xi, double& re, double& im)
{
    re = fma(wr, xr, re);
    re = fma(-wi, xi, re);
    im = fma(wr, xi, im);
    im = fma(wi, xr, im);
}

// wrow: row r of W, entries k = 0 .. r consecutive; a: the (calibrated) table row of one bin
__host__ __device__ inline void whiten_entry(const double2* wrow, const float2* a, const uint32_t r, float* o_re, float* o_im)
{
    double re = 0.0, im = 0.0;
    for (uint32_t k = 0; k <= r; ++k) whiten_fma(wrow[k].x, wrow[k].y, (double)a[k].x, (double)a[k].y, re, im);
    *o_re = (float)re;
    *o_im = (float)im;
}

constexpr int WHITEN_THREADS = 256;

// the lower triangle of the m x m row-major W, packed (row r at r (r + 1) / 2), into LDS; the caller synchronises
__device__ inline void stage_triangle(const double2* __restrict__ W, const uint32_t m, double2* sw)
{
    for (uint32_t e = threadIdx.x; e < m * m; e += blockDim.x) {
        const uint32_t r = e / m, k = e - r * m;
        if (k <= r) sw[r * (r + 1) / 2 + k] = W[e];
    }
}

// dst[b][r] = whiten_entry of the row src[b][.] (times gamma first where calib_on) for a [res][m] table.  Dynamic LDS:
// m (m + 1) / 2 double2.  Grid: any number of workgroups (each takes whole bins, 256 / m at a time).  `src` may be page-locked host
// memory addressed over the link (see copy_words_kernel): every entry is read once.
__global__ __launch_bounds__(WHITEN_THREADS) void table_whiten_kernel(const float2* __restrict__ src, float2* __restrict__ dst, const uint32_t res,
                                                                       const uint32_t m, const double2* __restrict__ W, const int calib_on,
                                                                       const bazcalib::CalibGamma gamma)
{
    extern __shared__ double2 sw[];
    __shared__ float2 sa[WHITEN_THREADS];
    __shared__ float2 sg[BAZ_CALIB_MAX_M];
    if (threadIdx.x < BAZ_CALIB_MAX_M) sg[threadIdx.x] = gamma.g[threadIdx.x];
    stage_triangle(W, m, sw);
    __syncthreads();
    const uint32_t bps = WHITEN_THREADS / m;               // whole bins per step
    const uint32_t bl = threadIdx.x / m, r = threadIdx.x - bl * m;
    for (uint32_t b0 = blockIdx.x * bps; b0 < res; b0 += gridDim.x * bps) {      // (workgroup-uniform: the barriers below are safe)
        const uint32_t nb = res - b0 < bps ? res - b0 : bps;
        const bool mine = bl < nb;
        const size_t i = (size_t)b0 * m + threadIdx.x;
        if (mine) {
            float2 a = src[i];
            if (calib_on) {
                const float2 g = sg[r];
                float2 o;
                bazcalib::calib_mul(g.x, g.y, a.x, a.y, &o.x, &o.y);
                a = o;
            }
            sa[threadIdx.x] = a;
        }
        __syncthreads();
        if (mine) {
            float2 o;
            whiten_entry(sw + r * (r + 1) / 2, sa + bl * m, r, &o.x, &o.y);
            dst[i] = o;
        }
        __syncthreads();
    }
}

template <int M>
struct WhitenGeom {
    static constexpr int GS = M <= 4 ? 4 : (M <= 8 ? 8 : 16);      // lanes per item
    static constexpr int THREADS = 64;
    static constexpr int IPB = THREADS / GS;                       // items per workgroup
};

// Rout[item] = W Rin[item] W^H for `batch` items of M x M complex128, row-major; W: M x M row-major (the upper triangle is not read).
// Grid: ceil(batch / IPB) workgroups of one wave.  Rin and Rout do not overlap.
template <int M>
__global__ __launch_bounds__(64) void whiten_kernel(const double2* __restrict__ Rin, double2* __restrict__ Rout, const double2* __restrict__ W,
                                                    const uint32_t batch)
{
    constexpr int GS = WhitenGeom<M>::GS, IPB = WhitenGeom<M>::IPB;
    __shared__ double2 sw[M * M];
    __shared__ double2 st[IPB][M][M + 1];
    for (int e = threadIdx.x; e < M * M; e += 64) sw[e] = W[e];
    __syncthreads();
    const int g = threadIdx.x / GS, j = threadIdx.x % GS;
    const uint32_t item = blockIdx.x * IPB + g;
    const bool live = item < batch && j < M;
    if (live) {
        const double2* __restrict__ R = Rin + (size_t)item * (M * M);
        double2 col[M];                                      // column j of the Hermitian matrix the lower triangle describes
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const double2 v = R[k < j ? j * M + k : k * M + j];
            col[k] = make_double2(v.x, k < j ? -v.y : (k == j ? 0.0 : v.y));
        }
#pragma unroll
        for (int r = 0; r < M; ++r) {                        // T_rj, straight into the turn-over buffer
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int k = 0; k <= r; ++k) {
                const double2 w = sw[r * M + k];
                whiten_fma(w.x, w.y, col[k].x, col[k].y, re, im);
            }
            st[g][r][j] = make_double2(re, im);
        }
    }
    __syncthreads();
    if (live) {
        double2* __restrict__ O = Rout + (size_t)item * (M * M);
        double2 row[M];                                      // row j of T
#pragma unroll
        for (int k = 0; k < M; ++k) row[k] = st[g][j][k];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            if (r < j) continue;
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int k = 0; k <= r; ++k) {
                const double2 w = sw[r * M + k];
                whiten_fma(w.x, w.y, row[k].x, -row[k].y, re, im);
            }
            if (r == j) {
                O[j * M + j] = make_double2(re, 0.0);
            } else {
                O[r * M + j] = make_double2(re, im);
                O[j * M + r] = make_double2(re, -im);
            }
        }
    }
}

// One "left-multiply by W" pass at a run-time m: s(r, j) = sum_{k <= r} W_rk in(k, j).
//   FIRST   in = R read as the Hermitian matrix its lower triangle describes; out = (W R)^H, every entry: out[j][r] = conj(s).
//   !FIRST  in = (W R)^H as the first pass left it; out = R': s for r >= j, its conjugate above, +0 as the diagonal's imaginary part.
// One workgroup per item, W's packed triangle in dynamic LDS (m (m + 1) / 2 double2: 33 KiB at m = 64); the item streams from L2 with
// unit stride across the lanes (consecutive lanes: consecutive j).  `in` and `out` do not overlap.
template <bool FIRST>
__global__ __launch_bounds__(WHITEN_THREADS) void whiten_wide_kernel(const double2* __restrict__ in, double2* __restrict__ out,
                                                                      const double2* __restrict__ W, const uint32_t m)
{
    extern __shared__ double2 sw[];
    stage_triangle(W, m, sw);
    __syncthreads();
    const double2* __restrict__ A = in + (size_t)blockIdx.x * m * m;
    double2* __restrict__ O = out + (size_t)blockIdx.x * m * m;
    for (uint32_t e = threadIdx.x; e < m * m; e += WHITEN_THREADS) {
        const uint32_t r = e / m, j = e - r * m;
        if (!FIRST && r < j) continue;
        const double2* wrow = sw + r * (r + 1) / 2;
        double re = 0.0, im = 0.0;
        for (uint32_t k = 0; k <= r; ++k) {
            double2 a;
            if (FIRST) {
                const double2 v = A[k < j ? j * m + k : k * m + j];
                a = make_double2(v.x, k < j ? -v.y : (k == j ? 0.0 : v.y));
            } else {
                a = A[k * m + j];
            }
            whiten_fma(wrow[k].x, wrow[k].y, a.x, a.y, re, im);
        }
        if (FIRST) {
            O[j * m + r] = make_double2(re, -im);
        } else if (r == j) {
            O[e] = make_double2(re, 0.0);
        } else {
            O[e] = make_double2(re, im);
            O[j * m + r] = make_double2(re, -im);
        }
    }
}

}  // namespace bazwhiten
