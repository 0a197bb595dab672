// spectrum_kernels.hip.h -- the opt-in Capon and Bartlett spectrum estimators (baz_music_set_estimator, include/baz_music_hip.h;
// DESIGN.md 8i): a power for EVERY bin of EVERY item from the item's covariance R and the raw table in force, no eigendecomposition.
//
//   spectrum_scan_kernel<M, KIND>        the scan: (float)P(b) for every (item, bin) into the spectrum (port 2 or the private one).
//   topn_spec_kernel<NMAX>               the reference's top-n rule on a float32 spectrum row, one wave per item (peak mode 0; peak
//                                        mode 1 runs bazmusic::peak_pick_kernel on the same row).
//   bartlett_host                        the Bartlett definition on the host, loop for loop (baz_music_spectrum_estimate).
//
// DEFINITION.  R is taken as the power mode takes it (capon_solve.hip.h): the lower triangle as stored, the imaginary part of the
// diagonal ignored; a = row b of the table, complex64 widened exactly.
//   Capon     P_C(b) = 1 / s,  s = sum_i |z_i|^2 / d_i from the unpivoted LDL^H of capon_solve.hip.h, the same degeneracy rule (a
//             degenerate item's whole row is 0) and the same s -> P step (power_from_s: s == 0 or not finite gives 0).
//   Bartlett  P_B(b) = q / (w w),  w = sum_i |a_i|^2,  q = Re(a^H R a);  0 when w == 0 or q or w is not finite.
// The criterion on the device is the float32 output: any fp64 evaluation is good to ~8 m cond 2^-52, so the forms below differ from
// the host's only where a float32 rounding boundary falls between them (one ulp_f32).  Here: s multiplies by 1 / d_i instead of
// dividing, and q = sum_i (Re R_ii |a_i|^2 + 2 Re(conj(a_i) sum_{j<i} R_ij a_j)) runs over the lower triangle only.  Every operation
// commutes with a power-of-two scale of R, so R -> 4R gives 4P bit for bit.
//
// LAYOUT.  A 256-thread workgroup takes IG = 256 / W consecutive items (W = 4 / 8 / 16 lanes per item for M <= 4 / 8 / 16, the groups
// of capon_kernel) and a range of bins (a multiple of 256).
//   phase 1   lane r of a group holds row r of its item's R and runs capon_kernel's column-by-column factorisation (the same text:
//             the same d, L and alive bits as the power mode); the strict lower triangle of L (packed, M (M-1) / 2 complex128), 1 / d
//             and the alive flag go to LDS.  Bartlett stores the strict lower triangle of R and the real diagonal instead.
//   phase 2   lane t takes bin range_start + 256 p + t of pass p: its table row once into registers (M complex64), then a loop over
//             the group's items: the forward substitution with L read from LDS at an address the whole workgroup shares (identical
//             addresses broadcast: no bank conflict), fully unrolled, z in registers; one float store per (item, bin), consecutive
//             lanes on consecutive bins (a wave writes a 256-byte run).
// An item beyond the batch is never looped over; a degenerate item and a lane beyond `res` run the same instructions and differ only
// in what they store.  Every word of the spectrum of every item of the batch is written.  gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capon_solve.hip.h"
#include "music_kernels.hip.h"

namespace bazspectrum {

enum { KIND_CAPON = 1, KIND_BARTLETT = 2 };     // BAZ_MUSIC_ESTIMATOR_CAPON / _BARTLETT

struct SpectrumArgs {
    const double2* R;          // [batch][M][M] the covariances (plain, or averaged), row-major
    const float2* raw;         // the raw table in force, [res][M] complex64
    float* spec;               // [batch][res]
    double rel_floor;          // BAZ_MUSIC_POWER_PIVOT_FLOOR
    uint32_t batch, res;
    uint32_t nranges;          // bin ranges per item group (grid = groups * nranges)
    uint32_t range_bins;       // bins per range, a multiple of 256
};

template <int M>
struct ScanGeom {
    static constexpr int W = bazcapon::Group<M>::W;             // lanes per item in phase 1
    static constexpr int IG = 256 / W;                          // items per workgroup
    static constexpr int TRI = M * (M - 1) / 2;                 // strict lower triangle
};

// q / (w w) with the definition's zero rule
__host__ __device__ inline double bartlett_from_qw(const double q, const double w)
{
    if (w == 0.0 || !(q - q == 0.0) || !(w - w == 0.0)) return 0.0;
    return q / (w * w);
}

template <int M, int KIND>
__global__ __launch_bounds__(256) void spectrum_scan_kernel(const SpectrumArgs A)
{
    using bazcapon::group_bcast;
    constexpr int W = ScanGeom<M>::W, IG = ScanGeom<M>::IG, TRI = ScanGeom<M>::TRI;
    __shared__ double2 sL[IG * TRI];                                        // L_ik (Bartlett: R_ik), i > k, at i (i - 1) / 2 + k
    __shared__ double sD[IG * M];                                           // 1 / d_i (Bartlett: Re R_ii)
    __shared__ int sAlive[IG];
    const uint32_t grp = blockIdx.x / A.nranges, range = blockIdx.x % A.nranges;
    const uint64_t item0 = (uint64_t)grp * IG;
    // ---- phase 1: one item per group of W lanes (capon_kernel's factorisation) ----
    {
        const uint32_t r = threadIdx.x % W, g = threadIdx.x / W;            // this lane's row, this group's item
        const uint64_t item = item0 + g;
        const bool live = item < A.batch;
        const bool rowlane = live && r < (uint32_t)M;
        double lr[M], li[M];
        {
            const double2* __restrict__ row = A.R + ((size_t)(live ? item : 0) * M + (r < (uint32_t)M ? r : 0)) * M;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double2 v = rowlane ? row[k] : make_double2(0.0, 0.0);
                lr[k] = v.x; li[k] = v.y;
            }
        }
        bool ok = true;
        double dmine = 1.0;
        if constexpr (KIND == KIND_CAPON) {
            double trace = 0.0;
#pragma unroll
            for (int j = 0; j < M; ++j) trace += group_bcast(lr[j], j, W);
            const double floor = bazcapon::power_pivot_floor(trace, (uint32_t)M, A.rel_floor);
            double d[M];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                double vr = lr[j], vi = li[j];
#pragma unroll
                for (int k = 0; k < j; ++k) {
                    const double pr = group_bcast(lr[k], j, W), pi = group_bcast(li[k], j, W);      // L_jk
                    const double wr = pr * d[k], wi = pi * d[k];
                    vr -= lr[k] * wr + li[k] * wi;
                    vi -= li[k] * wr - lr[k] * wi;
                }
                const double dj = group_bcast(vr, j, W);
                d[j] = dj;
                ok = ok && bazcapon::power_pivot_ok(dj, floor);
                if (r == (uint32_t)j) dmine = dj;
                lr[j] = vr / dj;
                li[j] = vi / dj;
            }
            dmine = 1.0 / dmine;
        } else {
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (r == (uint32_t)j) dmine = lr[j];
        }
        if (r < (uint32_t)M) {
            const uint32_t base = g * TRI + r * (r - 1u) / 2u;              // (r == 0 stores nothing below)
#pragma unroll
            for (int k = 0; k < M - 1; ++k)
                if ((uint32_t)k < r) sL[base + k] = make_double2(lr[k], li[k]);
            sD[g * M + r] = dmine;
        }
        if (r == 0) sAlive[g] = (ok && live) ? 1 : 0;
    }
    __syncthreads();
    // ---- phase 2: one bin per lane, the group's items in a loop ----
    const uint32_t nitems = (uint32_t)((A.batch - item0 < (uint64_t)IG) ? (A.batch - item0) : (uint64_t)IG);
    const uint32_t bin_lo = range * A.range_bins;
    const uint32_t bin_hi = (A.res - bin_lo < A.range_bins) ? A.res : bin_lo + A.range_bins;
    for (uint32_t bin0 = bin_lo; bin0 < bin_hi; bin0 += 256u) {
        const uint32_t bin = bin0 + threadIdx.x;
        const bool inb = bin < A.res;
        float ar[M], ai[M];
        {
            const float2* __restrict__ row = A.raw + (size_t)(inb ? bin : 0u) * M;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const float2 v = row[i];
                ar[i] = v.x; ai[i] = v.y;
            }
        }
        double w = 0.0;
        if constexpr (KIND == KIND_BARTLETT) {
#pragma unroll
            for (int i = 0; i < M; ++i) w += (double)ar[i] * (double)ar[i] + (double)ai[i] * (double)ai[i];
        }
        float* __restrict__ out = A.spec + (size_t)item0 * A.res + (inb ? bin : 0u);
        for (uint32_t it = 0; it < nitems; ++it) {
            const double2* __restrict__ L = sL + it * TRI;
            const double* __restrict__ D = sD + it * M;
            double P;
            if constexpr (KIND == KIND_CAPON) {
                double zr[M], zi[M];
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    double xr = (double)ar[i], xi = (double)ai[i];
#pragma unroll
                    for (int k = 0; k < i; ++k) {
                        const double2 l = L[i * (i - 1) / 2 + k];
                        xr -= l.x * zr[k] - l.y * zi[k];
                        xi -= l.x * zi[k] + l.y * zr[k];
                    }
                    zr[i] = xr; zi[i] = xi;
                    s += (xr * xr + xi * xi) * D[i];
                }
                P = sAlive[it] ? bazcapon::power_from_s(s) : 0.0;
            } else {
                double q = 0.0;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const double xr = (double)ar[i], xi = (double)ai[i];
                    double tr = 0.0, ti = 0.0;                              // sum_{k<i} R_ik a_k
#pragma unroll
                    for (int k = 0; k < i; ++k) {
                        const double2 l = L[i * (i - 1) / 2 + k];
                        const double kr = (double)ar[k], ki = (double)ai[k];
                        tr += l.x * kr - l.y * ki;
                        ti += l.x * ki + l.y * kr;
                    }
                    q += D[i] * (xr * xr + xi * xi) + 2.0 * (xr * tr + xi * ti);
                }
                P = bartlett_from_qw(q, w);
            }
            if (inb) out[(size_t)it * A.res] = (float)P;
        }
    }
}

// The reference's top-n rule (lib/baz_music_doa.cc:95,129-141) on the float32 values AS STORED: the n largest values in descending
// order, the earlier bin first on ties, a value reported only if it is > 0 (NaN never), (0, 0) for missing entries; lvl is the
// stored word itself, so lvl[i] == spectrum[bin_i] bit for bit.  One wave per item: peak_pick_kernel's shape and keys without the
// neighbour condition.
template <int NMAX>
__global__ __launch_bounds__(256) void topn_spec_kernel(const float* __restrict__ spec, float* __restrict__ ang, float* __restrict__ lvl,
                                                         uint32_t batch, uint32_t res, uint32_t n)
{
    using namespace bazmusic;
    const int lane = threadIdx.x & 63;
    const uint32_t it = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= batch) return;
    const float* __restrict__ s = spec + (size_t)it * res;
    double key[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i) key[i] = key_empty();
    for (uint32_t b = lane; b < res; b += 64) {
        const float v = s[b];
        if (v > 0.0f) {
            // smaller key = larger value, then earlier bin: high word 0x7F800000 - bits(v) (v > 0: bits <= 0x7F800000)
            const uint64_t k = ((uint64_t)(0x7F800000u - __float_as_uint(v)) << 32) | (uint64_t)b;
            key_insert<NMAX>(key, __builtin_bit_cast(double, k));
        }
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) key_merge_xor<NMAX>(key, mask);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < (int)n) {
                const uint64_t k = __builtin_bit_cast(uint64_t, key[i]);
                const bool used = k < (uint64_t)BAZ_KEY_EMPTY_BITS;
                const uint32_t bin = (uint32_t)k;
                ang[(size_t)it * n + i] = used ? (float)((double)bin * 360.0 / (double)res) : 0.0f;
                if (lvl) lvl[(size_t)it * n + i] = used ? __uint_as_float(0x7F800000u - (uint32_t)(k >> 32)) : 0.0f;
            }
    }
}

// The Bartlett definition on the host for one R (m x m complex128, interleaved) and one steering row (m complex64, interleaved):
//   w = sum_i |a_i|^2;  y_i = sum_{j<i} R_ij a_j + Re(R_ii) a_i + sum_{j>i} conj(R_ji) a_j;  q = sum_i Re(conj(a_i) y_i)
// all sums in index order.
inline double bartlett_host(const uint32_t m, const double* R_ri, const float* a)
{
    double w = 0.0, q = 0.0;
    for (uint32_t i = 0; i < m; ++i) w += (double)a[2 * i] * (double)a[2 * i] + (double)a[2 * i + 1] * (double)a[2 * i + 1];
    for (uint32_t i = 0; i < m; ++i) {
        double yr = 0.0, yi = 0.0;
        for (uint32_t j = 0; j < m; ++j) {
            const double xr = (double)a[2 * j], xi = (double)a[2 * j + 1];
            if (j < i) {            // R_ij a_j
                const double rr = R_ri[2 * ((size_t)i * m + j)], ri = R_ri[2 * ((size_t)i * m + j) + 1];
                yr += rr * xr - ri * xi;
                yi += rr * xi + ri * xr;
            } else if (j == i) {    // Re(R_ii) a_i
                const double rr = R_ri[2 * ((size_t)i * m + i)];
                yr += rr * xr;
                yi += rr * xi;
            } else {                // conj(R_ji) a_j
                const double rr = R_ri[2 * ((size_t)j * m + i)], ri = R_ri[2 * ((size_t)j * m + i) + 1];
                yr += rr * xr + ri * xi;
                yi += rr * xi - ri * xr;
            }
        }
        q += (double)a[2 * i] * yr + (double)a[2 * i + 1] * yi;
    }
    return bartlett_from_qw(q, w);
}

}  // namespace bazspectrum
