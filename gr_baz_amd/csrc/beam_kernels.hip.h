// beam_kernels.hip.h -- the opt-in MVDR beamformer output per reported entry (baz_music_set_beam_mode, include/baz_music_hip.h;
// DESIGN.md 8g): w = R_l^-1 a / (a^H R_l^-1 a) for every reported entry, and y = w^H X over the item's own snapshots.
//
//   beam_w_from_u              the s -> w step, __host__ __device__: beam_weights_kernel and baz_music_beam_weights() compile the same
//                              text (the degeneracy rule is power_kernels.hip.h's power_pivot_floor / power_pivot_ok, on R_l).
//   beam_weights_kernel<M>     one item per group of W lanes (W = 4 / 8 / 16 for M <= 4 / 8 / 16), power_kernel's layout.
//   beam_apply_kernel<M>       one (item, run of 256 snapshots) per wave, one snapshot per lane and pass; the last launch of a sequence.
//
// DEFINITION.  R_l = R with loading (sum_i Re R_ii) / m added to the real diagonal (the trace summed in index order, the imaginary part
// of the diagonal ignored).  Unpivoted LDL^H of R_l in fp64 from the lower triangle as stored, as power_kernels.hip.h states it, then
//     z_i  = a_i - sum_{k<i} L_ik z_k                            (a: the table row, complex64 widened exactly)
//     s    = sum_i |z_i|^2 / d_i
//     u_i  = z_i / d_i - sum_{k>i} conj(L_ki) u_k                (k = m-1 down to i+1)
//     w    = u / s                                               (w^H a = 1)
//     y[c] = sum_{r<m} conj(w_r) x[c m + r]                      (r = 0 .. m-1 in fp64, stored as complex64)
// An item is DEGENERATE when some d_j is not finite or d_j <= 2^-40 (sum_i Re (R_l)_ii) / m: all its entries get w = 0.  An entry whose
// s is 0 or not finite gets w = 0; a missing entry (lvl == 0) gets w = 0; w = 0 gives y = 0.
//
// WEIGHTS LAYOUT.  As power_kernel: lane r of a group owns row r of R, the factorisation and the forward substitution go by width-W
// shuffles that never leave a 16-lane row.  The back substitution needs COLUMN i of L in lane i: every lane writes its row of L into
// LDS once per item (rows padded to an odd number of 16-byte elements: the writes of a group fall on distinct banks) and lane i reads
// L_ki from row k -- the lanes of a group read neighbouring elements.  Each entry's back substitution then costs M - 1 broadcasts like
// its forward one.  L^H stays in LDS (no second register copy of L: M = 16 would not fit beside the first).  A degenerate item, an
// item beyond the batch or a lane beyond M runs the same instructions on zeros / garbage and only its stores differ: no lane leaves
// before the last shuffle or the barrier.  Every word of the weights is written once, M contiguous complex128 per (item, slot).
//
// APPLY LAYOUT.  A wave works on one item at a time: its n M weights are copied into LDS once (with one flag per entry: has it
// weights at all -- an entry without weights stores exact zeros whatever x holds) and every later read of them is a same-address
// (broadcast) LDS read.  Lane l takes snapshot c = 256 seg + 64 j + l (j = 0 .. 3): it reads the snapshot's M contiguous complex64
// -- 16-byte loads where M is even (and the input 16-byte aligned), 8-byte loads otherwise; the lanes of a wave cover one contiguous
// 512 M-byte run and no byte is read twice -- and stores n complex64, slot by slot, unit-stride over the lanes.  No atomics; no
// lane leaves before the barrier.  For M > 8 a lane's loads touch a cache line of their own each (cost).
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "power_kernels.hip.h"

namespace bazbeam {

// u, s -> w = u / s; an s that is 0 or not finite (or a dead item / missing entry: alive == false) gives w = 0
__host__ __device__ inline void beam_w_from_u(const double ur, const double ui, const double s, const bool alive, double* wr, double* wi)
{
    const bool good = alive && (s - s == 0.0) && s != 0.0;
    *wr = good ? ur / s : 0.0;
    *wi = good ? ui / s : 0.0;
}

struct BeamWeightsArgs {
    const float* ang_in;       // [batch * n] what the merge / picker / truncation left (device staging), on the grid
    const float* lvl_in;       // [batch * n] ... lvl != 0 marks a real entry
    float* ang_out;            // [batch * n] the caller's ang, or nullptr (refine_kernel / power_kernel writes it)
    float* lvl_out;            // [batch * n] the caller's lvl, or nullptr (not wired, or refine_kernel / power_kernel writes it)
    double2* w_out;            // [batch][n][M] the weights (baz_music_last_beam_weights)
    const double2* R;          // [batch][M][M] the covariances the EVD read, row-major
    const float2* raw;         // the raw table in force, [res][M] complex64
    double rel_floor;          // BAZ_MUSIC_POWER_PIVOT_FLOOR
    double loading;            // diagonal loading, in units of the mean diagonal
    uint32_t batch, n, res;
};

template <int M>
struct BeamGeom {
    static constexpr int W = bazpower::PowerGeom<M>::W;         // lanes per item
    static constexpr int THREADS = M <= 8 ? 256 : 128;          // (M > 8: half a block keeps the L^H tile under 40 KiB)
    static constexpr int IPB = THREADS / W;                     // items per block
    static constexpr int S = M | 1;                             // row pitch of the L^H tile, in complex128
};

template <int M>
__global__ __launch_bounds__(BeamGeom<M>::THREADS) void beam_weights_kernel(const BeamWeightsArgs A)
{
    using bazpower::group_bcast;
    constexpr int W = BeamGeom<M>::W, S = BeamGeom<M>::S;
    __shared__ double2 LT[BeamGeom<M>::IPB * M * S];
    const uint32_t r = threadIdx.x % W;                                     // this lane's row
    const uint64_t item = (uint64_t)blockIdx.x * BeamGeom<M>::IPB + threadIdx.x / W;
    const bool live = item < A.batch;                                       // (uniform over the group)
    const bool rowlane = live && r < (uint32_t)M;
    double2* const lt = LT + (threadIdx.x / W) * (M * S);                   // this group's tile
    // row r of R; zeros for lanes without a row
    double lr[M], li[M];
    {
        const double2* __restrict__ row = A.R + ((size_t)(live ? item : 0) * M + (r < (uint32_t)M ? r : 0)) * M;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const double2 v = rowlane ? row[k] : make_double2(0.0, 0.0);
            lr[k] = v.x; li[k] = v.y;
        }
    }
    // the loading, then the floor: both diagonals summed in index order (what the host routine does)
    double trace = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) trace += group_bcast(lr[j], j, W);
    const double delta = A.loading * (trace / (double)M);
#pragma unroll
    for (int j = 0; j < M; ++j)
        if (r == (uint32_t)j) lr[j] += delta;
    double trace_l = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) trace_l += group_bcast(lr[j], j, W);
    const double floor = bazpower::power_pivot_floor(trace_l, (uint32_t)M, A.rel_floor);
    // LDL^H, column by column (power_kernel's loop)
    double d[M];
    bool ok = true;
    double dmine = 1.0;                                                     // d_r
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
        const double dj = group_bcast(vr, j, W);                            // lane j's value is the pivot (its imaginary part ignored)
        d[j] = dj;
        ok = ok && bazpower::power_pivot_ok(dj, floor);
        if (r == (uint32_t)j) dmine = dj;
        lr[j] = vr / dj;
        li[j] = vi / dj;
    }
    // L^H: row r of L into the tile, read back by columns below
    if (r < (uint32_t)M) {
#pragma unroll
        for (int k = 0; k < M; ++k) lt[r * S + k] = make_double2(lr[k], li[k]);
    }
    __syncthreads();
    // the item's entries
    float ang_mine = 0.0f, lvl_mine = 0.0f;                                 // lane e keeps entry e
    for (uint32_t e = 0; e < A.n; ++e) {
        const size_t t = (size_t)(live ? item : 0) * A.n + e;
        const float a_in = A.ang_in[t], l_in = A.lvl_in[t];
        // the entry's bin (refine_kernel's recovery: within 1/16 of b up to 2^20 bins)
        uint32_t b = (uint32_t)__double2ll_rn((double)a_in * (double)A.res / 360.0);
        b = b < A.res ? b : A.res - 1u;
        const float2 av = r < (uint32_t)M ? A.raw[(size_t)b * M + r] : make_float2(0.0f, 0.0f);
        double zr = (double)av.x, zi = (double)av.y;
#pragma unroll
        for (int k = 0; k < M - 1; ++k) {
            const double kr = group_bcast(zr, k, W), ki = group_bcast(zi, k, W);            // z_k, final in lane k
            if (r > (uint32_t)k) {
                zr -= lr[k] * kr - li[k] * ki;
                zi -= lr[k] * ki + li[k] * kr;
            }
        }
        double s = r < (uint32_t)M ? (zr * zr + zi * zi) / dmine : 0.0;
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, W);
        double ur = r < (uint32_t)M ? zr / dmine : 0.0, ui = r < (uint32_t)M ? zi / dmine : 0.0;
#pragma unroll
        for (int k = M - 1; k > 0; --k) {
            const double kr = group_bcast(ur, k, W), ki = group_bcast(ui, k, W);            // u_k, final in lane k
            const double2 c = lt[r < (uint32_t)k ? k * S + (int)r : 0];                     // L_kr
            if (r < (uint32_t)k) {                                                          // conj(L_kr) u_k
                ur -= c.x * kr + c.y * ki;
                ui -= c.x * ki - c.y * kr;
            }
        }
        double wr, wi;
        beam_w_from_u(ur, ui, s, ok && l_in != 0.0f, &wr, &wi);
        if (rowlane) A.w_out[t * M + r] = make_double2(wr, wi);
        if (r == e) { ang_mine = a_in; lvl_mine = l_in; }
    }
    if (live && r < A.n) {
        const size_t t = (size_t)item * A.n + r;
        if (A.ang_out) A.ang_out[t] = ang_mine;
        if (A.lvl_out) A.lvl_out[t] = lvl_mine;
    }
}

struct BeamApplyArgs {
    const float2* x;           // [batch][K][M] the chunk's input (device memory, or the caller's mapped input on the zero-copy path)
    const double2* w;          // [batch][n][M] this chunk's weights
    float2* y;                 // [batch][n][K] this chunk's beams
    uint32_t batch, n, K;
    uint32_t nseg;             // runs of APPLY_SEG snapshots per item
};

constexpr int APPLY_THREADS = 256;
constexpr int APPLY_WAVES = APPLY_THREADS / 64;
constexpr int APPLY_SEG = 256;                                  // snapshots per wave: 4 passes of one snapshot per lane

// V4: 16-byte loads (M even and the input 16-byte aligned); else 8-byte loads
template <int M, bool V4>
__global__ __launch_bounds__(APPLY_THREADS) void beam_apply_kernel(const BeamApplyArgs A)
{
    extern __shared__ __align__(16) double2 beam_sw[];                      // [APPLY_WAVES][n * M] weights, then [APPLY_WAVES][n] flags
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint64_t unit = (uint64_t)blockIdx.x * APPLY_WAVES + wave;        // (item, run) of this wave
    const bool live = unit < (uint64_t)A.batch * A.nseg;                    // (uniform over the wave)
    const uint64_t item = live ? unit / A.nseg : 0;
    const uint32_t seg = live ? (uint32_t)(unit % A.nseg) : 0;
    const uint32_t nw = A.n * M;
    double2* const sw = beam_sw + (size_t)wave * nw;
    uint32_t* const alive = reinterpret_cast<uint32_t*>(beam_sw + (size_t)APPLY_WAVES * nw) + wave * A.n;
    {
        const double2* __restrict__ wsrc = A.w + item * nw;
        for (uint32_t i = lane; i < nw; i += 64) sw[i] = wsrc[i];
        // an entry without weights (missing, degenerate item, s not finite) has y = 0 whatever x holds (NaN and Inf included)
        for (uint32_t e = lane; e < A.n; e += 64) {
            bool nz = false;
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double2 v = wsrc[e * M + k];
                nz = nz || v.x != 0.0 || v.y != 0.0;
            }
            alive[e] = nz ? 1u : 0u;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < APPLY_SEG / 64; ++j) {
        const uint32_t c = seg * APPLY_SEG + j * 64 + lane;
        if (!live || c >= A.K) continue;                                    // (after the only barrier)
        const float2* __restrict__ xs = A.x + (item * A.K + c) * M;
        float2 x[M];
        if constexpr (V4) {
            static_assert(M % 2 == 0, "16-byte loads need an even M");
            const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xs);
#pragma unroll
            for (int k = 0; k < M / 2; ++k) {
                const float4 v = x4[k];
                x[2 * k] = make_float2(v.x, v.y);
                x[2 * k + 1] = make_float2(v.z, v.w);
            }
        } else {
#pragma unroll
            for (int k = 0; k < M; ++k) x[k] = xs[k];
        }
        float2* __restrict__ ys = A.y + item * A.n * A.K + c;
        for (uint32_t e = 0; e < A.n; ++e) {
            double yr = 0.0, yi = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) {                                   // conj(w_k) x_k
                const double2 wk = sw[e * M + k];
                const double xr = (double)x[k].x, xi = (double)x[k].y;
                yr += wk.x * xr + wk.y * xi;
                yi += wk.x * xi - wk.y * xr;
            }
            ys[(size_t)e * A.K] = alive[e] ? make_float2((float)yr, (float)yi) : make_float2(0.0f, 0.0f);
        }
    }
}

}  // namespace bazbeam
