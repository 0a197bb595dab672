// beam_kernels.hip.h -- the opt-in MVDR beamformer output per reported entry (baz_music_set_beam_mode, include/baz_music_hip.h;
// DESIGN.md 8g): w = R_l^-1 a / (a^H R_l^-1 a) for every reported entry, and y = w^H X over the item's own snapshots.
//
//   beam_weights_kernel<M>     one item per group of W lanes (capon_solve.hip.h; its beam_w_from_u is the (u, s) -> w step).
//   beam_apply_kernel<M>       one (item, run of 256 snapshots) per wave, one snapshot per lane and pass; the last launch of a sequence.
//
// DEFINITION.  R_l = R with loading (sum_i Re R_ii) / m added to the real diagonal (the trace summed in index order, the imaginary part
// of the diagonal ignored).  The solve of capon_solve.hip.h on R_l (d, L, z, s, the degeneracy rule on R_l's own diagonal), then
//     u_i  = z_i / d_i - sum_{k>i} conj(L_ki) u_k                (k = m-1 down to i+1)
//     w    = u / s                                               (w^H a = 1)
//     y[c] = sum_{r<m} conj(w_r) x[c m + r]                      (r = 0 .. m-1 in fp64, stored as complex64)
// A dead entry gets w = 0; w = 0 gives y = 0.
//
// WEIGHTS LAYOUT.  capon_kernel of capon_solve.hip.h with its beam blocks, the loading between the row load and the factorisation.  The
// back substitution needs COLUMN i of L in lane i: every lane writes its row of L into LDS once per item (rows padded to an odd number of
// 16-byte elements: the writes of a group fall on distinct banks) and lane i reads L_ki from row k -- the lanes of a group read
// neighbouring elements.  Each entry's back substitution then costs M - 1 broadcasts like its forward one.  L^H stays in LDS (no
// second register copy of L: M = 16 would not fit beside the first).  No lane leaves before the last shuffle or the barrier.  Every
// word of the weights is written once, M contiguous complex128 per (item, slot).
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

#include "capon_solve.hip.h"

namespace bazbeam {

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
    static constexpr int W = bazcapon::Group<M>::W;             // lanes per item
    static constexpr int THREADS = M <= 8 ? 256 : 128;          // (M > 8: half a block keeps the L^H tile under 40 KiB)
    static constexpr int IPB = THREADS / W;                     // items per block
};

template <int M>
inline constexpr auto beam_weights_kernel = &bazcapon::capon_kernel<M, BeamGeom<M>::THREADS, BeamGeom<M>::IPB, true, BeamWeightsArgs>;

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
