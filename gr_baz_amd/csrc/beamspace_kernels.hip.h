// beamspace_kernels.hip.h -- the opt-in beamspace front-end (baz_music_set_beamspace, include/baz_music_hip.h): every
// snapshot x of m antennas is projected onto B <= 16 beams, y = T^H x, and an inner context of shape (B, n, B K, res) on the table
// a' = T^H a runs the fast 2 .. 16-antenna path on the projected items.
//
//   beamspace_entry      the sums of NB beams of one column, __host__ __device__: beamspace_kernel and the host functions
//                        (baz_music_beamspace_apply, the table builder of baz_music_set_beamspace) run the same text, so device and
//                        host agree bit for bit (as whiten_entry / calib_mul do).
//   beamspace_row        one whole row on the host: the B sums, the optional normalisation, the conversion.
//   beamspace_kernel<B>  (columns x m) complex64 times conj(T) -> (columns x B) complex64, fp64 on the vector unit.
//
// DEFINITION.  y_b = fl32(sum_{r = 0 .. m-1} conj(T_rb) x_r): x widened exactly, the sum in fp64 from (+0, +0) with r ascending, each
// term the four fused multiply-adds of whiten_fma with wr = Re T_rb, wi = -Im T_rb, one round-to-nearest conversion per component.
// A column reads no other column.  The operand `tc` of every routine here is conj(T), row-major [antenna r][beam b].
//
// LAYOUT (beamspace_kernel).  A workgroup of four waves takes tiles of 64 columns.  The tile's 64 m entries are contiguous in HBM: they
// are read flat, 16 bytes per lane (8 at an unaligned edge), and laid into LDS as [column][m | 1] -- the odd row length lets the 64
// lanes of a wave read entry r of 64 different columns without a bank conflict.  Lane l of wave q owns column l and the beams
// q BQ .. q BQ + BQ - 1, BQ = ceil(B / 4): 2 BQ <= 8 fp64 accumulators in registers (all 2 B of a column live in registers, spread
// over the four waves; each beam's sum keeps its own order).  conj(T) sits in LDS once per workgroup and is read at wave-uniform
// addresses (a broadcast).  The B outputs of a column are contiguous: the tile's results are turned over through LDS
// ([column][B | 1]) and written flat, 16 bytes per lane, whole runs per wave.  A short last tile reads and writes its own columns only.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "whiten_kernels.hip.h"

namespace bazbeamspace {

// re[i] + j im[i] = sum_r tc[r * tstride + i] x[r], i < NB
template <int NB>
__host__ __device__ inline void beamspace_entry(const double2* tc, const uint32_t tstride, const float2* x, const uint32_t m, double (&re)[NB],
                                                double (&im)[NB])
{
#pragma unroll
    for (int i = 0; i < NB; ++i) re[i] = im[i] = 0.0;
    for (uint32_t r = 0; r < m; ++r) {
        const double xr = (double)x[r].x, xi = (double)x[r].y;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const double2 w = tc[(size_t)r * tstride + i];
            bazwhiten::whiten_fma(w.x, w.y, xr, xi, re[i], im[i]);
        }
    }
}

// Host: one row x (m entries) -> out (B entries).  normalise: the unrounded sums are divided by nu = sqrt(sum_b Re^2 + Im^2) (b ascending,
// re before im, by fma) in front of the conversion; a row whose nu is 0 or not finite becomes zeros.  `s` is scratch for 2 B doubles.
inline void beamspace_row(const double2* tc, const uint32_t m, const uint32_t B, const float2* x, const int normalise, double* s, float2* out)
{
    for (uint32_t b = 0; b < B; ++b) {
        double re[1], im[1];
        beamspace_entry<1>(tc + b, B, x, m, re, im);
        s[2 * b] = re[0];
        s[2 * b + 1] = im[0];
    }
    if (normalise) {
        double nu2 = 0.0;
        for (uint32_t b = 0; b < B; ++b) {
            nu2 = fma(s[2 * b], s[2 * b], nu2);
            nu2 = fma(s[2 * b + 1], s[2 * b + 1], nu2);
        }
        const double nu = sqrt(nu2);
        const bool ok = nu > 0.0 && (nu - nu == 0.0);
        for (uint32_t i = 0; i < 2 * B; ++i) s[i] = ok ? s[i] / nu : 0.0;
    }
    for (uint32_t b = 0; b < B; ++b) out[b] = make_float2((float)s[2 * b], (float)s[2 * b + 1]);
}

constexpr int BS_THREADS = 256;
constexpr uint32_t BS_TILE = 64;      // columns per tile: one per lane

__host__ __device__ constexpr uint32_t bs_x_stride(const uint32_t m) { return m | 1u; }
// dynamic LDS: conj(T), then the tile (its region also turns the results over: B | 1 <= m | 1)
inline size_t bs_lds_bytes(const uint32_t m, const uint32_t B) { return (size_t)m * B * sizeof(double2) + (size_t)BS_TILE * bs_x_stride(m) * sizeof(float2); }

// `cnt` consecutive complex64 from global memory, handed to put(e, value) for e < cnt: 16 bytes per lane where the pair lies inside
// the range (src need only be 8-byte aligned: the pairs start at the first 16-byte boundary at or in front of it), 8 at the edges
template <typename Put>
__device__ __forceinline__ void flat_load(const float2* __restrict__ src, const uint32_t cnt, Put put)
{
    const uint32_t off = (uint32_t)((reinterpret_cast<uintptr_t>(src) >> 3) & 1u);
    const uint32_t pairs = (cnt + off + 1u) >> 1;
    for (uint32_t p = threadIdx.x; p < pairs; p += BS_THREADS) {
        const int64_t e0 = 2 * (int64_t)p - off;
        if (e0 >= 0 && e0 + 1 < (int64_t)cnt) {
            const float4 v = *reinterpret_cast<const float4*>(src + e0);
            put((uint32_t)e0, make_float2(v.x, v.y));
            put((uint32_t)e0 + 1u, make_float2(v.z, v.w));
        } else {
            if (e0 >= 0) put((uint32_t)e0, src[e0]);                       // (then e0 + 1 == cnt)
            else if (e0 + 1 < (int64_t)cnt) put((uint32_t)(e0 + 1), src[e0 + 1]);
        }
    }
}

// ... and the same walk for a store: dst[e] = get(e), e < cnt
template <typename Get>
__device__ __forceinline__ void flat_store(float2* __restrict__ dst, const uint32_t cnt, Get get)
{
    const uint32_t off = (uint32_t)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1u);
    const uint32_t pairs = (cnt + off + 1u) >> 1;
    for (uint32_t p = threadIdx.x; p < pairs; p += BS_THREADS) {
        const int64_t e0 = 2 * (int64_t)p - off;
        if (e0 >= 0 && e0 + 1 < (int64_t)cnt) {
            const float2 a = get((uint32_t)e0), b = get((uint32_t)e0 + 1u);
            *reinterpret_cast<float4*>(dst + e0) = make_float4(a.x, a.y, b.x, b.y);
        } else {
            if (e0 >= 0) dst[e0] = get((uint32_t)e0);
            else if (e0 + 1 < (int64_t)cnt) dst[e0 + 1] = get((uint32_t)(e0 + 1));
        }
    }
}

// out[c][b] = fl32(sum_r Tc[r][b] in[c][r]) for c < columns.  Tc = conj(T), [m][B] complex128.  Dynamic LDS: bs_lds_bytes(m, B).
// Grid: any number of workgroups (each walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...).  in and out do not overlap.
template <int B>
__global__ __launch_bounds__(BS_THREADS) void beamspace_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                               const double2* __restrict__ Tc, const uint32_t m, const uint32_t columns)
{
    constexpr int BQ = (B + 3) / 4;               // beams per wave
    constexpr int NW = (B + BQ - 1) / BQ;         // waves that own beams
    constexpr int LAST = B - (NW - 1) * BQ;       // beams of the last of them
    constexpr uint32_t SO = (uint32_t)B | 1u;     // row length of the turn-over image
    extern __shared__ double2 bs_lds[];
    double2* const st = bs_lds;                                            // [m][B]
    float2* const sx = reinterpret_cast<float2*>(bs_lds + (size_t)m * B);  // [BS_TILE][S], then [BS_TILE][SO]
    const uint32_t S = bs_x_stride(m);
    for (uint32_t e = threadIdx.x; e < m * (uint32_t)B; e += BS_THREADS) st[e] = Tc[e];
    const uint32_t q = threadIdx.x >> 6, col = threadIdx.x & 63u;
    const uint32_t tiles = (columns + BS_TILE - 1u) / BS_TILE;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {             // (workgroup-uniform: the barriers below are safe)
        const uint32_t c0 = t * BS_TILE;
        const uint32_t nc = columns - c0 < BS_TILE ? columns - c0 : BS_TILE;
        __syncthreads();                                                   // (the previous tile's results have left the region)
        flat_load(in + (size_t)c0 * m, nc * m, [&](const uint32_t e, const float2 v) {
            const uint32_t c = e / m;
            sx[c * S + (e - c * m)] = v;
        });
        __syncthreads();
        double re[BQ], im[BQ];
        const bool live = col < nc && q < (uint32_t)NW;
        if (live) {
            if (q + 1u < (uint32_t)NW) {
                beamspace_entry<BQ>(st + q * BQ, B, sx + col * S, m, re, im);
            } else {
                double rl[LAST], il[LAST];
                beamspace_entry<LAST>(st + q * BQ, B, sx + col * S, m, rl, il);
#pragma unroll
                for (int i = 0; i < LAST; ++i) { re[i] = rl[i]; im[i] = il[i]; }
            }
        }
        __syncthreads();                                                   // (every lane has read its column)
        if (live) {
#pragma unroll
            for (int i = 0; i < BQ; ++i)
                if (i < LAST || q + 1u < (uint32_t)NW) sx[col * SO + q * BQ + i] = make_float2((float)re[i], (float)im[i]);
        }
        __syncthreads();
        flat_store(out + (size_t)c0 * B, nc * (uint32_t)B, [&](const uint32_t e) {
            const uint32_t c = e / (uint32_t)B;
            return sx[c * SO + (e - c * (uint32_t)B)];
        });
    }
}

}  // namespace bazbeamspace
