// subband_kernels.hip.h -- the opt-in wideband (subband) front-end (baz_music_set_subbands, include/baz_music_hip.h): every
// item is cut into blocks of F samples, an F-point DFT per antenna yields S used subbands, S inner contexts of shape (m, n, m K / F, res)
// run the fast path, each on its own subband's table, and their float32 spectra are combined into one row the pickers read.
//
//   subband_entry           the sums of NS subbands of one (block, antenna) column, __host__ __device__: subband_kernel and
//                           baz_music_subband_apply run the same text, so device and host agree bit for bit (as beamspace_entry does).
//   subband_kernel<SQ>      the channeliser: (items x K x m) complex64 times W -> [s][item][q][r] complex64, fp64 on the vector unit.
//   subband_combine_kernel  S spectrum rows -> one, harmonic or arithmetic mean in fp64.
//
// DEFINITION.  With Q = K / F, y_s(i, q, r) = fl32(sum_{t = 0 .. F-1} W[s][t] x(i, q F + t, r)): x widened exactly, the sum in fp64 from
// (+0, +0) with t ascending, each term the four fused multiply-adds of whiten_fma with wr = Re W[s][t], wi = Im W[s][t], one
// round-to-nearest conversion per component.  A (block, antenna) column reads no other column.
//
// LAYOUT (subband_kernel).  A column is one (block, antenna) pair; column c = b m + r of block b = item Q + q reads sample t at
// in[(b F + t) m + r], and subband s writes it at out[s C + c] (C columns in all): the [s][item][q][r] layout IS the column index.  A
// workgroup of four waves takes tiles of 64 consecutive columns.  The blocks a tile touches are contiguous in HBM: they are read flat,
// 16 bytes per lane (8 at an unaligned edge), and laid into LDS block by block with a block stride BS = F m + pad, pad < 32 chosen so
// that BS = m (mod 32): lane l then reads sample t at an LDS entry = l + t m + const (mod 32), so the 32 lanes of a ds_read_b64 group
// hit 32 different bank pairs.  W sits in LDS once per workgroup ([s][t] complex128, <= 32 KiB) and is read at wave-uniform addresses
// (a broadcast).  Lane l of wave w owns column l and the subbands w SQ .. w SQ + SQ - 1, SQ = ceil(S / 4): 2 SQ <= 16 fp64
// accumulators in registers; each subband's sum keeps its own order.  One subband's 64 outputs of a tile are 512 contiguous bytes: a
// wave stores them straight from its registers, no turn-over.  A short last tile reads its own blocks and writes its own columns only.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "beamspace_kernels.hip.h"
#include "whiten_kernels.hip.h"

namespace bazsubband {

// re[i] + j im[i] = sum_{t < F} w[min(i, live - 1) * F + t] x[t * xstride], i < NS (rows at and beyond `live` repeat the last live one:
// their sums are never stored)
template <int NS>
__host__ __device__ inline void subband_entry(const double2* w, const uint32_t live, const float2* x, const uint32_t xstride, const uint32_t F,
                                              double (&re)[NS], double (&im)[NS])
{
    const double2* row[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        re[i] = im[i] = 0.0;
        row[i] = w + (size_t)((uint32_t)i < live ? (uint32_t)i : live - 1u) * F;
    }
    for (uint32_t t = 0; t < F; ++t) {
        const float2 v = x[(size_t)t * xstride];
        const double xr = (double)v.x, xi = (double)v.y;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const double2 ww = row[i][t];
            bazwhiten::whiten_fma(ww.x, ww.y, xr, xi, re[i], im[i]);
        }
    }
}

constexpr int SB_THREADS = bazbeamspace::BS_THREADS;      // (flat_load walks with this stride)
constexpr uint32_t SB_TILE = 64;                          // columns per tile: one per lane

// LDS block stride in entries: F m + pad with (stride - m) a multiple of 32
__host__ __device__ constexpr uint32_t sb_block_stride(const uint32_t m, const uint32_t F) { return F * m + ((32u - ((F - 1u) * m) % 32u) % 32u); }
// the most blocks a tile can touch: its first column sits at most m - 1 columns into a block
__host__ __device__ constexpr uint32_t sb_tile_blocks(const uint32_t m) { return (m - 1u + SB_TILE - 1u) / m + 1u; }
// dynamic LDS: W, then the tile's blocks
inline size_t sb_lds_bytes(const uint32_t m, const uint32_t F, const uint32_t S)
{
    return (size_t)S * F * sizeof(double2) + (size_t)sb_tile_blocks(m) * sb_block_stride(m, F) * sizeof(float2);
}

// out[s * columns + c] = fl32(sum_t W[s][t] in[((c / m) F + t) m + c % m]) for c < columns = blocks * m, s < S.  W: [S][F] complex128.
// Dynamic LDS: sb_lds_bytes(m, F, S).  SQ = ceil(S / 4).  Grid: any number of workgroups (each walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...).  in and out do not overlap.
template <int SQ>
__global__ __launch_bounds__(SB_THREADS) void subband_kernel(const float2* __restrict__ in, float2* __restrict__ out, const double2* __restrict__ W,
                                                             const uint32_t m, const uint32_t F, const uint32_t S, const uint32_t columns)
{
    extern __shared__ double2 sb_lds[];
    double2* const sw = sb_lds;                                               // [S][F]
    float2* const sx = reinterpret_cast<float2*>(sb_lds + (size_t)S * F);     // [blocks of the tile][BS]
    const uint32_t BS = sb_block_stride(m, F), FM = F * m;
    for (uint32_t e = threadIdx.x; e < S * F; e += SB_THREADS) sw[e] = W[e];
    const uint32_t wv = threadIdx.x >> 6, col = threadIdx.x & 63u;
    const uint32_t s0 = wv * (uint32_t)SQ;                                    // this wave's first subband (wave-uniform)
    const uint32_t live = s0 < S ? (S - s0 < (uint32_t)SQ ? S - s0 : (uint32_t)SQ) : 0u;
    const uint32_t tiles = (columns + SB_TILE - 1u) / SB_TILE;
    for (uint32_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {             // (workgroup-uniform: the barriers below are safe)
        const uint32_t c0 = tl * SB_TILE;
        const uint32_t nc = columns - c0 < SB_TILE ? columns - c0 : SB_TILE;
        const uint32_t b_lo = c0 / m, b_hi = (c0 + nc - 1u) / m;              // (b_hi - b_lo + 1 <= sb_tile_blocks(m))
        __syncthreads();                                                      // (every lane has read the previous tile)
        bazbeamspace::flat_load(in + (size_t)b_lo * FM, (b_hi - b_lo + 1u) * FM, [&](const uint32_t e, const float2 v) {
            const uint32_t j = e / FM;
            sx[j * BS + (e - j * FM)] = v;
        });
        __syncthreads();
        if (col < nc && live) {
            const uint32_t c = c0 + col, b = c / m, r = c - b * m;
            double re[SQ], im[SQ];
            subband_entry<SQ>(sw + (size_t)s0 * F, live, sx + (b - b_lo) * BS + r, m, F, re, im);
#pragma unroll
            for (int i = 0; i < SQ; ++i)
                if ((uint32_t)i < live) out[(size_t)(s0 + (uint32_t)i) * columns + c] = make_float2((float)re[i], (float)im[i]);
        }
    }
}

constexpr int SBC_THREADS = 256;

// out[e] = fl32(S / sum_s 1 / (double)ps[s * total + e]) (harmonic; arithmetic: fl32((sum_s (double)ps[s * total + e]) / S)) for
// e < total: the sum from +0 with s ascending in plain fp64 adds, one division at the end; zeros, infinities and NaNs are IEEE's.
// Consecutive lanes take consecutive words; every word below `total` is written.
__global__ __launch_bounds__(SBC_THREADS) void subband_combine_kernel(const float* __restrict__ ps, float* __restrict__ out, const uint32_t S,
                                                                      const size_t total, const int arithmetic)
{
    const double n = (double)S;
    for (size_t e = (size_t)blockIdx.x * SBC_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * SBC_THREADS) {
        double acc = 0.0;
        if (arithmetic) {
            for (uint32_t s = 0; s < S; ++s) acc = acc + (double)ps[(size_t)s * total + e];
            out[e] = (float)(acc / n);
        } else {
            for (uint32_t s = 0; s < S; ++s) acc = acc + 1.0 / (double)ps[(size_t)s * total + e];
            out[e] = (float)(n / acc);
        }
    }
}

}  // namespace bazsubband
