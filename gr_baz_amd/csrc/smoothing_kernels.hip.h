// smoothing_kernels.hip.h -- the re-stacking kernel of the opt-in forward-backward averaging / spatial smoothing mode
// (baz_music_set_smoothing, include/baz_music_hip.h; DESIGN.md "Coherent emitters").
//
// With m_s the subarray size, L = m - m_s + 1 subarrays and X one item (m x K, x(r, c) = in[c*m + r]), the smoothed
// covariance is the plain covariance of the RE-STACKED item
//     Y = [X_0, ..., X_{L-1} (, P conj(X_0), ..., P conj(X_{L-1}))]      m_s x K',  K' = L * K * (fb ? 2 : 1),
// X_l = rows l .. l + m_s - 1 of X, P the centro-symmetry involution of the subarray (perm[] below).  Column c' = q*K + k of
// Y (q < L: forward block l = q; q >= L: backward block l = q - L) is
//     y(r, c') = x(r + l, k)                 forward
//     y(r, c') = conj(x(perm[r] + l, k))     backward
// and Y is laid out like any item, y(r, c') = out[c'*m_s + r], so the inner context of shape (m_s, n, m_s*K', res) reads
// it as its input.  The gather only moves, conjugates and permutes fp32 values: exact.
//
// Memory-bound (8 B read + 8 B written per output value; the reads of one item -- K*m*8 bytes -- come from L2 after the
// first of its 2L blocks touched them).  Each thread writes TWO consecutive output values with one 16-B store (the
// flattened output index 2t is even and the buffer 256-B aligned, so every store is aligned whatever m_s and K' are);
// consecutive lanes write consecutive 16 B: 1 KiB per wave store.  The two reads are 8-B loads: the source of an output
// pair is contiguous only in the forward blocks, and not 16-B aligned in general.  The grid covers the batch's output,
// flat: item = g / (K' m_s) per value (32-bit: the caller keeps a launch below 2^31 values, baz_music_hip.hip chunks the
// batch to BAZ_MUSIC_SMOOTH_WORKSPACE_BYTES).
// gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bazsmooth {

constexpr uint32_t RESTACK_THREADS = 256;

// the involution of the subarray's elements, by value in the kernel arguments (m_s <= 64)
struct Perm {
    uint8_t p[64];
};

struct RestackGeom {
    uint32_t m, ms, K, L;
    uint32_t per_item;      // K' * m_s: output values per item
    uint32_t fb;            // 1: the backward blocks follow the forward ones
};

__device__ inline float2 restack_value(const float2* __restrict__ in, const RestackGeom& g, const Perm& perm, uint32_t idx)
{
    const uint32_t item = idx / g.per_item;
    const uint32_t o = idx - item * g.per_item;
    const uint32_t col = o / g.ms, r = o - col * g.ms;
    const uint32_t q = col / g.K, k = col - q * g.K;
    const bool back = q >= g.L;
    const uint32_t l = back ? q - g.L : q;
    const uint32_t src = (back ? (uint32_t)perm.p[r] : r) + l;
    const float2 v = in[(size_t)item * g.K * g.m + (size_t)k * g.m + src];
    return back ? make_float2(v.x, -v.y) : v;
}

// total = batch * per_item output values; thread t writes values 2t and 2t + 1 (the last thread of an odd total one)
__global__ __launch_bounds__(RESTACK_THREADS) void restack_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                                   RestackGeom g, Perm perm, uint32_t total)
{
    const uint32_t t = blockIdx.x * RESTACK_THREADS + threadIdx.x;
    const uint32_t i0 = 2u * t;
    if (i0 >= total) return;
    const float2 a = restack_value(in, g, perm, i0);
    if (i0 + 1u < total) {
        const float2 b = restack_value(in, g, perm, i0 + 1u);
        *reinterpret_cast<float4*>(out + i0) = make_float4(a.x, a.y, b.x, b.y);
    } else {
        out[i0] = a;
    }
}

}  // namespace bazsmooth
