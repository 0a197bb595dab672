// average_kernels.hip.h -- the opt-in covariance averaging across the items of a stream (baz_music_set_averaging,
// include/baz_music_hip.h): a sliding window of W items with a forgetting factor, between the covariance and the EVD.
//
//   averaging_table         the weights, __host__ __device__: the library fills the kernels' table with it and
//                           baz_music_averaging_weights() hands out the same numbers, so the rule is testable without a device.
//   average_kernel          R-bar of a launch's items from their plain covariances and the history of the items before them.
//   average_history_kernel  the history the NEXT launch reads: the last W - 1 plain covariances of the stream so far.
//
// DEFINITION.  w_0 = 1, w_j = w_{j-1} beta (fp64); c(t) = min(W, t + 1) taps for stream item t;
//     R-bar_t = (sum_{j = c-1 .. 0} w_j R_{t-j}) inv_norm[c],   inv_norm[c] = 1 / sum_{j < c} w_j  (summed j ascending)
// per complex entry and component: from 0, one fp64 FMA per tap OLDEST TAP FIRST, then one multiply.  The sequence of operations
// of an output depends on (t, W, beta) alone -- not on where in a launch the item sits, not on how many of its taps come from
// the history -- so a stream gives the same bits however it is cut into launches.  No running sum, nothing is subtracted.
//
// LAYOUT.  m is a run-time quantity: R is [items][E] double2 with E = m^2, so on the flat array this is a FIR with stride E.  A lane
// owns one entry e (consecutive lanes: consecutive 16 bytes) and a tile of T consecutive items, with T accumulators indexed
// statically.  It walks the tile's T + W - 1 inputs once in ascending item order, eight loads in flight: every accumulator meets its taps oldest first
// and R is read (T + W - 1) / T times instead of W times.  Inputs in front of the launch come from the history buffer H
// ([W - 1][E], H[W - 1 + v] is launch-relative item v < 0; only the last `hist` of them exist).  The table sits in LDS; tap
// indices are uniform over the wave (they depend on the walk's step and the accumulator, not on the lane's tile), so a weight
// is one broadcast read.  The output goes to a second buffer: the plain R's are still inputs of their neighbours.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define BAZ_AVG_MAX_WINDOW 64      // == BAZ_MUSIC_MAX_AVG_WINDOW (include/baz_music_hip.h)

namespace bazavg {

struct AvgTable {
    double w[BAZ_AVG_MAX_WINDOW];             // w[j], j < W (0 beyond)
    double inv_norm[BAZ_AVG_MAX_WINDOW + 1];  // inv_norm[c], 1 <= c <= W (inv_norm[0] = 0: no item has no tap)
};

// Fills the table for (W, beta), 1 <= W <= BAZ_AVG_MAX_WINDOW, 0 < beta <= 1, and returns the effective number of items of a FULL
// window, n_eff = (sum w)^2 / sum w^2 (W for a boxcar: both sums are exact integers then).
__host__ __device__ inline double averaging_table(const uint32_t W, const double beta, AvgTable& t)
{
    for (uint32_t j = 0; j < BAZ_AVG_MAX_WINDOW; ++j) t.w[j] = 0.0;
    for (uint32_t j = 0; j <= BAZ_AVG_MAX_WINDOW; ++j) t.inv_norm[j] = 0.0;
    double s = 0.0, s2 = 0.0, w = 1.0;
    for (uint32_t j = 0; j < W; ++j) {
        if (j) w = w * beta;
        t.w[j] = w;
        s = s + w;
        s2 = s2 + w * w;
        t.inv_norm[j + 1] = 1.0 / s;
    }
    return (s * s) / s2;
}

constexpr int AVG_THREADS = 256;
constexpr int AVG_LOADS = 8;        // inputs a lane has in flight at once (the walk is latency-bound otherwise: 79 dependent steps at W = 64)

// Grid: ceil(ntiles * E / 256) workgroups, ntiles = ceil(batch / T).  `hist` <= W - 1: history items that exist.
template <int T>
__global__ __launch_bounds__(AVG_THREADS) void average_kernel(const double2* __restrict__ R, const double2* __restrict__ H,
                                                               double2* __restrict__ out, const AvgTable tab, const uint32_t batch,
                                                               const uint32_t E, const uint32_t W, const uint32_t hist)
{
    __shared__ double sw[BAZ_AVG_MAX_WINDOW];
    __shared__ double sinv[BAZ_AVG_MAX_WINDOW + 1];
    if (threadIdx.x < BAZ_AVG_MAX_WINDOW) sw[threadIdx.x] = tab.w[threadIdx.x];
    if (threadIdx.x <= BAZ_AVG_MAX_WINDOW) sinv[threadIdx.x] = tab.inv_norm[threadIdx.x];
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * AVG_THREADS + threadIdx.x;
    const uint64_t tile = g / E;
    const uint32_t e = (uint32_t)(g - tile * E);
    const int64_t i0 = (int64_t)tile * T;
    if (i0 >= (int64_t)batch) return;
    double ar[T], ai[T];
#pragma unroll
    for (int a = 0; a < T; ++a) { ar[a] = 0.0; ai[a] = 0.0; }
    const int taps = (int)W, steps = T + taps - 1;
    const int64_t v_lo = -(int64_t)hist, v_hi = (int64_t)batch - 1;          // the inputs that exist, launch-relative
    for (int u0 = 0; u0 < steps; u0 += AVG_LOADS) {
        // AVG_LOADS inputs at a time: their loads are issued together (an input that does not exist reads the nearest one that
        // does -- always inside R / H -- and is not used), then the FMAs in ascending input order
        double2 x[AVG_LOADS];
        bool ok[AVG_LOADS];
#pragma unroll
        for (int k = 0; k < AVG_LOADS; ++k) {
            const int64_t v = i0 - (taps - 1) + u0 + k;              // launch-relative item of this input
            ok[k] = u0 + k < steps && v >= v_lo && v <= v_hi;        // not in front of the stream's start / behind the launch
            const int64_t vc = v < v_lo ? v_lo : (v > v_hi ? v_hi : v);
            x[k] = vc < 0 ? H[(size_t)(taps - 1 + vc) * E + e] : R[(size_t)vc * E + e];
        }
#pragma unroll
        for (int k = 0; k < AVG_LOADS; ++k) {
            if (!ok[k]) continue;
#pragma unroll
            for (int a = 0; a < T; ++a) {
                const int j = a + (taps - 1) - (u0 + k);             // the tap this input is for item i0 + a (uniform over the wave)
                if (j >= 0 && j < taps) {
                    const double wj = sw[j];
                    ar[a] = fma(wj, x[k].x, ar[a]);
                    ai[a] = fma(wj, x[k].y, ai[a]);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < T; ++a) {
        const int64_t i = i0 + a;
        if (i < (int64_t)batch) {
            const uint64_t have = (uint64_t)hist + (uint64_t)i + 1u;            // c = min(W, items of the stream up to this one)
            const double s = sinv[have < W ? (uint32_t)have : W];
            out[(size_t)i * E + e] = make_double2(ar[a] * s, ai[a] * s);
        }
    }
}

// Hn[s] = launch-relative item batch - (W - 1) + s, s < W - 1: from R where that is >= 0, else from the old history (slot
// s + batch).  Hn and Ho are two buffers used in turn; slots in front of the stream's start carry over whatever they held (the
// buffers are zero-filled when they are allocated) and are never read as taps.  Grid: ceil((W - 1) E / 256).
__global__ __launch_bounds__(AVG_THREADS) void average_history_kernel(const double2* __restrict__ R, const double2* __restrict__ Ho,
                                                                       double2* __restrict__ Hn, const uint32_t batch, const uint32_t E,
                                                                       const uint32_t W)
{
    const uint64_t g = (uint64_t)blockIdx.x * AVG_THREADS + threadIdx.x;
    const uint64_t s = g / E;
    if (s >= (uint64_t)W - 1u) return;
    const uint32_t e = (uint32_t)(g - s * E);
    const int64_t v = (int64_t)batch - (int64_t)(W - 1u) + (int64_t)s;
    Hn[(size_t)s * E + e] = v >= 0 ? R[(size_t)v * E + e] : Ho[(size_t)(s + batch) * E + e];
}

}  // namespace bazavg
