// calib_kernels.hip.h -- the opt-in per-antenna gain / phase calibration (baz_music_set_calibration, baz_music_calibrate,
// include/baz_music_hip.h): the table in force becomes a'_r(bin) = gamma_r a_r(bin), and gamma can be estimated from a
// pilot's covariances.
//
//   calib_mul           the product of the definition, __host__ __device__: table_calib_kernel and baz_music_calibration_apply() run the
//                       same text, so the rule is testable without a device.
//   table_calib_kernel  the raw table from the page-locked staging copy, times gamma, into dRaw: takes the place of the first
//                       copy_words_kernel launch of build_tables_device while a calibration is on.  Every image follows from dRaw.
//   mean_geometry       how a batch of B covariances is cut into runs and chunks, __host__: a function of (B, m) alone.
//   cov_mean_kernel     sums of consecutive runs of [items][ncomp] doubles: level one over the covariances of a chunk, level two (one
//                       run, scaled by 1 / B) over the partial sums of all chunks.
//
// DEFINITION (calib_mul).  Both operands are widened exactly to fp64; each of the four products is exact there (two 24-bit significands);
//     re = g.re a.re - g.im a.im,  im = g.re a.im + g.im a.re
// take one fp64 rounding each (the same with or without FMA contraction: the contracted product is the exact one too), then one
// round-to-nearest-even conversion to fp32.  gamma = (1, 0) returns the bits of a, except that a component -0 may come back as +0.
//
// DEFINITION (R-bar).  The B covariances are cut into G = ceil(B / L) runs of L consecutive items.  Level one: P_g = the sum of run g,
// from 0, one fp64 addition per item in ascending item order, per real component.  Level two: R-bar = (sum_g P_g, g ascending from 0)
// times (1.0 / B).  L, G and the chunk cut (a multiple of L: no run straddles two launches) depend on (B, m) alone and nothing is
// accumulated atomically, so the bits of R-bar depend on the covariances and (B, m) alone.
//
// LAYOUT.  A covariance is ncomp = 2 m^2 consecutive doubles; a lane owns one real component (consecutive lanes: consecutive doubles,
// every wave load is one contiguous 512 bytes) and walks its run with MEAN_LOADS loads in flight.  The table kernel gives a lane one
// complex64 entry per step: an 8-byte load over the link, an 8-byte unit-stride store; gamma comes by value and sits in LDS.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define BAZ_CALIB_MAX_M 64         // == BAZ_MUSIC_MAX_M (include/baz_music_hip.h)

namespace bazcalib {

struct CalibGamma {
    float2 g[BAZ_CALIB_MAX_M];     // gamma_r, r < m (unused beyond)
};

__host__ __device__ inline void calib_mul(const float g_re, const float g_im, const float a_re, const float a_im, float* o_re, float* o_im)
{
    const double gr = (double)g_re, gi = (double)g_im, ar = (double)a_re, ai = (double)a_im;
    const double re = gr * ar - gi * ai;
    const double im = gr * ai + gi * ar;
    *o_re = (float)re;
    *o_im = (float)im;
}

constexpr int CALIB_THREADS = 256;

// dst[i] = gamma[i mod m] src[i] for the n = res * m entries of a [bin][antenna] table.  Grid: any number of workgroups (grid-stride).
// `src` may be page-locked host memory addressed over the link (see copy_words_kernel).
__global__ __launch_bounds__(CALIB_THREADS) void table_calib_kernel(const float2* __restrict__ src, float2* __restrict__ dst, const size_t n,
                                                                     const uint32_t m, const CalibGamma gamma)
{
    __shared__ float2 sg[BAZ_CALIB_MAX_M];
    if (threadIdx.x < BAZ_CALIB_MAX_M) sg[threadIdx.x] = gamma.g[threadIdx.x];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * CALIB_THREADS;
    size_t i = (size_t)blockIdx.x * CALIB_THREADS + threadIdx.x;
    uint32_t r = (uint32_t)(i % m);                        // the antenna of entry i, kept current without a division per step
    const uint32_t rstep = (uint32_t)(stride % m);
    for (; i < n; i += stride) {
        const float2 a = src[i];
        const float2 g = sg[r];
        float2 o;
        calib_mul(g.x, g.y, a.x, a.y, &o.x, &o.y);
        dst[i] = o;
        r += rstep;
        if (r >= m) r -= m;
    }
}

// The cut of a batch of B items at m antennas: runs of `run` items (G = ceil(B / run) <= 256 of them), launches of `chunk` items (a
// multiple of `run`; 2^20 / m^2 items, between 64 and 16,384, so that the R workspace of a chunk stays at 16 MiB).
struct MeanGeometry { uint32_t run, groups, chunk; };
inline MeanGeometry mean_geometry(const uint32_t B, const uint32_t m)
{
    MeanGeometry g;
    g.run = 8u * (uint32_t)(((uint64_t)B + 2047u) / 2048u);
    g.groups = (uint32_t)(((uint64_t)B + g.run - 1u) / g.run);
    uint32_t cap = (1u << 20) / (m * m);
    cap = cap < 64u ? 64u : (cap > 16384u ? 16384u : cap);
    g.chunk = cap <= g.run ? g.run : cap / g.run * g.run;
    return g;
}

constexpr int MEAN_THREADS = 256;
constexpr int MEAN_LOADS = 8;       // loads a lane has in flight (a run is a chain of dependent additions)

// dst[g][e] = scale * sum over the items t of run g (t = g run .. min(items, (g + 1) run) - 1, ascending) of src[t][e].
// Grid: (ceil(ncomp / 256), runs).  scale = 1.0 leaves the sum as it is (level one).
__global__ __launch_bounds__(MEAN_THREADS) void cov_mean_kernel(const double* __restrict__ src, double* __restrict__ dst, const uint32_t items,
                                                                 const uint32_t run, const uint32_t ncomp, const double scale)
{
    const uint32_t e = blockIdx.x * MEAN_THREADS + threadIdx.x;
    if (e >= ncomp) return;
    const uint64_t first = (uint64_t)blockIdx.y * run;
    if (first >= items) return;
    const uint64_t last = first + run < (uint64_t)items ? first + run : (uint64_t)items;     // one past the run's last item
    double acc = 0.0;
    for (uint64_t t0 = first; t0 < last; t0 += MEAN_LOADS) {
        double x[MEAN_LOADS];
#pragma unroll
        for (int k = 0; k < MEAN_LOADS; ++k) {
            const uint64_t t = t0 + k < last ? t0 + k : last - 1;      // (behind the run: reads its last item again, unused)
            x[k] = src[(size_t)t * ncomp + e];
        }
#pragma unroll
        for (int k = 0; k < MEAN_LOADS; ++k)
            if (t0 + k < last) acc = acc + x[k];
    }
    dst[(size_t)blockIdx.y * ncomp + e] = acc * scale;
}

}  // namespace bazcalib
