// power_kernels.hip.h -- the opt-in per-emitter Capon power estimate (baz_music_set_power_mode, include/baz_music_hip.h):
// P = 1 / Re(a^H R^-1 a) for every reported entry, from the covariance R the item's EVD decomposed and the entry's steering row a.
//
//   power_pivot_floor / power_pivot_ok   the degeneracy rule, __host__ __device__: power_kernel and baz_music_power_estimate() compile
//   power_from_s                         the same text, and so for the final s -> P step; testable without a device.
//   power_kernel<M>                      one item per group of W lanes (W = 4 / 8 / 16 for M <= 4 / 8 / 16), the last launch of a sequence.
//
// DEFINITION.  Unpivoted LDL^H of R in fp64 from the lower triangle as stored, the imaginary part of the diagonal ignored:
//     d_j  = Re R_jj - sum_{k<j} |L_jk|^2 d_k
//     L_ij = (R_ij - sum_{k<j} L_ik conj(L_jk) d_k) / d_j        (i > j)
//     z_i  = a_i - sum_{k<i} L_ik z_k                            (a: the table row, complex64 widened exactly)
//     s    = sum_i |z_i|^2 / d_i,     P = 1 / s
// An item is DEGENERATE when some d_j is not finite or d_j <= 2^-40 (sum_i Re R_ii) / m: all its entries get P = 0.  An entry whose s
// is 0 or not finite gets P = 0.  Missing entries (lvl == 0) get 0.
//
// LAYOUT.  Lane r of a group owns row r of R (M complex doubles in registers; a group's load is one contiguous 16 M^2-byte run, every
// byte of every line it touches used by the group).  The factorisation is column by column: at column j every lane forms its own
// R_ij - sum_k ... with the pivot row's L_jk broadcast from lane j by width-W shuffles (ds_bpermute inside the group; a group never
// crosses a 16-lane row), lane j's value is the pivot, broadcast again.  Lanes above the diagonal compute values nobody reads.
// Then, per entry of the item: lane i gathers a_i (the group reads M contiguous complex64), forward substitution with z_k broadcast
// from lane k, a butterfly sum of |z_i|^2 / d_i over the group.  R is read once and factorised once per item.  Results of entry e are
// kept by lane e of the group (n < M <= W) and stored after the loop: the stores of a wave are unit-stride.  No LDS, no scratch.
// A degenerate item, an item beyond the batch or a lane beyond M runs the same instructions on zeros / garbage and only its stores
// differ: no lane leaves before the last shuffle, so a neighbour group of the wave is never disturbed.
// Entries are read from the device-side staging copy the pickers wrote (ang on the GRID: refine_kernel never writes there) and the
// results go to the caller's buffers with plain stores -- nothing is read back from the caller's (possibly host-mapped) memory.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bazpower {

// the pivot floor of an item: 2^-40 of the mean diagonal (BAZ_MUSIC_POWER_PIVOT_FLOOR; the emitter-count mode's clamp)
__host__ __device__ inline double power_pivot_floor(const double trace, const uint32_t m, const double rel_floor)
{
    return rel_floor * (trace / (double)m);
}

// whether pivot d keeps the item alive: finite and above the floor (a NaN floor -- R holds NaN / Inf on its diagonal -- fails too)
__host__ __device__ inline bool power_pivot_ok(const double d, const double floor)
{
    return (d - d == 0.0) && d > floor;
}

// s = a^H R^-1 a -> P
__host__ __device__ inline double power_from_s(const double s)
{
    if (!(s - s == 0.0) || s == 0.0) return 0.0;
    return 1.0 / s;
}

struct PowerArgs {
    const float* ang_in;       // [batch * n] what the merge / picker / truncation left (device staging), on the grid
    const float* lvl_in;       // [batch * n] ... lvl != 0 marks a real entry
    float* ang_out;            // [batch * n] the caller's ang, or nullptr (refine_kernel writes it)
    float* lvl_out;            // [batch * n] the caller's lvl, or nullptr (port 1 not wired, or refine_kernel writes it)
    double* pow_out;           // [batch * n] P per entry (baz_music_last_powers)
    const double2* R;          // [batch][M][M] the covariances the EVD read, row-major
    const float2* raw;         // the raw table in force, [res][M] complex64
    double rel_floor;          // BAZ_MUSIC_POWER_PIVOT_FLOOR
    uint32_t batch, n, res;
    int lvl_is_power;          // mode 2: lvl_out carries (float)P instead of the staged bits
};

template <int M>
struct PowerGeom {
    static constexpr int W = M <= 4 ? 4 : (M <= 8 ? 8 : 16);    // lanes per item
    static constexpr int IPB = 256 / W;                         // items per 256-thread block
};

__device__ inline double group_bcast(const double v, const int src, const int width) { return __shfl(v, src, width); }

template <int M>
__global__ __launch_bounds__(256) void power_kernel(const PowerArgs A)
{
    constexpr int W = PowerGeom<M>::W;
    const uint32_t r = threadIdx.x % W;                                     // this lane's row
    const uint64_t item = (uint64_t)blockIdx.x * PowerGeom<M>::IPB + threadIdx.x / W;
    const bool live = item < A.batch;                                       // (uniform over the group)
    const bool rowlane = live && r < (uint32_t)M;
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
    // the floor: the diagonal summed in index order (what the host routine does)
    double trace = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) trace += group_bcast(lr[j], j, W);
    const double floor = power_pivot_floor(trace, (uint32_t)M, A.rel_floor);
    // LDL^H, column by column
    double d[M];
    bool ok = true;
    double dmine = 1.0;                                                     // d_r
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double vr = lr[j], vi = li[j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            const double pr = group_bcast(lr[k], j, W), pi = group_bcast(li[k], j, W);      // L_jk
            // L_ik conj(L_jk) d_k
            const double wr = pr * d[k], wi = pi * d[k];
            vr -= lr[k] * wr + li[k] * wi;
            vi -= li[k] * wr - lr[k] * wi;
        }
        const double dj = group_bcast(vr, j, W);                            // lane j's value is the pivot (its imaginary part ignored)
        d[j] = dj;
        ok = ok && power_pivot_ok(dj, floor);
        if (r == (uint32_t)j) dmine = dj;
        lr[j] = vr / dj;
        li[j] = vi / dj;
    }
    // the item's entries
    double mine = 0.0;                                                      // lane e keeps entry e
    float ang_mine = 0.0f, lvl_mine = 0.0f;
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
        const double P = (ok && l_in != 0.0f) ? power_from_s(s) : 0.0;
        if (r == e) { mine = P; ang_mine = a_in; lvl_mine = l_in; }
    }
    if (live && r < A.n) {
        const size_t t = (size_t)item * A.n + r;
        A.pow_out[t] = mine;
        if (A.ang_out) A.ang_out[t] = ang_mine;
        if (A.lvl_out) A.lvl_out[t] = A.lvl_is_power ? (float)mine : lvl_mine;
    }
}

}  // namespace bazpower
