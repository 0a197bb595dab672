// capon_solve.hip.h -- the one Capon solve behind the opt-in power mode (power_kernels.hip.h) and the opt-in beam mode
// (beam_kernels.hip.h): a^H R^-1 a and R^-1 a for the steering row a of every reported entry, from the covariance R the item's EVD
// decomposed.
//
//   power_pivot_floor / power_pivot_ok   the degeneracy rule, __host__ __device__: the kernels and HostSolve compile the same text,
//   power_from_s / beam_w_from_u         and so for the final s -> P and (u, s) -> w steps; testable without a device.
//   staged_bin                           the bin of a staged angle (refine_kernel, power_kernel, beam_weights_kernel).
//   capon_kernel<M, .., BEAM, Args>      one item per group of W lanes (W = 4 / 8 / 16 for M <= 4 / 8 / 16): power_kernel<M> and
//                                        beam_weights_kernel<M> are its two instances.
//   HostSolve                            the definition on the host, loop for loop (baz_music_power_estimate, baz_music_beam_weights).
//
// DEFINITION.  Unpivoted LDL^H of R in fp64 from the lower triangle as stored, the imaginary part of the diagonal ignored:
//     d_j  = Re R_jj - sum_{k<j} |L_jk|^2 d_k
//     L_ij = (R_ij - sum_{k<j} L_ik conj(L_jk) d_k) / d_j        (i > j)
//     z_i  = a_i - sum_{k<i} L_ik z_k                            (a: the table row, complex64 widened exactly)
//     s    = sum_i |z_i|^2 / d_i
// An item is DEGENERATE when some d_j is not finite or d_j <= 2^-40 (sum_i Re R_ii) / m: all its entries are dead.  An entry whose s
// is 0 or not finite is dead.  Missing entries (lvl == 0) are dead.  What a mode reports for a dead entry and what it makes of z, d
// and s is stated in its own header.
//
// LAYOUT.  Lane r of a group owns row r of R (M complex doubles in registers; a group's load is one contiguous 16 M^2-byte run, every
// byte of every line it touches used by the group).  The factorisation is column by column: at column j every lane forms its own
// R_ij - sum_k ... with the pivot row's L_jk broadcast from lane j by width-W shuffles (ds_bpermute inside the group; a group never
// crosses a 16-lane row), lane j's value is the pivot, broadcast again.  Lanes above the diagonal compute values nobody reads.
// Then, per entry of the item: lane i gathers a_i (the group reads M contiguous complex64), forward substitution with z_k broadcast
// from lane k, a butterfly sum of |z_i|^2 / d_i over the group.  R is read once and factorised once per item.  The caller's ang / lvl
// of entry e are kept by lane e of the group (n < M <= W) and stored after the loop: the stores of a wave are unit-stride.
// A degenerate item, an item beyond the batch or a lane beyond M runs the same instructions on zeros / garbage and only its stores
// differ: no lane leaves before the last shuffle, so a neighbour group of the wave is never disturbed.
// Entries are read from the device-side staging copy the pickers wrote (ang on the GRID: refine_kernel never writes there) and the
// results go to the caller's buffers with plain stores -- nothing is read back from the caller's (possibly host-mapped) memory.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace bazcapon {

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

// u, s -> w = u / s; an s that is 0 or not finite (or a dead item / missing entry: alive == false) gives w = 0
__host__ __device__ inline void beam_w_from_u(const double ur, const double ui, const double s, const bool alive, double* wr, double* wi)
{
    const bool good = alive && (s - s == 0.0) && s != 0.0;
    *wr = good ? ur / s : 0.0;
    *wi = good ? ui / s : 0.0;
}

// the bin of a staged angle: ang = (float)(b 360 / res) is within 2^-24 relative of b 360 / res, so up to 2^20 bins the product is
// within 1/16 of b
__device__ __forceinline__ uint32_t staged_bin(const float ang, const uint32_t res)
{
    uint32_t b = (uint32_t)__double2ll_rn((double)ang * (double)res / 360.0);
    b = b < res ? b : res - 1u;
    return b;
}

template <int M>
struct Group {
    static constexpr int W = M <= 4 ? 4 : (M <= 8 ? 8 : 16);    // lanes per item
    static constexpr int S = M | 1;                             // row pitch of the beam mode's L^H tile, in complex128
};

__device__ inline double group_bcast(const double v, const int src, const int width) { return __shfl(v, src, width); }

// One item per group of W lanes, IPB items per block of THREADS: power_kernel<M> (BEAM == false, Args = PowerArgs) and
// beam_weights_kernel<M> (BEAM == true, Args = BeamWeightsArgs).  The two Args share the fields this body reads outside its
// `if constexpr (BEAM)` blocks (capon_args of baz_music_hip.hip fills them); what a block reads is its mode's own, and so are the
// loading, the L^H tile, the barrier, the back substitution and the w store (beam) and P (power).  One kernel body, not device
// functions handing the row arrays on: so the two instances compile to the instructions the two copies compiled to
// (profiles/opt_in_shared_solve.txt; a row load or a column loop behind a call costs copies of the row registers).
template <int M, int THREADS, int IPB, bool BEAM, class Args>
__global__ __launch_bounds__(THREADS) void capon_kernel(const Args A)
{
    constexpr int W = Group<M>::W, S = Group<M>::S;
    const uint32_t r = threadIdx.x % W;                                     // this lane's row
    const uint64_t item = (uint64_t)blockIdx.x * IPB + threadIdx.x / W;
    const bool live = item < A.batch;                                       // (uniform over the group)
    const bool rowlane = live && r < (uint32_t)M;
    double2* lt = nullptr;                                                  // beam mode: this group's L^H tile
    if constexpr (BEAM) {
        __shared__ double2 LT[IPB * M * S];
        lt = LT + (threadIdx.x / W) * (M * S);
    }
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
    // the floor: the diagonal summed in index order (what the host routine does); beam mode: the loading first, from the same sum, and
    // the floor from the loaded diagonal (selected at compile time: the power mode adds nothing, not even 0.0)
    double trace = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) trace += group_bcast(lr[j], j, W);
    if constexpr (BEAM) {
        const double delta = A.loading * (trace / (double)M);
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (r == (uint32_t)j) lr[j] += delta;
        trace = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) trace += group_bcast(lr[j], j, W);
    }
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
    if constexpr (BEAM) {                                                   // L^H: row r of L into the tile, read back by columns below
        if (r < (uint32_t)M) {
#pragma unroll
            for (int k = 0; k < M; ++k) lt[r * S + k] = make_double2(lr[k], li[k]);
        }
        __syncthreads();
    }
    // the item's entries
    double mine = 0.0;                                                      // lane e keeps entry e (power mode: with its P)
    float ang_mine = 0.0f, lvl_mine = 0.0f;
    for (uint32_t e = 0; e < A.n; ++e) {
        const size_t t = (size_t)(live ? item : 0) * A.n + e;
        const float a_in = A.ang_in[t], l_in = A.lvl_in[t];
        const uint32_t b = staged_bin(a_in, A.res);
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
        if constexpr (BEAM) {
            double ur = r < (uint32_t)M ? zr / dmine : 0.0, ui = r < (uint32_t)M ? zi / dmine : 0.0;
#pragma unroll
            for (int k = M - 1; k > 0; --k) {
                const double kr = group_bcast(ur, k, W), ki = group_bcast(ui, k, W);        // u_k, final in lane k
                const double2 c = lt[r < (uint32_t)k ? k * S + (int)r : 0];                 // L_kr
                if (r < (uint32_t)k) {                                                      // conj(L_kr) u_k
                    ur -= c.x * kr + c.y * ki;
                    ui -= c.x * ki - c.y * kr;
                }
            }
            double wr, wi;
            beam_w_from_u(ur, ui, s, ok && l_in != 0.0f, &wr, &wi);
            if (rowlane) A.w_out[t * M + r] = make_double2(wr, wi);
            if (r == e) { ang_mine = a_in; lvl_mine = l_in; }
        } else {
            const double P = (ok && l_in != 0.0f) ? power_from_s(s) : 0.0;
            if (r == e) { mine = P; ang_mine = a_in; lvl_mine = l_in; }
        }
    }
    if (live && r < A.n) {
        const size_t t = (size_t)item * A.n + r;
        if constexpr (!BEAM) A.pow_out[t] = mine;
        if (A.ang_out) A.ang_out[t] = ang_mine;
        if constexpr (BEAM) {
            if (A.lvl_out) A.lvl_out[t] = lvl_mine;
        } else {
            if (A.lvl_out) A.lvl_out[t] = A.lvl_is_power ? (float)mine : lvl_mine;
        }
    }
}

// The definition on the host for one R (m x m complex128, interleaved) and any number of steering rows: the factorisation once, then
// solve() per row.  loading == nullptr is the power mode's R as stored; else *loading (sum_i Re R_ii) / m is added to the real diagonal
// first and the floor is taken on the loaded diagonal.  The unloaded path adds nothing (not even 0.0): R_ii + 0.0 is not R_ii for
// -0.0, and 0 (trace / m) is NaN for a trace that is not finite.
struct HostSolve {
    const uint32_t m;
    bool ok = true;            // false: a pivot failed (the item is degenerate; L and d are then incomplete)
    std::vector<double> Lr, Li, d, zr, zi;

    HostSolve(const uint32_t m_, const double* R_ri, const double* loading, const double rel_floor)
        : m(m_), Lr((size_t)m_ * m_, 0.0), Li((size_t)m_ * m_, 0.0), d(m_, 0.0), zr(m_), zi(m_)
    {
        std::vector<double> dg(m);
        double trace = 0.0;
        for (uint32_t i = 0; i < m; ++i) trace += (dg[i] = R_ri[2 * ((size_t)i * m + i)]);
        if (loading) {
            const double delta = *loading * (trace / (double)m);
            trace = 0.0;
            for (uint32_t i = 0; i < m; ++i) trace += (dg[i] += delta);
        }
        const double floor = power_pivot_floor(trace, m, rel_floor);
        for (uint32_t j = 0; j < m && ok; ++j) {
            for (uint32_t i = j; i < m; ++i) {
                double vr = i == j ? dg[i] : R_ri[2 * ((size_t)i * m + j)], vi = i == j ? 0.0 : R_ri[2 * ((size_t)i * m + j) + 1];
                for (uint32_t k = 0; k < j; ++k) {     // L_ik conj(L_jk) d_k
                    const double wr = Lr[(size_t)j * m + k] * d[k], wi = Li[(size_t)j * m + k] * d[k];
                    vr -= Lr[(size_t)i * m + k] * wr + Li[(size_t)i * m + k] * wi;
                    if (i != j) vi -= Li[(size_t)i * m + k] * wr - Lr[(size_t)i * m + k] * wi;
                }
                if (i == j) {
                    d[j] = vr;
                    ok = power_pivot_ok(vr, floor);
                    if (!ok) break;
                } else {
                    Lr[(size_t)i * m + j] = vr / d[j];
                    Li[(size_t)i * m + j] = vi / d[j];
                }
            }
        }
    }

    // z of the row a (m complex64, interleaved) into zr / zi; returns s.  Only while ok.
    double solve(const float* a)
    {
        double s = 0.0;
        for (uint32_t i = 0; i < m; ++i) {
            double xr = (double)a[2 * i], xi = (double)a[2 * i + 1];
            for (uint32_t k = 0; k < i; ++k) {
                xr -= Lr[(size_t)i * m + k] * zr[k] - Li[(size_t)i * m + k] * zi[k];
                xi -= Lr[(size_t)i * m + k] * zi[k] + Li[(size_t)i * m + k] * zr[k];
            }
            zr[i] = xr; zi[i] = xi;
            s += (xr * xr + xi * xi) / d[i];
        }
        return s;
    }
};

}  // namespace bazcapon
