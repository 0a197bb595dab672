// power_kernels.hip.h -- the opt-in per-emitter Capon power estimate (baz_music_set_power_mode, include/baz_music_hip.h):
// P = 1 / Re(a^H R^-1 a) for every reported entry, from the covariance R the item's EVD decomposed and the entry's steering row a.
//
//   power_kernel<M>                      one item per group of W lanes, the last launch of a sequence.
//
// DEFINITION, LAYOUT.  capon_solve.hip.h states the solve (d, L, z, s, the degeneracy rule) and how a group of lanes runs it; this
// kernel is capon_kernel without its beam blocks: the solve on R as stored, and P = 1 / s (power_from_s).  A dead entry gets P = 0.
// P of entry e is kept by lane e of the group beside the entry's ang / lvl and stored after the loop.  No LDS, no scratch.
// gfx950 only (the device side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capon_solve.hip.h"

namespace bazpower {

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
    static constexpr int W = bazcapon::Group<M>::W;             // lanes per item
    static constexpr int IPB = 256 / W;                         // items per 256-thread block
};

template <int M>
inline constexpr auto power_kernel = &bazcapon::capon_kernel<M, 256, PowerGeom<M>::IPB, false, PowerArgs>;

}  // namespace bazpower
