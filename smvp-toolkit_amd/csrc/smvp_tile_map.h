// smvp_tile_map.h -- which tile a workgroup of a tile-kernel launch takes.  No HIP includes: the host compiles it alone
// (tests/tile_map_check.cpp walks every grid the library can launch).
#pragma once

#if defined(__HIPCC__)
#define SMVP_HOST_DEVICE __host__ __device__
#else
#define SMVP_HOST_DEVICE
#endif

namespace smvp {

// Tiles per XCD turn for a launch of `ntiles` tiles: `wanted`, smaller for small matrices so that the grid (rounded up to a
// multiple of 8 * group) is not mostly empty blocks.
inline int tile_group_of(int ntiles, int wanted)
{
    const int fit = ntiles / 64;
    return fit < 1 ? 1 : (fit < wanted ? fit : wanted);
}

// grid of a launch of `ntiles` tiles: whole rounds of 8 * group workgroups
inline unsigned tile_grid_of(int ntiles, int group) { return (unsigned)((ntiles + 8 * group - 1) / (8 * group)) * 8u * group; }

// Blocks are dealt round-robin over the 8 XCDs; XCD i takes `group` consecutive tiles out of every run of 8 * group
// (the measurements are beside K2 in smvp_kernels.hip).  A permutation of every round of 8 * group blocks, hence of
// [0, grid) for a grid of whole rounds.
SMVP_HOST_DEVICE inline __attribute__((always_inline)) int tile_of_block(int block, int group)
{
    const int xcd = block & 7, seq = block >> 3;
    return (seq / group) * (8 * group) + xcd * group + seq % group;
}

// The same deal in either direction of the sweep.  back_grid = 0: forward.  back_grid = the launch's grid (a multiple of
// 8 * group): backward -- block b takes what block grid - 1 - b takes forward, so the workgroups dispatched first take the
// highest tiles, where the product before this one (a forward one) ended and what it left in the Infinity Cache lies.  The
// XCD turns stay whole: grid is a multiple of 8, so XCD i takes the groups XCD 7 - i had.  Speed only: every tile is still
// taken exactly once, and a tile's sums do not depend on who else runs.
SMVP_HOST_DEVICE inline __attribute__((always_inline)) int tile_of_block_swept(int block, int group, int back_grid)
{
    return tile_of_block(back_grid ? back_grid - 1 - block : block, group);
}

}  // namespace smvp
