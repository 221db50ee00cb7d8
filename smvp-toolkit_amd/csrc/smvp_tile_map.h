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
// (the measurements are beside K2' in smvp_owner_kernel.h).  A permutation of every round of 8 * group blocks, hence of
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

// Phase 1 of the tile kernel, row-ordered flavours, tiles of 256 * vpt entries (vpt 4 or 8): the offset in the tile of entry k
// (0 ... vpt - 1) of thread t.  A wavefront takes 64 * vpt consecutive entries in slabs of 128; of every slab lane l has the
// two entries 2 l and 2 l + 1 (owner_body's lane_entry).
SMVP_HOST_DEVICE inline __attribute__((always_inline)) int tile_lane_entry(int t, int k, int vpt)
{
    return (t >> 6) * (64 * vpt) + 2 * (t & 63) + 128 * (k >> 1) + (k & 1);
}

// Where the plan keeps the 16-bit column offset of the entry at offset o of a full, narrow tile (column_offsets writes it there,
// owner_body reads it from there): in the order the lanes hold the entries, so that the vpt offsets of a lane are one load.
// The inverse of tile_lane_entry: col16_slot(tile_lane_entry(t, k, vpt), vpt) = (t >> 6) * 64 * vpt + (t & 63) * vpt + k.
// A permutation inside every wavefront's chunk of 64 * vpt entries, hence inside the tile.
// The library lays out the 2048-entry tiles this way (vpt 8); the formula holds for vpt 4 as well.
constexpr int kCol16LaneOrderTile = 2048;
SMVP_HOST_DEVICE inline __attribute__((always_inline)) int col16_slot(int o, int vpt)
{
    const int chunk = 64 * vpt;
    const int w = o / chunk, q = o % chunk, l = (q % 128) / 2, k = 2 * (q / 128) + (q & 1);
    return w * chunk + l * vpt + k;
}

// The packed values of the same tiles (kFlavorCsr16P): one code per entry, kept in col16_slot order too -- an index into the hot
// table, one entry per lane of a wavefront, or the escape code.
constexpr int kHotValues = 64;
constexpr int kEscapeCode = 255;

}  // namespace smvp
