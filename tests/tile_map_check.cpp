// tile_map_check.cpp -- host check of csrc/smvp_tile_map.h: which tile a workgroup of the tile kernel takes, forward and backward.
// A program of its own (tests/test_tile_map.py compiles it with the host compiler alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer where the toolchain has them, and runs it): for every tile count 1 ... 5000 and the group the
// launcher picks for it (CSR: up to 64 tiles per XCD turn, TJDS: up to 32), and for EVERY group 1 ... 64 on the small counts and
// the edges, the blocks of the padded grid map one-to-one onto [0, grid) in either direction, backward is forward reversed,
// XCD i takes backward the groups XCD 7 - i takes forward, and the blocks dispatched first take the highest round of tiles.
// With the argument "grids" it checks nothing and prints, for every tile count 1 ... 5000, the group and the grid the launcher
// picks for CSR and for TJDS: "ntiles group grid group grid" (tests/test_timed_runs_host.py holds its Python mirror to them).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smvp_tile_map.h"

static long long g_checked = 0;

static int fail(const char *what, int ntiles, int group, int grid, int block, int got)
{
    printf("FAIL %s: ntiles %d group %d grid %d block %d -> %d\n", what, ntiles, group, grid, block, got);
    return 1;
}

static int check(int ntiles, int group)
{
    const int grid = (int)smvp::tile_grid_of(ntiles, group);
    const int round = 8 * group;
    if (grid % round != 0 || grid < ntiles || grid - ntiles >= round)
        return fail("grid is not ntiles rounded up to whole rounds", ntiles, group, grid, -1, grid);
    std::vector<int> fwd((size_t)grid), seen_f((size_t)grid, 0), seen_b((size_t)grid, 0);
    for (int b = 0; b < grid; ++b) {
        const int t = smvp::tile_of_block_swept(b, group, 0);
        if (t != smvp::tile_of_block(b, group))
            return fail("forward differs from tile_of_block", ntiles, group, grid, b, t);
        if (t < 0 || t >= grid)
            return fail("forward leaves [0, grid)", ntiles, group, grid, b, t);
        if ((t / group) % 8 != (b & 7))
            return fail("forward: the tile is not in a group of XCD block % 8", ntiles, group, grid, b, t);
        if (t / round != b / round)
            return fail("forward: the tile is not in the block's round", ntiles, group, grid, b, t);
        fwd[(size_t)b] = t;
        ++seen_f[(size_t)t];
    }
    for (int b = 0; b < grid; ++b) {
        const int t = smvp::tile_of_block_swept(b, group, grid);
        if (t < 0 || t >= grid)
            return fail("backward leaves [0, grid)", ntiles, group, grid, b, t);
        if (t != fwd[(size_t)(grid - 1 - b)])
            return fail("backward is not forward reversed", ntiles, group, grid, b, t);
        if ((t / group) % 8 != 7 - (b & 7))
            return fail("backward: the tile is not in a group XCD 7 - block % 8 had", ntiles, group, grid, b, t);
        if (t / round != (grid - 1 - b) / round)
            return fail("backward: the blocks dispatched first do not take the highest round", ntiles, group, grid, b, t);
        ++seen_b[(size_t)t];
    }
    for (int t = 0; t < grid; ++t)
        if (seen_f[(size_t)t] != 1 || seen_b[(size_t)t] != 1)
            return fail(seen_f[(size_t)t] != 1 ? "forward is not one-to-one" : "backward is not one-to-one", ntiles, group, grid, -1, t);
    g_checked += grid;
    return 0;
}

int main(int argc, char **argv)
{
    const int wanted[2] = {64, 32};  // kStreamTileGroup, kTjdsTileGroup (smvp_kernels.h)
    if (argc > 1 && strcmp(argv[1], "grids") == 0) {
        for (int ntiles = 1; ntiles <= 5000; ++ntiles) {
            const int g0 = smvp::tile_group_of(ntiles, wanted[0]), g1 = smvp::tile_group_of(ntiles, wanted[1]);
            printf("%d %d %u %d %u\n", ntiles, g0, smvp::tile_grid_of(ntiles, g0), g1, smvp::tile_grid_of(ntiles, g1));
        }
        return 0;
    }
    for (int ntiles = 1; ntiles <= 5000; ++ntiles) {
        for (int w : wanted) {
            const int group = smvp::tile_group_of(ntiles, w);
            if (group < 1 || group > w || (ntiles >= 64 * w && group != w) || (ntiles < 128 && group != 1))
                return fail("tile_group_of", ntiles, group, 0, -1, w);
            if (check(ntiles, group))
                return 1;
        }
        const bool edge = ntiles <= 320 || (ntiles >= 4090 && ntiles <= 4100) || ntiles == 4609 || ntiles == 5000;
        if (edge)
            for (int group = 1; group <= 64; ++group)
                if (check(ntiles, group))
                    return 1;
    }
    printf("tile map ok: %lld blocks checked\n", g_checked);
    return 0;
}
