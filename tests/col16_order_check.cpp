// col16_order_check.cpp -- host check of csrc/smvp_tile_map.h's col16_slot: where the plan keeps the 16-bit column offset of
// every entry of a full, narrow tile, so that the tile kernel's lane reads its VPT offsets with one load.  A program of its own
// (tests/test_col16_order_host.py compiles it with the host compiler alone, under AddressSanitizer and
// UndefinedBehaviorSanitizer where the toolchain has them, and runs it).  For tiles of 256 * VPT entries, VPT 4 and 8:
//   the slot function is a bijection of [0, 256 * VPT);
//   every slot stays inside its entry's chunk of 64 * VPT entries (one wavefront's);
//   the VPT entries of a lane -- the header's tile_lane_entry, held here against the formula written out -- have VPT
//   consecutive slots that start at a multiple of VPT, in the order k = 0 ... VPT - 1:
//   col16_slot(tile_lane_entry(t, k)) == (t >> 6) * 64 * VPT + (t & 63) * VPT + k for every thread t < 256.
#include <cstdio>
#include <vector>

#include "smvp_tile_map.h"

static int fail(const char *what, int vpt, int a, int b, int got)
{
    printf("FAIL %s: VPT %d, %d, %d -> %d\n", what, vpt, a, b, got);
    return 1;
}

static int check(int vpt, long long *checked)
{
    const int tile = 256 * vpt, chunk = 64 * vpt;
    std::vector<int> seen((size_t)tile, 0), entry_seen((size_t)tile, 0);
    for (int o = 0; o < tile; ++o) {
        const int slot = smvp::col16_slot(o, vpt);
        if (slot < 0 || slot >= tile)
            return fail("the slot leaves the tile", vpt, o, -1, slot);
        if (slot / chunk != o / chunk)
            return fail("the slot leaves its wavefront's chunk", vpt, o, -1, slot);
        ++seen[(size_t)slot];
    }
    for (int s = 0; s < tile; ++s)
        if (seen[(size_t)s] != 1)
            return fail("not a bijection: entries that take this slot", vpt, s, -1, seen[(size_t)s]);
    for (int t = 0; t < 256; ++t) {
        const int first = smvp::col16_slot(smvp::tile_lane_entry(t, 0, vpt), vpt);
        if (first % vpt != 0)
            return fail("a lane's slots do not start at a multiple of VPT", vpt, t, 0, first);
        for (int k = 0; k < vpt; ++k) {
            const int o = smvp::tile_lane_entry(t, k, vpt);
            // the formula written out: wavefront t / 64 takes 64 * VPT entries in slabs of 128, lane l entries 2 l, 2 l + 1 of slab k / 2
            const int wave = t / 64, lane = t % 64, want_o = wave * 64 * vpt + 128 * (k / 2) + 2 * lane + k % 2;
            if (o != want_o || o < 0 || o >= tile)
                return fail("tile_lane_entry", vpt, t, k, o);
            ++entry_seen[(size_t)o];
            const int slot = smvp::col16_slot(o, vpt);
            if (slot != first + k)
                return fail("a lane's slots are not consecutive in k", vpt, t, k, slot);
            if (slot != (t >> 6) * 64 * vpt + (t & 63) * vpt + k)
                return fail("the slot is not where the lane loads from", vpt, t, k, slot);
            ++*checked;
        }
    }
    for (int o = 0; o < tile; ++o)
        if (entry_seen[(size_t)o] != 1)
            return fail("tile_lane_entry does not give every entry to one (thread, k)", vpt, o, -1, entry_seen[(size_t)o]);
    return 0;
}

int main()
{
    long long checked = 0;
    for (int vpt : {4, 8})
        if (check(vpt, &checked))
            return 1;
    printf("col16 order ok: %lld (thread, entry) pairs checked\n", checked);
    return 0;
}
