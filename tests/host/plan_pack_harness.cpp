// plan_pack_harness.cpp -- plan::plan_pack (cufhe_amd/csrc/launch_plan.h) on the CPU, for tests/test_pack.py.  Reads lines
// "count cus pack_slices" and prints, per line, the plan and then every workgroup of its grid as the kernel decodes it
// (pack_keyswitch_kernel reads the same helpers): "wg chunk tile slice first_input inputs i_begin i_end".
// The geometry is the kernel's: tiles of 64 inputs, 8 chunks of 256 row words, n = 630 lvl0 words staged 16 at a time.
#include <cstdio>

#include "../../cufhe_amd/csrc/launch_plan.h"

int main()
{
    const plan::PackGeometry g{64, 8, 630, 16};
    long count, cus, forced;
    while (std::scanf("%ld %ld %ld", &count, &cus, &forced) == 3) {
        plan::Tuning t;
        t.pack_slices = forced;
        const plan::PackPlan p = plan::plan_pack((size_t)count, (int)cus, g, t);
        std::printf("plan %ld %ld %ld tiles %d slices %d grid %u %u max_slices %d\n", count, cus, forced, p.tiles, p.slices, p.grid_x, p.grid_y,
                    plan::pack_max_slices(g));
        for (unsigned x = 0; x < p.grid_x; x++)
            for (unsigned y = 0; y < p.grid_y; y++) {
                const int c = (int)x / p.tiles, tile = (int)x % p.tiles;
                std::printf("wg %d %d %u %ld %d %d %d\n", c, tile, y, plan::pack_tile_first(tile, g.tile), plan::pack_tile_inputs(tile, g.tile, count),
                            plan::pack_slice_begin((int)y, p.slices, g.in_words), plan::pack_slice_begin((int)y + 1, p.slices, g.in_words));
            }
    }
    return 0;
}
