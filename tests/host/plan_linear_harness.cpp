// plan_linear_harness.cpp -- plan::plan_linear (cufhe_amd/csrc/launch_plan.h) on the CPU, for tests/test_linear.py.  Reads lines
// "rows cols sets words cus" and prints, per line, the plan and how its grid covers the outputs: every (workgroup, wave, register, lane)
// is decoded as linear_kernel decodes it (the kernel reads the same helpers), a cell that the kernel would store -- its wave below
// `waves`, its row below `rows`, its word below `words` -- is counted at (set, row, word), and one whose set is not below `sets`
// is counted as outside.
//   plan rows cols sets words cus  row_tile R unroll U row_tiles T chunks C waves W per_block B grid G block X  cover MIN MAX outside O
#include <cstdio>
#include <vector>

#include "../../cufhe_amd/csrc/launch_plan.h"

int main()
{
    long rows, cols, sets, words, cus;
    while (std::scanf("%ld %ld %ld %ld %ld", &rows, &cols, &sets, &words, &cus) == 5) {
        const plan::LinearPlan p = plan::plan_linear((size_t)rows, (size_t)cols, (size_t)sets, (int)words, (int)cus);
        std::vector<int> cover((size_t)(sets * rows * words), 0);
        long outside = 0;
        const int waves_in_block = (int)p.block_x / plan::kLinearWaveWords;
        for (long b = 0; b < (long)p.grid_x; b++)
            for (int w = 0; w < waves_in_block; w++) {
                const long wave = plan::linear_wave_of(b, w, waves_in_block);
                if (wave >= p.waves) continue;
                const int tile = plan::linear_wave_tile(wave, p.row_tiles), chunk = plan::linear_wave_chunk(wave, p.row_tiles, p.chunks);
                const long set = plan::linear_wave_set(wave, p.row_tiles, p.chunks);
                for (int j = 0; j < p.row_tile; j++)
                    for (int l = 0; l < plan::kLinearWaveWords; l++) {
                        const long row = plan::linear_row(tile, j), i = plan::linear_word(chunk, l);
                        if (row >= rows || i >= words) continue;
                        if (set < 0 || set >= sets) { outside++; continue; }
                        cover[(size_t)((set * rows + row) * words + i)]++;
                    }
            }
        int lo = cover.empty() ? 1 : cover[0], hi = cover.empty() ? 1 : cover[0];
        for (int c : cover) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
        std::printf("plan %ld %ld %ld %ld %ld row_tile %d unroll %d row_tiles %d chunks %d waves %ld per_block %d grid %u block %u cover %d %d outside %ld\n",
                    rows, cols, sets, words, cus, p.row_tile, p.unroll, p.row_tiles, p.chunks, p.waves, p.waves_per_block, p.grid_x, p.block_x, lo, hi,
                    outside);
    }
    return 0;
}
