// r4_reduction_search.cpp -- the fewest reductions an inverse transform with the root-product tail needs (ntt_r4.h: InverseRootTail).
// Exhaustive over the registers worth reducing at each of the four places, with the compile-time bounds functions themselves:
//   g++ -std=c++17 -O2 -o r4_reduction_search tools/r4_reduction_search.cpp && ./r4_reduction_search
// prints every improvement it finds, then the masks of the best schedule and the bounds after each pass.  Host only.
#include <cstdio>
#include <vector>

#include "../cufhe_amd/csrc/ntt_r4.h"

using namespace cufhe_amd::r4;

namespace {
int best = 99;
unsigned best_masks[4], cur[4];

RegBounds stage(int lvl, const RegBounds& b)
{
    switch (lvl) {
    case 0: return gs_bounds<false>(xpose_cb_bounds(b));       // C -> B, stages 7-6
    case 1: return gs_bounds<true>(b);                         // stages 5-4
    case 2: return gs_bounds<false>(xpose_all_bounds(b));      // B -> A, stages 3-2
    default: return gs_last_bounds(b);                         // stages 1-0: the root products
    }
}
void search(int lvl, const RegBounds& b, int cost)
{
    if (max_of(b) >= kPoison) return;
    std::vector<int> cand;                                     // reducing a register that is below 0.9 p already buys next to nothing
    for (int r = 0; r < 16; r++)
        if (b.v[r] > 0.9) cand.push_back(r);
    const int n = (int)cand.size();
    for (unsigned m = 0; m < (1u << n); m++) {
        const int pc = __builtin_popcount(m);
        if (cost + pc >= best) continue;
        unsigned mask = 0;
        for (int i = 0; i < n; i++)
            if ((m >> i) & 1u) mask |= 1u << cand[i];
        const RegBounds nb = stage(lvl, reduce_mask_bounds(b, mask));
        if (max_of(nb) >= kPoison) continue;
        cur[lvl] = mask;
        if (lvl == 3) {
            best = cost + pc;
            for (int i = 0; i < 4; i++) best_masks[i] = cur[i];
            printf("%d reductions: masks %04x %04x %04x %04x\n", best, cur[0], cur[1], cur[2], cur[3]);
        } else {
            search(lvl + 1, nb, cost + pc);
        }
    }
}
}  // namespace

int main()
{
    using Sums = PointwiseSum<FwdDigits<32>::Spectrum, 6, true>;      // the sums of blind_rotate_kernel
    const RegBounds c1 = gs_bounds<false>(Sums::in());                // after stages 9-8
    search(0, c1, 0);
    RegBounds b = c1;
    for (int l = 0; l < 4; l++) {
        b = stage(l, reduce_mask_bounds(b, best_masks[l]));
        printf("after pass %d:", l + 2);
        for (int i = 0; i < 16; i++) printf(" %6.3f", b.v[i]);
        printf("\n");
    }
    return 0;
}
