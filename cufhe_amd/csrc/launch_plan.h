// launch_plan.h -- every rule that cuts a batch into launches: which kernel, over which part of the batch, in which shape.
// Host only, standard library only, no allocation: capi.hip and its .inc.h files turn the plans into launches, the scheduler's
// backend (sched_hip.inc.h) prices its levels with the same plans, and tests/host/launch_plan_harness.cpp prints them on the CPU
// (tests/test_launch_plan.py: the plans of the code this header replaced, tests/golden/launch_plans_v1.json; plan_pack:
// tests/host/plan_pack_harness.cpp, tests/test_pack.py; plan_linear: tests/host/plan_linear_harness.cpp, tests/test_linear.py).
//
// Every rule is in units of the device's CU count (MI355X: 256; the measured milliseconds in the comments are that chip's).
#pragma once

#include <algorithm>
#include <cstddef>

namespace plan {

// no CU count known (the device attribute could not be read): the rules behave as on MI355X
inline size_t device_cus(int cus) { return cus > 0 ? (size_t)cus : 256; }

constexpr int kBatchWaves = 8;     // rotations per workgroup of the batch kernel (kBrWavesPerBlock)
constexpr int kKsMaxPerWg = 16;    // ciphertexts per workgroup of the shared-table key switch, at most (kKsWaves)

// The options of cufhe_amd_set_option that tune the rules below; -1 = the measured rule.
struct Tuning {
    long ll_threshold = -1;        // rotations per launch up to which the 16-wave split-transform kernel is used; -1: by measured cost
    long ll2_threshold = -1;       // two-rotations-per-workgroup low-latency kernel: -1 by cost, 0 never, > 0 for launches up to this size
    long half_threshold = -1;      // ... up to which the batch kernel runs one rotation per SIMD (4 per workgroup); -1: by measured cost
    long tail_split = 1;           // 1: launches above one grid round are cut into full rounds + a tail that takes the cheapest kernel
    long ks_split_threshold = -1;  // key switches per launch up to which each ciphertext is split over 8 workgroups
    long ks_wg_threshold = -1;     // key switches per launch up to which the workgroup-per-ciphertext kernel is used
    long ks_per_wg = -1;           // ciphertexts per workgroup of the shared-table key switch: -1 by count, else 1..16
    long ks_slices = -1;           // runs the shared-table key switch cuts j into: -1 by count, else a power of two 1..64
    long ps_batch_threshold = -1;  // parameter sets: rotations per launch from which the wave-per-rotation kernel is used (-1: by cost)
    // N = 2048 blind rotation: 1 = four quarter waves per rotation, two rotations per CU (kernels_lvl2q.hip.h); 0 = eight half waves, one
    // rotation per CU (kernels_lvl2.hip.h); -1 = by measured cost: a launch that leaves CUs with a single rotation (<= one per CU) is
    // faster on the eight-wave kernel (256 rotations: 14.5 ms against 17.4), everything above on the four-wave one (512: 27.3 against 28.0,
    // 4096: 192 against 223)
    long lvl2_kernel = -1;
    long pack_slices = -1;         // TLWE packing: slices of i per tile of inputs (plan_pack); -1 by the rule, else clamped to 1 .. max
    long ks_mm_threshold = -1;     // lvl10 key switches per launch from which the matrix-product kernel runs: -1 by the measured rule, 0 never
};

// ---- blind rotation (kN = 1024, the default path) ----

enum class BrKernel { Batch, Ll, Ll2 };     // blind_rotate_kernel, blind_rotate_ll_kernel (a workgroup per rotation), blind_rotate_ll2_kernel (two)
// rotations [first, first + count) of the batch on one kernel; active: rotations per workgroup of the batch kernel (8, or 4 = one per
// SIMD), 0 on the other two
struct BrSegment { BrKernel kernel; size_t first, count; int active; };
struct BrPlan {
    int n = 0;
    BrSegment seg[3];      // full rounds + a paired tail + its last started round: no rule issues more
    void add(BrKernel k, size_t first, size_t count, int active = 0) { seg[n++] = BrSegment{k, first, count, active}; }
};

// One round of the batch kernel's grid is a workgroup of 8 rotations per CU and takes ~19 ms however few of its
// wave slots are used, so a launch of a few rotations past a whole round used to cost two rounds.  Launches are cut into
// whole rounds plus a tail, and the tail takes the cheapest of: the low-latency kernel (a CU per
// rotation, 3.3 ms per started round of one rotation per CU), its paired form (two per CU, 5.3 - 5.8 ms), the batch
// kernel with one rotation per SIMD (~12 ms per round of four per CU), a full round.  All variants compute identical words.
//
// forced_shape ("br_shape", per thread): 0 = by these rules; 1 / 2 / 3 = the whole launch on the batch kernel (8 rotations per
// workgroup) / the paired low-latency kernel / the single one -- a caller that places launches itself (the two-lane scheduler,
// tools/two_lane_probe.py).
inline BrPlan plan_blind_rotate(size_t count, int cus, const Tuning& t, long forced_shape)
{
    BrPlan p;
    if (count == 0) return p;
    if (forced_shape > 0) {
        if (forced_shape == 1) p.add(BrKernel::Batch, 0, count, kBatchWaves);
        else p.add(forced_shape == 2 ? BrKernel::Ll2 : BrKernel::Ll, 0, count);
        return p;
    }
    const size_t cu = (size_t)std::max(1, cus);
    const size_t round = cu * kBatchWaves;
    // Measured on MI355X, 256 CUs (tools/latency_sweep.py, tools/ll_times.py; profiles/r02_latency_sweep.txt, r05_ll_ab.txt), ms per
    // launch of n rotations, key switch included:
    //   low-latency kernel  2.9 (n <= 64), 3.3 / 6.7 / 10.0 / 13.3 / 16.6 per started round of one rotation per CU
    //   its paired form     5.0 - 5.3 per started round of two per CU (10.4 for four, 17.1 for six, 22.9 for eight)
    //   one rotation per SIMD 12.7 (n <= 4 per CU)          two per SIMD 20.7 (n <= 8 per CU)
    // so: low-latency up to one rotation per CU, rounds of two per CU on the paired kernel (+ a last round of up to one per CU on
    // the single one) up to six per CU, a full round of the batch kernel above.  ("ll2_threshold" 0 gives the rules without the
    // paired kernel: low-latency up to three per CU, one-per-SIMD up to four, both up to five.)
    const bool auto_ll = t.ll_threshold < 0, auto_half = t.half_threshold < 0;
    auto small = [&](size_t first, size_t n) {
        if (t.ll2_threshold > 0 && (long)n <= t.ll2_threshold) {
            p.add(BrKernel::Ll2, first, n);
        } else if (t.ll2_threshold < 0 && auto_ll && auto_half && n > cu && n <= 6 * cu) {
            // rounds of two rotations per CU on the paired kernel and a last started round of up to one per CU on the single one
            const size_t rem = n % (2 * cu), paired = (rem == 0 || rem > cu) ? n : n - rem;
            p.add(BrKernel::Ll2, first, paired);
            if (paired < n) p.add(BrKernel::Ll, first + paired, n - paired);
        } else if (auto_ll && auto_half && n > 4 * cu && n <= 5 * cu) {
            // (without the paired kernel) four per CU at one rotation per SIMD (12.0 ms) and the rest on the low-latency kernel (3.2):
            // 15.5 ms against 16.6 for five rounds of the low-latency kernel and 20 for a full round
            p.add(BrKernel::Batch, first, 4 * cu, kBatchWaves / 2);
            p.add(BrKernel::Ll, first + 4 * cu, n - 4 * cu);
        } else if (auto_ll ? n <= 3 * cu : (long)n <= t.ll_threshold) {
            p.add(BrKernel::Ll, first, n);
        } else {
            const bool half = auto_half ? n <= 4 * cu : (long)n <= t.half_threshold;
            p.add(BrKernel::Batch, first, n, half ? kBatchWaves / 2 : kBatchWaves);
        }
    };
    const size_t tail = count % round;
    const long tail_max = std::max(auto_half ? (long)(4 * cu) : t.half_threshold, auto_ll ? (long)((t.ll2_threshold < 0 ? 6 : 5) * cu) : t.ll_threshold);
    if (t.tail_split && count > round && tail != 0 && (long)tail <= tail_max) {
        p.add(BrKernel::Batch, 0, count - tail, kBatchWaves);
        small(count - tail, tail);
    } else {
        small(0, count);
    }
    return p;
}

// The scheduler's price of one dependence level of `count` rotations, key switch and launch gaps included (MI355X, ms;
// tools/tail_times.py): the segments of its plan under the DEFAULT Tuning -- option overrides move the launches, not this estimate.
// Under the default rules a batch segment runs 8 rotations per workgroup and a single-kernel segment is one started round.
inline double blind_rotate_ms(size_t count, int cus)
{
    const size_t c = device_cus(cus), round = kBatchWaves * c;
    const BrPlan p = plan_blind_rotate(count, (int)c, Tuning{}, 0);
    double ms = 0.0;
    for (int i = 0; i < p.n; i++) {
        const BrSegment& s = p.seg[i];
        switch (s.kernel) {
            case BrKernel::Batch: ms += (double)(s.count / round) * 18.25 + (s.count % round ? 18.2 : 0.0); break;
            case BrKernel::Ll2: ms += (double)((s.count + 2 * c - 1) / (2 * c)) * 5.0; break;
            case BrKernel::Ll: ms += i > 0 && p.seg[i - 1].kernel == BrKernel::Ll2 ? 2.9 : 3.1; break;
        }
    }
    return ms;
}

// Two lanes: measured on MI355X with both lanes running (tools/two_lane_probe.py, profiles/r06_two_lane_probe.txt) -- a step of the
// paired low-latency kernel on half of the CUs, key switch included, 4.80 ms beside the bulk lane (4.59 alone); a chunk of the batch
// kernel on the other half 18.6 ms (17.9 alone).  Half of the CUs each: an in-order stream then never has more workgroups in flight
// than the other lane leaves free, so neither lane ever queues behind the other (full-width chunks beside the chain: 132 ms
// against 79).  Fewer than 16 CUs: no lanes.
// M: sched::Backend::LaneModel (sched_core.h)
template <class M>
bool lane_model(int cus, M* m)
{
    const size_t c = device_cus(cus);
    if (c < 16) return false;
    m->chain_gates = 2 * (c / 2);
    m->bulk_gates = (size_t)kBatchWaves * (c / 2);
    m->chain_ms = 4.80;
    m->bulk_ms = 18.6;
    return true;
}
// the forced shape of a lane's launch of n rotations -- chain lane (0): the paired low-latency kernel (the single one for at most a
// rotation per CU of its half); bulk lane (1): the batch kernel
inline long lane_shape(int lane, size_t n, int cus) { return lane == 1 ? 1 : n <= device_cus(cus) / 2 ? 3 : 2; }

// ---- key switch ----

enum class KsKernel { Split8, WorkgroupPer, Shared };     // keyswitch_direct_kernel over 8 workgroups / one per ciphertext, keyswitch_kernel
struct KsPlan { KsKernel kernel; int per_wg, slices; };   // per_wg, slices: the shape of a shared-table launch
// what a path's key switch has to choose from
struct KsRule {
    bool split8;      // the 8-way split exists and the count thresholds apply by the measured rule (the default path)
    bool padded;      // a padded table for the shared-table kernel exists
};
constexpr KsRule kKsDefaultPath{true, true}, kKsFixedShapePath{false, true};

// The shape of a shared-table launch (keyswitch_kernel: per_wg ciphertexts per workgroup, the kn steps of j cut into `slices` runs):
// the cheapest by a model of the measured times -- a workgroup of 16 live waves takes 1.03 us per step (0.68 and 0.022 per live wave),
// 12 us around its steps; the workgroups run in rounds of one per CU; a launch with runs zeroes the outputs first.  kn = 1024 -- 4096
// ciphertexts: 256 workgroups x 1024 steps; 3072: 768 x 256 (three rounds); 2048: 256 x 512; 256: 256 x 64.  min_slices: a
// workgroup keeps the digit words of at most 1024 steps.
inline void ks_shared_shape(size_t count, int cus, int kn, int min_slices, const Tuning& t, int* per_wg, int* slices)
{
    const size_t c = device_cus(cus);
    if (t.ks_slices > 0 || t.ks_per_wg > 0) {            // forced (tests, sweeps): the other one by the round-5 rule
        const size_t p = (count + c - 1) / c;
        *per_wg = t.ks_per_wg > 0 ? (int)t.ks_per_wg : (int)(p < 1 ? 1 : p > 16 ? 16 : p);
        *slices = std::max(min_slices, t.ks_slices > 0 ? (int)t.ks_slices : 1);
        return;
    }
    auto cost = [&](int p, int sl) {                      // us
        const size_t wgs = (count + p - 1) / p * sl, rounds = (wgs + c - 1) / c;
        return rounds * (kn / sl * (0.68 + 0.022 * p) + 12.0) + (sl > 1 ? 20.0 : 15.0);
    };
    const size_t fit = (count * min_slices + c - 1) / c;  // fewest ciphertexts per workgroup that still fit one round
    int best_p = (int)(fit < 1 ? 1 : fit > 16 ? 16 : fit), best_sl = min_slices;
    double best = cost(best_p, best_sl);
    for (int sl = min_slices; sl <= 64; sl *= 2) {
        const double ms = cost(kKsMaxPerWg, sl);
        if (ms < best) { best = ms; best_p = kKsMaxPerWg; best_sl = sl; }
    }
    *per_wg = best_p;
    *slices = best_sl;
}

// Key switch launch shape, -1 = the measured rule (tools/ks_slices.py, MI355X, ms per launch of n key switches):
//   8 workgroups per ciphertext   0.046 (n = 1)  0.049 (16)  0.051 (32)  0.078 (64)  0.13 (128)  0.24 (256)  0.45 (512)  0.85 (1024)
//   a workgroup per ciphertext    0.22 (n <= 256)  0.42 (512)  0.80 (1024)  1.19 (1536)  1.63 (2048)  3.3 (4096)
//   table through LDS (keyswitch_kernel), 16 ciphertexts per workgroup and the steps of j cut into runs that fill the CUs:
//                                 0.040 (1)  0.052 (16)  0.059 (32)  0.070 (64)  0.084 (128)  0.12 (256)  0.19 (512)  0.32 (1024)
//                                 0.56 (1536)  0.58 (2048)  0.86 (3072)  1.04 - 1.09 (4096)
// so: split up to 32, the shared-table kernel above -- on 256 CUs; in units of the device's CU count: 1/8 ciphertext per CU.
// The workgroup-per-ciphertext kernel is no longer chosen by the rule ("ks_wg_threshold" still forces it: 2.1 us per ciphertext on
// the N = 2048 shape).  The parameter-set and N = 2048 paths run the shared-table kernel over their shape at any count, and the
// workgroup-per-ciphertext kernel only by "ks_wg_threshold" -- or when the padded table could not be built.
inline KsPlan plan_keyswitch(size_t count, int cus, int kn, int min_slices, KsRule rule, const Tuning& t)
{
    KsPlan p{KsKernel::Shared, 0, 0};
    if (rule.split8) {
        const long split_max = t.ks_split_threshold < 0 ? std::max(1, cus) / 8 : t.ks_split_threshold;
        const long wg_max = t.ks_wg_threshold < 0 ? 0 : t.ks_wg_threshold;
        if ((long)count <= split_max) p.kernel = KsKernel::Split8;
        else if ((long)count <= wg_max) p.kernel = KsKernel::WorkgroupPer;
    } else if (!rule.padded || (t.ks_wg_threshold > 0 && (long)count <= t.ks_wg_threshold)) {
        p.kernel = KsKernel::WorkgroupPer;
    }
    if (p.kernel == KsKernel::Shared) ks_shared_shape(count, cus, kn, min_slices, t, &p.per_wg, &p.slices);
    return p;
}

// The lvl10 key switch as an int8 matrix product (keyswitch_mm_kernel, kernels_ks2.hip.h) instead of the plan above?  Only when none
// of the four options that force a shape of the other kernels is set, so that every test and tool that asks for one of them gets it.
// plan_keyswitch and the cost models above do not know this kernel: the two-lane scheduler prices large key switches as before.
// The measured rule, in ciphertexts per CU (MI355X, ms per launch, tools/ks_mm_times.py, profiles/r19_keyswitch_matrix.md):
//   the plan above   0.104 (256)  0.173 (512)  0.305 (1024)  0.455 (1536)  0.549 (2048)  0.824 (3072)  1.048 (4096)
//   matrix product   0.139 (256)  0.141 (512)  0.143 (1024)  0.143 (1536)  0.145 (2048)  0.160 (3072)  0.216 (4096)
// so: from two ciphertexts per CU on.
constexpr long kKsMmFromPerCu = 2;
inline bool use_matrix_keyswitch(size_t count, int cus, const Tuning& t)
{
    if (t.ks_split_threshold != -1 || t.ks_wg_threshold != -1 || t.ks_per_wg != -1 || t.ks_slices != -1) return false;
    const long from = t.ks_mm_threshold < 0 ? kKsMmFromPerCu * (long)device_cus(cus) : t.ks_mm_threshold;
    return from > 0 && (long)count >= from;
}

// ---- the smaller rules ----

// Parameter sets, rotations per launch from which the wave-per-rotation kernel runs.  By cost (tools/ps_latency.py, tools/ps_times.py;
// blind rotation + key switch, MI355X): the workgroup-per-rotation kernel takes 4.3 / 3.4 / 3.7 ms per started round of one rotation
// per CU (default / k2n512 / cggi16; 4.2 / 3.0 / 3.5 for a few rotations), a round of the wave-per-rotation kernel (up to eight per
// CU) 21 / 18.5 / 26 ms: the second wins from the fifth / sixth / seventh started round on (the seventh of cggi16: a tie).
inline long ps_batch_from(int limbs, int nbit, int cus) { return (limbs > 1 ? 6L : nbit == 9 ? 5L : 4L) * std::max(1, cus) + 1; }
inline bool ps_use_batch(size_t count, int limbs, int nbit, int cus, const Tuning& t)
{
    return (long)count >= (t.ps_batch_threshold < 0 ? ps_batch_from(limbs, nbit, cus) : t.ps_batch_threshold);
}

// N = 2048 blind rotation: the four-quarter-wave kernel? (Tuning::lvl2_kernel)
inline bool lvl2_quarters(size_t count, int cus, const Tuning& t)
{
    return t.lvl2_kernel < 0 ? count > device_cus(cus) : t.lvl2_kernel == 1;
}

// Launch shape of the tile table-sum kernels (private_keyswitch_kernel, kernels_pks.hip.h, with two key functions; pack_keyswitch_kernel
// and pack_keyswitch_desc_kernel, kernels_pack.hip.h, with one): tiles of `tile` inputs share every key slice, `chunks` workgroups per tile and key function (one
// per 256 of the 2N row words); tiles that give fewer than four workgroups per CU cut the i range (`in_words`, staged `i_block` at a
// time) into slices, whose partial sums meet by vector atomics in a zeroed output, so the words do not depend on the shape.
// forced_slices > 0 ("pack_slices") sets the slices instead, clamped to 1 .. max.
// grid_x = key_functions * chunks * tiles (tile = blockIdx.x % tiles), grid_y = slices.
struct TableSumGeometry { int tile, chunks, in_words, i_block; };
struct TableSumPlan { int tiles, slices; unsigned grid_x, grid_y; };
constexpr int pack_max_slices(TableSumGeometry g) { return (g.in_words + g.i_block - 1) / g.i_block; }
// inputs [first, first + n) of tile `tile`; words [begin, end) of slice `slice` (empty for the last slices when `slices` does not
// divide the range evenly): the pack kernels and tests/host/plan_pack_harness.cpp both read the plan through these
constexpr long pack_tile_first(int tile, int tile_size) { return (long)tile * tile_size; }
constexpr int pack_tile_inputs(int tile, int tile_size, long count) { return (int)(count - pack_tile_first(tile, tile_size) < tile_size ? count - pack_tile_first(tile, tile_size) : tile_size); }
constexpr int pack_slice_begin(int slice, int slices, int in_words)
{
    return (in_words + slices - 1) / slices * slice < in_words ? (in_words + slices - 1) / slices * slice : in_words;
}
// pack_slice_begin against the cut without the clamp -- per = ceil(in_words / slices), [slice per, min(in_words, slice per + per)) -- for
// every slice of every slice count up to max_slices: the same words, or both empty
constexpr bool slices_match_unclamped_cut(int in_words, int max_slices)
{
    for (int slices = 1; slices <= max_slices; slices++) {
        const int per = (in_words + slices - 1) / slices;
        for (int slice = 0; slice < slices; slice++) {
            const int b0 = slice * per, e0 = b0 + per < in_words ? b0 + per : in_words;
            const int b1 = pack_slice_begin(slice, slices, in_words), e1 = pack_slice_begin(slice + 1, slices, in_words);
            if (b0 < e0 ? b0 != b1 || e0 != e1 : b1 < e1) return false;
        }
    }
    return true;
}
inline TableSumPlan plan_table_sum(size_t count, int cus, TableSumGeometry g, int key_functions, long forced_slices = -1)
{
    const int tiles = (int)((count + g.tile - 1) / g.tile), max_slices = pack_max_slices(g);
    const long wgs = (long)tiles * key_functions * g.chunks;
    const long want = 4L * (long)device_cus(cus);
    long slices = 1;
    if (forced_slices > 0) slices = forced_slices;
    else if (wgs > 0 && wgs < want) slices = (want + wgs - 1) / wgs;
    slices = std::max(1L, std::min<long>(slices, max_slices));
    return {tiles, (int)slices, (unsigned)wgs, (unsigned)slices};
}
// the rule under its two users' names: the private key switch (two key functions, no option) and TLWE packing (one, "pack_slices")
using PksGeometry = TableSumGeometry;
using PksPlan = TableSumPlan;
using PackGeometry = TableSumGeometry;
using PackPlan = TableSumPlan;
inline PksPlan plan_private_keyswitch(size_t count, int cus, PksGeometry g) { return plan_table_sum(count, cus, g, 2); }
inline PackPlan plan_pack(size_t count, int cus, PackGeometry g, const Tuning& t) { return plan_table_sum(count, cus, g, 1, t.pack_slices); }

// ---- linear layers ----

// Launch shape of linear_kernel (kernels_linear.hip.h): y[set][row] = sum_k W[row][k] x[set][k] (+ bias) on ciphertexts of `words` words.
// A lane owns one word index, a wave 64 consecutive ones (a chunk; the last chunk of a ciphertext is partial: 631 and 1025 are no
// multiples of 64) of one set and a tile of kLinearRowTile rows held in registers; it walks k in steps of kLinearUnroll.  Waves are
// numbered row tile first, then chunk, then set, so the waves of a workgroup read the same input words (one trip to L2 per workgroup,
// the others hit the CU's vector cache) and the workgroups in flight share few chunks.  Four waves per workgroup; a launch with fewer
// such workgroups than CUs runs one wave per workgroup instead, so that a small layer still spreads over the device.
constexpr int kLinearRowTile = 16;       // TJ: rows per wave, one accumulator register each
constexpr int kLinearUnroll = 4;         // U: inputs loaded before their products are formed
constexpr int kLinearWaveWords = 64;
constexpr int kLinearMaxWaves = 4;
struct LinearPlan {
    int row_tile, unroll;          // kLinearRowTile, kLinearUnroll: what the tests take their boundaries from
    int row_tiles, chunks;         // tiles of rows per set, chunks of 64 words per ciphertext
    long waves;                    // sets * chunks * row_tiles
    int waves_per_block;           // 4 or 1
    unsigned grid_x, block_x;      // ceil(waves / waves_per_block) workgroups of 64 * waves_per_block threads
};
// the wave's place in the plan, and register j / lane l of it: the kernel and tests/host/plan_linear_harness.cpp both read the plan
// through these
constexpr long linear_wave_of(long block, int wave_in_block, int waves_per_block) { return block * waves_per_block + wave_in_block; }
constexpr int linear_wave_tile(long wave, int row_tiles) { return (int)(wave % row_tiles); }
constexpr int linear_wave_chunk(long wave, int row_tiles, int chunks) { return (int)(wave / row_tiles % chunks); }
constexpr long linear_wave_set(long wave, int row_tiles, int chunks) { return wave / row_tiles / chunks; }
constexpr int linear_row(int tile, int j) { return tile * kLinearRowTile + j; }                 // live when < rows
constexpr int linear_word(int chunk, int lane) { return chunk * kLinearWaveWords + lane; }      // live when < words
inline LinearPlan plan_linear(size_t rows, size_t cols, size_t sets, int words, int cus)
{
    (void)cols;      // the walk over k is inside a wave: it changes no shape
    LinearPlan p{kLinearRowTile, kLinearUnroll, 0, 0, 0, kLinearMaxWaves, 0, 0};
    p.row_tiles = (int)((rows + kLinearRowTile - 1) / kLinearRowTile);
    p.chunks = (words + kLinearWaveWords - 1) / kLinearWaveWords;
    p.waves = (long)sets * p.chunks * p.row_tiles;
    if ((p.waves + kLinearMaxWaves - 1) / kLinearMaxWaves < (long)device_cus(cus)) p.waves_per_block = 1;
    p.grid_x = (unsigned)((p.waves + p.waves_per_block - 1) / p.waves_per_block);
    p.block_x = (unsigned)(kLinearWaveWords * p.waves_per_block);
    return p;
}

}  // namespace plan
