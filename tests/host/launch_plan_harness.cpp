// launch_plan_harness.cpp -- the launch-shape rules (cufhe_amd/csrc/launch_plan.h) printed as text, on the CPU.
// tests/test_launch_plan.py compares the text with what the code the header replaced printed (tests/golden/launch_plans_v1.json)
// and checks the plans' structure.
//
//   launch_plan_harness dump     every rule over the recorded grid, as blocks "# <rule> <inputs>" + lines.  A blind-rotate line is
//                                "count: K first count [active] | ..." (K = B batch, L low-latency, P its paired form); every other
//                                rule is constant over long runs of counts and prints "count value" where the value changes ("-" at
//                                count 0, where the launchers return before they ask)
//   launch_plan_harness query    one answer per request line on stdin (the forms are in query() below)
//
// g++ -O1 -std=c++17 -Wall -Wextra -Werror -o launch_plan_harness launch_plan_harness.cpp
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../cufhe_amd/csrc/launch_plan.h"

using plan::Tuning;

// the key-switch shapes (kn, min_slices) of KsShapeDefault and every KsShapePs / of KsShapeLvl2, the parameter sets' (limbs, Nbit)
// and private_keyswitch_kernel's geometry (kernels.hip.h, kernels_ks2.hip.h, kernels_ps.hip.h, kernels_pks.hip.h)
static const int kKsShapes[2][2] = {{1024, 1}, {2048, 2}};
static const int kPsSets[3][2] = {{1, 10}, {1, 9}, {2, 10}};
static const plan::PksGeometry kPks{64, 8, 2049, 16};
struct KsPath { const char* name; plan::KsRule rule; };
static const KsPath kKsPaths[4] = {{"default", plan::kKsDefaultPath}, {"ps", plan::kKsFixedShapePath}, {"ps_unpadded", {false, false}}, {"lvl2", plan::kKsFixedShapePath}};

// ---- the rules as text ----

static std::string br_text(size_t count, int cus, const Tuning& t, long shape)
{
    const plan::BrPlan p = plan::plan_blind_rotate(count, cus, t, shape);
    std::string out;
    for (int i = 0; i < p.n; i++) {
        const plan::BrSegment& s = p.seg[i];
        char buf[96];
        if (s.kernel == plan::BrKernel::Batch) snprintf(buf, sizeof buf, "B %zu %zu %d", s.first, s.count, s.active);
        else snprintf(buf, sizeof buf, "%c %zu %zu", s.kernel == plan::BrKernel::Ll ? 'L' : 'P', s.first, s.count);
        out += (i ? " | " : "") + std::string(buf);
    }
    return out;
}
static std::string ms_text(size_t count, int cus)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.16e", plan::blind_rotate_ms(count, cus));
    return buf;
}
static std::string lane_model_text(int cus)
{
    struct { size_t chain_gates, bulk_gates; double chain_ms, bulk_ms; } m{};
    if (!plan::lane_model(cus, &m)) return "none";
    char buf[128];
    snprintf(buf, sizeof buf, "%zu %zu %.16e %.16e", m.chain_gates, m.bulk_gates, m.chain_ms, m.bulk_ms);
    return buf;
}
static std::string lane_shape_text(size_t count, int cus)
{
    return std::to_string(plan::lane_shape(0, count, cus)) + " " + std::to_string(plan::lane_shape(1, count, cus));
}
static std::string ks_text(size_t count, int cus, int kn, int min_slices, const KsPath& path, const Tuning& t)
{
    const plan::KsPlan p = plan::plan_keyswitch(count, cus, kn, min_slices, path.rule, t);
    if (p.kernel == plan::KsKernel::Split8) return "S8";
    if (p.kernel == plan::KsKernel::WorkgroupPer) return "W";
    return "T " + std::to_string(p.per_wg) + " " + std::to_string(p.slices);
}
static std::string ps_text(size_t count, int limbs, int nbit, int cus, const Tuning& t)
{
    return std::to_string(plan::ps_batch_from(limbs, nbit, cus)) + (plan::ps_use_batch(count, limbs, nbit, cus, t) ? " batch" : " wg");
}
static std::string lvl2_text(size_t count, int cus, const Tuning& t) { return plan::lvl2_quarters(count, cus, t) ? "quarters" : "halves"; }
static std::string pks_text(size_t count, int cus)
{
    const plan::PksPlan p = plan::plan_private_keyswitch(count, cus, kPks);
    return std::to_string(p.tiles) + " " + std::to_string(p.slices);
}

// ---- dump ----

static std::vector<size_t> counts_of(int cus)
{
    std::vector<size_t> c;
    for (size_t n = 0; n <= (size_t)17 * cus + 9; n++) c.push_back(n);
    if (c.back() < 4600) c.push_back(4600);      // two rounds + a paired tail at 256 CUs
    c.push_back(32768);
    c.push_back(40960);
    return c;
}
template <class F>
static void runs(const std::vector<size_t>& counts, F text)
{
    std::string last;
    for (size_t n : counts) {
        const std::string s = text(n);
        if (n == counts[0] || s != last) printf("%zu %s\n", n, s.c_str());
        last = s;
    }
}

static void dump()
{
    const long big = 1L << 30;
    struct BrCase { long ll, ll2, half, tail, shape; };
    const BrCase br_cases[] = {{-1, -1, -1, 1, 0}, {0, 0, -1, 1, 0},   {-1, 0, -1, 1, 0}, {big, -1, -1, 1, 0}, {-1, 512, -1, 1, 0}, {-1, -1, 0, 1, 0},
                               {-1, -1, big, 1, 0}, {-1, -1, -1, 0, 0}, {-1, -1, -1, 1, 1}, {-1, -1, -1, 1, 2},  {-1, -1, -1, 1, 3}};
    struct KsCase { long split, wg, per_wg, slices; };
    const KsCase ks_cases[] = {{-1, -1, -1, -1}, {-1, -1, 4, -1}, {-1, -1, 16, -1}, {-1, -1, -1, 1},  {-1, -1, -1, 8}, {-1, -1, 16, 64},
                               {-1, 0, -1, -1},  {-1, 64, -1, -1}, {-1, big, -1, -1}, {0, -1, -1, -1}, {big, -1, -1, -1}, {0, 2048, -1, -1}};
    for (int cus : {1, 8, 15, 16, 40, 104, 256, 304}) {
        const std::vector<size_t> counts = counts_of(cus);
        for (const BrCase& c : br_cases) {
            Tuning t;
            t.ll_threshold = c.ll; t.ll2_threshold = c.ll2; t.half_threshold = c.half; t.tail_split = c.tail;
            printf("# br cus=%d ll=%ld ll2=%ld half=%ld tail=%ld shape=%ld\n", cus, c.ll, c.ll2, c.half, c.tail, c.shape);
            for (size_t n : counts) printf("%zu: %s\n", n, br_text(n, cus, t, c.shape).c_str());
        }
        printf("# ms cus=%d\n", cus);
        runs(counts, [&](size_t n) { return ms_text(n, cus); });
        printf("# lane cus=%d\nmodel %s\n", cus, lane_model_text(cus).c_str());
        runs(counts, [&](size_t n) { return lane_shape_text(n, cus); });
        for (const KsPath& path : kKsPaths)
            for (const auto& shape : kKsShapes)
                for (const KsCase& c : ks_cases) {
                    Tuning t;
                    t.ks_split_threshold = c.split; t.ks_wg_threshold = c.wg; t.ks_per_wg = c.per_wg; t.ks_slices = c.slices;
                    printf("# ks path=%s kn=%d min=%d cus=%d split=%ld wg=%ld per_wg=%ld slices=%ld\n", path.name, shape[0], shape[1], cus, c.split, c.wg,
                           c.per_wg, c.slices);
                    runs(counts, [&](size_t n) { return n ? ks_text(n, cus, shape[0], shape[1], path, t) : "-"; });
                }
        for (const auto& set : kPsSets)
            for (long thr : {-1L, 0L, 1000L}) {
                Tuning t;
                t.ps_batch_threshold = thr;
                printf("# ps limbs=%d nbit=%d cus=%d thr=%ld\n", set[0], set[1], cus, thr);
                runs(counts, [&](size_t n) { return n ? ps_text(n, set[0], set[1], cus, t) : "-"; });
            }
        for (long kernel : {-1L, 0L, 1L}) {
            Tuning t;
            t.lvl2_kernel = kernel;
            printf("# lvl2 cus=%d kernel=%ld\n", cus, kernel);
            runs(counts, [&](size_t n) { return n ? lvl2_text(n, cus, t) : "-"; });
        }
        printf("# pks cus=%d\n", cus);
        runs(counts, [&](size_t n) { return n ? pks_text(n, cus) : "-"; });
    }
}

// ---- query ----
//   br count cus ll ll2 half tail shape
//   ks count cus kn min_slices split8 padded split wg per_wg slices
//   ps count cus limbs nbit thr        lvl2 count cus kernel        pks count cus        ms count cus        lane count cus
static int query()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string rule;
        size_t count = 0;
        int cus = 0;
        in >> rule >> count >> cus;
        Tuning t;
        std::string out;
        if (rule == "br") {
            long shape = 0;
            in >> t.ll_threshold >> t.ll2_threshold >> t.half_threshold >> t.tail_split >> shape;
            out = br_text(count, cus, t, shape);
        } else if (rule == "ks") {
            int kn = 0, min_slices = 0, split8 = 0, padded = 0;
            in >> kn >> min_slices >> split8 >> padded >> t.ks_split_threshold >> t.ks_wg_threshold >> t.ks_per_wg >> t.ks_slices;
            out = ks_text(count, cus, kn, min_slices, KsPath{"query", plan::KsRule{split8 != 0, padded != 0}}, t);
        } else if (rule == "ps") {
            int limbs = 0, nbit = 0;
            in >> limbs >> nbit >> t.ps_batch_threshold;
            out = ps_text(count, limbs, nbit, cus, t);
        } else if (rule == "lvl2") {
            in >> t.lvl2_kernel;
            out = lvl2_text(count, cus, t);
        } else if (rule == "pks") {
            out = pks_text(count, cus);
        } else if (rule == "ms") {
            out = ms_text(count, cus);
        } else if (rule == "lane") {
            out = lane_model_text(cus) + " / " + lane_shape_text(count, cus);
        } else {
            in.setstate(std::ios::failbit);
        }
        if (in.fail()) {
            fprintf(stderr, "bad request: %s\n", line.c_str());
            return 2;
        }
        printf("%s\n", out.c_str());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "dump")) { dump(); return 0; }
    if (argc == 2 && !strcmp(argv[1], "query")) return query();
    fprintf(stderr, "usage: launch_plan_harness dump | query\n");
    return 2;
}
