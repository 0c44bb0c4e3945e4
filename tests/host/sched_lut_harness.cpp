// sched_lut_harness.cpp -- the stream scheduler (cufhe_amd/csrc/sched_core.h) with recorded lookups, Spreads and table rotations,
// against a stub device.
//
// Random netlists mix level-0 gates, LOOKUP GROUPS (the nout outputs of one evaluation, recorded by DeviceSched::record_gate_group as
// cufhe_amd_enqueue_lookup does: two level-0 address operands and a level-2 table as the third operand, node kind 0) and kind-2
// WRITERS of those level-2 buffers (Spread: TRLWE -> TRLWE; the table rotation: TRLWE, lvl0 -> TRLWE), recorded by record_gate with
// kind 2 as cufhe_amd_enqueue_spread / _enqueue_lut_rotate do.  Single-output lookups may run in place (out == in0).  The stub executes
// every launch at once, in submission order, every operand read before any output is written, and counts rotations as the HIP lowering
// does: one per distinct (definition, in0, in1, in2) of a launch for lookup outputs, one per gate and per table rotation, none for a
// Spread.  Checked for every configuration (renaming on and off, "sched_two_lane" 0 and 2):
//   - every ciphertext holds the words of an in-order interpreter,
//   - rotations == evaluations,
//   - a writer of a table sits in a strictly later dependence level than every recorded reader of the value it overwrites.
//
// Usage: sched_lut_harness <seeds>      prints one line per configuration, "ALL PASS" at the end.  Plain g++; also built with
// -fsanitize=address,undefined and run as it is (tests/test_sched_lut.py).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <tuple>

#include "../../cufhe_amd/csrc/sched_core.h"

using namespace cufhe_amd::sched;

static const int kWords0 = 37, kWords2 = 53;
static const int kBase = 16384, kDefs = 64;      // output j of definition k: kBase + k + j kDefs (CUFHE_AMD_LOOKUP_OP_OUTPUT)
static const int kSpread = 6400, kLutRotate = 6656, kCopy = 99;
static int def_nout(int k) { return 1 << (k % 4); }
static bool def_two_operands(int k) { return (k / 4) % 2 == 1; }
static bool is_lookup(int op) { return op >= kBase; }

static uint32_t mix(int op, uint32_t a, uint32_t b, uint32_t c, uint32_t w)
{
    uint32_t v = a * 0x9E3779B1u + ((b << 5) | (b >> 27)) * 0x85EBCA77u + ((c << 11) | (c >> 21)) * 0xC2B2AE3Du + (uint32_t)op * 0x27D4EB2Fu + w;
    return v ^ (a >> 15) ^ (v << 7);
}
// every op as a function of ALL words of its operands; `out` may be an operand (the result is formed first)
static void toy_op(int op, uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* c)
{
    uint32_t r[kWords2];
    if (is_lookup(op)) {            // (in0, in1 or null: lvl0; table: level 2) -> lvl0
        for (int w = 0; w < kWords0; w++) r[w] = mix(op, a[w], b ? b[w] : 0u, c[w] ^ c[kWords2 - 1 - w], (uint32_t)w);
        memcpy(out, r, kWords0 * 4);
    } else if (op == kSpread) {     // TRLWE -> TRLWE
        for (int w = 0; w < kWords2; w++) r[w] = mix(op, a[w], a[(w + 7) % kWords2], 0u, (uint32_t)w);
        memcpy(out, r, kWords2 * 4);
    } else if (op == kLutRotate) {  // (table, addr) -> TRLWE
        for (int w = 0; w < kWords2; w++) r[w] = mix(op, a[w], b[w % kWords0], 0u, (uint32_t)w);
        memcpy(out, r, kWords2 * 4);
    } else {                        // a level-0 gate
        for (int w = 0; w < kWords0; w++) r[w] = mix(op, a[w], b ? b[w] : 0u, c ? c[w] : 0u, (uint32_t)w);
        memcpy(out, r, kWords0 * 4);
    }
}
static int out_words(int op) { return op == kSpread || op == kLutRotate ? kWords2 : kWords0; }

struct Ev { bool done = true; };

class SyncBackend : public Backend {
   public:
    explicit SyncBackend(bool two_lane) : two_lane_(two_lane) {}
    void bind_thread() override {}
    int num_streams() override { return 4; }
    int words(int level) override { return level == 2 ? kWords2 : kWords0; }
    int alloc_device(size_t bytes, void** p) override { *p = calloc(1, bytes); return 0; }
    int free_device(void* p) override { free(p); return 0; }
    int alloc_pinned(size_t bytes, void** p) override { *p = calloc(1, bytes); return 0; }
    int free_pinned(void* p) override { free(p); return 0; }
    int h2d(int, void* dst, const void* src, size_t bytes) override { memcpy(dst, src, bytes); return 0; }
    int d2h(int, void* dst, const void* src, size_t bytes) override { memcpy(dst, src, bytes); return 0; }
    int copy_ctxts(int, const CopyRec* recs, size_t n, uint32_t* staging, bool to_ctxt) override
    {
        for (size_t i = 0; i < n; i++) {
            const size_t bytes = (size_t)words(recs[i].level) * 4;
            if (to_ctxt) memcpy(recs[i].dev, staging + recs[i].slot, bytes);
            else memcpy(staging + recs[i].slot, recs[i].dev, bytes);
        }
        return 0;
    }
    int run_gates(int, int level, const GateRef* g, size_t n) override
    {
        // rotations of the launch, as lower_lut_ops fuses them; then the ops, every operand read before any output is written
        std::set<std::tuple<int, const uint32_t*, const uint32_t*, const uint32_t*>> evals;
        std::vector<std::vector<uint32_t>> res(n, std::vector<uint32_t>(kWords2));
        for (size_t i = 0; i < n; i++) {
            if ((out_words(g[i].op) == kWords2) != (level == 2)) { fprintf(stderr, "op %d in a launch of kind %d\n", g[i].op, level); abort(); }
            if (is_lookup(g[i].op)) evals.insert(std::make_tuple((g[i].op - kBase) % kDefs, g[i].in0, g[i].in1, g[i].in2));
            else if (g[i].op != kCopy && g[i].op != kSpread) rotations++;
            if (g[i].op != kCopy) toy_op(g[i].op, res[i].data(), g[i].in0, g[i].in1, g[i].in2);
        }
        rotations += evals.size();
        for (size_t i = 0; i < n; i++)
            if (g[i].op == kCopy) memmove(g[i].out, g[i].in0, (size_t)words(level) * 4);
            else memcpy(g[i].out, res[i].data(), (size_t)out_words(g[i].op) * 4);
        return 0;
    }
    int event_create(void** ev) override { *ev = new Ev(); return 0; }
    int event_destroy(void* ev) override { delete (Ev*)ev; return 0; }
    int event_record(int, void*) override { return 0; }
    int event_query(void*) override { return 1; }
    int event_sync(void*) override { return 0; }
    int stream_wait(int, void*) override { return 0; }
    std::string error_text() override { return "stub"; }
    bool lane_model(LaneModel* m) override
    {
        if (!two_lane_) return false;
        m->chain_gates = 3; m->bulk_gates = 8; m->chain_ms = 1.0; m->bulk_ms = 3.0;
        return true;
    }
    double launch_ms(size_t n) override { return n ? 1000.0 : 0.0; }
    int gate_weight(int op) override { return op == kCopy || op == kSpread ? 0 : 1; }
    bool shares_rotation(int op) override { return is_lookup(op) && def_nout((op - kBase) % kDefs) > 1; }
    int lowering(int op) override { return is_lookup(op) || op == kSpread || op == kLutRotate ? 1 : 0; }
    int run_gates_lane(int s, int level, const GateRef* g, size_t n, int) override { return run_gates(s, level, g, n); }
    uint64_t rotations = 0;

   private:
    bool two_lane_;
};

static int g_failures = 0;

struct Totals { uint64_t rot = 0, want = 0, tl = 0, lookups = 0, writers = 0, in_place = 0, hazards = 0; };

static void run_program(uint64_t seed, bool luts, int two_lane, bool rename, Totals* t)
{
    std::mt19937_64 rng(seed);
    SyncBackend* be = nullptr;
    Scheduler S(1, false, [&](int) { be = new SyncBackend(two_lane != 0); return be; });
    S.dev(0).two_lane = two_lane;
    S.dev(0).rename_outputs = rename;
    S.dev(0).copy_op = kCopy;
    S.dev(0).set_level_flush_gates(8 + rng() % 40);
    const int C = 24, T = 5;
    std::vector<std::vector<uint32_t>> host(C + T), model(C + T);
    std::vector<cufhe_amd_ctxt*> h(C + T);
    std::string err;
    for (int i = 0; i < C + T; i++) {
        const int words = i < C ? kWords0 : kWords2;
        host[i].resize(words);
        for (int w = 0; w < words; w++) host[i][w] = (uint32_t)rng();
        model[i] = host[i];
        if (S.ctxt_create(i < C ? 0 : 2, host[i].data(), &h[i], &err)) { fprintf(stderr, "ctxt_create: %s\n", err.c_str()); abort(); }
    }
    // the dependence levels of the recorded lookups that read table t's current value
    std::vector<std::vector<uint32_t>> reader_levels(T);
    std::set<std::tuple<int, int, int, int>> used;
    void* streams[3] = {(void*)0x1001, (void*)0x1002, (void*)0x1003};
    const int G = 60 + (int)(rng() % 60);
    for (int gi = 0; gi < G; gi++) {
        void* st = streams[rng() % 3];
        const unsigned pick = luts ? (unsigned)(rng() % 10) : 9u;
        if (pick < 4) {                 // a lookup group
            // (no (definition, in0, in1, table) twice in a program: two such groups in one level are ONE evaluation to the lowering, and
            // rightly so -- same operands, same words -- but the count below takes one rotation per recorded group)
            int k, table, in0, in1;
            do {
                k = (int)(rng() % kDefs); table = (int)(rng() % T);
                in0 = (int)(rng() % C); in1 = def_two_operands(k) ? (int)(rng() % C) : -1;
            } while (!used.insert(std::make_tuple(k, in0, in1, table)).second);
            const int nout = def_nout(k);
            std::vector<int> outs;
            if (nout == 1) outs.push_back(rng() % 4 == 0 ? in0 : (int)(rng() % C));       // in place, one time in four
            while ((int)outs.size() < nout) {
                const int o = (int)(rng() % C);
                if (std::find(outs.begin(), outs.end(), o) == outs.end() && o != in0 && o != in1) outs.push_back(o);
            }
            cufhe_amd_ctxt* ins[3] = {h[in0], in1 >= 0 ? h[in1] : nullptr, h[C + table]};
            int ops[8];
            cufhe_amd_ctxt* oh[8];
            std::vector<std::vector<uint32_t>> r(nout, std::vector<uint32_t>(kWords0));
            for (int j = 0; j < nout; j++) {
                ops[j] = kBase + k + j * kDefs;
                oh[j] = h[outs[j]];
                toy_op(ops[j], r[j].data(), model[in0].data(), in1 >= 0 ? model[in1].data() : nullptr, model[C + table].data());
            }
            for (int j = 0; j < nout; j++) model[outs[j]] = r[j];
            if (int rc = S.dev(0).record_gate_group(st, ops, true, oh, (size_t)nout, ins)) { fprintf(stderr, "record_gate_group rc %d\n", rc); abort(); }
            const uint32_t level = oh[0]->d[0].wdepth;
            for (int j = 1; j < nout; j++)
                if (oh[j]->d[0].wdepth != level) { fprintf(stderr, "seed %llu: siblings in different levels\n", (unsigned long long)seed); g_failures++; }
            reader_levels[table].push_back(level);
            t->want++; t->lookups++;
            t->in_place += nout == 1 && outs[0] == in0;
        } else if (pick < 6) {          // a kind-2 writer of a table: Spread or the table rotation
            const bool rotate = rng() % 2 == 0;
            const int src = (int)(rng() % T), addr = (int)(rng() % C);
            int dst = (int)(rng() % T);
            if (dst == src) dst = (dst + 1) % T;
            std::vector<uint32_t> r(kWords2);
            toy_op(rotate ? kLutRotate : kSpread, r.data(), model[C + src].data(), rotate ? model[addr].data() : nullptr, nullptr);
            model[C + dst] = r;
            cufhe_amd_ctxt* ins[3] = {h[C + src], rotate ? h[addr] : nullptr, nullptr};
            if (int rc = S.dev(0).record_gate(st, rotate ? kLutRotate : kSpread, true, h[C + dst], ins, 2)) { fprintf(stderr, "record_gate rc %d\n", rc); abort(); }
            const uint32_t level = h[C + dst]->d[0].wdepth;
            for (uint32_t r_level : reader_levels[dst]) {
                t->hazards++;
                if (level <= r_level) {
                    fprintf(stderr, "seed %llu two_lane %d rename %d: a writer of table %d at level %u shares it with a reader at level %u\n",
                            (unsigned long long)seed, two_lane, (int)rename, dst, level, r_level);
                    g_failures++;
                }
            }
            reader_levels[dst].clear();
            t->want += rotate ? 1 : 0;
            t->writers++;
        } else {                        // a level-0 gate
            int in[3];
            const int arity = 1 + (int)(rng() % 3);
            for (int i = 0; i < 3; i++) in[i] = (int)(rng() % C);
            cufhe_amd_ctxt* ins[3] = {h[in[0]], arity >= 2 ? h[in[1]] : nullptr, arity == 3 ? h[in[2]] : nullptr};
            const int op = 1 + (int)(rng() % 9), o = (int)(rng() % C);
            std::vector<uint32_t> r(kWords0);
            toy_op(op, r.data(), model[in[0]].data(), arity >= 2 ? model[in[1]].data() : nullptr, arity == 3 ? model[in[2]].data() : nullptr);
            model[o] = r;
            if (int rc = S.dev(0).record_gate(st, op, true, h[o], ins)) { fprintf(stderr, "record_gate rc %d\n", rc); abort(); }
            t->want++;
        }
    }
    if (int rc = S.synchronize_all()) { fprintf(stderr, "synchronize rc %d\n", rc); abort(); }
    for (int i = 0; i < C + T; i++)
        if (host[i] != model[i]) {
            fprintf(stderr, "seed %llu two_lane %d rename %d luts %d: ciphertext %d differs from the in-order result\n",
                    (unsigned long long)seed, two_lane, (int)rename, (int)luts, i);
            g_failures++;
            break;
        }
    t->rot += be->rotations;
    t->tl += S.dev(0).stats().two_lane_groups.load();
    for (auto* c : h) S.ctxt_destroy(c);
}

int main(int argc, char** argv)
{
    const int seeds = argc > 1 ? atoi(argv[1]) : 40;
    for (int two_lane : {2, 0})
        for (bool rename : {true, false})
            for (bool luts : {true, false}) {
                Totals t;
                const int fail0 = g_failures;
                for (int s = 0; s < seeds; s++) run_program(3000 + s, luts, two_lane, rename, &t);
                if (t.rot != t.want) g_failures++;
                const bool ok = g_failures == fail0;
                printf("two_lane %d rename %d luts %d: rotations %llu for %llu evaluations, %llu lookups (%llu in place), %llu table writers "
                       "behind %llu readers, two-lane flushes %llu  %s\n", two_lane, (int)rename, (int)luts, (unsigned long long)t.rot,
                       (unsigned long long)t.want, (unsigned long long)t.lookups, (unsigned long long)t.in_place, (unsigned long long)t.writers,
                       (unsigned long long)t.hazards, (unsigned long long)t.tl, ok ? "PASS" : "FAIL");
                printf("RESULT {\"two_lane\": %d, \"rename\": %d, \"luts\": %d, \"rotations\": %llu, \"evaluations\": %llu, \"lookups\": %llu, "
                       "\"in_place\": %llu, \"writers\": %llu, \"readers_behind\": %llu, \"two_lane_groups\": %llu}\n", two_lane, (int)rename, (int)luts,
                       (unsigned long long)t.rot, (unsigned long long)t.want, (unsigned long long)t.lookups, (unsigned long long)t.in_place,
                       (unsigned long long)t.writers, (unsigned long long)t.hazards, (unsigned long long)t.tl);
            }
    printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
