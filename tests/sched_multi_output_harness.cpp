// sched_multi_output_harness.cpp -- the stream scheduler (cufhe_amd/csrc/sched_core.h) with multi-output gates, against a stub device.
//
// Random netlists of single-output gates and SIBLING GROUPS (the nout outputs of one evaluation, recorded together by
// DeviceSched::record_gate_group, as cufhe_amd_enqueue_gate_multi does) on copying ciphertexts, outputs overwriting earlier values
// (renaming and write-after-read hazards included).  The stub executes every launch at once, in submission order, and counts
// rotations as the HIP lowering does: one per distinct (definition, in0, in1, in2) of a launch for group outputs, one per other gate.
// Every run must give the words of an in-order interpreter and exactly one rotation per group, with "sched_two_lane" forced on
// (the planner then leaves flushes with groups to the level order) and off, with and without renaming.
//
// Usage: sched_multi_output_harness <seeds>      prints one line per configuration, "ALL PASS" at the end.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <tuple>

#include "../cufhe_amd/csrc/sched_core.h"

using namespace cufhe_amd::sched;

static const int kWords = 37;
static const int kBase = 1000, kDefs = 64;       // output j of definition k: kBase + k + j kDefs (CUFHE_AMD_USER_OP_OUTPUT)

static uint32_t mix(int op, uint32_t a, uint32_t b, uint32_t c, uint32_t w)
{
    uint32_t v = a * 0x9E3779B1u + ((b << 5) | (b >> 27)) * 0x85EBCA77u + ((c << 11) | (c >> 21)) * 0xC2B2AE3Du + (uint32_t)op * 0x27D4EB2Fu + w;
    return v ^ (a >> 15) ^ (v << 7);
}
static void toy_gate(int op, uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* c)
{
    uint32_t r[kWords];
    for (int w = 0; w < kWords; w++) r[w] = mix(op, a[w], b ? b[w] : 0u, c ? c[w] : 0u, (uint32_t)w);
    memcpy(out, r, sizeof r);
}
static bool is_group_op(int op) { return op >= kBase; }

struct Ev { bool done = true; };

class SyncBackend : public Backend {
   public:
    explicit SyncBackend(bool two_lane) : two_lane_(two_lane) {}
    void bind_thread() override {}
    int num_streams() override { return 4; }
    int words(int) override { return kWords; }
    int alloc_device(size_t bytes, void** p) override { *p = calloc(1, bytes); return 0; }
    int free_device(void* p) override { free(p); return 0; }
    int alloc_pinned(size_t bytes, void** p) override { *p = calloc(1, bytes); return 0; }
    int free_pinned(void* p) override { free(p); return 0; }
    int h2d(int, void* dst, const void* src, size_t bytes) override { memcpy(dst, src, bytes); return 0; }
    int d2h(int, void* dst, const void* src, size_t bytes) override { memcpy(dst, src, bytes); return 0; }
    int copy_ctxts(int, const CopyRec* recs, size_t n, uint32_t* staging, bool to_ctxt) override
    {
        for (size_t i = 0; i < n; i++) {
            if (to_ctxt) memcpy(recs[i].dev, staging + recs[i].slot, kWords * 4);
            else memcpy(staging + recs[i].slot, recs[i].dev, kWords * 4);
        }
        return 0;
    }
    int run_gates(int, int, const GateRef* g, size_t n) override
    {
        // rotations of the launch, as lower_gates fuses them; then the gates, every operand read before any output is written
        std::set<std::tuple<int, const uint32_t*, const uint32_t*, const uint32_t*>> evals;
        std::vector<std::vector<uint32_t>> res(n, std::vector<uint32_t>(kWords));
        for (size_t i = 0; i < n; i++) {
            if (is_group_op(g[i].op)) evals.insert(std::make_tuple((g[i].op - kBase) % kDefs, g[i].in0, g[i].in1, g[i].in2));
            else if (g[i].op != copy_op_) rotations++;
            toy_gate(g[i].op, res[i].data(), g[i].in0, g[i].in1, g[i].in2);
        }
        rotations += evals.size();
        for (size_t i = 0; i < n; i++)
            if (g[i].op == copy_op_) memmove(g[i].out, g[i].in0, kWords * 4);
            else memcpy(g[i].out, res[i].data(), kWords * 4);
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
    int gate_weight(int op) override { return op == copy_op_ ? 0 : 1; }
    bool shares_rotation(int op) override { return is_group_op(op); }
    int run_gates_lane(int s, int level, const GateRef* g, size_t n, int) override { return run_gates(s, level, g, n); }
    uint64_t rotations = 0;
    int copy_op_ = 99;

   private:
    bool two_lane_;
};

static int g_failures = 0;

// one random program; returns the number of group evaluations and single gates recorded
static void run_program(uint64_t seed, bool groups, int two_lane, bool rename, uint64_t* rot, uint64_t* want_rot, uint64_t* tl_groups)
{
    std::mt19937_64 rng(seed);
    SyncBackend* be = nullptr;
    Scheduler S(1, false, [&](int) { be = new SyncBackend(two_lane != 0); return be; });
    S.dev(0).two_lane = two_lane;
    S.dev(0).rename_outputs = rename;
    S.dev(0).copy_op = 99;
    S.dev(0).set_level_flush_gates(8 + rng() % 40);
    const int C = 24;
    std::vector<std::vector<uint32_t>> host(C, std::vector<uint32_t>(kWords)), model(C, std::vector<uint32_t>(kWords));
    std::vector<cufhe_amd_ctxt*> h(C);
    std::string err;
    for (int i = 0; i < C; i++) {
        for (int w = 0; w < kWords; w++) host[i][w] = model[i][w] = (uint32_t)rng();
        if (S.ctxt_create(0, host[i].data(), &h[i], &err)) { fprintf(stderr, "ctxt_create: %s\n", err.c_str()); abort(); }
    }
    void* streams[3] = {(void*)0x1001, (void*)0x1002, (void*)0x1003};
    const int G = 60 + (int)(rng() % 60);
    uint64_t expect = 0;
    for (int gi = 0; gi < G; gi++) {
        void* st = streams[rng() % 3];
        int in[3];
        const int arity = 1 + (int)(rng() % 3);
        for (int i = 0; i < 3; i++) in[i] = (int)(rng() % C);
        cufhe_amd_ctxt* ins[3] = {h[in[0]], arity >= 2 ? h[in[1]] : nullptr, arity == 3 ? h[in[2]] : nullptr};
        if (groups && rng() % 3 == 0) {
            const int nout = 2 << (rng() % 3), k = (int)(rng() % kDefs);
            std::vector<int> outs;
            while ((int)outs.size() < nout) {
                const int o = (int)(rng() % C);
                bool bad = std::find(outs.begin(), outs.end(), o) != outs.end();
                for (int i = 0; i < arity; i++) bad = bad || o == in[i];
                if (!bad) outs.push_back(o);
            }
            int ops[8];
            cufhe_amd_ctxt* oh[8];
            std::vector<std::vector<uint32_t>> r(nout, std::vector<uint32_t>(kWords));
            for (int j = 0; j < nout; j++) {
                ops[j] = kBase + k + j * kDefs;
                oh[j] = h[outs[j]];
                toy_gate(ops[j], r[j].data(), model[in[0]].data(), arity >= 2 ? model[in[1]].data() : nullptr,
                         arity == 3 ? model[in[2]].data() : nullptr);
            }
            for (int j = 0; j < nout; j++) model[outs[j]] = r[j];
            if (int rc = S.dev(0).record_gate_group(st, ops, true, oh, (size_t)nout, ins)) { fprintf(stderr, "record_gate_group rc %d\n", rc); abort(); }
            expect++;
        } else {
            const int op = 1 + (int)(rng() % 9), o = (int)(rng() % C);
            std::vector<uint32_t> r(kWords);
            toy_gate(op, r.data(), model[in[0]].data(), arity >= 2 ? model[in[1]].data() : nullptr, arity == 3 ? model[in[2]].data() : nullptr);
            model[o] = r;
            cufhe_amd_ctxt* o_h = h[o];
            if (int rc = S.dev(0).record_gate(st, op, true, o_h, ins)) { fprintf(stderr, "record_gate rc %d\n", rc); abort(); }
            expect++;
        }
    }
    if (int rc = S.synchronize_all()) { fprintf(stderr, "synchronize rc %d\n", rc); abort(); }
    for (int i = 0; i < C; i++)
        if (host[i] != model[i]) {
            fprintf(stderr, "seed %llu two_lane %d rename %d groups %d: ciphertext %d differs from the in-order result\n",
                    (unsigned long long)seed, two_lane, (int)rename, (int)groups, i);
            g_failures++;
            break;
        }
    *rot += be->rotations;
    *want_rot += expect;
    *tl_groups += S.dev(0).stats().two_lane_groups.load();
    for (auto* c : h) S.ctxt_destroy(c);
}

int main(int argc, char** argv)
{
    const int seeds = argc > 1 ? atoi(argv[1]) : 40;
    for (int two_lane : {2, 0})
        for (bool rename : {true, false})
            for (bool groups : {true, false}) {
                uint64_t rot = 0, want = 0, tl = 0;
                const int fail0 = g_failures;
                for (int s = 0; s < seeds; s++) run_program(1000 + s, groups, two_lane, rename, &rot, &want, &tl);
                const bool ok = g_failures == fail0 && rot == want;
                if (rot != want) g_failures++;
                printf("two_lane %d rename %d groups %d: rotations %llu for %llu evaluations, two-lane flushes %llu  %s\n", two_lane,
                       (int)rename, (int)groups, (unsigned long long)rot, (unsigned long long)want, (unsigned long long)tl,
                       ok ? "PASS" : "FAIL");
                printf("RESULT {\"two_lane\": %d, \"rename\": %d, \"groups\": %d, \"rotations\": %llu, \"evaluations\": %llu, \"two_lane_groups\": %llu}\n",
                       two_lane, (int)rename, (int)groups, (unsigned long long)rot, (unsigned long long)want, (unsigned long long)tl);
            }
    printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
