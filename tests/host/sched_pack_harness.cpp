// sched_pack_harness.cpp -- the stream scheduler (cufhe_amd/csrc/sched_core.h) with recorded packs, nodes of variable arity
// (DeviceSched::record_pack, what cufhe_amd_enqueue_pack records), against a stub device.
//
// Random programs over 1 or 3 stub devices mix
//   - level-0 gates, copying and on device buffers;
//   - PACKS of arity drawn from {1, 2, 3, 4, 5, 64, 65, 200} into level-2 buffers, with repeated handles and repeated positions;
//   - kind-2 readers of packed TRLWEs (an extraction TRLWE -> lvl0) and in-place kind-2 writers (a refresh, out == in);
//   - gates that overwrite an input of a pack after the pack was recorded, re-packs into a buffer that still has readers;
//   - cufhe_amd_ctxt_destroy of an input right after the pack was recorded, a new ciphertext taking its place (and, when the scheduler
//     lets go of the buffer too early, its device slot);
//   - Synchronize now and then, so that packs meet inputs that have long been resident beside inputs produced a level ago.
// The stub runs every launch at once, all operands of a launch read before any output is written.  Checked in every configuration
// (renaming on / off, "sched_two_lane" forced / off, 1 and 3 devices): the host words of every ciphertext and, fetched at the end, the
// device words on every device equal an in-order interpreter's; no flush that holds a pack is run on two lanes.  The generator counts
// the hazard classes it formed (HAZARDS) and a run that misses one fails.
//
// Usage: sched_pack_harness <seeds>      one line per configuration, "ALL PASS" at the end.  Plain g++; also built with
// -fsanitize=address,undefined and run as it is (tests/test_sched_pack.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "../../cufhe_amd/csrc/sched_core.h"

using namespace cufhe_amd::sched;

static const int kWords0 = 37, kWords2 = 53;
static const int kPack = 6912, kExtract = 3, kRefresh = 2, kCopy = 99, kGateBase = 100;
static const int kPositions = 1024;

static uint32_t mix(int op, uint32_t a, uint32_t b, uint32_t c, uint32_t w)
{
    uint32_t v = a * 0x9E3779B1u + ((b << 5) | (b >> 27)) * 0x85EBCA77u + ((c << 11) | (c >> 21)) * 0xC2B2AE3Du + (uint32_t)op * 0x27D4EB2Fu + w;
    return v ^ (a >> 15) ^ (v << 7);
}
// one term of a pack: a function of ALL words of the input and of its position; terms add mod 2^32 (order-free, like the kernel's)
static void toy_pack_term(uint32_t* acc, const uint32_t* in, int pos)
{
    for (int w = 0; w < kWords2; w++) acc[w] += mix(kPack, in[w % kWords0], in[(w * 7 + pos) % kWords0], (uint32_t)pos, (uint32_t)w);
}
static void toy_op(int op, uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* c)
{
    uint32_t r[kWords2];
    if (op == kExtract) {           // TRLWE -> lvl0
        for (int w = 0; w < kWords0; w++) r[w] = mix(op, a[w], a[kWords2 - 1 - w], 0u, (uint32_t)w);
        memcpy(out, r, kWords0 * 4);
    } else if (op == kRefresh) {    // TRLWE -> TRLWE, in place
        for (int w = 0; w < kWords2; w++) r[w] = mix(op, a[w], a[(w + 7) % kWords2], 0u, (uint32_t)w);
        memcpy(out, r, kWords2 * 4);
    } else {                        // a level-0 gate
        for (int w = 0; w < kWords0; w++) r[w] = mix(op, a[w], b ? b[w] : 0u, c ? c[w] : 0u, (uint32_t)w);
        memcpy(out, r, kWords0 * 4);
    }
}
static int out_words(int op) { return op == kPack || op == kRefresh ? kWords2 : kWords0; }

struct Ev { int unused = 0; };

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
        const uint64_t group = ds ? ds->stats().groups : 0;      // flush() counts the group before it launches it (no worker threads here)
        std::vector<std::vector<uint32_t>> res(n, std::vector<uint32_t>(kWords2, 0u));
        for (size_t i = 0; i < n; i++) {
            if (g[i].op == kCopy) continue;
            if (g[i].op == kPack) {
                if (level != 2) { fprintf(stderr, "a pack in a launch of kind %d\n", level); abort(); }
                groups_with_pack.insert(group);
                const PackNode* node = pack_node(g[i]);
                if (!node || node->terms.empty() || g[i].in1 || g[i].in2) { fprintf(stderr, "a pack without its term list\n"); abort(); }
                for (const PackTerm& t : node->terms) toy_pack_term(res[i].data(), t.in, t.pos);
                terms += node->terms.size();
            } else toy_op(g[i].op, res[i].data(), g[i].in0, g[i].in1, g[i].in2);
        }
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
    int gate_weight(int op) override { return op == kCopy || op == kPack ? 0 : 1; }
    int lowering(int op) override { return op == kPack ? 1 : 0; }
    int run_gates_lane(int s, int level, const GateRef* g, size_t n, int lane) override
    {
        if (lane == 0 || lane == 1) groups_on_lanes.insert(ds ? ds->stats().groups : 0);
        return run_gates(s, level, g, n);
    }
    DeviceSched* ds = nullptr;
    std::set<uint64_t> groups_with_pack, groups_on_lanes;
    uint64_t terms = 0;

   private:
    bool two_lane_;
};

static int g_failures = 0;

enum Hazard { kWarInLow, kWarInHigh, kWarOut, kWawOut, kDestroyed, kHazards };
static const char* const kHazardName[kHazards] = {"war_input_below_3", "war_input_from_3", "war_out", "waw_out", "destroyed_input"};
struct Totals { uint64_t hazard[kHazards] = {0, 0, 0, 0, 0}; uint64_t packs = 0, terms = 0, tl = 0, gates = 0; };

static void run_program(uint64_t seed, int gpus, bool packs, int two_lane, bool rename, Totals* t)
{
    std::mt19937_64 rng(seed);
    std::vector<SyncBackend*> be;
    Scheduler S(gpus, false, [&](int) { be.push_back(new SyncBackend(two_lane != 0)); return be.back(); });
    for (int d = 0; d < gpus; d++) {
        be[(size_t)d]->ds = &S.dev(d);
        S.dev(d).two_lane = two_lane;
        S.dev(d).rename_outputs = rename;
        S.dev(d).copy_op = kCopy;
        S.dev(d).set_level_flush_gates(8 + rng() % 40);
    }
    const int C = 48, T = 4;
    void* streams[3] = {(void*)0x1001, (void*)0x1002, (void*)0x1003};
    // the in-order interpreter: the host words and the words of every device buffer of every ciphertext
    std::vector<std::vector<uint32_t>> host(C + T), mhost(C + T);
    std::vector<std::vector<std::vector<uint32_t>>> mdev((size_t)gpus, std::vector<std::vector<uint32_t>>(C + T));
    std::vector<cufhe_amd_ctxt*> h(C + T);
    std::string err;
    auto fail_rc = [&](const char* what, int rc) { fprintf(stderr, "seed %llu: %s rc %d\n", (unsigned long long)seed, what, rc); abort(); };
    auto create = [&](int i) {
        const int words = i < C ? kWords0 : kWords2;
        // (a destroyed ciphertext's host words are free to go: ctxt_destroy has saved them for the uploads still on record)
        host[i] = std::vector<uint32_t>((size_t)words);
        for (int w = 0; w < words; w++) host[i][w] = (uint32_t)rng();
        mhost[i] = host[i];
        if (S.ctxt_create(i < C ? 0 : 2, host[i].data(), &h[i], &err)) { fprintf(stderr, "ctxt_create: %s\n", err.c_str()); abort(); }
        for (int d = 0; d < gpus; d++) {          // every device buffer starts as the host words
            if (int rc = S.dev(d).record_copy(streams[0], h[i], true)) fail_rc("record_copy", rc);
            mdev[(size_t)d][i] = mhost[i];
        }
    };
    for (int i = 0; i < C + T; i++) create(i);
    // since the last Synchronize: the lowest input index under which a recorded pack names ciphertext i (-1: none), the recorded
    // readers / writers of table j
    std::vector<int> pack_input(C, -1);
    std::vector<int> table_readers(T, 0), table_writers(T, 0);
    auto forget_pending = [&] {
        std::fill(pack_input.begin(), pack_input.end(), -1);
        std::fill(table_readers.begin(), table_readers.end(), 0);
        std::fill(table_writers.begin(), table_writers.end(), 0);
    };
    auto value = [&](bool copying, int d, int i) -> std::vector<uint32_t>& {      // what an op on device d reads for ciphertext i
        if (copying) mdev[(size_t)d][i] = mhost[i];
        return mdev[(size_t)d][i];
    };
    auto wrote_input = [&](int o) {
        if (pack_input[o] < 0) return;
        t->hazard[pack_input[o] < 3 ? kWarInLow : kWarInHigh]++;
        pack_input[o] = -1;
    };
    static const int kArity[8] = {1, 2, 3, 4, 5, 64, 65, 200};
    const int G = 120 + (int)(rng() % 80);
    int last_pack_input = -1;                       // an input at index >= 3 of the newest pack: the next gate may overwrite it
    for (int gi = 0; gi < G; gi++) {
        void* st = streams[rng() % 3];
        const int d = (int)(rng() % (unsigned)gpus);
        const bool copying = seed % 2 == 0 && rng() % 3 == 0;      // (odd seeds: device forms only, so nothing but the program's shape decides about two lanes)
        const unsigned pick = packs ? (unsigned)(rng() % 20) : 19u;
        if (pick < 5) {                 // a pack
            const int n = kArity[rng() % 8], table = (int)(rng() % T);
            std::vector<cufhe_amd_ctxt*> ins((size_t)n);
            std::vector<int> idx((size_t)n);
            std::vector<int32_t> pos((size_t)n);
            for (int m = 0; m < n; m++) {
                idx[m] = m > 0 && rng() % 6 == 0 ? idx[rng() % (unsigned)m] : (int)(rng() % C);          // repeated handles
                pos[m] = m > 0 && rng() % 6 == 0 ? pos[rng() % (unsigned)m] : (int32_t)(rng() % kPositions);   // repeated positions
                ins[m] = h[idx[m]];
            }
            std::vector<uint32_t> r(kWords2, 0u);
            for (int m = 0; m < n; m++) toy_pack_term(r.data(), value(copying, d, idx[m]).data(), pos[m]);
            mdev[(size_t)d][C + table] = r;
            if (copying) mhost[C + table] = r;
            if (table_readers[table]) t->hazard[kWarOut]++;
            if (table_writers[table]) t->hazard[kWawOut]++;
            if (int rc = S.dev(d).record_pack(st, kPack, copying, h[C + table], ins.data(), pos.data(), (size_t)n)) fail_rc("record_pack", rc);
            table_readers[table] = 0;
            table_writers[table]++;
            for (int m = 0; m < n; m++)
                if (pack_input[idx[m]] < 0 || m < pack_input[idx[m]]) pack_input[idx[m]] = m;
            t->packs++;
            // an input that the pack names at index >= 3 only: destroyed at once, one time in three; else kept for the next gate to overwrite
            last_pack_input = -1;
            for (int m = n - 1; m >= 3 && last_pack_input < 0; m--) {
                bool low = false;
                for (int k = 0; k < 3; k++) low = low || idx[k] == idx[m];
                if (!low) last_pack_input = idx[m];
            }
            if (last_pack_input >= 0 && rng() % 3 == 0) {
                const int x = last_pack_input;
                S.ctxt_destroy(h[x]);
                t->hazard[kDestroyed]++;
                pack_input[x] = -1;
                // its successor takes the free device slot if the scheduler has let go of it, and uploads into it at the earliest level
                create(x);
                last_pack_input = -1;
            }
        } else if (pick < 7) {          // a kind-2 reader of a table: TRLWE -> lvl0
            const int table = (int)(rng() % T), o = (int)(rng() % C);
            std::vector<uint32_t> r(kWords0);
            toy_op(kExtract, r.data(), value(copying, d, C + table).data(), nullptr, nullptr);
            mdev[(size_t)d][o] = r;
            if (copying) mhost[o] = r;
            wrote_input(o);
            cufhe_amd_ctxt* ins[3] = {h[C + table], nullptr, nullptr};
            if (int rc = S.dev(d).record_gate(st, kExtract, copying, h[o], ins, 2)) fail_rc("record_gate", rc);
            table_readers[table]++;
        } else if (pick < 8) {          // an in-place kind-2 writer of a table
            const int table = (int)(rng() % T);
            std::vector<uint32_t> r(kWords2);
            toy_op(kRefresh, r.data(), value(copying, d, C + table).data(), nullptr, nullptr);
            mdev[(size_t)d][C + table] = r;
            if (copying) mhost[C + table] = r;
            cufhe_amd_ctxt* ins[3] = {h[C + table], nullptr, nullptr};
            if (int rc = S.dev(d).record_gate(st, kRefresh, copying, h[C + table], ins, 2)) fail_rc("record_gate", rc);
            table_readers[table] = 0;
            table_writers[table]++;
        } else if (pick < 9) {          // Synchronize: everything retires, what is recorded next meets resident values
            if (int rc = S.synchronize_all()) fail_rc("synchronize", rc);
            forget_pending();
            last_pack_input = -1;
        } else {                        // a level-0 gate; now and then onto an input (index >= 3) of the pack just recorded
            int in[3];
            const int arity = 1 + (int)(rng() % 3);
            for (int i = 0; i < 3; i++) in[i] = (int)(rng() % C);
            int o = (int)(rng() % C);
            if (last_pack_input >= 0 && rng() % 2 == 0) o = last_pack_input;
            last_pack_input = -1;
            const int op = kGateBase + (int)(rng() % 9);
            std::vector<uint32_t> r(kWords0);
            const uint32_t* a = value(copying, d, in[0]).data();
            const uint32_t* b = arity >= 2 ? value(copying, d, in[1]).data() : nullptr;
            const uint32_t* c = arity == 3 ? value(copying, d, in[2]).data() : nullptr;
            toy_op(op, r.data(), a, b, c);
            mdev[(size_t)d][o] = r;
            if (copying) mhost[o] = r;
            wrote_input(o);
            cufhe_amd_ctxt* ins[3] = {h[in[0]], arity >= 2 ? h[in[1]] : nullptr, arity == 3 ? h[in[2]] : nullptr};
            if (int rc = S.dev(d).record_gate(st, op, copying, h[o], ins)) fail_rc("record_gate", rc);
            t->gates++;
        }
    }
    auto compare = [&](const char* what, const std::vector<std::vector<uint32_t>>& want) {
        for (int i = 0; i < C + T; i++)
            if (host[i] != want[i]) {
                fprintf(stderr, "seed %llu gpus %d two_lane %d rename %d packs %d: %s of ciphertext %d differ from the in-order result\n",
                        (unsigned long long)seed, gpus, two_lane, (int)rename, (int)packs, what, i);
                g_failures++;
                return;
            }
    };
    if (int rc = S.synchronize_all()) fail_rc("synchronize", rc);
    compare("the host words", mhost);
    for (int d = 0; d < gpus; d++) {
        for (int i = 0; i < C + T; i++)
            if (int rc = S.dev(d).record_copy(streams[0], h[i], false)) fail_rc("record_copy", rc);
        if (int rc = S.synchronize_all()) fail_rc("synchronize", rc);
        compare("the device words", mdev[(size_t)d]);
    }
    for (int d = 0; d < gpus; d++) {
        for (uint64_t g : be[(size_t)d]->groups_with_pack)
            if (be[(size_t)d]->groups_on_lanes.count(g)) {
                fprintf(stderr, "seed %llu: a flush that holds a pack ran on two lanes\n", (unsigned long long)seed);
                g_failures++;
            }
        t->terms += be[(size_t)d]->terms;
        t->tl += S.dev(d).stats().two_lane_groups.load();
    }
    for (auto* c : h) S.ctxt_destroy(c);
}

int main(int argc, char** argv)
{
    const int seeds = argc > 1 ? atoi(argv[1]) : 30;
    for (int gpus : {1, 3})
        for (int two_lane : {2, 0})
            for (bool rename : {true, false})
                for (bool packs : {true, false}) {
                    Totals t;
                    const int fail0 = g_failures;
                    for (int s = 0; s < seeds; s++) run_program(7000 + (uint64_t)s, gpus, packs, two_lane, rename, &t);
                    if (packs)
                        for (int k = 0; k < kHazards; k++)
                            if (t.hazard[k] < 3) {
                                fprintf(stderr, "hazard class %s formed %llu times\n", kHazardName[k], (unsigned long long)t.hazard[k]);
                                g_failures++;
                            }
                    const bool ok = g_failures == fail0;
                    printf("gpus %d two_lane %d rename %d packs %d: %llu packs of %llu terms, %llu gates, two-lane flushes %llu  %s\n", gpus, two_lane,
                           (int)rename, (int)packs, (unsigned long long)t.packs, (unsigned long long)t.terms, (unsigned long long)t.gates,
                           (unsigned long long)t.tl, ok ? "PASS" : "FAIL");
                    printf("RESULT {\"gpus\": %d, \"two_lane\": %d, \"rename\": %d, \"with_packs\": %d, \"packs\": %llu, \"terms\": %llu, \"gates\": %llu, "
                           "\"two_lane_groups\": %llu", gpus, two_lane, (int)rename, (int)packs, (unsigned long long)t.packs, (unsigned long long)t.terms,
                           (unsigned long long)t.gates, (unsigned long long)t.tl);
                    for (int k = 0; k < kHazards; k++) printf(", \"%s\": %llu", kHazardName[k], (unsigned long long)t.hazard[k]);
                    printf("}\n");
                }
    printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
