// sched_harness.cpp -- the stream scheduler (cufhe_amd/csrc/sched_core.h) against a stubbed device layer.
//
// The stub is an asynchronous machine with the ordering rules of HIP streams and nothing more:
// work submitted to one internal stream runs in order, streams are ordered only by events, copies
// read their source when they EXECUTE, and execution happens at arbitrary later moments (a seeded
// random interleaving, advanced only when the scheduler queries or waits for an event).  "Gates" are
// a non-commutative word mixer, executed in random order within a launch -- so a scheduler that puts
// two dependent gates into one launch, lets a copy overtake a gate, or delivers a stale result fails
// the comparison with a plain in-order interpreter of the reference API's semantics
// (include/cufhe_gpu.cuh:193-313, src/cufhe_gates_gpu.cu:148-167).
//
// Usage: sched_harness <seeds> <gpus> <threaded 0|1>      prints one line per check, "ALL PASS" at the end.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <random>

#include "../../cufhe_amd/csrc/sched_core.h"
#include "../../cufhe_amd/csrc/launch_plan.h"

using namespace cufhe_amd::sched;

static const int kWords[4] = {37, 53, 71, 89};  // toy ciphertext sizes (odd on purpose): lvl0, lvl1, TRLWE, TRGSW holder (NTT domain)
enum { OP_NOT = 12, OP_COPY = 13, OP_MUX = 10, OP_NMUX = 11, TL_BOOT = 100, TL_REFRESH = 101, TL_SEIKS = 102,
       TL_CMUX = 103,           // CUFHE_AMD_TL_CMUX: ins = {c1, c0, cs} of levels 2, 2, 3 -> level 2 (sched_hip.inc.h, cufhe_amd_enqueue_cmux)
       TL_CB = 104,             // CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP: lvl0 -> a level-3 holder
       OP_HOME_COPY = 99,       // DeviceSched::copy_op here: the scheduler's own copy of a renamed value back to the ciphertext's buffer (the user-visible ops, Copy included, are word mixers)
       // user gates (cufhe_amd_define_gate[_multi]): definition k, output j is USER_BASE + k + j * kUserDefs as in CUFHE_AMD_USER_OP_OUTPUT; the toy
       // definitions have arity 1 + k % 3 and 1, 2, 4 or 8 outputs (user_nout)
       USER_BASE = 200, kUserDefs = 64, kUserOutputs = 8,
       TL_SEIKS_AT0 = 1000, kSeiksIdx = 64,         // CUFHE_AMD_TL_SEIKS_AT(j): level 2 -> level 0, kind 2, j in the op id
       TL_CMUX_ROT0 = 2000, kRotExps = 128 };       // CUFHE_AMD_TL_CMUX_ROTATE(e): ins = {c, nullptr, cs}, usually in place
static int user_op(int k, int j) { return USER_BASE + k + j * kUserDefs; }
static bool is_user(int op) { return op >= USER_BASE && op < USER_BASE + kUserDefs * kUserOutputs; }
static int user_def(int op) { return (op - USER_BASE) % kUserDefs; }
static int user_arity(int k) { return 1 + k % 3; }
static int user_nout(int k) { return k < 12 ? 1 : k < 16 ? 2 : k < 20 ? 4 : 8; }       // definitions 0..23 exist
static bool is_seiks_at(int op) { return op >= TL_SEIKS_AT0 && op < TL_SEIKS_AT0 + kSeiksIdx; }
static bool is_cmux_rot(int op) { return op >= TL_CMUX_ROT0 && op < TL_CMUX_ROT0 + kRotExps; }
static bool is_tl(int op) { return (op >= TL_BOOT && op <= TL_CB) || is_seiks_at(op) || is_cmux_rot(op); }
static int tl_in_level(int op) { return op == TL_BOOT || op == TL_CB ? 0 : 2; }
static int tl_out_level(int op) { return op == TL_SEIKS || is_seiks_at(op) ? 0 : op == TL_CB ? 3 : 2; }

static inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static uint32_t mix(int op, uint32_t a, uint32_t b, uint32_t c, uint32_t w)
{
    uint32_t v = a * 0x9E3779B1u + rotl(b, 5) * 0x85EBCA77u + rotl(c, 11) * 0xC2B2AE3Du + (uint32_t)op * 0x27D4EB2Fu + w;
    return v ^ (a >> 15) ^ (v << 7);
}
static void toy_gate(int op, int level, uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* c)
{
    if (op == OP_HOME_COPY) { memmove(out, a, kWords[level] * 4); return; }
    if (op == TL_CMUX || is_cmux_rot(op)) {      // every word of the selector enters: a torn or stale holder shows
        const int wt = kWords[2], ws = kWords[3], e = is_cmux_rot(op) ? op - TL_CMUX_ROT0 + 1 : 0;
        std::vector<uint32_t> r(wt);
        for (int w = 0; w < wt; w++) {
            const uint32_t sel = c[w] + rotl(c[(w * 5 + 2) % ws], 9) + c[ws - 1 - w % 18];
            r[w] = mix(op, a[w], is_cmux_rot(op) ? a[(w + e) % wt] : b[w], sel, (uint32_t)w);
        }
        memcpy(out, r.data(), r.size() * 4);      // (in place on c1, c0 or c: all operands were read first, like the kernels)
        return;
    }
    if (is_tl(op)) {          // the other TRLWE-level operations map one ciphertext kind to another
        const int wi = kWords[tl_in_level(op)], wo = kWords[tl_out_level(op)];
        std::vector<uint32_t> r(wo);
        for (int w = 0; w < wo; w++) r[w] = mix(op, a[w % wi], a[(w * 7 + 3) % wi], 0u, (uint32_t)w);
        memcpy(out, r.data(), r.size() * 4);
        return;
    }
    std::vector<uint32_t> r(kWords[level]);
    for (int w = 0; w < kWords[level]; w++) r[w] = mix(op, a[w], b ? b[w] : 0u, c ? c[w] : 0u, (uint32_t)w);
    memcpy(out, r.data(), r.size() * 4);
}

static bool g_two_lane = true;     // argv[6]: flushes of several levels are scheduled gate by gate on two lanes when eligible (DeviceSched::compile_two_lane)
static bool g_zero_copy = false;   // argv[5]: the stub's pinned memory is "visible to the device" (Backend::device_alias): no staging copies

static std::atomic<bool> g_hold_launch{false};   // a launch worker stops at the start of its next launch (device_alias) until this is cleared: a slow worker, on demand
static std::atomic<int> g_stub_failures{0};      // what the stub device itself refused (counted into the run's failures)

struct FakeEvent { uint64_t submitted = 0, completed = 0; };

class FakeBackend : public Backend {
   public:
    FakeBackend(int nstreams, uint64_t seed) : q_(nstreams), rng_(seed) {}
    void bind_thread() override {}
    int num_streams() override { return (int)q_.size(); }
    int words(int level) override { return kWords[level]; }
    int alloc_device(size_t bytes, void** p) override { *p = calloc(1, bytes); return 0; }
    int free_device(void* p) override { free(p); return 0; }
    int alloc_pinned(size_t bytes, void** p) override { *p = malloc(bytes); memset(*p, 0xAB, bytes); return 0; }
    int free_pinned(void* p) override { free(p); return 0; }
    // the launch worker announces itself here (DeviceSched's worker thread calls this once when it starts): the hold below is for it alone
    int bind_worker_thread() override
    {
        std::lock_guard<std::mutex> lk(mu_);
        worker_ = std::this_thread::get_id();
        return 0;
    }
    void* device_alias(void* pinned) override
    {
        bool is_worker;
        { std::lock_guard<std::mutex> lk(mu_); is_worker = worker_ == std::this_thread::get_id(); }
        // g_hold_launch: the worker waits here, at the start of a launch -- never the issuing thread, and never for ever
        for (long spins = 0; is_worker && g_hold_launch.load(); spins++) {
            if (spins == 2000000000L) { fprintf(stderr, "stub device: the launch worker was held and never released\n"); abort(); }
            std::this_thread::yield();
        }
        return g_zero_copy ? pinned : nullptr;
    }
    uint64_t launches_so_far() { std::lock_guard<std::mutex> lk(mu_); return launches; }
    int h2d(int s, void* dst, const void* src, size_t bytes) override { push(s, [=] { memcpy(dst, src, bytes); }); return 0; }
    int d2h(int s, void* dst, const void* src, size_t bytes) override { push(s, [=] { memcpy(dst, src, bytes); }); return 0; }
    int copy_ctxts(int s, const CopyRec* recs, size_t n, uint32_t* staging, bool to_ctxt) override
    {
        std::vector<CopyRec> r(recs, recs + n);
        push(s, [=] {
            for (const CopyRec& c : r) {
                if (to_ctxt) memcpy(c.dev, staging + c.slot, kWords[c.level] * 4);
                else memcpy(staging + c.slot, c.dev, kWords[c.level] * 4);
            }
        });
        return 0;
    }
    int run_gates(int s, int level, const GateRef* g, size_t n) override
    {
        std::vector<GateRef> v(g, g + n);
        {
            std::lock_guard<std::mutex> lk(mu_);      // the launch worker and the issuing thread (event_query) share rng_
            launches++;
            std::shuffle(v.begin(), v.end(), rng_);
        }
        // the launch of kind 2 knows the TRLWE-level operations only (lower_trlwe_ops, capi.hip: "unknown TRLWE-level op"): a copy of a
        // renamed TRLWE or holder back to its buffer has no kernel there, so such buffers must never be renamed
        for (const GateRef& r : v)
            if (level == 2 ? !is_tl(r.op) : is_tl(r.op)) { printf("FAIL stub device: op %d in a launch of kind %d\n", r.op, level); g_stub_failures++; }
        push(s, [=] {
            for (const GateRef& r : v) toy_gate(r.op, level, r.out, r.in0, r.in1, r.in2);
        });
        return 0;
    }
    int event_create(void** ev) override { *ev = new FakeEvent(); return 0; }
    int event_destroy(void* ev) override
    {
        // as in HIP, a wait that was enqueued on the event stays valid when the event object goes: the scheduler only destroys
        // completed events, so such a wait is satisfied
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = (FakeEvent*)ev;
        auto release = [&](std::deque<Op>& q) {
            for (Op& op : q)
                if (op.wait == e) {
                    if (e->completed < op.target) { fprintf(stderr, "stub device: an event with a pending, unsatisfied wait was destroyed\n"); abort(); }
                    op.wait = nullptr;
                }
        };
        for (auto& q : q_) release(q);
        for (auto& kv : cq_) release(kv.second);
        delete e;
        return 0;
    }
    int event_record(int s, void* ev) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = (FakeEvent*)ev;
        e->submitted++;
        q_[s].push_back({[e] { e->completed++; }, nullptr, 0});
        return 0;
    }
    int stream_wait(int s, void* ev) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = (FakeEvent*)ev;
        q_[s].push_back({[] {}, e, e->submitted});
        return 0;
    }
    int event_query(void* ev) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        const int n = (int)(rng_() % 4);
        for (int i = 0; i < n; i++) pump_one();
        FakeEvent* e = (FakeEvent*)ev;
        return e->completed == e->submitted ? 1 : 0;
    }
    int event_sync(void* ev) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = (FakeEvent*)ev;
        while (e->completed != e->submitted)
            if (!pump_one()) { fprintf(stderr, "stub device: event can never complete (missing dependence?)\n"); abort(); }
        return 0;
    }
    std::string error_text() override { return "stub"; }
    // two lanes: a toy model under which the per-gate plan wins whenever a flush is eligible -- the harness is after its ORDER, not its timing
    bool lane_model(LaneModel* m) override
    {
        if (!g_two_lane) return false;
        m->chain_gates = 3; m->bulk_gates = 8; m->chain_ms = 1.0; m->bulk_ms = 3.0;
        return true;
    }
    double launch_ms(size_t n) override { return n ? 1000.0 : 0.0; }
    int gate_weight(int op) override { return op == OP_MUX || op == OP_NMUX ? 2 : op == OP_HOME_COPY ? 0 : 1; }
    bool shares_rotation(int op) override { return is_user(op) && user_nout(user_def(op)) > 1; }      // as HipBackend: siblings stay in the level order
    int run_gates_lane(int s, int level, const GateRef* g, size_t n, int lane) override
    {
        { std::lock_guard<std::mutex> lk(mu_); lane_launches[lane == 0 ? 0 : 1]++; }
        return run_gates(s, level, g, n);
    }
    uint64_t lane_launches[2] = {0, 0};
    // the caller's own streams (raw handles of Stream::st()): queues like the internal ones, filled by the test itself
    int caller_stream_wait(void* cs, void* ev) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = (FakeEvent*)ev;
        caller_waits++;
        cq_[cs].push_back({[] {}, e, e->submitted});
        return 0;
    }
    int wait_for_caller_stream(int s, void* cs) override
    {
        std::lock_guard<std::mutex> lk(mu_);
        FakeEvent* e = new FakeEvent();
        owned_.push_back(e);
        e->submitted++;
        cq_[cs].push_back({[e] { e->completed++; }, nullptr, 0});
        q_[s].push_back({[] {}, e, e->submitted});
        return 0;
    }
    void push_caller(void* cs, std::function<void()> fn)
    {
        std::lock_guard<std::mutex> lk(mu_);
        cq_[cs].push_back({std::move(fn), nullptr, 0});
    }
    ~FakeBackend() override { for (FakeEvent* e : owned_) delete e; }
    uint64_t caller_waits = 0;
    void drain()
    {
        std::lock_guard<std::mutex> lk(mu_);
        while (pump_one()) {}
    }
    uint64_t launches = 0;

   private:
    struct Op { std::function<void()> fn; FakeEvent* wait; uint64_t target; };
    void push(int s, std::function<void()> fn)
    {
        std::lock_guard<std::mutex> lk(mu_);
        q_[s].push_back({std::move(fn), nullptr, 0});
    }
    bool pump_one()
    {
        std::vector<std::deque<Op>*> ready;
        auto is_ready = [](std::deque<Op>& q) { return !q.empty() && (!q.front().wait || q.front().wait->completed >= q.front().target); };
        for (auto& q : q_)
            if (is_ready(q)) ready.push_back(&q);
        for (auto& kv : cq_)
            if (is_ready(kv.second)) ready.push_back(&kv.second);
        if (ready.empty()) return false;
        std::deque<Op>* q = ready[rng_() % ready.size()];
        Op op = std::move(q->front());
        q->pop_front();
        op.fn();
        return true;
    }
    std::mutex mu_;
    std::thread::id worker_;
    std::vector<std::deque<Op>> q_;
    std::map<void*, std::deque<Op>> cq_;
    std::vector<FakeEvent*> owned_;
    std::mt19937_64 rng_;
};

// ---- in-order interpreter of the reference semantics ----
struct ModelCtxt {
    int level;
    std::vector<uint32_t> host;                 // what tlwehost will eventually hold
    std::vector<std::vector<uint32_t>> dev;     // per device
    std::vector<bool> dev_defined;
};

static bool g_rename = false;      // argv[4]: outputs take fresh device buffers instead of waiting (DeviceSched::rename_outputs)

struct Test {
    int G;
    Scheduler* S;
    std::vector<FakeBackend*> be;
    std::mt19937_64 rng;
    struct C {
        cufhe_amd_ctxt* h; std::vector<uint32_t> host; ModelCtxt m; void* last_host_writer_stream = nullptr; bool alive = true;
        std::vector<uint32_t*> home;                   // the device pointers as of creation: what the reference publishes as tlwedevices
        std::vector<void*> last_dev_writer_stream;     // per device: the caller stream of the newest gate that wrote the device value
        std::vector<void*> last_dev_upload_stream;     // per device: the caller stream of an upload that is the NEWEST write of the device value (nullptr: a gate's write is)
        std::vector<void*> only_stream;                // per device: the one caller stream all recorded accesses were issued on (nullptr: none yet, kMany: several)
        // a ciphertext the program only ever touches on ONE stream of one device: what a caller may read and write through that stream's raw
        // handle with a defined outcome (across streams the reference orders nothing)
        void* priv_stream = nullptr;
        int priv_dev = -1;
        // what the generator needs to recognise the hazard classes (note_hazards): the program still ON RECORD is, conservatively, what was
        // issued since the last Synchronize
        struct Track { int wkind = 0; bool on_record = false, read = false, cmux_read = false, renamed_k2 = false, in_place_rot = false; int rot_chain = 0; void* wstream = nullptr; };
        std::vector<Track> tr;                         // per device
        int hk = 0;                                    // the kind of record whose result is on its way to (or in) `host` since the last Synchronize
        void* hk_wstream = nullptr;                    // ... the stream that computed it
        bool hk_by_d2h = false, hk_renamed = false;    // ... fetched by an explicit D2H; computed into a renamed buffer
        bool copying_cmux_named = false;               // a copying CMUX that took the holder's present host words is on record
    };
    enum { WK_NONE, WK_UPLOAD, WK_GATE, WK_USER, WK_BOOT, WK_REFRESH, WK_SEIKS, WK_SEIKS_AT, WK_CMUX, WK_ROT, WK_CB, WK_CALLER };
    static int wk_of(int op)
    {
        return op == TL_BOOT ? WK_BOOT : op == TL_REFRESH ? WK_REFRESH : op == TL_SEIKS ? WK_SEIKS : is_seiks_at(op) ? WK_SEIKS_AT : op == TL_CMUX ? WK_CMUX :
               is_cmux_rot(op) ? WK_ROT : op == TL_CB ? WK_CB : is_user(op) ? WK_USER : WK_GATE;
    }
    std::map<std::string, uint64_t>* haz = nullptr;    // hazard-class counters of the run (random_program)
    std::map<std::pair<int, uint32_t>, int> level_mask;      // (device, dependence level) -> kinds recorded there: 1 kind 0, 2 kind 1, 4 kind 2, 8 a circuit bootstrap
    void count(const char* cls) { if (haz) (*haz)[cls]++; }
    static void* many() { return (void*)(uintptr_t)-1; }
    static void touch(C* c, int dev, void* st) { void*& o = c->only_stream[dev]; o = (o == nullptr || o == st) ? st : many(); }
    // reads the caller enqueued on a raw handle: what the buffer must hold when the read executes
    struct CallerRead { std::vector<uint32_t> got, want; bool done = false; };
    std::vector<std::shared_ptr<CallerRead>> caller_reads;
    std::vector<C*> ct;
    int failures = 0;

    Test(int gpus, bool threaded, uint64_t seed, int nstreams) : G(gpus), rng(seed)
    {
        S = new Scheduler(gpus, threaded, [&](int d) {
            FakeBackend* b = new FakeBackend(nstreams, seed * 131 + d);
            be.push_back(b);
            return b;
        });
        for (int d = 0; d < gpus; d++) {
            S->dev(d).rename_outputs = g_rename; S->dev(d).two_lane = g_two_lane ? 1 : 0; S->dev(d).copy_op = OP_HOME_COPY;
            S->dev(d).parallel_copy_min = seed % 2 ? 3 : 1024;       // every other program: the gathers and deliveries split over the copy threads
        }
    }
    ~Test()
    {
        S->synchronize_all();
        for (C* c : ct) { if (c->alive) S->ctxt_destroy(c->h); delete c; }
        delete S;
    }
    C* make(int level)
    {
        C* c = new C();
        c->host.resize(kWords[level]);
        for (auto& w : c->host) w = (uint32_t)rng();
        std::string err;
        if (S->ctxt_create(level, c->host.data(), &c->h, &err)) { fprintf(stderr, "ctxt_create: %s\n", err.c_str()); abort(); }
        c->m.level = level;
        c->m.host = c->host;
        c->m.dev.assign(G, std::vector<uint32_t>(kWords[level], 0));
        c->m.dev_defined.assign(G, false);
        for (int d = 0; d < G; d++) c->home.push_back(c->h->d[d].dev);
        c->last_dev_writer_stream.assign(G, nullptr);
        c->only_stream.assign(G, nullptr);
        c->last_dev_upload_stream.assign(G, nullptr);
        c->tr.assign(G, C::Track());
        ct.push_back(c);
        return c;
    }
    bool trace = getenv("SCHED_HARNESS_TRACE") != nullptr;
    int idx(C* c) { for (size_t i = 0; i < ct.size(); i++) if (ct[i] == c) return (int)i; return -1; }
    void gate(int dev, void* st, int op, bool copying, C* out, C* a, C* b, C* c3) { issue(dev, st, &op, copying, &out, 1, a, b, c3, false); }
    // the outputs of one multi-output evaluation, recorded together (cufhe_amd_enqueue_gate_multi -> record_gate_group)
    void gate_group(int dev, void* st, int k, bool copying, const std::vector<C*>& outs, C* a, C* b, C* c3)
    {
        int ops[kUserOutputs];
        for (size_t j = 0; j < outs.size(); j++) ops[j] = user_op(k, (int)j);
        bool all_read = true;
        for (C* o : outs) all_read = all_read && o->tr[dev].read;
        if (all_read) count("group_outputs_all_have_readers");
        issue(dev, st, ops, copying, outs.data(), outs.size(), a, b, c3, true);
        // record_gate_group's promise to the lowering: all outputs in ONE dependence level (one launch of their kind, so one shared rotation)
        for (C* o : outs)
            if (o->h->d[dev].wdepth != outs[0]->h->d[dev].wdepth) { failures++; printf("FAIL the outputs of one evaluation were recorded at different levels (ctxt [%d])\n", idx(o)); break; }
    }
    // The hazard classes a record belongs to, from the generator's own bookkeeping (before the record's effects are applied to it).
    void note_hazards(int dev, void* st, int op, bool copying, C* out, C* const (&ins)[3])
    {
        const bool cmux = op == TL_CMUX || is_cmux_rot(op);
        int sk[3] = {0, 0, 0};        // the kind of record that produced each operand, if that record is still on record
        for (int i = 0; i < 3; i++)
            if (ins[i]) sk[i] = copying ? ins[i]->hk : ins[i]->tr[dev].on_record ? ins[i]->tr[dev].wkind : (int)WK_NONE;
        if (op == TL_BOOT && (sk[0] == WK_GATE || sk[0] == WK_USER)) count("raw_gate_to_tl_bootstrap");
        if (!is_tl(op) && (sk[0] == WK_SEIKS_AT || sk[1] == WK_SEIKS_AT || sk[2] == WK_SEIKS_AT)) count(is_user(op) ? "raw_seiks_at_to_user_gate" : "raw_seiks_at_to_gate");
        if (cmux && sk[2] == WK_CB) count("raw_circuit_bootstrap_to_selector");
        if (is_seiks_at(op) && sk[0] == WK_CMUX) count("raw_cmux_to_seiks_at");
        C::Track& to = out->tr[dev];
        if (to.on_record) count(out->m.level == 0 ? "waw_level0" : out->m.level == 1 ? "waw_level1" : out->m.level == 2 ? "waw_level2" : "waw_level3");
        if (out->m.level == 2 && to.cmux_read) count(out == ins[0] || out == ins[1] ? "war_trlwe_in_place_after_cmux" : "war_trlwe_after_cmux");
        if (out->m.level == 3 && to.cmux_read) count("war_holder_circuit_bootstrap_after_cmux");
        if (op == TL_CMUX && out == ins[0]) count("cmux_in_place_on_c1");
        if (op == TL_CMUX && out == ins[1] && out != ins[0]) count("cmux_in_place_on_c0");
        int chain = 0;
        if (is_cmux_rot(op) && out == ins[0]) {
            chain = to.in_place_rot && to.on_record ? to.rot_chain + 1 : 1;
            if (chain == 3) count("cmux_rotate_chain_of_3_in_place");
        }
        for (int i = 0; i < 3; i++) {
            if (!ins[i]) continue;
            C::Track& ti = ins[i]->tr[dev];
            if (copying) { ti.wkind = WK_UPLOAD; ti.on_record = true; ti.in_place_rot = false; }     // (what the reference's upload writes; the scheduler may find it already there)
            ti.read = true;
            if (cmux) ti.cmux_read = true;
        }
        if (cmux && copying) ins[2]->copying_cmux_named = true;
        to.wkind = wk_of(op);
        to.on_record = true;
        to.read = to.cmux_read = false;
        to.wstream = st;
        to.in_place_rot = chain > 0;
        to.rot_chain = chain;
        // (a lvl0 output of a kind-2 op is renamed like a gate's: is its value in another buffer than the ciphertext's own now?)
        to.renamed_k2 = (op == TL_SEIKS || is_seiks_at(op)) && out->h->d[dev].dev != out->home[dev];
        if (copying) { out->hk = to.wkind; out->hk_wstream = st; out->hk_by_d2h = false; out->hk_renamed = to.renamed_k2; }
        int& mask = level_mask[{dev, out->h->d[dev].wdepth}];
        const int before = mask;
        mask |= op == TL_CB ? 8 : is_tl(op) ? 4 : out->m.level == 1 ? 2 : 1;
        if (mask == 15 && before != 15) count("level_with_kinds_0_1_2_and_circuit_bootstrap");
    }
    void issue(int dev, void* st, const int* ops, bool copying, C* const* outs, size_t n, C* a, C* b, C* c3, bool grouped)
    {
        const int op = ops[0];
        if (trace) {
            printf("T %s dev %d st %p op %d %s out", grouped ? "group" : "gate", dev, st, op, copying ? "copying" : "g");
            for (size_t j = 0; j < n; j++) printf(" %d", idx(outs[j]));
            printf(" in %d %d %d\n", idx(a), b ? idx(b) : -1, c3 ? idx(c3) : -1);
        }
        C* ins[3] = {a, b, c3};
        cufhe_amd_ctxt* hs[3] = {a->h, b ? b->h : nullptr, c3 ? c3->h : nullptr};
        if (grouped) {
            cufhe_amd_ctxt* ho[kUserOutputs];
            for (size_t j = 0; j < n; j++) ho[j] = outs[j]->h;
            if (int rc = S->dev(dev).record_gate_group(st, ops, copying, ho, n, hs)) { fprintf(stderr, "record_gate_group rc %d: %s\n", rc, S->dev(dev).error_text().c_str()); abort(); }
        } else if (int rc = S->dev(dev).record_gate(st, op, copying, outs[0]->h, hs, is_tl(op) ? 2 : -1)) { fprintf(stderr, "record_gate rc %d: %s\n", rc, S->dev(dev).error_text().c_str()); abort(); }
        for (C* i : ins)
            if (i) touch(i, dev, st);
        for (size_t j = 0; j < n; j++) { touch(outs[j], dev, st); note_hazards(dev, st, ops[j], copying, outs[j], ins); }
        // model, in issue order
        if (copying)
            for (C* i : ins)
                if (i) { i->m.dev[dev] = i->m.host; i->m.dev_defined[dev] = true; i->last_dev_upload_stream[dev] = st; }
        std::vector<std::vector<uint32_t>> r(n);
        for (size_t j = 0; j < n; j++) {      // (every output from the operands as they stand: an in-place gate reads before it writes)
            r[j].resize(kWords[outs[j]->m.level]);
            toy_gate(ops[j], outs[j]->m.level, r[j].data(), a->m.dev[dev].data(), b ? b->m.dev[dev].data() : nullptr, c3 ? c3->m.dev[dev].data() : nullptr);
        }
        for (size_t j = 0; j < n; j++) {
            C* out = outs[j];
            out->m.dev[dev] = r[j];
            out->m.dev_defined[dev] = true;
            out->last_dev_writer_stream[dev] = st;
            out->last_dev_upload_stream[dev] = nullptr;
            if (copying) { out->m.host = r[j]; out->last_host_writer_stream = st; }
        }
    }
    // TRGSW2NTT on a holder (cufhe_amd_trgsw_to_ntt, sched_hip.inc.h): the scheduler is told, the holder's host words are rewritten at once, and
    // the upload of the new words is recorded like a CtxtCopyH2D.
    void trgsw_to_ntt(int dev, void* st, C* h)
    {
        if (trace) printf("T trgsw_to_ntt dev %d st %p holder %d\n", dev, st, idx(h));
        if (h->copying_cmux_named) count("holder_host_rewritten_under_copying_cmux");
        if (int rc = S->before_direct_host_write(h->h)) { fprintf(stderr, "before_direct_host_write rc %d\n", rc); abort(); }
        check_host(h, "before TRGSW2NTT");               // a result that was on its way (a copying circuit bootstrap) has landed
        for (auto& w : h->host) w = (uint32_t)rng();
        h->m.host = h->host;
        h->hk = WK_NONE;
        h->copying_cmux_named = false;
        copy(dev, st, h, true);
    }
    void copy(int dev, void* st, C* c, bool to_device)
    {
        if (trace) printf("T copy dev %d st %p %s ctxt %d\n", dev, st, to_device ? "H2D" : "D2H", idx(c));
        if (int rc = S->dev(dev).record_copy(st, c->h, to_device)) { fprintf(stderr, "record_copy rc %d\n", rc); abort(); }
        touch(c, dev, st);
        C::Track& t = c->tr[dev];
        if (to_device) {
            if (t.on_record) count(c->m.level == 0 ? "waw_level0" : c->m.level == 1 ? "waw_level1" : c->m.level == 2 ? "waw_level2" : "waw_level3");
            if (c->m.level == 2 && t.cmux_read) count("war_trlwe_after_cmux");
            if (c->m.level == 3 && t.cmux_read) count("war_holder_upload_after_cmux");
            t.wkind = WK_UPLOAD; t.on_record = true; t.read = t.cmux_read = t.in_place_rot = false; t.wstream = st;
        } else {
            t.read = true;
            c->hk = t.on_record ? t.wkind : (int)WK_NONE; c->hk_wstream = t.wstream; c->hk_by_d2h = true; c->hk_renamed = t.renamed_k2;
        }
        if (to_device) { c->m.dev[dev] = c->m.host; c->m.dev_defined[dev] = true; c->last_dev_upload_stream[dev] = st; }
        else { c->m.host = c->m.dev[dev]; c->last_host_writer_stream = st; }
    }
    // StreamQuery(st) returned true, or StreamSynchronize(st) came back: what was delivered through st is in the host members
    void check_stream_results(void* st, const char* when)
    {
        for (C* c : ct) {
            if (!c->alive || c->last_host_writer_stream != st) continue;
            check_host(c, when);
            if ((c->hk == WK_SEIKS || c->hk == WK_SEIKS_AT) && c->hk_by_d2h && c->hk_renamed && c->hk_wstream != st) {
                count("renamed_kind2_output_fetched_and_polled_on_another_stream");
                c->hk = WK_NONE;
            }
        }
    }
    // Stream::st(): the raw handle is handed out (stream_fence), then the caller puts its own work on it.
    // A read of a ciphertext's OWN device buffer (the published tlwedevices pointer) must see what the gates issued on `st` before
    // the call left there; a write into it must be seen by the g-gates issued on `st` afterwards (src/cufhe_gates_gpu.cu:148-167: in
    // the reference all of this is one stream's order).
    void caller_read(int dev, void* st, C* c)
    {
        if (trace) printf("T caller_read dev %d st %p ctxt %d\n", dev, st, idx(c));
        if (int rc = S->dev(dev).stream_fence(st)) { fprintf(stderr, "stream_fence rc %d\n", rc); abort(); }
        auto r = std::make_shared<CallerRead>();
        r->want = c->m.dev[dev];
        const uint32_t* home = c->home[dev];
        const int words = kWords[c->m.level];
        be[dev]->push_caller(st, [r, home, words] { r->got.assign(home, home + words); r->done = true; });
        caller_reads.push_back(r);
    }
    void caller_write(int dev, void* st, C* c)
    {
        if (trace) printf("T caller_write dev %d st %p ctxt %d\n", dev, st, idx(c));
        if (int rc = S->dev(dev).stream_fence(st)) { fprintf(stderr, "stream_fence rc %d\n", rc); abort(); }
        std::vector<uint32_t> w(kWords[c->m.level]);
        for (auto& x : w) x = (uint32_t)rng();
        uint32_t* home = c->home[dev];
        be[dev]->push_caller(st, [w, home] { memcpy(home, w.data(), w.size() * 4); });
        c->m.dev[dev] = w;
        c->m.dev_defined[dev] = true;
        c->last_dev_writer_stream[dev] = st;
        c->last_dev_upload_stream[dev] = nullptr;
        c->tr[dev].wkind = WK_CALLER;
        touch(c, dev, st);
    }
    void check_caller_reads()
    {
        for (auto& r : caller_reads) {
            if (!r->done) { failures++; printf("FAIL a read on the caller's stream never ran\n"); continue; }
            if (r->got != r->want) { failures++; printf("FAIL a read on the caller's stream (raw handle of Stream::st()) saw stale words\n"); }
        }
        caller_reads.clear();
    }
    void check_host(C* c, const char* when)
    {
        if (c->host != c->m.host) {
            failures++;
            printf("FAIL host mismatch (%s) ctxt %p [%d] level %d\n", when, (void*)c, idx(c), c->m.level);
        }
    }
    // StreamQuery(st) returned true: what gates on st wrote must be in the ciphertexts' OWN device buffers (the pointers
    // published at creation), renaming or not -- and so must a value that an upload on st refreshed after a gate on ANOTHER stream
    // had renamed the ciphertext away from its buffer (the upload lands in the renamed buffer).
    void check_home_after_query(int dev, void* st)
    {
        for (auto* b : be) b->drain();
        for (C* c : ct) {
            if (!c->alive || !c->m.dev_defined[dev]) continue;
            if (c->last_dev_upload_stream[dev] ? c->last_dev_upload_stream[dev] != st : c->last_dev_writer_stream[dev] != st) continue;
            if (c->h->d[dev].dev != c->home[dev]) { failures++; printf("FAIL ctxt %p [%d] still renamed after StreamQuery (dev %d stream %p)\n", (void*)c, idx(c), dev, st); }
        }
    }
    void sync_and_check(bool check_dev)
    {
        if (trace) printf("T synchronize\n");
        if (int rc = S->synchronize_all()) { fprintf(stderr, "synchronize rc %d\n", rc); abort(); }
        for (auto* b : be) b->drain();
        check_caller_reads();
        level_mask.clear();
        for (C* c : ct) {
            c->hk = WK_NONE;
            c->copying_cmux_named = false;
            for (C::Track& t : c->tr) t = C::Track();        // nothing is on record any more
            if (!c->alive) continue;
            check_host(c, "after Synchronize");
            if (check_dev)
                for (int d = 0; d < G; d++)
                    if (c->m.dev_defined[d] && (c->h->d[d].dev != c->home[d] || memcmp(c->home[d], c->m.dev[d].data(), kWords[c->m.level] * 4))) {
                        failures++;
                        printf("FAIL device mismatch ctxt %p [%d] dev %d%s\n", (void*)c, idx(c), d, c->h->d[d].dev != c->home[d] ? " (value not in the ciphertext's own buffer)" : "");
                    }
        }
    }
};

static std::map<std::string, uint64_t> g_hazards;      // hazard classes over the random programs of the run

static int random_program(uint64_t seed, int gpus, bool threaded)
{
    std::mt19937_64 prng(seed);
    Test t(gpus, threaded, seed, 1 + (int)(prng() % 4));
    t.haz = &g_hazards;
    const int stub_failures_before = g_stub_failures.load();
    for (int d = 0; d < gpus; d++) {
        t.S->dev(d).set_round_gates(8 + prng() % 32);        // (the idle rule: one round)
        t.S->dev(d).set_level_flush_gates(4 + prng() % 40);  // exercise partial flushes
        t.S->dev(d).total_flush_gates = 30 + prng() % 200;
    }
    const int kStreams = 6;
    const bool use_raw_handles = seed % 3 == 0;     // (a handle that is out switches the shared-upload shortcut off: not in every program)
    auto stream_handle = [&](int dev, int s) { return (void*)(uintptr_t)(0x1000 + dev * 64 + s); };
    for (int i = 0; i < 30; i++) t.make(i % 5 == 4 ? 2 : i % 3 == 0 ? 1 : 0);
    for (int i = 0; i < 4; i++) t.make(3);        // TRGSW holders
    if (use_raw_handles)
        for (int i = 0; i < 12; i++) {
            Test::C* c = t.make(i % 3 == 0 ? 1 : 0);
            c->priv_dev = (int)(prng() % gpus);
            c->priv_stream = stream_handle(c->priv_dev, (int)(prng() % 2));     // two streams per device carry the private ciphertexts
        }
    const int steps = (300 + (int)(prng() % 500)) * 3 / 2;      // (a third of the steps go to the kinds beyond the built-in gates)
    int cur_dev = 0;
    void* cur_st = nullptr;
    auto usable = [&](Test::C* c) { return c->alive && (!c->priv_stream || (c->priv_stream == cur_st && c->priv_dev == cur_dev)); };
    auto pick = [&](int level) {
        for (;;) {
            Test::C* c = t.ct[prng() % t.ct.size()];
            if (usable(c) && c->m.level == level) return c;
        }
    };
    auto pick_defined = [&](int level, int dev) -> Test::C* {
        for (int tries = 0; tries < 64; tries++) {
            Test::C* c = t.ct[prng() % t.ct.size()];
            if (usable(c) && c->m.level == level && c->m.dev_defined[dev]) return c;
        }
        return nullptr;
    };
    // ciphertexts no private stream owns: what records on several streams may name
    auto pick_pub = [&](int level, int dev, bool defined) -> Test::C* {
        for (int tries = 0; tries < 64; tries++) {
            Test::C* c = t.ct[prng() % t.ct.size()];
            if (c->alive && !c->priv_stream && c->m.level == level && (!defined || c->m.dev_defined[dev])) return c;
        }
        return nullptr;
    };
    auto ok = [&](Test::C* c, int level, int dev, bool defined) { return c && c->alive && !c->priv_stream && c->m.level == level && (!defined || c->m.dev_defined[dev]); };
    // the newest outputs per kind of record: operands are drawn from them now and then, so that values cross kinds while still on record
    Test::C *last_gate_out = nullptr, *last_seiks_at_out = nullptr, *last_cmux_out = nullptr, *last_cb_out = nullptr, *rot_target = nullptr, *rot_sel = nullptr;
    // the outputs of one multi-output evaluation recorded ONE BY ONE (CUFHE_AMD_USER_OP_OUTPUT(op, j) through record_gate), in shuffled order, with
    // whatever the program does between them
    struct Siblings {
        bool active = false; int dev = 0; void* st = nullptr; int k = 0; bool copying = false; Test::C *a = nullptr, *b = nullptr, *c3 = nullptr;
        std::vector<Test::C*> outs; std::vector<int> order; size_t next = 0; bool wrote_operand = false, flushed = false, other = false;
    } sib;
    auto sib_alive = [&]() {
        bool all = sib.a->alive && (!sib.b || sib.b->alive) && (!sib.c3 || sib.c3->alive);
        for (Test::C* o : sib.outs) all = all && o->alive;
        return all;
    };
    auto sib_record_next = [&](void* st) {
        if (sib.next > 0) {
            if (sib.wrote_operand) t.count("siblings_separated_by_operand_write");
            else if (sib.flushed) t.count("siblings_separated_by_flush");
            else if (!sib.other) t.count("siblings_adjacent");
            else t.count("siblings_separated_by_other_records");
            if (st != sib.st) t.count("siblings_on_different_streams");
        }
        const int j = sib.order[sib.next++];
        t.gate(sib.dev, st, user_op(sib.k, j), sib.copying, sib.outs[j], sib.a, sib.b, sib.c3);
        sib.wrote_operand = sib.flushed = sib.other = false;
        if (sib.next == sib.order.size()) sib.active = false;
    };
    for (int step = 0; step < steps; step++) {
        int dev = (int)(prng() % gpus);
        void* st = stream_handle(dev, (int)(prng() % kStreams));
        cur_dev = dev;
        cur_st = st;
        const int level = prng() % 4 == 0 ? 1 : 0;
        if (sib.active && !sib_alive()) sib.active = false;
        if (sib.active) {
            const unsigned u = (unsigned)(prng() % 8);
            if (u < 4) { sib_record_next(prng() % 5 == 0 ? st = stream_handle(sib.dev, (int)(prng() % kStreams)) : sib.st); continue; }
            if (u == 4) {                          // a write to an operand between two siblings: the later ones see the new value
                Test::C *x = pick_pub(sib.a->m.level, sib.dev, !sib.copying), *y = pick_pub(sib.a->m.level, sib.dev, !sib.copying);
                if (x && y) { t.gate(sib.dev, sib.st, (int)(prng() % 10), sib.copying, sib.a, x, y, nullptr); sib.wrote_operand = true; }
                continue;
            }
            if (u == 5) { t.S->dev(sib.dev).flush(); sib.flushed = true; continue; }
            sib.other = true;
        }
        if (prng() % 100 < 34) {                    // ---- the kinds of record beyond the built-in gates ----
            const unsigned q = (unsigned)(prng() % 100);
            const bool copying = prng() % 2 == 0;
            if (q < 12) {                           // user gate of arity 1, 2 or 3 at level 0 or 1
                const int k = (int)(prng() % 12), ar = user_arity(k);
                Test::C* a = level == 0 && prng() % 3 == 0 && ok(last_seiks_at_out, 0, dev, !copying) && usable(last_seiks_at_out) ? last_seiks_at_out : copying ? pick(level) : pick_defined(level, dev);
                Test::C* b = ar >= 2 ? (copying ? pick(level) : pick_defined(level, dev)) : nullptr;
                Test::C* c3 = ar == 3 ? (copying ? pick(level) : pick_defined(level, dev)) : nullptr;
                if (!a || (ar >= 2 && !b) || (ar == 3 && !c3)) continue;
                Test::C* out = prng() % 5 == 0 ? a : pick(level);
                t.gate(dev, st, user_op(k, 0), copying, out, a, b, c3);
                last_gate_out = out;
            } else if (q < 18) {                    // a built-in gate on the newest SEIKS_AT result
                if (!ok(last_seiks_at_out, 0, dev, !copying) || !usable(last_seiks_at_out)) continue;
                Test::C* b = copying ? pick(0) : pick_defined(0, dev);
                if (!b) continue;
                Test::C* out = pick(0);
                t.gate(dev, st, (int)(prng() % 10), copying, out, last_seiks_at_out, b, nullptr);
                last_gate_out = out;
            } else if (q < 34) {                    // multi-output evaluation of 2, 4 or 8 outputs: together, or one by one
                const int k = 12 + (int)(prng() % 12), ar = user_arity(k), nout = user_nout(k);
                const bool together = prng() % 2 == 0;
                if (!together && sib.active) continue;
                Test::C* a = pick_pub(level, dev, !copying);
                Test::C* b = ar >= 2 ? pick_pub(level, dev, !copying) : nullptr;
                Test::C* c3 = ar == 3 ? pick_pub(level, dev, !copying) : nullptr;
                if (!a || (ar >= 2 && !b) || (ar == 3 && !c3)) continue;
                std::vector<Test::C*> outs;
                for (int tries = 0; tries < 200 && (int)outs.size() < nout; tries++) {
                    Test::C* o = pick_pub(level, dev, false);
                    if (prng() % 2 && o && !o->tr[dev].read) continue;       // (outputs whose present value has recorded readers, more often than not)
                    bool fresh = o && o != a && o != b && o != c3;
                    for (Test::C* x : outs) fresh = fresh && x != o;
                    if (fresh) outs.push_back(o);
                }
                if ((int)outs.size() < nout) continue;
                if (together) { t.gate_group(dev, st, k, copying, outs, a, b, c3); continue; }
                sib = Siblings();
                sib.active = true; sib.dev = dev; sib.st = st; sib.k = k; sib.copying = copying; sib.a = a; sib.b = b; sib.c3 = c3; sib.outs = outs;
                for (int j = 0; j < nout; j++) sib.order.push_back(j);
                std::shuffle(sib.order.begin(), sib.order.end(), prng);
                sib_record_next(st);
            } else if (q < 40) {                    // TL_BOOTSTRAP of what a gate just produced
                Test::C* in = ok(last_gate_out, 0, dev, !copying) && usable(last_gate_out) ? last_gate_out : copying ? pick(0) : pick_defined(0, dev);
                if (!in) continue;
                t.gate(dev, st, TL_BOOT, copying, pick(2), in, nullptr, nullptr);
            } else if (q < 50) {                    // SEIKS_AT(j): TRLWE -> lvl0, now and then fetched and polled on another stream
                Test::C* in = prng() % 2 && ok(last_cmux_out, 2, dev, !copying) ? last_cmux_out : copying ? pick(2) : pick_defined(2, dev);
                if (!in) continue;
                Test::C* out = pick(0);
                for (int tries = 0; tries < 8 && !out->tr[dev].read; tries++) out = pick(0);       // (an output whose value has recorded readers is renamed)
                t.gate(dev, st, TL_SEIKS_AT0 + (int)(prng() % kSeiksIdx), copying, out, in, nullptr, nullptr);
                last_seiks_at_out = out;
                if (!out->priv_stream && prng() % 2 == 0) {     // fetched on another stream and polled there until it has arrived
                    void* st2 = stream_handle(dev, (int)(prng() % kStreams));
                    if (st2 == st) continue;
                    t.copy(dev, st2, out, false);
                    int done = 0;
                    for (long polls = 0; polls < 100000000 && done == 0; polls++) done = t.S->dev(dev).stream_query(st2);
                    if (done != 1) { t.failures++; printf("FAIL a fetched SEIKS_AT result never arrived (stream_query %d)\n", done); continue; }
                    t.check_stream_results(st2, "after StreamQuery");
                    t.check_home_after_query(dev, st2);
                }
            } else if (q < 64) {                    // CMUX: res = c0 + cs [x] (c1 - c0), now and then in place on c1 or on c0
                Test::C* cs = prng() % 2 && ok(last_cb_out, 3, dev, !copying) ? last_cb_out : copying ? pick(3) : pick_defined(3, dev);
                Test::C *c1 = copying ? pick(2) : pick_defined(2, dev), *c0 = copying ? pick(2) : pick_defined(2, dev);
                if (!cs || !c1 || !c0) continue;
                const unsigned w = (unsigned)(prng() % 5);
                Test::C* res = w == 0 ? c1 : w == 1 ? c0 : pick(2);
                t.gate(dev, st, TL_CMUX, copying, res, c1, c0, cs);
                last_cmux_out = res;
            } else if (q < 80) {                    // CMUX_ROTATE(e): mostly in place, mostly going on with the buffer of the step before
                const bool go_on = prng() % 3 != 0 && ok(rot_target, 2, dev, true) && ok(rot_sel, 3, dev, true);
                Test::C* c = go_on ? rot_target : copying ? pick(2) : pick_defined(2, dev);
                Test::C* cs = go_on ? rot_sel : prng() % 2 && ok(last_cb_out, 3, dev, !copying) ? last_cb_out : copying ? pick(3) : pick_defined(3, dev);
                if (!c || !cs) continue;
                Test::C* res = go_on || prng() % 3 != 0 ? c : pick(2);
                t.gate(dev, st, TL_CMUX_ROT0 + (int)(prng() % kRotExps), go_on ? false : copying, res, c, nullptr, cs);
                rot_target = res;
                rot_sel = cs;
            } else if (q < 90) {                    // circuit bootstrap: lvl0 -> holder, of what a gate produced
                Test::C* in = prng() % 2 && ok(last_gate_out, 0, dev, !copying) && usable(last_gate_out) ? last_gate_out : copying ? pick(0) : pick_defined(0, dev);
                if (!in) continue;
                Test::C* out = pick(3);
                t.gate(dev, st, TL_CB, copying, out, in, nullptr, nullptr);
                last_cb_out = out;
            } else {                                // TRGSW2NTT: the holder's host words rewritten at once, their upload recorded
                t.trgsw_to_ntt(dev, st, pick(3));
            }
            continue;
        }
        const unsigned r = (unsigned)(prng() % 100);
        if (use_raw_handles && prng() % 16 == 0) {  // the caller takes the raw handle of the stream and reads / writes a device buffer on it
            Test::C* c = nullptr;
            for (int tries = 0; tries < 64 && !c; tries++) {
                Test::C* x = t.ct[prng() % t.ct.size()];
                if (x->alive && x->priv_stream == st && x->priv_dev == dev && x->m.dev_defined[dev]) c = x;
            }
            if (!c) continue;
            if (prng() % 4 == 0) {
                // a result on its way to tlwehost, the device buffer rewritten through the raw handle, then a copying gate that reads the
                // ciphertext: the reference's upload brings the RESULT back (resolve_host), whatever the buffer holds now
                const int lv = c->m.level;
                t.gate(dev, st, (int)(prng() % 10), true, c, pick(lv), pick(lv), nullptr);
                t.caller_write(dev, st, c);
                t.gate(dev, st, (int)(prng() % 10), true, pick(lv), c, pick(lv), nullptr);
                continue;
            }
            if (prng() % 2) t.caller_read(dev, st, c);
            else t.caller_write(dev, st, c);
            continue;
        }
        if (r < 8) {                                // TRLWE-level operation (copying or device-resident)
            const int op = TL_BOOT + (int)(prng() % 3);
            const bool copying = prng() % 2 == 0;
            Test::C* in = copying ? pick(tl_in_level(op)) : pick_defined(tl_in_level(op), dev);
            if (!in) continue;
            Test::C* out = (tl_in_level(op) == tl_out_level(op) && prng() % 4 == 0) ? in : pick(tl_out_level(op));
            t.gate(dev, st, op, copying, out, in, nullptr, nullptr);
        } else if (r < 40) {                        // copying gate
            const int kind = (int)(prng() % 10);
            Test::C* out = pick(level);
            Test::C* a = prng() % 5 == 0 ? out : pick(level);      // in-place now and then
            if (kind == 0) t.gate(dev, st, prng() % 2 ? OP_NOT : OP_COPY, true, out, a, nullptr, nullptr);
            else if (kind <= 2) t.gate(dev, st, prng() % 2 ? OP_MUX : OP_NMUX, true, out, a, pick(level), pick(level));
            else t.gate(dev, st, (int)(prng() % 10), true, out, a, prng() % 7 == 0 ? a : pick(level), nullptr);
        } else if (r < 65) {                        // g-gate on device-resident values
            Test::C *a = pick_defined(level, dev), *b = pick_defined(level, dev), *c3 = pick_defined(level, dev);
            if (!a || !b || !c3) continue;
            Test::C* out = prng() % 4 == 0 ? a : pick(level);
            const int kind = (int)(prng() % 10);
            if (kind == 0) t.gate(dev, st, OP_NOT, false, out, a, nullptr, nullptr);
            else if (kind <= 2) t.gate(dev, st, OP_MUX, false, out, a, b, c3);
            else t.gate(dev, st, (int)(prng() % 10), false, out, a, b, nullptr);
        } else if (r < 72) {
            t.copy(dev, st, pick(prng() % 4 == 0 ? 2 + (int)(prng() % 2) : level), true);
        } else if (r < 80) {
            Test::C* c = pick_defined(prng() % 4 == 0 ? 2 + (int)(prng() % 2) : level, dev);
            if (c) t.copy(dev, st, c, false);
        } else if (r < 92) {                        // StreamQuery poll
            const int q = t.S->dev(dev).stream_query(st);
            if (q < 0) { fprintf(stderr, "stream_query rc %d\n", q); abort(); }
            if (q == 1) {
                t.check_stream_results(st, "after StreamQuery");
                t.check_home_after_query(dev, st);
            }
        } else if (r < 95) {                        // Synchronize, then the host may edit ciphertexts
            t.sync_and_check(true);
            for (int k = 0; k < 3; k++) {
                Test::C* c = t.ct[prng() % t.ct.size()];
                if (!c->alive) continue;
                for (auto& w : c->host) w = (uint32_t)prng();
                c->m.host = c->host;
            }
        } else if (r < 96) {                        // the caller rewrites a tlwehost itself, without Synchronize (TRGSW2NTT on a holder)
            Test::C* c = t.ct[prng() % t.ct.size()];
            if (!c->alive) continue;
            if (int rc = t.S->before_direct_host_write(c->h)) { fprintf(stderr, "before_direct_host_write rc %d\n", rc); abort(); }
            for (auto* b : t.be) b->drain();
            t.check_host(c, "before a direct host write");      // a result that was on its way has landed
            for (auto& w : c->host) w = (uint32_t)prng();
            c->m.host = c->host;
        } else if (r < 97) {                        // StreamSynchronize(st): everything issued on st is complete and delivered
            if (int rc = t.S->dev(dev).stream_synchronize(st)) { fprintf(stderr, "stream_synchronize rc %d\n", rc); abort(); }
            t.check_stream_results(st, "after StreamSynchronize");
            t.check_home_after_query(dev, st);
        } else if (r < 98) {                        // a ciphertext goes out of scope while work on it is recorded
            Test::C* c = t.ct[prng() % t.ct.size()];
            if (!c->alive || c->priv_stream) continue;
            t.S->ctxt_destroy(c->h);
            c->alive = false;
            for (auto& w : c->host) w = 0xDEADBEEFu;      // the caller's memory is gone: nobody may read it any more
            t.make(c->m.level);
        } else {
            t.S->dev(dev).flush();
        }
    }
    t.sync_and_check(true);
    return t.failures + (g_stub_failures.load() - stub_failures_before);
}

// ---- random single-kind netlists: what the per-gate (two-lane) order of a flush is made for ----
// One device, level-0 ciphertexts only, inputs uploaded by the first gates that read them, then a few hundred gates whose operands are
// drawn from everything computed so far: deep chains beside wide independent work, temporaries re-used (renamed), in-place gates,
// copying and device-resident gates mixed, Mux gates (two rotations), explicit D2H copies, several streams; Synchronize once at the end
// (or in the middle, so that a second flush depends on the first).  Every value is compared with the in-order interpreter.
static uint64_t g_two_lane_groups = 0, g_two_lane_launches = 0;
static int dag_program(uint64_t seed, bool threaded)
{
    std::mt19937_64 prng(seed);
    Test t(1, threaded, seed, 2 + (int)(prng() % 3));
    t.S->dev(0).set_round_gates(100000);            // nothing is launched before the Synchronize: the whole netlist is one flush
    t.S->dev(0).total_flush_gates = 1u << 30;
    const int inputs = 6 + (int)(prng() % 10), temps = 4 + (int)(prng() % 12), gates = 60 + (int)(prng() % 400);
    std::vector<Test::C*> pool;
    for (int i = 0; i < inputs + temps; i++) pool.push_back(t.make(0));
    std::vector<bool> defined(pool.size(), false);
    auto st = [&](int i) { return (void*)(uintptr_t)(0x500 + i % 5); };
    // the inputs reach the device with the first copying gates
    for (int i = 0; i < inputs; i += 2) {
        Test::C* out = pool[inputs + (i / 2) % temps];
        t.gate(0, st(i), (int)(prng() % 10), true, out, pool[i], pool[(i + 1) % inputs], nullptr);
        defined[i] = defined[(i + 1) % inputs] = true;
        defined[inputs + (i / 2) % temps] = true;
    }
    const int mid_sync = prng() % 3 == 0 ? (int)(prng() % gates) : -1;
    for (int k = 0; k < gates; k++) {
        auto pick_def = [&]() {
            for (;;) {
                const size_t i = prng() % pool.size();
                if (defined[i]) return i;
            }
        };
        const size_t a = pick_def(), b = pick_def(), c = pick_def();
        const bool chain = prng() % 3 != 0;              // most gates extend what was just computed: long chains
        static size_t last = 0;
        const size_t in0 = chain && defined[last] ? last : a;
        size_t o = inputs + prng() % temps;
        if (prng() % 6 == 0) o = in0;                    // in place
        const unsigned r = (unsigned)(prng() % 20);
        if (r == 0) t.gate(0, st(k), OP_NOT, false, pool[o], pool[in0], nullptr, nullptr);
        else if (r <= 2) t.gate(0, st(k), prng() % 2 ? OP_MUX : OP_NMUX, false, pool[o], pool[in0], pool[b], pool[c]);
        else if (r == 3) t.copy(0, st(k), pool[in0], false);
        else if (r == 4 && pool[in0]->m.dev[0] == pool[in0]->m.host) t.gate(0, st(k), (int)(prng() % 10), true, pool[o], pool[in0], pool[b], nullptr);   // a copying gate whose re-upload is the device value
        else t.gate(0, st(k), (int)(prng() % 10), false, pool[o], pool[in0], pool[b], nullptr);
        if (r != 3) { defined[o] = true; last = o; }
        if (k == mid_sync) t.sync_and_check(true);
    }
    for (size_t i = 0; i < pool.size(); i++)
        if (defined[i] && prng() % 2) t.copy(0, st((int)i), pool[i], false);      // fetch some of the results
    t.sync_and_check(true);
    g_two_lane_groups += t.S->dev(0).stats().two_lane_groups.load();
    g_two_lane_launches += t.S->dev(0).stats().two_lane_launches.load();
    return t.failures;
}

// ---- shaped programs with launch-count expectations ----
struct Shape { const char* name; uint64_t launch_sequences, levels, gates, groups, uploads, uploads_shared; int failures; uint64_t two_lane_groups = 0, two_lane_launches = 0; };

static Shape chained(bool threaded)
{
    // test/test_api_gpu.cu:140-159 as tests/cpp/test_gate_api.cpp Chained(): 64 chains x 5 in-place gates on 8 streams
    Test t(1, threaded, 7, 4);
    const int K = 64;
    std::vector<Test::C*> a, b, c;
    for (int i = 0; i < K; i++) { a.push_back(t.make(0)); b.push_back(t.make(0)); c.push_back(t.make(0)); }
    for (int i = 0; i < K; i++) {
        void* st = (void*)(uintptr_t)(0x100 + i % 8);
        t.gate(0, st, 0, true, a[i], a[i], b[i], nullptr);
        t.gate(0, st, 4, true, a[i], a[i], b[i], nullptr);
        t.gate(0, st, 5, true, a[i], a[i], c[i], nullptr);
        t.gate(0, st, OP_NOT, true, a[i], a[i], nullptr, nullptr);
        t.gate(0, st, OP_MUX, true, a[i], a[i], b[i], c[i]);
    }
    t.sync_and_check(true);
    const Stats& s = t.S->dev(0).stats();
    return {"chained", s.launch_sequences, s.levels, s.gates, s.groups, s.uploads, s.uploads_shared, t.failures};
}

static Shape ripple(bool threaded)
{
    // tests/cpp/test_gate_api.cpp RippleAdders(): 16 x 8-bit ripple-carry adders, one stream each, issued bit by bit
    Test t(1, threaded, 8, 4);
    const int A = 16, B = 8;
    std::vector<Test::C*> x, y, sum, carry, t1, t2;
    for (int i = 0; i < A * B; i++) { x.push_back(t.make(0)); y.push_back(t.make(0)); sum.push_back(t.make(0)); }
    for (int i = 0; i < A; i++) { carry.push_back(t.make(0)); t1.push_back(t.make(0)); t2.push_back(t.make(0)); }
    for (int k = 0; k < B; k++)
        for (int i = 0; i < A; i++) {
            void* st = (void*)(uintptr_t)(0x200 + i);
            Test::C *X = x[i * B + k], *Y = y[i * B + k], *Sm = sum[i * B + k], *Cy = carry[i];
            t.gate(0, st, 5, true, t1[i], X, Y, nullptr);
            t.gate(0, st, 5, true, Sm, t1[i], Cy, nullptr);
            t.gate(0, st, 3, true, t2[i], t1[i], Cy, nullptr);
            t.gate(0, st, 3, true, t1[i], X, Y, nullptr);
            t.gate(0, st, 4, true, Cy, t1[i], t2[i], nullptr);
        }
    t.sync_and_check(true);
    const Stats& s = t.S->dev(0).stats();
    return {"ripple_adders", s.launch_sequences, s.levels, s.gates, s.groups, s.uploads, s.uploads_shared, t.failures, s.two_lane_groups.load(), s.two_lane_launches.load()};
}

static Shape intensive(bool threaded)
{
    // test/test_intensive.cc:21-128: poll StreamQuery and refill, three inputs shared by every stream
    Test t(1, threaded, 9, 4);
    const int kStreams = 200, kRounds = 4;
    Test::C *in0 = t.make(0), *in1 = t.make(0), *inc = t.make(0);
    std::vector<Test::C*> out;
    std::vector<int> round(kStreams, 0);
    for (int i = 0; i < kStreams; i++) out.push_back(t.make(0));
    auto st = [](int i) { return (void*)(uintptr_t)(0x300 + i); };
    for (int i = 0; i < kStreams; i++) t.gate(0, st(i), 0, true, out[i], in0, in1, nullptr);
    int done = 0;
    long polls = 0;
    while (done < kStreams && polls < 100000000) {
        for (int i = 0; i < kStreams; i++) {
            polls++;
            if (round[i] >= kRounds) continue;
            if (t.S->dev(0).stream_query(st(i)) != 1) continue;
            t.check_host(out[i], "intensive");
            if (++round[i] == kRounds) { done++; continue; }
            if (round[i] % 2) t.gate(0, st(i), OP_MUX, true, out[i], inc, in1, in0);
            else t.gate(0, st(i), 0, true, out[i], in0, in1, nullptr);
        }
    }
    if (done < kStreams) { t.failures++; printf("FAIL intensive never completed\n"); }
    t.sync_and_check(true);
    const Stats& s = t.S->dev(0).stats();
    return {"intensive", s.launch_sequences, s.levels, s.gates, s.groups, s.uploads, s.uploads_shared, t.failures};
}

static Shape multi_gpu(bool threaded)
{
    // test/test_gate_gpu_multi.cc:36-93: default-constructed streams round-robin the devices
    // (include/cufhe_gpu.cuh:154-159); every gate must land on its stream's device only
    const int G = 3, K = 96;
    Test t(G, threaded, 10, 2);
    std::vector<Test::C*> a, b, o;
    for (int i = 0; i < K; i++) { a.push_back(t.make(0)); b.push_back(t.make(0)); o.push_back(t.make(0)); }
    for (int i = 0; i < K; i++) t.gate(i % G, (void*)(uintptr_t)(0x400 + i), 0, true, o[i], a[i], b[i], nullptr);
    // a second round consuming results produced on ANOTHER device: the host copy has to land first
    for (int i = 0; i < K; i++) t.gate((i + 1) % G, (void*)(uintptr_t)(0x400 + i), 5, true, a[i], o[i], b[i], nullptr);
    t.sync_and_check(true);
    Shape sh{"multi_gpu", 0, 0, 0, 0, 0, 0, t.failures};
    for (int d = 0; d < G; d++) {
        const Stats& s = t.S->dev(d).stats();
        if (s.gates != 2 * K / G) { sh.failures++; printf("FAIL device %d recorded %llu gates, expected %d\n", d, (unsigned long long)s.gates, 2 * K / G); }
        sh.launch_sequences += s.launch_sequences; sh.levels += s.levels; sh.gates += s.gates; sh.groups += s.groups;
        sh.uploads += s.uploads; sh.uploads_shared += s.uploads_shared;
    }
    return sh;
}

// A copying multi-output evaluation while a raw stream handle is out (found by the random programs): with a handle out every copying
// gate uploads its operands anew (resolve_host), and the outputs of ONE evaluation recorded through record_gate_group used to do so one by
// one -- each upload behind the sibling before it, eight outputs on eight levels (eight rotations on the device).  One upload, one level.
static Shape group_with_raw_handle_out(bool threaded)
{
    Test t(1, threaded, 11, 2);
    void* st = (void*)(uintptr_t)0x600;
    Test::C *a = t.make(0), *b = t.make(0), *c = t.make(0), *x = t.make(0);
    std::vector<Test::C*> outs;
    for (int j = 0; j < 8; j++) outs.push_back(t.make(0));
    t.gate(0, st, 3, true, x, a, b, nullptr);
    t.caller_read(0, st, x);                          // Stream::st(): the handle is out from here on
    t.gate_group(0, st, 22, true, outs, a, b, c);     // definition 22: three operands, eight outputs
    t.gate(0, st, 5, true, x, outs[7], outs[0], nullptr);
    t.sync_and_check(true);
    const Stats& s = t.S->dev(0).stats();
    if (s.levels != 3) { t.failures++; printf("FAIL group_with_raw_handle_out ran as %llu levels, expected 3\n", (unsigned long long)s.levels); }
    return {"group_with_raw_handle_out", s.launch_sequences, s.levels, s.gates, s.groups, s.uploads, s.uploads_shared, t.failures};
}

// A delivery to tlwehost ahead of a recorded upload out of the same tlwehost (found by the random programs, with renaming): a copying gate
// reads c -- its upload sits late, behind the device-resident gates that wrote c's buffer -- then a copying gate on fresh operands
// overwrites c.  Renamed, that gate waits for nothing and sits in the front level, which is launched by itself once it holds two gates; a
// StreamQuery of its stream delivers its result to c's tlwehost; the upload, launched afterwards, then read the NEW words.  (It takes a
// launch worker that is slower than the issuing thread: the stub holds it at the start of the second launch until the poll is over.)
static Shape delivery_ahead_of_upload(bool threaded)
{
    Test t(1, threaded, 12, 2);
    t.S->dev(0).set_round_gates(100000);
    t.S->dev(0).set_level_flush_gates(2);            // a front level of two gates is launched at once when the level behind it holds one
    void *sa = (void*)(uintptr_t)0x700, *sb = (void*)(uintptr_t)0x701;
    Test::C *c = t.make(0), *x = t.make(0), *y = t.make(0), *z = t.make(0), *r = t.make(0);
    t.copy(0, sa, c, true);
    t.copy(0, sa, x, true);
    for (int k = 0; k < 3; k++) t.gate(0, sa, 3 + k, false, c, c, x, nullptr);       // c's buffer is written three levels deep
    t.gate(0, sa, 5, true, r, c, y, nullptr);                                        // uploads c's tlwehost behind them
    t.gate(0, sb, 4, true, c, y, z, nullptr);                                        // overwrites c: delivered to the same tlwehost
    if (threaded) {
        for (long spins = 0; spins < 100000000 && t.be[0]->launches_so_far() == 0; spins++) std::this_thread::yield();      // the front level is on the device
        g_hold_launch = true;
    }
    int done = 0;
    for (long polls = 0; polls < 100000000 && done == 0; polls++) {
        if (polls == 20000) g_hold_launch = false;          // (a scheduler that keeps the delivery behind the upload needs the second launch)
        done = t.S->dev(0).stream_query(sb);
    }
    g_hold_launch = false;
    if (done != 1) { t.failures++; printf("FAIL delivery_ahead_of_upload: StreamQuery %d\n", done); }
    else t.check_stream_results(sb, "after StreamQuery");
    t.sync_and_check(true);
    const Stats& s = t.S->dev(0).stats();
    return {"delivery_ahead_of_upload", s.launch_sequences, s.levels, s.gates, s.groups, s.uploads, s.uploads_shared, t.failures};
}

// ---- host cost of the issuing thread at the real ciphertext size (no device work at all) ----
class NullBackend : public Backend {
   public:
    void bind_thread() override {}
    int num_streams() override { return 4; }
    int words(int level) override { return level ? 1025 : 631; }
    int alloc_device(size_t bytes, void** p) override { *p = malloc(bytes); return 0; }
    int free_device(void* p) override { free(p); return 0; }
    int alloc_pinned(size_t bytes, void** p) override { *p = malloc(bytes); return 0; }
    int free_pinned(void* p) override { free(p); return 0; }
    int h2d(int, void*, const void*, size_t) override { return 0; }
    int d2h(int, void*, const void*, size_t) override { return 0; }
    int copy_ctxts(int, const CopyRec*, size_t, uint32_t*, bool) override { return 0; }
    int run_gates(int, int, const GateRef*, size_t) override { return 0; }
    int event_create(void** ev) override { *ev = (void*)1; return 0; }
    int event_destroy(void*) override { return 0; }
    int event_record(int, void*) override { return 0; }
    int event_query(void*) override { return 1; }
    int event_sync(void*) override { return 0; }
    int stream_wait(int, void*) override { return 0; }
    std::string error_text() override { return ""; }
};

// The benchmark's dependent netlist (tools/bench_api.cpp: 256 x 16-bit ripple-carry adders, issued adder by adder) against a device
// that does nothing but carries the HIP backend's cost model (launch_plan.h: lane_model, blind_rotate_ms for 256 CUs): with
// CUFHE_AMD_SCHED_DEBUG=1 the scheduler prints what the level order and the two-lane plan are estimated to cost -- the plan can be
// tuned here, on the CPU.
class ModelBackend : public NullBackend {
   public:
    bool lane_model(LaneModel* m) override { return plan::lane_model(256, m); }
    double launch_ms(size_t n) override { return plan::blind_rotate_ms(n, 256); }
    int gate_weight(int op) override { return op == 10 || op == 11 ? 2 : op == 12 || op == 13 ? 0 : 1; }
    uint64_t lanes[3] = {0, 0, 0};
    int run_gates_lane(int, int, const GateRef*, size_t, int lane) override { lanes[lane == 0 ? 0 : 1]++; return 0; }
    int run_gates(int, int, const GateRef*, size_t) override { lanes[2]++; return 0; }
};

static void plan_netlist(int adders, int bits)
{
    ModelBackend* mb = nullptr;
    Scheduler S(1, true, [&](int) { mb = new ModelBackend(); return mb; });
    S.dev(0).set_round_gates(2048);
    std::vector<std::vector<uint32_t>> host;
    std::vector<cufhe_amd_ctxt*> c;
    std::string err;
    auto make = [&]() { host.emplace_back(631, 7u); c.push_back(nullptr); S.ctxt_create(0, host.back().data(), &c.back(), &err); return c.back(); };
    host.reserve((size_t)adders * (3 * bits + 3) + 8);
    std::vector<cufhe_amd_ctxt*> x, y, sum, carry, t1, t2;
    for (int i = 0; i < adders * bits; i++) { x.push_back(make()); y.push_back(make()); sum.push_back(make()); }
    for (int i = 0; i < adders; i++) { carry.push_back(make()); t1.push_back(make()); t2.push_back(make()); }
    auto gate = [&](void* st, int op, cufhe_amd_ctxt* o, cufhe_amd_ctxt* a, cufhe_amd_ctxt* b) {
        cufhe_amd_ctxt* ins[3] = {a, b, nullptr};
        S.dev(0).record_gate(st, op, true, o, ins);
    };
    for (int i = 0; i < adders; i++) {
        void* st = (void*)(uintptr_t)(0x1000 + i % 256);
        for (int k = 0; k < bits; k++) {
            cufhe_amd_ctxt *X = x[i * bits + k], *Y = y[i * bits + k], *Sm = sum[i * bits + k], *C = carry[i];
            gate(st, 5, t1[i], X, Y);
            gate(st, 5, Sm, t1[i], C);
            gate(st, 3, t2[i], t1[i], C);
            gate(st, 3, t1[i], X, Y);
            gate(st, 4, C, t1[i], t2[i]);
        }
    }
    S.synchronize_all();
    const Stats& st = S.dev(0).stats();
    printf("PLAN {\"adders\": %d, \"bits\": %d, \"gates\": %llu, \"levels\": %llu, \"two_lane_groups\": %llu, \"chain_steps\": %llu, \"bulk_chunks\": %llu, \"other_launches\": %llu}\n",
           adders, bits, (unsigned long long)st.gates, (unsigned long long)st.levels, (unsigned long long)st.two_lane_groups.load(),
           (unsigned long long)mb->lanes[0], (unsigned long long)mb->lanes[1], (unsigned long long)mb->lanes[2]);
    for (auto* k : c) S.ctxt_destroy(k);
}

static void host_cost(int gpus, int gates_per_gpu)
{
    // what tools/bench_api.cpp does, for `gpus` devices from one issuing thread: Nand(out, a, b, st) on
    // host-resident lvl0 ciphertexts over 256 streams per device, then Synchronize()
    Scheduler S(gpus, true, [](int) { return new NullBackend(); });
    const int total = gpus * gates_per_gpu, W = 631;
    std::vector<std::vector<uint32_t>> host(3 * (size_t)total, std::vector<uint32_t>(W, 7u));
    std::vector<cufhe_amd_ctxt*> c(3 * (size_t)total);
    std::string err;
    for (size_t i = 0; i < c.size(); i++) S.ctxt_create(0, host[i].data(), &c[i], &err);
    double best = 1e30, best_rec = 0;
    for (int rep = 0; rep < 5; rep++) {
        for (auto& h : host) h[0]++;          // fresh inputs every round
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < total; i++) {
            cufhe_amd_ctxt* ins[3] = {c[3 * (size_t)i + 1], c[3 * (size_t)i + 2], nullptr};
            S.dev(i % gpus).record_gate((void*)(uintptr_t)(0x1000 + (i / gpus) % 256), 0, true, c[3 * (size_t)i], ins);
        }
        auto t1 = std::chrono::steady_clock::now();
        S.synchronize_all();
        auto t2 = std::chrono::steady_clock::now();
        const double tot = std::chrono::duration<double, std::micro>(t2 - t0).count();
        if (tot < best) { best = tot; best_rec = std::chrono::duration<double, std::micro>(t1 - t0).count(); }
    }
    // busy time of the issuing thread (recording + delivering results) and of the busiest launch worker, from the
    // scheduler's own clocks over all five rounds: wall time above also contains waiting for the workers
    uint64_t rec = 0, ret = 0, worker = 0, gates = 0;
    for (int d = 0; d < gpus; d++) {
        const Stats& st = S.dev(d).stats();
        rec += st.record_ns; ret += st.retire_ns; gates += st.gates;
        worker = std::max<uint64_t>(worker, st.launch_ns.load());
    }
    printf("HOSTCOST {\"gpus\": %d, \"gates\": %d, \"wall_us_per_gate\": %.4f, \"enqueue_wall_us_per_gate\": %.4f, "
           "\"issuing_thread_us_per_gate\": %.4f, \"issuing_thread_gates_per_s\": %.0f, \"worker_us_per_gate_per_device\": %.4f}\n",
           gpus, total, best / total, best_rec / total, (rec + ret) * 1e-3 / gates, gates / ((rec + ret) * 1e-9),
           worker * 1e-3 / (gates / gpus));
    for (auto* x : c) S.ctxt_destroy(x);
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "plan")) {
        plan_netlist(argc > 2 ? atoi(argv[2]) : 256, argc > 3 ? atoi(argv[3]) : 16);
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "hostcost")) {
        host_cost(1, 4096);
        host_cost(8, 4096);
        return 0;
    }
    const int seeds = argc > 1 ? atoi(argv[1]) : 50;
    const int gpus = argc > 2 ? atoi(argv[2]) : 2;
    const bool threaded = argc > 3 ? atoi(argv[3]) != 0 : true;
    g_rename = argc > 4 ? atoi(argv[4]) != 0 : false;
    g_zero_copy = argc > 5 ? atoi(argv[5]) != 0 : false;
    g_two_lane = argc > 6 ? atoi(argv[6]) != 0 : true;
    int failures = 0;
    if (const char* one = getenv("SCHED_HARNESS_SEED")) {      // one random program, for debugging: SCHED_HARNESS_SEED=1038 sched_harness 0 3 1
        const int sd = atoi(one);
        if (sd >= 5000) {
            const int f = dag_program(sd, threaded);
            printf("netlist seed %d: %d mismatches\n", sd, f);
            return f ? 1 : 0;
        }
        const int f = random_program(sd, 1 + ((sd - 1000) % gpus), threaded);
        printf("seed %d: %d mismatches\n", sd, f);
        return f ? 1 : 0;
    }
    for (int s = 1; s <= seeds; s++) {
        const int f = random_program(1000 + s, 1 + (s % gpus), threaded);
        if (f) printf("FAIL random program seed %d: %d mismatches\n", 1000 + s, f);
        failures += f;
    }
    printf("random programs: %d seeds, %d failures\n", seeds, failures);
    // Every hazard class must have occurred over the seeds of the run (at least 3 times): a condition on the GENERATOR, so that no choice of
    // seeds hides a gap.  (Asked for from 12 seeds on, the fewest any test runs; the renamed-output class needs renaming.)
    {
        std::vector<std::string> need = {
            "raw_gate_to_tl_bootstrap", "raw_seiks_at_to_gate", "raw_seiks_at_to_user_gate", "raw_circuit_bootstrap_to_selector", "raw_cmux_to_seiks_at",
            "war_trlwe_after_cmux", "war_trlwe_in_place_after_cmux", "war_holder_upload_after_cmux", "war_holder_circuit_bootstrap_after_cmux",
            "waw_level0", "waw_level1", "waw_level2", "waw_level3",
            "cmux_rotate_chain_of_3_in_place", "cmux_in_place_on_c1", "cmux_in_place_on_c0", "holder_host_rewritten_under_copying_cmux",
            "siblings_adjacent", "siblings_separated_by_operand_write", "siblings_separated_by_flush", "siblings_separated_by_other_records",
            "siblings_on_different_streams", "group_outputs_all_have_readers", "level_with_kinds_0_1_2_and_circuit_bootstrap"};
        if (g_rename) need.push_back("renamed_kind2_output_fetched_and_polled_on_another_stream");
        printf("HAZARDS {");
        for (size_t i = 0; i < need.size(); i++) printf("%s\"%s\": %llu", i ? ", " : "", need[i].c_str(), (unsigned long long)g_hazards[need[i]]);
        printf("}\n");
        if (seeds >= 12)
            for (const std::string& n : need)
                if (g_hazards[n] < 3) { printf("FAIL hazard class %s occurred %llu times over %d seeds (at least 3 wanted)\n", n.c_str(), (unsigned long long)g_hazards[n], seeds); failures++; }
    }
    int dag_failures = 0;
    for (int s = 1; s <= seeds; s++) {
        const int f = dag_program(5000 + s, threaded);
        if (f) printf("FAIL random netlist seed %d: %d mismatches\n", 5000 + s, f);
        dag_failures += f;
    }
    printf("random netlists: %d seeds, %d failures, %llu flushes scheduled gate by gate on two lanes (%llu launches)\n", seeds, dag_failures,
           (unsigned long long)g_two_lane_groups, (unsigned long long)g_two_lane_launches);
    failures += dag_failures;
    for (Shape sh : {chained(threaded), ripple(threaded), intensive(threaded), multi_gpu(threaded), group_with_raw_handle_out(threaded), delivery_ahead_of_upload(threaded)}) {
        printf("SHAPE {\"name\": \"%s\", \"launch_sequences\": %llu, \"levels\": %llu, \"gates\": %llu, \"groups\": %llu, "
               "\"uploads\": %llu, \"uploads_shared\": %llu, \"failures\": %d, \"two_lane_groups\": %llu, \"two_lane_launches\": %llu}\n",
               sh.name, (unsigned long long)sh.launch_sequences, (unsigned long long)sh.levels, (unsigned long long)sh.gates,
               (unsigned long long)sh.groups, (unsigned long long)sh.uploads, (unsigned long long)sh.uploads_shared, sh.failures,
               (unsigned long long)sh.two_lane_groups, (unsigned long long)sh.two_lane_launches);
        failures += sh.failures;
    }
    printf("%s\n", failures ? "FAILED" : "ALL PASS");
    return failures ? 1 : 0;
}
