// capi.hip -- implementation of the C ABI declared in include/cufhe_amd.h.
// Host side of the gate path: device/key management (reference: src/cufhe_gates_gpu.cu:38-65,
// src/bootstrap_gpu.cu:97-155, src/keyswitch_gpu.cu:6-24) and the launch sequences that
// replace the per-gate launchers of src/bootstrap_gpu.cu:834-1292.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/cufhe_amd.h"
#include "sched_core.h"
#include "launch_plan.h"
#include "op_registry.h"
#include "kernels.hip.h"
#include "kernels_lvl2.hip.h"
#include "kernels_lvl2q.hip.h"
#include "kernels_ks2.hip.h"
#include "kernels_pks.hip.h"
#include "kernels_pack.hip.h"
#include "kernels_lut.hip.h"
#define CUFHE_AMD_LL_DECLARATIONS_ONLY      // defined in kernels_ll.hip
#include "kernels_ll.hip.h"
#include "kernels_ps.hip.h"

using namespace cufhe_amd;

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(-2, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                std::to_string(__LINE__) + ")");                               \
    } while (0)

struct EventPair { hipEvent_t a, b; uint64_t units; };

// Pinned host staging for descriptor uploads.  hipMemcpyAsync from pageable memory may
// return before the bytes have been read, so descriptors are staged in pinned blocks that
// are recycled only once the event recorded behind their copy has completed.
// A block is free again when its owner has RECORDED `done` behind the last device access, that event has completed, and the owner
// is not itself still reading the block on the host (`held`, cufhe_amd_trgsw_to_ntt_host): completion of a never-recorded or stale
// event says nothing about the current owner.
struct PinnedBlock { void* host = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; bool busy = false, recorded = false, held = false; };

// Per-stream device workspace (temporaries + descriptor arrays of one launch sequence).
// Work on one stream is ordered, so the next sequence on the same stream may overwrite the
// workspace of the previous one; distinct streams get distinct workspaces.  Grow-only.
// ks_digits: the digit words of the stream's last matrix-product key switch (launch_keyswitch), grow-only like the rest.
struct Workspace { char* base = nullptr; size_t bytes = 0; char* ks_digits = nullptr; size_t ks_digit_bytes = 0; };

// A dynamic-LDS opt-in (hipFuncSetAttribute) made once per device.  Calls on different streams may come from different threads, and each
// reads and sets the flag of the kernels it launches: atomic, set behind the attribute calls.  Two threads may both find it unset and both
// make the calls, which are idempotent; no thread launches before its own calls have returned.
struct OptInFlag {
    std::atomic<bool> v{false};
    OptInFlag() = default;
    OptInFlag(const OptInFlag& o) : v(o.v.load(std::memory_order_acquire)) {}
    OptInFlag& operator=(const OptInFlag& o) { v.store(o.v.load(std::memory_order_acquire), std::memory_order_release); return *this; }
    OptInFlag& operator=(bool b) { v.store(b, std::memory_order_release); return *this; }
    operator bool() const { return v.load(std::memory_order_acquire); }
};

struct DeviceState {
    bool ntt_ready = false, keys_ready = false;
    int cus = 0;                         // hipDeviceProp_t::multiProcessorCount (launch-shape rules: one grid round = a workgroup per CU)
    NttTables* tables = nullptr;
    NttTables* tables_r4 = nullptr;      // the same transform's tables for the radix-4 passes (ntt_r4.h): blind_rotate_kernel
    Ntt512Tables* tables512 = nullptr;   // [3]: the two 512-point halves (low-latency kernel), stand-alone N = 512
    double* bk_ntt = nullptr;
    uint32_t* ksk = nullptr;
    ksmm_v4i* ksk_mm = nullptr;          // the same key in matrix form [j][column][16] int8 (keyswitch_mm_kernel); null: could not be allocated
    uint32_t* tvs = nullptr;             // [kMaxUserGates][kN]: the user gates' test vectors (cufhe_amd_define_gate); CleanUp frees it
    // device fault word: pinned, host-coherent, mapped into the device (kernels_common.hip.h: kFault*); sticky until CleanUp
    uint32_t* fault_host = nullptr;
    uint32_t* fault = nullptr;
    bool profiling = false;
    OptInFlag br_lds_opt_in, ks_lds_opt_in;
    // N = 2048 / 64-bit torus (lvl2.inc.h)
    bool keys2_ready = false;
    OptInFlag br2_lds_opt_in, ks2_lds_opt_in;
    NttTables* tables2 = nullptr;      // [2]: the two half transforms
    double* bk2_ntt = nullptr;
    Ntt512Tables* tables2q = nullptr;  // [4]: the four quarter transforms (kernels_lvl2q.hip.h)
    double* bk2q_ntt = nullptr;        // the same key in the quarter layout
    OptInFlag br2q_lds_opt_in;
    uint32_t* ksk2 = nullptr;
    uint64_t* tvs2 = nullptr;          // [kTvRows2][k2N]: the lvl2 user gates' test vectors (cufhe_amd_lvl2_define_gate) and the library's own row (lvl2.inc.h: ensure_tvs2); CleanUp frees it
    uint32_t* cb_pksk = nullptr;       // circuit bootstrapping: the private key-switching key lvl2 -> lvl1 (cb.inc.h)
    uint32_t* pack_key = nullptr;      // TLWE packing: the lvl0 -> TRLWE key-switching key (pack.inc.h)
    std::vector<EventPair> br_events, ks_events;
    cufhe_amd_profile prof{};
    std::deque<PinnedBlock> staging;
    std::map<hipStream_t, Workspace> workspaces;
    std::mutex staging_mu;
};

// "cus_override" > 0: every launch-shape and flush rule behaves as on a device with that many CUs (a partitioned device, another
// chip; the rules are all in CU units) -- what tests use to check that nothing is tied to MI355X's 256
long g_cus_override = 0;
int cus_of(const struct DeviceState& s);
int g_gpu_num = 1;
int g_device_base = 0;         // physical HIP device of logical device 0 (one process per GPU: LOCAL_RANK)
long g_share_devices = 0;      // 1: logical devices beyond the visible GPUs wrap around (SetGPUNum(G) rehearsed on fewer GPUs)
int g_phys_count = 0;
int phys_device(int device)
{
    if (g_share_devices && g_phys_count > 0) return (g_device_base + device) % g_phys_count;
    return device + g_device_base;
}
// the launch-shape options ("ll_threshold", "ks_slices", ...: launch_plan.h); cus_of(s) and this are what every plan is made from
plan::Tuning g_tuning;
// "br_shape": 0 = by the rules of plan::plan_blind_rotate; 1 / 2 / 3 = every launch whole on the batch kernel (8 rotations per workgroup) / the
// paired low-latency kernel (2 per workgroup) / the single one.  thread_local: the scheduler's launch worker picks a shape per launch.
thread_local long g_br_shape = 0;
long g_cb_rotations = 3;       // lvl02 rotations per circuit bootstrap: 3 (one per TRGSW row) or 1 (all rows from one rotation)
long g_lvl0_ring = 1024;       // ring through which gates on lvl0 ciphertexts bootstrap: 1024 (lvl01/lvl10) or 2048 (lvl02/lvl20)
constexpr int kMaxLogicalDevices = 64;    // SetGPUNum bound (per-device tables of fixed size: paramsets.inc.h)
std::deque<DeviceState> g_dev(1);    // re-created only while no device is initialised (SetGPUNum)
int cus_of(const DeviceState& s) { return g_cus_override > 0 ? (int)g_cus_override : s.cus; }
std::mutex g_mu;

// /sys/bus/pci/devices/<domain:bus:dev.fn>/local_cpulist of a physical HIP device ("" when it cannot be read)
std::string device_local_cpulist(int phys)
{
    char pci[64];
    if (hipDeviceGetPCIBusId(pci, (int)sizeof pci, phys) != hipSuccess) { (void)hipGetLastError(); return ""; }
    std::string id(pci);
    for (auto& ch : id) ch = (char)tolower((unsigned char)ch);
    FILE* f = fopen(("/sys/bus/pci/devices/" + id + "/local_cpulist").c_str(), "r");
    if (!f) return "";
    char line[1024] = "";
    const bool ok = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    std::string out(ok ? line : "");
    while (!out.empty() && (out.back() == '\n' || out.back() == ' ')) out.pop_back();
    return out;
}

// Device allocations of the Initialize entry points go through here: "test_fail_alloc" n makes the (n+1)-th one fail like an exhausted
// device (then disarms itself), so that the error paths -- the old keys stay loaded and usable, nothing leaks -- can be exercised
long g_fail_alloc_countdown = -1;
hipError_t init_malloc(void** p, size_t bytes)
{
    if (g_fail_alloc_countdown >= 0 && g_fail_alloc_countdown-- == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipMalloc(p, bytes);
}

int check_device(int device)
{
    if (device < 0 || device >= g_gpu_num) return fail(-1, "device index out of range (SetGPUNum first)");
    return 0;
}
int use_device(int device)
{
    if (int rc = check_device(device)) return rc;
    HIP_TRY(hipSetDevice(phys_device(device)));
    return 0;
}

// DeviceState::cus of a logical device
int read_cus(DeviceState& s, int device)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, phys_device(device)));
    s.cus = prop.multiProcessorCount;
    return 0;
}

// twiddle tables: built by ntt_tables.h (host-only, checked on the CPU by tests/test_ntt_tables.py), uploaded here
int ensure_ntt(int device)
{
    DeviceState& s = g_dev[device];
    if (s.ntt_ready) return 0;
    HIP_TRY(hipSetDevice(phys_device(device)));
    if (int rc = read_cus(s, device)) return rc;
    // every allocation of this function is released again when a later one fails: a retry starts from nothing
    auto undo = [&]() {
        if (s.fault_host) { (void)hipHostFree(s.fault_host); s.fault_host = nullptr; s.fault = nullptr; }
        if (s.tables) { (void)hipFree(s.tables); s.tables = nullptr; }
        if (s.tables_r4) { (void)hipFree(s.tables_r4); s.tables_r4 = nullptr; }
        if (s.tables512) { (void)hipFree(s.tables512); s.tables512 = nullptr; }
    };
#define CUFHE_AMD_TRY_UNDO(expr)                                                               \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            undo();                                                                            \
            return fail(-2, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
        }                                                                                      \
    } while (0)
    CUFHE_AMD_TRY_UNDO(hipHostMalloc((void**)&s.fault_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    *s.fault_host = 0;
    CUFHE_AMD_TRY_UNDO(hipHostGetDevicePointer((void**)&s.fault, s.fault_host, 0));
    NttTables host;
    build_tables(host);
    CUFHE_AMD_TRY_UNDO(hipMalloc((void**)&s.tables, sizeof(NttTables)));
    CUFHE_AMD_TRY_UNDO(hipMemcpy(s.tables, &host, sizeof(NttTables), hipMemcpyHostToDevice));
    build_tables(host, true);
    CUFHE_AMD_TRY_UNDO(hipMalloc((void**)&s.tables_r4, sizeof(NttTables)));
    CUFHE_AMD_TRY_UNDO(hipMemcpy(s.tables_r4, &host, sizeof(NttTables), hipMemcpyHostToDevice));
    static Ntt512Tables host512[3];
    build_tables_512(host512);
    for (int h = 0; h < 2; h++)
        if (!fill_r4_products_512(host512[h])) return fail(-2, "half-transform tables: the stage-b twiddles of a block are not I apart (radix-4 form)");
    CUFHE_AMD_TRY_UNDO(hipMalloc((void**)&s.tables512, sizeof(host512)));
    CUFHE_AMD_TRY_UNDO(hipMemcpy(s.tables512, host512, sizeof(host512), hipMemcpyHostToDevice));
#undef CUFHE_AMD_TRY_UNDO
    s.ntt_ready = true;
    return 0;
}

// A kernel that found its own result untrustworthy has set a bit in the device's fault word (today: the bounded LDS
// rendezvous of blind_rotate_ll2_kernel).  Called wherever the host observes completion (Synchronize, StreamQuery,
// StreamSynchronize, the scheduler's event polls): status -5 with text, where the reference would have printed
// "CuCheckError() failed" and exited (include/details/error_gpu.cuh:40-60; the C++ shim aborts on any negative status).
// Sticky, like a CUDA context error, until CleanUp().
int device_fault(int device)
{
    DeviceState& s = g_dev[device];
    if (!s.fault_host) return 0;
    const uint32_t bits = __atomic_load_n(s.fault_host, __ATOMIC_ACQUIRE);
    if (bits == 0) return 0;
    std::string what;
    if (bits & kFaultLl2SyncTimeout) what += " blind_rotate_ll2_kernel: the inverse waves' LDS rendezvous timed out;";
    if (bits & ~kFaultLl2SyncTimeout) what += " unknown bits;";
    char hex[16];
    snprintf(hex, sizeof hex, "0x%x", bits);
    return fail(-5, std::string("device ") + std::to_string(device) + " fault word " + hex + ":" + what +
                        " ciphertexts produced since Initialize() are not trustworthy -- CleanUp() and Initialize() again");
}


struct Scratch {   // bump allocator over the stream's workspace
    char* cur;
    char* end;
    hipStream_t st;
    int alloc(void** p, size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        if (cur + bytes > end) return fail(-4, "internal: workspace under-sized");
        *p = cur;
        cur += bytes;
        return 0;
    }
};

int open_scratch(DeviceState& s, hipStream_t st, size_t bytes, Scratch* sc)
{
    std::lock_guard<std::mutex> lk(s.staging_mu);
    Workspace& w = s.workspaces[st];
    if (w.bytes < bytes) {
        if (w.base) {
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(hipFree(w.base));
            w.base = nullptr; w.bytes = 0;
        }
        const size_t want = bytes + bytes / 4 + (1 << 20);
        HIP_TRY(hipMalloc((void**)&w.base, want));
        w.bytes = want;
    }
    sc->cur = w.base; sc->end = w.base + w.bytes; sc->st = st;
    return 0;
}

int acquire_staging(DeviceState& s, size_t bytes, PinnedBlock** out)
{
    std::lock_guard<std::mutex> lk(s.staging_mu);
    for (auto& b : s.staging) {
        if (b.busy && b.recorded && !b.held && hipEventQuery(b.done) == hipSuccess) b.busy = false;
        if (!b.busy && b.bytes >= bytes) { b.busy = true; b.recorded = false; b.held = false; *out = &b; return 0; }
    }
    PinnedBlock nb;
    nb.bytes = bytes < 65536 ? 65536 : bytes;
    HIP_TRY(hipHostMalloc(&nb.host, nb.bytes, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&nb.done, hipEventDisableTiming));
    nb.busy = true;
    s.staging.push_back(nb);
    *out = &s.staging.back();
    return 0;
}
// the owner's last device access to the block is on `st`: from its completion on the block may be handed out again
int staging_done_after(DeviceState& s, PinnedBlock* blk, hipStream_t st)
{
    HIP_TRY(hipEventRecord(blk->done, st));
    std::lock_guard<std::mutex> lk(s.staging_mu);
    blk->recorded = true;
    return 0;
}
void staging_hold(DeviceState& s, PinnedBlock* blk, bool held)
{
    std::lock_guard<std::mutex> lk(s.staging_mu);
    blk->held = held;
}
// The owner of a block between acquire_staging and staging_done_after.  A failing HIP call in between returns early: without this
// guard the block would stay busy and unrecorded for ever (a pinned-memory leak, and every later call would allocate a new block).
// On that path the device may still be reading or writing the block, so it is handed back only after the device has drained.
struct StagingOwner {
    DeviceState& s;
    PinnedBlock* b;
    bool ok = false;
    void recorded() { ok = true; }
    ~StagingOwner()
    {
        if (!ok) (void)hipDeviceSynchronize();
        std::lock_guard<std::mutex> lk(s.staging_mu);
        b->held = false;
        if (!ok) { b->busy = false; b->recorded = false; }
    }
};

template <class Desc>
int upload_descs(DeviceState& s, Scratch& sc, const std::vector<Desc>& h, Desc** d)
{
    *d = nullptr;
    if (h.empty()) return 0;
    const size_t bytes = h.size() * sizeof(Desc);
    if (int rc = sc.alloc((void**)d, bytes)) return rc;
    PinnedBlock* blk = nullptr;
    if (int rc = acquire_staging(s, bytes, &blk)) return rc;
    StagingOwner owner{s, blk};
    memcpy(blk->host, h.data(), bytes);
    HIP_TRY(hipMemcpyAsync(*d, blk->host, bytes, hipMemcpyHostToDevice, sc.st));
    if (int rc = staging_done_after(s, blk, sc.st)) return rc;
    owner.recorded();
    return 0;
}

// HIP events around one launcher call on its stream (cufhe_amd_profile_enable): begin() creates the pair and records the first,
// commit() records the second and hands the pair with `units` to br_events / ks_events (cufhe_amd_profile_get).  A return in
// between destroys the pair instead of leaking it.
struct ProfScope {
    DeviceState& s;
    hipStream_t st;
    uint64_t units;
    bool keyswitch;
    EventPair ev{};
    int begin()
    {
        if (!s.profiling) return 0;
        HIP_TRY(hipEventCreate(&ev.a));
        HIP_TRY(hipEventCreate(&ev.b));
        HIP_TRY(hipEventRecord(ev.a, st));
        return 0;
    }
    int commit()
    {
        if (!ev.a) return 0;
        HIP_TRY(hipEventRecord(ev.b, st));
        ev.units = units;
        std::lock_guard<std::mutex> lk(s.staging_mu);
        (keyswitch ? s.ks_events : s.br_events).push_back(ev);
        ev = EventPair{};
        return 0;
    }
    ~ProfScope()
    {
        if (ev.a) (void)hipEventDestroy(ev.a);
        if (ev.b) (void)hipEventDestroy(ev.b);
    }
};

// tables (optional, a device array parallel to d): rotation g starts from X^bbar times the TRLWE tables[g] instead of its descriptor's
// test vector (cufhe_amd_lut_*_batch, lut.inc.h), on the <true> instantiations of the same three kernels; nullptr: every other launch
int launch_blind_rotate(DeviceState& s, hipStream_t st, const LinDesc* d, size_t count, int steps, uint32_t* acc_dump,
                        const uint32_t* const* tables)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, false};
    if (int rc = prof.begin()) return rc;
    if (!s.br_lds_opt_in) {      // > 64 KiB of dynamic LDS needs an opt-in, per device
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kBrLdsBytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kBrLdsBytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ll_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLlLdsBytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ll_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLlLdsBytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ll2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLl2LdsBytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ll2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLl2LdsBytes));
        s.br_lds_opt_in = true;
    }
    const plan::BrPlan p = plan::plan_blind_rotate(count, cus_of(s), g_tuning, g_br_shape);
    for (int i = 0; i < p.n; i++) {
        const plan::BrSegment& seg = p.seg[i];
        const LinDesc* dd = d + seg.first;
        uint32_t* dump = acc_dump ? acc_dump + seg.first * 2 * kN : nullptr;
        const uint32_t* const* tt = tables ? tables + seg.first : nullptr;
        const int n = (int)seg.count;
        const dim3 batch_grid((unsigned)((seg.count + seg.active - 1) / seg.active)), ll_grid((unsigned)seg.count), ll2_grid((unsigned)((seg.count + 1) / 2));
        switch (seg.kernel) {
            case plan::BrKernel::Batch:
                hipLaunchKernelGGL(tt ? blind_rotate_kernel<true> : blind_rotate_kernel<false>, batch_grid, dim3(kBrThreads), kBrLdsBytes, st,
                                   dd, n, s.bk_ntt, s.tables_r4, steps, dump, seg.active, s.tvs, tt);
                break;
            case plan::BrKernel::Ll:      // one 16-wave workgroup per rotation, transforms split in halves (kernels_ll.hip.h)
                hipLaunchKernelGGL(tt ? blind_rotate_ll_kernel<true> : blind_rotate_ll_kernel<false>, ll_grid, dim3(kLlThreads), kLlLdsBytes, st,
                                   dd, n, s.bk_ntt, s.tables512, steps, dump, s.tvs, tt);
                break;
            case plan::BrKernel::Ll2:     // two rotations per workgroup: the row phase of one beside the inverse transforms of the other
                hipLaunchKernelGGL(tt ? blind_rotate_ll2_kernel<true> : blind_rotate_ll2_kernel<false>, ll2_grid, dim3(kLlThreads), kLl2LdsBytes, st,
                                   dd, n, s.bk_ntt, s.tables512, steps, dump, s.fault, s.tvs, tt);
                break;
        }
    }
    HIP_TRY(hipGetLastError());
    return prof.commit();
}
static_assert(plan::kBatchWaves == kBrWavesPerBlock && plan::kKsMaxPerWg == kKsWaves && kKsSplit == 8, "launch_plan.h plans for these kernels");
// the key-switch plan of a path (launch_plan.h) over the shape S
template <class S>
plan::KsPlan plan_keyswitch_of(const DeviceState& s, size_t count, plan::KsRule rule)
{
    return plan::plan_keyswitch(count, cus_of(s), S::kn, KsDims<S>::min_slices, rule, g_tuning);
}
// keyswitch_kernel<S> over `ksk_padded` ([kn][t][2][row_pad] u32); *opted_in: the instantiation's dynamic-LDS opt-in on this device
template <class S>
int launch_keyswitch_shared(DeviceState& s, hipStream_t st, const typename S::Desc* d, size_t count, const uint32_t* ksk_padded, OptInFlag* opted_in, const plan::KsPlan& p)
{
    if (!*opted_in) {
        HIP_TRY(hipFuncSetAttribute((const void*)keyswitch_kernel<S>, hipFuncAttributeMaxDynamicSharedMemorySize, KsDims<S>::lds_bytes));
        *opted_in = true;
    }
    const int per_wg = p.per_wg, slices = p.slices;
    if (slices > 1) hipLaunchKernelGGL(keyswitch_zero_kernel<S>, dim3((unsigned)count), dim3(256), 0, st, d, (int)count);
    const unsigned ks_blocks = (unsigned)((count + per_wg - 1) / per_wg) * (unsigned)slices;
    hipLaunchKernelGGL(keyswitch_kernel<S>, dim3(ks_blocks), dim3(kKsThreads), KsDims<S>::lds_bytes, st, d, (int)count, ksk_padded, per_wg, slices);
    return 0;
}
// keyswitch_direct_kernel<S, SPLIT>: SPLIT workgroups per ciphertext, rows straight from L2; above one they add into a zeroed output
template <class S, int SPLIT>
void launch_keyswitch_direct(hipStream_t st, const typename S::Desc* d, size_t count, const uint32_t* ksk_padded)
{
    if (SPLIT > 1) hipLaunchKernelGGL(keyswitch_zero_kernel<S>, dim3((unsigned)count), dim3(256), 0, st, d, (int)count);
    hipLaunchKernelGGL((keyswitch_direct_kernel<S, SPLIT>), dim3((unsigned)count * SPLIT), dim3(kKsThreads), 0, st, d, (int)count, ksk_padded);
}
// keyswitch_mm_kernel: the digit words of the launch into the stream's grow-only buffer, then the product (kernels_ks2.hip.h)
int launch_keyswitch_matrix(DeviceState& s, hipStream_t st, const LinDesc* d, size_t count)
{
    uint32_t* dig = nullptr;
    {
        std::lock_guard<std::mutex> lk(s.staging_mu);
        Workspace& w = s.workspaces[st];
        const size_t bytes = ks_mm_digit_bytes(count);
        if (w.ks_digit_bytes < bytes) {
            if (w.ks_digits) {
                HIP_TRY(hipStreamSynchronize(st));
                HIP_TRY(hipFree(w.ks_digits));
                w.ks_digits = nullptr; w.ks_digit_bytes = 0;
            }
            HIP_TRY(hipMalloc((void**)&w.ks_digits, bytes));
            w.ks_digit_bytes = bytes;
        }
        dig = (uint32_t*)w.ks_digits;
    }
    const unsigned tiles = (unsigned)((count + kKsMmRows - 1) / kKsMmRows);
    hipLaunchKernelGGL(ks_mm_digits_kernel<KsShapeDefault>, dim3(tiles, kKsMmSteps / kKsMmDigitChunk), dim3(256), 0, st, d, (int)count, dig);
    hipLaunchKernelGGL(keyswitch_mm_kernel<KsShapeDefault>, dim3(tiles * kKsMmWordBlocks), dim3(64), 0, st, d, (int)count, s.ksk_mm, dig);
    return 0;
}
int launch_keyswitch(DeviceState& s, hipStream_t st, const LinDesc* d, size_t count)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, true};
    if (int rc = prof.begin()) return rc;
    if (s.ksk_mm && plan::use_matrix_keyswitch(count, cus_of(s), g_tuning)) {
        if (int rc = launch_keyswitch_matrix(s, st, d, count)) return rc;
        HIP_TRY(hipGetLastError());
        return prof.commit();
    }
    const plan::KsPlan p = plan_keyswitch_of<KsShapeDefault>(s, count, plan::kKsDefaultPath);
    if (p.kernel == plan::KsKernel::Split8) {
        launch_keyswitch_direct<KsShapeDefault, kKsSplit>(st, d, count, s.ksk);
    } else if (p.kernel == plan::KsKernel::WorkgroupPer) {
        launch_keyswitch_direct<KsShapeDefault, 1>(st, d, count, s.ksk);
    } else {
        if (int rc = launch_keyswitch_shared<KsShapeDefault>(s, st, d, count, s.ksk, &s.ks_lds_opt_in, p)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return prof.commit();
}
int launch_lincomb(hipStream_t st, const LinDesc* d, size_t count, int words)
{
    if (count == 0) return 0;
    const unsigned blocks = (unsigned)(count < 4096 ? count : 4096);
    hipLaunchKernelGGL(lincomb_kernel, dim3(blocks), dim3(256), 0, st, d, (int)count, words);
    HIP_TRY(hipGetLastError());
    return 0;
}

// (ca, cb, offset/mu) of the ten two-input gates, src/bootstrap_gpu.cu:424-512,591-679
const int kGateTab[10][3] = {
    {-1, -1, 1}, {-1, -1, -1}, {-2, -2, -2}, {1, 1, -1}, {1, 1, 1},
    {2, 2, 2},   {-1, 1, -1},  {1, -1, -1},  {-1, 1, 1}, {1, -1, 1},
};

using sched::GateRef;

// The op ids a caller defines (user gates of the three paths, lookups): ranges, tables and the rule of where an id runs are
// op_registry.h's.  The test vector of definition k is row k of every device's table: DeviceState::tvs, ::tvs2 (64-bit, lvl2.inc.h), or
// PsState::tvs of the set the definition was made for (N words of that set, paramsets.inc.h).  CleanUp drops the definitions.
using opreg::UserGate;
using opreg::user_gate_arity;
opreg::Registry g_ops;
static_assert(opreg::kUserOps.cap == kMaxUserGates && opreg::kPsUserOps.cap == kMaxUserGates && opreg::kLvl2UserOps.cap == kMaxUserGates2,
              "the header's capacities are the device tables'");
static_assert(opreg::kOutputShift == kMaxOutputShift && opreg::kRingN == kN, "the registry's output shift and ring are the kernels'");
int refuse(opreg::Refusal r) { return r == opreg::Refusal::None ? 0 : fail(-1, opreg::refusal_text(r)); }
// packed ROM words: op ids that carry an index / an exponent (include/cufhe_amd.h)
bool is_seiks_at(int op) { return op >= CUFHE_AMD_TL_SEIKS_AT(0) && op <= CUFHE_AMD_TL_SEIKS_AT(kN - 1); }
bool is_cmux_rotate(int op) { return op >= CUFHE_AMD_TL_CMUX_ROTATE(0) && op <= CUFHE_AMD_TL_CMUX_ROTATE(2 * kN - 1); }
int fail_packed_rom_set() { return fail(-1, "packed ROM words (TRLWE rotation, rotating CMUX, indexed SampleExtract) run on the default path only: not with \"param_set\" active"); }

template <class GetGate>
int run_gates_lvl2(int device, void* stream, size_t count, GetGate get);   // lvl2.inc.h
template <class GetGate>
int run_gates_ps(int set, int device, void* stream, int level, size_t count, GetGate get);   // paramsets.inc.h
int ps_ctxt_words(int set, int level);
void lvl2_release_host_key();          // lvl2.inc.h
// The compiled parameter sets of kernels_ps.hip.h in the order of their indices ("param_set", cufhe_amd_ps_*): ps_dispatch
// (paramsets.inc.h) and the TRGSW slot size below are both taken from this one list.
using CompiledSets = std::tuple<PsDefault, PsK2N512, PsCggi16, PsSmallMod>;
static_assert(std::tuple_size_v<CompiledSets> == kParamSets, "every compiled parameter set is listed once");
// a TRGSW holder's device slot (ciphertext handle of level 3) fits the NTT-domain TRGSW of every compiled set, key limbs included
constexpr int kMaxTrgswNttWords =
    std::apply([](auto... ps) { return std::max({(int)(2 * kBkStepDoubles), (int)(2 * PsDims<decltype(ps)>::bk_ntt_step_doubles)...}); }, CompiledSets{});
int run_trlwe_ops_ps(int set, int device, void* stream, const GateRef* g, size_t n);         // paramsets.inc.h
int ps_trgsw_to_ntt_host(int set, int device, void* stream, const uint32_t* trgsw_host, double* trgsw_ntt_host);
// >= 0: the per-gate API (both ciphertext levels, both gate orders) runs on this compiled parameter set -- the reference's build-time
// choice (CMakeLists.txt:8-24) serves every entry point the same way; ciphertexts then have the set's sizes (cufhe_amd_ctxt_words)
long g_param_set = -1;

// The gate lowering of every bootstrapping path (BasePath below, PsPath<PS> in paramsets.inc.h, Lvl2Path in lvl2.inc.h): a list of
// gates -> rotation, key-switch and lincomb descriptors and one launch of each.  The path P gives
//   RotD, KsD          the descriptors its rotation and key-switch launchers take
//   Mid, mid_words     word type and size of the ciphertext between rotation and key switch (lvl1; lvl2 on the N = 2048 path)
//   lvl0_words, n      lvl0 ciphertext words, CMux steps of a blind rotation
//   ks_mu              the mu of the Mux sum in the key switch
//   lvl1_gates         whether it has gates on Mid ciphertexts (level 1)
//   s, ready(), rotate(), keyswitch()   its device, the readiness check and the two launchers
//   path, set_index    the route it is (opreg::Path) and the compiled parameter set it runs on, -1 for the default path and the N = 2048
//                      ring: which user gates it runs is the registry's rule (op_registry.h)
//   pad(row, s)        the rotation descriptor's pad that names row `row` of its test-vector table with 2^s outputs
//   rotate_takes_tv_rows   whether rotate() takes one more argument: whether any descriptor names a row
// Level 0: blind rotate -> key switch (__HomGate__ br -> iks); level 1: key switch -> blind rotate (iks -> br); Not / Copy and the
// level-1 Mux sums run last, as one lincomb.  The three-input user gates' c0 in0 + c1 in1 run first, as one lincomb into temporaries.
template <class P, class GetGate>
int lower_gates(const P& p, hipStream_t st, int level, size_t count, GetGate get)
{
    using Mid = typename P::Mid;
    // every id is put to the registry once; what it answers (the definition, its row and the output) serves both passes below
    std::vector<opreg::Admission> adm;        // stays empty for a list without a user gate's id
    const opreg::Route route{P::path, P::set_index, level, g_param_set >= 0};
    if (int rc = refuse(opreg::admit_list(g_ops, count, [&](size_t g) { return get(g).op; }, route, opreg::Entry::Direct, &adm))) return rc;
    if (int rc = p.ready()) return rc;
    if (level != 0 && level != 1) return fail(-1, "level must be 0 or 1");
    if (count == 0) return 0;
    const uint32_t negmu = 0u - kMu;
    bool tv_rows = false;         // a rotation descriptor names a test-vector row (read by the launchers of the lvl2 path and of the sets)

    // Outputs of one multi-output definition on the same operands form one evaluation (one rotation, all nout outputs extracted into
    // scratch): fused by (definition, in0, in1, in2) whatever the order of the list.  fuse[g] is the evaluation of gate g.
    struct Eval { uint32_t* t1; uint32_t* t0; bool done; };
    std::map<std::tuple<int, const uint32_t*, const uint32_t*, const uint32_t*>, size_t> evals;
    std::vector<size_t> fuse;
    std::vector<Eval> ev;
    size_t nmulti_words = 0;
    // first pass: count temporaries
    size_t nrot = 0, npre = 0;
    for (size_t g = 0; g < count; g++) {
        const int op = get(g).op;
        if (const UserGate* u = adm.empty() ? nullptr : adm[g].gate) {
            const int arity = user_gate_arity(*u);
            bool rotation = true;        // the gate brings a rotation of its own: not the second, third, .. output of an evaluation
            if (u->nout > 1) {
                const GateRef gr = get(g);
                const auto key = std::make_tuple(adm[g].k, (const uint32_t*)gr.in0, arity >= 2 ? gr.in1 : nullptr, arity == 3 ? gr.in2 : nullptr);
                if (fuse.empty()) fuse.assign(count, (size_t)-1);
                const auto [it, fresh] = evals.emplace(key, ev.size());
                if ((rotation = fresh)) {
                    ev.push_back({nullptr, nullptr, false});
                    nmulti_words += (size_t)u->nout;
                }
                fuse[g] = it->second;
            } else {
                nrot += 1;
            }
            if (rotation && arity == 3) npre += 1;
            continue;
        }
        if (op < 0 || op >= CUFHE_AMD_NUM_OPS) return fail(-1, "unknown gate op");
        if (op == CUFHE_AMD_MUX || op == CUFHE_AMD_NMUX) nrot += 2;
        else if (op < CUFHE_AMD_MUX) nrot += 1;
    }
    const size_t level_words = level ? P::mid_words * sizeof(Mid) / sizeof(uint32_t) : P::lvl0_words;
    Scratch sc;
    {
        const size_t desc = std::max({sizeof(typename P::RotD), sizeof(typename P::KsD), sizeof(LinDesc)});
        const size_t need = nrot * (P::mid_words * sizeof(Mid) + P::lvl0_words * sizeof(uint32_t)) + npre * level_words * sizeof(uint32_t) +
                            nmulti_words * P::mid_words * sizeof(Mid) + ev.size() * P::lvl0_words * sizeof(uint32_t) + (count * 6 + 8) * desc + 8192;
        if (int rc = open_scratch(p.s, st, need, &sc)) return rc;
    }
    Mid* tmpm = nullptr;          // the multi-output evaluations' outputs, nout contiguous lvl1 ciphertexts each
    uint32_t* tmpm0 = nullptr;    // level 1: their key switches' results, one per evaluation
    if (!ev.empty()) {
        if (int rc = sc.alloc((void**)&tmpm, nmulti_words * P::mid_words * sizeof(Mid))) return rc;
        if (level == 1)
            if (int rc = sc.alloc((void**)&tmpm0, ev.size() * P::lvl0_words * sizeof(uint32_t))) return rc;
    }
    Mid* tmp1 = nullptr;          // the rotations' results, one per rotation
    uint32_t* tmp0 = nullptr;     // level 1: the key switches' results, one per rotation
    uint32_t* tmpp = nullptr;     // the pre-added c0 in0 + c1 in1 of the three-input user gates, at the gates' level
    if (nrot) {
        if (int rc = sc.alloc((void**)&tmp1, nrot * P::mid_words * sizeof(Mid))) return rc;
        if (level == 1)
            if (int rc = sc.alloc((void**)&tmp0, nrot * P::lvl0_words * sizeof(uint32_t))) return rc;
    }
    if (npre)
        if (int rc = sc.alloc((void**)&tmpp, npre * level_words * sizeof(uint32_t))) return rc;
    std::vector<typename P::RotD> rot;
    std::vector<typename P::KsD> ks;
    std::vector<LinDesc> lin, pre;
    rot.reserve(count * 2); ks.reserve(count * 2); lin.reserve(count); pre.reserve(npre);
    size_t ir = 0, im = 0;
    for (size_t g = 0; g < count; g++) {
        const GateRef gr = get(g);
        if (!gr.out || !gr.in0) return fail(-1, "null ciphertext pointer");
        if (const UserGate* u = adm.empty() ? nullptr : adm[g].gate) {
            // x = c0 in0 + c1 in1 + c2 in2 + (0, ..., 0, off) through the two-input gate path; the rotation starts from the definition's
            // test vector (pad: its row and output shift) or from mu (pad 0).  Output j of a multi-output evaluation: the evaluation's
            // one rotation is emitted with its first requested output and writes all nout outputs to scratch
            if (const char* missing = opreg::missing_operand(*u, gr.in1 != nullptr, gr.in2 != nullptr)) return fail(-1, missing);
            const uint32_t pad = u->tv ? P::pad(adm[g].k, u->s) : 0u;
            tv_rows |= pad != 0;
            const bool multi = u->nout > 1;
            Eval own{nullptr, nullptr, false};
            Eval& e = multi ? ev[fuse[g]] : own;
            if (!e.done) {
                e.done = true;
                if (multi) {
                    e.t1 = (uint32_t*)(tmpm + im * P::mid_words);
                    e.t0 = level ? tmpm0 + fuse[g] * P::lvl0_words : nullptr;
                    im += (size_t)u->nout;
                } else {      // level 1: the rotation writes straight to `out`
                    e.t1 = level ? gr.out : (uint32_t*)(tmp1 + ir * P::mid_words);
                    e.t0 = level ? tmp0 + ir * P::lvl0_words : nullptr;
                    ir += 1;
                }
                const opreg::GateOperands x = opreg::user_gate_operands(*u, gr.in0, gr.in1, gr.in2, [&] { return tmpp + pre.size() * level_words; }, pre);
                if (level == 0) {
                    rot.push_back({x.a, x.b, (Mid*)e.t1, x.ca, x.cb, u->off, pad});
                } else if constexpr (P::lvl1_gates) {
                    ks.push_back({x.a, x.b, e.t0, x.ca, x.cb, u->off});
                    rot.push_back({e.t0, e.t0, (Mid*)e.t1, 1, 0, 0u, pad});
                }
            }
            // level 0: the key switch of output j into out; level 1: a copy of scratch output j into out (last lincomb)
            Mid* tj = (Mid*)e.t1 + (size_t)adm[g].j * P::mid_words;
            if (level == 0) ks.push_back({tj, tj, gr.out, 1, 0, 0u});
            else if (multi) lin.push_back({(const uint32_t*)tj, (const uint32_t*)tj, (uint32_t*)gr.out, 1, 0, 0u, 0u});
            continue;
        }
        if (gr.op == CUFHE_AMD_NOT || gr.op == CUFHE_AMD_COPY) {
            lin.push_back({gr.in0, gr.in0, gr.out, gr.op == CUFHE_AMD_NOT ? -1 : 1, 0, 0u, 0u});
            continue;
        }
        if (!gr.in1) return fail(-1, "gate needs a second operand");
        if (gr.op == CUFHE_AMD_MUX || gr.op == CUFHE_AMD_NMUX) {
            if (!gr.in2) return fail(-1, "mux needs a third operand");
            Mid* ta = tmp1 + (ir + 0) * P::mid_words;
            Mid* tb = tmp1 + (ir + 1) * P::mid_words;
            const bool neg = gr.op == CUFHE_AMD_NMUX;
            if (level == 0) {   // src/bootstrap_gpu.cu:515-588
                rot.push_back({gr.in0, gr.in1, ta, 1, 1, negmu});
                rot.push_back({gr.in0, gr.in2, tb, -1, 1, negmu});
                ks.push_back({ta, tb, gr.out, neg ? -1 : 1, neg ? -1 : 1, neg ? 0u - P::ks_mu : P::ks_mu});
            } else if constexpr (P::lvl1_gates) {   // src/bootstrap_gpu.cu:706-780: two key switches, two rotations, the sum of the extracted ciphertexts
                uint32_t* t0a = tmp0 + (ir + 0) * P::lvl0_words;
                uint32_t* t0b = tmp0 + (ir + 1) * P::lvl0_words;
                ks.push_back({gr.in0, gr.in1, t0a, 1, 1, negmu});
                ks.push_back({gr.in0, gr.in2, t0b, -1, 1, negmu});
                rot.push_back({t0a, t0a, ta, 1, 0, 0u});
                rot.push_back({t0b, t0b, tb, 1, 0, 0u});
                lin.push_back({ta, tb, gr.out, neg ? -1 : 1, neg ? -1 : 1, neg ? negmu : kMu, 0u});
            }
            ir += 2;
            continue;
        }
        const int ca = kGateTab[gr.op][0], cb = kGateTab[gr.op][1];
        const uint32_t off = (uint32_t)kGateTab[gr.op][2] * kMu;
        if (level == 0) {       // __HomGate__ br -> iks, src/bootstrap_gpu.cu:402-421
            Mid* t1 = tmp1 + ir * P::mid_words;
            rot.push_back({gr.in0, gr.in1, t1, ca, cb, off});
            ks.push_back({t1, t1, gr.out, 1, 0, 0u});
        } else if constexpr (P::lvl1_gates) {   // __HomGate__ iks -> br, src/bootstrap_gpu.cu:383-400
            uint32_t* t0 = tmp0 + ir * P::lvl0_words;
            ks.push_back({gr.in0, gr.in1, t0, ca, cb, off});
            rot.push_back({t0, t0, gr.out, 1, 0, 0u});
        }
        ir += 1;
    }
    // Mux/NMux at level 1 write their rotations to temporaries, two-input gates at level 1
    // write straight to `out`; a lincomb that reads tmp1 must run after the rotations.
    typename P::RotD* drot;
    typename P::KsD* dks;
    LinDesc *dlin, *dpre;
    if (int rc = upload_descs(p.s, sc, rot, &drot)) return rc;
    if (int rc = upload_descs(p.s, sc, ks, &dks)) return rc;
    if (int rc = upload_descs(p.s, sc, lin, &dlin)) return rc;
    if (int rc = upload_descs(p.s, sc, pre, &dpre)) return rc;
    if (int rc = launch_lincomb(st, dpre, pre.size(), (int)level_words)) return rc;
    auto rotate = [&] {
        if constexpr (P::rotate_takes_tv_rows) return p.rotate(st, drot, rot.size(), P::n, nullptr, tv_rows);
        else return p.rotate(st, drot, rot.size(), P::n, nullptr);
    };
    if (level == 0) {
        if (int rc = rotate()) return rc;
        if (int rc = p.keyswitch(st, dks, ks.size())) return rc;
    } else if constexpr (P::lvl1_gates) {
        if (int rc = p.keyswitch(st, dks, ks.size())) return rc;
        if (int rc = rotate()) return rc;
    }
    return launch_lincomb(st, dlin, lin.size(), level ? P::mid_words : P::lvl0_words);
}

// The TRLWE-level operations recorded through the scheduler (include/cufhe_gpu.cuh:124-146,209-216,282-285;
// src/cufhe_gates_gpu.cu:86-146) or given as a batch (trlwe_batch below) on BasePath or a PsPath<PS>: any mix of
//   CUFHE_AMD_TL_BOOTSTRAP  lvl0 TLWE -> TRLWE     __BlindRotateGlobal__, src/bootstrap_gpu.cu:317-323
//   CUFHE_AMD_TL_REFRESH    TRLWE -> TRLWE         __SEIandBootstrap2TRLWE__, :325-364
//   CUFHE_AMD_TL_SEIKS      TRLWE -> lvl0 TLWE     __SEIandKS__, src/keyswitch_gpu.cu:26-40
// as ONE launch sequence: sample extracts, one key-switch launch, one blind-rotate launch, scatter; and the CMUXNTT calls of the level
// (src/bootstrap_gpu.cu:197-285).  Beside what lower_gates uses the path gives se_kernel (the sample extract), trlwe_words, and
// has_cmux with cmux(): only the small-modulus build of the reference leaves CMUXNTT out (src/cufhe_gates_gpu.cu:68-86).
int lower_cb_ops(DeviceState& s, hipStream_t st, const GateRef* g, size_t n);   // cb.inc.h
int cb_ready(const DeviceState& s, bool rotate);

template <class P>
int lower_trlwe_ops(const P& p, hipStream_t st, const GateRef* g, size_t n)
{
    DeviceState& s = p.s;
    if (n == 0) return 0;
    constexpr size_t tw = P::trlwe_words;
    size_t n_se = 0, n_rot = 0, n_t0 = 0, n_cmux = 0, n_cb = 0, n_cmuxr = 0;
    for (size_t i = 0; i < n; i++) {
        if (!g[i].out || !g[i].in0) return fail(-1, "null operand");
        switch (g[i].op) {
            case CUFHE_AMD_TL_BOOTSTRAP: n_rot++; break;
            case CUFHE_AMD_TL_REFRESH: n_se++; n_rot++; n_t0++; break;
            case CUFHE_AMD_TL_SEIKS: n_se++; break;
            case CUFHE_AMD_TL_CMUX:
                if (!P::has_cmux) return fail(-1, "CMUXNTT: the small-modulus build of the reference has none (src/cufhe_gates_gpu.cu:68-86)");
                if (!g[i].in1 || !g[i].in2) return fail(-1, "CMUXNTT: null operand");
                n_cmux++;
                break;
            case CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP: n_cb++; break;
            default:
                // packed ROM words: the indexed extraction joins the level's sample extracts and key switch, the rotating CMUX its CMUXNTT calls
                if (P::packed_rom && is_seiks_at(g[i].op)) { n_se++; break; }
                if (P::packed_rom && is_cmux_rotate(g[i].op)) {
                    if (!g[i].in2) return fail(-1, "rotating CMUX: null operand");
                    n_cmuxr++;
                    break;
                }
                return fail(-1, "unknown TRLWE-level op");
        }
    }
    if (n_cmux + n_cmuxr + n_cb < n)
        if (int rc = p.ready()) return rc;
    if ((n_cmux || n_cmuxr) && !s.ntt_ready) return fail(-3, "Initialize() has not been called for this device");
    // the circuit bootstraps of this level first, on their own scratch (the stream orders the reuse of the workspace)
    if (n_cb) {
        if (int rc = lower_cb_ops(s, st, g, n)) return rc;
        if (n_cb == n) return 0;
    }
    Scratch sc;
    // descriptors: a Refresh has one in each of four lists (se, ks, rot, scat), every other operation fewer
    const size_t need = (n_se * P::mid_words + n_t0 * P::lvl0_words + n_rot * tw) * 4 + (4 * n + 8) * sizeof(LinDesc) +
                        n_cmux * sizeof(CmuxDesc) + n_cmuxr * sizeof(CmuxRotDesc) + 16384;
    if (int rc = open_scratch(s, st, need, &sc)) return rc;
    if (n_cmux) {      // the CMUXNTT calls of this level: independent of its other operations (the scheduler's contract); needs no key
        if constexpr (P::has_cmux) {
            std::vector<CmuxDesc> cm;
            cm.reserve(n_cmux);
            for (size_t i = 0; i < n; i++)
                if (g[i].op == CUFHE_AMD_TL_CMUX) cm.push_back({g[i].in0, g[i].in1, g[i].out, (const double*)g[i].in2});
            CmuxDesc* dcm;
            if (int rc = upload_descs(s, sc, cm, &dcm)) return rc;
            if (int rc = p.cmux(st, dcm, cm.size())) return rc;
        }
        if (n_cmux + n_cb == n) return 0;
    }
    if (n_cmuxr) {     // ... and its rotating CMUX calls (cufhe_amd_enqueue_cmux_rotate): in0 = c, in2 = the selector, the exponent in the op id
        if constexpr (P::packed_rom) {
            std::vector<CmuxRotDesc> cr;
            cr.reserve(n_cmuxr);
            for (size_t i = 0; i < n; i++)
                if (is_cmux_rotate(g[i].op))
                    cr.push_back({g[i].in0, g[i].out, (const double*)g[i].in2, (uint32_t)(g[i].op - CUFHE_AMD_TL_CMUX_ROTATE(0)), 0u});
            CmuxRotDesc* dcr;
            if (int rc = upload_descs(s, sc, cr, &dcr)) return rc;
            if (int rc = p.cmux_rotate(st, dcr, cr.size())) return rc;
        }
        if (n_cmux + n_cmuxr + n_cb == n) return 0;
    }
    uint32_t *t1 = nullptr, *t0 = nullptr, *dump = nullptr;
    if (n_se) if (int rc = sc.alloc((void**)&t1, n_se * P::mid_words * 4)) return rc;
    if (n_t0) if (int rc = sc.alloc((void**)&t0, n_t0 * P::lvl0_words * 4)) return rc;
    if (n_rot) if (int rc = sc.alloc((void**)&dump, n_rot * tw * 4)) return rc;
    std::vector<LinDesc> se, sei, ks, rot, scat;
    size_t i_se = 0, i_t0 = 0, i_rot = 0;
    for (size_t i = 0; i < n; i++) {
        if (g[i].op == CUFHE_AMD_TL_CMUX || g[i].op == CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP || is_cmux_rotate(g[i].op)) continue;
        if (is_seiks_at(g[i].op)) {       // extraction at the id's index (the descriptor's pad), then the level's one key-switch launch
            uint32_t* a = t1 + i_se++ * P::mid_words;
            sei.push_back({g[i].in0, g[i].in0, a, 1, 0, 0u, (uint32_t)(g[i].op - CUFHE_AMD_TL_SEIKS_AT(0))});
            ks.push_back({a, a, g[i].out, 1, 0, 0u, 0u});
            continue;
        }
        if (g[i].op == CUFHE_AMD_TL_BOOTSTRAP) {
            rot.push_back({g[i].in0, g[i].in0, nullptr, 1, 0, 0u, 0u});
        } else {
            uint32_t* a = t1 + i_se++ * P::mid_words;
            se.push_back({g[i].in0, g[i].in0, a, 1, 0, 0u, 0u});
            if (g[i].op == CUFHE_AMD_TL_SEIKS) {
                ks.push_back({a, a, g[i].out, 1, 0, 0u, 0u});
                continue;
            }
            uint32_t* b = t0 + i_t0++ * P::lvl0_words;
            ks.push_back({a, a, b, 1, 0, 0u, 0u});
            rot.push_back({b, b, nullptr, 1, 0, 0u, 0u});
        }
        uint32_t* d = dump + i_rot++ * tw;
        scat.push_back({d, d, g[i].out, 1, 0, 0u, 0u});
    }
    LinDesc *dse, *dsei, *dks, *drot, *dscat;
    if (int rc = upload_descs(s, sc, se, &dse)) return rc;
    if (int rc = upload_descs(s, sc, sei, &dsei)) return rc;
    if (int rc = upload_descs(s, sc, ks, &dks)) return rc;
    if (int rc = upload_descs(s, sc, rot, &drot)) return rc;
    if (int rc = upload_descs(s, sc, scat, &dscat)) return rc;
    if (!se.empty()) {
        hipLaunchKernelGGL(P::se_kernel, dim3((unsigned)(se.size() < 2048 ? se.size() : 2048)), dim3(256), 0, st, dse, (int)se.size());
        HIP_TRY(hipGetLastError());
    }
    if constexpr (P::packed_rom) {
        if (!sei.empty()) {
            hipLaunchKernelGGL(sample_extract_index_desc_kernel, dim3((unsigned)(sei.size() < 2048 ? sei.size() : 2048)), dim3(256), 0, st, dsei, (int)sei.size());
            HIP_TRY(hipGetLastError());
        }
    }
    if (int rc = p.keyswitch(st, dks, ks.size())) return rc;
    if (int rc = p.rotate(st, drot, rot.size(), P::n, dump)) return rc;
    return launch_lincomb(st, dscat, scat.size(), (int)tw);
}

// The hand-scheduled kernels (the default path)
struct BasePath {
    using RotD = LinDesc;
    using KsD = LinDesc;
    using Mid = uint32_t;
    static constexpr int lvl0_words = kLvl0Words, mid_words = kLvl1Words, n = kLvl0N;
    static constexpr uint32_t ks_mu = kMu;
    static constexpr bool lvl1_gates = true, has_cmux = true, packed_rom = true, rotate_takes_tv_rows = false;
    static constexpr opreg::Path path = opreg::Path::Default;
    static constexpr int set_index = -1;
    static constexpr uint32_t pad(int row, int s) { return make_pad(row, s); }
    static constexpr size_t trlwe_words = 2 * kN;
    static constexpr auto se_kernel = sample_extract_desc_kernel;
    DeviceState& s;
    int ready() const { return s.keys_ready ? 0 : fail(-3, "Initialize(ek) has not been called for this device"); }
    int rotate(hipStream_t st, const LinDesc* d, size_t count, int steps, uint32_t* dump) const { return launch_blind_rotate(s, st, d, count, steps, dump, nullptr); }
    int keyswitch(hipStream_t st, const LinDesc* d, size_t count) const { return launch_keyswitch(s, st, d, count); }
    // one wave per descriptor, kNttWavesPerBlock of them beside the workgroup's copy of the tables: both CMUX kernels
    template <class Desc>
    int launch_cmux(void (*kernel)(const Desc*, int, const NttTables*), hipStream_t st, const Desc* d, size_t count) const
    {
        const unsigned blocks = (unsigned)((count + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, st, d, (int)count, s.tables);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    int cmux(hipStream_t st, const CmuxDesc* d, size_t count) const { return launch_cmux(cmux_desc_kernel, st, d, count); }
    int cmux_rotate(hipStream_t st, const CmuxRotDesc* d, size_t count) const { return launch_cmux(cmux_rotate_desc_kernel, st, d, count); }
};
static_assert([] { for (int k = 0; k < kMaxUserGates; k++) if (BasePath::pad(k, 0) != (uint32_t)(opreg::kUserOps.id(k) - CUFHE_AMD_USER_OP_BASE) + 1) return false; return true; }(),
              "a single-output definition's pad is LinDesc::pad's row + 1: (op - CUFHE_AMD_USER_OP_BASE) + 1 for its one id");

template <class GetGate>
int run_gates(int device, void* stream, int level, size_t count, GetGate get)
{
    // user ops are refused before any device work when they are not defined or the path they would take does not run them
    const opreg::Route route = opreg::route_of_options(g_param_set, g_lvl0_ring, level);
    if (int rc = refuse(opreg::admit_list(g_ops, count, [&](size_t g) { return get(g).op; }, route, opreg::Entry::List, nullptr))) return rc;
    if (level == 0 && g_lvl0_ring == 2048) return run_gates_lvl2(device, stream, count, get);
    if ((level == 0 || level == 1) && g_param_set >= 0) return run_gates_ps((int)g_param_set, device, stream, level, count, get);
    if (int rc = use_device(device)) return rc;
    return lower_gates(BasePath{g_dev[device]}, (hipStream_t)stream, level, count, get);
}

int run_trlwe_ops(int device, void* stream, const GateRef* g, size_t n)
{
    if (g_param_set >= 0) return run_trlwe_ops_ps((int)g_param_set, device, stream, g, n);
    if (int rc = use_device(device)) return rc;
    return lower_trlwe_ops(BasePath{g_dev[device]}, (hipStream_t)stream, g, n);
}

// The direct batch entry points (cufhe_amd_{,ps_,lvl2_}blind_rotate_batch / keyswitch_batch): descriptor g = make(g) for each
// ciphertext, uploaded through the stream's workspace, then one call of `launch` on the device copy
template <class Make, class Launch>
int direct_batch(DeviceState& s, hipStream_t st, size_t count, Make make, Launch launch)
{
    using Desc = decltype(make(size_t{0}));
    std::vector<Desc> h(count);
    for (size_t g = 0; g < count; g++) h[g] = make(g);
    Scratch sc;
    if (int rc = open_scratch(s, st, count * sizeof(Desc) + 4096, &sc)) return rc;
    Desc* d;
    if (int rc = upload_descs(s, sc, h, &d)) return rc;
    return launch(d);
}

// The TRLWE-level batch entry points (cufhe_amd_refresh_batch / sample_extract*_keyswitch_batch / cmux*_batch, cufhe_amd_ps_cmux_batch):
// item g is the TRLWE-level operation make(g), the batch one level of lower_trlwe_ops on `path` -- what the scheduler launches for it
template <class P, class Make>
int trlwe_batch(const P& path, hipStream_t st, size_t count, Make make)
{
    std::vector<GateRef> refs(count);
    for (size_t g = 0; g < count; g++) refs[g] = make(g);
    return lower_trlwe_ops(path, st, refs.data(), count);
}

// A device allocation of an Initialize call (through init_malloc, on the current device): freed on that device when the owner goes
// out of scope, unless release() has handed it over first -- a failure on the way leaves nothing allocated
template <class T>
struct DevPtr {
    T* p = nullptr;
    int phys = 0;
    DevPtr() = default;
    DevPtr(const DevPtr&) = delete;
    DevPtr& operator=(const DevPtr&) = delete;
    hipError_t alloc(size_t n)
    {
        if (hipError_t e = hipGetDevice(&phys)) return e;
        return init_malloc((void**)&p, n * sizeof(T));
    }
    T* release() { T* r = p; p = nullptr; return r; }
    ~DevPtr()
    {
        if (!p) return;
        (void)hipSetDevice(phys);
        (void)hipFree(p);
    }
};

// A key-switching key of `rows` rows of row_words words, uploaded with every row padded to row_pad words (zeros) for the
// shared-table key switch (keyswitch_kernel)
int upload_ksk_padded(DevPtr<uint32_t>& d, const uint32_t* ksk, size_t rows, size_t row_words, size_t row_pad)
{
    HIP_TRY(d.alloc(rows * row_pad));
    HIP_TRY(hipMemset(d.p, 0, rows * row_pad * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy2D(d.p, row_pad * sizeof(uint32_t), ksk, row_words * sizeof(uint32_t), row_words * sizeof(uint32_t), rows,
                        hipMemcpyHostToDevice));
    return 0;
}
// The padded key in matrix form for keyswitch_mm_kernel (42 MB more per device).  A device without room for it keeps the other
// kernels at every count: *out stays null and that is no error.
void build_ksk_matrix(const uint32_t* ksk_padded, ksmm_v4i** out)
{
    *out = nullptr;
    ksmm_v4i* p = nullptr;
    if (hipMalloc((void**)&p, kKsMmKeyBytes) != hipSuccess) { (void)hipGetLastError(); return; }
    hipLaunchKernelGGL(ks_mm_key_kernel, dim3(KsShapeDefault::kn, kKsMmColumns / 256), dim3(256), 0, 0, ksk_padded, p);
    if (hipGetLastError() != hipSuccess) { (void)hipFree(p); return; }
    *out = p;
}


// A new definition of `table` (the caller holds g_mu): every device must be ready(i), else -3 with `not_ready`; the table must have
// room, else `full`.  If it `writes`, write_row(i, k) then puts the definition's test vector into row k of device i's table (device i is
// current), synchronously like the key replicas: no launch reads the row before its id exists; else no device is touched.
template <class Table, class Def, class Ready, class WriteRow>
int define_op(Table& table, const Def& def, Ready ready, const char* not_ready, const char* full, bool writes, WriteRow write_row, int* op)
{
    for (int i = 0; i < g_gpu_num; i++)
        if (!ready(i)) return fail(-3, not_ready);
    const int k = table.next_free();
    if (k < 0) return fail(-1, full);
    for (int i = 0; writes && i < g_gpu_num; i++) {
        HIP_TRY(hipSetDevice(phys_device(i)));
        if (int rc = write_row(i, k)) return rc;
    }
    *op = table.publish(k, def);
    return 0;
}
// row k of a table of `rows` rows of `words` words that is allocated when its first row is written
template <class T>
int write_tv_row(T** table, int rows, size_t words, int k, const T* test_vector)
{
    if (!*table) {
        DevPtr<T> t;
        HIP_TRY(t.alloc((size_t)rows * words));
        *table = t.release();
    }
    HIP_TRY(hipMemcpy(*table + (size_t)k * words, test_vector, words * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
UserGate make_user_gate(const int32_t coeffs[3], uint32_t offset, bool tv, int s) { return UserGate{{coeffs[0], coeffs[1], coeffs[2]}, offset, tv, 1 << s, s}; }

// a user gate of the default path with nout = 2^s outputs (1: cufhe_amd_define_gate); the caller holds g_mu
int define_user_gate(const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector, int s, int* op)
{
    if (!coeffs || !op) return fail(-1, "null pointer");
    if (coeffs[0] == 0) return fail(-1, "user gate: c0 must not be 0");
    if (g_param_set >= 0) return fail(-1, "user gates run on the default path only: not while \"param_set\" is active");
    return define_op(g_ops.user, make_user_gate(coeffs, offset, test_vector != nullptr, s), [](int i) { return g_dev[i].keys_ready; },
                     "Initialize(ek) has not been called for every device", "user gate table full (CUFHE_AMD_MAX_USER_GATES definitions until CleanUp)",
                     test_vector != nullptr, [&](int i, int k) { return write_tv_row(&g_dev[i].tvs, kMaxUserGates, kN, k, test_vector); }, op);
}
}  // namespace

#include "sched_hip.inc.h"
#include "lvl2.inc.h"
#include "cb.inc.h"
#include "pack.inc.h"
#include "lut.inc.h"
#include "paramsets.inc.h"

extern "C" {

const char* cufhe_amd_last_error(void) { return g_err.c_str(); }

int cufhe_amd_get_params(cufhe_amd_params* p)
{
    if (!p) return fail(-1, "null");
    p->n = kLvl0N; p->N = kN; p->nbit = kNbit; p->k = 1; p->l = kL; p->Bgbit = kBgbit;
    p->t = kKsT; p->basebit = kKsBasebit; p->mu = kMu;
    p->lvl0_words = kLvl0Words; p->lvl1_words = kLvl1Words;
    p->bk_words = (uint64_t)kLvl0N * kBkStepDoubles;
    p->ksk_words = (uint64_t)kN * kKsT * kKsNumBase * kKsRowWords;
    p->bk_ntt_bytes = (uint64_t)kLvl0N * kBkStepDoubles * sizeof(double);
    return 0;
}

int cufhe_amd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cufhe_amd_device_identity(int device, char* buf, size_t len)
{
    if (int rc = check_device(device)) return rc;
    if (!buf || len < 2) return fail(-1, "null / short buffer");
    const int phys = phys_device(device);
    char pci[64] = "?";
    HIP_TRY(hipDeviceGetPCIBusId(pci, (int)sizeof pci, phys));
    hipUUID uuid;
    memset(&uuid, 0, sizeof uuid);
    char hex[2 * sizeof(uuid.bytes) + 1] = "";
    if (hipDeviceGetUuid(&uuid, phys) == hipSuccess)
        for (size_t i = 0; i < sizeof(uuid.bytes); i++) snprintf(hex + 2 * i, 3, "%02x", (unsigned char)uuid.bytes[i]);
    (void)hipGetLastError();
    // CPUs close to the device (what the launch worker of this device is pinned to, "sched_affinity")
    std::string cpus = device_local_cpulist(phys);
    snprintf(buf, len, "pci=%s uuid=%s hip_device=%d local_cpus=%s", pci, hex[0] ? hex : "?", phys, cpus.empty() ? "?" : cpus.c_str());
    return 0;
}

int cufhe_amd_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes)
{
    if (int rc = use_device(device)) return rc;
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

int cufhe_amd_device_cus(int device)
{
    if (int rc = check_device(device)) return rc;
    if (g_cus_override > 0) return (int)g_cus_override;
    int n = 0;
    HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, phys_device(device)));
    return n;
}

int cufhe_amd_set_gpu_num(int gpu_num)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (gpu_num < 1) return fail(-1, "gpu_num must be >= 1");
    if (gpu_num > kMaxLogicalDevices) return fail(-1, "gpu_num exceeds the 64 logical devices this build is sized for");
    for (auto& d : g_dev)
        if (d.ntt_ready || d.keys_ready || d.tables2) return fail(-1, "SetGPUNum after Initialize: call CleanUp first");
    int have = cufhe_amd_device_count();
    g_phys_count = have;
    if (have < 1) return fail(-1, "no GPU visible");
    if (!g_share_devices && gpu_num + g_device_base > have) return fail(-1, "gpu_num (plus device_base) exceeds the visible device count");
    if (gpu_num != g_gpu_num) {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        sched_retire_generation();
    }
    g_gpu_num = gpu_num;
    g_dev.clear();
    g_dev.resize(gpu_num);
    return 0;
}
int cufhe_amd_get_gpu_num(void) { return g_gpu_num; }

int cufhe_amd_initialize_ntt(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < g_gpu_num; i++)
        if (int rc = ensure_ntt(i)) return rc;
    return 0;
}

int cufhe_amd_initialize(const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const size_t want_bk = (size_t)kLvl0N * kBkStepDoubles;
    const size_t want_ksk = (size_t)kN * kKsT * kKsNumBase * kKsRowWords;
    if (!bk || !ksk) return fail(-1, "null key pointer");
    if (bk_words != want_bk) return fail(-1, "bootstrapping key has the wrong size for this parameter set");
    if (ksk_words != want_ksk) return fail(-1, "key-switching key has the wrong size for this parameter set");
    // Build first, swap last: the new keys of EVERY device are allocated and converted beside whatever is loaded; only when all of that
    // has succeeded do they replace the old ones.  A failure on the way (a full device: 104 MB per replica, and 42 MB for the key switch's matrix form, which may be missing) frees what this call
    // allocated and leaves every device with the keys -- and the results -- it had.
    struct Built { DevPtr<double> bk_ntt; DevPtr<uint32_t> ksk, d_bk; };
    std::vector<Built> built((size_t)g_gpu_num);      // the torus-domain staging copies d_bk are freed on every return
    for (int i = 0; i < g_gpu_num; i++) {
        if (int rc = ensure_ntt(i)) return rc;
        DeviceState& s = g_dev[i];
        Built& b = built[(size_t)i];
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(b.bk_ntt.alloc(want_bk));
        // KeySwitchingKeyToDevice (src/keyswitch_gpu.cu:6-16), rows padded 631 -> 640 words
        if (int rc = upload_ksk_padded(b.ksk, ksk, want_ksk / kKsRowWords, kKsRowWords, kKsRowPad)) return rc;
        HIP_TRY(b.d_bk.alloc(want_bk));
        HIP_TRY(hipMemcpy(b.d_bk.p, bk, want_bk * sizeof(uint32_t), hipMemcpyHostToDevice));
        const size_t polys = want_bk / kN;
        const unsigned blocks = (unsigned)((polys + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
        hipLaunchKernelGGL(bk_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, 0, b.bk_ntt.p, b.d_bk.p,
                           polys, s.tables, n_inverse(kN));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());        // also: nothing on this device still reads the keys that are about to go
    }
    for (int i = 0; i < g_gpu_num; i++) {
        DeviceState& s = g_dev[i];
        (void)hipSetDevice(phys_device(i));
        if (s.keys_ready) { (void)hipFree(s.bk_ntt); (void)hipFree(s.ksk); }
        if (s.ksk_mm) { (void)hipFree(s.ksk_mm); s.ksk_mm = nullptr; }
        s.bk_ntt = built[(size_t)i].bk_ntt.release();
        s.ksk = built[(size_t)i].ksk.release();
        // the matrix form is optional (a device without 42 MB to spare keeps the other key-switch kernels), so it cannot fail the swap
        build_ksk_matrix(s.ksk, &s.ksk_mm);
        if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); if (s.ksk_mm) (void)hipFree(s.ksk_mm); s.ksk_mm = nullptr; }
        s.keys_ready = true;
    }
    return 0;
}

int cufhe_amd_cleanup(void)
{
    {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        sched_quiesce();
    }
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < g_gpu_num; i++) {
        DeviceState& s = g_dev[i];
        if (!s.ntt_ready && !s.keys_ready && !s.tables2) continue;
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(hipDeviceSynchronize());
        for (auto* v : {&s.br_events, &s.ks_events}) {
            for (auto& e : *v) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
            v->clear();
        }
        if (s.keys_ready) { HIP_TRY(hipFree(s.bk_ntt)); HIP_TRY(hipFree(s.ksk)); }
        if (s.ksk_mm) { HIP_TRY(hipFree(s.ksk_mm)); s.ksk_mm = nullptr; }
        if (s.tvs) { HIP_TRY(hipFree(s.tvs)); s.tvs = nullptr; }
        if (s.tvs2) { HIP_TRY(hipFree(s.tvs2)); s.tvs2 = nullptr; }
        ps_release(i);
        if (s.keys2_ready) { if (s.bk2_ntt) HIP_TRY(hipFree(s.bk2_ntt)); HIP_TRY(hipFree(s.bk2q_ntt)); HIP_TRY(hipFree(s.ksk2)); }
        if (s.cb_pksk) { HIP_TRY(hipFree(s.cb_pksk)); s.cb_pksk = nullptr; }
        if (s.pack_key) { HIP_TRY(hipFree(s.pack_key)); s.pack_key = nullptr; }
        if (s.tables2) HIP_TRY(hipFree(s.tables2));
        if (s.tables2q) HIP_TRY(hipFree(s.tables2q));
        s.keys2_ready = false;
        s.br2_lds_opt_in = false;
        s.br2q_lds_opt_in = false;
        s.ks2_lds_opt_in = false;
        s.tables2 = nullptr; s.tables2q = nullptr; s.bk2_ntt = nullptr; s.bk2q_ntt = nullptr; s.ksk2 = nullptr;
        if (s.ntt_ready) { HIP_TRY(hipFree(s.tables)); HIP_TRY(hipFree(s.tables_r4)); HIP_TRY(hipFree(s.tables512)); }
        if (s.fault_host) { (void)hipHostFree(s.fault_host); s.fault_host = nullptr; s.fault = nullptr; }   // the fault, if any, ends with the keys
        for (auto& b : s.staging) { (void)hipEventDestroy(b.done); (void)hipHostFree(b.host); }
        s.staging.clear();
        for (auto& kv : s.workspaces) { (void)hipFree(kv.second.base); (void)hipFree(kv.second.ks_digits); }
        s.workspaces.clear();
        s.ntt_ready = s.keys_ready = false;
        s.br_lds_opt_in = false;
        s.ks_lds_opt_in = false;
        s.tables = nullptr; s.tables_r4 = nullptr; s.tables512 = nullptr; s.bk_ntt = nullptr; s.ksk = nullptr;
        s.prof = cufhe_amd_profile{};
    }
    lvl2_release_host_key();
    g_ops.user.clear(); g_ops.lvl2.clear(); g_ops.ps.clear();
    return 0;
}

int cufhe_amd_synchronize(void)
{
    {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        if (int rc = sched_synchronize_all()) return rc;
    }
    for (int i = 0; i < g_gpu_num; i++) {
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(hipDeviceSynchronize());
        if (int rc = device_fault(i)) return rc;
    }
    return 0;
}

int cufhe_amd_stream_create(int device, void** stream)
{
    if (int rc = use_device(device)) return rc;
    hipStream_t st;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = (void*)st;
    return 0;
}
int cufhe_amd_stream_destroy(int device, void* stream)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    {
        std::lock_guard<std::mutex> lk(s.staging_mu);
        auto it = s.workspaces.find((hipStream_t)stream);
        if (it != s.workspaces.end()) {
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            (void)hipFree(it->second.base);
            (void)hipFree(it->second.ks_digits);
            s.workspaces.erase(it);
        }
    }
    if (int rc = linear_forget_stream(device, (hipStream_t)stream)) return rc;      // the temporary of cufhe_amd_linear_gate_batch
    {
        std::lock_guard<std::mutex> lk(g_sched_mu);
        if (g_scheduler && device < g_scheduler->gpu_num()) {
            (void)g_scheduler->dev(device).retire_external_stream(stream);      // no queued launch may still name the raw handle
            g_scheduler->dev(device).forget_stream(stream);
            if (device < (int)g_sched_backends.size()) g_sched_backends[device]->forget_caller_stream(stream);
        }
    }
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return device_fault(device);      // the workspace release above may have waited for the stream
}
int cufhe_amd_stream_query(int device, void* stream)
{
    if (int rc = use_device(device)) return rc;
    if (sched_active()) {
        int q = cufhe_amd_sched_stream_query(device, stream);
        if (q <= 0) return q;
    }
    hipError_t e = hipStreamQuery((hipStream_t)stream);
    if (e == hipSuccess) {
        if (int rc = device_fault(device)) return rc;
        return 1;
    }
    if (e == hipErrorNotReady) return 0;
    return fail(-2, std::string("hipStreamQuery: ") + hipGetErrorString(e));
}
int cufhe_amd_stream_synchronize(int device, void* stream)
{
    if (int rc = use_device(device)) return rc;
    if (sched_active()) {       // what was recorded on the stream through the per-gate API: launched, complete, delivered to the tlwehosts
        std::lock_guard<std::mutex> lk(g_sched_mu);
        if (int rc = g_scheduler->dev(device).stream_synchronize(stream)) return sched_error(g_scheduler->dev(device), rc);
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return device_fault(device);
}

int cufhe_amd_malloc(int device, size_t bytes, void** dptr)
{
    if (int rc = use_device(device)) return rc;
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 16));
    return 0;
}
int cufhe_amd_free(int device, void* dptr)
{
    if (int rc = use_device(device)) return rc;
    HIP_TRY(hipFree(dptr));
    return 0;
}
int cufhe_amd_host_register(void* hptr, size_t bytes)
{
    HIP_TRY(hipHostRegister(hptr, bytes, hipHostRegisterDefault));
    return 0;
}
int cufhe_amd_host_unregister(void* hptr)
{
    HIP_TRY(hipHostUnregister(hptr));
    return 0;
}
int cufhe_amd_memcpy_h2d(int device, void* stream, void* dptr, const void* hptr, size_t bytes)
{
    if (int rc = use_device(device)) return rc;
    HIP_TRY(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}
int cufhe_amd_memcpy_d2h(int device, void* stream, void* hptr, const void* dptr, size_t bytes)
{
    if (int rc = use_device(device)) return rc;
    HIP_TRY(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}

int cufhe_amd_gate(int device, void* stream, int op, int level, uint32_t* out, const uint32_t* in0,
                   const uint32_t* in1, const uint32_t* in2)
{
    return run_gates(device, stream, level, 1, [&](size_t) { return GateRef{op, out, in0, in1, in2}; });
}

int cufhe_amd_gate_batch(int device, void* stream, int level, size_t count, const int32_t* ops, int ops_stride,
                         uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                         size_t stride_words)
{
    if (!ops) return fail(-1, "null ops");
    // the kernels move the ciphertext size of the set the entry point runs on ("param_set" / "lvl0_ring"): a smaller stride would make
    // neighbouring ciphertexts overlap and the last one run past the buffer
    if (count > 1 && (level == 0 || level == 1) && (long)stride_words < (long)cufhe_amd_ctxt_words(level))
        return fail(-1, "stride_words is smaller than a ciphertext of the active parameter set (cufhe_amd_ctxt_words)");
    return run_gates(device, stream, level, count, [&](size_t g) {
        return GateRef{ops[g * (size_t)ops_stride], out + g * stride_words, in0 ? in0 + g * stride_words : nullptr,
                       in1 ? in1 + g * stride_words : nullptr, in2 ? in2 + g * stride_words : nullptr};
    });
}

int cufhe_amd_gate_list(int device, void* stream, int level, size_t count, const int32_t* ops,
                        uint32_t* const* outs, const uint32_t* const* in0s, const uint32_t* const* in1s,
                        const uint32_t* const* in2s)
{
    if (!ops || !outs || !in0s) return fail(-1, "null array");
    return run_gates(device, stream, level, count, [&](size_t g) {
        return GateRef{ops[g], outs[g], in0s[g], in1s ? in1s[g] : nullptr, in2s ? in2s[g] : nullptr};
    });
}

int cufhe_amd_define_gate(const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return define_user_gate(coeffs, offset, test_vector, 0, op);
}

int cufhe_amd_define_gate_multi(const int32_t coeffs[3], uint32_t offset, int nout, const uint32_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (nout != 2 && nout != 4 && nout != 8) return fail(-1, "multi-output user gate: nout must be 2, 4 or 8");
    if (!test_vector) return fail(-1, "multi-output user gate: the test vector is required");
    return define_user_gate(coeffs, offset, test_vector, nout == 2 ? 1 : nout == 4 ? 2 : 3, op);
}

int cufhe_amd_test_vector(const uint32_t* values, int p, uint32_t* tv)
{
    if (!values || !tv) return fail(-1, "null pointer");
    if (p < 2 || p > kN / 2 || (p & (p - 1))) return fail(-1, "p must be a power of two in [2, N/2]");
    // coefficient j lies in the box of m = round(j p / N); the top half-box (m = p) is the wrap of m = 0's lower half: -values[0]
    const int box = kN / p;
    for (int j = 0; j < kN; j++) {
        const int m = (j + box / 2) / box;
        tv[j] = m == p ? 0u - values[0] : values[m];
    }
    return 0;
}

int cufhe_amd_test_vector_multi(const uint32_t* values, int p, int nout, uint32_t* tv)
{
    if (!values || !tv) return fail(-1, "null pointer");
    if (nout != 1 && nout != 2 && nout != 4 && nout != 8) return fail(-1, "nout must be 1, 2, 4 or 8");
    if (p < 2 || (p & (p - 1)) || p * nout > kN / 2) return fail(-1, "p must be a power of two >= 2 with p nout <= N/2");
    // TV[nout q + j] = values[j][m], m the box of position nout q under cufhe_amd_test_vector's boxes (the top half-box: -values[j][0])
    const int box = kN / p;
    for (int q = 0; q < kN / nout; q++) {
        const int m = (nout * q + box / 2) / box;
        for (int j = 0; j < nout; j++) {
            const uint32_t* v = values + (size_t)j * p;
            tv[nout * q + j] = m == p ? 0u - v[0] : v[m];
        }
    }
    return 0;
}

int cufhe_amd_bootstrap_batch(int device, void* stream, size_t count, uint32_t* out, const uint32_t* in)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (!out || !in) return fail(-1, "null pointer");
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc;
    if (int rc = open_scratch(s, st, count * (kLvl1Words * sizeof(uint32_t) + 2 * sizeof(LinDesc)) + 8192, &sc)) return rc;
    uint32_t* t1;
    if (int rc = sc.alloc((void**)&t1, count * kLvl1Words * sizeof(uint32_t))) return rc;
    std::vector<LinDesc> rot(count), ks(count);
    for (size_t g = 0; g < count; g++) {
        rot[g] = {in + g * kLvl0Words, in + g * kLvl0Words, t1 + g * kLvl1Words, 1, 0, 0u, 0u};
        ks[g] = {t1 + g * kLvl1Words, t1 + g * kLvl1Words, out + g * kLvl0Words, 1, 0, 0u, 0u};
    }
    LinDesc *drot, *dks;
    if (int rc = upload_descs(s, sc, rot, &drot)) return rc;
    if (int rc = upload_descs(s, sc, ks, &dks)) return rc;
    if (int rc = launch_blind_rotate(s, st, drot, count, kLvl0N, nullptr, nullptr)) return rc;
    return launch_keyswitch(s, st, dks, count);
}

int cufhe_amd_blind_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint32_t* acc, int steps)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (!tlwe0 || !acc) return fail(-1, "null pointer");
    if (steps < 0 || steps > kLvl0N) steps = kLvl0N;
    hipStream_t st = (hipStream_t)stream;
    return direct_batch(s, st, count, [&](size_t g) { return LinDesc{tlwe0 + g * kLvl0Words, tlwe0 + g * kLvl0Words, nullptr, 1, 0, 0u, 0u}; },
                        [&](const LinDesc* d) { return launch_blind_rotate(s, st, d, count, steps, acc, nullptr); });
}

int cufhe_amd_keyswitch_batch(int device, void* stream, size_t count, const uint32_t* tlwe1, uint32_t* tlwe0)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (!tlwe0 || !tlwe1) return fail(-1, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    return direct_batch(s, st, count, [&](size_t g) { return LinDesc{tlwe1 + g * kLvl1Words, tlwe1 + g * kLvl1Words, tlwe0 + g * kLvl0Words, 1, 0, 0u, 0u}; },
                        [&](const LinDesc* d) { return launch_keyswitch(s, st, d, count); });
}

int cufhe_amd_trgsw_to_ntt_batch(int device, void* stream, size_t count, const uint32_t* trgsw, double* trgsw_ntt)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (!trgsw || !trgsw_ntt) return fail(-1, "null pointer");
    if (count == 0) return 0;
    const size_t polys = count * kBkPolysPerStep;
    const unsigned blocks = (unsigned)((polys + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(bk_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, (hipStream_t)stream, trgsw_ntt,
                       trgsw, polys, g_dev[device].tables, n_inverse(kN));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cufhe_amd_trgsw_to_ntt_host(int device, void* stream, const uint32_t* trgsw_host, double* trgsw_ntt_host)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (!trgsw_host || !trgsw_ntt_host) return fail(-1, "null pointer");
    if (g_param_set >= 0) return ps_trgsw_to_ntt_host((int)g_param_set, device, stream, trgsw_host, trgsw_ntt_host);     // the active set's sizes and limbs
    DeviceState& s = g_dev[device];
    hipStream_t st = (hipStream_t)stream;
    // torus words in, NTT-domain doubles out: both staged in the stream's grow-only workspace and in recycled pinned
    // blocks, nothing is allocated or freed per call (the reference's TRGSW2NTT is allocation-free as well,
    // src/bootstrap_gpu.cu:75-94)
    constexpr size_t in_bytes = kBkStepDoubles * sizeof(uint32_t), out_bytes = kBkStepDoubles * sizeof(double);
    Scratch sc;
    if (int rc = open_scratch(s, st, in_bytes + out_bytes + 4096, &sc)) return rc;
    uint32_t* d_in;
    double* d_out;
    if (int rc = sc.alloc((void**)&d_in, in_bytes)) return rc;
    if (int rc = sc.alloc((void**)&d_out, out_bytes)) return rc;
    PinnedBlock* blk = nullptr;
    if (int rc = acquire_staging(s, in_bytes + out_bytes, &blk)) return rc;
    StagingOwner owner{s, blk};          // releases `held`; hands the block back if a call below fails before the event is recorded
    staging_hold(s, blk, true);          // the host reads the result out of the block after the stream has finished with it
    memcpy(blk->host, trgsw_host, in_bytes);
    HIP_TRY(hipMemcpyAsync(d_in, blk->host, in_bytes, hipMemcpyHostToDevice, st));
    const unsigned blocks = (unsigned)((kBkPolysPerStep + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(bk_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, st, d_out, d_in, (size_t)kBkPolysPerStep,
                       s.tables, n_inverse(kN));
    HIP_TRY(hipGetLastError());
    char* pin_out = (char*)blk->host + in_bytes;
    HIP_TRY(hipMemcpyAsync(pin_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    if (int rc = staging_done_after(s, blk, st)) return rc;
    owner.recorded();
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(trgsw_ntt_host, pin_out, out_bytes);
    return device_fault(device);
}

int cufhe_amd_cmux_batch(int device, void* stream, size_t count, const double* trgsw_ntt, const uint32_t* c1,
                         const uint32_t* c0, uint32_t* res)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (!trgsw_ntt || !c1 || !c0 || !res) return fail(-1, "null pointer");
    if (count == 0) return 0;
    return trlwe_batch(BasePath{g_dev[device]}, (hipStream_t)stream, count, [&](size_t g) {
        return GateRef{CUFHE_AMD_TL_CMUX, res + g * 2 * kN, c1 + g * 2 * kN, c0 + g * 2 * kN, (const uint32_t*)(trgsw_ntt + g * kBkStepDoubles)};
    });
}

int cufhe_amd_sample_extract_keyswitch_batch(int device, void* stream, size_t count, const uint32_t* trlwe, uint32_t* tlwe0)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (!trlwe || !tlwe0) return fail(-1, "null pointer");
    if (count == 0) return 0;
    return trlwe_batch(BasePath{s}, (hipStream_t)stream, count, [&](size_t g) {
        return GateRef{CUFHE_AMD_TL_SEIKS, tlwe0 + g * kLvl0Words, trlwe + g * 2 * kN, nullptr, nullptr};
    });
}

// ---- packed ROM words ----
int cufhe_amd_trlwe_rotate_batch(int device, void* stream, size_t count, const uint32_t* in, const int32_t* exps, uint32_t* out)
{
    if (g_param_set >= 0) return fail_packed_rom_set();
    if (int rc = check_device(device)) return rc;
    if (!in || !exps || !out) return fail(-1, "null pointer");
    // the kernel gathers from `in` while other waves store to `out`: any overlap of the two arrays is refused
    if (count && in < out + count * 2 * kN && out < in + count * 2 * kN) return fail(-1, "trlwe_rotate_batch: out must not overlap in");
    for (size_t g = 0; g < count; g++)
        if (exps[g] < 0 || exps[g] >= 2 * kN) return fail(-1, "trlwe_rotate_batch: exponent outside [0, 2N)");
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    hipStream_t st = (hipStream_t)stream;
    Scratch sc;
    if (int rc = open_scratch(s, st, count * sizeof(int32_t) + 4096, &sc)) return rc;
    int32_t* dexps;
    if (int rc = upload_descs(s, sc, std::vector<int32_t>(exps, exps + count), &dexps)) return rc;
    const unsigned blocks = (unsigned)((count + kRotWavesPerBlock - 1) / kRotWavesPerBlock);
    hipLaunchKernelGGL(trlwe_rotate_kernel, dim3(blocks), dim3(64 * kRotWavesPerBlock), 0, st, out, in, dexps, (int)count);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cufhe_amd_cmux_rotate_batch(int device, void* stream, size_t count, const double* trgsw_ntt, const int32_t* exps,
                                const uint32_t* c, uint32_t* res)
{
    if (g_param_set >= 0) return fail_packed_rom_set();
    if (int rc = check_device(device)) return rc;
    if (!trgsw_ntt || !exps || !c || !res) return fail(-1, "null pointer");
    // a wave reads its whole item before it stores: res == c is the in-place form; a partial overlap would cross items
    if (count && res != c && c < res + count * 2 * kN && res < c + count * 2 * kN)
        return fail(-1, "cmux_rotate_batch: res must be c itself or not overlap it");
    for (size_t g = 0; g < count; g++)
        if (exps[g] < 0 || exps[g] >= 2 * kN) return fail(-1, "cmux_rotate_batch: exponent outside [0, 2N)");
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    // one selector for the launch: every item names the same TRGSW
    return trlwe_batch(BasePath{g_dev[device]}, (hipStream_t)stream, count, [&](size_t g) {
        return GateRef{CUFHE_AMD_TL_CMUX_ROTATE(exps[g]), res + g * 2 * kN, c + g * 2 * kN, nullptr, (const uint32_t*)trgsw_ntt};
    });
}

static int check_extract_index_args(size_t count, const uint32_t* trlwe, const int32_t* src, const int32_t* idx, const uint32_t* out)
{
    if (!trlwe || !idx || !out) return fail(-1, "null pointer");
    if (count > (size_t)INT32_MAX) return fail(-1, "sample_extract_index: count exceeds the index type of src");
    for (size_t g = 0; g < count; g++) {
        if (idx[g] < 0 || idx[g] >= kN) return fail(-1, "sample_extract_index: index outside [0, N)");
        if (src && src[g] < 0) return fail(-1, "sample_extract_index: negative source index");
    }
    return 0;
}

int cufhe_amd_sample_extract_index_batch(int device, void* stream, size_t count, const uint32_t* trlwe, const int32_t* src,
                                         const int32_t* idx, uint32_t* tlwe1)
{
    if (g_param_set >= 0) return fail_packed_rom_set();
    if (int rc = check_device(device)) return rc;
    if (int rc = check_extract_index_args(count, trlwe, src, idx, tlwe1)) return rc;
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return direct_batch(g_dev[device], st, count, [&](size_t g) {
        const uint32_t* in = trlwe + (size_t)(src ? src[g] : g) * 2 * kN;
        return LinDesc{in, in, tlwe1 + g * kLvl1Words, 1, 0, 0u, (uint32_t)idx[g]};
    }, [&](const LinDesc* d) {
        hipLaunchKernelGGL(sample_extract_index_desc_kernel, dim3((unsigned)(count < 2048 ? count : 2048)), dim3(256), 0, st, d, (int)count);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int cufhe_amd_sample_extract_index_keyswitch_batch(int device, void* stream, size_t count, const uint32_t* trlwe, const int32_t* src,
                                                   const int32_t* idx, uint32_t* tlwe0)
{
    if (g_param_set >= 0) return fail_packed_rom_set();
    if (int rc = check_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (int rc = check_extract_index_args(count, trlwe, src, idx, tlwe0)) return rc;
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    return trlwe_batch(BasePath{s}, (hipStream_t)stream, count, [&](size_t g) {
        return GateRef{CUFHE_AMD_TL_SEIKS_AT(idx[g]), tlwe0 + g * kLvl0Words, trlwe + (size_t)(src ? src[g] : g) * 2 * kN, nullptr, nullptr};
    });
}

int cufhe_amd_refresh_batch(int device, void* stream, size_t count, const uint32_t* trlwe_in, uint32_t* trlwe_out)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (!trlwe_in || !trlwe_out) return fail(-1, "null pointer");
    if (count == 0) return 0;
    return trlwe_batch(BasePath{s}, (hipStream_t)stream, count, [&](size_t g) {
        return GateRef{CUFHE_AMD_TL_REFRESH, trlwe_out + g * 2 * kN, trlwe_in + g * 2 * kN, nullptr, nullptr};
    });
}

int cufhe_amd_polymul_batch(int device, void* stream, size_t count, const int32_t* a, const uint32_t* b, uint32_t* res)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (count == 0) return 0;
    const unsigned blocks = (unsigned)((count + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(polymul_kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, (hipStream_t)stream, res, a, b,
                       (int)count, g_dev[device].tables, n_inverse(kN));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cufhe_amd_polymul512_batch(int device, void* stream, size_t count, const int32_t* a, const uint32_t* b, uint32_t* res)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (count == 0) return 0;
    const unsigned blocks = (unsigned)((count + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(polymul512_kernel, dim3(blocks), dim3(kNttThreads), kPoly512LdsBytes, (hipStream_t)stream, res, a, b,
                       (int)count, g_dev[device].tables512 + 2, n_inverse(kH));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cufhe_amd_set_option(const char* key, long value)
{
    if (!key) return fail(-1, "null key");
    if (!strcmp(key, "device_base")) {
        for (auto& d : g_dev)
            if (d.ntt_ready || d.keys_ready || d.tables2) return fail(-1, "device_base must be set before Initialize");
        if (value < 0 || value + g_gpu_num > cufhe_amd_device_count()) return fail(-1, "device_base out of range");
        if (value != g_device_base) {
            std::lock_guard<std::mutex> lk2(g_sched_mu);
            sched_retire_generation();
        }
        g_device_base = (int)value;
        return 0;
    }
    if (!strcmp(key, "sched_streams") || !strcmp(key, "sched_threads")) {
        // structure of the scheduler: takes effect for the next scheduler generation
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        if (value < 0 || value > 64) return fail(-1, "value out of range");
        if (g_scheduler && g_scheduler->live_ctxts()) return fail(-1, "sched_streams / sched_threads must be set before the first ciphertext is created");
        sched_retire_generation();
        (key[6] == 's' ? g_sched_streams : g_sched_threads) = value;
        return 0;
    }
    if (!strcmp(key, "sched_level_gates") || !strcmp(key, "sched_total_gates")) {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        if (value < 1 && !(key[6] == 'l' && value == -1)) return fail(-1, "value out of range (sched_level_gates: -1 = two grid rounds of the device)");
        (key[6] == 'l' ? g_sched_level_gates : g_sched_total_gates) = value;
        sched_apply_settings();
        return 0;
    }
    if (!strcmp(key, "test_fail_alloc")) { g_fail_alloc_countdown = value; return 0; }
    if (!strcmp(key, "cus_override")) {
        if (value < 0 || value > 4096) return fail(-1, "cus_override must be 0 (the device's own CU count) or a CU count");
        g_cus_override = value;
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        sched_apply_settings();        // the scheduler's flush rules are in grid rounds of 8 rotations per CU
        return 0;
    }
    if (!strcmp(key, "sched_idle_gates")) {
        if (value < 1 && value != -1) return fail(-1, "sched_idle_gates must be -1 (one grid round) or a gate count");
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        g_sched_idle_gates = value;
        sched_apply_settings();
        return 0;
    }
    if (!strcmp(key, "sched_copy_threads")) {
        if (value < 1 || value > 16) return fail(-1, "sched_copy_threads must be 1..16");
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        g_sched_copy_threads = value;
        sched_apply_settings();          // takes effect for devices that have not flushed yet (the helpers start with the first large copy)
        return 0;
    }
    if (!strcmp(key, "sched_two_lane")) {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        if (int rc = sched_synchronize_all()) return rc;      // what is recorded was recorded under the old renaming policy
        if (value < 0 || value > 2) return fail(-1, "sched_two_lane must be 0 (never), 1 (by the cost model) or 2 (whenever a flush is eligible)");
        g_sched_two_lane = value;
        sched_apply_settings();
        return 0;
    }
    if (!strcmp(key, "cb_rotations")) {
        // 3: one lvl02 rotation per TRGSW row (constant test vectors); 1: all l rows from one rotation (cb.inc.h)
        if (value != 1 && value != 3) return fail(-1, "cb_rotations must be 3 (one rotation per TRGSW row) or 1 (all rows from one rotation)");
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        if (int rc = sched_synchronize_all()) return rc;      // recorded circuit bootstraps complete in the form they were recorded under
        g_cb_rotations = value;
        return 0;
    }
    if (!strcmp(key, "sched_rename")) {
        std::lock_guard<std::mutex> lk2(g_sched_mu);
        g_sched_rename = value != 0;
        sched_apply_settings();
        return 0;
    }
    if (!strcmp(key, "sched_affinity")) { g_sched_affinity = value != 0; return 0; }
    if (!strcmp(key, "sched_zero_copy")) { g_sched_zero_copy = value != 0; return 0; }
    if (!strcmp(key, "share_devices")) { g_share_devices = value; g_phys_count = cufhe_amd_device_count(); return 0; }
    // the launch-shape options that take any value (launch_plan.h); "ks_slices", "ks_per_wg" and "lvl2_kernel" check theirs below
    static const struct { const char* key; long plan::Tuning::*field; } kPlanOptions[] = {
        {"ll_threshold", &plan::Tuning::ll_threshold},   {"ll2_threshold", &plan::Tuning::ll2_threshold},
        {"half_threshold", &plan::Tuning::half_threshold}, {"tail_split", &plan::Tuning::tail_split},
        {"ks_wg_threshold", &plan::Tuning::ks_wg_threshold}, {"ks_split_threshold", &plan::Tuning::ks_split_threshold},
        {"ps_batch_threshold", &plan::Tuning::ps_batch_threshold}, {"pack_slices", &plan::Tuning::pack_slices},
    };
    for (const auto& o : kPlanOptions)
        if (!strcmp(key, o.key)) { g_tuning.*o.field = value; return 0; }
    if (!strcmp(key, "br_shape")) {
        if (value < 0 || value > 3) return fail(-1, "br_shape must be 0 (rules), 1 (batch kernel), 2 (paired low-latency kernel) or 3 (single)");
        g_br_shape = value;        // of the calling thread
        return 0;
    }
    if (!strcmp(key, "param_set") || !strcmp(key, "lvl0_param_set")) {
        if (value >= 0) {
            cufhe_amd_ps_params p;
            if (int rc = cufhe_amd_ps_get_params((int)value, &p)) return rc;
            // ciphertext device slots are carved for the largest compiled sizes (HipBackend::slot_words), so a set only has to fit them
            if ((int)p.lvl0_words > kLvl0Words || (int)p.lvl1_words > kLvl1Words) return fail(-1, "param_set: the set's ciphertexts exceed the per-gate API's buffers");
        }
        if (value != g_param_set) {
            // recorded gates were sized and routed for the old set: they complete first
            std::lock_guard<std::mutex> lk2(g_sched_mu);
            if (int rc = sched_synchronize_all()) return rc;
        }
        g_param_set = value;
        return 0;
    }
    if (!strcmp(key, "ks_slices")) {
        if (value != -1 && (value < 1 || value > 64 || (value & (value - 1)))) return fail(-1, "ks_slices must be -1 or a power of two 1..64");
        g_tuning.ks_slices = value;
        return 0;
    }
    if (!strcmp(key, "ks_per_wg")) {
        if (value != -1 && (value < 1 || value > 16)) return fail(-1, "ks_per_wg must be -1 or 1..16");
        g_tuning.ks_per_wg = value;
        return 0;
    }
    if (!strcmp(key, "ks_mm_threshold")) {
        if (value < -1) return fail(-1, "ks_mm_threshold must be -1 (the measured rule), 0 (never) or a count of ciphertexts");
        g_tuning.ks_mm_threshold = value;
        return 0;
    }
    if (!strcmp(key, "lvl2_kernel")) {
        if (value < -1 || value > 1) return fail(-1, "lvl2_kernel must be -1 (by cost), 0 (eight half waves) or 1 (four quarter waves)");
        g_tuning.lvl2_kernel = value;
        return 0;
    }
    if (!strcmp(key, "lvl0_ring")) {
        if (value != 1024 && value != 2048) return fail(-1, "lvl0_ring must be 1024 or 2048");
        g_lvl0_ring = value;
        return 0;
    }
    return fail(-1, std::string("unknown option ") + key);
}

int cufhe_amd_profile_enable(int device, int on)
{
    if (int rc = check_device(device)) return rc;
    g_dev[device].profiling = on != 0;
    return 0;
}

int cufhe_amd_probe_clock(int device, double* hz)
{
    if (int rc = use_device(device)) return rc;
    if (!hz) return fail(-1, "null");
    constexpr int kBlocks = 256, kWaves = 8;
    double* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (kBlocks * kWaves + 1) * sizeof(double)));
    std::vector<double> h(kBlocks * kWaves);
    for (int rep = 0; rep < 2; rep++)        // the second launch runs on a chip that is already under load
        hipLaunchKernelGGL(clock_probe_kernel, dim3(kBlocks), dim3(64 * kWaves), 0, 0, d, d + kBlocks * kWaves, 3000);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(-2, std::string("clock probe: ") + hipGetErrorString(e));
    std::sort(h.begin(), h.end());
    *hz = h[h.size() / 2];
    return 0;
}

int cufhe_amd_profile_get(int device, cufhe_amd_profile* out, int reset)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    auto drain = [&](std::vector<EventPair>& v, double& ms, uint64_t& launches, uint64_t& units) -> int {
        for (auto& e : v) {
            HIP_TRY(hipEventSynchronize(e.b));
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, e.a, e.b));
            ms += t; launches += 1; units += e.units;
            (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
        }
        v.clear();
        return 0;
    };
    std::vector<EventPair> br, ks;
    {
        std::lock_guard<std::mutex> lk(s.staging_mu);     // the scheduler's worker thread records launches too
        br.swap(s.br_events);
        ks.swap(s.ks_events);
    }
    if (int rc = drain(br, s.prof.blind_rotate_ms, s.prof.blind_rotate_launches, s.prof.blind_rotations)) return rc;
    if (int rc = drain(ks, s.prof.keyswitch_ms, s.prof.keyswitch_launches, s.prof.keyswitches)) return rc;
    if (out) *out = s.prof;
    if (reset) s.prof = cufhe_amd_profile{};
    return device_fault(device);      // hipEventSynchronize above observed completions
}

}  // extern "C"
