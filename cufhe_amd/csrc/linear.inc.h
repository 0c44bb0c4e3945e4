// linear.inc.h -- host side of linear layers (included behind lut.inc.h): a dense int32 matrix and a bias
// word per row, applied to vectors of lvl0 or lvl1 ciphertexts by linear_kernel (kernels_linear.hip.h) in the shape of
// plan::plan_linear (launch_plan.h).  Word arithmetic mod 2^32: no key, exact, the same words under any active parameter set.  A layer
// is an id in a table of its own (not an op id: no gate entry point takes it), its weights live on every device of SetGPUNum from
// cufhe_amd_linear_define on, and CleanUp drops them all (linear_drop_all, called where CleanUp quiesces the scheduler).  The batch and
// the list form reach the one kernel as pointer tables staged through the stream's workspace; the fused form runs the kernel into a
// pooled block of the stream and hands that to the gate path as the operands of sets * rows one-input user gates.  Nothing here is
// recorded by the scheduler: cufhe_amd_stream_fence orders a call behind the gates recorded on its stream.

#include <unordered_set>

#include "kernels_linear.hip.h"

namespace {

static_assert(plan::kLinearWaveWords == 64, "a wave of 64 lanes owns 64 word indices");

struct LinearLayer {
    int rows = 0, cols = 0;
    std::vector<int32_t*> weights;      // per logical device: [row_tiles][cols][kLinearTJ]
    std::vector<uint32_t*> bias;        // per logical device: [row_tiles * kLinearTJ]
};
// the fused form's temporary of one (device, stream): grow-only, like the key switch's digit words; released by cufhe_amd_stream_destroy
// (linear_forget_stream) and by CleanUp
struct LinearTmp { uint32_t* p = nullptr; size_t words = 0; };

std::mutex g_linear_mu;                 // the table and the pool below
LinearLayer g_linear[CUFHE_AMD_MAX_LINEAR_LAYERS];
int g_linear_count = 0;                 // layers count from the last cufhe_amd_cleanup
std::map<std::pair<int, hipStream_t>, LinearTmp> g_linear_tmp;

// CleanUp (sched_quiesce): every layer and every pooled temporary goes; what was launched with them completes first
void linear_drop_all()
{
    std::lock_guard<std::mutex> lk(g_linear_mu);
    auto release = [](int device, void* p) {
        if (!p || device >= g_gpu_num) return;
        if (hipSetDevice(phys_device(device)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return; }
        (void)hipFree(p);
    };
    for (int k = 0; k < g_linear_count; k++) {
        LinearLayer& l = g_linear[k];
        for (size_t d = 0; d < l.weights.size(); d++) { release((int)d, l.weights[d]); release((int)d, l.bias[d]); }
        l = LinearLayer{};
    }
    g_linear_count = 0;
    for (auto& kv : g_linear_tmp) release(kv.first.first, kv.second.p);
    g_linear_tmp.clear();
}

// cufhe_amd_stream_destroy: the stream's pooled temporary goes with its workspace (the device is current).  A later stream may get the
// same handle: it starts without a block, like any new stream.  The stream is drained first -- at no cost behind the workspace release,
// which has waited already.
int linear_forget_stream(int device, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(g_linear_mu);
    auto it = g_linear_tmp.find({device, st});
    if (it == g_linear_tmp.end()) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(it->second.p);
    g_linear_tmp.erase(it);
    return 0;
}

// the layer of an id, copied out under the lock (a few words and two small vectors); false: never defined, or dropped by CleanUp
bool linear_find(int layer, LinearLayer* out)
{
    std::lock_guard<std::mutex> lk(g_linear_mu);
    const int k = layer - CUFHE_AMD_LINEAR_LAYER_BASE;
    if (k < 0 || k >= g_linear_count) return false;
    *out = g_linear[k];
    return true;
}
int fail_linear_layer() { return fail(-1, "linear layer not defined (cufhe_amd_linear_define; CleanUp drops the layers)"); }

// words [p, p + (count - 1) stride + words) of `count` ciphertexts `stride` words apart
size_t linear_span(size_t count, size_t stride, size_t words) { return count ? (count - 1) * stride + words : 0; }

// What every form refuses before any device work, in the order of the header: the layer, the level, and the size of the launch.
int check_linear_call(const char* who, int device, int layer, int level, size_t sets, LinearLayer* l, int* words)
{
    if (int rc = check_device(device)) return rc;
    if (!linear_find(layer, l)) return fail_linear_layer();
    if (level != 0 && level != 1) return fail(-1, std::string(who) + ": level must be 0 or 1");
    *words = cufhe_amd_ctxt_words(level);
    if (*words <= 0) return -1;
    if (sets > (size_t)CUFHE_AMD_LINEAR_MAX_POINTERS / (size_t)std::max(l->rows, l->cols))
        return fail(-1, std::string(who) + ": sets * max(rows, cols) exceeds 2^24 (the pointer tables of one launch)");
    const plan::LinearPlan p = plan::plan_linear((size_t)l->rows, (size_t)l->cols, sets, *words, 1);
    if (p.waves > (long)INT32_MAX) return fail(-1, std::string(who) + ": the launch exceeds the kernel's grid");
    return 0;
}

// One launch of linear_kernel: ins [sets][cols] and outs [sets][rows] (host arrays of device pointers, already checked) go to the
// device through the stream's workspace.
int launch_linear(DeviceState& s, int device, hipStream_t st, const LinearLayer& l, int words, size_t sets, const std::vector<const uint32_t*>& ins,
                  const std::vector<uint32_t*>& outs)
{
    Scratch sc;
    if (int rc = open_scratch(s, st, (ins.size() + outs.size()) * sizeof(void*) + 4096, &sc)) return rc;
    const uint32_t** dins;
    uint32_t** douts;
    if (int rc = upload_descs(s, sc, ins, &dins)) return rc;
    if (int rc = upload_descs(s, sc, outs, &douts)) return rc;
    const plan::LinearPlan p = plan::plan_linear((size_t)l.rows, (size_t)l.cols, sets, words, cus_of(s));
    hipLaunchKernelGGL(linear_kernel, dim3(p.grid_x), dim3(p.block_x), 0, st, dins, douts, l.weights[(size_t)device], l.bias[(size_t)device], l.rows,
                       l.cols, words, p.row_tiles, p.chunks, p.waves);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the pointer tables of the batch forms
void linear_batch_tables(const LinearLayer& l, size_t sets, const uint32_t* in, size_t in_stride, uint32_t* out, size_t out_stride,
                         std::vector<const uint32_t*>* ins, std::vector<uint32_t*>* outs)
{
    ins->resize(sets * (size_t)l.cols);
    outs->resize(sets * (size_t)l.rows);
    for (size_t g = 0; g < ins->size(); g++) (*ins)[g] = in + g * in_stride;
    for (size_t g = 0; g < outs->size(); g++) (*outs)[g] = out + g * out_stride;
}

// what the two batch forms refuse about their arrays
int check_linear_arrays(const char* who, const LinearLayer& l, int words, size_t sets, const uint32_t* in, size_t in_stride, const uint32_t* out,
                        size_t out_stride)
{
    if (in_stride < (size_t)words || out_stride < (size_t)words)
        return fail(-1, std::string(who) + ": a stride is smaller than a ciphertext of the active parameter set (cufhe_amd_ctxt_words)");
    // waves of other rows still read the inputs while a row is stored: any overlap of the two arrays is refused
    if (ranges_overlap(in, linear_span(sets * (size_t)l.cols, in_stride, (size_t)words), out, linear_span(sets * (size_t)l.rows, out_stride, (size_t)words)))
        return fail(-1, std::string(who) + ": out must not overlap in");
    return 0;
}

}  // namespace

extern "C" {

int cufhe_amd_linear_define(size_t rows, size_t cols, const int32_t* weights, const uint32_t* bias, int* layer)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!weights || !layer) return fail(-1, "linear_define: null pointer");
    if (rows < 1 || cols < 1 || rows > CUFHE_AMD_LINEAR_MAX_DIM || cols > CUFHE_AMD_LINEAR_MAX_DIM || rows * cols > CUFHE_AMD_LINEAR_MAX_WEIGHTS)
        return fail(-1, "linear_define: 1 <= rows, cols <= 16384 and rows * cols <= 2^26 are required");
    {
        std::lock_guard<std::mutex> lk2(g_linear_mu);
        if (g_linear_count >= CUFHE_AMD_MAX_LINEAR_LAYERS) return fail(-1, "linear layer table full (CUFHE_AMD_MAX_LINEAR_LAYERS layers until CleanUp)");
    }
    // the device copy's layout, once on the host; then build first, publish last: a failure on the way leaves nothing allocated
    std::vector<int32_t> w(linear_weight_words(rows, cols), 0);
    for (size_t j = 0; j < rows; j++)
        for (size_t k = 0; k < cols; k++) w[linear_weight_index(j, k, cols)] = weights[j * cols + k];
    std::vector<uint32_t> b((rows + kLinearTJ - 1) / kLinearTJ * kLinearTJ, 0u);
    if (bias) std::copy(bias, bias + rows, b.begin());
    std::vector<DevPtr<int32_t>> dw((size_t)g_gpu_num);
    std::vector<DevPtr<uint32_t>> db((size_t)g_gpu_num);
    for (int i = 0; i < g_gpu_num; i++) {
        if (int rc = ensure_ntt(i)) return rc;      // the device's state exists (its CU count; CleanUp releases what the calls stage)
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(dw[(size_t)i].alloc(w.size()));
        HIP_TRY(db[(size_t)i].alloc(b.size()));
        HIP_TRY(hipMemcpy(dw[(size_t)i].p, w.data(), w.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(db[(size_t)i].p, b.data(), b.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    std::lock_guard<std::mutex> lk2(g_linear_mu);
    LinearLayer& l = g_linear[g_linear_count];
    l.rows = (int)rows; l.cols = (int)cols;
    l.weights.clear(); l.bias.clear();
    for (int i = 0; i < g_gpu_num; i++) { l.weights.push_back(dw[(size_t)i].release()); l.bias.push_back(db[(size_t)i].release()); }
    *layer = CUFHE_AMD_LINEAR_LAYER_BASE + g_linear_count++;
    return 0;
}

int cufhe_amd_linear_get(int layer, size_t* rows, size_t* cols)
{
    LinearLayer l;
    if (!linear_find(layer, &l)) return fail_linear_layer();
    if (rows) *rows = (size_t)l.rows;
    if (cols) *cols = (size_t)l.cols;
    return 0;
}

int cufhe_amd_linear_batch(int device, void* stream, int layer, int level, size_t sets, const uint32_t* in, size_t in_stride_words, uint32_t* out,
                           size_t out_stride_words)
{
    if (!in || !out) return fail(-1, "linear_batch: null pointer");
    LinearLayer l;
    int words = 0;
    if (int rc = check_linear_call("linear_batch", device, layer, level, sets, &l, &words)) return rc;
    if (int rc = check_linear_arrays("linear_batch", l, words, sets, in, in_stride_words, out, out_stride_words)) return rc;
    if (sets == 0) return 0;
    if (int rc = use_device(device)) return rc;
    std::vector<const uint32_t*> ins;
    std::vector<uint32_t*> outs;
    linear_batch_tables(l, sets, in, in_stride_words, out, out_stride_words, &ins, &outs);
    return launch_linear(g_dev[device], device, (hipStream_t)stream, l, words, sets, ins, outs);
}

int cufhe_amd_linear_list(int device, void* stream, int layer, int level, size_t sets, const uint32_t* const* ins, uint32_t* const* outs)
{
    if (!ins || !outs) return fail(-1, "linear_list: null array");
    LinearLayer l;
    int words = 0;
    if (int rc = check_linear_call("linear_list", device, layer, level, sets, &l, &words)) return rc;
    std::vector<const uint32_t*> hin(ins, ins + sets * (size_t)l.cols);
    std::vector<uint32_t*> hout(outs, outs + sets * (size_t)l.rows);
    // waves of other rows still read the inputs while a row is stored: no output may be an input (of any set)
    std::unordered_set<const uint32_t*> read(hin.begin(), hin.end());
    if (read.count(nullptr)) return fail(-1, "linear_list: null ciphertext pointer");
    for (const uint32_t* o : hout) {
        if (!o) return fail(-1, "linear_list: null ciphertext pointer");
        if (read.count(o)) return fail(-1, "linear_list: an output must not be an input");
    }
    if (sets == 0) return 0;
    if (int rc = use_device(device)) return rc;
    return launch_linear(g_dev[device], device, (hipStream_t)stream, l, words, sets, hin, hout);
}

int cufhe_amd_linear_gate_batch(int device, void* stream, int layer, int op, int level, size_t sets, const uint32_t* in, size_t in_stride_words,
                                uint32_t* out, size_t out_stride_words)
{
    if (!in || !out) return fail(-1, "linear_gate_batch: null pointer");
    LinearLayer l;
    int words = 0;
    if (int rc = check_linear_call("linear_gate_batch", device, layer, level, sets, &l, &words)) return rc;
    if (int rc = check_linear_arrays("linear_gate_batch", l, words, sets, in, in_stride_words, out, out_stride_words)) return rc;
    if (g_param_set >= 0 || g_lvl0_ring == 2048)
        return fail(-1, "linear_gate_batch runs on the default path only: not with \"param_set\" active or \"lvl0_ring\" 2048");
    DeviceState& s = g_dev[device];
    if (!s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    // the op: a user gate of the default path, an output of a multi-output definition included, that reads one operand
    const opreg::Admission a = opreg::admit(g_ops, op, opreg::route_of_options(g_param_set, g_lvl0_ring, level), opreg::Entry::List);
    if (a.family != opreg::Family::User) return fail(-1, "linear_gate_batch: op must be a user gate of the default path (cufhe_amd_define_gate)");
    if (int rc = refuse(a.refusal)) return rc;
    if (!a.gate || user_gate_arity(*a.gate) != 1) return fail(-1, "linear_gate_batch: the user gate must read one operand (c1 = c2 = 0)");
    if (sets == 0) return 0;
    if (int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t count = sets * (size_t)l.rows;
    uint32_t* tmp = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_linear_mu);
        LinearTmp& t = g_linear_tmp[{device, st}];
        if (t.words < count * (size_t)words) {
            if (t.p) {
                HIP_TRY(hipStreamSynchronize(st));
                HIP_TRY(hipFree(t.p));
                t.p = nullptr; t.words = 0;
            }
            HIP_TRY(hipMalloc((void**)&t.p, count * (size_t)words * sizeof(uint32_t)));
            t.words = count * (size_t)words;
        }
        tmp = t.p;
    }
    std::vector<const uint32_t*> ins;
    std::vector<uint32_t*> outs;
    linear_batch_tables(l, sets, in, in_stride_words, tmp, (size_t)words, &ins, &outs);
    if (int rc = launch_linear(s, device, st, l, words, sets, ins, outs)) return rc;
    return run_gates(device, stream, level, count, [&](size_t g) { return GateRef{op, out + g * out_stride_words, tmp + g * (size_t)words, nullptr, nullptr}; });
}

}  // extern "C"
