// pack.inc.h -- host side of TLWE packing (included by capi.hip): lvl0 TLWEs -> coefficients of lvl1
// TRLWEs by pack_keyswitch_kernel (kernels_pack.hip.h) in the shape of plan::plan_pack (launch_plan.h).  The packing key is the
// caller's (cufhe_amd_pack_initialize); default parameter set only.  Two forms: cufhe_amd_pack_batch on raw device arrays, which callers
// order behind gates recorded on a stream with cufhe_amd_stream_fence, and the recorded cufhe_amd_enqueue_pack on ciphertext handles, a
// scheduler node of n inputs (DeviceSched::record_pack); all recorded packs of a dependence level are lowered together by
// lower_pack_ops: one zeroing launch and one launch of pack_keyswitch_desc_kernel over the concatenation of their terms.

namespace {

int fail_pack_set() { return fail(-1, "TLWE packing runs on the default path only: not with \"param_set\" active"); }

// The recorded packs of ONE dependence level.  Their outputs are distinct buffers (a second writer of a buffer sits in a later level)
// that nothing else of the level touches, so they are zeroed through a pointer table and every term of every pack adds into them from
// one launch in the shape plan_pack gives for the total: a tile of 64 terms may straddle outputs.  Descriptors live in the stream's
// workspace from offset 0, like every lowering's (HipBackend::run_gates runs this as a launch sequence of its own).
int lower_pack_ops(DeviceState& s, hipStream_t st, const GateRef* g, size_t n)
{
    if (n == 0) return 0;
    if (g_param_set >= 0) return fail_pack_set();
    if (!s.pack_key) return fail(-3, "cufhe_amd_pack_initialize has not been called for this device");
    std::vector<uint32_t*> outs;
    std::vector<PackDesc> terms;
    outs.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const sched::PackNode* node = sched::pack_node(g[i]);
        if (g[i].op != CUFHE_AMD_TL_PACK || !g[i].out || !node || node->terms.empty()) return fail(-1, "internal: not a recorded pack");
        outs.push_back(g[i].out);
        for (const sched::PackTerm& t : node->terms) {
            if (!t.in || t.pos < 0 || t.pos >= kN) return fail(-1, "internal: recorded pack term out of range");
            terms.push_back({t.in, g[i].out, t.pos});
        }
    }
    if (terms.size() > (size_t)INT32_MAX / 2) return fail(-1, "recorded packs: the terms of one level exceed the kernel's index type");
    ProfScope prof{s, st, terms.size(), true};       // as in the batch call: zeroing, staging of the descriptors and the kernel, one launcher call
    if (int rc = prof.begin()) return rc;
    Scratch sc;
    if (int rc = open_scratch(s, st, terms.size() * sizeof(PackDesc) + outs.size() * sizeof(uint32_t*) + 8192, &sc)) return rc;
    uint32_t** douts;
    PackDesc* dterms;
    if (int rc = upload_descs(s, sc, outs, &douts)) return rc;
    if (int rc = upload_descs(s, sc, terms, &dterms)) return rc;
    hipLaunchKernelGGL(pack_zero_desc_kernel, dim3((unsigned)outs.size()), dim3(kPackThreads), 0, st, douts, (int)outs.size());
    HIP_TRY(hipGetLastError());
    const plan::PackPlan p = plan::plan_pack(terms.size(), cus_of(s), kPackGeometry, g_tuning);
    hipLaunchKernelGGL(pack_keyswitch_desc_kernel, dim3(p.grid_x, p.grid_y), dim3(kPackThreads), 0, st, dterms, (int)terms.size(), s.pack_key,
                       p.tiles, p.slices);
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

}  // namespace

extern "C" {

int cufhe_amd_pack_get_params(cufhe_amd_pack_params* p)
{
    if (!p) return fail(-1, "null");
    p->n = kLvl0N; p->N = kN; p->t = kPackT; p->basebit = kPackBasebit;
    p->key_words = kPackKeyWords;
    return 0;
}

int cufhe_amd_pack_initialize(const uint32_t* key, size_t words)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!key) return fail(-1, "null key pointer");
    if (words != kPackKeyWords) return fail(-1, "packing key has the wrong size: K[n][t][2^basebit - 1][k + 1][N] uint32");
    if (g_param_set >= 0) return fail_pack_set();
    // build first, swap last: every device's copy is uploaded beside what is loaded, through one pinned chunk
    constexpr size_t kChunk = (size_t)32 << 20;
    void* pinned = nullptr;
    HIP_TRY(hipHostMalloc(&pinned, kChunk, hipHostMallocDefault));
    struct PinnedFree { void* p; ~PinnedFree() { (void)hipHostFree(p); } } pf{pinned};
    std::vector<DevPtr<uint32_t>> built((size_t)g_gpu_num);
    for (int i = 0; i < g_gpu_num; i++) {
        if (int rc = ensure_ntt(i)) return rc;      // the device's state exists (CleanUp releases what is loaded here)
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(built[(size_t)i].alloc(kPackKeyWords));
        const char* src = (const char*)key;
        char* dst = (char*)built[(size_t)i].p;
        for (size_t off = 0, total = kPackKeyWords * sizeof(uint32_t); off < total; off += kChunk) {
            const size_t b = std::min(kChunk, total - off);
            memcpy(pinned, src + off, b);
            HIP_TRY(hipMemcpy(dst + off, pinned, b, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipDeviceSynchronize());        // also: nothing on this device still reads the key that is about to go
    }
    for (int i = 0; i < g_gpu_num; i++) {
        DeviceState& s = g_dev[i];
        (void)hipSetDevice(phys_device(i));
        if (s.pack_key) (void)hipFree(s.pack_key);
        s.pack_key = built[(size_t)i].release();
    }
    return 0;
}

int cufhe_amd_pack_batch(int device, void* stream, size_t count_in, const uint32_t* tlwe0, const int32_t* dst, const int32_t* pos,
                         size_t count_out, uint32_t* trlwe)
{
    if (g_param_set >= 0) return fail_pack_set();
    if (int rc = check_device(device)) return rc;
    if (!trlwe || (count_in && (!tlwe0 || !dst || !pos))) return fail(-1, "null pointer");
    if (count_in > (size_t)INT32_MAX / 2 || count_out > (size_t)INT32_MAX) return fail(-1, "pack_batch: count exceeds the index type of dst");
    for (size_t m = 0; m < count_in; m++) {
        if (dst[m] < 0 || (size_t)dst[m] >= count_out) return fail(-1, "pack_batch: dst outside [0, count_out)");
        if (pos[m] < 0 || pos[m] >= kN) return fail(-1, "pack_batch: pos outside [0, N)");
    }
    DeviceState& s = g_dev[device];
    if (!s.pack_key) return fail(-3, "cufhe_amd_pack_initialize has not been called for this device");
    if (count_out == 0) return 0;
    if (int rc = use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof{s, st, count_in, true};       // zeroing, staging of dst / pos and the kernel
    if (int rc = prof.begin()) return rc;
    HIP_TRY(hipMemsetAsync(trlwe, 0, count_out * kPackRowWords * sizeof(uint32_t), st));
    if (count_in == 0) return prof.commit();
    Scratch sc;
    if (int rc = open_scratch(s, st, 2 * count_in * sizeof(int32_t) + 4096, &sc)) return rc;
    std::vector<int32_t> h(2 * count_in);
    std::copy(dst, dst + count_in, h.begin());
    std::copy(pos, pos + count_in, h.begin() + (ptrdiff_t)count_in);
    int32_t* d;
    if (int rc = upload_descs(s, sc, h, &d)) return rc;
    const plan::PackPlan p = plan::plan_pack(count_in, cus_of(s), kPackGeometry, g_tuning);
    hipLaunchKernelGGL(pack_keyswitch_kernel, dim3(p.grid_x, p.grid_y), dim3(kPackThreads), 0, st, tlwe0, (int)count_in, d, s.pack_key,
                       trlwe, p.tiles, p.slices);
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

int cufhe_amd_enqueue_pack(int device, void* stream, int copying, cufhe_amd_ctxt* out, size_t count_in, cufhe_amd_ctxt* const* ins,
                           const int32_t* pos)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    if (g_param_set >= 0) return fail_pack_set();
    if (int rc = check_device(device)) return rc;
    if (!out || !ins || !pos) return fail(-1, "enqueue_pack: null pointer");
    if (count_in < 1 || count_in > (size_t)kN) return fail(-1, "enqueue_pack: count_in outside [1, N]");
    for (size_t m = 0; m < count_in; m++) {
        if (!ins[m]) return fail(-1, "enqueue_pack: null ciphertext");
        if (pos[m] < 0 || pos[m] >= kN) return fail(-1, "enqueue_pack: pos outside [0, N)");
    }
    if (out->level != 2) return fail(-1, "enqueue_pack: out is a TRLWE (level 2), the inputs lvl0 ciphertexts (level 0)");
    for (size_t m = 0; m < count_in; m++)
        if (ins[m]->level != 0) return fail(-1, "enqueue_pack: out is a TRLWE (level 2), the inputs lvl0 ciphertexts (level 0)");
    sched::Scheduler* S = scheduler();
    if (int rc = sched_check_ctxt(S, out)) return rc;
    for (size_t m = 0; m < count_in; m++)
        if (int rc = sched_check_ctxt(S, ins[m])) return rc;
    if (!g_dev[device].pack_key) return fail(-3, "cufhe_amd_pack_initialize has not been called for this device");
    if (int rc = S->dev(device).record_pack(stream, CUFHE_AMD_TL_PACK, copying != 0, out, ins, pos, count_in)) return sched_error(S->dev(device), rc);
    return 0;
}

}  // extern "C"
