// pack.inc.h -- host side of TLWE packing (included by capi.hip): lvl0 TLWEs -> coefficients of lvl1
// TRLWEs by pack_keyswitch_kernel (kernels_pack.hip.h) in the shape of plan::plan_pack (launch_plan.h).  The packing key is the
// caller's (cufhe_amd_pack_initialize); default parameter set only.  There is no recorded form: callers order the call behind gates
// recorded on a stream with cufhe_amd_stream_fence.

namespace {

int fail_pack_set() { return fail(-1, "TLWE packing runs on the default path only: not with \"param_set\" active"); }

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

}  // extern "C"
