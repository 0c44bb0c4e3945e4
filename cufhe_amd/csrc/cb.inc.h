// cb.inc.h -- host side of circuit bootstrapping (included by capi.hip): lvl0 TLWE -> lvl1 TRGSW, torus or NTT domain.
// Kernels: the lvl02 rotations of kernels_lvl2*.hip.h with RotDesc2::pad = log2 mu_r and cb_add_mu_kernel -- or, with "cb_rotations" 1,
// one rotation per input from the library's test-vector row and cb_gather_mu_kernel -- and private_keyswitch_kernel
// (kernels_pks.hip.h), bk_to_ntt_kernel for TRGSW2NTT.  Needs the lvl02 key (cufhe_amd_lvl2_initialize) and the private key-switching
// key (cufhe_amd_cb_initialize); runs on the default parameter set only.

namespace {

int cb_ready(const DeviceState& s, bool rotate)
{
    if (g_param_set >= 0) return fail(-1, "circuit bootstrapping targets the default lvl1 shape: not with \"param_set\" active");
    if (!s.cb_pksk) return fail(-3, "cufhe_amd_cb_initialize has not been called for this device");
    if (rotate && !s.keys2_ready) return fail(-3, "circuit bootstrapping needs the lvl02 key: cufhe_amd_lvl2_initialize has not been called");
    return 0;
}

// private_keyswitch_kernel in the shape of plan::plan_private_keyswitch (launch_plan.h); slices add into a zeroed output
int launch_private_keyswitch(DeviceState& s, hipStream_t st, const uint64_t* in, size_t count, uint32_t* out, int rows_per_out)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, true};
    if (int rc = prof.begin()) return rc;
    const plan::PksPlan p = plan::plan_private_keyswitch(count, cus_of(s), kPksGeometry);
    if (p.slices > 1)
        HIP_TRY(hipMemsetAsync(out, 0, (count / rows_per_out) * 2 * rows_per_out * kCbRowWords * sizeof(uint32_t), st));
    hipLaunchKernelGGL(private_keyswitch_kernel, dim3(p.grid_x, p.grid_y), dim3(kPksThreads), 0, st, in, (int)count, s.cb_pksk, out,
                       rows_per_out, p.tiles, p.slices);
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

// scratch of stage 1 beside its result: the descriptors and, in the one-rotation form, the 2^kCbShift outputs of every rotation
size_t cb_stage1_scratch(size_t count)
{
    if (g_cb_rotations == 1) return count * (sizeof(RotDesc2) + ((size_t)1 << kCbShift) * kPksIn * sizeof(uint64_t)) + 4096;
    return count * kCbL * sizeof(RotDesc2) + 4096;
}

// stage 1 of `count` circuit bootstraps of the lvl0 ciphertexts in(g) into tlwe2 [count][l][N2 + 1], mu_r added to b: l rotations each
// with constant test vectors, or ("cb_rotations" 1) one rotation each that leaves every row.  Descriptors and the one-rotation form's
// outputs come out of `sc` (the caller's scratch, sized with cb_stage1_scratch: its other buffers stay valid)
template <class GetIn>
int cb_rotate(DeviceState& s, hipStream_t st, Scratch& sc, size_t count, GetIn in, uint64_t* tlwe2)
{
    RotDesc2* d;
    if (g_cb_rotations == 1) {
        if (int rc = ensure_tvs2(s)) return rc;
        uint64_t* all;
        if (int rc = sc.alloc((void**)&all, count * ((size_t)1 << kCbShift) * kPksIn * sizeof(uint64_t))) return rc;
        std::vector<RotDesc2> h(count);
        for (size_t g = 0; g < count; g++)
            h[g] = RotDesc2{in(g), in(g), all + g * ((size_t)1 << kCbShift) * kPksIn, 1, 0, 0u, make_pad2(kCbRow2, kCbShift)};
        if (int rc = upload_descs(s, sc, h, &d)) return rc;
        if (int rc = launch_blind_rotate_lvl2(s, st, d, count, kLvl0N, nullptr, true)) return rc;
        hipLaunchKernelGGL(cb_gather_mu_kernel, dim3((unsigned)(count * kCbL)), dim3(256), 0, st, all, tlwe2, (int)(count * kCbL));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    std::vector<RotDesc2> h(count * kCbL);
    for (size_t g = 0; g < count; g++)
        for (int r = 0; r < kCbL; r++)
            h[g * kCbL + r] = RotDesc2{in(g), in(g), tlwe2 + (g * kCbL + r) * kPksIn, 1, 0, 0u, cb_mu_log2(r)};
    if (int rc = upload_descs(s, sc, h, &d)) return rc;
    if (int rc = launch_blind_rotate_lvl2(s, st, d, h.size(), kLvl0N, nullptr, false)) return rc;
    const int n = (int)h.size();
    hipLaunchKernelGGL(cb_add_mu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tlwe2, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cb_to_ntt(DeviceState& s, hipStream_t st, size_t count, const uint32_t* trgsw, double* trgsw_ntt)
{
    const size_t polys = count * kBkPolysPerStep;
    const unsigned blocks = (unsigned)((polys + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(bk_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttLdsBytes, st, trgsw_ntt, trgsw, polys, s.tables,
                       n_inverse(kN));
    HIP_TRY(hipGetLastError());
    return 0;
}

// the whole circuit bootstrap: tlwe0 [count][n + 1] -> trgsw [count][12288] (torus, may be null) and / or trgsw_ntt (may be null)
int cb_run(DeviceState& s, hipStream_t st, size_t count, const uint32_t* tlwe0, uint32_t* trgsw, double* trgsw_ntt)
{
    if (count == 0) return 0;
    const size_t t2_bytes = count * kCbL * kPksIn * sizeof(uint64_t), tg_bytes = trgsw ? 0 : count * kCbTrgswWords * sizeof(uint32_t);
    Scratch sc;
    if (int rc = open_scratch(s, st, t2_bytes + tg_bytes + cb_stage1_scratch(count) + 8192, &sc)) return rc;
    uint64_t* t2;
    if (int rc = sc.alloc((void**)&t2, t2_bytes)) return rc;
    uint32_t* tg = trgsw;
    if (!tg)
        if (int rc = sc.alloc((void**)&tg, tg_bytes)) return rc;
    if (int rc = cb_rotate(s, st, sc, count, [&](size_t g) { return tlwe0 + g * kLvl0Words; }, t2)) return rc;
    if (int rc = launch_private_keyswitch(s, st, t2, count * kCbL, tg, kCbL)) return rc;
    return trgsw_ntt ? cb_to_ntt(s, st, count, tg, trgsw_ntt) : 0;
}

// the circuit bootstraps of one dependence level of the per-gate scheduler (lower_trlwe_ops): in0 = a lvl0 ciphertext, out = the device
// words of a TRGSW holder (level 3, NTT domain).  One rotation launch, one private key-switch launch, one TRGSW2NTT launch.
int lower_cb_ops(DeviceState& s, hipStream_t st, const GateRef* g, size_t n)
{
    if (int rc = cb_ready(s, true)) return rc;
    if (!s.ntt_ready) return fail(-3, "Initialize() has not been called for this device");
    std::vector<const uint32_t*> ins;
    std::vector<double*> outs;
    for (size_t i = 0; i < n; i++)
        if (g[i].op == CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP) { ins.push_back(g[i].in0); outs.push_back((double*)g[i].out); }
    const size_t count = ins.size();
    const size_t t2_bytes = count * kCbL * kPksIn * sizeof(uint64_t), tg_bytes = count * kCbTrgswWords * sizeof(uint32_t);
    Scratch sc;
    if (int rc = open_scratch(s, st, t2_bytes + tg_bytes + cb_stage1_scratch(count) + count * kBkPolysPerStep * sizeof(LinDesc) + 16384, &sc))
        return rc;
    uint64_t* t2;
    uint32_t* tg;
    if (int rc = sc.alloc((void**)&t2, t2_bytes)) return rc;
    if (int rc = sc.alloc((void**)&tg, tg_bytes)) return rc;
    if (int rc = cb_rotate(s, st, sc, count, [&](size_t c) { return ins[c]; }, t2)) return rc;
    if (int rc = launch_private_keyswitch(s, st, t2, count * kCbL, tg, kCbL)) return rc;
    // TRGSW2NTT into the holders: contiguous runs of holders are one launch of the batch conversion; scattered ones one launch each
    size_t a = 0;
    while (a < count) {
        size_t b = a + 1;
        while (b < count && outs[b] == outs[b - 1] + kBkStepDoubles) b++;
        if (int rc = cb_to_ntt(s, st, b - a, tg + a * kCbTrgswWords, outs[a])) return rc;
        a = b;
    }
    return 0;
}

}  // namespace

extern "C" {

int cufhe_amd_cb_get_params(cufhe_amd_cb_params* p)
{
    if (!p) return fail(-1, "null");
    p->n = kLvl0N; p->N = kN; p->k = 1; p->l = kCbL; p->Bgbit = kCbBgbit;
    p->N2 = k2N; p->l2 = k2L; p->Bgbit2 = k2Bgbit; p->t = kPksT; p->basebit = kPksBasebit;
    p->lvl0_words = kLvl0Words; p->lvl2_words = kPksIn; p->trgsw_words = kCbTrgswWords; p->trgsw_ntt_doubles = (uint32_t)kBkStepDoubles;
    p->privksk_words = kPksKeyWords;
    return 0;
}

int cufhe_amd_cb_initialize(const uint32_t* privksk, size_t words)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!privksk) return fail(-1, "null key pointer");
    if (words != kPksKeyWords) return fail(-1, "private key-switching key has the wrong size: K[2][N2 + 1][t][2^basebit - 1][k + 1][N] uint32");
    if (g_param_set >= 0) return fail(-1, "circuit bootstrapping targets the default lvl1 shape: not with \"param_set\" active");
    // build first, swap last: every device's copy is uploaded beside what is loaded, through one pinned chunk
    constexpr size_t kChunk = (size_t)64 << 20;
    void* pinned = nullptr;
    HIP_TRY(hipHostMalloc(&pinned, kChunk, hipHostMallocDefault));
    struct PinnedFree { void* p; ~PinnedFree() { (void)hipHostFree(p); } } pf{pinned};
    std::vector<DevPtr<uint32_t>> built((size_t)g_gpu_num);
    for (int i = 0; i < g_gpu_num; i++) {
        if (int rc = ensure_ntt(i)) return rc;
        HIP_TRY(hipSetDevice(phys_device(i)));
        if (int rc = ensure_tvs2(g_dev[i])) return rc;        // the one-rotation form's test-vector row
        HIP_TRY(built[(size_t)i].alloc(kPksKeyWords));
        const char* src = (const char*)privksk;
        char* dst = (char*)built[(size_t)i].p;
        for (size_t off = 0, total = kPksKeyWords * sizeof(uint32_t); off < total; off += kChunk) {
            const size_t b = std::min(kChunk, total - off);
            memcpy(pinned, src + off, b);
            HIP_TRY(hipMemcpy(dst + off, pinned, b, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipDeviceSynchronize());        // also: nothing on this device still reads the key that is about to go
    }
    for (int i = 0; i < g_gpu_num; i++) {
        DeviceState& s = g_dev[i];
        (void)hipSetDevice(phys_device(i));
        if (s.cb_pksk) (void)hipFree(s.cb_pksk);
        s.cb_pksk = built[(size_t)i].release();
    }
    return 0;
}

int cufhe_amd_cb_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint64_t* tlwe2)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (int rc = cb_ready(s, true)) return rc;
    if (!tlwe0 || !tlwe2) return fail(-1, "null pointer");
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc;
    if (int rc = open_scratch(s, st, cb_stage1_scratch(count) + 4096, &sc)) return rc;
    return cb_rotate(s, st, sc, count, [&](size_t g) { return tlwe0 + g * kLvl0Words; }, tlwe2);
}

int cufhe_amd_private_keyswitch_batch(int device, void* stream, size_t count, const uint64_t* tlwe2, uint32_t* trlwe)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (int rc = cb_ready(s, false)) return rc;
    if (!tlwe2 || !trlwe) return fail(-1, "null pointer");
    return launch_private_keyswitch(s, (hipStream_t)stream, tlwe2, count, trlwe, 1);
}

int cufhe_amd_circuit_bootstrap_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint32_t* trgsw, double* trgsw_ntt)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (int rc = cb_ready(s, true)) return rc;
    if (!tlwe0 || (!trgsw && !trgsw_ntt)) return fail(-1, "null pointer");
    if (trgsw_ntt) {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    return cb_run(s, (hipStream_t)stream, count, tlwe0, trgsw, trgsw_ntt);
}

}  // extern "C"
