// lvl2.inc.h -- host side of the N = 2048 / 64-bit-torus gate path (included by capi.hip).
// Gates take and return lvl0 ciphertexts; the bootstrap runs through the lvl2 ring:
// blind rotate lvl02 -> sample extract -> key switch lvl20, i.e. __HomGate__ (br -> iks,
// src/bootstrap_gpu.cu:402-421) and the Mux of :515-588 instantiated at brP = lvl02,
// iksP = lvl20.  Kernels: kernels_lvl2.hip.h.

namespace {

int ensure_tables_lvl2(int device)
{
    DeviceState& s = g_dev[device];
    if (s.tables2 && s.tables2q) return 0;
    HIP_TRY(hipSetDevice(phys_device(device)));
    if (!s.cus)
        if (int rc = read_cus(s, device)) return rc;
    if (!s.tables2) {
        static NttTables host[2];
        build_tables_lvl2(host);
        HIP_TRY(hipMalloc((void**)&s.tables2, sizeof(host)));
        HIP_TRY(hipMemcpy(s.tables2, host, sizeof(host), hipMemcpyHostToDevice));
    }
    if (!s.tables2q) {
        static Ntt512Tables hostq[4];
        build_tables_lvl2q(hostq);
        for (int q = 0; q < 4; q++)
            if (!fill_r4_products_512(hostq[q])) return fail(-2, "quarter tables: the stage-b twiddles of a block are not I apart (radix-4 form)");
        HIP_TRY(hipMalloc((void**)&s.tables2q, sizeof(hostq)));
        HIP_TRY(hipMemcpy(s.tables2q, hostq, sizeof(hostq), hipMemcpyHostToDevice));
    }
    return 0;
}

// The half-transform kernel's layout of the key (495 MB) is built on first use: the quarter-transform kernel serves every launch above
// one rotation per CU, so a process that only ever runs batches never pays for the second layout.  The torus-domain key is kept on the
// HOST for that (165 MB of ordinary memory, once per process), not on the devices.
std::vector<uint64_t> g_bk2_host;
std::mutex g_bk2_mu;
int ensure_bk2_half_layout(DeviceState& s)
{
    std::lock_guard<std::mutex> lk(g_bk2_mu);
    if (s.bk2_ntt) return 0;
    if (g_bk2_host.empty()) return fail(-3, "cufhe_amd_lvl2_initialize has not been called");
    const size_t want_bk = g_bk2_host.size();
    DevPtr<double> half;
    DevPtr<uint64_t> d_bk;            // the torus-domain staging copy: freed on every return
    HIP_TRY(half.alloc((size_t)kLvl0N * k2BkStepDoubles));
    HIP_TRY(d_bk.alloc(want_bk));
    HIP_TRY(hipMemcpy(d_bk.p, g_bk2_host.data(), want_bk * sizeof(uint64_t), hipMemcpyHostToDevice));
    const size_t polys = want_bk / k2N, waves = polys * k2Limbs;
    const unsigned blocks = (unsigned)((waves + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(bk2_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttWavesPerBlock * kTileBytes, 0,
                       half.p, d_bk.p, polys, s.tables2, n_inverse(k2N));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());        // complete before any stream's kernel reads it
    s.bk2_ntt = half.release();
    return 0;
}

void lvl2_release_host_key()
{
    std::lock_guard<std::mutex> lk(g_bk2_mu);
    std::vector<uint64_t>().swap(g_bk2_host);
}

int launch_blind_rotate_lvl2(DeviceState& s, hipStream_t st, const RotDesc2* d, size_t count, int steps, uint64_t* acc_dump)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, false};
    if (int rc = prof.begin()) return rc;
    if (plan::lvl2_quarters(count, cus_of(s), g_tuning)) {
        // four quarter waves per rotation, two rotations per CU (kernels_lvl2q.hip.h)
        if (!s.br2q_lds_opt_in) {
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2q_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kQLdsBytes));
            s.br2q_lds_opt_in = true;
        }
        hipLaunchKernelGGL(blind_rotate_lvl2q_kernel, dim3((unsigned)count), dim3(kQThreads), kQLdsBytes, st, d, (int)count,
                           s.bk2q_ntt, s.tables2q, steps, acc_dump);
    } else {
        if (int rc = ensure_bk2_half_layout(s)) return rc;
        if (!s.br2_lds_opt_in) {
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k3LdsBytes));
            s.br2_lds_opt_in = true;
        }
        hipLaunchKernelGGL(blind_rotate_lvl2_kernel, dim3((unsigned)count), dim3(k2Threads), k3LdsBytes, st, d, (int)count,
                           s.bk2_ntt, s.tables2, steps, acc_dump);
    }
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

int launch_keyswitch_lvl2(DeviceState& s, hipStream_t st, const LinDesc64* d, size_t count)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, true};
    if (int rc = prof.begin()) return rc;
    const plan::KsPlan p = plan_keyswitch_of<KsShapeLvl2>(s, count, plan::kKsFixedShapePath);
    if (p.kernel == plan::KsKernel::WorkgroupPer) {
        launch_keyswitch_direct<KsShapeLvl2, 1>(st, d, count, s.ksk2);
    } else {
        if (int rc = launch_keyswitch_shared<KsShapeLvl2>(s, st, d, count, s.ksk2, &s.ks2_lds_opt_in, p)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

// The N = 2048 ring for lower_gates (capi.hip): gates on lvl0 ciphertexts only, lvl2 TLWEs between rotation and key switch
struct Lvl2Path {
    using RotD = RotDesc2;
    using KsD = LinDesc64;
    using Mid = uint64_t;
    static constexpr int lvl0_words = kLvl0Words, mid_words = k2Words, n = kLvl0N;
    static constexpr uint64_t ks_mu = k2Mu;
    static constexpr bool lvl1_gates = false, user_gates = false;
    DeviceState& s;
    int ready() const { return s.keys2_ready ? 0 : fail(-3, "cufhe_amd_lvl2_initialize has not been called for this device"); }
    int rotate(hipStream_t st, const RotDesc2* d, size_t count, int steps, uint64_t* dump) const { return launch_blind_rotate_lvl2(s, st, d, count, steps, dump); }
    int keyswitch(hipStream_t st, const LinDesc64* d, size_t count) const { return launch_keyswitch_lvl2(s, st, d, count); }
};

template <class GetGate>
int run_gates_lvl2(int device, void* stream, size_t count, GetGate get)
{
    if (int rc = use_device(device)) return rc;
    return lower_gates(Lvl2Path{g_dev[device]}, (hipStream_t)stream, 0, count, get);
}

}  // namespace

extern "C" {

int cufhe_amd_lvl2_get_params(cufhe_amd_lvl2_params* p)
{
    if (!p) return fail(-1, "null");
    p->n = kLvl0N; p->N = k2N; p->nbit = k2Nbit; p->k = 1; p->l = k2L; p->Bgbit = k2Bgbit;
    p->t = k2KsT; p->basebit = k2KsBasebit;
    p->lvl0_words = kLvl0Words; p->lvl2_words = k2Words;
    p->mu = k2Mu;
    p->bk_words = (uint64_t)kLvl0N * k2BkRows * 2 * k2N;
    p->ksk_words = (uint64_t)k2N * k2KsT * k2KsNumBase * kKsRowWords;
    p->bk_ntt_bytes = (uint64_t)kLvl0N * k2BkStepDoubles * sizeof(double);
    return 0;
}

int cufhe_amd_lvl2_initialize(const uint64_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const size_t want_bk = (size_t)kLvl0N * k2BkRows * 2 * k2N;
    const size_t want_ksk = (size_t)k2N * k2KsT * k2KsNumBase * kKsRowWords;
    if (!bk || !ksk) return fail(-1, "null key pointer");
    if (bk_words != want_bk) return fail(-1, "lvl02 bootstrapping key has the wrong size for this parameter set");
    if (ksk_words != want_ksk) return fail(-1, "lvl20 key-switching key has the wrong size for this parameter set");
    // build first, swap last (as cufhe_amd_initialize): the quarter-transform layout and the key-switching key of every device beside
    // what is loaded; the half-transform layout follows on first use (ensure_bk2_half_layout)
    struct Built { DevPtr<double> bk2q; DevPtr<uint32_t> ksk2; DevPtr<uint64_t> d_bk; };
    std::vector<Built> built((size_t)g_gpu_num);      // the torus-domain staging copies d_bk are freed on every return
    for (int i = 0; i < g_gpu_num; i++) {
        if (int rc = ensure_tables_lvl2(i)) return rc;
        DeviceState& s = g_dev[i];
        Built& b = built[(size_t)i];
        HIP_TRY(hipSetDevice(phys_device(i)));
        HIP_TRY(b.bk2q.alloc((size_t)kLvl0N * k2BkStepDoubles));
        if (int rc = upload_ksk_padded(b.ksk2, ksk, want_ksk / kKsRowWords, kKsRowWords, kKsRowPad)) return rc;
        HIP_TRY(b.d_bk.alloc(want_bk));
        HIP_TRY(hipMemcpy(b.d_bk.p, bk, want_bk * sizeof(uint64_t), hipMemcpyHostToDevice));
        const size_t polys = want_bk / k2N;
        const size_t waves = polys * k2Limbs;
        const unsigned blocks = (unsigned)((waves + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
        hipLaunchKernelGGL(bk2q_to_ntt_kernel, dim3(blocks), dim3(kNttThreads), kNttWavesPerBlock * kTile512Bytes, 0,
                           b.bk2q.p, b.d_bk.p, polys, s.tables2q, n_inverse(k2N));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());        // also: nothing on this device still reads the keys that are about to go
    }
    {
        std::lock_guard<std::mutex> lk2(g_bk2_mu);
        g_bk2_host.assign(bk, bk + want_bk);
        for (int i = 0; i < g_gpu_num; i++) {
            DeviceState& s = g_dev[i];
            (void)hipSetDevice(phys_device(i));
            if (s.keys2_ready) { (void)hipFree(s.bk2q_ntt); (void)hipFree(s.ksk2); }
            (void)hipFree(s.bk2_ntt);          // the half layout of the OLD key, if it was ever built
            s.bk2_ntt = nullptr;
            s.bk2q_ntt = built[(size_t)i].bk2q.release();
            s.ksk2 = built[(size_t)i].ksk2.release();
            s.keys2_ready = true;
        }
    }
    return 0;
}

int cufhe_amd_lvl2_gate_batch(int device, void* stream, size_t count, const int32_t* ops, int ops_stride,
                              uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                              size_t stride_words)
{
    if (!ops) return fail(-1, "null ops");
    return run_gates_lvl2(device, stream, count, [&](size_t g) {
        return GateRef{ops[g * (size_t)ops_stride], out + g * stride_words, in0 ? in0 + g * stride_words : nullptr,
                       in1 ? in1 + g * stride_words : nullptr, in2 ? in2 + g * stride_words : nullptr};
    });
}

int cufhe_amd_lvl2_blind_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint64_t* acc, int steps)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys2_ready) return fail(-3, "cufhe_amd_lvl2_initialize has not been called for this device");
    if (!tlwe0 || !acc) return fail(-1, "null pointer");
    if (steps < 0 || steps > kLvl0N) steps = kLvl0N;
    hipStream_t st = (hipStream_t)stream;
    return direct_batch(s, st, count, [&](size_t g) { return RotDesc2{tlwe0 + g * kLvl0Words, tlwe0 + g * kLvl0Words, nullptr, 1, 0, 0u, 0u}; },
                        [&](const RotDesc2* d) { return launch_blind_rotate_lvl2(s, st, d, count, steps, acc); });
}

int cufhe_amd_lvl2_keyswitch_batch(int device, void* stream, size_t count, const uint64_t* tlwe2, uint32_t* tlwe0)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    if (!s.keys2_ready) return fail(-3, "cufhe_amd_lvl2_initialize has not been called for this device");
    if (!tlwe0 || !tlwe2) return fail(-1, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    return direct_batch(s, st, count, [&](size_t g) { return LinDesc64{tlwe2 + g * k2Words, tlwe2 + g * k2Words, tlwe0 + g * kLvl0Words, 1, 0, 0ull}; },
                        [&](const LinDesc64* d) { return launch_keyswitch_lvl2(s, st, d, count); });
}

}  // extern "C"
