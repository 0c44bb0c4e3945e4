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

// The ring's table of test vectors on device `device`: kMaxUserGates2 rows of the users' definitions and, behind them, the library's own
// row kCbRow2 -- the test vector of the one-rotation circuit bootstrap, TV[4 q + r] = 2^(63 - 6 (r + 1)) for r < l = 3 and TV[4 q + 3] = 0.
// Allocated with the first definition, by cufhe_amd_cb_initialize or by the first one-rotation circuit bootstrap; CleanUp frees it.
// The device of `s` is the calling thread's current device.
std::mutex g_tvs2_mu;
int ensure_tvs2(DeviceState& s)
{
    std::lock_guard<std::mutex> lk(g_tvs2_mu);
    if (s.tvs2) return 0;
    DevPtr<uint64_t> t;
    HIP_TRY(t.alloc((size_t)kTvRows2 * k2N));
    std::vector<uint64_t> row((size_t)k2N);
    for (int i = 0; i < k2N; i++) row[(size_t)i] = (i & 3) < 3 ? 1ull << (63 - 6 * ((i & 3) + 1)) : 0ull;
    HIP_TRY(hipMemcpy(t.p + (size_t)kCbRow2 * k2N, row.data(), k2N * sizeof(uint64_t), hipMemcpyHostToDevice));
    s.tvs2 = t.release();
    return 0;
}

// tv_rows: a descriptor names a row of the lvl2 user gates' table (pad >= kPadRow2): the launch runs the <true> instantiation, which
// also handles constant pads; every other launch (built-in gates, circuit bootstrapping) runs <false>, the kernels as they were
int launch_blind_rotate_lvl2(DeviceState& s, hipStream_t st, const RotDesc2* d, size_t count, int steps, uint64_t* acc_dump, bool tv_rows)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, false};
    if (int rc = prof.begin()) return rc;
    if (plan::lvl2_quarters(count, cus_of(s), g_tuning)) {
        // four quarter waves per rotation, two rotations per CU (kernels_lvl2q.hip.h)
        if (!s.br2q_lds_opt_in) {
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2q_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kQLdsBytes));
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2q_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kQLdsBytes));
            s.br2q_lds_opt_in = true;
        }
        hipLaunchKernelGGL(tv_rows ? blind_rotate_lvl2q_kernel<true> : blind_rotate_lvl2q_kernel<false>, dim3((unsigned)count), dim3(kQThreads),
                           kQLdsBytes, st, d, (int)count, s.bk2q_ntt, s.tables2q, steps, acc_dump, s.tvs2);
    } else {
        if (int rc = ensure_bk2_half_layout(s)) return rc;
        if (!s.br2_lds_opt_in) {
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, k3LdsBytes));
            HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_lvl2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, k3LdsBytes));
            s.br2_lds_opt_in = true;
        }
        hipLaunchKernelGGL(tv_rows ? blind_rotate_lvl2_kernel<true> : blind_rotate_lvl2_kernel<false>, dim3((unsigned)count), dim3(k2Threads),
                           k3LdsBytes, st, d, (int)count, s.bk2_ntt, s.tables2, steps, acc_dump, s.tvs2);
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
    static constexpr bool lvl1_gates = false, rotate_takes_tv_rows = true;
    // the ring's own definitions (cufhe_amd_lvl2_define_gate) alone run here: the registry's rule
    static constexpr opreg::Path path = opreg::Path::Ring;
    static constexpr int set_index = -1;
    static constexpr uint32_t pad(int row, int s) { return make_pad2(row, s); }
    DeviceState& s;
    int ready() const { return s.keys2_ready ? 0 : fail(-3, "cufhe_amd_lvl2_initialize has not been called for this device"); }
    int rotate(hipStream_t st, const RotDesc2* d, size_t count, int steps, uint64_t* dump, bool tv_rows) const { return launch_blind_rotate_lvl2(s, st, d, count, steps, dump, tv_rows); }
    int keyswitch(hipStream_t st, const LinDesc64* d, size_t count) const { return launch_keyswitch_lvl2(s, st, d, count); }
};

template <class GetGate>
int run_gates_lvl2(int device, void* stream, size_t count, GetGate get)
{
    if (int rc = use_device(device)) return rc;
    return lower_gates(Lvl2Path{g_dev[device]}, (hipStream_t)stream, 0, count, get);
}

// The parity hooks of the lvl2 user gates: `count` evaluations of definition `op` on [count][n + 1] arrays, with the rotation
// descriptors of the gate path (lower_gates: arity, the pre-added c0 in0 + c1 in1 of three operands, the pad) and another tail: the
// accumulator after `steps` steps (acc), or the sample-extracted lvl2 TLWE without its key switch (tlwe2).  Of a multi-output
// definition acc takes output 0's id (the one accumulator); tlwe2 takes any output id: the rotations write all nout outputs to scratch
// and output j alone is copied to the caller's [count][N2 + 1].
int lvl2_user_rotations(int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                        int steps, uint64_t* acc, uint64_t* tlwe2)
{
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    const opreg::Admission adm = opreg::admit(g_ops, op, opreg::Route{opreg::Path::Ring, -1, 0, g_param_set >= 0}, opreg::Entry::Lvl2Hook);
    if (!adm) return refuse(adm.refusal);
    const UserGate* u = adm.gate;
    const int out_j = adm.j;
    if (acc && out_j != 0) return fail(-1, "the accumulator of a multi-output definition is dumped under output 0's id");
    if (!s.keys2_ready) return fail(-3, "cufhe_amd_lvl2_initialize has not been called for this device");
    if (!in0 || (!acc && !tlwe2)) return fail(-1, "null pointer");
    if (const char* missing = opreg::missing_operand(*u, in1 != nullptr, in2 != nullptr)) return fail(-1, missing);
    const int arity = user_gate_arity(*u);
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc;
    const bool multi = u->nout > 1;
    const size_t multi_bytes = multi && tlwe2 ? count * (size_t)u->nout * k2Words * sizeof(uint64_t) : 0;
    if (int rc = open_scratch(s, st, multi_bytes + count * (sizeof(RotDesc2) + 2 * sizeof(LinDesc) + (arity == 3 ? kLvl0Words * sizeof(uint32_t) : 0)) + 8192, &sc))
        return rc;
    uint32_t* tmpp = nullptr;
    if (arity == 3)
        if (int rc = sc.alloc((void**)&tmpp, count * kLvl0Words * sizeof(uint32_t))) return rc;
    uint64_t* all = nullptr;          // a multi-output definition: [count][nout][N2 + 1], of which output out_j reaches tlwe2
    if (multi_bytes)
        if (int rc = sc.alloc((void**)&all, multi_bytes)) return rc;
    const uint32_t pad = u->tv ? Lvl2Path::pad(adm.k, u->s) : 0u;
    std::vector<RotDesc2> rot(count);
    std::vector<LinDesc> pre;
    for (size_t g = 0; g < count; g++) {
        const size_t w = g * kLvl0Words;
        const opreg::GateOperands x = opreg::user_gate_operands(*u, in0 + w, in1 ? in1 + w : nullptr, in2 ? in2 + w : nullptr, [&] { return tmpp + w; }, pre);
        uint64_t* o = !tlwe2 ? nullptr : multi ? all + g * (size_t)u->nout * k2Words : tlwe2 + g * k2Words;
        rot[g] = RotDesc2{x.a, x.b, o, x.ca, x.cb, u->off, pad};
    }
    RotDesc2* drot;
    LinDesc* dpre;
    if (int rc = upload_descs(s, sc, rot, &drot)) return rc;
    if (int rc = upload_descs(s, sc, pre, &dpre)) return rc;
    if (int rc = launch_lincomb(st, dpre, pre.size(), kLvl0Words)) return rc;
    if (int rc = launch_blind_rotate_lvl2(s, st, drot, count, steps, acc, pad != 0)) return rc;
    if (!all) return 0;
    // output out_j of every evaluation: a copy of 2 (N2 + 1) 32-bit words
    std::vector<LinDesc> cp(count);
    for (size_t g = 0; g < count; g++) {
        const uint32_t* src = (const uint32_t*)(all + (g * (size_t)u->nout + (size_t)out_j) * k2Words);
        cp[g] = LinDesc{src, src, (uint32_t*)(tlwe2 + g * k2Words), 1, 0, 0u, 0u};
    }
    LinDesc* dcp;
    if (int rc = upload_descs(s, sc, cp, &dcp)) return rc;
    return launch_lincomb(st, dcp, cp.size(), 2 * k2Words);
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

// a lvl2 user gate with nout = 2^sh outputs (1: cufhe_amd_lvl2_define_gate); the caller holds g_mu
static int define_lvl2_user_gate(const int32_t coeffs[3], uint32_t offset, const uint64_t* test_vector, int sh, int* op)
{
    if (!coeffs || !op) return fail(-1, "null pointer");
    if (coeffs[0] == 0) return fail(-1, "lvl2 user gate: c0 must not be 0");
    if (g_param_set >= 0) return fail(-1, "lvl2 user gates run on the N = 2048 ring only: not while \"param_set\" is active");
    // the ring's table holds the library's own rows too, so it exists on every device whether or not this definition has a test vector
    return define_op(g_ops.lvl2, make_user_gate(coeffs, offset, test_vector != nullptr, sh), [](int i) { return g_dev[i].keys2_ready; },
                     "cufhe_amd_lvl2_initialize has not been called for every device",
                     "lvl2 user gate table full (CUFHE_AMD_LVL2_MAX_USER_GATES definitions until CleanUp)",
                     true, [&](int i, int k) {
                         if (int rc = ensure_tvs2(g_dev[i])) return rc;
                         return test_vector ? write_tv_row(&g_dev[i].tvs2, kTvRows2, k2N, k, test_vector) : 0;
                     }, op);
}

int cufhe_amd_lvl2_define_gate(const int32_t coeffs[3], uint32_t offset, const uint64_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return define_lvl2_user_gate(coeffs, offset, test_vector, 0, op);
}

int cufhe_amd_lvl2_define_gate_multi(const int32_t coeffs[3], uint32_t offset, int nout, const uint64_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (nout != 2 && nout != 4 && nout != 8) return fail(-1, "multi-output lvl2 user gate: nout must be 2, 4 or 8");
    if (!test_vector) return fail(-1, "multi-output lvl2 user gate: the test vector is required (cufhe_amd_lvl2_test_vector_multi)");
    return define_lvl2_user_gate(coeffs, offset, test_vector, nout == 2 ? 1 : nout == 4 ? 2 : 3, op);
}

int cufhe_amd_lvl2_test_vector(const uint64_t* values, int p, uint64_t* tv)
{
    if (!values || !tv) return fail(-1, "null pointer");
    if (p < 2 || p > k2N / 2 || (p & (p - 1))) return fail(-1, "p must be a power of two in [2, N2/2]");
    // the boxes of cufhe_amd_test_vector on N2 coefficients: m = round(j p / N2), the top half-box (m = p) holds -values[0]
    const int box = k2N / p;
    for (int j = 0; j < k2N; j++) {
        const int m = (j + box / 2) / box;
        tv[j] = m == p ? 0ull - values[0] : values[m];
    }
    return 0;
}

int cufhe_amd_lvl2_test_vector_multi(const uint64_t* values, int p, int nout, uint64_t* tv)
{
    if (!values || !tv) return fail(-1, "null pointer");
    if (nout != 1 && nout != 2 && nout != 4 && nout != 8) return fail(-1, "nout must be 1, 2, 4 or 8");
    if (p < 2 || (p & (p - 1)) || p * nout > k2N / 2) return fail(-1, "p must be a power of two >= 2 with p nout <= N2/2");
    // TV[nout q + j] = values[j][m], m the box of position nout q under cufhe_amd_lvl2_test_vector's boxes (the top half-box: -values[j][0])
    const int box = k2N / p;
    for (int q = 0; q < k2N / nout; q++) {
        const int m = (nout * q + box / 2) / box;
        for (int j = 0; j < nout; j++) {
            const uint64_t* v = values + (size_t)j * p;
            tv[nout * q + j] = m == p ? 0ull - v[0] : v[m];
        }
    }
    return 0;
}

int cufhe_amd_lvl2_user_rotate_batch(int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1,
                                     const uint32_t* in2, int steps, uint64_t* acc)
{
    if (!acc) return fail(-1, "null pointer");
    if (steps < 0 || steps > kLvl0N) steps = kLvl0N;
    return lvl2_user_rotations(device, stream, count, op, in0, in1, in2, steps, acc, nullptr);
}

int cufhe_amd_lvl2_user_extract_batch(int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1,
                                      const uint32_t* in2, uint64_t* tlwe2)
{
    if (!tlwe2) return fail(-1, "null pointer");
    return lvl2_user_rotations(device, stream, count, op, in0, in1, in2, kLvl0N, nullptr, tlwe2);
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
                        [&](const RotDesc2* d) { return launch_blind_rotate_lvl2(s, st, d, count, steps, acc, false); });
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
