// paramsets.inc.h -- host side of the parameter-set-generic gate path (kernels_ps.hip.h); included by
// capi.hip.  The reference chooses its parameter set when it is built (CMakeLists.txt:8-24); here every
// set of kernels_ps.hip.h is compiled in and chosen by index at run time ("param_set" puts the whole per-gate
// API on one, as the reference's build-time choice does).  Both gate orders of the reference: on lvl0 ciphertexts
// of the chosen set blind rotate -> sample extract -> key switch (__HomGate__ br -> iks, src/bootstrap_gpu.cu:402-421;
// Mux :515-588), on lvl1 ciphertexts (k N + 1 words) key switch of the linear combination -> blind rotate -> sample
// extract (__HomGate__ iks -> br, :383-400; Mux :706-780); Not / Copy :681-703.

namespace {

struct PsState {
    bool ready = false;
    OptInFlag lds_opt_in, lds_opt_in_tv, ks_lds_opt_in;
    double* bk_ntt = nullptr;
    uint32_t* ksk = nullptr;
    uint32_t* ksk_padded = nullptr;   // sets whose key switch has the default shape: rows padded for keyswitch_kernel
    uint32_t* tvs = nullptr;          // [kMaxUserGates][N]: the test vectors of the set's user gates (cufhe_amd_ps_define_gate), allocated
                                      // by the first definition that has one; kept when the set's keys are replaced, freed by CleanUp
};

// kN = 1024, n = 630, t = 8, basebit = 2: the hand-scheduled shared-table key switch of kernels.hip.h applies as it is
template <class PS>
constexpr bool ps_ks_is_default_shape = PS::k * PsDims<PS>::N == kN && PS::n == kLvl0N && PS::t == kKsT && PS::basebit == kKsBasebit;
static_assert(PsKs<PsDefault>::row_pad == kKsRowPad, "a set with the default key-switch shape shares keyswitch_kernel<KsShapeDefault>");

template <class PS>
int ps_launch_keyswitch(DeviceState& s, PsState& ps, hipStream_t st, const LinDesc* d, size_t count)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, true};
    if (int rc = prof.begin()) return rc;
    using Shape = std::conditional_t<ps_ks_is_default_shape<PS>, KsShapeDefault, KsShapePs<PS>>;
    const plan::KsPlan p = plan_keyswitch_of<Shape>(s, count, plan::KsRule{false, ps.ksk_padded != nullptr});
    if (p.kernel == plan::KsKernel::Shared) {
        if (int rc = launch_keyswitch_shared<Shape>(s, st, d, count, ps.ksk_padded, ps_ks_is_default_shape<PS> ? &s.ks_lds_opt_in : &ps.ks_lds_opt_in, p)) return rc;
    } else {
        hipLaunchKernelGGL(keyswitch_ps_kernel<PS>, dim3((unsigned)count), dim3(kKsThreads), 0, st, d, (int)count, ps.ksk);
    }
    HIP_TRY(hipGetLastError());
    return prof.commit();
}
PsState g_ps[kParamSets][kMaxLogicalDevices];

PsState& ps_state(int set, int device) { return g_ps[set][device]; }

// f(PS{}) for the set of index `set` in CompiledSets (capi.hip)
template <size_t I = 0, class F>
int ps_dispatch(int set, F&& f)
{
    if constexpr (I < std::tuple_size_v<CompiledSets>) {
        if (set == (int)I) return f(std::tuple_element_t<I, CompiledSets>{});
        return ps_dispatch<I + 1>(set, f);
    } else {
        return fail(-1, "unknown parameter set");
    }
}

template <class PS>
const typename Poly<PS::Nbit>::Tables* ps_tables(DeviceState& s)
{
    if constexpr (PS::Nbit == 10) return s.tables;
    else return s.tables512 + 2;            // the stand-alone 512-point negacyclic transform
}

// the wave-per-rotation kernel of a 1024-point set runs the radix-4 transform: its tables
template <class PS>
const typename Poly<PS::Nbit>::Tables* ps_tables_batch(DeviceState& s)
{
    if constexpr (PS::Nbit == 10) return PsbPolyOf<PS>::kR4Tables ? s.tables_r4 : s.tables;
    else return s.tables512 + 2;
}

// user: some descriptor of the launch is a user gate's (LinDesc::pad != 0): the <true> instantiations, which read pad and the set's
// table; every other launch runs the <false> ones
template <class PS, bool TV>
int ps_launch_blind_rotate_tv(DeviceState& s, PsState& ps, hipStream_t st, const LinDesc* d, size_t count, int steps, uint32_t* dump)
{
    OptInFlag& opt_in = TV ? ps.lds_opt_in_tv : ps.lds_opt_in;
    if (!opt_in) {
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ps_kernel<PS, TV>, hipFuncAttributeMaxDynamicSharedMemorySize, PsLds<PS>::bytes));
        HIP_TRY(hipFuncSetAttribute((const void*)blind_rotate_ps_batch_kernel<PS, TV>, hipFuncAttributeMaxDynamicSharedMemorySize, PsbLds<PS>::bytes));
        opt_in = true;
    }
    if (plan::ps_use_batch(count, PS::limbs, PS::Nbit, cus_of(s), g_tuning)) {
        // one wave per rotation, 8 rotations per workgroup share the key rows (throughput shape)
        const unsigned blocks = (unsigned)((count + PsbLds<PS>::waves - 1) / PsbLds<PS>::waves);
        hipLaunchKernelGGL((blind_rotate_ps_batch_kernel<PS, TV>), dim3(blocks), dim3(PsbLds<PS>::threads), PsbLds<PS>::bytes, st, d, (int)count,
                           ps.bk_ntt, ps_tables_batch<PS>(s), steps, dump, ps.tvs);
    } else {
        // one workgroup per rotation (latency shape)
        hipLaunchKernelGGL((blind_rotate_ps_kernel<PS, TV>), dim3((unsigned)count), dim3(PsLds<PS>::threads), PsLds<PS>::bytes, st, d, (int)count,
                           ps.bk_ntt, kPsWgR4 ? ps_tables_batch<PS>(s) : ps_tables<PS>(s), steps, dump, ps.tvs);
    }
    return 0;
}
template <class PS>
int ps_launch_blind_rotate(DeviceState& s, PsState& ps, hipStream_t st, const LinDesc* d, size_t count, int steps, uint32_t* dump, bool user)
{
    if (count == 0) return 0;
    ProfScope prof{s, st, count, false};
    if (int rc = prof.begin()) return rc;
    if (int rc = user ? ps_launch_blind_rotate_tv<PS, true>(s, ps, st, d, count, steps, dump) : ps_launch_blind_rotate_tv<PS, false>(s, ps, st, d, count, steps, dump))
        return rc;
    HIP_TRY(hipGetLastError());
    return prof.commit();
}

// CMUXNTT on a set (src/bootstrap_gpu.cu:197-285: in the reference the set chosen at build time serves it too; only its small-modulus
// build leaves it out, src/cufhe_gates_gpu.cu:68-86)
template <class PS>
int ps_launch_cmux(DeviceState& s, hipStream_t st, const CmuxDesc* d, size_t count)
{
    using PO = Poly<PS::Nbit>;
    if (count == 0) return 0;
    const unsigned blocks = (unsigned)((count + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
    hipLaunchKernelGGL(cmux_desc_ps_kernel<PS>, dim3(blocks), dim3(kNttThreads), PO::table_bytes + kNttWavesPerBlock * PO::tile_bytes, st, d,
                       (int)count, ps_tables<PS>(s));
    HIP_TRY(hipGetLastError());
    return 0;
}

// index of PS in CompiledSets: the `set` of the C ABI
template <class PS, size_t I = 0>
constexpr int ps_index_of()
{
    static_assert(I < std::tuple_size_v<CompiledSets>, "not a compiled parameter set");
    if constexpr (std::is_same_v<PS, std::tuple_element_t<I, CompiledSets>>) return (int)I;
    else return ps_index_of<PS, I + 1>();
}

// A parameter set for lower_gates / lower_trlwe_ops (capi.hip)
template <class PS>
struct PsPath {
    using D = PsDims<PS>;
    using RotD = LinDesc;
    using KsD = LinDesc;
    using Mid = uint32_t;
    static constexpr int lvl0_words = D::lvl0_words, mid_words = D::lvl1_words, n = PS::n;
    static constexpr uint32_t ks_mu = kMu;
    static constexpr bool lvl1_gates = true, has_cmux = !PS::small_modulus, packed_rom = false, rotate_takes_tv_rows = true;
    // the definitions made for this set (cufhe_amd_ps_define_gate) alone run here: the registry's rule
    static constexpr opreg::Path path = opreg::Path::Set;
    static constexpr int set_index = ps_index_of<PS>();
    static constexpr uint32_t pad(int row, int s) { return make_pad(row, s); }
    static constexpr size_t trlwe_words = (size_t)D::K1 * D::N;
    static constexpr auto se_kernel = sample_extract_ps_kernel<PS>;
    DeviceState& s;
    PsState& ps;
    int ready() const { return ps.ready ? 0 : fail(-3, "cufhe_amd_ps_initialize has not been called for this parameter set and device"); }
    // tv_rows: some descriptor names a test-vector row (lower_gates; false for every launch without user gates)
    int rotate(hipStream_t st, const LinDesc* d, size_t count, int steps, uint32_t* dump, bool tv_rows = false) const
    {
        return ps_launch_blind_rotate<PS>(s, ps, st, d, count, steps, dump, tv_rows);
    }
    int keyswitch(hipStream_t st, const LinDesc* d, size_t count) const { return ps_launch_keyswitch<PS>(s, ps, st, d, count); }
    int cmux(hipStream_t st, const CmuxDesc* d, size_t count) const { return ps_launch_cmux<PS>(s, st, d, count); }
};

template <class GetGate>
int run_gates_ps(int set, int device, void* stream, int level, size_t count, GetGate get)
{
    return ps_dispatch(set, [&](auto psx) -> int {
        if (int rc = use_device(device)) return rc;
        return lower_gates(PsPath<decltype(psx)>{g_dev[device], ps_state(set, device)}, (hipStream_t)stream, level, count, get);
    });
}

int run_trlwe_ops_ps(int set, int device, void* stream, const GateRef* g, size_t n)
{
    return ps_dispatch(set, [&](auto psx) -> int {
        if (int rc = use_device(device)) return rc;
        return lower_trlwe_ops(PsPath<decltype(psx)>{g_dev[device], ps_state(set, device)}, (hipStream_t)stream, g, n);
    });
}

// words of a level-0 / level-1 ciphertext, (level 2) a TRLWE or (level 3) a TRGSW in the NTT domain (uint32 words: two per double) of a set
int ps_ctxt_words(int set, int level)
{
    int w = 0;
    (void)ps_dispatch(set, [&](auto psx) {
        using D = PsDims<decltype(psx)>;
        w = level == 3 ? (int)(2 * D::bk_ntt_step_doubles) : level == 2 ? D::K1 * D::N : level ? D::lvl1_words : D::lvl0_words;
        return 0;
    });
    return w;
}

// TRGSW2NTT on host memory over a set (cufhe_amd_trgsw_to_ntt_host while "param_set" is active): the same staging as the BASELINE
// path, the set's sizes and key-conversion kernel (limbs included)
int ps_trgsw_to_ntt_host(int set, int device, void* stream, const uint32_t* trgsw_host, double* trgsw_ntt_host)
{
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        using PO = Poly<PS::Nbit>;
        if (PS::small_modulus) return fail(-1, "TRGSW2NTT: the small-modulus build of the reference has none (src/bootstrap_gpu.cu:73-95)");
        DeviceState& s = g_dev[device];
        hipStream_t st = (hipStream_t)stream;
        constexpr size_t in_bytes = D::bk_step_polys * D::N * sizeof(uint32_t), out_bytes = D::bk_ntt_step_doubles * sizeof(double);
        Scratch sc;
        if (int rc = open_scratch(s, st, in_bytes + out_bytes + 4096, &sc)) return rc;
        uint32_t* d_in;
        double* d_out;
        if (int rc = sc.alloc((void**)&d_in, in_bytes)) return rc;
        if (int rc = sc.alloc((void**)&d_out, out_bytes)) return rc;
        PinnedBlock* blk = nullptr;
        if (int rc = acquire_staging(s, in_bytes + out_bytes, &blk)) return rc;
        StagingOwner owner{s, blk};
        staging_hold(s, blk, true);          // the host reads the result out of the block after the stream has finished with it
        memcpy(blk->host, trgsw_host, in_bytes);
        HIP_TRY(hipMemcpyAsync(d_in, blk->host, in_bytes, hipMemcpyHostToDevice, st));
        const size_t waves = D::bk_step_polys * PS::limbs;
        hipLaunchKernelGGL(bk_to_ntt_ps_kernel<PS>, dim3((unsigned)((waves + kNttWavesPerBlock - 1) / kNttWavesPerBlock)), dim3(kNttThreads),
                           PO::table_bytes + kNttWavesPerBlock * PO::tile_bytes, st, d_out, d_in, (size_t)D::bk_step_polys, ps_tables<PS>(s),
                           n_inverse(D::N));
        HIP_TRY(hipGetLastError());
        char* pin_out = (char*)blk->host + in_bytes;
        HIP_TRY(hipMemcpyAsync(pin_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        if (int rc = staging_done_after(s, blk, st)) return rc;
        owner.recorded();
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(trgsw_ntt_host, pin_out, out_bytes);
        return device_fault(device);
    });
}

void ps_release(int device)
{
    for (int set = 0; set < kParamSets; set++) {
        PsState& ps = ps_state(set, device);
        if (!ps.ready) continue;
        (void)hipFree(ps.bk_ntt);
        (void)hipFree(ps.ksk);
        if (ps.ksk_padded) (void)hipFree(ps.ksk_padded);
        if (ps.tvs) (void)hipFree(ps.tvs);
        ps = PsState{};
    }
}

// a user gate of parameter set `set` with nout = 2^sh outputs (1: cufhe_amd_ps_define_gate); the caller holds g_mu
int define_ps_user_gate(int set, const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector, int sh, int* op)
{
    if (!coeffs || !op) return fail(-1, "null pointer");
    if (coeffs[0] == 0) return fail(-1, "parameter set user gate: c0 must not be 0");
    return ps_dispatch(set, [&](auto psx) -> int {
        constexpr size_t N = PsDims<decltype(psx)>::N;
        return define_op(g_ops.ps, opreg::PsUserGate{make_user_gate(coeffs, offset, test_vector != nullptr, sh), set},
                         [&](int i) { return ps_state(set, i).ready; },
                         "cufhe_amd_ps_initialize has not been called for this parameter set on every device",
                         "parameter set user gate table full (CUFHE_AMD_PS_MAX_USER_GATES definitions until CleanUp)",
                         test_vector != nullptr, [&](int i, int k) { return write_tv_row(&ps_state(set, i).tvs, kMaxUserGates, N, k, test_vector); }, op);
    });
}

}  // namespace

extern "C" {

int cufhe_amd_ps_count(void) { return kParamSets; }

int cufhe_amd_ps_get_params(int set, cufhe_amd_ps_params* p)
{
    if (!p) return fail(-1, "null");
    return ps_dispatch(set, [&](auto ps) {
        using PS = decltype(ps);
        using D = PsDims<PS>;
        memset(p, 0, sizeof(*p));
        strncpy(p->name, PS::name, sizeof(p->name) - 1);
        p->n = PS::n; p->N = D::N; p->nbit = PS::Nbit; p->k = PS::k; p->l = PS::l; p->Bgbit = PS::Bgbit;
        p->t = PS::t; p->basebit = PS::basebit; p->key_limbs = PS::limbs; p->key_limb_bits = PS::limb_bits; p->mu = kMu;
        p->lvl0_words = D::lvl0_words; p->lvl1_words = D::lvl1_words;
        p->bk_words = D::bk_words; p->ksk_words = D::ksk_words;
        p->bk_ntt_bytes = (uint64_t)PS::n * D::bk_ntt_step_doubles * sizeof(double);
        p->small_ntt_modulus = PS::small_modulus ? smallmod::P : 0u;
        return 0;
    });
}

int cufhe_amd_ps_initialize(int set, const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!bk || !ksk) return fail(-1, "null key pointer");
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        using PO = Poly<PS::Nbit>;
        if (bk_words != D::bk_words) return fail(-1, "bootstrapping key has the wrong size for this parameter set");
        if (ksk_words != D::ksk_words) return fail(-1, "key-switching key has the wrong size for this parameter set");
        // build first, swap last (as cufhe_amd_initialize): a failure leaves every device with the keys of this set it had
        struct Built { DevPtr<double> bk_ntt; DevPtr<uint32_t> ksk, ksk_padded, d_bk; };
        std::vector<Built> built((size_t)g_gpu_num);      // the torus-domain staging copies d_bk are freed on every return
        for (int i = 0; i < g_gpu_num; i++) {
            if (int rc = ensure_ntt(i)) return rc;
            DeviceState& s = g_dev[i];
            Built& b = built[(size_t)i];
            HIP_TRY(hipSetDevice(phys_device(i)));
            HIP_TRY(b.bk_ntt.alloc((size_t)PS::n * D::bk_ntt_step_doubles));
            HIP_TRY(b.ksk.alloc(D::ksk_words));
            HIP_TRY(hipMemcpy(b.ksk.p, ksk, D::ksk_words * sizeof(uint32_t), hipMemcpyHostToDevice));
            // the same table with rows padded to a multiple of 64 words, for the shared-table kernels
            if (int rc = upload_ksk_padded(b.ksk_padded, ksk, D::ksk_words / D::lvl0_words, D::lvl0_words, PsKs<PS>::row_pad)) return rc;
            HIP_TRY(b.d_bk.alloc(D::bk_words));
            HIP_TRY(hipMemcpy(b.d_bk.p, bk, D::bk_words * sizeof(uint32_t), hipMemcpyHostToDevice));
            const size_t polys = D::bk_words / D::N, waves = polys * PS::limbs;
            const unsigned blocks = (unsigned)((waves + kNttWavesPerBlock - 1) / kNttWavesPerBlock);
            hipLaunchKernelGGL(bk_to_ntt_ps_kernel<PS>, dim3(blocks), dim3(kNttThreads), PO::table_bytes + kNttWavesPerBlock * PO::tile_bytes, 0,
                               b.bk_ntt.p, b.d_bk.p, polys, ps_tables<PS>(s), n_inverse(D::N));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());        // also: nothing on this device still reads the keys that are about to go
        }
        for (int i = 0; i < g_gpu_num; i++) {
            PsState& ps = ps_state(set, i);
            (void)hipSetDevice(phys_device(i));
            if (ps.ready) {
                (void)hipFree(ps.bk_ntt);
                (void)hipFree(ps.ksk);
                if (ps.ksk_padded) (void)hipFree(ps.ksk_padded);
            }
            Built& b = built[(size_t)i];
            uint32_t* tvs = ps.tvs;              // the set's user gates outlive a change of its keys
            ps = PsState{};
            ps.tvs = tvs;
            ps.bk_ntt = b.bk_ntt.release();
            ps.ksk = b.ksk.release();
            ps.ksk_padded = b.ksk_padded.release();
            ps.ready = true;
        }
        return 0;
    });
}

/* The reference has ONE selector for its parameters: TFHEpp's macro fixes the numbers and every kernel is a template over them
 * (CMakeLists.txt:8-24, include/bootstrap_gpu.cuh:51-53).  Here the caller hands over the numbers it was compiled with and the
 * library picks the compiled set that has exactly those -- key SIZES alone do not see Bgbit, and t * 2^(basebit-1) is 16 for both
 * (8, 2) and (4, 3). */
int cufhe_amd_find_param_set(const cufhe_amd_param_numbers* q)
{
    if (!q) return fail(-1, "null");
    for (int set = 0; set < kParamSets; set++) {
        cufhe_amd_ps_params p;
        if (cufhe_amd_ps_get_params(set, &p)) continue;
        if (p.n == q->n && p.nbit == q->nbit && p.k == q->k && p.l == q->l && p.Bgbit == q->Bgbit && p.t == q->t && p.basebit == q->basebit &&
            p.small_ntt_modulus == q->small_ntt_modulus)
            return set;
    }
    char buf[320];
    snprintf(buf, sizeof buf, "no compiled parameter set has n=%u nbit=%u k=%u l=%u Bgbit=%u t=%u basebit=%u small_ntt_modulus=%u "
             "(cufhe_amd_ps_get_params lists the compiled sets)", q->n, q->nbit, q->k, q->l, q->Bgbit, q->t, q->basebit, q->small_ntt_modulus);
    return fail(-1, buf);
}

int cufhe_amd_initialize_params(const cufhe_amd_param_numbers* numbers, const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words)
{
    const int set = cufhe_amd_find_param_set(numbers);
    if (set < 0) return set;
    if (set == 0) {        // the BASELINE numbers: the hand-scheduled kernels
        if (int rc = cufhe_amd_initialize(bk, bk_words, ksk, ksk_words)) return rc;
        return cufhe_amd_set_option("param_set", -1);
    }
    if (int rc = cufhe_amd_initialize_ntt()) return rc;
    if (int rc = cufhe_amd_ps_initialize(set, bk, bk_words, ksk, ksk_words)) return rc;
    return cufhe_amd_set_option("param_set", set);
}

int cufhe_amd_ps_gate_batch_level(int set, int device, void* stream, int level, size_t count, const int32_t* ops, int ops_stride,
                                  uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, size_t stride_words)
{
    if (!ops) return fail(-1, "null ops");
    return run_gates_ps(set, device, stream, level, count, [&](size_t g) {
        return GateRef{ops[g * (size_t)ops_stride], out + g * stride_words, in0 ? in0 + g * stride_words : nullptr,
                       in1 ? in1 + g * stride_words : nullptr, in2 ? in2 + g * stride_words : nullptr};
    });
}

int cufhe_amd_ps_gate_batch(int set, int device, void* stream, size_t count, const int32_t* ops, int ops_stride,
                            uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, size_t stride_words)
{
    return cufhe_amd_ps_gate_batch_level(set, device, stream, 0, count, ops, ops_stride, out, in0, in1, in2, stride_words);
}

int cufhe_amd_ps_blind_rotate_batch(int set, int device, void* stream, size_t count, const uint32_t* tlwe0, uint32_t* acc, int steps)
{
    if (int rc = use_device(device)) return rc;
    if (!tlwe0 || !acc) return fail(-1, "null pointer");
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        const PsPath<PS> p{g_dev[device], ps_state(set, device)};
        if (int rc = p.ready()) return rc;
        const int st_steps = (steps < 0 || steps > PS::n) ? PS::n : steps;
        hipStream_t st = (hipStream_t)stream;
        return direct_batch(p.s, st, count, [&](size_t g) { return LinDesc{tlwe0 + g * D::lvl0_words, tlwe0 + g * D::lvl0_words, nullptr, 1, 0, 0u, 0u}; },
                            [&](const LinDesc* d) { return p.rotate(st, d, count, st_steps, acc); });
    });
}

int cufhe_amd_ps_define_gate(int set, const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return define_ps_user_gate(set, coeffs, offset, test_vector, 0, op);
}

int cufhe_amd_ps_define_gate_multi(int set, const int32_t coeffs[3], uint32_t offset, int nout, const uint32_t* test_vector, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (nout != 2 && nout != 4 && nout != 8) return fail(-1, "multi-output user gate of a parameter set: nout must be 2, 4 or 8");
    if (!test_vector) return fail(-1, "multi-output user gate of a parameter set: the test vector is required (cufhe_amd_ps_test_vector_multi)");
    return define_ps_user_gate(set, coeffs, offset, test_vector, nout == 2 ? 1 : nout == 4 ? 2 : 3, op);
}

int cufhe_amd_ps_test_vector_multi(int set, const uint32_t* values, int p, int nout, uint32_t* tv)
{
    if (!values || !tv) return fail(-1, "null pointer");
    if (nout != 1 && nout != 2 && nout != 4 && nout != 8) return fail(-1, "nout must be 1, 2, 4 or 8");
    return ps_dispatch(set, [&](auto psx) -> int {
        constexpr int N = PsDims<decltype(psx)>::N;
        if (p < 2 || (p & (p - 1)) || p > N / 2 || p * nout > N / 2) return fail(-1, "p must be a power of two >= 2 with p nout <= N/2 of the parameter set");
        // the boxes of cufhe_amd_test_vector_multi on the set's N: TV[nout q + j] = values[j][m], m the box of position nout q (the top
        // half-box, m = p, is the wrap of m = 0's lower half: -values[j][0])
        const int box = N / p;
        for (int q = 0; q < N / nout; q++) {
            const int m = (nout * q + box / 2) / box;
            for (int j = 0; j < nout; j++) {
                const uint32_t* v = values + (size_t)j * p;
                tv[nout * q + j] = m == p ? 0u - v[0] : v[m];
            }
        }
        return 0;
    });
}

int cufhe_amd_ps_test_vector(int set, const uint32_t* values, int p, uint32_t* tv) { return cufhe_amd_ps_test_vector_multi(set, values, p, 1, tv); }

/* The parity hook of a set's user gates: `count` evaluations of definition `op` on [count][n + 1] lvl0 arrays with the rotation
 * descriptors of the gate path (lower_gates: arity, the pre-added c0 in0 + c1 in1 of three operands, the pad); acc[count][(k+1) N]
 * receives the accumulators after `steps` CMux steps (negative: all).  A multi-output definition is named by output 0's id. */
int cufhe_amd_ps_user_rotate(int set, int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1,
                             const uint32_t* in2, uint32_t* acc, int steps)
{
    if (int rc = use_device(device)) return rc;
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using P = PsPath<PS>;
        constexpr size_t w0 = P::lvl0_words;
        const opreg::Admission adm = opreg::admit(g_ops, op, opreg::Route{opreg::Path::Set, set, 0, g_param_set >= 0}, opreg::Entry::PsHook);
        if (!adm) return refuse(adm.refusal);
        const UserGate* u = adm.gate;
        if (adm.j != 0) return fail(-1, "the accumulator of a multi-output definition is dumped under output 0's id");
        const P p{g_dev[device], ps_state(set, device)};
        if (int rc = p.ready()) return rc;
        if (!in0 || !acc) return fail(-1, "null pointer");
        if (const char* missing = opreg::missing_operand(*u, in1 != nullptr, in2 != nullptr)) return fail(-1, missing);
        const int arity = user_gate_arity(*u);
        if (count == 0) return 0;
        hipStream_t st = (hipStream_t)stream;
        Scratch sc;
        if (int rc = open_scratch(p.s, st, count * (2 * sizeof(LinDesc) + (arity == 3 ? w0 * sizeof(uint32_t) : 0)) + 8192, &sc)) return rc;
        uint32_t* tmpp = nullptr;
        if (arity == 3)
            if (int rc = sc.alloc((void**)&tmpp, count * w0 * sizeof(uint32_t))) return rc;
        const uint32_t pad = u->tv ? P::pad(adm.k, u->s) : 0u;
        std::vector<LinDesc> rot(count), pre;
        for (size_t g = 0; g < count; g++) {
            const size_t w = g * w0;
            const opreg::GateOperands x = opreg::user_gate_operands(*u, in0 + w, in1 ? in1 + w : nullptr, in2 ? in2 + w : nullptr, [&] { return tmpp + w; }, pre);
            rot[g] = LinDesc{x.a, x.b, nullptr, x.ca, x.cb, u->off, pad};
        }
        LinDesc *drot, *dpre;
        if (int rc = upload_descs(p.s, sc, rot, &drot)) return rc;
        if (int rc = upload_descs(p.s, sc, pre, &dpre)) return rc;
        if (int rc = launch_lincomb(st, dpre, pre.size(), (int)w0)) return rc;
        return p.rotate(st, drot, count, (steps < 0 || steps > PS::n) ? PS::n : steps, acc, pad != 0);
    });
}

int cufhe_amd_ps_trlwe_op_batch(int set, int device, void* stream, int op, size_t count, uint32_t* out, const uint32_t* in)
{
    if (!out || !in) return fail(-1, "null pointer");
    if (op != CUFHE_AMD_TL_BOOTSTRAP && op != CUFHE_AMD_TL_REFRESH && op != CUFHE_AMD_TL_SEIKS) return fail(-1, "unknown TRLWE-level op");
    const size_t w0 = (size_t)ps_ctxt_words(set, 0), wt = (size_t)ps_ctxt_words(set, 2);
    if (!w0) return fail(-1, "unknown parameter set");
    const size_t win = op == CUFHE_AMD_TL_BOOTSTRAP ? w0 : wt, wout = op == CUFHE_AMD_TL_SEIKS ? w0 : wt;
    std::vector<GateRef> g(count);
    for (size_t i = 0; i < count; i++) g[i] = GateRef{op, out + i * wout, in + i * win, nullptr, nullptr};
    return run_trlwe_ops_ps(set, device, stream, g.data(), count);
}

/* TRGSW2NTT / CMUXNTT on a set, device-resident (src/bootstrap_gpu.cu:75-94,197-285 instantiated for the set the build selected):
 * trgsw[count][(k+1)l][k+1][N] torus words -> trgsw_ntt[count][limbs][(k+1)l][k+1][N] doubles; res = c0 + trgsw [x] (c1 - c0) on
 * TRLWEs [count][(k+1)N].  Needs Initialize() only. */
int cufhe_amd_ps_trgsw_to_ntt_batch(int set, int device, void* stream, size_t count, const uint32_t* trgsw, double* trgsw_ntt)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (!trgsw || !trgsw_ntt) return fail(-1, "null pointer");
    if (count == 0) return 0;
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        using PO = Poly<PS::Nbit>;
        if (PS::small_modulus) return fail(-1, "TRGSW2NTT: the small-modulus build of the reference has none (src/bootstrap_gpu.cu:73-95)");
        const size_t polys = count * D::bk_step_polys, waves = polys * PS::limbs;
        hipLaunchKernelGGL(bk_to_ntt_ps_kernel<PS>, dim3((unsigned)((waves + kNttWavesPerBlock - 1) / kNttWavesPerBlock)), dim3(kNttThreads),
                           PO::table_bytes + kNttWavesPerBlock * PO::tile_bytes, (hipStream_t)stream, trgsw_ntt, trgsw, polys,
                           ps_tables<PS>(g_dev[device]), n_inverse(D::N));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int cufhe_amd_ps_cmux_batch(int set, int device, void* stream, size_t count, const double* trgsw_ntt, const uint32_t* c1,
                            const uint32_t* c0, uint32_t* res)
{
    if (int rc = use_device(device)) return rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (int rc = ensure_ntt(device)) return rc;
    }
    if (!trgsw_ntt || !c1 || !c0 || !res) return fail(-1, "null pointer");
    if (count == 0) return 0;
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        if constexpr (PS::small_modulus) {
            return fail(-1, "CMUXNTT: the small-modulus build of the reference has none (src/cufhe_gates_gpu.cu:68-86)");
        } else {
            constexpr size_t tw = (size_t)D::K1 * D::N;
            return trlwe_batch(PsPath<PS>{g_dev[device], ps_state(set, device)}, (hipStream_t)stream, count, [&](size_t g) {
                return GateRef{CUFHE_AMD_TL_CMUX, res + g * tw, c1 + g * tw, c0 + g * tw, (const uint32_t*)(trgsw_ntt + g * D::bk_ntt_step_doubles)};
            });
        }
    });
}

int cufhe_amd_ps_keyswitch_batch(int set, int device, void* stream, size_t count, const uint32_t* tlwe1, uint32_t* tlwe0)
{
    if (int rc = use_device(device)) return rc;
    if (!tlwe0 || !tlwe1) return fail(-1, "null pointer");
    return ps_dispatch(set, [&](auto psx) -> int {
        using PS = decltype(psx);
        using D = PsDims<PS>;
        const PsPath<PS> p{g_dev[device], ps_state(set, device)};
        if (int rc = p.ready()) return rc;
        if (count == 0) return 0;
        hipStream_t st = (hipStream_t)stream;
        return direct_batch(p.s, st, count, [&](size_t g) { return LinDesc{tlwe1 + g * D::lvl1_words, tlwe1 + g * D::lvl1_words, tlwe0 + g * D::lvl0_words, 1, 0, 0u, 0u}; },
                            [&](const LinDesc* d) { return p.keyswitch(st, d, count); });
    });
}

}  // extern "C"
