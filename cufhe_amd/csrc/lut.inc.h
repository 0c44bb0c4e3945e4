// lut.inc.h -- host side of the encrypted-table lookup (included by capi.hip): blind rotations whose initial
// accumulator is a caller's TRLWE (the table instantiations of the three default-path kernels, launch_blind_rotate with a table array),
// the lookup's key switch on the path the multi-output gates take at level 0, and the keyless Spread (kernels_lut.hip.h).  Default
// parameter set only.  The batch entry points are not recorded (callers order a call behind gates recorded on a stream with
// cufhe_amd_stream_fence); the recorded forms -- cufhe_amd_enqueue_lookup, _enqueue_spread, _enqueue_lut_rotate -- are scheduler nodes whose
// ops the HIP backend splits off a level's gate list (sched_hip.inc.h: HipBackend::run_gates) and hands to lower_lut_ops below: one
// rotation launch sequence, one key-switch launch and one Spread launch per dependence level.

namespace {

int fail_lut_set() { return fail(-1, "encrypted-table lookups (lut_rotate, lut_lookup, trlwe_spread) run on the default path only: not with \"param_set\" active"); }

bool ranges_overlap(const uint32_t* a, size_t a_words, const uint32_t* b, size_t b_words)
{
    return a_words && b_words && a < b + b_words && b < a + a_words;
}

// what both rotation entry points refuse before any device work; *shift = log2(nout)
int check_lut_args(const char* who, int device, size_t count, const uint32_t* tlwe0, const uint32_t* tables, size_t table_count, const int32_t* src,
                   int nout, const uint32_t* out, size_t out_words, int* shift)
{
    if (g_param_set >= 0) return fail_lut_set();
    if (int rc = check_device(device)) return rc;
    if (!tlwe0 || !tables || !out) return fail(-1, std::string(who) + ": null pointer");
    int s = 0;
    while (s <= kMaxOutputShift && (1 << s) != nout) s++;
    if (s > kMaxOutputShift) return fail(-1, std::string(who) + ": nout must be 1, 2, 4 or 8");
    if (count > (size_t)INT32_MAX / 8) return fail(-1, std::string(who) + ": count exceeds the index type of src");
    if (count && table_count == 0) return fail(-1, std::string(who) + ": table_count is 0");
    for (size_t g = 0; g < count; g++) {
        const long long t = src ? (long long)src[g] : (long long)g;
        if (t < 0 || (size_t)t >= table_count) return fail(-1, std::string(who) + ": src outside [0, table_count)");
    }
    // the rotations gather from the tables while other workgroups store: no output word may be a table word
    if (ranges_overlap(out, out_words, tables, table_count * 2 * kN)) return fail(-1, std::string(who) + ": the output must not overlap tables");
    if (!g_dev[device].keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    *shift = s;
    return 0;
}

// descriptors (pad = s << 8: the output shift without a test-vector row) and the parallel table-pointer array of `count` rotations
int upload_lut_rotations(DeviceState& s, Scratch& sc, size_t count, const uint32_t* tlwe0, const uint32_t* tables, const int32_t* src, int shift,
                         uint32_t* out, size_t out_stride, LinDesc** drot, const uint32_t*** dtab)
{
    std::vector<LinDesc> rot(count);
    std::vector<const uint32_t*> tab(count);
    for (size_t g = 0; g < count; g++) {
        const uint32_t* x = tlwe0 + g * kLvl0Words;
        rot[g] = {x, x, out ? out + g * out_stride : nullptr, 1, 0, 0u, (uint32_t)shift << 8};
        tab[g] = tables + (size_t)(src ? src[g] : (int32_t)g) * 2 * kN;
    }
    if (int rc = upload_descs(s, sc, rot, drot)) return rc;
    return upload_descs(s, sc, tab, dtab);
}


// ---- the recorded forms ----
// The ids of the recorded forms, their ranges against every other range, and the lookups' definitions (g_ops.lookup): op_registry.h
using opreg::kLookupOps;
bool is_spread_op(int op) { return op >= CUFHE_AMD_TL_SPREAD_BASE && op < opreg::kSpreadOpEnd; }
bool is_lut_rotate_op(int op) { return op >= CUFHE_AMD_TL_LUT_ROTATE_BASE && op < opreg::kLutRotateOpEnd; }
bool is_lut_op(int op) { return kLookupOps.contains(op) || is_spread_op(op) || is_lut_rotate_op(op); }

int log2_exact(long long v)      // -1 unless v is a power of two >= 1
{
    int a = 0;
    while (a < 31 && (1LL << a) < v) a++;
    return v >= 1 && (1LL << a) == v ? a : -1;
}

// The recorded lookups, table rotations and Spreads of ONE dependence level (any mix, any order), as one launch sequence:
//   lookups      siblings of one evaluation are fused by (definition, in0, in1, table) whatever their order in the list (as lower_gates
//                fuses the outputs of a multi-output gate); one rotation per evaluation with the address sum in its descriptor, its nout
//                lvl1 results contiguous in scratch; one key-switch descriptor per REQUESTED output, scratch -> out
//   LUT_ROTATE   the same rotation with the accumulator kept.  launch_blind_rotate dumps accumulators to ONE contiguous array for the
//                whole launch (acc_dump) and extracts nothing when it does, so the two kinds cannot share a launch: they run back to
//                back, the accumulators into scratch, and a Copy launch moves them to the scattered `out` buffers
//   Spread       one launch of trlwe_spread_desc_kernel, an item's own (stride, reps) in its descriptor
// Every rotation reads its operands and writes scratch only; outputs are written by the key switch, the Copy and the Spread, which follow
// all rotations -- so an in-place lookup (out == in0) is safe.  No allocation: scratch and descriptors come from the stream's workspace.
// The workspace is reused from offset 0 by every launch sequence, so the sequence completes before the level's other gates are lowered
// (HipBackend::run_gates); that is as good as interleaving them, because the scheduler never puts a writer of a buffer into the level of
// another operation that reads or writes it.
int lower_lut_ops(DeviceState& s, hipStream_t st, const GateRef* g, size_t n)
{
    if (n == 0) return 0;
    if (g_param_set >= 0) return fail_lut_set();
    struct Eval { const LookupDef* d; const uint32_t *in0, *in1, *table; size_t first; };
    std::map<std::tuple<int, const uint32_t*, const uint32_t*, const uint32_t*>, size_t> evals;
    std::vector<Eval> ev;
    std::vector<size_t> fuse(n, (size_t)-1);
    size_t nmid = 0, nks = 0, nacc = 0, nspread = 0;
    for (size_t i = 0; i < n; i++) {
        const GateRef& gr = g[i];
        if (!gr.out || !gr.in0) return fail(-1, "null ciphertext pointer");
        if (kLookupOps.contains(gr.op)) {
            const LookupDef* d = g_ops.lookup.find(gr.op);
            if (!d) return fail(-1, "lookup op " + std::to_string(gr.op) + " is not defined (cufhe_amd_define_lookup)");
            if (!gr.in2) return fail(-1, "lookup without a table");
            if (d->c[1] != 0 && !gr.in1) return fail(-1, "lookup needs a second address operand");
            const uint32_t* in1 = d->c[1] != 0 ? gr.in1 : nullptr;
            const auto key = std::make_tuple(kLookupOps.def(gr.op), gr.in0, in1, gr.in2);
            auto it = evals.find(key);
            if (it == evals.end()) {
                it = evals.emplace(key, ev.size()).first;
                ev.push_back({d, gr.in0, in1, gr.in2, nmid});
                nmid += (size_t)d->nout;
            }
            fuse[i] = it->second;
            nks++;
        } else if (is_lut_rotate_op(gr.op)) {
            if (!gr.in1) return fail(-1, "table rotation without an address");
            nacc++;
        } else if (is_spread_op(gr.op)) {
            const int a = (gr.op - CUFHE_AMD_TL_SPREAD_BASE) >> 4, b = (gr.op - CUFHE_AMD_TL_SPREAD_BASE) & 15;
            if (a + b > 10) return fail(-1, "recorded Spread: stride * reps > N");
            nspread++;
        } else return fail(-1, "internal: not a recorded lookup, Spread or table rotation");
    }
    if ((nks || nacc) && !s.keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    Scratch sc;
    const size_t need = (nmid * kLvl1Words + nacc * 2 * kN) * sizeof(uint32_t) + (ev.size() + 2 * nacc + nks) * (sizeof(LinDesc) + sizeof(uint32_t*)) +
                        nspread * sizeof(SpreadDesc) + 8192;
    if (int rc = open_scratch(s, st, need, &sc)) return rc;
    uint32_t *t1 = nullptr, *accs = nullptr;
    if (nmid)
        if (int rc = sc.alloc((void**)&t1, nmid * kLvl1Words * sizeof(uint32_t))) return rc;
    if (nacc)
        if (int rc = sc.alloc((void**)&accs, nacc * 2 * kN * sizeof(uint32_t))) return rc;
    std::vector<LinDesc> rot, ks, rot2, home;
    std::vector<const uint32_t*> tab, tab2;
    std::vector<SpreadDesc> spread;
    rot.reserve(ev.size()); tab.reserve(ev.size()); ks.reserve(nks);
    for (const Eval& e : ev) {
        rot.push_back({e.in0, e.in1 ? e.in1 : e.in0, t1 + e.first * kLvl1Words, e.d->c[0], e.in1 ? e.d->c[1] : 0, e.d->off, (uint32_t)e.d->s << 8});
        tab.push_back(e.table);
    }
    for (size_t i = 0; i < n; i++) {
        const GateRef& gr = g[i];
        if (kLookupOps.contains(gr.op)) {
            uint32_t* tj = t1 + (ev[fuse[i]].first + (size_t)kLookupOps.output(gr.op)) * kLvl1Words;
            ks.push_back({tj, tj, gr.out, 1, 0, 0u, 0u});
        } else if (is_lut_rotate_op(gr.op)) {       // operands (table, addr, -)
            uint32_t* acc = accs + rot2.size() * 2 * kN;
            rot2.push_back({gr.in1, gr.in1, nullptr, 1, 0, 0u, (uint32_t)(gr.op - CUFHE_AMD_TL_LUT_ROTATE_BASE) << 8});
            tab2.push_back(gr.in0);
            home.push_back({acc, acc, gr.out, 1, 0, 0u, 0u});
        } else {
            const int a = (gr.op - CUFHE_AMD_TL_SPREAD_BASE) >> 4, b = (gr.op - CUFHE_AMD_TL_SPREAD_BASE) & 15;
            spread.push_back({gr.in0, gr.out, 1 << a, 1 << b});
        }
    }
    LinDesc *drot, *dks, *drot2, *dhome;
    const uint32_t **dtab, **dtab2;
    SpreadDesc* dspread;
    if (int rc = upload_descs(s, sc, rot, &drot)) return rc;
    if (int rc = upload_descs(s, sc, tab, &dtab)) return rc;
    if (int rc = upload_descs(s, sc, rot2, &drot2)) return rc;
    if (int rc = upload_descs(s, sc, tab2, &dtab2)) return rc;
    if (int rc = upload_descs(s, sc, ks, &dks)) return rc;
    if (int rc = upload_descs(s, sc, home, &dhome)) return rc;
    if (int rc = upload_descs(s, sc, spread, &dspread)) return rc;
    if (int rc = launch_blind_rotate(s, st, drot, rot.size(), kLvl0N, nullptr, dtab)) return rc;
    if (int rc = launch_blind_rotate(s, st, drot2, rot2.size(), kLvl0N, accs, dtab2)) return rc;
    if (int rc = launch_keyswitch(s, st, dks, ks.size())) return rc;
    if (int rc = launch_lincomb(st, dhome, home.size(), 2 * kN)) return rc;
    if (!spread.empty()) {
        const int polys = (int)(2 * spread.size());
        const unsigned blocks = (unsigned)((polys + kSpreadWavesPerBlock - 1) / kSpreadWavesPerBlock);
        hipLaunchKernelGGL(trlwe_spread_desc_kernel, dim3(blocks), dim3(64 * kSpreadWavesPerBlock), 0, st, dspread, polys);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int cufhe_amd_define_lookup(const int32_t coeffs[2], uint32_t offset, int nout, int* op)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!coeffs || !op) return fail(-1, "define_lookup: null pointer");
    if (coeffs[0] == 0) return fail(-1, "define_lookup: c0 must not be 0");
    const int s = log2_exact(nout);
    if (s < 0 || s > kMaxOutputShift) return fail(-1, "define_lookup: nout must be 1, 2, 4 or 8");
    if (g_param_set >= 0) return fail_lut_set();
    // a lookup's table comes with each call: there is no row to write
    return define_op(g_ops.lookup, LookupDef{{coeffs[0], coeffs[1]}, offset, nout, s}, [](int i) { return g_dev[i].keys_ready; },
                     "Initialize(ek) has not been called for every device", "lookup table full (CUFHE_AMD_MAX_LOOKUPS definitions until CleanUp)",
                     false, [](int, int) { return 0; }, op);
}

int cufhe_amd_enqueue_lookup(int device, void* stream, int op, int copying, int nout, cufhe_amd_ctxt* const* outs, cufhe_amd_ctxt* table,
                             cufhe_amd_ctxt* in0, cufhe_amd_ctxt* in1)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    if (g_param_set >= 0) return fail_lut_set();
    if (g_lvl0_ring == 2048) return fail(-1, "enqueue_lookup: lookups run on the default path only: not on the N = 2048 ring (\"lvl0_ring\")");
    if (int rc = check_device(device)) return rc;
    const LookupDef* d = g_ops.lookup.find(op);
    if (!d || kLookupOps.output(op) != 0) return fail(-1, "enqueue_lookup: op must be a defined lookup (cufhe_amd_define_lookup; its output-0 id)");
    if (nout != d->nout) return fail(-1, "enqueue_lookup: nout must be the definition's output count");
    if (!outs || !table || !in0) return fail(-1, "enqueue_lookup: null ciphertext");
    if (d->c[1] != 0 && !in1) return fail(-1, "enqueue_lookup: the definition needs a second address operand");
    cufhe_amd_ctxt* ins[3] = {in0, d->c[1] != 0 ? in1 : nullptr, table};
    // the REQUESTED outputs: outs[j] == nullptr asks for no output j (no key switch, no buffer); the group is what remains, in j order
    int ops[1 << kMaxOutputShift];
    cufhe_amd_ctxt* req[1 << kMaxOutputShift];
    size_t nreq = 0;
    for (int j = 0; j < nout; j++) {
        if (!outs[j]) continue;
        for (size_t i = 0; i < nreq; i++)
            if (req[i] == outs[j]) return fail(-1, "enqueue_lookup: two outputs are the same ciphertext");
        // record_gate_group's precondition (sched_core.h: record_gate): no output of a group of several is one of its operands
        if (nout > 1)
            for (cufhe_amd_ctxt* c : ins)
                if (outs[j] == c) return fail(-1, "enqueue_lookup: an output of a multi-output lookup is also an operand");
        ops[nreq] = CUFHE_AMD_LOOKUP_OP_OUTPUT(op, j);
        req[nreq++] = outs[j];
    }
    if (nreq == 0) return fail(-1, "enqueue_lookup: null ciphertext (no output is requested)");
    sched::Scheduler* S = scheduler();
    for (size_t j = 0; j < nreq; j++) {
        if (int rc = sched_check_ctxt(S, req[j])) return rc;
        if (req[j]->level != 0) return fail(-1, "enqueue_lookup: outputs are lvl0 ciphertexts (level 0)");
    }
    for (int i = 0; i < 3; i++) {
        if (!ins[i]) continue;
        if (int rc = sched_check_ctxt(S, ins[i])) return rc;
        if (ins[i]->level != (i == 2 ? 2 : 0)) return fail(-1, "enqueue_lookup: address operands have level 0, the table level 2");
    }
    if (!g_dev[device].keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    if (int rc = S->dev(device).record_gate_group(stream, ops, copying != 0, req, nreq, ins)) return sched_error(S->dev(device), rc);
    return 0;
}

int cufhe_amd_enqueue_spread(int device, void* stream, int copying, cufhe_amd_ctxt* out, cufhe_amd_ctxt* in, int stride, int reps)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    if (g_param_set >= 0) return fail_lut_set();
    if (int rc = check_device(device)) return rc;
    if (!out || !in) return fail(-1, "enqueue_spread: null ciphertext");
    if (out == in) return fail(-1, "enqueue_spread: out must not be in");
    const int a = log2_exact(stride), b = log2_exact(reps);
    if (a < 0 || b < 0 || a + b > 10)
        return fail(-1, "enqueue_spread: stride and reps must be powers of two with stride * reps <= N (other pairs: cufhe_amd_trlwe_spread_batch)");
    sched::Scheduler* S = scheduler();
    if (int rc = sched_check_ctxt(S, out)) return rc;
    if (int rc = sched_check_ctxt(S, in)) return rc;
    if (out->level != 2 || in->level != 2) return fail(-1, "enqueue_spread: out and in are TRLWEs (level 2)");
    cufhe_amd_ctxt* ins[3] = {in, nullptr, nullptr};
    if (int rc = S->dev(device).record_gate(stream, CUFHE_AMD_TL_SPREAD(a, b), copying != 0, out, ins, 2)) return sched_error(S->dev(device), rc);
    return 0;
}

int cufhe_amd_enqueue_lut_rotate(int device, void* stream, int copying, int nout, cufhe_amd_ctxt* out, cufhe_amd_ctxt* table, cufhe_amd_ctxt* addr)
{
    std::lock_guard<std::mutex> lk(g_sched_mu);
    if (g_param_set >= 0) return fail_lut_set();
    if (int rc = check_device(device)) return rc;
    if (!out || !table || !addr) return fail(-1, "enqueue_lut_rotate: null ciphertext");
    if (out == table) return fail(-1, "enqueue_lut_rotate: out must not be table");
    const int s = log2_exact(nout);
    if (s < 0 || s > kMaxOutputShift) return fail(-1, "enqueue_lut_rotate: nout must be 1, 2, 4 or 8");
    sched::Scheduler* S = scheduler();
    for (cufhe_amd_ctxt* c : {out, table, addr})
        if (int rc = sched_check_ctxt(S, c)) return rc;
    if (out->level != 2 || table->level != 2 || addr->level != 0) return fail(-1, "enqueue_lut_rotate: out and table are TRLWEs (level 2), addr a lvl0 ciphertext");
    if (!g_dev[device].keys_ready) return fail(-3, "Initialize(ek) has not been called for this device");
    cufhe_amd_ctxt* ins[3] = {table, addr, nullptr};
    if (int rc = S->dev(device).record_gate(stream, CUFHE_AMD_TL_LUT_ROTATE(s), copying != 0, out, ins, 2)) return sched_error(S->dev(device), rc);
    return 0;
}

int cufhe_amd_lut_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, const uint32_t* tables, size_t table_count,
                               const int32_t* src, int nout, int steps, uint32_t* acc)
{
    int shift = 0;
    if (int rc = check_lut_args("lut_rotate_batch", device, count, tlwe0, tables, table_count, src, nout, acc, count * 2 * kN, &shift)) return rc;
    if (count == 0) return 0;
    if (steps < 0 || steps > kLvl0N) steps = kLvl0N;
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    hipStream_t st = (hipStream_t)stream;
    Scratch sc;
    if (int rc = open_scratch(s, st, count * (sizeof(LinDesc) + sizeof(uint32_t*)) + 4096, &sc)) return rc;
    LinDesc* drot;
    const uint32_t** dtab;
    if (int rc = upload_lut_rotations(s, sc, count, tlwe0, tables, src, shift, nullptr, 0, &drot, &dtab)) return rc;
    return launch_blind_rotate(s, st, drot, count, steps, acc, dtab);
}

int cufhe_amd_lut_lookup_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, const uint32_t* tables, size_t table_count,
                               const int32_t* src, int nout, uint32_t* tlwe0_out)
{
    int shift = 0;
    if (int rc = check_lut_args("lut_lookup_batch", device, count, tlwe0, tables, table_count, src, nout, tlwe0_out,
                                count * (size_t)(nout > 0 ? nout : 0) * kLvl0Words, &shift))
        return rc;
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    DeviceState& s = g_dev[device];
    hipStream_t st = (hipStream_t)stream;
    // one rotation per item, its nout extracted lvl1 ciphertexts contiguous in scratch, one key switch per output: the sequence of a
    // multi-output gate at level 0 (lower_gates)
    const size_t outs = count * (size_t)nout;
    Scratch sc;
    if (int rc = open_scratch(s, st, outs * (kLvl1Words * sizeof(uint32_t) + sizeof(LinDesc)) + count * (sizeof(LinDesc) + sizeof(uint32_t*)) + 8192, &sc))
        return rc;
    uint32_t* t1;
    if (int rc = sc.alloc((void**)&t1, outs * kLvl1Words * sizeof(uint32_t))) return rc;
    LinDesc *drot, *dks;
    const uint32_t** dtab;
    if (int rc = upload_lut_rotations(s, sc, count, tlwe0, tables, src, shift, t1, (size_t)nout * kLvl1Words, &drot, &dtab)) return rc;
    std::vector<LinDesc> ks(outs);
    for (size_t o = 0; o < outs; o++) ks[o] = {t1 + o * kLvl1Words, t1 + o * kLvl1Words, tlwe0_out + o * kLvl0Words, 1, 0, 0u, 0u};
    if (int rc = upload_descs(s, sc, ks, &dks)) return rc;
    if (int rc = launch_blind_rotate(s, st, drot, count, kLvl0N, nullptr, dtab)) return rc;
    return launch_keyswitch(s, st, dks, outs);
}

int cufhe_amd_trlwe_spread_batch(int device, void* stream, size_t count, const uint32_t* in, int stride, int reps, uint32_t* out)
{
    if (g_param_set >= 0) return fail_lut_set();
    if (int rc = check_device(device)) return rc;
    if (!in || !out) return fail(-1, "trlwe_spread_batch: null pointer");
    if (stride < 1 || reps < 1 || (long long)stride * reps > kN) return fail(-1, "trlwe_spread_batch: stride >= 1, reps >= 1 and stride * reps <= N are required");
    if (count > (size_t)INT32_MAX / 4) return fail(-1, "trlwe_spread_batch: count exceeds the kernel's index type");
    // every wave gathers its whole polynomial while others store: any overlap of the two arrays is refused
    if (ranges_overlap(in, count * 2 * kN, out, count * 2 * kN)) return fail(-1, "trlwe_spread_batch: out must not overlap in");
    if (count == 0) return 0;
    if (int rc = use_device(device)) return rc;
    const int polys = (int)(2 * count);
    const unsigned blocks = (unsigned)((polys + kSpreadWavesPerBlock - 1) / kSpreadWavesPerBlock);
    hipLaunchKernelGGL(trlwe_spread_kernel, dim3(blocks), dim3(64 * kSpreadWavesPerBlock), 0, (hipStream_t)stream, out, in, polys, stride, reps);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// linear layers: the one leveled operation on TLWEs, in front of the gates and lookups above
#include "linear.inc.h"
