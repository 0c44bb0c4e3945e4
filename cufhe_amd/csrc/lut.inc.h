// lut.inc.h -- host side of the encrypted-table lookup (included by capi.hip): blind rotations whose initial
// accumulator is a caller's TRLWE (the table instantiations of the three default-path kernels, launch_blind_rotate with a table array),
// the lookup's key switch on the path the multi-output gates take at level 0, and the keyless Spread (kernels_lut.hip.h).  Default
// parameter set only.  There is no recorded form: callers order a call behind gates recorded on a stream with cufhe_amd_stream_fence.

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

}  // namespace

extern "C" {

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
