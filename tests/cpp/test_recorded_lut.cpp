// test_recorded_lut.cpp -- the worked example of INTEGRATION.md section 13 in its RECORDED form, through include/cufhe_amd.hpp: a
// host-encrypted TRLWE holds four bit entries at coefficients m N / 4, gSpread fills the boxes, gLookup reads it by host-encrypted
// padded addresses m / 8 -- every call returns at once, nothing is fenced, and ONE Synchronize() follows the whole program.  A fifth
// lookup forms its address 1/8 + 2/8 from two ciphertexts inside the rotation (DefineLookup({1, 1}, 0, 1)), and gLutRotate followed by
// an extraction at index 0 gives the words of the lookup.  Checked: the spread words against the defining sum computed on the host,
// the decrypted entry of every read, one launch sequence per level and kind (cufhe_amd_sched_get_stats).
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

constexpr int N = ORC_N, n = ORC_n, kRow = 2 * ORC_N, P = 4;
static std::vector<uint32_t> g_s0(ORC_n), g_s1(ORC_K * ORC_N);

static std::vector<uint32_t> encrypt_trlwe(const std::vector<uint32_t>& msgs, double sigma, std::mt19937& eng)
{
    std::vector<uint32_t> c(2 * N), prod(N);
    std::vector<int32_t> s(N);
    std::normal_distribution<double> noise(0.0, sigma);
    for (int i = 0; i < N; i++) { c[i] = eng(); s[i] = (int32_t)g_s1[i]; }
    orc_polymul_ntt(prod.data(), s.data(), c.data());
    for (int i = 0; i < N; i++) c[N + i] = prod[i] + msgs[i] + (uint32_t)(int32_t)noise(eng);
    return c;
}

// a lvl0 encryption of the torus word msg, noise sigma = 2^-15 of the torus
static void encrypt_torus0(uint32_t msg, std::mt19937& eng, uint32_t* out)
{
    std::normal_distribution<double> noise(0.0, 131072.0);
    uint32_t b = msg + (uint32_t)(int32_t)noise(eng);
    for (int i = 0; i < n; i++) { out[i] = eng(); b += out[i] * g_s0[i]; }
    out[n] = b;
}

// Spread by its defining sum: X^(-stride floor(reps/2)) sum_i X^(i stride) c on both polynomials
static std::vector<uint32_t> spread_formula(const uint32_t* c, int stride, int reps)
{
    std::vector<uint32_t> out(kRow, 0u);
    for (int p = 0; p < 2; p++)
        for (int k = 0; k < N; k++)
            for (int i = 0; i < reps; i++) {
                const int idx = ((k + stride * (reps / 2) - i * stride) % (2 * N) + 2 * N) % (2 * N);
                out[p * N + k] += idx >= N ? 0u - c[p * N + idx - N] : c[p * N + idx];
            }
    return out;
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(9094);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());

    Stream st;
    st.Create();
    int v[P] = {1, 0, 1, 0}, failures = 0;
    for (int m = 1; m < 3; m++) v[m] = (int)(eng() & 1);
    std::vector<uint32_t> msgs(N, 0u);
    for (int m = 0; m < P; m++) msgs[m * N / P] = v[m] ? 1u << 29 : 0u - (1u << 29);       // +-1/8 at coefficient m N / p
    auto packed_p = std::make_unique<cuFHETRLWElvl1>(), table_p = std::make_unique<cuFHETRLWElvl1>(), rot_p = std::make_unique<cuFHETRLWElvl1>();
    cuFHETRLWElvl1 &packed = *packed_p, &table = *table_p, &rotated = *rot_p;
    const std::vector<uint32_t> enc = encrypt_trlwe(msgs, 128.0, eng);                       // sigma = 2^-25 of the torus
    std::memcpy(packed.trlwehost[0].data(), enc.data(), kRow * sizeof(uint32_t));
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), packed.handle, 1));

    const int one = DefineLookup({1, 0}, 0u, 1), two = DefineLookup({1, 1}, 0u, 1);
    std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> addr, out;
    for (int m = 0; m < P + 2; m++) { addr.emplace_back(new Ctxt<TFHEpp::lvl0param>); out.emplace_back(new Ctxt<TFHEpp::lvl0param>); }
    cufhe_amd_sched_stats stats;
    CUFHE_AMD_CHECK(cufhe_amd_sched_get_stats(st.device_id(), &stats, 1));
    gSpread(table, packed, 1, N / P, st);                    // boxes; the top half box = -v[0].  Recorded: returns at once
    for (int m = 0; m < P; m++) {
        encrypt_torus0((uint32_t)m << 29, eng, addr[m]->tlwehost.data());      // the padded message m / 8
        CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), addr[m]->handle, 1));
        gLookup({out[m].get()}, table, *addr[m], nullptr, one, st);
    }
    gLookup({out[P].get()}, table, *addr[1], addr[2].get(), two, st);          // address 1/8 + 2/8: entry 3
    gLutRotate(rotated, table, *addr[2], st);
    gSampleExtractAndKeySwitch(*out[P + 1], rotated, 0, st);
    for (auto& o : out) CtxtCopyD2H(*o, st);
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), table.handle, 0));
    Synchronize();
    CUFHE_AMD_CHECK(cufhe_amd_sched_get_stats(st.device_id(), &stats, 0));

    int bad_reads = 0;
    for (int m = 0; m <= P; m++) {
        const int want = m < P ? v[m] : v[3];
        const int got = orc_tlwe_decrypt(0, g_s0.data(), out[m]->tlwehost.data());
        bad_reads += got != want;
        std::printf("read %d: %d, want %d\n", m, got, want);
    }
    const int bad_rot = std::memcmp(out[P + 1]->tlwehost.data(), out[2]->tlwehost.data(), (n + 1) * sizeof(uint32_t)) != 0;
    std::printf("%-56s %s\n", "lookup == gLutRotate + extraction at index 0", bad_rot ? "FAIL" : "PASS");
    const std::vector<uint32_t> want_table = spread_formula(enc.data(), 1, N / P);
    const int bad_words = std::memcmp(table.trlwehost[0].data(), want_table.data(), kRow * sizeof(uint32_t)) != 0;
    std::printf("%-56s %s\n", "recorded spread: words == the defining sum on the host", bad_words ? "FAIL" : "PASS");
    std::printf("%-56s %s (%d/%d failures)\n", "recorded lookups: decrypted entries", bad_reads ? "FAIL" : "PASS", bad_reads, P + 1);
    // Spread; then the five lookups (lvl0 kind) and the table rotation (TRLWE kind); then the extraction: three dependence levels, one
    // launch sequence per level and kind
    const int bad_levels = !(stats.levels == 3 && stats.launch_sequences == 4);
    std::printf("%-56s %s (%llu levels, %llu sequences)\n", "three levels, four launch sequences", bad_levels ? "FAIL" : "PASS",
                (unsigned long long)stats.levels, (unsigned long long)stats.launch_sequences);
    failures += bad_words + bad_reads + bad_rot + bad_levels;
    addr.clear(); out.clear();
    packed_p.reset(); table_p.reset(); rot_p.reset();
    st.Destroy();
    CleanUp();
    std::printf(failures ? "FAILURES: %d\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
