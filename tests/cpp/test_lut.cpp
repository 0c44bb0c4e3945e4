// test_lut.cpp -- the worked example of INTEGRATION.md section 13 through include/cufhe_amd.hpp: four Xor gates on encrypted bits make
// the entries of a table, gPackTLWEs puts entry m at coefficient m N / 4 of one TRLWE, gSpreadTRLWE fills the boxes, gLookupTRLWE reads
// it by a host-encrypted padded address m / 8 -- one blind rotation per read.  The packing key is genuine, built here from the oracle's
// secret keys as in test_pack.cpp.  Checked: the spread words against the defining sum computed on the host, the decrypted entry for
// every address, and gBlindRotateTRLWE followed by an extraction at index 0 for one address.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

constexpr int N = ORC_N, n = ORC_n, T = 8, kRow = 2 * ORC_N, P = 4;
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
    std::mt19937 eng(9093);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());

    cufhe_amd_pack_params pp;
    CUFHE_AMD_CHECK(cufhe_amd_pack_get_params(&pp));
    std::vector<uint32_t> key((size_t)pp.key_words);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < T; j++)
            for (int v = 1; v <= 3; v++) {
                std::vector<uint32_t> msgs(N, 0u);
                msgs[0] = (uint32_t)v * g_s0[i] << (32 - 2 * (j + 1));
                const std::vector<uint32_t> row = encrypt_trlwe(msgs, 128.0, eng);      // sigma = 2^-25 of the torus
                std::memcpy(key.data() + (((size_t)i * T + j) * 3 + (v - 1)) * kRow, row.data(), kRow * sizeof(uint32_t));
            }
    InitializePacking(key.data(), key.size());

    Stream st;
    st.Create();
    orc_rng rng;
    orc_rng_seed(&rng, 78);
    int a[P], b[P], failures = 0;
    std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> ca, cb, cv;
    for (int m = 0; m < P; m++) {
        a[m] = (int)(eng() & 1); b[m] = (int)(eng() & 1);
        ca.emplace_back(new Ctxt<TFHEpp::lvl0param>); cb.emplace_back(new Ctxt<TFHEpp::lvl0param>); cv.emplace_back(new Ctxt<TFHEpp::lvl0param>);
        orc_tlwe_encrypt(&rng, 0, g_s0.data(), a[m], ca[m]->tlwehost.data());
        orc_tlwe_encrypt(&rng, 0, g_s0.data(), b[m], cb[m]->tlwehost.data());
        Xor(*cv[m], *ca[m], *cb[m], st);                 // table entries made by gates: recorded, launched by the fence inside gPackTLWEs
    }
    auto packed_p = std::make_unique<cuFHETRLWElvl1>(), table_p = std::make_unique<cuFHETRLWElvl1>(), rot_p = std::make_unique<cuFHETRLWElvl1>();
    cuFHETRLWElvl1 &packed = *packed_p, &table = *table_p, &rotated = *rot_p;
    std::vector<Ctxt<TFHEpp::lvl0param>*> ins;
    std::vector<int> pos;
    for (int m = 0; m < P; m++) { ins.push_back(cv[m].get()); pos.push_back(m * N / P); }
    gPackTLWEs(packed, ins, pos, st);                    // entry m at coefficient m N / p
    gSpreadTRLWE(table, packed, 1, N / P, st);           // boxes; the top half box = -v[0]
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), packed.handle, 0));
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), table.handle, 0));

    int bad_reads = 0;
    for (int m = 0; m < P; m++) {
        Ctxt<TFHEpp::lvl0param> addr, out;
        encrypt_torus0((uint32_t)m << 29, eng, addr.tlwehost.data());      // the padded message m / 8
        CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), addr.handle, 1));
        gLookupTRLWE({&out}, table, addr, st);
        CtxtCopyD2H(out, st);
        Synchronize();
        const int got = orc_tlwe_decrypt(0, g_s0.data(), out.tlwehost.data());
        bad_reads += got != (a[m] ^ b[m]);
        std::printf("address %d: read %d, want %d\n", m, got, a[m] ^ b[m]);
        if (m == 2) {      // the rotation alone, then the extraction at index 0: the same entry
            Ctxt<TFHEpp::lvl0param> out2;
            gBlindRotateTRLWE(rotated, table, addr, st);
            gSampleExtractAndKeySwitch(out2, rotated, 0, st);
            CtxtCopyD2H(out2, st);
            Synchronize();
            const int bad = std::memcmp(out2.tlwehost.data(), out.tlwehost.data(), (n + 1) * sizeof(uint32_t)) != 0;
            std::printf("%-48s %s\n", "lookup == rotation + extraction at index 0", bad ? "FAIL" : "PASS");
            failures += bad;
        }
    }
    const std::vector<uint32_t> want_table = spread_formula(packed.trlwehost[0].data(), 1, N / P);
    const int bad_words = std::memcmp(table.trlwehost[0].data(), want_table.data(), kRow * sizeof(uint32_t)) != 0;
    std::printf("%-48s %s\n", "spread: words == the defining sum on the host", bad_words ? "FAIL" : "PASS");
    std::printf("%-48s %s (%d/%d failures)\n", "lookup: decrypted entries", bad_reads ? "FAIL" : "PASS", bad_reads, P);
    failures += bad_words + bad_reads;
    ca.clear(); cb.clear(); cv.clear();
    packed_p.reset(); table_p.reset(); rot_p.reset();
    st.Destroy();
    CleanUp();
    std::printf(failures ? "FAILURES: %d\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
