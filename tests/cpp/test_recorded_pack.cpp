// test_recorded_pack.cpp -- the RAM-write path of tests/cpp/test_pack.cpp with the RECORDED pack of include/cufhe_amd.hpp: eight Xor
// gates on encrypted bits, gPack of the results at coefficients 0 .. 7 of one TRLWE -- a scheduler node, no fence and no wait before the
// final Synchronize --, the copying Pack of the same ciphertexts into a second TRLWE, gCMUXNTT against a host-encrypted TRLWE under a host-encrypted selector (a step of the oracle's
// bootstrapping key), gSampleExtractAndKeySwitch at 0 .. 7.  The packing key is genuine, built here from the oracle's secret keys:
// K[i][j][v-1] = TRLWE_s1(v s0_i 2^(32 - 2 (j+1))), masks uniform, noise sigma = 2^-25.  Checked: the packed words against the
// formula of INTEGRATION.md section 12 computed on the host, and the decrypted word for both selector values.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

constexpr int N = ORC_N, n = ORC_n, W0 = ORC_n + 1, kTrgswWords = 2 * 3 * 2 * ORC_N, T = 8, kRow = 2 * ORC_N;
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

// sum_m X^pos[m] PackKS(in[m]) by the formula
static std::vector<uint32_t> pack_formula(const std::vector<uint32_t>& key, const std::vector<std::vector<uint32_t>>& in, const std::vector<int>& pos)
{
    std::vector<uint32_t> out(kRow, 0u);
    for (size_t m = 0; m < in.size(); m++) {
        std::vector<uint32_t> ks(kRow, 0u);
        for (int i = 0; i < n; i++) {
            const uint32_t abar = in[m][i] + (1u << 15);
            for (int j = 0; j < T; j++) {
                const uint32_t d = (abar >> (32 - 2 * (j + 1))) & 3u;
                if (!d) continue;
                const uint32_t* row = key.data() + (((size_t)i * T + j) * 3 + (d - 1)) * kRow;
                for (int w = 0; w < kRow; w++) ks[w] -= row[w];
            }
        }
        ks[N] += in[m][n];
        for (int p = 0; p < 2; p++)
            for (int k = 0; k < N; k++) {
                const int kk = k + pos[m];
                out[p * N + kk % N] += kk >= N ? 0u - ks[p * N + k] : ks[p * N + k];
            }
    }
    return out;
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(9092);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());

    cufhe_amd_pack_params pp;
    CUFHE_AMD_CHECK(cufhe_amd_pack_get_params(&pp));
    int failures = 0;
    const bool params_ok = pp.n == (uint32_t)n && pp.N == (uint32_t)N && pp.t == (uint32_t)T && pp.basebit == 2 && pp.key_words == (uint64_t)n * T * 3 * kRow;
    std::printf("%-48s %s\n", "packing: parameters", params_ok ? "PASS" : "FAIL");
    failures += !params_ok;

    // the genuine key
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
    orc_rng_seed(&rng, 77);
    int a[8], b[8];
    const uint32_t other = eng() & 0xFF;
    std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> ca, cb, cx;
    for (int k = 0; k < 8; k++) {
        a[k] = (int)(eng() & 1); b[k] = (int)(eng() & 1);
        ca.emplace_back(new Ctxt<TFHEpp::lvl0param>); cb.emplace_back(new Ctxt<TFHEpp::lvl0param>); cx.emplace_back(new Ctxt<TFHEpp::lvl0param>);
        orc_tlwe_encrypt(&rng, 0, g_s0.data(), a[k], ca[k]->tlwehost.data());
        orc_tlwe_encrypt(&rng, 0, g_s0.data(), b[k], cb[k]->tlwehost.data());
        Xor(*cx[k], *ca[k], *cb[k], st);                 // recorded; the pack below is recorded a level behind it
    }
    auto packed_p = std::make_unique<cuFHETRLWElvl1>(), packed2_p = std::make_unique<cuFHETRLWElvl1>(), rom_p = std::make_unique<cuFHETRLWElvl1>(), res_p = std::make_unique<cuFHETRLWElvl1>();
    cuFHETRLWElvl1 &packed = *packed_p, &packed2 = *packed2_p, &rom = *rom_p, &res = *res_p;
    std::vector<Ctxt<TFHEpp::lvl0param>*> ins;
    std::vector<int> pos;
    for (int k = 0; k < 8; k++) { ins.push_back(cx[k].get()); pos.push_back(k); }
    uint64_t recorded_before = 0, recorded_after = 0;
    {
        cufhe_amd_sched_stats stats;
        CUFHE_AMD_CHECK(cufhe_amd_sched_get_stats(st.device_id(), &stats, 0));
        recorded_before = stats.gates;
        gPack(packed, ins, pos, st);
        Pack(packed2, ins, pos, st);                     // inputs from the Xor results on their way to tlwehost, the result to packed2.trlwehost
        CUFHE_AMD_CHECK(cufhe_amd_sched_get_stats(st.device_id(), &stats, 0));
        recorded_after = stats.gates;
    }
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), packed.handle, 0));

    std::vector<uint32_t> msgs(N, 0u);
    for (int k = 0; k < 8; k++) msgs[k] = ((other >> k) & 1) ? ORC_MU : 0u - ORC_MU;
    const std::vector<uint32_t> rom_words = encrypt_trlwe(msgs, 64.0, eng);
    std::memcpy(rom.trlwehost[0].data(), rom_words.data(), kRow * sizeof(uint32_t));
    CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st.device_id(), st.raw(), rom.handle, 1));
    auto selector = [&](int v) {
        for (int i = 0; i < ORC_n; i++)
            if ((int)g_s0[i] == v) return bk.data() + (size_t)i * kTrgswWords;
        std::fprintf(stderr, "no key bit %d\n", v);
        std::exit(2);
    };
    int bad_reads = 0;
    std::vector<std::vector<uint32_t>> gate_words;
    for (int bit = 1; bit >= 0; bit--) {
        cuFHETRGSWNTTlvl1 sel;
        TRGSW2NTT(sel, *reinterpret_cast<const TFHEpp::TRGSW<TFHEpp::lvl1param>*>(selector(bit)), st);
        gCMUXNTT(res, sel, packed, rom, st);
        std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> outs;
        for (int k = 0; k < 8; k++) {
            outs.emplace_back(new Ctxt<TFHEpp::lvl0param>);
            gSampleExtractAndKeySwitch(*outs.back(), res, k, st);
            CtxtCopyD2H(*outs.back(), st);
        }
        Synchronize();
        uint32_t word = 0, want = 0;
        for (int k = 0; k < 8; k++) {
            word |= (uint32_t)orc_tlwe_decrypt(0, g_s0.data(), outs[k]->tlwehost.data()) << k;
            want |= (uint32_t)(bit ? (a[k] ^ b[k]) : (int)((other >> k) & 1)) << k;
        }
        bad_reads += word != want;
        std::printf("selector %d: read 0x%02x, want 0x%02x\n", bit, word, want);
    }
    for (int k = 0; k < 8; k++) gate_words.emplace_back(cx[k]->tlwehost.begin(), cx[k]->tlwehost.end());
    const std::vector<uint32_t> want_packed = pack_formula(key, gate_words, pos);
    const int bad_words = std::memcmp(packed.trlwehost[0].data(), want_packed.data(), kRow * sizeof(uint32_t)) != 0;
    std::printf("%-48s %s\n", "recorded pack: words == the formula on the host", bad_words ? "FAIL" : "PASS");
    const int bad_copying = std::memcmp(packed2.trlwehost[0].data(), want_packed.data(), kRow * sizeof(uint32_t)) != 0;
    std::printf("%-48s %s\n", "copying Pack: the same words in trlwehost", bad_copying ? "FAIL" : "PASS");
    const int bad_count = recorded_after - recorded_before != 2;
    std::printf("%-48s %s\n", "a pack is one recorded gate", bad_count ? "FAIL" : "PASS");
    failures += bad_copying + bad_count;
    std::printf("%-48s %s (%d/2 failures)\n", "packing: RAM write, decrypted words", bad_reads ? "FAIL" : "PASS", bad_reads);
    failures += bad_words + bad_reads;
    ca.clear(); cb.clear(); cx.clear();
    packed_p.reset(); packed2_p.reset(); rom_p.reset(); res_p.reset();
    st.Destroy();
    CleanUp();
    std::printf(failures ? "FAILURES: %d\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
