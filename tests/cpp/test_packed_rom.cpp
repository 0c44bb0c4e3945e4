// test_packed_rom.cpp -- a packed ROM read through include/cufhe_amd.hpp: 2 TRLWEs of 4 words of 8 bits (bit b of word w at
// coefficient 8 w + b, messages +-mu) under the oracle's lvl1 key; address bits as TRGSW selectors (steps of the oracle's
// bootstrapping key: step i encrypts s0[i]) uploaded with TRGSW2NTT.  Recorded per address on its own stream: gCMUXRotateNTT with
// exponents 2N - 8 and 2N - 16 on both TRLWEs in place, one gCMUXNTT on the high bit, 8 x gSampleExtractAndKeySwitch(.., index b),
// one Synchronize().  Every output word is compared with the composition of the CPU oracle this program links, and decrypted.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

constexpr int N = ORC_N, W0 = ORC_n + 1, kTrgswWords = 2 * 3 * 2 * ORC_N;
static std::vector<uint32_t> g_s0(ORC_n), g_s1(ORC_K * ORC_N);

// X^e c on both polynomials (negacyclic), 0 <= e < 2N
static std::vector<uint32_t> rotate(const std::vector<uint32_t>& c, int e)
{
    std::vector<uint32_t> r(2 * N);
    for (int p = 0; p < 2; p++)
        for (int i = 0; i < N; i++) {
            const int k = ((i - e) % (2 * N) + 2 * N) % (2 * N);
            const uint32_t v = c[p * N + k % N];
            r[p * N + i] = k >= N ? 0u - v : v;
        }
    return r;
}

static std::vector<uint32_t> encrypt_trlwe(const std::vector<uint32_t>& msgs, std::mt19937& eng)
{
    std::vector<uint32_t> c(2 * N), prod(N);
    std::vector<int32_t> s(N);
    std::normal_distribution<double> noise(0.0, 64.0);
    for (int i = 0; i < N; i++) { c[i] = eng(); s[i] = (int32_t)g_s1[i]; }
    orc_polymul_schoolbook(prod.data(), s.data(), c.data());
    for (int i = 0; i < N; i++) c[N + i] = prod[i] + msgs[i] + (uint32_t)(int32_t)noise(eng);
    return c;
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(9091);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    orc_evalkey* ek = orc_evalkey_create(bk.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());

    // the table and its two TRLWEs
    uint32_t table[2][4];
    std::vector<std::vector<uint32_t>> rom(2);
    for (int t = 0; t < 2; t++) {
        std::vector<uint32_t> msgs(N, 0u);
        for (int w = 0; w < 4; w++) {
            table[t][w] = eng() & 0xFF;
            for (int b = 0; b < 8; b++) msgs[8 * w + b] = ((table[t][w] >> b) & 1) ? ORC_MU : 0u - ORC_MU;
        }
        rom[t] = encrypt_trlwe(msgs, eng);
    }
    // selector of address bit k with value v: the (k+1)-th step of the bootstrapping key whose key bit is v
    auto selector = [&](int k, int v) {
        int seen = 0;
        for (int i = 0; i < ORC_n; i++)
            if ((int)g_s0[i] == v && seen++ == k) return bk.data() + (size_t)i * kTrgswWords;
        std::fprintf(stderr, "no key bit %d\n", v);
        std::exit(2);
    };
    const int exps[2] = {2 * N - 8, 2 * N - 16};

    std::vector<Stream> st(8);
    std::vector<std::unique_ptr<cuFHETRGSWNTTlvl1>> sels;
    std::vector<std::unique_ptr<cuFHETRLWElvl1>> trl;
    std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> outs;
    for (int addr = 0; addr < 8; addr++) {
        st[addr].Create();
        cuFHETRGSWNTTlvl1* s[3];
        for (int k = 0; k < 3; k++) {
            sels.emplace_back(new cuFHETRGSWNTTlvl1);
            s[k] = sels.back().get();
            TRGSW2NTT(*s[k], *reinterpret_cast<const TFHEpp::TRGSW<TFHEpp::lvl1param>*>(selector(k, (addr >> k) & 1)), st[addr]);
        }
        cuFHETRLWElvl1* c[2];
        for (int t = 0; t < 2; t++) {
            trl.emplace_back(new cuFHETRLWElvl1);
            c[t] = trl.back().get();
            std::memcpy(c[t]->trlwehost[0].data(), rom[t].data(), 2 * N * sizeof(uint32_t));
            CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st[addr].device_id(), st[addr].raw(), c[t]->handle, 1));
            for (int k = 0; k < 2; k++) gCMUXRotateNTT(*c[t], *s[k], *c[t], exps[k], st[addr]);
        }
        trl.emplace_back(new cuFHETRLWElvl1);
        cuFHETRLWElvl1* root = trl.back().get();
        gCMUXNTT(*root, *s[2], *c[1], *c[0], st[addr]);
        for (int b = 0; b < 8; b++) {
            outs.emplace_back(new Ctxt<TFHEpp::lvl0param>);
            gSampleExtractAndKeySwitch(*outs.back(), *root, b, st[addr]);
            CtxtCopyD2H(*outs.back(), st[addr]);
        }
    }
    Synchronize();

    int bad_words = 0, bad_reads = 0;
    for (int addr = 0; addr < 8; addr++) {
        // the oracle composition
        std::vector<uint32_t> c[2] = {rom[0], rom[1]}, res(2 * N), t1(N + 1), t0(W0);
        for (int t = 0; t < 2; t++)
            for (int k = 0; k < 2; k++) {
                const std::vector<uint32_t> r = rotate(c[t], exps[k]);
                orc_cmux(res.data(), selector(k, (addr >> k) & 1), r.data(), c[t].data());
                c[t] = res;
            }
        orc_cmux(res.data(), selector(2, (addr >> 2) & 1), c[1].data(), c[0].data());
        uint32_t word = 0;
        for (int b = 0; b < 8; b++) {
            const std::vector<uint32_t> r = b ? rotate(res, 2 * N - b) : res;      // SE_b(c) = SE_0(X^-b c)
            orc_sample_extract0(t1.data(), r.data());
            orc_keyswitch(ek, t0.data(), t1.data());
            auto& got = *outs[addr * 8 + b];
            bad_words += std::memcmp(got.tlwehost.data(), t0.data(), W0 * sizeof(uint32_t)) != 0;
            word |= (uint32_t)orc_tlwe_decrypt(0, g_s0.data(), got.tlwehost.data()) << b;
        }
        bad_reads += word != table[addr >> 2][addr & 3];
    }
    std::printf("%-48s %s (%d/64 failures)\n", "packed ROM: outputs == the oracle composition", bad_words ? "FAIL" : "PASS", bad_words);
    std::printf("%-48s %s (%d/8 failures)\n", "packed ROM: decrypted words", bad_reads ? "FAIL" : "PASS", bad_reads);
    outs.clear(); trl.clear(); sels.clear();
    for (auto& s : st) s.Destroy();
    CleanUp();
    orc_evalkey_destroy(ek);
    const int failures = bad_words + bad_reads;
    std::printf(failures ? "FAILURES: %d\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
