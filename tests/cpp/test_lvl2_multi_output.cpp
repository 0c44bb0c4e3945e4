// test_lvl2_multi_output.cpp -- a multi-output gate of the N = 2048 ring through include/cufhe_amd.hpp: DefineGateLvl2(.., 2),
// TestVectorMultiLvl2 and both outputs by the per-gate API (gApply of Output(g, j)) on Streams with "lvl0_ring" 2048.
// 64 full adders: sum and carry of x = a + b + c from ONE rotation each, bits as padded p = 4 messages b / 8; the oracle's +-1/8 bit
// encryptions are first mapped to b / 8 by a one-input gate of the ring.  Keys, encryption and decryption come from the CPU oracle.
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"
#include "../../oracle/tfhe_oracle_lvl2.h"

using namespace cufhe;
using P = TFHEpp::lvl0param;

static const uint64_t kEighth64 = 1ull << 61;       // 1/8 on the 64-bit torus: p = 4 with a padding bit, message m is m / 8

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(1818);
    orc_rng rng;
    orc_rng_seed(&rng, 779);
    std::vector<uint32_t> s0(ORC_n), s1(ORC_K * ORC_N), s2(ORC2_N);
    orc_keygen(1, s0.data(), s1.data());
    orc2_keygen(7, s2.data());
    std::vector<uint64_t> bk2(ORC2_BK_WORDS);
    std::vector<uint32_t> ksk2(ORC2_KSK_WORDS);
    orc2_bkgen(3007, s0.data(), s2.data(), bk2.data());
    orc2_kskgen(4007, s0.data(), s2.data(), ksk2.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, s0.data(), s1.data(), bk.data());
    orc_kskgen(2001, s0.data(), s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());
    lvl2::Initialize(bk2.data(), bk2.size(), ksk2.data(), ksk2.size());
    CUFHE_AMD_CHECK(cufhe_amd_set_option("lvl0_ring", 2048));

    // +-1/8 + 1/8 = message 0 or 2 -> b / 8
    const UserGate to_eighths = DefineGateLvl2({1, 0, 0}, 1u << 29, TestVectorLvl2({0, 0, kEighth64, kEighth64}).data());
    const std::vector<uint64_t> sum = {0, kEighth64, 0, kEighth64}, carry = {0, 0, kEighth64, kEighth64};
    const UserGate fa = DefineGateLvl2({1, 1, 1}, 0, TestVectorMultiLvl2({sum, carry}, 4).data(), 2);
    int failures = fa.nout != 2 || fa.output(1) != CUFHE_AMD_LVL2_USER_OP_OUTPUT(fa.op, 1);

    const int K = 64;
    std::vector<Ctxt<P>> raw(3 * K), in(3 * K), s(K), c(K);
    std::vector<int> bits(3 * K);
    Stream st[4];
    for (auto& t : st) t.Create();
    for (int i = 0; i < K; i++) {
        Stream t = st[i % 4];
        for (int k = 0; k < 3; k++) {
            bits[3 * i + k] = eng() & 1;
            orc_tlwe_encrypt(&rng, 0, s0.data(), bits[3 * i + k], raw[3 * i + k].tlwehost.data());
            CtxtCopyH2D(raw[3 * i + k], t);
            gApply(to_eighths, in[3 * i + k], raw[3 * i + k], t);
        }
        gApply(Output(fa, 1), c[i], in[3 * i], in[3 * i + 1], in[3 * i + 2], t);
        gApply(Output(fa, 0), s[i], in[3 * i], in[3 * i + 1], in[3 * i + 2], t);
        CtxtCopyD2H(s[i], t);
        CtxtCopyD2H(c[i], t);
    }
    Synchronize();
    int bad = 0;
    for (int i = 0; i < K; i++) {
        const int x = bits[3 * i] + bits[3 * i + 1] + bits[3 * i + 2];
        auto decode = [&](Ctxt<P>& ct) { return (int)(((orc_tlwe_phase(0, s0.data(), ct.tlwehost.data()) + (1u << 28)) >> 29) & 7); };
        bad += decode(s[i]) != (x & 1) || decode(c[i]) != (x >> 1);
    }
    std::printf("%-48s %s (%d/%d failures)\n", "full adders, one 2-output lvl2 gate each", bad ? "FAIL" : "PASS", bad, K);
    failures += bad;
    for (auto& t : st) t.Destroy();
    CUFHE_AMD_CHECK(cufhe_amd_set_option("lvl0_ring", 1024));
    CleanUp();
    std::printf(failures ? "FAILURES: %d\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
