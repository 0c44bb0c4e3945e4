// test_multi_output_gates.cpp -- multi-output user gates through include/cufhe_amd.hpp: DefineGate(.., nout), TestVectorMulti,
// ApplyMulti and gApplyMulti.  Keys, encryption and decryption come from the CPU oracle.
//   - 16-bit ripple-carry adders of ONE 2-output gate per bit (sum and carry of x = a + b + cin, bits as padded p = 4 messages b / 8),
//     g-forms on device buffers, one stream per adder; the oracle's +-1/8 bit encryptions are first mapped to b / 8 by a one-input gate
//   - the copying form on lvl1 ciphertexts: a 4-output gate of one input (x = a + 1/8, message m = 0 or 2: m, 3 - m, m >> 1, m & 1)
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

static std::vector<uint32_t> g_s0(ORC_n), g_s1(ORC_K * ORC_N);
static orc_rng g_rng;
static int g_failures = 0;
static const uint32_t kEighth = 1u << 29;       // p = 4 with a padding bit: message m is m / 8

template <class P> const uint32_t* key() { return detail::level_of<P>() ? g_s1.data() : g_s0.data(); }
template <class P> void encrypt(Ctxt<P>& c, int bit) { orc_tlwe_encrypt(&g_rng, detail::level_of<P>(), key<P>(), bit, c.tlwehost.data()); }
// the nearest eighth of the phase
template <class P> int decode(Ctxt<P>& c)
{
    const uint32_t ph = orc_tlwe_phase(detail::level_of<P>(), key<P>(), c.tlwehost.data());
    return (int)(((ph + (kEighth >> 1)) >> 29) & 7);
}

static void report(const char* what, int bad, int total)
{
    std::printf("%-48s %s (%d/%d failures)\n", what, bad ? "FAIL" : "PASS", bad, total);
    g_failures += bad;
}

static void Adders(std::mt19937& eng)
{
    using P = TFHEpp::lvl0param;
    const int A = 32, B = 16;
    // +-1/8 + 1/8 = message 0 or 2 -> b / 8
    const UserGate to_eighths = DefineGate({1, 0, 0}, kEighth, TestVector({0, 0, kEighth, kEighth}).data());
    const std::vector<uint32_t> sum = {0, kEighth, 0, kEighth}, carry = {0, 0, kEighth, kEighth};
    const UserGate fa = DefineGate({1, 1, 1}, 0, TestVectorMulti({sum, carry}, 4).data(), 2);
    std::vector<Ctxt<P>> xr(A * B), yr(A * B), x(A * B), y(A * B), s(A * B), c(A * (B + 1)), c0(A);
    std::vector<uint32_t> va(A), vb(A);
    std::vector<Stream> st(A);
    for (int i = 0; i < A; i++) {
        st[i].Create();
        va[i] = eng() & 0xFFFF;
        vb[i] = eng() & 0xFFFF;
        for (int k = 0; k < B; k++) {
            encrypt(xr[i * B + k], (va[i] >> k) & 1);
            encrypt(yr[i * B + k], (vb[i] >> k) & 1);
            CtxtCopyH2D(xr[i * B + k], st[i]);
            CtxtCopyH2D(yr[i * B + k], st[i]);
            gApply(to_eighths, x[i * B + k], xr[i * B + k], st[i]);
            gApply(to_eighths, y[i * B + k], yr[i * B + k], st[i]);
        }
        encrypt(c0[i], 0);
        CtxtCopyH2D(c0[i], st[i]);
        gApply(to_eighths, c[i * (B + 1)], c0[i], st[i]);
    }
    for (int k = 0; k < B; k++)
        for (int i = 0; i < A; i++)
            gApplyMulti(fa, {&s[i * B + k], &c[i * (B + 1) + k + 1]}, x[i * B + k], y[i * B + k], c[i * (B + 1) + k], st[i]);
    for (int i = 0; i < A; i++) {
        for (int k = 0; k < B; k++) CtxtCopyD2H(s[i * B + k], st[i]);
        CtxtCopyD2H(c[i * (B + 1) + B], st[i]);
    }
    Synchronize();
    int bad = 0;
    for (int i = 0; i < A; i++) {
        uint32_t v = (uint32_t)decode(c[i * (B + 1) + B]) << B;
        for (int k = 0; k < B; k++) v |= (uint32_t)decode(s[i * B + k]) << k;
        bad += v != va[i] + vb[i];
    }
    report("16-bit adders, one 2-output gate per bit (lvl0)", bad, A);
    for (auto& t : st) t.Destroy();
}

static void CopyingForm(std::mt19937& eng)
{
    using P = TFHEpp::lvl1param;
    const int K = 64;
    // x = a + 1/8 for a +-1/8 bit: message m = 2a
    std::vector<std::vector<uint32_t>> f(4, std::vector<uint32_t>(4));
    for (int m = 0; m < 4; m++) {
        f[0][m] = (uint32_t)m * kEighth;
        f[1][m] = (uint32_t)(3 - m) * kEighth;
        f[2][m] = (uint32_t)(m >> 1) * kEighth;
        f[3][m] = (uint32_t)(m & 1) * kEighth;
    }
    const UserGate g = DefineGate({1, 0, 0}, kEighth, TestVectorMulti(f, 4).data(), 4);
    std::vector<Ctxt<P>> a(K), o0(K), o1(K), o2(K), o3(K);
    std::vector<int> pa(K);
    Stream st[4];
    for (auto& s : st) s.Create();
    for (int i = 0; i < K; i++) {
        pa[i] = eng() & 1;
        encrypt(a[i], pa[i]);
    }
    for (int i = 0; i < K; i++) ApplyMulti(g, {&o0[i], &o1[i], &o2[i], &o3[i]}, a[i], st[i % 4]);
    Synchronize();
    int bad = 0;
    for (int i = 0; i < K; i++) {
        const int m = 2 * pa[i];
        bad += decode(o0[i]) != m || decode(o1[i]) != 3 - m || decode(o2[i]) != (m >> 1) || decode(o3[i]) != (m & 1);
    }
    report("4-output gate, 1 input (ApplyMulti, lvl1)", bad, K);
    for (auto& s : st) s.Destroy();
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(4343);
    orc_rng_seed(&g_rng, 778);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());
    Adders(eng);
    CopyingForm(eng);
    CleanUp();
    std::printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
