// test_user_gates.cpp -- user gates (programmable bootstrapping) through include/cufhe_amd.hpp: DefineGate, TestVector, Apply and
// gApply on Ctxt<lvl0param> and Ctxt<lvl1param> with one to three inputs.  Keys, encryption and decryption come from the CPU oracle.
//   - 16-bit ripple-carry adders of MAJ = (1, 1, 1) and XOR3 = (2, 2, 2) + 4 mu: two bootstraps per bit, g-forms on device buffers
//     (CtxtCopyH2D in, gApply, CtxtCopyD2H out), one stream per adder
//   - the copying forms on lvl1 ciphertexts: MAJ, a two-input user gate with NAND's numbers, a one-input table function (p = 4)
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

static std::vector<uint32_t> g_s0(ORC_n), g_s1(ORC_K * ORC_N);
static orc_rng g_rng;
static int g_failures = 0;

template <class P> const uint32_t* key() { return detail::level_of<P>() ? g_s1.data() : g_s0.data(); }
template <class P> void encrypt(Ctxt<P>& c, int bit) { orc_tlwe_encrypt(&g_rng, detail::level_of<P>(), key<P>(), bit, c.tlwehost.data()); }
template <class P> int decrypt(Ctxt<P>& c) { return orc_tlwe_decrypt(detail::level_of<P>(), key<P>(), c.tlwehost.data()); }

static void report(const char* what, int bad, int total)
{
    std::printf("%-40s %s (%d/%d failures)\n", what, bad ? "FAIL" : "PASS", bad, total);
    g_failures += bad;
}

static void Adders(UserGate maj, UserGate xor3, std::mt19937& eng)
{
    const int A = 32, B = 16;
    std::vector<Ctxt<TFHEpp::lvl0param>> x(A * B), y(A * B), s(A * B), c(A * (B + 1));
    std::vector<uint32_t> va(A), vb(A);
    std::vector<Stream> st(A);
    for (int i = 0; i < A; i++) {
        st[i].Create();
        va[i] = eng() & 0xFFFF;
        vb[i] = eng() & 0xFFFF;
        for (int k = 0; k < B; k++) {
            encrypt(x[i * B + k], (va[i] >> k) & 1);
            encrypt(y[i * B + k], (vb[i] >> k) & 1);
            CtxtCopyH2D(x[i * B + k], st[i]);
            CtxtCopyH2D(y[i * B + k], st[i]);
        }
        encrypt(c[i * (B + 1)], 0);
        CtxtCopyH2D(c[i * (B + 1)], st[i]);
    }
    for (int k = 0; k < B; k++)
        for (int i = 0; i < A; i++) {
            auto& X = x[i * B + k];
            auto& Y = y[i * B + k];
            auto& C = c[i * (B + 1) + k];
            gApply(xor3, s[i * B + k], X, Y, C, st[i]);
            gApply(maj, c[i * (B + 1) + k + 1], X, Y, C, st[i]);
        }
    for (int i = 0; i < A; i++) {
        for (int k = 0; k < B; k++) CtxtCopyD2H(s[i * B + k], st[i]);
        CtxtCopyD2H(c[i * (B + 1) + B], st[i]);
    }
    Synchronize();
    int bad = 0;
    for (int i = 0; i < A; i++) {
        uint32_t sum = (uint32_t)decrypt(c[i * (B + 1) + B]) << B;
        for (int k = 0; k < B; k++) sum |= (uint32_t)decrypt(s[i * B + k]) << k;
        bad += sum != va[i] + vb[i];
    }
    report("16-bit MAJ/XOR3 adders (gApply, lvl0)", bad, A);
    for (auto& t : st) t.Destroy();
}

static void CopyingForms(UserGate maj, std::mt19937& eng)
{
    using P = TFHEpp::lvl1param;
    const int K = 64;
    const UserGate nand = DefineGate({-1, -1, 0}, ORC_MU);                  // NAND's (ca, cb) and offset: the built-in gate
    const uint32_t eighth = 1u << 29;                                       // p = 4: message m is m / 8
    const std::vector<uint32_t> f = {1, 3, 0, 2};
    std::vector<uint32_t> values(4);
    for (int m = 0; m < 4; m++) values[m] = f[m] * eighth;
    const std::vector<uint32_t> tv = TestVector(values);
    const UserGate table = DefineGate({1, 0, 0}, eighth, tv.data());        // one input: x = (+-1/8) + 1/8 -> message 0 or 2 (bit 0 / 1)
    std::vector<Ctxt<P>> a(K), b(K), c(K), o_maj(K), o_nand(K), o_tab(K);
    std::vector<int> pa(K), pb(K), pc(K);
    Stream st[4];
    for (auto& s : st) s.Create();
    for (int i = 0; i < K; i++) {
        pa[i] = eng() & 1; pb[i] = eng() & 1; pc[i] = eng() & 1;
        encrypt(a[i], pa[i]); encrypt(b[i], pb[i]); encrypt(c[i], pc[i]);
    }
    for (int i = 0; i < K; i++) {
        Apply(maj, o_maj[i], a[i], b[i], c[i], st[i % 4]);
        Apply(nand, o_nand[i], a[i], b[i], st[i % 4]);
        Apply(table, o_tab[i], a[i], st[i % 4]);
    }
    Synchronize();
    int bad_maj = 0, bad_nand = 0, bad_tab = 0;
    for (int i = 0; i < K; i++) {
        bad_maj += decrypt(o_maj[i]) != (pa[i] + pb[i] + pc[i] >= 2);
        bad_nand += decrypt(o_nand[i]) != !(pa[i] && pb[i]);
        // the output is f(m) / 8: decoded to the nearest eighth, not by its sign
        const uint32_t ph = orc_tlwe_phase(1, g_s1.data(), o_tab[i].tlwehost.data());
        bad_tab += ((ph + (eighth >> 1)) >> 29) != f[pa[i] ? 2 : 0];
    }
    report("MAJ, 3 inputs (Apply, lvl1)", bad_maj, K);
    report("NAND as a user gate, 2 inputs (Apply, lvl1)", bad_nand, K);
    report("table function p = 4, 1 input (Apply, lvl1)", bad_tab, K);
    for (auto& s : st) s.Destroy();
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(4242);
    orc_rng_seed(&g_rng, 777);
    orc_keygen(1, g_s0.data(), g_s1.data());
    std::vector<uint32_t> bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_bkgen(1001, g_s0.data(), g_s1.data(), bk.data());
    orc_kskgen(2001, g_s0.data(), g_s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());
    const UserGate maj = DefineGate({1, 1, 1}, 0);
    const UserGate xor3 = DefineGate({2, 2, 2}, 4 * ORC_MU);
    Adders(maj, xor3, eng);
    CopyingForms(maj, eng);
    CleanUp();
    std::printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
