// test_ps_user_gates.cpp -- user gates on a compiled parameter set through include/cufhe_amd.hpp.  Built with
// -DCUFHE_AMD_PARAM_SET_K2N512 (tests/ps_user_gate_checker.py): Initialize puts the per-gate API on the `k2n512` set, and DefineGate,
// TestVector, TestVectorMulti, Apply, gApply and ApplyMulti then define and run gates of THAT set (cufhe_amd_ps_define_gate) with its
// N = 512 and k = 2.  Keys, encryption and decryption come from the CPU oracle compiled for the same set.
//   - 4-bit ripple-carry adders of MAJ = (1, 1, 1) and XOR3 = (2, 2, 2) + 4 mu on Ctxt<lvl0param>: g-forms on device buffers, one
//     stream per adder, decrypted against the plain sum
//   - the copying forms on Ctxt<lvl1param>: MAJ, NAND's numbers as a user gate, a one-input table function (p = 4) through TestVector
//   - a full adder from ONE two-output gate (TestVectorMulti, ApplyMulti) on Ctxt<lvl0param>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;

static_assert(kParamSetIndex == 1 && TFHEpp::lvl1param::n == 512 && TFHEpp::lvl1param::k == 2, "this program is built for the k2n512 set");
static_assert(ORC_N == 512 && ORC_K == 2, "the oracle must be compiled for the same set (-DORC_SET_K2N512)");

static std::vector<uint32_t> g_s0(ORC_n), g_s1(ORC_K * ORC_N);
static orc_rng g_rng;
static int g_failures = 0;

template <class P> const uint32_t* key() { return detail::level_of<P>() ? g_s1.data() : g_s0.data(); }
template <class P> void encrypt(Ctxt<P>& c, int bit) { orc_tlwe_encrypt(&g_rng, detail::level_of<P>(), key<P>(), bit, c.tlwehost.data()); }
template <class P> int decrypt(Ctxt<P>& c) { return orc_tlwe_decrypt(detail::level_of<P>(), key<P>(), c.tlwehost.data()); }

static void report(const char* what, int bad, int total)
{
    std::printf("%-52s %s (%d/%d failures)\n", what, bad ? "FAIL" : "PASS", bad, total);
    g_failures += bad;
}

static void Adders(UserGate maj, UserGate xor3, std::mt19937& eng)
{
    const int A = 8, B = 4;
    std::vector<Ctxt<TFHEpp::lvl0param>> x(A * B), y(A * B), s(A * B), c(A * (B + 1));
    std::vector<uint32_t> va(A), vb(A);
    std::vector<Stream> st(A);
    for (int i = 0; i < A; i++) {
        st[i].Create();
        va[i] = eng() & 0xF;
        vb[i] = eng() & 0xF;
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
    report("4-bit MAJ/XOR3 adders (gApply, lvl0)", bad, A);
    for (auto& t : st) t.Destroy();
}

static void CopyingForms(UserGate maj, std::mt19937& eng)
{
    using P = TFHEpp::lvl1param;
    const int K = 16;
    const UserGate nand = DefineGate({-1, -1, 0}, ORC_MU);                  // NAND's (ca, cb) and offset: the built-in gate
    const uint32_t eighth = 1u << 29;                                       // p = 4: message m is m / 8
    const std::vector<uint32_t> f = {1, 3, 0, 2};
    std::vector<uint32_t> values(4);
    for (int m = 0; m < 4; m++) values[m] = f[m] * eighth;
    const std::vector<uint32_t> tv = TestVector(values);
    if (tv.size() != 512) report("TestVector has the set's N words", 1, 1);
    const UserGate table = DefineGate({1, 0, 0}, eighth, tv.data());        // one input: x = (+-1/8) + 1/8 -> message 0 or 2 (bit 0 / 1)
    if (table.op < CUFHE_AMD_PS_USER_OP_BASE) report("DefineGate returns an id of the parameter sets' range", 1, 1);
    std::vector<Ctxt<P>> a(K), b(K), c(K), o_maj(K), o_nand(K), o_tab(K);
    std::vector<int> pa(K), pb(K), pc(K);
    Stream st[2];
    for (auto& s : st) s.Create();
    for (int i = 0; i < K; i++) {
        pa[i] = eng() & 1; pb[i] = eng() & 1; pc[i] = eng() & 1;
        encrypt(a[i], pa[i]); encrypt(b[i], pb[i]); encrypt(c[i], pc[i]);
    }
    for (int i = 0; i < K; i++) {
        Apply(maj, o_maj[i], a[i], b[i], c[i], st[i % 2]);
        Apply(nand, o_nand[i], a[i], b[i], st[i % 2]);
        Apply(table, o_tab[i], a[i], st[i % 2]);
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

// t = ones of (a, b, c): a + b + c + 3 mu = 2 t mu lies on box 2 t of p = 4 (t >= 2: the negacyclic wrap of box 2 t - 4); output 0 is
// the carry as +-mu, output 1 the sum bit as 0 / 2^31 -- both functions with f(t + 2) = -f(t)
static void TwoOutputAdder()
{
    using P = TFHEpp::lvl0param;
    const uint32_t mu = ORC_MU;
    const std::vector<uint32_t> tv = TestVectorMulti({{0u - mu, 0u - mu, 0u - mu, 0u - mu}, {0u, 0u, 1u << 31, 1u << 31}}, 4);
    const UserGate adder = DefineGate({1, 1, 1}, 3 * mu, tv.data(), 2);
    std::vector<Ctxt<P>> a(8), b(8), c(8), carry(8), sum(8);
    Stream st;
    st.Create();
    for (int i = 0; i < 8; i++) {
        encrypt(a[i], (i >> 2) & 1); encrypt(b[i], (i >> 1) & 1); encrypt(c[i], i & 1);
        ApplyMulti<P>(adder, {&carry[i], &sum[i]}, a[i], b[i], c[i], st);
    }
    Synchronize();
    int bad = 0;
    for (int i = 0; i < 8; i++) {
        const int t = ((i >> 2) & 1) + ((i >> 1) & 1) + (i & 1);
        const uint32_t ph = orc_tlwe_phase(0, g_s0.data(), sum[i].tlwehost.data());
        bad += decrypt(carry[i]) != (t >= 2);
        bad += (int)(((ph + (1u << 30)) >> 31) & 1) != (t & 1);
    }
    report("full adder from one two-output gate (ApplyMulti, lvl0)", bad, 16);
    st.Destroy();
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
    TwoOutputAdder();
    CleanUp();
    std::printf(g_failures ? "FAILURES: %d\n" : "ALL PASS\n", g_failures);
    return g_failures ? 1 : 0;
}
