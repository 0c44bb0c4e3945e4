// root_products.cpp -- the tail of the CMux step of blind_rotate_kernel on the CPU: the four-operation products by the eighth
// roots of unity (fpfield.h: mul_root8, mul_root8_cubed), the last inverse pass built from them (ntt_r4.h: gs_pass_hi_last), the
// reduction schedule InverseRootTail6x32 and the FP64 lift, against 128-bit integer arithmetic and against the general passes.
// A stand-alone program (plain g++, also with -fsanitize=address,undefined): prints one line per check, exit status = failed checks.
// The 64 emulated lanes, the r4 twiddle blocks and the schedule of the other passes are those of host_model.cpp, included as it is.
#include <cinttypes>
#include <cstdio>
#include <random>

#include "../../cufhe_amd/csrc/fpfield.h"
#include "../../cufhe_amd/csrc/ntt_r4.h"
#include "../../cufhe_amd/csrc/ntt_tables.h"
#include "host_model.cpp"

namespace {
using namespace cufhe_amd::r4;
typedef __int128 i128;
constexpr double k2p53 = 9007199254740992.0;
const int64_t Z = 5440, Z3 = Z * Z * Z, PI = (int64_t)fpf::P_U64;

int g_failed = 0;
void report(const char* what, long bad, long cases)
{
    printf("%-58s %8ld cases  %s\n", what, cases, bad ? "FAILED" : "ok");
    if (bad) { printf("    %ld violations\n", bad); g_failed++; }
}
bool congruent(i128 a, i128 b) { return (a - b) % (i128)PI == 0; }

// ---- 1. the root products ---------------------------------------------------------------------------------------------
template <class F>
int bad_product(F f, int64_t root, double after, int64_t x)
{
    const double r = f((double)x);
    int bad = 0;
    if (r != std::nearbyint(r) || std::fabs(r) >= k2p53) return 1;
    if (!congruent((i128)x * root, (i128)(int64_t)r)) bad++;
    if (std::fabs(r) > after * fpf::P) bad++;
    return bad;
}
template <class F>
void check_product(const char* name, F f, int64_t root, double after, int64_t divisor)
{
    std::vector<int64_t> xs = {0, 1, PI / 2, PI / 2 + 1, PI, (1ll << 52) - 1, (1ll << 52) + 1, (1ll << 53) - 1};
    // rounding ties of x / divisor: x = k d +- d/2 (d is even) and its neighbours, for the largest k below 2^53 and a few small ones
    const int64_t kmax = ((1ll << 53) - 1 - divisor / 2) / divisor;
    for (int64_t k : {kmax, kmax - 1, kmax / 2, (int64_t)1, (int64_t)0})
        for (int64_t half : {divisor / 2, -divisor / 2})
            for (int64_t d = -1; d <= 1; d++) xs.push_back(k * divisor + half + d);
    long bad = 0, cases = 0;
    for (int64_t x : xs)
        for (int64_t s : {1, -1})
            if (std::llabs(x) < (1ll << 53)) { bad += bad_product(f, root, after, s * x); cases++; }
    report((std::string(name) + ": special values and rounding ties").c_str(), bad, cases);
    std::mt19937_64 rng(1800);
    std::uniform_int_distribution<int64_t> any(-((1ll << 53) - 1), (1ll << 53) - 1);
    bad = 0;
    double worst = 0;
    for (int i = 0; i < 1000000; i++) {
        const int64_t x = any(rng);
        bad += bad_product(f, root, after, x);
        worst = std::fmax(worst, std::fabs(f((double)x)) / fpf::P);
    }
    report((std::string(name) + ": uniform integers below 2^53").c_str(), bad, 1000000);
    printf("    largest |result| / p = %.7f, bound %.7f\n", worst, after);
}

// ---- 2. the last pass against the general one ---------------------------------------------------------------------------
using Spec = FwdDigits<32>::Spectrum;
using Sums = PointwiseSum<Spec, 6, true>;
using Tail = InverseRootTail6x32<Sums>;
using General = Inverse<Sums>;
static_assert(valid(Tail::Out::in()), "the schedule under test");

struct Tw3 { double t[3]; double operator()(int k) const { return t[k]; } };

long last_pass_differs(const double (&in)[16], const Tw3& tw)
{
    double a[16], b[16];
    for (int r = 0; r < 16; r++) a[r] = b[r] = in[r];
    gs_pass_hi_last<Tail::A1>(a);
    gs_pass_hi<Tail::A1>(b, tw);           // the wide / narrow choice of its products from the same bounds
    constexpr RegBounds ob = Tail::Out::in();
    long bad = 0;
    for (int r = 0; r < 16; r++) {
        if (a[r] != std::nearbyint(a[r]) || std::fabs(a[r]) >= k2p53) { bad++; continue; }
        if (!congruent((i128)(int64_t)a[r], (i128)(int64_t)b[r])) bad++;
        if (std::fabs(a[r]) > ob.v[r] * fpf::P) bad++;
    }
    return bad;
}
void check_last_pass()
{
    static cufhe_amd::NttTables t;
    cufhe_amd::build_tables(t, true);
    const Tw3 tw = {{t.tu_inv[0], t.tu_inv[1], t.tu_inv[2]}};
    // the signs the butterfly takes into its differences are the table's: w = -I, v = -zeta^3, v w = -zeta
    report("table slots 0-2 of the last pass are -I, -zeta^3, -zeta", (tw.t[0] != -fpf::ROOT4) + (tw.t[1] != -(double)Z3) + (tw.t[2] != -(double)Z), 3);
    constexpr RegBounds ib = Tail::A1::in();
    printf("    input bounds of the pass (units of p):");
    for (int r = 0; r < 16; r++) printf(" %.3f", ib.v[r]);
    printf("\n");
    std::mt19937_64 rng(1801);
    long bad = 0;
    for (int i = 0; i < 20000; i++) {
        double x[16];
        for (int r = 0; r < 16; r++) {
            const int64_t m = (int64_t)std::floor(ib.v[r] * fpf::P);
            x[r] = (double)std::uniform_int_distribution<int64_t>(-m, m)(rng);
        }
        bad += last_pass_differs(x, tw);
    }
    report("last pass = general pass (mod p), random inputs at the bounds", bad, 20000);
    bad = 0;
    for (int signs = 0; signs < 16; signs++) {         // all-maximum inputs, every combination of signs within a group
        double x[16];
        for (int r = 0; r < 16; r++) x[r] = ((signs >> (r >> 2)) & 1 ? -1.0 : 1.0) * std::floor(ib.v[r] * fpf::P);
        bad += last_pass_differs(x, tw);
    }
    report("last pass = general pass (mod p), all-maximum inputs", bad, 16);
}

// ---- 3. the lift ----------------------------------------------------------------------------------------------------------
constexpr double kSumMax = 2.0 * 3 * 1024 * 32 * 2147483648.0;         // (k+1) l N (Bg/2) 2^31: the largest true value of a sum
uint32_t tail_lift(double v, int reg)
{
    constexpr RegBounds b = Tail::Out::in();
    return fpf::lift_reduced_ok(b.v[reg], kSumMax / fpf::P + 1e-3) ? fpf::lift_u32_reduced(v) : fpf::lift_u32(v);
}
void check_lift()
{
    constexpr RegBounds b = Tail::Out::in();
    const double cmax = kSumMax / fpf::P + 1e-3;           // as the kernel rounds it up (thousandths of p)
    std::mt19937_64 rng(1802);
    std::uniform_int_distribution<int64_t> value(-(int64_t)kSumMax, (int64_t)kSumMax);
    long bad = 0, cases = 0, direct = 0;
    for (int r = 0; r < 16; r++) {
        const bool red = fpf::lift_reduced_ok(b.v[r], cmax);
        direct += red;
        for (int i = 0; i < 20000; i++) {
            const int64_t c = i == 0 ? (int64_t)kSumMax : i == 1 ? -(int64_t)kSumMax : i == 2 ? 0 : value(rng);
            for (int k = -11; k <= 11; k++) {
                const i128 a = (i128)c + (i128)k * PI;
                const double mag = (double)(a < 0 ? -a : a);
                if (mag > b.v[r] * fpf::P || mag >= k2p53) continue;          // not a value this register can hold
                if (red && k != 0) bad++;                                       // a reduced register holds nothing but c itself
                const double v = (double)(int64_t)a;
                const uint32_t want = (uint32_t)(uint64_t)c;
                if (fpf::lift_u32(v) != want || tail_lift(v, r) != want) bad++;
                cases++;
            }
        }
    }
    report("lift per register = lift_u32 = c mod 2^32 on c + k p", bad, cases);
    printf("    %ld of 16 registers take the rounding add alone\n", direct);
    report("twelve registers of the tail need no reduction in the lift", direct != 12, 1);
}

// ---- 4. the whole external product on 64 lanes, every value against the bound of its register --------------------------------
template <class V>
void inverse_tail(double* X, r4m::Check& ck)
{
    using namespace r4m;
    per_lane(X, 'C', [&](double (&x)[16], int lane) {
        ck.regs<typename V::In>(x);
        gs_pass_lo<typename V::In, 0, 4>(x, block_c_r4(g_inv, lane));
        ck.regs<typename V::C1>(x);
        reduce_mask<V::kMaskC1>(x);
    });
    per_lane(X, 'B', [&](double (&x)[16], int lane) {
        const Block tw = block_r4(g_inv, 16, lane & 15);
        ck.regs<typename V::B0>(x);
        gs_pass_lo<typename V::B0, 3, 7>(x, tw);
        ck.regs<AfterGs<typename V::B0, false>>(x);
        reduce_mask<V::kMaskB0>(x);
        ck.regs<typename V::B1>(x);
        gs_pass_hi<typename V::B1>(x, tw);
        ck.regs<AfterGs<typename V::B1, true>>(x);
        reduce_mask<V::kMaskB1>(x);
        ck.regs<typename V::B2>(x);
    });
    per_lane(X, 'A', [&](double (&x)[16], int) {
        const Block tw = block_r4(g_inv, 1, 0);
        ck.regs<typename V::A0>(x);
        gs_pass_lo<typename V::A0, 3, 7>(x, tw);
        ck.regs<AfterGs<typename V::A0, false>>(x);
        reduce_mask<V::kMaskA0>(x);
        ck.regs<typename V::A1>(x);
        gs_pass_hi_last<typename V::A1>(x);
        ck.regs<typename V::Out>(x);
    });
}
// hm_external_product_r4 of host_model.cpp with the tail under test; returns violations, *worst = largest value / its bound
long external_product_tail(uint32_t* out, const int32_t* dig, const uint32_t* bk, double* worst)
{
    using namespace r4m;
    tables();
    Track t;
    Check ck;
    constexpr RegBounds sb = Spec::in();
    std::vector<double> A0(N, 0.0), A1(N, 0.0), x(N), y0(N), y1(N);
    for (int row = 0; row < 6; row++) {
        for (int i = 0; i < N; i++) {
            x[i] = (double)dig[row * N + i];
            y0[i] = (double)(int32_t)bk[(row * 2 + 0) * N + i];
            y1[i] = (double)(int32_t)bk[(row * 2 + 1) * N + i];
        }
        forward_digits<32>(x.data(), ck);
        fwd(y0.data(), t, nullptr, false); fwd(y1.data(), t, nullptr, false);
        for (int i = 0; i < N; i++) {
            y0[i] = fpf::reduce(mm(y0[i], g_ninv, true, t));
            y1[i] = fpf::reduce(mm(y1[i], g_ninv, true, t));
            const bool wide = needs_wide(sb.v[i & 15]);
            if (row == 5) {
                A0[i] = wide ? fpf::mulmod_add_wide(x[i], y0[i], A0[i]) : fpf::mulmod_add(x[i], y0[i], A0[i]);
                A1[i] = wide ? fpf::mulmod_add_wide(x[i], y1[i], A1[i]) : fpf::mulmod_add(x[i], y1[i], A1[i]);
            } else {
                A0[i] += wide ? fpf::mulmod_wide(x[i], y0[i]) : fpf::mulmod(x[i], y0[i]);
                A1[i] += wide ? fpf::mulmod_wide(x[i], y1[i]) : fpf::mulmod(x[i], y1[i]);
            }
        }
    }
    inverse_tail<Tail>(A0.data(), ck); inverse_tail<Tail>(A1.data(), ck);
    for (int i = 0; i < N; i++) { out[i] = tail_lift(A0[i], i >> 6); out[N + i] = tail_lift(A1[i], i >> 6); }
    *worst = ck.worst;
    return t.bad + ck.bad;
}
void check_external_product()
{
    std::mt19937_64 rng(1803);
    std::vector<int32_t> dig(6 * N);
    std::vector<uint32_t> bk(12 * N), got(2 * N), want(2 * N);
    const char* names[] = {"all digits -32, all key words 0x80000000", "digits -32, key words 0x80000000 / 0x7fffffff by turns",
                           "random digits of either extreme, random key words", "random digits, random key words"};
    for (int c = 0; c < 5; c++) {
        for (auto& d : dig) d = c <= 1 ? -32 : c == 2 ? ((rng() & 1) ? -32 : 31) : (int32_t)(rng() % 64) - 32;
        for (size_t i = 0; i < bk.size(); i++) bk[i] = c == 0 ? 0x80000000u : c == 1 ? ((i & 1) ? 0x7fffffffu : 0x80000000u) : (uint32_t)rng();
        double worst = 0, stats[40];
        long bad = external_product_tail(got.data(), dig.data(), bk.data(), &worst);
        hm_external_product_r4(want.data(), dig.data(), bk.data(), stats);      // the general schedule, which tests/test_fpfield.py holds against the schoolbook product
        bad += (long)stats[0];
        for (int i = 0; i < 2 * N; i++) bad += got[i] != want[i];
        if (worst > 1.0) bad++;
        report((std::string("external product, tail schedule: ") + names[c < 4 ? c : 3]).c_str(), bad, 2 * N);
        printf("    largest value / bound of its register = %.4f\n", worst);
    }
}
}  // namespace

int main()
{
    check_product("mul_root8", [](double x) { return fpf::mul_root8(x); }, Z, fpf::AFTER_MUL_ROOT8, Z3);
    check_product("mul_root8_cubed", [](double x) { return fpf::mul_root8_cubed(x); }, Z3, fpf::AFTER_MUL_ROOT8_CUBED, Z);
    check_last_pass();
    check_lift();
    check_external_product();
    printf("%d checks failed\n", g_failed);
    return g_failed;
}
