// CPU checks of cufhe_amd/csrc/ks_matrix.h, the arithmetic of keyswitch_mm_kernel (tests/test_ks_matrix.py): the balanced
// base-256 split of a key word, the expansion of a digit word into the coefficients of an A fragment, the plane-wise product
// against the word-wise sum that ks_digit_acc (kernels.hip.h) describes, and the bound of a plane sum.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../cufhe_amd/csrc/ks_matrix.h"

static int g_failed = 0;
static void check(bool ok, const char* what)
{
    if (!ok) g_failed++;
    printf("%s %s\n", what, ok ? "ok" : "FAILED");
}

// the key switch of one j as keyswitch_kernel does it: field f of the digit word adds row (v = 2), adds row (v = 1), nothing, or
// subtracts row (v = 1); rows[kappa * 2 + (v - 1)]
static uint32_t wordwise(unsigned dw, const std::vector<uint32_t>& rows, int words, int i)
{
    uint32_t r = 0;
    for (int kappa = 0; kappa < ksmm::kFields; kappa++) {
        const unsigned f = (dw >> (16 - 2 * (kappa + 1))) & 3u;
        if (f == 0) r += rows[(size_t)(kappa * 2 + 1) * words + i];
        else if (f == 1) r += rows[(size_t)(kappa * 2) * words + i];
        else if (f == 3) r -= rows[(size_t)(kappa * 2) * words + i];
    }
    return r;
}

static bool split_ok(uint32_t w)
{
    uint32_t sum = 0;
    for (int b = 0; b < ksmm::kPlanes; b++) {
        const int d = ksmm::plane_digit(w, b);
        if (d < -128 || d > 127) return false;
        sum += (uint32_t)d << (8 * b);
    }
    return sum == w;
}

int main()
{
    std::mt19937_64 rng(20261019);

    {   // digit split
        bool ok = true;
        for (uint32_t w : {0u, 0x7fu, 0x80u, 0xffu, 0x7fffffffu, 0x80000000u, 0x80808080u, 0x7f7f7f7fu, 0xffffffffu}) ok = ok && split_ok(w);
        check(ok, "digit split: the named words");
        ok = true;
        // every single-byte pattern that carries into the next plane (byte value >= 128), in each plane, alone and on a background
        // of 0x7f (a carry that stops) and of 0xff / 0x7f...ff (a carry that runs on)
        for (int b = 0; b < ksmm::kPlanes; b++)
            for (uint32_t v = 0x80; v <= 0xff; v++)
                for (uint32_t bg : {0u, 0x7f7f7f7fu, 0xffffffffu, 0x7fffffffu}) ok = ok && split_ok((bg & ~(0xffu << (8 * b))) | (v << (8 * b)));
        check(ok, "digit split: every carrying byte in every plane");
        ok = true;
        for (int i = 0; i < 100000; i++) ok = ok && split_ok((uint32_t)rng());
        check(ok, "digit split: 100000 random words");
        ok = ksmm::recombine(ksmm::plane_digit(0x80808080u, 0), ksmm::plane_digit(0x80808080u, 1), ksmm::plane_digit(0x80808080u, 2),
                             ksmm::plane_digit(0x80808080u, 3)) == 0x80808080u &&
             ksmm::plane_digit(0x80u, 0) == -128 && ksmm::plane_digit(0x80u, 1) == 1 && ksmm::plane_digit(0xffffffffu, 3) == 0;
        check(ok, "digit split: recombine, and the digits of 0x80 and 0xffffffff");
    }

    {   // digit-word expansion: all 65536 words, by slot and through the byte table the kernel keeps
        bool ok = true, table = true;
        for (unsigned dw = 0; dw < 65536; dw++) {
            for (int e = 0; e < ksmm::kSlots; e++) {
                const unsigned f = (dw >> (16 - 2 * (e / 2 + 1))) & 3u;
                const int want = e % 2 == 0 ? (f == 1 ? 1 : f == 3 ? -1 : 0) : (f == 0 ? 1 : 0);     // row v = 1 / row v = 2
                ok = ok && ksmm::slot_coeff(dw, e) == want && ksmm::slot_kappa(e) * 2 + (ksmm::slot_v(e) - 1) == e;
                const uint64_t regs = ksmm::expand_byte(e < 8 ? dw >> 8 : dw & 0xffu);
                table = table && (int)(int8_t)(uint8_t)(regs >> (8 * (e % 8))) == want;
            }
        }
        check(ok, "digit-word expansion: 65536 words x 16 slots");
        check(table, "digit-word expansion: the 256-entry byte table");
        bool null_word = true;
        for (int e = 0; e < ksmm::kSlots; e++) null_word = null_word && ksmm::slot_coeff(ksmm::kNullDigitWord, e) == 0;
        check(null_word, "digit-word expansion: the null word");
    }

    {   // reference product: 1000 random (digit word, 16 rows of 640 words)
        const int words = 640;
        bool ok = true;
        long long max_abs = 0;
        std::vector<uint32_t> rows((size_t)ksmm::kSlots * words);
        for (int it = 0; it < 1000; it++) {
            const unsigned dw = (unsigned)(rng() & 0xffffu);
            for (auto& w : rows) w = (uint32_t)rng();
            if (it % 4 == 1) for (auto& w : rows) w = (w & 1u) ? 0x80808080u : 0x7f7f7f7fu;      // extreme digits
            for (int i = 0; i < words; i++) {
                int32_t c[ksmm::kPlanes];
                for (int b = 0; b < ksmm::kPlanes; b++) {
                    long long sum = 0;
                    for (int e = 0; e < ksmm::kSlots; e++) sum += (long long)ksmm::slot_coeff(dw, e) * ksmm::plane_digit(rows[(size_t)e * words + i], b);
                    if (sum < 0 ? -sum > max_abs : sum > max_abs) max_abs = sum < 0 ? -sum : sum;
                    c[b] = (int32_t)sum;
                }
                ok = ok && ksmm::recombine(c[0], c[1], c[2], c[3]) == wordwise(dw, rows, words, i);
            }
        }
        check(ok, "reference product: plane-wise int32 sums recombine to the word-wise sum");
        check(max_abs <= ksmm::kFields * 128, "reference product: a j adds at most 8 x 128 to a plane sum");
    }

    {   // bound: K = 16384 slots at |d| = 128 (one live row per field would already be half of this)
        long long sum = 0;
        for (int k = 0; k < ksmm::kKnMax * ksmm::kSlots; k++) sum += 128;
        check(sum == (1ll << 21) && sum == ksmm::kMaxPartialSum && sum < (1ll << 31), "bound: 16384 x 128 = 2^21 < 2^31");
        // the worst key and digits in the arithmetic itself: every word 0x80808080 (planes -128, -127, -127, -127), every field 1
        long long c0 = 0;
        for (int j = 0; j < ksmm::kKnMax; j++)
            for (int e = 0; e < ksmm::kSlots; e++) c0 += (long long)ksmm::slot_coeff(0x5555u, e) * ksmm::plane_digit(0x80808080u, 0);
        check(c0 == -(1ll << 20), "bound: 1024 x 8 rows of digit -128 sum to -2^20");
    }

    printf("%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
