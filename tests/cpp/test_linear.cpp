// test_linear.cpp -- linear layers through include/cufhe_amd.hpp: DefineLinear, gLinear and gLinearApply on Ctxt<lvl0param>.
// The inputs are random 32-bit words (the layer is word arithmetic: every input has one right answer).  Checked: gLinear against the
// defining sum of INTEGRATION.md section 14 computed on the host, and gLinearApply against the words of cufhe_amd_linear_gate_batch
// on a contiguous copy of the same inputs -- the C entry point tests/test_gpu_linear.py holds against the composed checker.
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "../../include/cufhe_amd.hpp"
#include "../../oracle/tfhe_oracle.h"

using namespace cufhe;
using C0 = Ctxt<TFHEpp::lvl0param>;

constexpr int W0 = ORC_n + 1, N = ORC_N;

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::mt19937 eng(1414);
    std::vector<uint32_t> s0(ORC_n), s1(ORC_K * ORC_N), bk(ORC_BK_WORDS), ksk(ORC_KSK_WORDS);
    orc_keygen(1, s0.data(), s1.data());
    orc_bkgen(1001, s0.data(), s1.data(), bk.data());
    orc_kskgen(2001, s0.data(), s1.data(), ksk.data());
    SetGPUNum(1);
    Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());
    int failures = 0;
    auto report = [&](const char* what, bool ok) {
        std::printf("%-64s %s\n", what, ok ? "PASS" : "FAIL");
        failures += !ok;
    };

    constexpr size_t rows = 3, cols = 5;
    std::vector<int32_t> W(rows * cols);
    for (auto& w : W) w = (int32_t)eng();
    W[0] = INT32_MIN; W[1] = INT32_MAX; W[2] = -1; W[3] = 0;
    std::vector<uint32_t> bias(rows);
    for (auto& b : bias) b = eng();
    const LinearLayer layer = DefineLinear(rows, cols, W.data(), bias.data());
    size_t r = 0, c = 0;
    CUFHE_AMD_CHECK(cufhe_amd_linear_get(layer.id, &r, &c));
    report("linear: the layer reports its shape", r == rows && c == cols && layer.id >= CUFHE_AMD_LINEAR_LAYER_BASE);

    Stream st;
    st.Create();
    std::vector<std::unique_ptr<C0>> x, y, z;
    std::vector<C0*> ins, outs, acts;
    for (size_t k = 0; k < cols; k++) {
        x.emplace_back(new C0);
        for (int i = 0; i < W0; i++) x[k]->tlwehost[i] = eng();
        CtxtCopyH2D(*x[k], st);          // recorded: launched by the fence inside gLinear
        ins.push_back(x[k].get());
    }
    for (size_t j = 0; j < rows; j++) {
        y.emplace_back(new C0); z.emplace_back(new C0);
        outs.push_back(y[j].get()); acts.push_back(z[j].get());
    }
    gLinear(outs, layer, ins, st);
    for (size_t j = 0; j < rows; j++) CtxtCopyD2H(*y[j], st);
    Synchronize();
    bool sums_ok = true;
    for (size_t j = 0; j < rows; j++)
        for (int i = 0; i < W0; i++) {
            uint32_t want = i == W0 - 1 ? bias[j] : 0u;
            for (size_t k = 0; k < cols; k++) want += (uint32_t)W[j * cols + k] * x[k]->tlwehost[i];
            sums_ok &= y[j]->tlwehost[i] == want;
        }
    report("gLinear: the words of the defining sum", sums_ok);

    // a random test vector behind the layer
    std::vector<uint32_t> tv(N);
    for (auto& t : tv) t = eng();
    const UserGate act = DefineGate({1, 0, 0}, 0x12345678u, tv.data());
    gLinearApply(act, acts, layer, ins, st);
    for (size_t j = 0; j < rows; j++) CtxtCopyD2H(*z[j], st);
    Synchronize();
    // the same through the C entry point on contiguous arrays
    const int dev = st.device_id();
    void *din = nullptr, *dout = nullptr;
    CUFHE_AMD_CHECK(cufhe_amd_malloc(dev, cols * W0 * sizeof(uint32_t), &din));
    CUFHE_AMD_CHECK(cufhe_amd_malloc(dev, rows * W0 * sizeof(uint32_t), &dout));
    std::vector<uint32_t> flat(cols * W0), got(rows * W0);
    for (size_t k = 0; k < cols; k++)
        for (int i = 0; i < W0; i++) flat[k * W0 + i] = x[k]->tlwehost[i];
    CUFHE_AMD_CHECK(cufhe_amd_memcpy_h2d(dev, st.raw(), din, flat.data(), flat.size() * sizeof(uint32_t)));
    CUFHE_AMD_CHECK(cufhe_amd_linear_gate_batch(dev, st.raw(), layer.id, act.op, 0, 1, (const uint32_t*)din, W0, (uint32_t*)dout, W0));
    CUFHE_AMD_CHECK(cufhe_amd_memcpy_d2h(dev, st.raw(), got.data(), dout, got.size() * sizeof(uint32_t)));
    CUFHE_AMD_CHECK(cufhe_amd_stream_synchronize(dev, st.raw()));
    bool act_ok = true, moved = false;
    for (size_t j = 0; j < rows; j++)
        for (int i = 0; i < W0; i++) {
            act_ok &= z[j]->tlwehost[i] == got[j * W0 + i];
            moved |= z[j]->tlwehost[i] != y[j]->tlwehost[i];
        }
    report("gLinearApply: the words of cufhe_amd_linear_gate_batch", act_ok && moved);
    CUFHE_AMD_CHECK(cufhe_amd_free(dev, din));
    CUFHE_AMD_CHECK(cufhe_amd_free(dev, dout));

    report("linear: a null array is refused", cufhe_amd_linear_list(dev, st.raw(), layer.id, 0, 1, nullptr, nullptr) == -1);
    x.clear(); y.clear(); z.clear();
    st.Destroy();
    CleanUp();
    report("linear: CleanUp drops the layer", cufhe_amd_linear_get(layer.id, &r, &c) == -1);
    std::printf(failures ? "%d FAILED\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
