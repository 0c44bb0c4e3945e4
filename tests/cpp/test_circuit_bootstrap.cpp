// test_circuit_bootstrap.cpp -- a ROM read through include/cufhe_amd.hpp on Streams: address bits as Ctxt<lvl0param>,
// CircuitBootstrapping into cuFHETRGSWNTTlvl1 selectors, then a CMUX tree (CMUXNTT on the ROM entries' host words, gCMUXNTT above)
// whose root is fetched to the host.  One stream per address, everything recorded before one Synchronize().
//
// Usage: test_circuit_bootstrap DIR BITS ADDRESSES
// DIR holds the keys and ciphertexts as raw little-endian words (written by tests/test_gpu_circuit_bootstrap.py):
//   bk.u32 ksk.u32 (lvl01 / lvl10), bk2.u64 ksk2.u32 (lvl02 / lvl20), pksk.u32 (private key switching lvl2 -> lvl1),
//   rom.u32 [2^BITS][2][N], addr.u32 [ADDRESSES][BITS][n + 1] (bit k of address a).
// Writes DIR/out.u32 [ADDRESSES][2][N]: the root of each tree; the caller decrypts it.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cufhe_amd.hpp"

using namespace cufhe;

template <class T>
static std::vector<T> load(const std::string& path)
{
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "short read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s DIR BITS ADDRESSES\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int bits = std::atoi(argv[2]), A = std::atoi(argv[3]), R = 1 << bits;
    constexpr size_t N = TFHEpp::lvl1param::n, W0 = TFHEpp::lvl0param::n + 1;
    SetGPUNum(1);
    {
        auto bk = load<uint32_t>(dir + "/bk.u32");
        auto ksk = load<uint32_t>(dir + "/ksk.u32");
        Initialize(bk.data(), bk.size(), ksk.data(), ksk.size());
        auto bk2 = load<uint64_t>(dir + "/bk2.u64");
        auto ksk2 = load<uint32_t>(dir + "/ksk2.u32");
        lvl2::Initialize(bk2.data(), bk2.size(), ksk2.data(), ksk2.size());
        auto pksk = load<uint32_t>(dir + "/pksk.u32");
        InitializeCircuitBootstrapping(pksk.data(), pksk.size());
    }
    const auto rom_words = load<uint32_t>(dir + "/rom.u32");
    const auto addr_words = load<uint32_t>(dir + "/addr.u32");
    if (rom_words.size() != (size_t)R * 2 * N || addr_words.size() != (size_t)A * bits * W0) { std::fprintf(stderr, "bad sizes\n"); return 2; }

    std::vector<std::unique_ptr<cuFHETRLWElvl1>> rom;
    for (int r = 0; r < R; r++) {
        rom.emplace_back(new cuFHETRLWElvl1);
        std::memcpy(rom.back()->trlwehost[0].data(), &rom_words[(size_t)r * 2 * N], 2 * N * sizeof(uint32_t));
    }
    std::vector<Stream> st(A);
    std::vector<std::unique_ptr<Ctxt<TFHEpp::lvl0param>>> in;
    std::vector<std::unique_ptr<cuFHETRGSWNTTlvl1>> sel;
    std::vector<std::unique_ptr<cuFHETRLWElvl1>> nodes;
    std::vector<cuFHETRLWElvl1*> root(A);
    for (int a = 0; a < A; a++) {
        st[a].Create();
        std::vector<cuFHETRGSWNTTlvl1*> s(bits);
        for (int k = 0; k < bits; k++) {
            in.emplace_back(new Ctxt<TFHEpp::lvl0param>);
            std::memcpy(in.back()->tlwehost.data(), &addr_words[((size_t)a * bits + k) * W0], W0 * sizeof(uint32_t));
            sel.emplace_back(new cuFHETRGSWNTTlvl1);
            CircuitBootstrapping(*sel.back(), *in.back(), st[a]);       // from tlwehost: uploaded in stream order
            s[k] = sel.back().get();
        }
        std::vector<cuFHETRLWElvl1*> level;
        for (auto& e : rom) level.push_back(e.get());
        for (int k = 0; k < bits; k++) {
            std::vector<cuFHETRLWElvl1*> next;
            for (size_t j = 0; j + 1 < level.size(); j += 2) {
                nodes.emplace_back(new cuFHETRLWElvl1);
                if (k == 0) CMUXNTT(*nodes.back(), *s[k], *level[j + 1], *level[j], st[a]);    // the ROM's host words
                else gCMUXNTT(*nodes.back(), *s[k], *level[j + 1], *level[j], st[a]);
                next.push_back(nodes.back().get());
            }
            level = next;
        }
        root[a] = level[0];
        CUFHE_AMD_CHECK(cufhe_amd_enqueue_copy(st[a].device_id(), st[a].raw(), root[a]->handle, 0));
    }
    Synchronize();
    FILE* f = std::fopen((dir + "/out.u32").c_str(), "wb");
    for (int a = 0; a < A; a++) std::fwrite(root[a]->trlwehost[0].data(), sizeof(uint32_t), 2 * N, f);
    std::fclose(f);
    nodes.clear(); sel.clear(); in.clear(); rom.clear();
    for (auto& s : st) s.Destroy();
    CleanUp();
    std::printf("ROM read of %d addresses over %d entries: done\n", A, R);
    return 0;
}
