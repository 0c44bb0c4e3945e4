// ntt_tables_harness.cpp -- the library's own twiddle-table builders (cufhe_amd/csrc/ntt_tables.h) on the CPU, for
// tests/test_ntt_tables.py.  Plain g++, no HIP.
//   ntt_tables_harness tables   the thirteen tables as the library uploads them, raw bytes on stdout, in this order:
//                               1024-point plain, 1024-point r4, lvl2 halves 0 1 (NttTables);
//                               512-point 0 1 2 (r4 products on the halves 0 and 1, not on the stand-alone 2), lvl2 quarters 0-3
//                               (r4 products on all four) (Ntt512Tables)
//   ntt_tables_harness roots    one JSON object: the constants, the root arrays the tables are cut from and their sub-transforms
#include <cstdio>
#include <cstring>

#include "../../cufhe_amd/csrc/ntt_tables.h"

using namespace cufhe_amd;

namespace {
void put(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }

int tables()
{
    static NttTables plain, r4, half2[2];
    static Ntt512Tables t512[3], quarter[4];
    build_tables(plain);
    build_tables(r4, true);
    build_tables_lvl2(half2);
    build_tables_512(t512);
    for (int h = 0; h < 2; h++)
        if (!fill_r4_products_512(t512[h])) return 2;
    build_tables_lvl2q(quarter);
    for (int q = 0; q < 4; q++)
        if (!fill_r4_products_512(quarter[q])) return 3;
    put(&plain, sizeof plain);
    put(&r4, sizeof r4);
    put(half2, sizeof half2);
    put(t512, sizeof t512);
    put(quarter, sizeof quarter);
    return 0;
}

// every entry is an integer below 2^50 in magnitude: printed exactly
void array(const char* name, const std::vector<double>& v, const char* end)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? ", " : "", (long long)v[i]);
    printf("]%s", end);
}
void roots_json(const char* name, const Roots& r, const char* end)
{
    printf("\"%s\": {", name);
    array("fwd", r.fwd, ", ");
    array("inv", r.inv, "}");
    printf("%s\n", end);
}
int roots()
{
    const Roots r1024 = negacyclic_roots(fpf::PSI_2048, 10), r2048 = negacyclic_roots(kPsi4096, 11);
    printf("{\"p\": %llu, \"psi_2048\": %llu, \"psi_4096\": %llu, \"root4\": %lld,\n", (unsigned long long)fpf::P_U64,
           (unsigned long long)fpf::PSI_2048, (unsigned long long)kPsi4096, (long long)fpf::ROOT4);
    printf("\"n_inverse\": {\"512\": %lld, \"1024\": %lld, \"2048\": %lld},\n", (long long)n_inverse(512), (long long)n_inverse(1024),
           (long long)n_inverse(2048));
    roots_json("roots_512", negacyclic_roots(mulmod_u64(fpf::PSI_2048, fpf::PSI_2048), 9), ",");
    roots_json("roots_1024", r1024, ",");
    roots_json("roots_2048", r2048, ",");
    char name[32];
    for (int h = 0; h < 2; h++) {
        snprintf(name, sizeof name, "half_%d_of_1024", h);
        roots_json(name, sub_transform(r1024, 2, h), ",");
        snprintf(name, sizeof name, "half_%d_of_2048", h);
        roots_json(name, sub_transform(r2048, 2, h), ",");
    }
    for (int q = 0; q < 4; q++) {
        snprintf(name, sizeof name, "quarter_%d_of_2048", q);
        roots_json(name, sub_transform(r2048, 4, q), q < 3 ? "," : "}");
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "tables")) return tables();
    if (argc == 2 && !strcmp(argv[1], "roots")) return roots();
    fprintf(stderr, "usage: %s tables | roots\n", argv[0]);
    return 1;
}
