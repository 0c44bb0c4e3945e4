// CPU harness of cufhe_amd/csrc/op_registry.h for tests/test_op_registry.py (plain g++, no HIP):
//   ranges            every id around the four ranges: "name op contains def output"
//   table             the write-once table: find before and after publish, the output bound, a full table, clear; "ok" or the failure
//   texts             every refusal text
//   admit A B         the admission of the cases on stdin, one per line: "entry param_set lvl0_ring level op [op]" -> "code<TAB>text", in
//                     the table state of tools/record_user_op_refusals.py (its definitions made for the sets A and B)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cufhe_amd/csrc/op_registry.h"

using namespace opreg;

static int dump_ranges()
{
    const struct { const char* name; OpRange r; } all[] = {{"user", kUserOps}, {"lvl2", kLvl2UserOps}, {"ps", kPsUserOps}, {"lookup", kLookupOps}};
    for (const auto& x : all)
        for (int op = x.r.base - 2; op < x.r.end() + 2; op++) {
            const bool in = x.r.contains(op);
            printf("%s %d %d %d %d\n", x.name, op, in ? 1 : 0, in ? x.r.def(op) : -1, in ? x.r.output(op) : -1);
        }
    return 0;
}

#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static int check_table()
{
    static OpTable<UserGate, kLvl2UserOps.cap> t{kLvl2UserOps};
    const OpRange r = kLvl2UserOps;
    const UserGate one{{1, 0, 0}, 7u, false, 1, 0}, four{{1, 2, 3}, 9u, true, 4, 2};
    EXPECT(t.next_free() == 0 && !t.find(r.id(0)) && !t.row(0));
    EXPECT(t.publish(0, one) == r.base && t.next_free() == 1);
    EXPECT(t.find(r.id(0)) && t.find(r.id(0))->off == 7u && t.row(0) == t.find(r.id(0)));
    EXPECT(!t.find(r.id(0, 1)) && !t.find(r.id(1)) && !t.find(r.base - 1) && !t.find(r.end()));      // output bound, undefined k, outside
    EXPECT(t.publish(1, four) == r.base + 1);
    for (int j = 0; j < 8; j++) EXPECT((t.find(r.id(1, j)) != nullptr) == (j < 4));
    EXPECT(t.find(r.id(1, 3)) == t.row(1) && t.find(r.id(1, 3))->s == 2);
    for (int k = 2; k < r.cap; k++) EXPECT(t.next_free() == k && t.publish(k, one) == r.base + k);
    EXPECT(t.next_free() == -1 && t.find(r.id(r.cap - 1)) && !t.find(r.id(r.cap - 1, 1)));               // full
    t.clear();
    EXPECT(t.next_free() == 0 && !t.find(r.id(0)) && !t.find(r.id(1, 3)) && !t.row(1));
    EXPECT(t.publish(0, four) == r.base && t.find(r.id(0, 3)) && !t.find(r.id(1)));                      // k = 0 again
    // a set's entry carries its set; a lookup's table has the same rule
    static OpTable<PsUserGate, kPsUserOps.cap> p{kPsUserOps};
    EXPECT(p.publish(p.next_free(), PsUserGate{four, 2}) == kPsUserOps.base && p.find(kPsUserOps.id(0, 3))->set == 2 && !p.find(kPsUserOps.id(0, 4)));
    static OpTable<LookupDef, kLookupOps.cap> l{kLookupOps};
    EXPECT(l.publish(l.next_free(), LookupDef{{1, 0}, 0u, 2, 1}) == kLookupOps.base && l.find(kLookupOps.id(0, 1)) && !l.find(kLookupOps.id(0, 2)));
    // operands of a user gate: one, two and three of them
    struct Lin { const uint32_t *a, *b; uint32_t* out; int32_t ca, cb; uint32_t off, pad; };
    std::vector<Lin> pre;
    uint32_t x[4] = {0, 0, 0, 0};
    auto tmp = [&] { return &x[3]; };
    GateOperands o = user_gate_operands(one, &x[0], &x[1], &x[2], tmp, pre);
    EXPECT(o.a == &x[0] && o.b == &x[0] && o.ca == 1 && o.cb == 0 && pre.empty() && user_gate_arity(one) == 1);
    const UserGate two{{3, -2, 0}, 0u, false, 1, 0};
    o = user_gate_operands(two, &x[0], &x[1], &x[2], tmp, pre);
    EXPECT(o.a == &x[0] && o.b == &x[1] && o.ca == 3 && o.cb == -2 && pre.empty());
    o = user_gate_operands(four, &x[0], &x[1], &x[2], tmp, pre);
    EXPECT(o.a == &x[3] && o.b == &x[2] && o.ca == 1 && o.cb == 3 && pre.size() == 1);
    EXPECT(pre[0].a == &x[0] && pre[0].b == &x[1] && pre[0].out == &x[3] && pre[0].ca == 1 && pre[0].cb == 2 && pre[0].off == 0u && pre[0].pad == 0u);
    EXPECT(!missing_operand(one, false, false) && missing_operand(two, false, true) && !missing_operand(two, true, false));
    EXPECT(missing_operand(four, true, false) && !strcmp(missing_operand(four, false, false), "user gate needs a second operand"));
    // cufhe_amd_enqueue_gate without an output or a first operand: "null ciphertext" comes after the default family's "not defined" and
    // before the other two families' path refusal, whatever the route
    static Registry reg;
    reg.user.publish(0, one);
    const Route wrong = route_of_options(3, 2048, -1), right = route_of_options(-1, 1024, -1);
    for (const Route& route : {wrong, right}) {
        EXPECT(admit(reg, kUserOps.id(1), route, Entry::Recorded, false).refusal == Refusal::UserNotDefined);
        EXPECT(admit(reg, kUserOps.id(0, 1), route, Entry::Recorded, false).refusal == Refusal::UserNotOutput);
        EXPECT(admit(reg, kUserOps.id(0), route, Entry::Recorded, false).refusal == Refusal::NullCiphertext);
        EXPECT(admit(reg, kLvl2UserOps.id(0), route, Entry::Recorded, false).refusal == Refusal::NullCiphertext);
        EXPECT(admit(reg, kPsUserOps.id(0), route, Entry::Recorded, false).refusal == Refusal::NullCiphertext);
        EXPECT(admit(reg, CUFHE_AMD_NAND, route, Entry::Recorded, false).refusal == Refusal::None);      // a built-in op: the caller's check
    }
    EXPECT(admit(reg, kUserOps.id(0), wrong, Entry::Recorded, true).refusal == Refusal::UserPath && admit(reg, kUserOps.id(0), right, Entry::Recorded, true));
    EXPECT(admit(reg, kLvl2UserOps.id(0), right, Entry::Recorded, true).refusal == Refusal::Lvl2Path);
    EXPECT(admit(reg, kPsUserOps.id(0), right, Entry::Recorded, true).refusal == Refusal::PsPath);
    // a list keeps admissions only when it has a user gate's id
    std::vector<Admission> adm;
    const int plain[2] = {CUFHE_AMD_NAND, CUFHE_AMD_MUX}, mixed[2] = {CUFHE_AMD_NAND, kUserOps.id(0)};
    EXPECT(admit_list(reg, 2, [&](size_t g) { return plain[g]; }, right, Entry::Direct, &adm) == Refusal::None && adm.empty());
    EXPECT(admit_list(reg, 2, [&](size_t g) { return mixed[g]; }, right, Entry::Direct, &adm) == Refusal::None && adm.size() == 2);
    EXPECT(!adm[0].gate && adm[1].gate == reg.user.row(0) && adm[1].k == 0 && adm[1].j == 0);
    printf("ok\n");
    return 0;
}

static Registry g_reg;

static int answer(Refusal r)
{
    printf("%d\t%s\n", r == Refusal::None ? 0 : -1, refusal_text(r));
    return 0;
}

static int admit_cases(int set_a, int set_b)
{
    // tools/record_user_op_refusals.py: row 0 a single-output gate of two operands, row 1 a two-output one; the sets' row 2 is set B's
    const UserGate single{{-1, -1, 0}, 1u << 29, false, 1, 0}, pair{{1, 1, 0}, 0u, true, 2, 1};
    g_reg.user.publish(0, single); g_reg.user.publish(1, pair);
    g_reg.lvl2.publish(0, single); g_reg.lvl2.publish(1, pair);
    g_reg.ps.publish(0, {single, set_a}); g_reg.ps.publish(1, {pair, set_a}); g_reg.ps.publish(2, {single, set_b});
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char entry[64];
        long param_set, ring;
        int level, ops[2] = {0, 0};
        const int n = sscanf(line, "%63s %ld %ld %d %d %d", entry, &param_set, &ring, &level, &ops[0], &ops[1]) - 4;
        if (n < 1) { fprintf(stderr, "bad case: %s", line); return 2; }
        const bool active = param_set >= 0;
        const std::string e = entry;
        auto op_of = [&](size_t g) { return ops[g]; };
        const Route ring_route{Path::Ring, -1, 0, active}, set_route{Path::Set, set_a, level, active};
        Refusal r = Refusal::None;
        if (e == "gate_list") {
            const Route route = route_of_options(param_set, ring, level);
            r = admit_list(g_reg, (size_t)n, op_of, route, Entry::List, nullptr);
            if (r == Refusal::None) {      // then the path's lowering asks again
                const Route lowered = route.path == Path::Ring ? ring_route : Route{route.path, route.path == Path::Set ? (int)param_set : -1, level, active};
                r = admit_list(g_reg, (size_t)n, op_of, lowered, Entry::Direct, nullptr);
            }
        } else if (e == "ring_batch") {
            r = admit_list(g_reg, (size_t)n, op_of, ring_route, Entry::Direct, nullptr);
        } else if (e == "set_batch") {
            r = admit_list(g_reg, (size_t)n, op_of, set_route, Entry::Direct, nullptr);
        } else if (e == "enqueue_gate" || e == "enqueue_gate.in1_null") {
            r = admit(g_reg, ops[0], route_of_options(param_set, ring, level), Entry::Recorded, true).refusal;
        } else if (e == "enqueue_gate_multi") {
            r = admit(g_reg, ops[0], Route{}, Entry::RecordedMulti).refusal;
        } else if (e == "lvl2_hook") {
            r = admit(g_reg, ops[0], ring_route, Entry::Lvl2Hook).refusal;
        } else if (e == "ps_hook") {
            r = admit(g_reg, ops[0], Route{Path::Set, set_a, 0, active}, Entry::PsHook).refusal;
        } else {
            fprintf(stderr, "unknown entry %s\n", entry);
            return 2;
        }
        answer(r);
    }
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ranges") return dump_ranges();
    if (mode == "table") return check_table();
    if (mode == "texts") {
        for (int r = 1; r <= (int)Refusal::NotPsRange; r++) printf("%s\n", refusal_text((Refusal)r));
        return 0;
    }
    if (mode == "admit" && argc == 4) return admit_cases(atoi(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: op_registry_harness ranges | table | texts | admit A B\n");
    return 2;
}
