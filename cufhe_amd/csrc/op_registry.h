// op_registry.h -- the op ids a caller defines (cufhe_amd_define_gate, cufhe_amd_lvl2_define_gate, cufhe_amd_ps_define_gate,
// cufhe_amd_define_lookup): their id ranges, their definition tables, and the one rule that says where such an id may run and what a
// refusal says.  Host only: no HIP header, plain C++17; capi.hip and tests/host/op_registry_harness.cpp both include it.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/cufhe_amd.h"

namespace opreg {

// ---- id ranges ----
// Definition k of a family is op base + k; output j of a multi-output definition is base + k + j * cap (CUFHE_AMD_*_OP_OUTPUT), j < 8.
constexpr int kOutputShift = 3;          // at most 8 outputs (kMaxOutputShift of the kernels)
constexpr int kRingN = 1024;             // N of the default path: the SEIKS_AT / CMUX_ROTATE ids carry an index / an exponent below N / 2N
struct OpRange {
    int base, cap;
    constexpr int end() const { return base + (cap << kOutputShift); }
    constexpr bool contains(int op) const { return op >= base && op < end(); }
    constexpr int def(int op) const { return (op - base) % cap; }        // definition index k
    constexpr int output(int op) const { return (op - base) / cap; }     // output j
    constexpr int id(int k, int j = 0) const { return base + k + j * cap; }
};
constexpr OpRange kUserOps{CUFHE_AMD_USER_OP_BASE, CUFHE_AMD_MAX_USER_GATES};
constexpr OpRange kLvl2UserOps{CUFHE_AMD_LVL2_USER_OP_BASE, CUFHE_AMD_LVL2_MAX_USER_GATES};
constexpr OpRange kPsUserOps{CUFHE_AMD_PS_USER_OP_BASE, CUFHE_AMD_PS_MAX_USER_GATES};
constexpr OpRange kLookupOps{CUFHE_AMD_LOOKUP_OP_BASE, CUFHE_AMD_MAX_LOOKUPS};
constexpr int kSpreadOpEnd = CUFHE_AMD_TL_SPREAD(10, 0) + 1;          // a + b <= 10: the largest id is (10, 0)
constexpr int kLutRotateOpEnd = CUFHE_AMD_TL_LUT_ROTATE(kOutputShift) + 1;

constexpr bool id_ranges_apart(int a0, int a1, int b0, int b1) { return a1 <= b0 || b1 <= a0; }      // [a0, a1) and [b0, b1)
// [lo, hi) against the built-in ops, the TRLWE-level ops, the packed ROM words and the three user-gate ranges
constexpr bool apart_from_existing(int lo, int hi)
{
    return id_ranges_apart(lo, hi, 0, CUFHE_AMD_NUM_OPS) && id_ranges_apart(lo, hi, CUFHE_AMD_TL_BOOTSTRAP, CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP + 1) &&
           id_ranges_apart(lo, hi, kUserOps.base, kUserOps.end() + 1) &&
           id_ranges_apart(lo, hi, CUFHE_AMD_TL_SEIKS_AT(0), CUFHE_AMD_TL_SEIKS_AT(kRingN - 1) + 1) &&
           id_ranges_apart(lo, hi, CUFHE_AMD_TL_CMUX_ROTATE(0), CUFHE_AMD_TL_CMUX_ROTATE(2 * kRingN - 1) + 1) &&
           id_ranges_apart(lo, hi, kLvl2UserOps.base, kLvl2UserOps.end()) && id_ranges_apart(lo, hi, kPsUserOps.base, kPsUserOps.end());
}
static_assert(CUFHE_AMD_USER_OP_OUTPUT(kUserOps.id(kUserOps.cap - 1), (1 << kOutputShift) - 1) == kUserOps.end() - 1 &&
                  CUFHE_AMD_LVL2_USER_OP_OUTPUT(kLvl2UserOps.id(kLvl2UserOps.cap - 1), (1 << kOutputShift) - 1) == kLvl2UserOps.end() - 1 &&
                  CUFHE_AMD_PS_USER_OP_OUTPUT(kPsUserOps.id(kPsUserOps.cap - 1), (1 << kOutputShift) - 1) == kPsUserOps.end() - 1 &&
                  CUFHE_AMD_LOOKUP_OP_OUTPUT(kLookupOps.id(kLookupOps.cap - 1), (1 << kOutputShift) - 1) == kLookupOps.end() - 1,
              "the output ids of each family fill [base, base + 8 * 64)");
static_assert(kUserOps.base > CUFHE_AMD_TL_CMUX, "user op ids do not overlap the built-in or TRLWE-level ops");
// packed ROM words: op ids that carry an index / an exponent (include/cufhe_amd.h)
static_assert(CUFHE_AMD_TL_SEIKS_AT(0) >= kUserOps.end() && CUFHE_AMD_TL_SEIKS_AT(0) > CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP &&
                  CUFHE_AMD_TL_SEIKS_AT(0) >= CUFHE_AMD_NUM_OPS, "SEIKS_AT ids lie above the built-in, TRLWE-level and user ops");
static_assert(CUFHE_AMD_TL_CMUX_ROTATE(0) > CUFHE_AMD_TL_SEIKS_AT(kRingN - 1), "CMUX_ROTATE ids lie above the SEIKS_AT ids");
static_assert(kLvl2UserOps.base > CUFHE_AMD_TL_CMUX_ROTATE(2 * kRingN - 1) && kLvl2UserOps.base > CUFHE_AMD_TL_SEIKS_AT(kRingN - 1) &&
                  kLvl2UserOps.base > CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP && kLvl2UserOps.base >= CUFHE_AMD_NUM_OPS,
              "lvl2 user op ids lie above the built-in ops and the packed ROM words");
static_assert(kPsUserOps.base > CUFHE_AMD_TL_CMUX_ROTATE(2 * kRingN - 1) && kPsUserOps.base > CUFHE_AMD_TL_SEIKS_AT(kRingN - 1) &&
                  kPsUserOps.base > CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP, "parameter-set user op ids lie above the built-in ops and the packed ROM words");
// each pair of the four ranges, once (the lookups' against the three others: apart_from_existing below)
static_assert(kLvl2UserOps.base >= kUserOps.end(), "lvl2 user op ids lie above the user op ids");
static_assert(kPsUserOps.base >= kUserOps.end(), "parameter-set user op ids lie above the user op ids");
static_assert(kPsUserOps.base >= kLvl2UserOps.end(), "parameter-set user op ids lie above the lvl2 user op ids");
// the recorded lookups, Spreads, table rotations and packs against everything else
static_assert(apart_from_existing(kLookupOps.base, kLookupOps.end()), "lookup ids overlap no other op id");
static_assert(apart_from_existing(CUFHE_AMD_TL_SPREAD_BASE, kSpreadOpEnd), "recorded Spread ids overlap no other op id");
static_assert(apart_from_existing(CUFHE_AMD_TL_LUT_ROTATE_BASE, kLutRotateOpEnd), "recorded table-rotation ids overlap no other op id");
static_assert(id_ranges_apart(CUFHE_AMD_TL_SPREAD_BASE, kSpreadOpEnd, CUFHE_AMD_TL_LUT_ROTATE_BASE, kLutRotateOpEnd) &&
                  id_ranges_apart(CUFHE_AMD_TL_SPREAD_BASE, kSpreadOpEnd, kLookupOps.base, kLookupOps.end()) &&
                  id_ranges_apart(CUFHE_AMD_TL_LUT_ROTATE_BASE, kLutRotateOpEnd, kLookupOps.base, kLookupOps.end()),
              "the three recorded ranges do not overlap one another");
static_assert(apart_from_existing(CUFHE_AMD_TL_PACK, CUFHE_AMD_TL_PACK + 1) &&
                  id_ranges_apart(CUFHE_AMD_TL_PACK, CUFHE_AMD_TL_PACK + 1, CUFHE_AMD_TL_SPREAD_BASE, kSpreadOpEnd) &&
                  id_ranges_apart(CUFHE_AMD_TL_PACK, CUFHE_AMD_TL_PACK + 1, CUFHE_AMD_TL_LUT_ROTATE_BASE, kLutRotateOpEnd) &&
                  id_ranges_apart(CUFHE_AMD_TL_PACK, CUFHE_AMD_TL_PACK + 1, kLookupOps.base, kLookupOps.end()),
              "the recorded pack's id (pack.inc.h) overlaps no other op id");

// ---- definitions ----
// A user gate x = c0 in0 + c1 in1 + c2 in2 + (0, ..., 0, off) bootstrapped through a test vector (tv: row k of the path's device table;
// else the constant mu) with nout = 2^s outputs; the rotations of a multi-output definition (s > 0) carry s beside the row.
struct UserGate { int32_t c[3]; uint32_t off; bool tv; int nout; int s; };
struct PsUserGate : UserGate { int set; };       // a set's definition is made for ONE compiled parameter set
struct LookupDef { int32_t c[2]; uint32_t off; int nout; int s; };      // a recorded lookup: x = c0 in0 + c1 in1 + (0, .., 0, off), nout = 2^s outputs
// operands a user gate reads: in0 (c1 = c2 = 0), in0 and in1 (c2 = 0), all three
inline int user_gate_arity(const UserGate& u) { return u.c[2] ? 3 : u.c[1] ? 2 : 1; }

// The definitions of one family.  A definition is written once, before the count is raised past it (release), and never changes
// afterwards, so the gate paths read it without a lock (acquire); clear() (CleanUp) drops them all and the next one is k = 0 again.
template <class Def, int Cap>
struct OpTable {
    OpRange range;
    explicit constexpr OpTable(OpRange r) : range(r.cap == Cap ? r : throw "the range's capacity is the table's") {}
    const Def* row(int k) const { return k < count_.load(std::memory_order_acquire) ? &defs_[k] : nullptr; }      // nullptr: not defined
    // the definition of `op`; nullptr when op is outside the range, names an undefined k, or names an output j >= nout
    const Def* find(int op) const
    {
        const Def* d = range.contains(op) ? row(range.def(op)) : nullptr;
        return d && range.output(op) < d->nout ? d : nullptr;
    }
    int next_free() const { return count_.load(std::memory_order_relaxed) < range.cap ? count_.load(std::memory_order_relaxed) : -1; }      // -1: full
    int publish(int k, const Def& d)     // k = next_free(); the op id of the new definition
    {
        defs_[k] = d;
        count_.store(k + 1, std::memory_order_release);
        return range.id(k);
    }
    void clear() { count_.store(0, std::memory_order_release); }

   private:
    Def defs_[Cap];
    std::atomic<int> count_{0};
};

struct Registry {
    OpTable<UserGate, kUserOps.cap> user{kUserOps};
    OpTable<UserGate, kLvl2UserOps.cap> lvl2{kLvl2UserOps};
    OpTable<PsUserGate, kPsUserOps.cap> ps{kPsUserOps};
    OpTable<LookupDef, kLookupOps.cap> lookup{kLookupOps};
};

// ---- admission ----
// Where the gates of a call run: the hand-scheduled default path, the N = 2048 ring (level 0 only), or compiled parameter set `set`;
// level: of the gates' ciphertexts, -1 when there is none to ask; set_active: "param_set" is active, whichever path this call takes
enum class Path { Default, Ring, Set };
struct Route { Path path; int set; int level; bool set_active; };
// the route the library's options give the gates of `level` ("lvl0_ring" wins at level 0)
constexpr Route route_of_options(long param_set, long lvl0_ring, int level)
{
    return {level == 0 && lvl0_ring == 2048 ? Path::Ring : param_set >= 0 ? Path::Set : Path::Default, (int)param_set, level, param_set >= 0};
}
// How the id reached the library: List = a gate list through run_gates (cufhe_amd_gate, _gate_batch, _gate_list, a recorded level);
// Direct = lower_gates (the ring's or a set's own batch entry, and every list after run_gates let it through); Recorded(Multi) =
// cufhe_amd_enqueue_gate(_multi); the parity hooks cufhe_amd_lvl2_user_rotate_batch / _extract_batch and cufhe_amd_ps_user_rotate
enum class Entry { List, Direct, Recorded, RecordedMulti, Lvl2Hook, PsHook };
enum class Family : int8_t { None = -1, User, Lvl2, Ps };      // None: not a user gate's id (a built-in op, or unknown: the caller's business)
constexpr int kFamilies = 3, kEntries = 6;
constexpr Family family_of(int op)
{
    return kUserOps.contains(op) ? Family::User : kLvl2UserOps.contains(op) ? Family::Lvl2 : kPsUserOps.contains(op) ? Family::Ps : Family::None;
}

enum class Refusal : uint8_t {
    None, UserNotDefined, UserNotOutput, UserPath, Lvl2NotDefined, Lvl2NotOutput, Lvl2Path, PsNotDefined, PsOtherSet, PsNotOutput, PsPath,
    NullCiphertext, MultiLvl2, MultiPs, NotLvl2Range, NotPsRange,
};
// the text of a refusal (every one is returned with code -1), in the order of the enum; callers and tests match on these
constexpr const char* kRefusalText[] = {
    "",
    "user gate op not defined (cufhe_amd_define_gate; CleanUp drops the definitions)",
    "unknown gate op: not an output of a defined multi-output user gate (CUFHE_AMD_USER_OP_OUTPUT(op, j), j < nout)",
    "user gates run on the default path only: not with \"param_set\" active or on the N = 2048 ring (\"lvl0_ring\")",
    "lvl2 user gate op not defined (cufhe_amd_lvl2_define_gate; CleanUp drops the definitions)",
    "unknown gate op: not an output of a defined multi-output user gate (CUFHE_AMD_LVL2_USER_OP_OUTPUT(op, j), j < nout)",
    "lvl2 user gates run on the N = 2048 ring only: lvl0 ciphertexts through cufhe_amd_lvl2_gate_batch or with \"lvl0_ring\" 2048, "
    "not with \"param_set\" active",
    "parameter set user gate op not defined (cufhe_amd_ps_define_gate; CleanUp drops the definitions)",
    "user gate op was defined for another parameter set (cufhe_amd_ps_define_gate(set, ...))",
    "unknown gate op: not an output of a defined multi-output user gate of this parameter set (CUFHE_AMD_PS_USER_OP_OUTPUT(op, j), j < nout)",
    "user gates of a parameter set run on that set only: through cufhe_amd_ps_gate_batch or with \"param_set\" active, "
    "not on the default path or on the N = 2048 ring",
    "null ciphertext",
    "enqueue_gate_multi: lvl2 user gates have one output (cufhe_amd_enqueue_gate)",
    "enqueue_gate_multi: the outputs of a parameter set's user gate are recorded one by one (cufhe_amd_enqueue_gate with "
    "CUFHE_AMD_PS_USER_OP_OUTPUT(op, j)); siblings on the same operands in one flush share the rotation",
    "op is not in the lvl2 user gates' id range (CUFHE_AMD_LVL2_USER_OP_BASE + k)",
    "op is not in the parameter sets' user gate id range (CUFHE_AMD_PS_USER_OP_BASE + k)",
};
static_assert(sizeof(kRefusalText) / sizeof(kRefusalText[0]) == (size_t)Refusal::NotPsRange + 1, "one text per refusal");
constexpr const char* refusal_text(Refusal r) { return kRefusalText[(int)r]; }

// What an entry asks about an id of a family, in the order it asks.  The entries grew one by one and differ in that order; the
// differences are kept as they are, here, as data:
//   Defined    the id names a definition of the family (for a set: of the route's set) and an output it has
//   Routed     the route runs the family: User on Path::Default; Lvl2 on Path::Ring at level 0 without an active set; Ps on Path::Set
//   Operands   the call's output and first operand are there ("null ciphertext")
//   Refused    the entry takes no id of this family: `foreign` says why
enum class Check : uint8_t { End, Defined, Routed, Operands, Refused };
struct Rule { Check checks[3]; Refusal foreign; };
constexpr Rule kRules[kEntries][kFamilies] = {
    // List: the default family asks "defined?" first, the two later ones "right path?" first
    {{{Check::Defined, Check::Routed}, {}}, {{Check::Routed, Check::Defined}, {}}, {{Check::Routed, Check::Defined}, {}}},
    // Direct: "right path?" first for all three, so an undefined default-family id says "default path only" on the ring or a set
    {{{Check::Routed, Check::Defined}, {}}, {{Check::Routed, Check::Defined}, {}}, {{Check::Routed, Check::Defined}, {}}},
    // Recorded: "null ciphertext" comes after the default family's "not defined", before the other two families' path refusal
    {{{Check::Defined, Check::Operands, Check::Routed}, {}},
     {{Check::Operands, Check::Routed, Check::Defined}, {}},
     {{Check::Operands, Check::Routed, Check::Defined}, {}}},
    // RecordedMulti: the default family only, and its route is asked after the caller's own checks (routed())
    {{{Check::Defined}, {}}, {{Check::Refused}, Refusal::MultiLvl2}, {{Check::Refused}, Refusal::MultiPs}},
    // the parity hooks: their own family only (ids of no family included)
    {{{Check::Refused}, Refusal::NotLvl2Range}, {{Check::Routed, Check::Defined}, {}}, {{Check::Refused}, Refusal::NotLvl2Range}},
    {{{Check::Refused}, Refusal::NotPsRange}, {{Check::Refused}, Refusal::NotPsRange}, {{Check::Routed, Check::Defined}, {}}},
};
// the order in which a list's families are reported when several have a bad id (within a family: the first in list order)
constexpr Family kListOrder[2][kFamilies] = {{Family::User, Family::Lvl2, Family::Ps}, {Family::User, Family::Ps, Family::Lvl2}};      // [entry == Direct]

// whether `route` runs the gates of `family`; else the refusal
constexpr Refusal routed(Family family, const Route& route)
{
    switch (family) {
        case Family::User: return route.path == Path::Default ? Refusal::None : Refusal::UserPath;
        case Family::Lvl2: return route.path == Path::Ring && !route.set_active && route.level == 0 ? Refusal::None : Refusal::Lvl2Path;
        case Family::Ps: return route.path == Path::Set ? Refusal::None : Refusal::PsPath;
        case Family::None: break;
    }
    return Refusal::None;
}

struct Admission {
    const UserGate* gate = nullptr;    // the definition, when the entry asked for it and did not refuse
    Refusal refusal = Refusal::None;
    Family family = Family::None;      // None with no refusal: not a user gate's id -- a built-in op, or one the caller does not know
    uint8_t k = 0, j = 0;              // its row in the family's table and the output the id names
    explicit operator bool() const { return refusal == Refusal::None; }
};

// May `op` run on `route`, coming in through `entry`?  operands: whether the call's output and first operand are non-null (Recorded).
inline Admission admit(const Registry& reg, int op, const Route& route, Entry entry, bool operands = true)
{
    Admission a;
    a.family = family_of(op);
    if (a.family == Family::None) {      // the hooks refuse an id of no family like one of another family
        a.refusal = entry == Entry::Lvl2Hook ? Refusal::NotLvl2Range : entry == Entry::PsHook ? Refusal::NotPsRange : Refusal::None;
        return a;
    }
    const OpRange range = a.family == Family::User ? kUserOps : a.family == Family::Lvl2 ? kLvl2UserOps : kPsUserOps;
    a.k = (uint8_t)range.def(op), a.j = (uint8_t)range.output(op);
    const Rule& rule = kRules[(int)entry][(int)a.family];
    for (Check c : rule.checks) {
        switch (c) {
            case Check::End: return a;
            case Check::Refused: a.refusal = rule.foreign; return a;
            case Check::Operands: if (!operands) a.refusal = Refusal::NullCiphertext; break;
            case Check::Routed: a.refusal = routed(a.family, route); break;
            case Check::Defined:
                if (a.family == Family::Ps) {
                    // "not defined" comes before "another set's", which comes before "not an output"
                    const PsUserGate* d = reg.ps.row(a.k);
                    a.refusal = !d ? Refusal::PsNotDefined : d->set != route.set ? Refusal::PsOtherSet : a.j >= d->nout ? Refusal::PsNotOutput : Refusal::None;
                    if (a.refusal == Refusal::None) a.gate = d;
                } else {
                    // an id that names no definition: "not defined" under output 0's id, "not an output" under any other
                    const bool user = a.family == Family::User;
                    a.gate = (user ? reg.user : reg.lvl2).find(op);
                    if (!a.gate) a.refusal = a.j == 0 ? (user ? Refusal::UserNotDefined : Refusal::Lvl2NotDefined) : (user ? Refusal::UserNotOutput : Refusal::Lvl2NotOutput);
                }
                break;
        }
        if (a.refusal != Refusal::None) return a;
    }
    return a;
}

// The admission of a whole list: the refusal the entry reports -- of the first family in the entry's order that has a refused gate, the
// first such gate in list order -- and (*adm)[g] for every gate; adm stays empty for a list without a user gate's id, and may be null.
template <class GetOp>
Refusal admit_list(const Registry& reg, size_t count, GetOp op_of, const Route& route, Entry entry, std::vector<Admission>* adm)
{
    Refusal first[kFamilies] = {Refusal::None, Refusal::None, Refusal::None};
    for (size_t g = 0; g < count; g++) {
        const Admission a = admit(reg, op_of(g), route, entry);
        if (adm && a.family != Family::None && adm->empty()) adm->resize(count);
        if (adm && a.family != Family::None) (*adm)[g] = a;
        if (!a && first[(int)a.family] == Refusal::None) first[(int)a.family] = a.refusal;
    }
    for (Family f : kListOrder[entry == Entry::Direct])
        if (first[(int)f] != Refusal::None) return first[(int)f];
    return Refusal::None;
}

// ---- operands of a user gate ----
// the refusal of a user gate whose second / third operand is needed and missing; nullptr: all there
inline const char* missing_operand(const UserGate& u, bool have_in1, bool have_in2)
{
    const int arity = user_gate_arity(u);
    return arity >= 2 && !have_in1 ? "user gate needs a second operand" : arity == 3 && !have_in2 ? "user gate needs a third operand" : nullptr;
}
// A user gate enters the two-input gate path as ca a + cb b (+ off).  One operand: c0 in0 + 0 in0; two: c0 in0 + c1 in1; three: one more
// descriptor of `pre` (a lincomb that runs first) adds c0 in0 + c1 in1 into the temporary t = tmp(), and the gate is 1 t + c2 in2.
struct GateOperands { const uint32_t *a, *b; int32_t ca, cb; };
template <class Tmp, class Pre>
GateOperands user_gate_operands(const UserGate& u, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, Tmp tmp, Pre& pre)
{
    const int arity = user_gate_arity(u);
    if (arity < 3) return {in0, arity == 2 ? in1 : in0, u.c[0], u.c[1]};
    uint32_t* t = tmp();
    pre.push_back(typename Pre::value_type{in0, in1, t, u.c[0], u.c[1], 0u, 0u});
    return {t, in2, 1, u.c[2]};
}

}  // namespace opreg
