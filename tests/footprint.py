"""Memory footprint of the batched entry points: helpers of tests/test_footprint.py and tests/test_gpu_footprint.py.

Every other GPU test asks whether the words a call was meant to write are the reference's.  This module asks the other half: did the
call write anything else?  `Arena` lays all device operands of ONE call out inside ONE allocation, each between guards that carry a
position-dependent pattern; after the call the whole allocation is downloaded once and `Arena.check` lists every word that changed
outside the rows the call was documented to write -- a row past the end, a row before the start, a pad word of a strided operand, a
word of an input.  `CASES` is the table of entry points the GPU module runs through it (tests/test_footprint.py: every `_batch`
declaration of include/cufhe_amd.h is a key).

Host only: nothing here needs a GPU or the library; the GPU module passes a device allocator, the CPU tests a numpy one.
"""
import os
import re

import numpy as np

import positions as pos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cufhe_amd", "csrc")
ALIGN = 256                         # bytes: what hipMalloc gives every existing caller, and all the header's callers pass
ALIGN_WORDS = ALIGN // 4
GUARD = 0x6A09E667                  # guard word i holds GUARD ^ hash(i): a guard word copied onto another one is still a change
ROLES = ("in", "out", "inout")


def guard_pattern(words, first=0):
    """the guard words of arena positions [first, first + words): distinct in neighbouring positions and across rows of any size"""
    i = np.arange(first, first + words, dtype=np.uint64)
    h = (i + np.uint64(1)) * np.uint64(0x9E3779B1)
    h ^= h >> np.uint64(15)
    h *= np.uint64(0x85EBCA77)
    h ^= h >> np.uint64(13)
    return (np.uint64(GUARD) ^ h).astype(np.uint32)


def _round_up(x, m):
    return (x + m - 1) // m * m


class Operand:
    """One device array of a call: `rows` rows of `row_elems` elements of `dtype`, row g at g * stride elements (stride >= row_elems;
    the elements between two rows are pad words).  role: "in" (must not change), "out" (pre-filled with the poison; its rows may
    change), "inout" (holds input words; its rows may change)."""

    def __init__(self, name, dtype, rows, row_elems, role, stride=None):
        assert role in ROLES, role
        self.name, self.dtype, self.rows, self.row_elems, self.role = name, np.dtype(dtype), int(rows), int(row_elems), role
        self.stride = int(row_elems if stride is None else stride)
        assert self.dtype.itemsize % 4 == 0 and self.stride >= self.row_elems > 0 and self.rows >= 0
        self.wpe = self.dtype.itemsize // 4          # arena words (uint32) per element
        self.written_rows = None                     # out / inout: the rows the call may write (None: all of them)
        self.start = self.end = None                 # arena words [start, end) of the rows and their pads; set by Arena

    @property
    def row_words(self):
        return self.stride * self.wpe

    def word_mask(self):
        """[rows * stride * wpe] bool: True on operand words, False on pad words"""
        m = np.zeros((self.rows, self.stride), bool)
        m[:, :self.row_elems] = True
        return np.repeat(m.reshape(-1), self.wpe)


class View:
    """what every function of cufhe_amd/api.py takes for a device array"""

    def __init__(self, ptr, words):
        self.ptr, self.words = ptr, words


class NumpyBackend:
    """alloc / upload / download over a numpy array: the CPU tests' device"""

    def alloc(self, words):
        raw = np.zeros(words + ALIGN_WORDS, np.uint32)
        skip = (-raw.ctypes.data % ALIGN) // 4
        self.mem = raw[skip:skip + words]
        return self.mem.ctypes.data

    def upload(self, host):
        self.mem[:] = host

    def download(self):
        return self.mem.copy()


class Arena:
    """All operands of one call in one allocation.

    Layout, in this order for every operand: a front guard of at least one of its rows and at least 256 bytes, the operand on a
    256-byte boundary, a back guard of at least two of its rows that ends on the next 256-byte boundary.  Inputs get the same guards
    as outputs: a launch of one row too many (the harness's self-test) then reads and writes inside the allocation.
    backend: an object with alloc(words) -> base pointer (256-byte aligned), upload(host uint32 array), download() -> uint32 array.
    """

    def __init__(self, label, operands, backend=None):
        self.label = label
        self.operands = list(operands)
        assert len({o.name for o in self.operands}) == len(self.operands)
        cursor = 0
        for o in self.operands:
            front = _round_up(max(o.row_words, ALIGN_WORDS), ALIGN_WORDS)
            o.start = cursor + front
            o.end = o.start + o.rows * o.row_words
            cursor = _round_up(o.end + 2 * o.row_words, ALIGN_WORDS)
            o.front_guard, o.back_guard = front, cursor - o.end
        self.words = cursor
        # kind of every arena word: 0 guard, 1 operand word, 2 pad word; owner: index of the operand for kinds 1 and 2
        self.kind = np.zeros(self.words, np.uint8)
        self.owner = np.full(self.words, -1, np.int32)
        self.host = guard_pattern(self.words)
        for k, o in enumerate(self.operands):
            m = o.word_mask()
            self.kind[o.start:o.end] = np.where(m, 1, 2)
            self.owner[o.start:o.end] = k
            if o.role == "out":
                seg = self.host[o.start:o.end]
                seg[m] = pos.POISON
        self.backend = backend or NumpyBackend()
        self.base = self.backend.alloc(self.words)
        assert self.base % ALIGN == 0, "the allocator returned a pointer of less than 256-byte alignment"
        self.before = None

    def __getitem__(self, name):
        for o in self.operands:
            if o.name == name:
                return o
        raise KeyError(name)

    def view(self, name):
        o = self[name]
        return View(self.base + 4 * o.start, o.end - o.start)

    def ptr(self, name, row=0):
        o = self[name]
        return self.base + 4 * (o.start + row * o.row_words)

    def set(self, name, rows):
        """the words of an "in" / "inout" operand: rows is [rows][row_elems] of its dtype"""
        o = self[name]
        a = np.ascontiguousarray(rows).reshape(o.rows, o.row_elems)
        assert a.dtype == o.dtype, f"{name}: {a.dtype} given, {o.dtype} declared"
        seg = self.host[o.start:o.end].reshape(o.rows, o.row_words)
        seg[:, :o.row_elems * o.wpe] = a.view(np.uint32).reshape(o.rows, o.row_elems * o.wpe)

    def written(self, name, rows):
        """restrict the rows of an out / inout operand the call may write (scattered operands of cufhe_amd_gate_list)"""
        self[name].written_rows = np.asarray(rows, np.int64)

    def upload(self):
        self.before = self.host.copy()
        self.backend.upload(self.host)

    def download(self):
        after = np.asarray(self.backend.download(), np.uint32)
        assert after.shape == (self.words,)
        return after

    def rows(self, after, name):
        """[rows][row_elems] of the operand's dtype out of a downloaded arena"""
        o = self[name]
        seg = after[o.start:o.end].reshape(o.rows, o.row_words)[:, :o.row_elems * o.wpe]
        return np.ascontiguousarray(seg).view(o.dtype).reshape(o.rows, o.row_elems)

    def allowed(self):
        """bool per arena word: the call may change it"""
        ok = np.zeros(self.words, bool)
        for o in self.operands:
            if o.role == "in":
                continue
            m = o.word_mask().reshape(o.rows, o.row_words)
            if o.written_rows is not None:
                keep = np.zeros(o.rows, bool)
                keep[o.written_rows] = True
                m = m & keep[:, None]
            ok[o.start:o.end] = m.reshape(-1)
        return ok

    def findings(self, after):
        """every run of changed words outside the rows the call may write, as dicts:
        operand: the nearest operand; side: "before" / "after" (guard words), "pad", "input" (an "in" word) or "row" (a row of an
        out / inout operand the call must not write); distance: elements of that operand from its first word ("before": negative)
        or from the end of its last row ("after": 0 = directly behind it), inside the operand: from its first word; rows: the same
        in rows of the operand; words: changed elements in the run; old / new: the first element before and after."""
        assert self.before is not None, "upload() first"
        after = np.asarray(after, np.uint32)
        bad = np.flatnonzero((after != self.before) & ~self.allowed())
        out = []
        if bad.size == 0:
            return out
        cuts = np.flatnonzero(np.diff(bad) != 1) + 1
        for run in np.split(bad, cuts):
            # a run never spans two kinds of place: split where the kind or the owner changes
            key = self.kind[run].astype(np.int64) * 65536 + self.owner[run]
            for part in np.split(run, np.flatnonzero(np.diff(key) != 0) + 1):
                out.append(self._describe(part, after))
        return out

    def _describe(self, run, after):
        first = int(run[0])
        k = int(self.owner[first])
        if k >= 0:
            o = self.operands[k]
            side = "pad" if self.kind[first] == 2 else "input" if o.role == "in" else "row"
            dist = first - o.start
        else:
            # nearest operand by distance to its extent
            best = None
            for o2 in self.operands:
                d = o2.start - first if first < o2.start else first - o2.end + 1
                if best is None or d < best[0]:
                    best = (d, o2)
            o = best[1]
            side = "before" if first < o.start else "after"
            dist = first - o.start if side == "before" else first - o.end
        elems = -((-dist) // o.wpe) if dist < 0 else dist // o.wpe
        e0 = first - (first - o.start) % o.wpe        # the element the first changed word belongs to
        old = self.before[e0:e0 + o.wpe].copy().view(o.dtype if o.dtype.kind != "f" else np.uint64)[0]
        new = after[e0:e0 + o.wpe].copy().view(o.dtype if o.dtype.kind != "f" else np.uint64)[0]
        return dict(operand=o.name, side=side, distance=int(elems), rows=elems / o.stride,
                    words=int(-(-run.size // o.wpe)), first_word=first, old=int(old) & (2 ** (32 * o.wpe) - 1),
                    new=int(new) & (2 ** (32 * o.wpe) - 1), count_rows=o.rows)

    def check(self, after):
        """None, or the message that lists every changed word outside the out / inout rows"""
        found = self.findings(after)
        if not found:
            return None
        lines = [f"{self.label}: {sum(f['words'] for f in found)} words changed outside the documented outputs, in {len(found)} runs"]
        for f in found[:40]:
            o = self[f["operand"]]
            if f["side"] == "after":
                where = f"starting {f['distance']} words after the last row"
                if f["distance"] % o.stride == 0:
                    where += f" (= row `count` + {f['distance'] // o.stride})" if f["distance"] else " (= row `count`)"
                else:
                    where += f" ({f['rows']:.3f} rows)"
            elif f["side"] == "before":
                where = f"starting {-f['distance']} words before the first row ({f['rows']:.3f} rows)"
            else:
                what = {"pad": "pad words", "input": "words of this input", "row": "words of a row the call must not write"}[f["side"]]
                where = f"{what}, row {f['distance'] // o.stride} word {f['distance'] % o.stride}"
            lines.append(f"  {self.label}, {f['operand']}: {f['words']} words changed {where}; first {f['old']:#x} -> {f['new']:#x}")
        if len(found) > 40:
            lines.append(f"  ... and {len(found) - 40} more runs")
        return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# the unit U of a launch shape: items one workgroup / tile takes, read from the named constant it comes from
# ---------------------------------------------------------------------------------------------------------------------------------
_constants = {}


def csrc_constant(name, files=None):
    """the value of `constexpr int <name> = <integer>;` in cufhe_amd/csrc (the library's own number, not a copy of it)"""
    if name not in _constants:
        found = []
        for f in sorted(os.listdir(CSRC)):
            if files and f not in files:
                continue
            text = open(os.path.join(CSRC, f)).read()
            found += re.findall(r"constexpr\s+(?:int|unsigned|size_t|long)\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text)
        assert len(set(found)) == 1, f"{name}: {len(found)} definitions with an integer value in {CSRC}"
        _constants[name] = int(found[0])
    return _constants[name]


def counts_for(unit, second_level=False):
    """0, 1 and U + 1 (U = 1 gives 0, 1, 2; one workgroup per item: 3 instead, two full units and a tail); 2U + 1 where the shape
    has a second grouping level"""
    c = [0, 1, unit + 1 if unit > 1 else 3]
    if second_level:
        c.append(2 * unit + 1)
    return sorted(set(c))


# launch shapes of the default path's blind rotation (tests/test_gpu_positions.py::SHAPES holds the options): rotations per workgroup
BR_SHAPE_UNIT = {
    "batch": lambda: csrc_constant("kBatchWaves", ("launch_plan.h",)),
    "half": lambda: csrc_constant("kBatchWaves", ("launch_plan.h",)) // 2,
    "ll": lambda: 1,
    "ll2": lambda: 1,           # a workgroup per rotation (ll) / per pair (ll2): counts 0, 1 and 3
}
KS_SHAPES = [(1, 1), (6, 1), (16, 2), (16, 64)]      # (ks_per_wg, ks_slices); slices > 1: zero, then vector atomics


def ks_options(per, slices):
    return dict(ks_wg_threshold=0, ks_split_threshold=0, ks_per_wg=per, ks_slices=slices)


class Case:
    """One entry point of include/cufhe_amd.h.
    symbol: the C symbol.  unit(variant) -> U and unit_source: where U comes from.  variants: the dicts a run is made for -- each
    holds "opts" (cufhe_amd_set_option keys for positions.options) and the case's own parameters.  counts(variant) -> the counts.
    build(env, variant, count) -> Call (operands, input words, the callable that makes the call, the expected words); it lives in
    tests/test_gpu_footprint.py under the name `build`, as does the reference it uses.  aliasing: the overlaps the header permits
    (run once at U + 1 with the aliased operand declared inout) and forbids (must return -1 and leave the arena unchanged)."""

    def __init__(self, symbol, unit_source, variants, unit, build, second_level=False, permitted=(), forbidden=(), counts=None):
        self.symbol, self.unit_source, self.variants, self.unit, self.build = symbol, unit_source, variants, unit, build
        self.second_level, self.permitted, self.forbidden = second_level, tuple(permitted), tuple(forbidden)
        self._counts = counts

    def counts(self, variant):
        if self._counts is not None:
            return list(self._counts(variant))
        return counts_for(self.unit(variant), self.second_level)

    def runs(self):
        """(variant id, variant, count) of every run of the case"""
        out = []
        for v in self.variants:
            for c in self.counts(v):
                out.append((f"{v['id']}-{c}", v, c))
        return out


def _v(id_, opts=None, **params):
    return dict(id=id_, opts=opts or {}, **params)


def _br_variants(extra=({},)):
    import itertools
    out = []
    for shape, e in itertools.product(BR_SHAPE_UNIT, extra):
        tag = "-".join(f"{k}{v}" for k, v in e.items())
        out.append(_v(shape + ("-" + tag if tag else ""), shape=shape, **e))      # opts: SHAPES[shape], resolved by the GPU module
    return out


def _br_unit(v):
    return BR_SHAPE_UNIT[v["shape"]]()


def _ks_variants():
    return [_v(f"{p}x{s}", ks_options(p, s), per=p) for p, s in KS_SHAPES] + [_v("default", {}, per=None)]


def _ks_unit(v):
    return v["per"] if v["per"] else csrc_constant("kKsMaxPerWg", ("launch_plan.h",))


def _const_unit(name, files=None):
    return lambda v: csrc_constant(name, files)


PS_SETS = ("k2n512", "cggi16", "smallmod")
PS_CMUX_SETS = ("k2n512", "cggi16")                  # the small-modulus set has no TRGSW2NTT / CMUXNTT (include/cufhe_amd.h)
PS_THRESHOLDS = {"wave-per-rotation": 1, "workgroup-per-rotation": 1 << 30}      # test_paramset_forced_shapes' two extremes


def _ps_unit(v):
    """the wave-per-rotation kernel takes kPsbWavesOf rotations per workgroup, the other one rotation"""
    if v.get("threshold") == "workgroup-per-rotation":
        return 1
    return csrc_constant("kPsbWavesOf", ("kernels_ps.hip.h",))


def _ps_variants(levels=(None,), thresholds=True, sets=PS_SETS, extra=({},)):
    out = []
    for s in sets:
        for lv in levels:
            for t in (PS_THRESHOLDS if thresholds else (None,)):
                for e in extra:
                    tag = "-".join([s] + ([f"level{lv}"] if lv is not None else []) + ([t] if t else []) + [f"{k}{x}" for k, x in e.items() if x is not None])
                    opts = dict(ps_batch_threshold=PS_THRESHOLDS[t]) if t else {}
                    out.append(_v(tag, opts, set=s, level=lv, threshold=t, **e))
    return out


CASES = {}


def _case(symbol, unit_source, variants, unit, **kw):
    CASES[symbol] = Case(symbol, unit_source, variants, unit, build=symbol[len("cufhe_amd_"):], **kw)


# a. the default path's blind-rotation entry points, on the four forced shapes
_U_BR = "plan::kBatchWaves (launch_plan.h): 8 per workgroup, 4 on the half shape, a workgroup per rotation on ll / ll2"
_GATE_LIST = 17      # the op list of the gate cases holds 15 ops; 17 = 2 * 8 + 1 runs all of it on every shape
_case("cufhe_amd_gate_batch", _U_BR, _br_variants([dict(level=0), dict(level=1), dict(level=0, pad=1), dict(level=1, pad=1)]), _br_unit,
      counts=lambda v: sorted(set(counts_for(_br_unit(v)) + [_GATE_LIST])), permitted=("out == in0",))
_case("cufhe_amd_gate_list", _U_BR, _br_variants([dict(level=0), dict(level=1)]), _br_unit,
      counts=lambda v: sorted(set(counts_for(_br_unit(v)) + [_GATE_LIST])))
_case("cufhe_amd_blind_rotate_batch", _U_BR, _br_variants([dict(steps=1), dict(steps=-1)]), _br_unit)
_case("cufhe_amd_bootstrap_batch", _U_BR, _br_variants(), _br_unit)
_case("cufhe_amd_refresh_batch", _U_BR, _br_variants(), _br_unit, permitted=("trlwe_out == trlwe_in",))
_case("cufhe_amd_lut_rotate_batch", _U_BR, _br_variants([dict(nout=1), dict(nout=8)]), _br_unit)
_case("cufhe_amd_lut_lookup_batch", _U_BR, _br_variants([dict(nout=1), dict(nout=8)]), _br_unit)
# b. key switches
_U_KS = "ks_per_wg (cufhe_amd_set_option); under the default rule plan::kKsMaxPerWg (launch_plan.h), the most a workgroup takes"
for _s in ("cufhe_amd_keyswitch_batch", "cufhe_amd_sample_extract_keyswitch_batch", "cufhe_amd_sample_extract_index_keyswitch_batch"):
    _case(_s, _U_KS, _ks_variants(), _ks_unit)
# c. TRLWE level
_U_NTT = "kNttWavesPerBlock (kernels_common.hip.h)"
_U_ROT = "kRotWavesPerBlock (kernels.hip.h)"
_case("cufhe_amd_trgsw_to_ntt_batch", _U_NTT, [_v("default")], _const_unit("kNttWavesPerBlock"))
_case("cufhe_amd_cmux_batch", _U_NTT, [_v("default")], _const_unit("kNttWavesPerBlock"), permitted=("res == c0", "res == c1"))
_case("cufhe_amd_trlwe_rotate_batch", _U_ROT, [_v("default")], _const_unit("kRotWavesPerBlock"), forbidden=("out overlaps in",))
_case("cufhe_amd_cmux_rotate_batch", _U_NTT, [_v("default")], _const_unit("kNttWavesPerBlock"), permitted=("res == c",))
_case("cufhe_amd_sample_extract_index_batch", _U_ROT, [_v("src-null", src=False), _v("src-shared", src=True)], _const_unit("kRotWavesPerBlock"))
_case("cufhe_amd_polymul_batch", _U_NTT, [_v("default")], _const_unit("kNttWavesPerBlock"))
_case("cufhe_amd_polymul512_batch", _U_NTT, [_v("default")], _const_unit("kNttWavesPerBlock"))
SPREADS = [(1, 1), (1, 2), (1, 3), (1, 256), (1, 1024), (4, 64), (8, 128), (3, 341)]      # tests/test_gpu_lut.py::SPREADS (test_footprint.py compares)
_case("cufhe_amd_trlwe_spread_batch", "kSpreadWavesPerBlock (kernels_lut.hip.h)",
      [_v(f"stride{s}-reps{r}", stride=s, reps=r) for s, r in SPREADS], _const_unit("kSpreadWavesPerBlock"), forbidden=("out overlaps in",))
# d. the N = 2048 ring: a workgroup per rotation on both kernels
_U_ONE = "one workgroup per rotation (kernels_lvl2.hip.h, kernels_lvl2q.hip.h): counts 0, 1 and 3"
_RING = [_v(f"lvl2_kernel{k}", dict(lvl2_kernel=k)) for k in (0, 1)]
_case("cufhe_amd_lvl2_gate_batch", _U_ONE, _RING, lambda v: 1)
_case("cufhe_amd_lvl2_blind_rotate_batch", _U_ONE, [_v(f"lvl2_kernel{k}-steps{s}", dict(lvl2_kernel=k), steps=s) for k in (0, 1) for s in (1, -1)],
      lambda v: 1)
_case("cufhe_amd_lvl2_user_rotate_batch", _U_ONE, _RING, lambda v: 1)
_case("cufhe_amd_lvl2_user_extract_batch", _U_ONE, _RING, lambda v: 1)
_case("cufhe_amd_lvl2_keyswitch_batch", _U_KS, [_v("default", {}, per=None), _v("16x64", dict(ks_wg_threshold=0, ks_per_wg=16, ks_slices=64), per=16)],
      _ks_unit)
# e. circuit bootstrapping and packing
_case("cufhe_amd_cb_rotate_batch", _U_ONE, _RING, lambda v: 1)
_case("cufhe_amd_private_keyswitch_batch", "kPksTile (kernels_pks.hip.h); small counts cut i into slices: zero, then vector atomics",
      [_v("default")], _const_unit("kPksTile"))
_case("cufhe_amd_circuit_bootstrap_batch", _U_ONE + "; three rotations and one private key switch per input",
      [_v("both", outs=("trgsw", "trgsw_ntt")), _v("torus-only", outs=("trgsw",)), _v("ntt-only", outs=("trgsw_ntt",))], lambda v: 1)
_case("cufhe_amd_pack_batch", "kPackTile (kernels_pack.hip.h)",
      [_v(f"out{o}" + (f"-cus{c}" if c else ""), dict(cus_override=c) if c else {}, count_out=o) for o in (1, 5) for c in (0, 40)],
      _const_unit("kPackTile"))
# f. the parameter sets
_U_PS = "kPsbWavesOf (kernels_ps.hip.h) on the wave-per-rotation kernel, 1 on the workgroup-per-rotation kernel (ps_batch_threshold)"
_case("cufhe_amd_ps_gate_batch", _U_PS, _ps_variants(), _ps_unit)
_case("cufhe_amd_ps_gate_batch_level", _U_PS, _ps_variants(levels=(0, 1)), _ps_unit)
_case("cufhe_amd_ps_blind_rotate_batch", _U_PS, _ps_variants(), _ps_unit)
_case("cufhe_amd_ps_keyswitch_batch", _U_KS, _ps_variants(thresholds=False, extra=[dict(per=None)]), _ks_unit)
_case("cufhe_amd_ps_trgsw_to_ntt_batch", _U_NTT, _ps_variants(thresholds=False, sets=PS_CMUX_SETS), _const_unit("kNttWavesPerBlock"))
_case("cufhe_amd_ps_cmux_batch", _U_NTT, _ps_variants(thresholds=False, sets=PS_CMUX_SETS), _const_unit("kNttWavesPerBlock"),
      permitted=("res == c0", "res == c1"))
_case("cufhe_amd_ps_trlwe_op_batch", _U_PS, _ps_variants(extra=[dict(op="bootstrap"), dict(op="refresh"), dict(op="seiks")]), _ps_unit)

# symbol -> reason: only entry points whose outputs are not caller-owned device arrays
EXCLUDED = {}

# the three launches of one row too many by which the GPU module proves that it can fail (tests/test_gpu_footprint.py)
OVERLONG = ("cufhe_amd_blind_rotate_batch", "cufhe_amd_keyswitch_batch", "cufhe_amd_trlwe_rotate_batch")


def header_batch_symbols(path=None):
    """every function include/cufhe_amd.h declares whose name ends in _batch or _batch_level, plus cufhe_amd_gate_list"""
    text = open(path or os.path.join(ROOT, "include", "cufhe_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = re.findall(r"\bint\s+(cufhe_amd_\w+)\s*\(", text)
    return sorted({s for s in names if s.endswith("_batch") or s.endswith("_batch_level") or s == "cufhe_amd_gate_list"})
