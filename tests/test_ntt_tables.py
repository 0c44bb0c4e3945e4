"""CPU tests of the twiddle tables every transform kernel reads (cufhe_amd/csrc/ntt_tables.h), built by the library's own
builders in tests/host/ntt_tables_harness.cpp: the bytes are the ones recorded from the code the header replaced
(tests/golden/ntt_tables_v1.json), and the roots, the sub-transform selection, the radix-4 product slots and the packed copies
have the properties the kernels rely on, computed here in Python integers."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from test_fpfield import hm  # noqa: F401  (fixture: the host model, which holds its own transcription of the r4 tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ntt_tables_harness.cpp")
EXE = os.path.join(ROOT, "tests", "host", "ntt_tables_harness")
DEPS = [SRC, os.path.join(ROOT, "cufhe_amd", "csrc", "ntt_tables.h"), os.path.join(ROOT, "cufhe_amd", "csrc", "fpfield.h")]
P = 875781160960001
PSI_2048 = 423584205157050
ROOT4 = 5440**2


def _fields(*spec):
    return np.dtype([(name, "<f8", (count,)) for name, count in spec])


NTT = _fields(("tu_fwd", 16), ("tu_inv", 16), ("tb_fwd", 240), ("tb_inv", 240), ("tc_fwd", 768), ("tc_inv", 768),
              ("tbp_fwd", 288), ("tbp_inv", 288), ("tcp_fwd", 896), ("tcp_inv", 896))
NTT512 = _fields(("tu_fwd", 8), ("tu_inv", 8), ("tb_fwd", 56), ("tb_inv", 56), ("tc_fwd", 448), ("tc_inv", 448),
                 ("uwb_fwd", 8), ("uwb_inv", 8), ("uwc_fwd", 64), ("uwc_inv", 64))
# the order of `ntt_tables_harness tables`
LAYOUT = [("ntt1024", NTT), ("ntt1024_r4", NTT), ("lvl2_half_0", NTT), ("lvl2_half_1", NTT),
          ("ntt512_half_0", NTT512), ("ntt512_half_1", NTT512), ("ntt512_standalone", NTT512),
          ("lvl2_quarter_0", NTT512), ("lvl2_quarter_1", NTT512), ("lvl2_quarter_2", NTT512), ("lvl2_quarter_3", NTT512)]
R4_512 = [name for name, _ in LAYOUT[4:] if name != "ntt512_standalone"]


def _bal(v):
    v %= P
    return v - P if v > P // 2 else v


def _ints(a):
    out = [int(v) for v in a]
    assert all(float(v) == w for v, w in zip(out, a))       # every entry an integer
    return out


def _split(raw):
    assert len(raw) == sum(dt.itemsize for _, dt in LAYOUT)
    out, off = {}, 0
    for name, dt in LAYOUT:
        out[name] = raw[off:off + dt.itemsize]
        off += dt.itemsize
    return out


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-o", EXE, SRC])
    return EXE


@pytest.fixture(scope="module")
def table_bytes(harness):
    return _split(subprocess.run([harness, "tables"], capture_output=True, check=True, timeout=300).stdout)


@pytest.fixture(scope="module")
def tables(table_bytes):
    """name -> {field -> list of Python integers}"""
    return {name: {f: _ints(np.frombuffer(table_bytes[name], dt)[0][f]) for f in dt.names} for name, dt in LAYOUT}


@pytest.fixture(scope="module")
def roots(harness):
    return json.loads(subprocess.run([harness, "roots"], capture_output=True, check=True, text=True, timeout=300).stdout)


def test_same_bytes_as_the_recorded_tables(table_bytes):
    """The fixture was recorded from the builders this header replaced (see its "what"): the refactoring moved no byte."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "ntt_tables_v1.json")))["sha256"]
    assert sorted(want) == sorted(name for name, _ in LAYOUT)
    got = {name: hashlib.sha256(b).hexdigest() for name, b in table_bytes.items()}
    assert got == want


def test_constants(roots):
    assert roots["p"] == P and roots["psi_2048"] == PSI_2048 and roots["root4"] == ROOT4
    psi = roots["psi_4096"]
    assert psi * psi % P == PSI_2048 and pow(psi, 1024, P) == ROOT4
    assert pow(psi, 2048, P) == P - 1                      # a primitive 4096-th root
    for n, v in roots["n_inverse"].items():
        assert abs(v) <= P // 2 and int(n) * v % P == 1


@pytest.mark.parametrize("name,psi_of,bits", [("roots_512", lambda r: PSI_2048**2 % P, 9), ("roots_1024", lambda r: PSI_2048, 10),
                                              ("roots_2048", lambda r: r["psi_4096"], 11)])
def test_roots_are_inverse_pairs_in_bit_reversed_order(roots, name, psi_of, bits):
    fwd, inv, psi = roots[name]["fwd"], roots[name]["inv"], psi_of(roots)
    assert len(fwd) == len(inv) == 1 << bits
    for i in range(1 << bits):
        assert fwd[i] * inv[i] % P == 1
        assert abs(fwd[i]) <= P // 2 and abs(inv[i]) <= P // 2
        assert fwd[i] == _bal(pow(psi, int(format(i, "0%db" % bits)[::-1], 2), P))


@pytest.mark.parametrize("full,parts,part", [("roots_1024", 2, "half_%d_of_1024"), ("roots_2048", 2, "half_%d_of_2048"),
                                             ("roots_2048", 4, "quarter_%d_of_2048")])
def test_sub_transforms_interleave_to_the_full_roots(roots, full, parts, part):
    """root_h[m + g] = root[parts m + h m + g]: put back by that rule, the sub-transforms fill every entry of the full array behind
    the first `parts` (the stages in front of the split) exactly once -- and their pairs are inverse to each other too."""
    for d in ("fwd", "inv"):
        want = roots[full][d]
        n = len(want) // parts
        got, hits = [None] * len(want), [0] * len(want)
        for h in range(parts):
            sub = roots[part % h][d]
            assert len(sub) == n and sub[0] == 0
            m = 1
            while m < n:
                for g in range(m):
                    got[parts * m + h * m + g] = sub[m + g]
                    hits[parts * m + h * m + g] += 1
                m *= 2
        assert hits == [0] * parts + [1] * (len(want) - parts)
        assert got[parts:] == want[parts:]
    for h in range(parts):
        sub = roots[part % h]
        assert all(f * v % P == 1 for f, v in zip(sub["fwd"][1:], sub["inv"][1:]))


def _r4_slots_1024():
    """(field, product slot, factor slot, factor slot) of an r4 NttTables"""
    for d in ("fwd", "inv"):
        yield "tu_" + d, 2, 1, 0
        for g in range(4):
            yield "tu_" + d, 8 + 2 * g, 7 + 2 * g, 3 + g
        for lam in range(16):
            yield "tb_" + d, 2 * 16 + lam, 1 * 16 + lam, lam
            for g in range(4):
                yield "tb_" + d, (8 + 2 * g) * 16 + lam, (7 + 2 * g) * 16 + lam, (3 + g) * 16 + lam
        for lane in range(64):
            for g in range(4):
                yield "tc_" + d, (5 + 2 * g) * 64 + lane, (4 + 2 * g) * 64 + lane, g * 64 + lane


def test_r4_product_slots_of_the_1024_point_tables(tables):
    """ntt_r4.h: slot 2 = u w, slot 8 + 2g = u_g w_g (tc: slot 5 + 2g); every other slot is the plain table's."""
    plain, r4 = tables["ntt1024"], tables["ntt1024_r4"]
    products = {}
    for f, slot, a, b in _r4_slots_1024():
        assert r4[f][slot] == _bal(plain[f][a] * plain[f][b]), (f, slot)
        products.setdefault(f, set()).add(slot)
    assert sum(len(s) for s in products.values()) == 2 * (5 + 16 * 5 + 64 * 4)
    for f in ("tu_fwd", "tu_inv", "tb_fwd", "tb_inv", "tc_fwd", "tc_inv"):
        assert all(r4[f][i] == plain[f][i] for i in range(len(plain[f])) if i not in products[f]), f


@pytest.mark.parametrize("name", R4_512)
def test_r4_product_slots_of_the_512_point_tables(tables, name):
    """ntt_wave512.h q4: u w in tu[7], uwb[lam], uwc[lane]; the block's second stage-b twiddle is I times (inverse: -I times) the first."""
    t = tables[name]
    for d, i4 in (("fwd", ROOT4), ("inv", -ROOT4)):
        tu, tb, tc = t["tu_" + d], t["tb_" + d], t["tc_" + d]
        assert tu[7] == _bal(tu[0] * tu[1]) and tu[2] == _bal(i4 * tu[1])
        for lam in range(8):
            assert t["uwb_" + d][lam] == _bal(tb[lam] * tb[8 + lam]) and tb[16 + lam] == _bal(i4 * tb[8 + lam])
        for lane in range(64):
            assert t["uwc_" + d][lane] == _bal(tc[lane] * tc[64 + lane]) and tc[128 + lane] == _bal(i4 * tc[64 + lane])


def test_stand_alone_512_point_table_has_no_r4_products(tables):
    """Its kernels run the radix-2 form: the product fields stay zero."""
    t = tables["ntt512_standalone"]
    assert t["tu_fwd"][7] == 0 and t["tu_inv"][7] == 0
    assert not any(t["uwb_fwd"] + t["uwb_inv"] + t["uwc_fwd"] + t["uwc_inv"])


@pytest.mark.parametrize("name", [n for n, dt in LAYOUT if dt is NTT])
def test_packed_arrays_are_the_per_lane_transposes(tables, name):
    """tbp[lam][k] = tb[k][lam] at stride 18, tcp[lane][k] = tc[k][lane] at stride 14, padding zero -- in the r4 table; the others
    leave the packed block zero."""
    t = tables[name]
    for d in ("fwd", "inv"):
        tbp, tcp = t["tbp_" + d], t["tcp_" + d]
        if name != "ntt1024_r4":
            assert not any(tbp) and not any(tcp)
            continue
        for lam in range(16):
            assert tbp[lam * 18:lam * 18 + 18] == [t["tb_" + d][k * 16 + lam] for k in range(15)] + [0, 0, 0]
        for lane in range(64):
            assert tcp[lane * 14:lane * 14 + 14] == [t["tc_" + d][k * 64 + lane] for k in range(12)] + [0, 0]


def test_r4_table_equals_the_host_models_transcription(tables, hm):  # noqa: F811
    """tests/host/host_model.cpp writes the r4 twiddle blocks down on its own (it does not include ntt_tables.h) and runs the
    device's radix-4 passes on them (test_fpfield.py): the library's r4 table is that, entry for entry."""
    hm.hm_r4_tables.argtypes = [np.ctypeslib.ndpointer(np.float64, flags="C")]
    hm.hm_r4_tables.restype = None
    out = np.zeros(2 * (15 + 240 + 768))
    hm.hm_r4_tables(out)
    model = _ints(out)
    t = tables["ntt1024_r4"]
    assert model[0:15] == t["tu_fwd"][:15] and model[15:30] == t["tu_inv"][:15]
    assert model[30:270] == t["tb_fwd"] and model[270:510] == t["tb_inv"]
    assert model[510:1278] == t["tc_fwd"] and model[1278:2046] == t["tc_inv"]


def test_sanitizers(tmp_path, table_bytes, roots):
    """The same program under AddressSanitizer + UBSan, as its own process: same output."""
    exe = str(tmp_path / "ntt_tables_harness_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.run([exe, "tables"], capture_output=True, timeout=300)
    assert out.returncode == 0 and out.stderr == b"", out.stderr[-3000:]
    assert _split(out.stdout) == table_bytes
    out = subprocess.run([exe, "roots"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-3000:]
    assert json.loads(out.stdout) == roots
