"""Python mirror of the cuFHE host API for the gate path, over the C ABI.

Names, argument order and completion semantics follow include/cufhe_gpu.cuh of the
reference (SetGPUNum / Initialize / CleanUp / Synchronize / Stream / StreamQuery / Ctxt /
And ... NMux, Not, Copy and the g-prefixed device-resident variants,
/root/reference/include/cufhe_gpu.cuh:54-313, src/cufhe_gates_gpu.cu:148-665).
Everything here is plumbing: the arithmetic runs in libcufhe_amd.so.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check, Params, Profile, Lvl2Params, SchedStats, PsParams, CbParams, PackParams

# op codes (include/cufhe_amd.h)
NAND, NOR, XNOR, AND, OR, XOR, ANDNY, ANDYN, ORNY, ORYN, MUX, NMUX, NOT, COPY = range(14)
OP_NAMES = ["NAND", "NOR", "XNOR", "AND", "OR", "XOR", "ANDNY", "ANDYN", "ORNY", "ORYN",
            "MUX", "NMUX", "NOT", "COPY"]


def params():
    p = Params()
    check(lib.cufhe_amd_get_params(ctypes.byref(p)))
    return p


PARAMS = params()
LVL_WORDS = (PARAMS.lvl0_words, PARAMS.lvl1_words)

_stream_count = 0          # `streamCount`, src/cufhe_gates_gpu.cu:36


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a


def SetGPUNum(gpu_num):
    check(lib.cufhe_amd_set_gpu_num(int(gpu_num)))


def GetGPUNum():
    return lib.cufhe_amd_get_gpu_num()


def DeviceCount():
    return lib.cufhe_amd_device_count()


def device_identity(device=0):
    """Which physical GPU a logical device is: {'pci': ..., 'uuid': ..., 'hip_device': ..., 'local_cpus': ...}."""
    buf = ctypes.create_string_buffer(512)
    check(lib.cufhe_amd_device_identity(int(device), buf, len(buf)))
    return dict(kv.split("=", 1) for kv in buf.value.decode().split())


def device_cus(device=0):
    """compute units of a logical device ("cus_override" included): the unit of the launch-shape and flush rules"""
    return check(lib.cufhe_amd_device_cus(int(device)))


def device_mem_info(device=0):
    """(free, total) bytes of the device (hipMemGetInfo)"""
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib.cufhe_amd_device_mem_info(int(device), ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def Initialize(bk=None, ksk=None):
    """Initialize() / Initialize(ek): bk, ksk are the torus-domain keys as uint32 arrays."""
    if bk is None:
        check(lib.cufhe_amd_initialize_ntt())
        return
    bk = np.ascontiguousarray(bk, dtype=np.uint32).ravel()
    ksk = np.ascontiguousarray(ksk, dtype=np.uint32).ravel()
    check(lib.cufhe_amd_initialize(_ptr(bk), bk.size, _ptr(ksk), ksk.size))


def CleanUp():
    check(lib.cufhe_amd_cleanup())


def Synchronize():
    check(lib.cufhe_amd_synchronize())


class Stream:
    """class Stream, include/cufhe_gpu.cuh:152-189: default ctor round-robins devices,
    Create() makes a non-blocking stream, the destructor does not destroy it."""

    def __init__(self, device_id=None):
        global _stream_count
        self._device_id = (_stream_count % GetGPUNum()) if device_id is None else int(device_id)
        _stream_count += 1
        self._st = ctypes.c_void_p(None)

    def Create(self):
        check(lib.cufhe_amd_stream_create(self._device_id, ctypes.byref(self._st)))

    def Destroy(self):
        check(lib.cufhe_amd_stream_destroy(self._device_id, self._st))
        self._st = ctypes.c_void_p(None)

    def st(self):
        return self._st

    def device_id(self):
        return self._device_id


def StreamQuery(st):
    return check(lib.cufhe_amd_stream_query(st.device_id(), st.st())) == 1


class DeviceBuffer:
    """`words` uint32 words of device memory on one GPU."""

    def __init__(self, words, device=0):
        self.words, self.device = int(words), int(device)
        p = ctypes.c_void_p()
        check(lib.cufhe_amd_malloc(self.device, self.words * 4, ctypes.byref(p)))
        self.ptr = p.value
        _lib.live.add(self)

    def upload(self, host, stream=None):
        host = np.ascontiguousarray(host, dtype=np.uint32).ravel()
        assert host.size <= self.words
        check(lib.cufhe_amd_memcpy_h2d(self.device, stream, self.ptr, _ptr(host), host.size * 4))
        check(lib.cufhe_amd_stream_synchronize(self.device, stream))
        return self

    def download(self, words=None, stream=None):
        out = np.empty(self.words if words is None else words, dtype=np.uint32)
        check(lib.cufhe_amd_memcpy_d2h(self.device, stream, _ptr(out), self.ptr, out.size * 4))
        check(lib.cufhe_amd_stream_synchronize(self.device, stream))
        return out

    def free(self):
        if self.ptr and not _lib.closed:
            check(lib.cufhe_amd_free(self.device, self.ptr))
        self.ptr = None

    release = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Ctxt:
    """template<class P> struct Ctxt, include/cufhe_gpu.cuh:102-121: a pinned host TLWE
    (`tlwehost`) plus one device buffer per GPU (`tlwedevices`).  level 0 = lvl0param,
    level 1 = lvl1param."""

    def __init__(self, level=0):
        self.level = int(level)
        # n + 1 / k N + 1 words of the parameter set the per-gate API runs on ("param_set"; the BASELINE set unless chosen otherwise)
        self.tlwehost = np.zeros(lib.cufhe_amd_ctxt_words(self.level), dtype=np.uint32)
        h = ctypes.c_void_p()
        check(lib.cufhe_amd_ctxt_create(self.level, _ptr(self.tlwehost), ctypes.byref(h)))
        self._h = h
        _lib.live.add(self)

    @property
    def tlwedevices(self):
        return [lib.cufhe_amd_ctxt_device_ptr(self._h, d) for d in range(GetGPUNum())]

    def release(self):
        if self._h and not _lib.closed:
            lib.cufhe_amd_ctxt_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Trlwe(Ctxt):
    """struct cuFHETRLWElvl1, include/cufhe_gpu.cuh:124-134: `trlwehost` ((k+1) N words) + a device buffer per GPU."""

    def __init__(self):
        self.level = 2
        self.tlwehost = np.zeros(lib.cufhe_amd_ctxt_words(2), dtype=np.uint32)      # (k+1) N words of the active parameter set
        self.trlwehost = self.tlwehost
        h = ctypes.c_void_p()
        check(lib.cufhe_amd_ctxt_create(2, _ptr(self.tlwehost), ctypes.byref(h)))
        self._h = h
        _lib.live.add(self)


class TrgswNtt(Ctxt):
    """struct cuFHETRGSWNTTlvl1, include/cufhe_gpu.cuh:136-146: a TRGSW in the NTT domain (ciphertext handle of level 3): the selector of
    CMUXNTT, the output of CircuitBootstrapping."""

    def __init__(self):
        super().__init__(3)
        self.trgswhost = self.tlwehost


TL_BOOTSTRAP, TL_REFRESH, TL_SEIKS, TL_CMUX, TL_CIRCUIT_BOOTSTRAP = 100, 101, 102, 103, 104


def _trlwe_op(op, copying, out, inp, st):
    check(lib.cufhe_amd_enqueue_trlwe_op(st.device_id(), st.st(), op, 1 if copying else 0, out._h, inp._h))


def GateBootstrappingTLWE2TRLWElvl01NTT(out, inp, st):     # src/cufhe_gates_gpu.cu:96-104
    _trlwe_op(TL_BOOTSTRAP, True, out, inp, st)


def gGateBootstrappingTLWE2TRLWElvl01NTT(out, inp, st):    # :86-94
    _trlwe_op(TL_BOOTSTRAP, False, out, inp, st)


def Refresh(out, inp, st):                                 # :115-124
    _trlwe_op(TL_REFRESH, True, out, inp, st)


def gRefresh(out, inp, st):                                # :106-113
    _trlwe_op(TL_REFRESH, False, out, inp, st)


TL_SEIKS_AT_BASE, TL_CMUX_ROTATE_BASE = 2048, 4096         # op ids that carry an index / an exponent (include/cufhe_amd.h)


def TL_SEIKS_AT(index):
    """CUFHE_AMD_TL_SEIKS_AT(index): SampleExtract at `index`, then the key switch (packed ROM words)"""
    return TL_SEIKS_AT_BASE + int(index)


def gSampleExtractAndKeySwitch(out, inp, st, index=None):  # :126-135 (uploads in.trlwehost, as the reference does)
    """index given (0 included): extraction at that coefficient on device buffers only -- the form that follows gCMUXNTT /
    gCMUXRotateNTT without a copy; the reference's index-less call keeps its upload of inp.trlwehost."""
    if index is not None:
        return _trlwe_op(TL_SEIKS_AT(index), False, out, inp, st)
    CtxtCopyH2D(inp, st)
    _trlwe_op(TL_SEIKS, False, out, inp, st)


def SampleExtractAndKeySwitch(out, inp, st, index=0):      # :137-146
    """index != 0: extraction at that coefficient, from inp.trlwehost to out.tlwehost"""
    if index != 0:
        return _trlwe_op(TL_SEIKS_AT(index), True, out, inp, st)
    gSampleExtractAndKeySwitch(out, inp, st)
    CtxtCopyD2H(out, st)


def gCMUXNTT(res, cs, c1, c0, st):                         # res = c0 + cs [x] (c1 - c0), device buffers
    check(lib.cufhe_amd_enqueue_cmux(st.device_id(), st.st(), 0, res._h, cs._h, c1._h, c0._h))


def CMUXNTT(res, cs, c1, c0, st):                          # the same from and to the host members
    check(lib.cufhe_amd_enqueue_cmux(st.device_id(), st.st(), 1, res._h, cs._h, c1._h, c0._h))


def gCMUXRotateNTT(res, cs, c, exponent, st):              # res = c + cs [x] (X^exponent c - c), device buffers; res may be c
    check(lib.cufhe_amd_enqueue_cmux_rotate(st.device_id(), st.st(), 0, res._h, cs._h, c._h, int(exponent)))


def CMUXRotateNTT(res, cs, c, exponent, st):               # the same from and to the host members
    check(lib.cufhe_amd_enqueue_cmux_rotate(st.device_id(), st.st(), 1, res._h, cs._h, c._h, int(exponent)))


def gCircuitBootstrapping(out, inp, st):
    """out (TrgswNtt) <- the circuit bootstrap of lvl0 ciphertext inp, device buffers (cufhe_amd_circuit_bootstrap_batch)"""
    _trlwe_op(TL_CIRCUIT_BOOTSTRAP, False, out, inp, st)


def CircuitBootstrapping(out, inp, st):
    """the same from inp.tlwehost, the NTT-domain words delivered to out.trgswhost"""
    _trlwe_op(TL_CIRCUIT_BOOTSTRAP, True, out, inp, st)


def TRGSW2NTT(out, trgsw, st):                             # src/bootstrap_gpu.cu:75-94
    """out (TrgswNtt) <- the NTT-domain words of the torus-domain TRGSW `trgsw` ((k+1) l (k+1) N uint32): written to out.trgswhost
    before the call returns, their upload to the stream's device recorded like a CtxtCopyH2D (cufhe_amd_trgsw_to_ntt)"""
    t = np.ascontiguousarray(trgsw, dtype=np.uint32)
    check(lib.cufhe_amd_trgsw_to_ntt(st.device_id(), st.st(), t.ctypes.data, out._h))


def CtxtCopyH2D(c, st):
    check(lib.cufhe_amd_enqueue_copy(st.device_id(), st.st(), c._h, 1))


def CtxtCopyD2H(c, st):
    check(lib.cufhe_amd_enqueue_copy(st.device_id(), st.st(), c._h, 0))


def CopyOnHost(out, inp):
    out.tlwehost[:] = inp.tlwehost


def Flush(device=0):
    """Launch the recorded gates of `device` without waiting (no reference counterpart:
    the reference launches at call time)."""
    check(lib.cufhe_amd_flush(device))


def _gate(op, copying, out, ins, st):
    hs = [c._h for c in ins] + [None] * (3 - len(ins))
    check(lib.cufhe_amd_enqueue_gate(st.device_id(), st.st(), op, 1 if copying else 0, out._h, *hs))


def _make2(op, copying):
    def f(out, in0, in1, st):
        _gate(op, copying, out, [in0, in1], st)
    return f


def _make1(op, copying):
    def f(out, in0, st):
        _gate(op, copying, out, [in0], st)
    return f


def _make3(op, copying):
    def f(out, inc, in1, in0, st):               # Mux(out, inc, in1, in0, st)
        _gate(op, copying, out, [inc, in1, in0], st)
    return f


And, gAnd = _make2(AND, True), _make2(AND, False)
AndYN, gAndYN = _make2(ANDYN, True), _make2(ANDYN, False)
AndNY, gAndNY = _make2(ANDNY, True), _make2(ANDNY, False)
Or, gOr = _make2(OR, True), _make2(OR, False)
OrYN, gOrYN = _make2(ORYN, True), _make2(ORYN, False)
OrNY, gOrNY = _make2(ORNY, True), _make2(ORNY, False)
Nand, gNand = _make2(NAND, True), _make2(NAND, False)
Nor, gNor = _make2(NOR, True), _make2(NOR, False)
Xor, gXor = _make2(XOR, True), _make2(XOR, False)
Xnor, gXnor = _make2(XNOR, True), _make2(XNOR, False)
Not, gNot = _make1(NOT, True), _make1(NOT, False)
Copy, gCopy = _make1(COPY, True), _make1(COPY, False)
Mux, gMux = _make3(MUX, True), _make3(MUX, False)
NMux, gNMux = _make3(NMUX, True), _make3(NMUX, False)


# ---- user gates: programmable bootstrapping (cufhe_amd_define_gate, include/cufhe_amd.h) ----
USER_OP_BASE, MAX_USER_GATES = 1000, 64


def define_gate(coeffs, offset=0, test_vector=None, nout=1):
    """A user gate x = c0 in0 + c1 in1 + c2 in2 + (0, .., 0, offset) bootstrapped through `test_vector` (N torus words; None: the
    constant mu).  coeffs: one to three integers (missing ones are 0).  Returns the op id, usable wherever a built-in op is.
    nout = 2, 4 or 8: a multi-output gate (cufhe_amd_define_gate_multi; test_vector from test_vector_multi, required); output j is
    user_op_output(op, j)."""
    c = np.zeros(3, dtype=np.int32)
    c[:len(coeffs)] = coeffs
    tv = None
    if test_vector is not None:
        tv = np.ascontiguousarray(test_vector, dtype=np.uint32)
        if tv.size != PARAMS.N:
            raise ValueError(f"test vector must have N = {PARAMS.N} words")
    tvp = tv.ctypes.data_as(_lib.c_u32p) if tv is not None else None
    op = ctypes.c_int()
    if nout == 1:
        check(lib.cufhe_amd_define_gate(c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, tvp, ctypes.byref(op)))
    else:
        check(lib.cufhe_amd_define_gate_multi(c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, int(nout), tvp, ctypes.byref(op)))
    return op.value


def user_op_output(op, j):
    """The op id of output j of multi-output definition `op` (CUFHE_AMD_USER_OP_OUTPUT)."""
    return op + j * MAX_USER_GATES


def test_vector_multi(values):
    """The interleaved test vector of nout functions on p messages: values is [nout][p] torus words (cufhe_amd_test_vector_multi);
    TV[nout q + j] = values[j][box of position nout q]."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    if v.ndim != 2:
        raise ValueError("values must be [nout][p]")
    tv = np.empty(PARAMS.N, dtype=np.uint32)
    check(lib.cufhe_amd_test_vector_multi(v.ctypes.data_as(_lib.c_u32p), int(v.shape[1]), int(v.shape[0]), tv.ctypes.data_as(_lib.c_u32p)))
    return tv


test_vector_multi.__test__ = False


def test_vector(values):
    """The test vector of a function on len(values) messages (a power of two, 2 .. N/2) encoded with a padding bit, m -> m 2^32 / (2p):
    values are the output torus words (cufhe_amd_test_vector)."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    tv = np.empty(PARAMS.N, dtype=np.uint32)
    check(lib.cufhe_amd_test_vector(v.ctypes.data_as(_lib.c_u32p), int(v.size), tv.ctypes.data_as(_lib.c_u32p)))
    return tv


test_vector.__test__ = False      # not a pytest test where it is imported by name


def Apply(op, out, *ins_and_st):
    """Apply(op, out, in0[, in1[, in2]], st): a user gate (or any op) on the per-gate API, inputs from tlwehost, result delivered to
    out's tlwehost -- the copying form, like And(..)."""
    *ins, st = ins_and_st
    _gate(op, True, out, ins, st)


def gApply(op, out, *ins_and_st):
    """gApply(op, out, in0[, in1[, in2]], st): the device-resident form, like gAnd(..)."""
    *ins, st = ins_and_st
    _gate(op, False, out, ins, st)


def _gate_multi(op, copying, outs, ins, st):
    hs = [c._h for c in ins] + [None] * (3 - len(ins))
    arr = (ctypes.c_void_p * len(outs))(*[o._h for o in outs])
    check(lib.cufhe_amd_enqueue_gate_multi(st.device_id(), st.st(), op, 1 if copying else 0, len(outs), arr, *hs))


def ApplyMulti(op, outs, *ins_and_st):
    """ApplyMulti(op, [o0, o1, ..], in0[, in1[, in2]], st): all outputs of one evaluation of a multi-output gate (one rotation), inputs
    from tlwehost, results delivered to each output's tlwehost."""
    *ins, st = ins_and_st
    _gate_multi(op, True, list(outs), ins, st)


def gApplyMulti(op, outs, *ins_and_st):
    """gApplyMulti(op, [o0, o1, ..], in0[, in1[, in2]], st): the device-resident form."""
    *ins, st = ins_and_st
    _gate_multi(op, False, list(outs), ins, st)


# ---- native batched entry points (what bench.py and the parity tests drive) ----
def gate_batch(ops, level, out, in0, in1=None, in2=None, count=None, device=0, stream=None, stride_words=None, ops_stride=None):
    """ops: one op code or an int array of `count` codes; operands are DeviceBuffers holding
    `count` contiguous ciphertexts.  stride_words: words from one ciphertext of an operand to the next (default: packed);
    ops_stride: gate g takes ops[g * ops_stride] (default: 0 for one op code, 1 for an array)."""
    # n + 1 / k N + 1 words of the set the gate entry points run on NOW ("param_set"): the library dispatches level 0 and 1 to that set
    words = lib.cufhe_amd_ctxt_words(level) if level in (0, 1) else 1     # a bad level is rejected by the library
    if stride_words is None:
        stride_words = words
    if count is None:
        count = out.words // stride_words
    if np.isscalar(ops):
        ops_arr, stride = np.array([ops], dtype=np.int32), 0
    else:
        ops_arr, stride = np.ascontiguousarray(ops, dtype=np.int32), 1
    if ops_stride is not None:
        stride = int(ops_stride)
    assert count == 0 or ops_arr.size > (count - 1) * stride
    check(lib.cufhe_amd_gate_batch(device, stream, level, count, _ptr(ops_arr), stride, out.ptr, in0.ptr,
                                   in1.ptr if in1 is not None else None,
                                   in2.ptr if in2 is not None else None, stride_words))


def blind_rotate_batch(tlwe0, acc, count, steps=-1, device=0, stream=None):
    check(lib.cufhe_amd_blind_rotate_batch(device, stream, count, tlwe0.ptr, acc.ptr, steps))


def bootstrap_batch(out, inp, count, device=0, stream=None):
    """Bootstrap (src/bootstrap_gpu.cu:782-788): refresh `count` lvl0 ciphertexts."""
    check(lib.cufhe_amd_bootstrap_batch(device, stream, count, out.ptr, inp.ptr))


def keyswitch_batch(tlwe1, tlwe0, count, device=0, stream=None):
    check(lib.cufhe_amd_keyswitch_batch(device, stream, count, tlwe1.ptr, tlwe0.ptr))


def sample_extract_keyswitch_batch(trlwe, tlwe0, count, device=0, stream=None):
    check(lib.cufhe_amd_sample_extract_keyswitch_batch(device, stream, count, trlwe.ptr, tlwe0.ptr))


def refresh_batch(trlwe_in, trlwe_out, count, device=0, stream=None):
    check(lib.cufhe_amd_refresh_batch(device, stream, count, trlwe_in.ptr, trlwe_out.ptr))


def trgsw_to_ntt_batch(trgsw, trgsw_ntt, count, device=0, stream=None):
    check(lib.cufhe_amd_trgsw_to_ntt_batch(device, stream, count, trgsw.ptr, trgsw_ntt.ptr))


def cmux_batch(trgsw_ntt, c1, c0, res, count, device=0, stream=None):
    check(lib.cufhe_amd_cmux_batch(device, stream, count, trgsw_ntt.ptr, c1.ptr, c0.ptr, res.ptr))


# ---- packed ROM words: exps / src / idx are host integers, one per item ----
def _i32(values, count):
    a = np.ascontiguousarray(values, dtype=np.int32).ravel()
    assert a.size >= count
    return a


def trlwe_rotate_batch(inp, exps, out, count, device=0, stream=None):
    """out[g] = X^exps[g] inp[g] (negacyclic, 0 <= exps[g] < 2N) on TRLWEs [count][2N]; out must not overlap inp"""
    e = _i32(exps, count)
    check(lib.cufhe_amd_trlwe_rotate_batch(device, stream, count, inp.ptr, _ptr(e), out.ptr))


def cmux_rotate_batch(trgsw_ntt, exps, c, res, count, device=0, stream=None):
    """res[g] = c[g] + trgsw [x] (X^exps[g] c[g] - c[g]) with ONE selector for the launch; res may be c"""
    e = _i32(exps, count)
    check(lib.cufhe_amd_cmux_rotate_batch(device, stream, count, trgsw_ntt.ptr, _ptr(e), c.ptr, res.ptr))


def sample_extract_index_batch(trlwe, idx, tlwe1, count, src=None, device=0, stream=None):
    """tlwe1[g] = SampleExtract(idx[g])(trlwe[src[g]]) (src None: g), lvl1 TLWEs [count][N+1]"""
    j = _i32(idx, count)
    s = _i32(src, count) if src is not None else None
    check(lib.cufhe_amd_sample_extract_index_batch(device, stream, count, trlwe.ptr, _ptr(s), _ptr(j), tlwe1.ptr))


def sample_extract_index_keyswitch_batch(trlwe, idx, tlwe0, count, src=None, device=0, stream=None):
    """the same followed by the key switch: lvl0 TLWEs [count][n+1]"""
    j = _i32(idx, count)
    s = _i32(src, count) if src is not None else None
    check(lib.cufhe_amd_sample_extract_index_keyswitch_batch(device, stream, count, trlwe.ptr, _ptr(s), _ptr(j), tlwe0.ptr))


def polymul_batch(a, b, res, count, device=0, stream=None):
    check(lib.cufhe_amd_polymul_batch(device, stream, count, a.ptr, b.ptr, res.ptr))


# ---- N = 2048 ring / 64-bit torus (configs[4]); gates on lvl0 ciphertexts ----
def lvl2_params():
    p = Lvl2Params()
    check(lib.cufhe_amd_lvl2_get_params(ctypes.byref(p)))
    return p


def lvl2_initialize(bk, ksk):
    """bk: the lvl02 bootstrapping key as uint64 torus words, ksk: the lvl20 key-switching key (uint32)."""
    bk = np.ascontiguousarray(bk, dtype=np.uint64).ravel()
    ksk = np.ascontiguousarray(ksk, dtype=np.uint32).ravel()
    check(lib.cufhe_amd_lvl2_initialize(_ptr(bk), bk.size, _ptr(ksk), ksk.size))


def lvl2_gate_batch(ops, out, in0, in1=None, in2=None, count=None, device=0, stream=None):
    words = LVL_WORDS[0]
    if count is None:
        count = out.words // words
    if np.isscalar(ops):
        ops_arr, stride = np.array([ops], dtype=np.int32), 0
    else:
        ops_arr, stride = np.ascontiguousarray(ops, dtype=np.int32), 1
        assert ops_arr.size >= count
    check(lib.cufhe_amd_lvl2_gate_batch(device, stream, count, _ptr(ops_arr), stride, out.ptr, in0.ptr,
                                        in1.ptr if in1 is not None else None,
                                        in2.ptr if in2 is not None else None, words))


def lvl2_blind_rotate_batch(tlwe0, acc, count, steps=-1, device=0, stream=None):
    check(lib.cufhe_amd_lvl2_blind_rotate_batch(device, stream, count, tlwe0.ptr, acc.ptr, steps))


def lvl2_keyswitch_batch(tlwe2, tlwe0, count, device=0, stream=None):
    check(lib.cufhe_amd_lvl2_keyswitch_batch(device, stream, count, tlwe2.ptr, tlwe0.ptr))


# ---- user gates on the N = 2048 ring (cufhe_amd_lvl2_define_gate, include/cufhe_amd.h) ----
LVL2_USER_OP_BASE, LVL2_MAX_USER_GATES, LVL2_N = 8192, 64, 2048


def lvl2_user_op_output(op, j):
    """the op id of output j of multi-output lvl2 definition `op` (CUFHE_AMD_LVL2_USER_OP_OUTPUT)"""
    return op + j * LVL2_MAX_USER_GATES


def lvl2_define_gate(coeffs, offset=0, test_vector=None, nout=1):
    """A user gate of the N = 2048 ring: x = c0 in0 + c1 in1 + c2 in2 + (0, .., 0, offset) on lvl0 ciphertexts, bootstrapped through
    `test_vector` (2048 uint64 torus words; None: the constant 2^61).  Returns the op id: an op of lvl2_gate_batch, and of gate_batch /
    Apply / gApply at level 0 while "lvl0_ring" is 2048.  nout = 2, 4 or 8: a multi-output definition (interleaved test vector of
    lvl2_test_vector_multi, required); output j is the op lvl2_user_op_output(op, j)."""
    c = np.zeros(3, dtype=np.int32)
    c[:len(coeffs)] = coeffs
    tv = None
    if test_vector is not None:
        tv = np.ascontiguousarray(test_vector, dtype=np.uint64)
        if tv.size != LVL2_N:
            raise ValueError(f"test vector must have N2 = {LVL2_N} words")
    op = ctypes.c_int()
    if nout != 1:
        check(lib.cufhe_amd_lvl2_define_gate_multi(c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, int(nout),
                                                   _ptr(tv) if tv is not None else None, ctypes.byref(op)))
        return op.value
    check(lib.cufhe_amd_lvl2_define_gate(c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, _ptr(tv) if tv is not None else None,
                                         ctypes.byref(op)))
    return op.value


def lvl2_test_vector(values):
    """The 64-bit test vector of a function on len(values) messages (a power of two, 2 .. N2/2) encoded with a padding bit at level 0,
    m -> m 2^32 / (2p): values are the output torus words, uint64 (cufhe_amd_lvl2_test_vector)."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    tv = np.empty(LVL2_N, dtype=np.uint64)
    check(lib.cufhe_amd_lvl2_test_vector(_ptr(v), int(v.size), _ptr(tv)))
    return tv


def lvl2_test_vector_multi(values):
    """The interleaved 64-bit test vector of nout = len(values) functions (1, 2, 4 or 8) on p = len(values[0]) messages each,
    p nout <= N2/2 (cufhe_amd_lvl2_test_vector_multi)."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    if v.ndim != 2:
        raise ValueError("values must be [nout][p]")
    tv = np.empty(LVL2_N, dtype=np.uint64)
    check(lib.cufhe_amd_lvl2_test_vector_multi(_ptr(v), int(v.shape[1]), int(v.shape[0]), _ptr(tv)))
    return tv


def lvl2_user_rotate_batch(op, in0, acc, count, in1=None, in2=None, steps=-1, device=0, stream=None):
    """acc[count][2][N2] (uint64): the accumulator of lvl2 user gate `op` after `steps` CMux steps (parity hook)."""
    check(lib.cufhe_amd_lvl2_user_rotate_batch(device, stream, count, op, in0.ptr, in1.ptr if in1 is not None else None,
                                               in2.ptr if in2 is not None else None, steps, acc.ptr))


def lvl2_user_extract_batch(op, in0, tlwe2, count, in1=None, in2=None, device=0, stream=None):
    """tlwe2[count][N2 + 1] (uint64): lvl2 user gate `op` without its key switch -- the input form of private_keyswitch_batch."""
    check(lib.cufhe_amd_lvl2_user_extract_batch(device, stream, count, op, in0.ptr, in1.ptr if in1 is not None else None,
                                                in2.ptr if in2 is not None else None, tlwe2.ptr))


# ---- circuit bootstrapping: lvl0 TLWE -> lvl1 TRGSW (include/cufhe_amd.h) ----
def cb_params():
    p = CbParams()
    check(lib.cufhe_amd_cb_get_params(ctypes.byref(p)))
    return p


def cb_initialize(privksk):
    """privksk: the private key-switching key lvl2 -> lvl1, uint32 [2][N2 + 1][t][2^basebit - 1][k + 1][N] (2.35 GB)"""
    privksk = np.ascontiguousarray(privksk, dtype=np.uint32).ravel()
    check(lib.cufhe_amd_cb_initialize(_ptr(privksk), privksk.size))


def cb_rotate_batch(tlwe0, tlwe2, count, device=0, stream=None):
    """stage 1: tlwe0 [count][n + 1] -> tlwe2 [count][l][N2 + 1] uint64 (two words each in the DeviceBuffer)"""
    check(lib.cufhe_amd_cb_rotate_batch(device, stream, count, tlwe0.ptr, tlwe2.ptr))


def private_keyswitch_batch(tlwe2, trlwe, count, device=0, stream=None):
    """stage 2: tlwe2 [count][N2 + 1] uint64 -> trlwe [count][2][k + 1][N] uint32"""
    check(lib.cufhe_amd_private_keyswitch_batch(device, stream, count, tlwe2.ptr, trlwe.ptr))


def circuit_bootstrap_batch(tlwe0, count, trgsw=None, trgsw_ntt=None, device=0, stream=None):
    """tlwe0 [count][n + 1] -> trgsw [count][(k + 1) l][k + 1][N] torus words and / or trgsw_ntt (NTT domain, doubles)"""
    check(lib.cufhe_amd_circuit_bootstrap_batch(device, stream, count, tlwe0.ptr, trgsw.ptr if trgsw is not None else None,
                                                trgsw_ntt.ptr if trgsw_ntt is not None else None))


# ---- TLWE packing: lvl0 TLWEs -> coefficients of a lvl1 TRLWE ----
def pack_params():
    p = PackParams()
    check(lib.cufhe_amd_pack_get_params(ctypes.byref(p)))
    return p


def pack_initialize(key):
    """key: the packing key lvl0 -> TRLWE, uint32 [n][t][2^basebit - 1][k + 1][N] (123.9 MB)"""
    key = np.ascontiguousarray(key, dtype=np.uint32).ravel()
    check(lib.cufhe_amd_pack_initialize(_ptr(key), key.size))


def pack_batch(tlwe0, dst, pos, trlwe, count_in, count_out, device=0, stream=None):
    """trlwe[o] = sum over the inputs m with dst[m] = o of X^pos[m] PackKS(tlwe0[m]); tlwe0 [count_in][n + 1], trlwe [count_out][2][N]
    device buffers, dst / pos host integers"""
    d, p = _i32(dst, count_in), _i32(pos, count_in)
    check(lib.cufhe_amd_pack_batch(device, stream, count_in, tlwe0.ptr, _ptr(d), _ptr(p), count_out, trlwe.ptr))


def gPackTLWEs(out_trlwe, ins, positions, st):
    """out_trlwe (Trlwe) <- sum_m X^positions[m] PackKS(ins[m]) on device buffers: the stream is fenced first (cufhe_amd_stream_fence),
    so the call runs behind the gates recorded on it and what is recorded afterwards runs behind the call; the inputs' device buffers
    are gathered into one array by a Copy launch on the same stream."""
    count = len(ins)
    assert count == len(positions) and all(c.level == 0 for c in ins) and out_trlwe.level == 2
    dev = st.device_id()
    check(lib.cufhe_amd_stream_fence(dev, st.st()))
    gathered = DeviceBuffer(max(count, 1) * LVL_WORDS[0], dev)
    if count:
        words = LVL_WORDS[0]
        outs = (ctypes.c_void_p * count)(*[gathered.ptr + m * words * 4 for m in range(count)])
        srcs = (ctypes.c_void_p * count)(*[lib.cufhe_amd_ctxt_device_ptr(c._h, dev) for c in ins])
        ops = np.full(count, COPY, np.int32)
        check(lib.cufhe_amd_gate_list(dev, st.st(), 0, count, _ptr(ops), outs, srcs, None, None))
    pack_batch(gathered, np.zeros(count, np.int32), positions, _DevicePtr(lib.cufhe_amd_ctxt_device_ptr(out_trlwe._h, dev)), count, 1,
               device=dev, stream=st.st())
    check(lib.cufhe_amd_stream_synchronize(dev, st.st()))      # `gathered` is released on return
    gathered.free()


class _DevicePtr:
    def __init__(self, ptr):
        self.ptr = ptr


# ---- encrypted-table lookup: blind rotation from a caller's TRLWE ----
def lut_rotate_batch(tlwe0, tables, acc, count, table_count, src=None, nout=1, steps=-1, device=0, stream=None):
    """acc[g] = LutRotate(tables[src[g]], tlwe0[g], log2 nout) after `steps` CMux steps (< 0: all n): the blind rotation whose initial
    accumulator is X^bbar times the TRLWE tables[src[g]] (src None: g).  tlwe0 [count][n + 1], tables [table_count][2][N], acc
    [count][2][N] device buffers; src host integers."""
    s = _i32(src, count) if src is not None else None
    check(lib.cufhe_amd_lut_rotate_batch(device, stream, count, tlwe0.ptr, tables.ptr, table_count, _ptr(s), int(nout), int(steps), acc.ptr))


def lut_lookup_batch(tlwe0, tables, out, count, table_count, src=None, nout=1, device=0, stream=None):
    """out[g][j] = KeySwitch(SampleExtract(j)(LutRotate(tables[src[g]], tlwe0[g]))), j < nout: lvl0 TLWEs [count][nout][n + 1]"""
    s = _i32(src, count) if src is not None else None
    check(lib.cufhe_amd_lut_lookup_batch(device, stream, count, tlwe0.ptr, tables.ptr, table_count, _ptr(s), int(nout), out.ptr))


def trlwe_spread_batch(inp, out, count, stride, reps, device=0, stream=None):
    """out[g] = X^(-stride (reps // 2)) sum_{i < reps} X^(i stride) inp[g] on TRLWEs [count][2][N]; out must not overlap inp"""
    check(lib.cufhe_amd_trlwe_spread_batch(device, stream, count, inp.ptr, int(stride), int(reps), out.ptr))


def _ctxt_ptr(c, dev):
    return _DevicePtr(lib.cufhe_amd_ctxt_device_ptr(c._h, dev))


def gBlindRotateTRLWE(out_trlwe, table, addr, st, nout=1):
    """out_trlwe (Trlwe) <- LutRotate(table, addr, log2 nout) on device buffers: table a Trlwe, addr a level-0 Ctxt.  Not recorded: the
    stream is fenced first (cufhe_amd_stream_fence), so the call runs behind the gates recorded on it and what is recorded afterwards
    runs behind the call.  out_trlwe must not be table."""
    assert out_trlwe.level == 2 and table.level == 2 and addr.level == 0
    dev = st.device_id()
    check(lib.cufhe_amd_stream_fence(dev, st.st()))
    lut_rotate_batch(_ctxt_ptr(addr, dev), _ctxt_ptr(table, dev), _ctxt_ptr(out_trlwe, dev), 1, 1, nout=nout, device=dev, stream=st.st())


def gLookupTRLWE(outs, table, addr, st):
    """outs[j] (level-0 Ctxts, 1, 2, 4 or 8 of them) <- output j of the lookup of `table` (Trlwe) at the encrypted address `addr`, on
    device buffers; fenced like gBlindRotateTRLWE.  The outputs are computed into one array and scattered to the objects' device
    buffers by a Copy launch on the same stream."""
    outs = list(outs)
    nout = len(outs)
    assert table.level == 2 and addr.level == 0 and all(o.level == 0 for o in outs)
    dev = st.device_id()
    check(lib.cufhe_amd_stream_fence(dev, st.st()))
    words = LVL_WORDS[0]
    res = DeviceBuffer(max(nout, 1) * words, dev)
    lut_lookup_batch(_ctxt_ptr(addr, dev), _ctxt_ptr(table, dev), res, 1, 1, nout=nout, device=dev, stream=st.st())
    dsts = (ctypes.c_void_p * nout)(*[lib.cufhe_amd_ctxt_device_ptr(o._h, dev) for o in outs])
    srcs = (ctypes.c_void_p * nout)(*[res.ptr + j * words * 4 for j in range(nout)])
    ops = np.full(nout, COPY, np.int32)
    check(lib.cufhe_amd_gate_list(dev, st.st(), 0, nout, _ptr(ops), dsts, srcs, None, None))
    check(lib.cufhe_amd_stream_synchronize(dev, st.st()))      # `res` is released on return
    res.free()


def gSpreadTRLWE(out, inp, stride, reps, st):
    """out (Trlwe) <- Spread(inp, stride, reps) on device buffers; fenced like gBlindRotateTRLWE.  out must not be inp."""
    assert out.level == 2 and inp.level == 2
    dev = st.device_id()
    check(lib.cufhe_amd_stream_fence(dev, st.st()))
    trlwe_spread_batch(_ctxt_ptr(inp, dev), _ctxt_ptr(out, dev), 1, stride, reps, device=dev, stream=st.st())


# ---- the recorded forms: scheduler nodes like the gates (they return at once; all of one dependence level share one launch sequence) ----
LOOKUP_OP_BASE = 16384
MAX_LOOKUPS = 64


def DefineLookup(coeffs, offset=0, nout=1):
    """A lookup definition: the address x = c0 in0 + c1 in1 + (0, .., 0, offset) formed inside the rotation, and the output count
    (1, 2, 4 or 8).  Returns the op id for Lookup / gLookup (cufhe_amd_define_lookup)."""
    c = (ctypes.c_int32 * 2)(int(coeffs[0]), int(coeffs[1]) if len(coeffs) > 1 else 0)
    op = ctypes.c_int(-1)
    check(lib.cufhe_amd_define_lookup(c, int(offset) & 0xFFFFFFFF, int(nout), ctypes.byref(op)))
    return op.value


def _lookup(op, copying, outs, table, in0, in1, st):
    outs = list(outs)
    arr = (ctypes.c_void_p * max(len(outs), 1))(*[None if o is None else o._h for o in outs])
    check(lib.cufhe_amd_enqueue_lookup(st.device_id(), st.st(), int(op), 1 if copying else 0, len(outs), arr, table._h, in0._h,
                                       in1._h if in1 is not None else None))


def Lookup(outs, table, in0, in1, op, st):
    """outs[j] <- output j of the lookup `op` (DefineLookup) of `table` (Trlwe) at the address formed from in0 and in1 (None for a
    one-operand definition): recorded; operands from their host members, results delivered to the outputs' host members.  outs has the
    definition's nout entries; None requests no output j (no key switch)."""
    _lookup(op, True, outs, table, in0, in1, st)


def gLookup(outs, table, in0, in1, op, st):
    """Lookup on device buffers only, recorded like gNand."""
    _lookup(op, False, outs, table, in0, in1, st)


def gSpread(out, inp, stride, reps, st):
    """out (Trlwe) <- Spread(inp, stride, reps), recorded (stride and reps powers of two, stride * reps <= N); out must not be inp."""
    check(lib.cufhe_amd_enqueue_spread(st.device_id(), st.st(), 0, out._h, inp._h, int(stride), int(reps)))


def gLutRotate(out, table, addr, st, nout=1):
    """out (Trlwe) <- LutRotate(table, addr, log2 nout), recorded; out must not be table."""
    check(lib.cufhe_amd_enqueue_lut_rotate(st.device_id(), st.st(), 0, int(nout), out._h, table._h, addr._h))


TL_PACK = 6912


def _pack(copying, out_trlwe, ins, positions, st):
    ins = list(ins)
    count = len(ins)
    assert count == len(positions)
    arr = (ctypes.c_void_p * max(count, 1))(*[c._h for c in ins])
    p = _i32(positions, count)
    check(lib.cufhe_amd_enqueue_pack(st.device_id(), st.st(), 1 if copying else 0, out_trlwe._h, count, arr, _ptr(p)))


def gPack(out_trlwe, ins, positions, st):
    """out_trlwe (Trlwe) <- sum_m X^positions[m] PackKS(ins[m]), the words of gPackTLWEs, RECORDED: a scheduler node of len(ins) inputs
    (1 .. N; handles and positions may repeat) on device buffers.  No fence, no gather, no wait; all packs of one dependence level
    share one launch."""
    _pack(False, out_trlwe, ins, positions, st)


def Pack(out_trlwe, ins, positions, st):
    """gPack with the inputs taken from their host members and the result delivered to out_trlwe's host words (after Synchronize /
    StreamQuery)."""
    _pack(True, out_trlwe, ins, positions, st)


# ---- linear layers: an integer matrix times a vector of ciphertexts ----
class LinearLayer:
    """a layer id of cufhe_amd_linear_define with its shape; valid until CleanUp"""

    def __init__(self, layer_id, rows, cols):
        self.id, self.rows, self.cols = int(layer_id), int(rows), int(cols)


def define_linear(W, bias=None):
    """W: [rows][cols] integers that fit int32; bias: rows torus words (uint32) or None for zeros.  The weights are copied to every
    device of SetGPUNum before the call returns.  Noise (variance times sum_k W[j][k]^2) and the padding bit are the caller's concern."""
    w = np.asarray(W)
    assert w.ndim == 2 and w.size and np.issubdtype(w.dtype, np.integer)
    assert w.min() >= -(1 << 31) and w.max() < (1 << 31), "weights are int32"
    w = np.ascontiguousarray(w, dtype=np.int32)
    b = None
    if bias is not None:
        b = np.ascontiguousarray(np.asarray(bias, dtype=np.uint64) & 0xFFFFFFFF, dtype=np.uint32)
        assert b.shape == (w.shape[0],)
    layer = ctypes.c_int(-1)
    check(lib.cufhe_amd_linear_define(w.shape[0], w.shape[1], _ptr(w), _ptr(b) if b is not None else None, ctypes.byref(layer)))
    return LinearLayer(layer.value, w.shape[0], w.shape[1])


def _linear_strides(level, in_stride_words, out_stride_words):
    words = lib.cufhe_amd_ctxt_words(level) if level in (0, 1) else 1     # a bad level is rejected by the library
    return (words if in_stride_words is None else in_stride_words), (words if out_stride_words is None else out_stride_words)


def linear_batch(layer, level, out, inp, sets, device=0, stream=None, in_stride_words=None, out_stride_words=None):
    """out[s rows + j] = sum_k W[j][k] inp[s cols + k] + (0, .., 0, bias[j]) mod 2^32 on DeviceBuffers of `sets` input vectors; strides
    in words from one ciphertext to the next (default: packed).  Not recorded: Stream.fence() orders it behind recorded gates."""
    si, so = _linear_strides(level, in_stride_words, out_stride_words)
    check(lib.cufhe_amd_linear_batch(device, stream, layer.id, level, sets, inp.ptr, si, out.ptr, so))


def linear_list(layer, level, outs, ins, sets, device=0, stream=None):
    """the same on lists of device pointers (ints): ins[s cols + k], outs[s rows + j]; operands are read where they lie"""
    assert len(ins) == sets * layer.cols and len(outs) == sets * layer.rows
    a = (ctypes.c_void_p * max(len(ins), 1))(*ins)
    o = (ctypes.c_void_p * max(len(outs), 1))(*outs)
    check(lib.cufhe_amd_linear_list(device, stream, layer.id, level, sets, a, o))


def linear_gate_batch(layer, op, level, out, inp, sets, device=0, stream=None, in_stride_words=None, out_stride_words=None):
    """linear_batch into a temporary of the library, then the one-input user gate `op` (define_gate with c1 = c2 = 0, or an output id of
    such a multi-output definition) on each of the sets * rows sums: a fully connected layer with the gate's test vector as activation."""
    si, so = _linear_strides(level, in_stride_words, out_stride_words)
    check(lib.cufhe_amd_linear_gate_batch(device, stream, layer.id, int(op), level, sets, inp.ptr, si, out.ptr, so))


def polymul512_batch(a, b, res, count, device=0, stream=None):
    check(lib.cufhe_amd_polymul512_batch(device, stream, count, a.ptr, b.ptr, res.ptr))


def set_option(key, value):
    check(lib.cufhe_amd_set_option(key.encode(), int(value)))


def profile_enable(on=True, device=0):
    check(lib.cufhe_amd_profile_enable(device, 1 if on else 0))


def probe_clock(device=0):
    """Shader clock in Hz under an FP64 load, measured now (cufhe_amd_probe_clock)."""
    hz = ctypes.c_double(0.0)
    check(lib.cufhe_amd_probe_clock(device, ctypes.byref(hz)))
    return hz.value


def profile_get(device=0, reset=True):
    p = Profile()
    check(lib.cufhe_amd_profile_get(device, ctypes.byref(p), 1 if reset else 0))
    return p


def sched_stats(device=0, reset=False):
    """Counters of the per-gate API's scheduler: levels, launch sequences, copies (include/cufhe_amd.h)."""
    s = SchedStats()
    check(lib.cufhe_amd_sched_get_stats(device, ctypes.byref(s), 1 if reset else 0))
    return s


# ---- other parameter sets (include/cufhe_amd.h: cufhe_amd_ps_*) ----
def sched_trace(device=0, clear=True, max_entries=64):
    """the per-flush timeline of the per-gate API (cufhe_amd_sched_get_trace): list of dicts, oldest first"""
    buf = (_lib.GroupTrace * max_entries)()
    n = check(lib.cufhe_amd_sched_get_trace(int(device), buf, max_entries, int(bool(clear))))
    return [{f: getattr(buf[i], f) for f, _ in _lib.GroupTrace._fields_ if not f.startswith("pad")} for i in range(n)]


def ps_count():
    return lib.cufhe_amd_ps_count()


def ps_params(ps):
    p = PsParams()
    check(lib.cufhe_amd_ps_get_params(int(ps), ctypes.byref(p)))
    return p


def ps_index(name):
    for i in range(ps_count()):
        if ps_params(i).name.decode() == name:
            return i
    raise KeyError(name)


def ps_initialize(ps, bk, ksk):
    bk = np.ascontiguousarray(bk, dtype=np.uint32).ravel()
    ksk = np.ascontiguousarray(ksk, dtype=np.uint32).ravel()
    check(lib.cufhe_amd_ps_initialize(int(ps), _ptr(bk), bk.size, _ptr(ksk), ksk.size))


def ps_gate_batch(ps, ops, out, in0, in1=None, in2=None, count=None, device=0, stream=None, level=0):
    """level 0: blind rotate then key switch on n + 1 words; level 1: key switch then blind rotate on k N + 1 words"""
    words = ps_params(ps).lvl1_words if level else ps_params(ps).lvl0_words
    if count is None:
        count = out.words // words
    if np.isscalar(ops):
        ops_arr, stride = np.array([ops], dtype=np.int32), 0
    else:
        ops_arr, stride = np.ascontiguousarray(ops, dtype=np.int32), 1
        assert ops_arr.size >= count
    check(lib.cufhe_amd_ps_gate_batch_level(int(ps), device, stream, int(level), count, _ptr(ops_arr), stride, out.ptr, in0.ptr,
                                            in1.ptr if in1 is not None else None,
                                            in2.ptr if in2 is not None else None, words))


def ps_blind_rotate_batch(ps, tlwe0, acc, count, steps=-1, device=0, stream=None):
    check(lib.cufhe_amd_ps_blind_rotate_batch(int(ps), device, stream, count, tlwe0.ptr, acc.ptr, steps))


def ps_keyswitch_batch(ps, tlwe1, tlwe0, count, device=0, stream=None):
    check(lib.cufhe_amd_ps_keyswitch_batch(int(ps), device, stream, count, tlwe1.ptr, tlwe0.ptr))


def ps_trlwe_op_batch(ps, op, out, inp, count, device=0, stream=None):
    """op: TL_BOOTSTRAP (lvl0 TLWEs -> TRLWEs), TL_REFRESH (TRLWEs -> TRLWEs) or TL_SEIKS (TRLWEs -> lvl0 TLWEs), device buffers of the set's sizes"""
    check(lib.cufhe_amd_ps_trlwe_op_batch(int(ps), device, stream, int(op), count, out.ptr, inp.ptr))


# ---- user gates on a parameter set (cufhe_amd_ps_define_gate, include/cufhe_amd.h) ----
PS_USER_OP_BASE, PS_MAX_USER_GATES = 12288, 64


def ps_user_op_output(op, j):
    """the op id of output j of a set's multi-output definition `op` (CUFHE_AMD_PS_USER_OP_OUTPUT)"""
    return op + j * PS_MAX_USER_GATES


def ps_define_gate(ps, coeffs, offset=0, test_vector=None, nout=1):
    """A user gate of compiled parameter set `ps`: x = c0 in0 + c1 in1 + c2 in2 + (0, .., 0, offset) on the set's ciphertexts,
    bootstrapped through `test_vector` (N torus words of the set; None: the constant mu).  Returns the op id: an op of ps_gate_batch on
    that set at either level, and of gate_batch / Apply / gApply while "param_set" is that set.  nout = 2, 4 or 8: a multi-output
    definition (interleaved test vector of ps_test_vector_multi, required); output j is the op ps_user_op_output(op, j)."""
    c = np.zeros(3, dtype=np.int32)
    c[:len(coeffs)] = coeffs
    tv = None
    if test_vector is not None:
        tv = np.ascontiguousarray(test_vector, dtype=np.uint32)
        if tv.size != ps_params(ps).N:
            raise ValueError(f"test vector must have N = {ps_params(ps).N} words")
    op = ctypes.c_int()
    if nout != 1:
        check(lib.cufhe_amd_ps_define_gate_multi(int(ps), c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, int(nout),
                                                 _ptr(tv) if tv is not None else None, ctypes.byref(op)))
        return op.value
    check(lib.cufhe_amd_ps_define_gate(int(ps), c.ctypes.data_as(_lib.c_i32p), int(offset) & 0xFFFFFFFF, _ptr(tv) if tv is not None else None,
                                       ctypes.byref(op)))
    return op.value


def ps_test_vector(ps, values):
    """The test vector (N words of set `ps`) of a function on len(values) messages (a power of two, 2 .. N/2) encoded with a padding
    bit, m -> m 2^32 / (2p): values are the output torus words (cufhe_amd_ps_test_vector; host only)."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    tv = np.empty(ps_params(ps).N, dtype=np.uint32)
    check(lib.cufhe_amd_ps_test_vector(int(ps), _ptr(v), int(v.size), _ptr(tv)))
    return tv


def ps_test_vector_multi(ps, values):
    """The interleaved test vector of nout = len(values) functions (1, 2, 4 or 8) on p = len(values[0]) messages each, p nout <= N/2
    of set `ps` (cufhe_amd_ps_test_vector_multi; host only)."""
    v = np.ascontiguousarray(values, dtype=np.uint32)
    if v.ndim != 2:
        raise ValueError("values must be [nout][p]")
    tv = np.empty(ps_params(ps).N, dtype=np.uint32)
    check(lib.cufhe_amd_ps_test_vector_multi(int(ps), _ptr(v), int(v.shape[1]), int(v.shape[0]), _ptr(tv)))
    return tv


def ps_user_rotate(ps, op, in0, acc, count, in1=None, in2=None, steps=-1, device=0, stream=None):
    """acc[count][(k+1) N]: the accumulators of the set's user gate `op` on lvl0 operands after `steps` CMux steps (parity hook)."""
    check(lib.cufhe_amd_ps_user_rotate(int(ps), device, stream, count, int(op), in0.ptr, in1.ptr if in1 is not None else None,
                                       in2.ptr if in2 is not None else None, acc.ptr, steps))


def ps_trgsw_to_ntt_batch(ps, trgsw, trgsw_ntt, count, device=0, stream=None):
    """TRGSW2NTT on a set: trgsw[count][(k+1)l][k+1][N] torus words -> trgsw_ntt[count][limbs][(k+1)l][k+1][N] doubles (2 words each)"""
    check(lib.cufhe_amd_ps_trgsw_to_ntt_batch(int(ps), device, stream, count, trgsw.ptr, trgsw_ntt.ptr))


def ps_cmux_batch(ps, trgsw_ntt, c1, c0, res, count, device=0, stream=None):
    """CMUXNTT on a set: res = c0 + trgsw [x] (c1 - c0) on TRLWEs of (k+1) N words"""
    check(lib.cufhe_amd_ps_cmux_batch(int(ps), device, stream, count, trgsw_ntt.ptr, c1.ptr, c0.ptr, res.ptr))
