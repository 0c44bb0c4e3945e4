/*
 * cufhe_amd.h -- C ABI of the MI355X gate-bootstrapping engine.
 *
 * This is the drop-in boundary for the gate path of virtualsecureplatform/cuFHE: every
 * entry point below replaces one piece of the reference's host interface (file:line
 * under /root/reference cited per function).  Plain pointers and sizes only; no HIP,
 * torch or C++ types.  All functions return 0 on success and a negative code on failure
 * (cufhe_amd_last_error() gives the text); the reference aborts instead
 * (include/details/error_gpu.cuh:40-60) and the C++ shim include/cufhe_amd.hpp restores
 * that behaviour.  Codes: -1 bad argument, -2 a HIP call failed, -3 keys not initialised,
 * -5 a kernel reported through the device's fault word that its own result cannot be trusted
 * (a bounded device-side wait expired): returned by cufhe_amd_synchronize / _stream_query /
 * _stream_synchronize and by the call that makes the scheduler observe the completion,
 * sticky until cufhe_amd_cleanup; ciphertexts produced since Initialize must be discarded.
 *
 * Conventions
 *   - "device" is the reference's GPU index in [0, gpuNum) (Stream::device_id(),
 *     include/cufhe_gpu.cuh:152-189).
 *   - "stream" is an opaque hipStream_t (NULL = the device's default stream).
 *     The stream contract of every cufhe_amd_*_batch / _list entry point (tests/test_gpu_stream_contract.py): a call is asynchronous
 *     and ordered on its stream -- it may return before any of its work has run, and it runs behind everything issued on that
 *     stream before it.  HOST argument arrays (ops, exponents, src / idx, dst / pos, the pointer lists) are consumed before the
 *     call returns: the caller may overwrite or free them at once.  DEVICE operands must stay valid and unmodified until the stream
 *     has reached the call (outputs: until it has completed it).  Distinct streams are independent: each has its own workspace and
 *     temporaries in the library, streams of cufhe_amd_stream_create do not order against the NULL stream, and calls on different
 *     streams may be in flight together.  Calls on different streams may come from different threads, one stream per thread at a
 *     time; calls on one stream are issued by one thread at a time.  cufhe_amd_set_option and the Initialize / define / CleanUp
 *     calls are not meant to run beside batch calls of another thread ("br_shape" is the calling thread's own).
 *     cufhe_amd_stream_destroy completes the stream's work (no synchronise is needed first) and releases everything the library
 *     pooled for the stream: its workspace, the digit words of its matrix key switches, the temporary of
 *     cufhe_amd_linear_gate_batch.
 *   - level 0 ciphertexts are lvl0 TLWEs: n+1 = 631 uint32 words (a[0..n-1], b);
 *     level 1 ciphertexts are lvl1 TLWEs: N+1 = 1025 words (TFHEpp::TLWE<P>,
 *     include/cufhe_gpu.cuh:118).  All ciphertext pointers passed to gate functions are
 *     DEVICE pointers, as in the reference's launchers (src/bootstrap_gpu.cu:834-1292).
 *   - op codes: enum cufhe_amd_op.  For CUFHE_AMD_MUX/NMUX the operands are
 *     (in0, in1, in2) = (inc, in1, in0) of Mux(out, inc, in1, in0).
 */
#ifndef CUFHE_AMD_H
#define CUFHE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum cufhe_amd_op {
    CUFHE_AMD_NAND = 0, CUFHE_AMD_NOR, CUFHE_AMD_XNOR, CUFHE_AMD_AND, CUFHE_AMD_OR, CUFHE_AMD_XOR,
    CUFHE_AMD_ANDNY, CUFHE_AMD_ANDYN, CUFHE_AMD_ORNY, CUFHE_AMD_ORYN,
    CUFHE_AMD_MUX, CUFHE_AMD_NMUX, CUFHE_AMD_NOT, CUFHE_AMD_COPY, CUFHE_AMD_NUM_OPS
};

/* parameter set compiled into the library (TFHEpp lvl0/lvl1/lvl10 params) */
typedef struct cufhe_amd_params {
    uint32_t n, N, nbit, k, l, Bgbit, t, basebit, mu;
    uint32_t lvl0_words, lvl1_words;
    uint64_t bk_words;        /* n * (k+1)l * (k+1) * N torus words   */
    uint64_t ksk_words;       /* k N * t * 2^(basebit-1) * (n+1) words */
    uint64_t bk_ntt_bytes;    /* bytes one blind rotation reads        */
} cufhe_amd_params;
int cufhe_amd_get_params(cufhe_amd_params* out);
const char* cufhe_amd_last_error(void);

/* ---- device management: src/cufhe_gates_gpu.cu:38-65, include/cufhe_gpu.cuh:54-74 ---- */
int cufhe_amd_set_gpu_num(int gpu_num);                 /* SetGPUNum             :38 */
int cufhe_amd_get_gpu_num(void);
int cufhe_amd_device_count(void);                       /* physical GPUs visible     */
/* Which physical GPU logical device `device` is: "pci=<domain:bus:dev.fn> uuid=<hex> hip_device=<index> local_cpus=<list>"
 * (hipDeviceGetPCIBusId / hipDeviceGetUuid; local_cpus = /sys/bus/pci/devices/<pci>/local_cpulist, the CPUs the
 * device's launch worker is pinned to).  The reference has no counterpart: it addresses GPUs by index
 * (cudaSetDevice(i), include/cufhe_gpu.cuh:68-74); bench.py uses this to prove that N ranks / N logical devices
 * are N distinct GPUs (test/test_gate_gpu_multi.cc:36-93 assumes it). */
int cufhe_amd_device_identity(int device, char* buf, size_t len);
/* Compute units of logical device `device` -- the unit of every launch-shape and flush rule of this library (one grid round of the
 * blind rotation = a workgroup of 8 rotations per CU); "cus_override" (cufhe_amd_set_option) replaces it. */
int cufhe_amd_device_cus(int device);
/* hipMemGetInfo of the device: what Initialize leaves free (every key is replicated per GPU, src/bootstrap_gpu.cu:115-137) */
int cufhe_amd_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int cufhe_amd_initialize_ntt(void);                     /* Initialize()          :40 */
/* Initialize(const EvalKey&) :42-47 = InitializeNTThandlers + BootstrappingKeyToNTT
 * (src/bootstrap_gpu.cu:111-138) + KeySwitchingKeyToDevice (src/keyswitch_gpu.cu:6-16).
 * bk: host, [n][(k+1)l][k+1][N] torus words; ksk: host, [kN][t][2^(basebit-1)][n+1]. */
int cufhe_amd_initialize(const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words);
int cufhe_amd_cleanup(void);                            /* CleanUp               :49 */
int cufhe_amd_synchronize(void);                        /* Synchronize  cufhe_gpu.cuh:68-74 */

/* ---- streams: class Stream include/cufhe_gpu.cuh:152-189, StreamQuery :55-65 ---- */
int cufhe_amd_stream_create(int device, void** stream);
int cufhe_amd_stream_destroy(int device, void* stream);
int cufhe_amd_stream_query(int device, void* stream);   /* 1 = idle, 0 = busy, <0 = error */
/* cudaStreamSynchronize(st.st()) of a reference program: everything issued on `stream` -- recorded gates included -- is launched,
 * complete and delivered to the tlwehosts on return. */
int cufhe_amd_stream_synchronize(int device, void* stream);
/* What makes the raw handle mean what it means in the reference, where a gate IS enqueued on st.st() at the call
 * (src/cufhe_gates_gpu.cu:148-167): called when the handle is handed to the caller (Stream::st() of include/cufhe_amd.hpp does).
 * Everything recorded on `stream` so far is launched -- values it wrote return to the ciphertexts' own buffers (tlwedevices) first --
 * and the raw stream is made to wait for it: a hipMemcpyAsync / hipEventRecord / hipStreamSynchronize the caller issues on the handle
 * afterwards is ordered behind those gates; and from now on gates recorded on `stream` wait for what the caller has put on the raw
 * stream before them (an upload into tlwedevices, a hipStreamWaitEvent).  Host results (tlwehost) are delivered by the completion
 * calls: cufhe_amd_stream_synchronize / _stream_query / _synchronize. */
int cufhe_amd_stream_fence(int device, void* stream);

/* ---- ciphertext storage: ctxtInitialize/ctxtDelete include/cufhe_gpu.cuh:76-95,
 *      CtxtCopyH2D/D2H :193-207 ---- */
int cufhe_amd_malloc(int device, size_t bytes, void** dptr);
int cufhe_amd_free(int device, void* dptr);
int cufhe_amd_host_register(void* hptr, size_t bytes);
int cufhe_amd_host_unregister(void* hptr);
int cufhe_amd_memcpy_h2d(int device, void* stream, void* dptr, const void* hptr, size_t bytes);
int cufhe_amd_memcpy_d2h(int device, void* stream, void* hptr, const void* dptr, size_t bytes);

/* ---- gates on device-resident ciphertexts ----
 * One gate, one launch sequence on `stream`: the g-prefixed gates of
 * src/cufhe_gates_gpu.cu:160-167 etc. (NandBootstrap ... NMuxBootstrap, NotBootstrap,
 * CopyBootstrap).  in1/in2 may be NULL where the op does not read them. */
int cufhe_amd_gate(int device, void* stream, int op, int level, uint32_t* out,
                   const uint32_t* in0, const uint32_t* in1, const uint32_t* in2);
/* The native batched entry: `count` independent gates in one launch sequence.
 * ops[g * ops_stride] is the op of gate g (ops_stride 0: ops[0] for all; ops is a HOST
 * array).  Operand g of each array is at base + g * stride_words. */
int cufhe_amd_gate_batch(int device, void* stream, int level, size_t count,
                         const int32_t* ops, int ops_stride, uint32_t* out,
                         const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                         size_t stride_words);
/* Same with per-gate operand pointers (HOST arrays of DEVICE pointers): what the
 * stream scheduler of include/cufhe_amd.hpp flushes. */
int cufhe_amd_gate_list(int device, void* stream, int level, size_t count, const int32_t* ops,
                        uint32_t* const* outs, const uint32_t* const* in0s,
                        const uint32_t* const* in1s, const uint32_t* const* in2s);

/* ---- user gates: programmable bootstrapping (no counterpart in the reference) ----
 * A user gate is defined once after cufhe_amd_initialize; its op id is then accepted wherever a built-in op is: cufhe_amd_gate,
 * _gate_batch, _gate_list and _enqueue_gate (mixed freely with built-in ops).  Definition: integer coefficients (c0, c1, c2), c0 != 0,
 * a torus offset and an optional test vector TV of N = 1024 lvl1 torus words (NULL: the constant mu).  With
 *     x = c0 in0 + c1 in1 + c2 in2 + (0, ..., 0, offset)   mod 2^32, at the level of the op,
 * the gate runs the built-in two-input gate path on x -- level 0: blind rotate, SampleExtract(0), key switch; level 1: key switch,
 * blind rotate, SampleExtract(0) -- except that the accumulator starts as (0, X^bbar TV) (negacyclic; bbar = 2N - (b >> (32 - 1 - nbit))
 * as for the built-in gates) instead of (0, X^bbar mu).  So (ca, cb, 0) and offset of a built-in two-input gate with TV NULL, or an
 * all-mu TV, give that gate's words exactly.  Operands: in0 only when c1 = c2 = 0, in0 and in1 when c2 = 0, else all three (c0 in0 +
 * c1 in1 is formed first, into a temporary).
 * Op ids: CUFHE_AMD_USER_OP_BASE + k for the k-th definition since the last cufhe_amd_cleanup, k < CUFHE_AMD_MAX_USER_GATES; the
 * range overlaps neither enum cufhe_amd_op nor enum cufhe_amd_trlwe_op.  Definitions are immutable; the test vector is copied into
 * every device's table before the call returns.  cufhe_amd_cleanup drops every definition: its id is refused afterwards.
 * Refused: c0 = 0 (-1); a full table (-1); a definition while "param_set" is active (-1); before cufhe_amd_initialize (-3).  The
 * parameter-set kernels ("param_set") have no user gates, and the N = 2048 ring ("lvl0_ring" 2048) has its own
 * (cufhe_amd_lvl2_define_gate below): an op of this range there returns -1 before any device work, as does an op id in the range
 * that is not defined. */
#define CUFHE_AMD_USER_OP_BASE 1000
#define CUFHE_AMD_MAX_USER_GATES 64
int cufhe_amd_define_gate(const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector, int* op);
/* Host helper: the test vector (N words) of a function on a message space of p values, p a power of two, 2 <= p <= N/2, messages
 * encoded with a padding bit as m -> m 2^32 / (2p).  Coefficient j in the box [m N/p - N/(2p), m N/p + N/(2p)) holds values[m]; the
 * top half-box [N - N/(2p), N) holds -values[0], so that m = 0 with negative noise still gives values[0].  values: p torus words. */
int cufhe_amd_test_vector(const uint32_t* values, int p, uint32_t* tv);

/* ---- multi-output user gates: several functions of one linear combination from one blind rotation (many-LUT bootstrapping) ----
 * A definition of nout = 2^s in {2, 4, 8} outputs has coefficients and offset as above and a REQUIRED test vector TV that interleaves
 * the nout functions (cufhe_amd_test_vector_multi).  With x as above (nbit = 10) the modulus switch is rounded to multiples of 2^s:
 *     abar_i = ((a_i + 2^(30 - nbit + s)) >> (31 - nbit + s)) << s,   bbar = 2N - ((b >> (31 - nbit + s)) << s)
 * (s = 0 gives the rounding of every other gate), the accumulator starts as (0, X^bbar TV), and output j, 0 <= j < nout, is
 * SampleExtract(j) of the rotated accumulator -- out[m] = a[j - m] (m <= j), -a[N + j - m] (m > j), out[N] = b[j] -- then the key
 * switch at level 0 (level 0: rotate, extract, key switch; level 1: key switch, rotate, extract).
 * CUFHE_AMD_USER_OP_OUTPUT(op, j) is the op id of output j of definition op (output 0 is op itself; ids stay below
 * CUFHE_AMD_USER_OP_BASE + 8 CUFHE_AMD_MAX_USER_GATES).  It is an ordinary single-output op for cufhe_amd_gate, _gate_batch,
 * _gate_list and _enqueue_gate; outputs of one definition on the same operands in one call (or one dependence level of the scheduler)
 * share one rotation.  An output j >= nout, or an id of the range with no definition, is refused before any device work.
 * A definition takes one slot (and one test-vector row) of the CUFHE_AMD_MAX_USER_GATES.  Refused: nout not 2, 4 or 8, a NULL TV,
 * c0 = 0, a full table, "param_set" active (-1); before cufhe_amd_initialize (-3).  The "param_set" and N = 2048 paths refuse the ops. */
#define CUFHE_AMD_USER_OP_OUTPUT(op, j) ((op) + (j) * CUFHE_AMD_MAX_USER_GATES)
int cufhe_amd_define_gate_multi(const int32_t coeffs[3], uint32_t offset, int nout, const uint32_t* test_vector, int* op);
/* Host helper: the interleaved test vector of nout functions on p messages (as cufhe_amd_test_vector): TV[nout q + j] = values[j][m],
 * m the box of position nout q under cufhe_amd_test_vector's boxes (the top half-box holds -values[j][0]).  values: [nout][p] torus
 * words; p a power of two >= 2, nout in {1, 2, 4, 8}, p nout <= N/2.  nout = 1 gives cufhe_amd_test_vector's words. */
int cufhe_amd_test_vector_multi(const uint32_t* values, int p, int nout, uint32_t* tv);

/* ---- the reference's per-gate API on host-visible ciphertexts ----
 * template<class P> struct Ctxt (include/cufhe_gpu.cuh:102-121): `host_words` is the
 * caller-owned tlwehost storage (n+1 or N+1 words, kept alive by the caller); the handle
 * adds the per-GPU device buffers (tlwedevices).  Create after SetGPUNum. */
typedef struct cufhe_amd_ctxt cufhe_amd_ctxt;
int cufhe_amd_ctxt_create(int level, uint32_t* host_words, cufhe_amd_ctxt** out);
int cufhe_amd_ctxt_destroy(cufhe_amd_ctxt* c);
uint32_t* cufhe_amd_ctxt_device_ptr(cufhe_amd_ctxt* c, int device);   /* constant for the life of the ciphertext */
/* Nand(out, in0, in1, st) ... NMux, Not, Copy (copying != 0: src/cufhe_gates_gpu.cu:148-158,
 * inputs taken from tlwehost, result delivered to out's tlwehost) and gNand ... (copying == 0:
 * :160-167, device buffers only).  The gate is RECORDED with its data dependences; the recorded
 * program of a device is launched level by level (all gates whose operands are ready: one
 * blind-rotate + one key-switch launch per level) at Synchronize / StreamQuery / cufhe_amd_flush,
 * or as soon as a level holds two grid rounds of gates (one when the device is idle; a round = 8 gates per compute unit).  A flush of several
 * levels (a recorded netlist) may instead be scheduled gate by gate on two lanes ("sched_two_lane" below).  Stream order, output aliasing,
 * shared inputs and completion semantics are those of the reference (see cufhe_amd/csrc/sched_core.h).
 * cufhe_amd_ctxt_destroy never waits: buffers are recycled when the last recorded gate naming
 * them has retired. */
int cufhe_amd_enqueue_gate(int device, void* stream, int op, int copying, cufhe_amd_ctxt* out,
                           cufhe_amd_ctxt* in0, cufhe_amd_ctxt* in1, cufhe_amd_ctxt* in2);
/* The nout outputs of ONE evaluation of a multi-output user gate (cufhe_amd_define_gate_multi): outs[j] receives output j.  The
 * operands are resolved once, before any output is recorded; the evaluation costs one blind rotation under every schedule.  Refused
 * (-1, nothing recorded): op not a multi-output definition (output 0 id), nout not its output count, an output that is also an input,
 * two outputs that are the same handle. */
int cufhe_amd_enqueue_gate_multi(int device, void* stream, int op, int copying, int nout, cufhe_amd_ctxt* const* outs,
                                 cufhe_amd_ctxt* in0, cufhe_amd_ctxt* in1, cufhe_amd_ctxt* in2);
/* TRLWE-level operations through the same scheduler: struct cuFHETRLWElvl1 (include/cufhe_gpu.cuh:124-134) is a
 * ciphertext handle of level 2 ((k+1) N words; cufhe_amd_ctxt_create(2, ...)), and
 * gGateBootstrappingTLWE2TRLWElvl01NTT / gRefresh / gSampleExtractAndKeySwitch (src/cufhe_gates_gpu.cu:86-146;
 * copying != 0: their upload-and-fetch forms) are recorded with their dependences and launched level by level:
 * 4096 Refresh calls on 800 streams (test/test_perf.cc:63-81) become a handful of launches. */
/* CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP: `in` a lvl0 ciphertext (level 0), `out` a TRGSW holder (level 3) that receives the circuit bootstrap of
 * `in` in the NTT domain, ready as the selector of cufhe_amd_enqueue_cmux (see cufhe_amd_circuit_bootstrap_batch).  One dependence
 * level of them is one rotation, one private key-switch and one TRGSW2NTT launch.  Refused before anything is recorded: -3 without
 * cufhe_amd_cb_initialize or cufhe_amd_lvl2_initialize, -1 with "param_set" active or operands of other levels. */
enum cufhe_amd_trlwe_op { CUFHE_AMD_TL_BOOTSTRAP = 100, CUFHE_AMD_TL_REFRESH = 101, CUFHE_AMD_TL_SEIKS = 102, CUFHE_AMD_TL_CMUX = 103,
                          CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP = 104 };
int cufhe_amd_enqueue_trlwe_op(int device, void* stream, int op, int copying, cufhe_amd_ctxt* out, cufhe_amd_ctxt* in);
/* CMUXNTT(res, cs, c1, c0, st) (src/cufhe_gates_gpu.cu:68-85; kernel __CMUXNTT__ src/bootstrap_gpu.cu:197-285): res = c0 + cs [x] (c1 - c0),
 * recorded like a gate and ordered against its operands by the scheduler -- as in the reference it returns at once and the
 * result is in res.trlwehost after Synchronize() / StreamQuery(st).  `cs` is a handle of level 3 (struct cuFHETRGSWNTTlvl1,
 * include/cufhe_gpu.cuh:136-146: cufhe_amd_ctxt_create(3, trgswhost as words, ..): (k+1)l (k+1) N doubles in this library's NTT
 * domain), res / c1 / c0 are TRLWE handles (level 2).  copying != 0: operands from their host members, result delivered to
 * the host (the reference's only form); 0: device buffers only.  Needs Initialize() only, like the reference. */
int cufhe_amd_enqueue_cmux(int device, void* stream, int copying, cufhe_amd_ctxt* res, cufhe_amd_ctxt* cs,
                           cufhe_amd_ctxt* c1, cufhe_amd_ctxt* c0);
/* ---- packed ROM words, recorded forms (no counterpart in the reference; default parameter set only) ----
 * Op ids that carry a number, the way CUFHE_AMD_USER_OP_OUTPUT does.  Ranges (none overlaps enum cufhe_amd_op, enum cufhe_amd_trlwe_op
 * or the user-gate range CUFHE_AMD_USER_OP_BASE .. CUFHE_AMD_USER_OP_BASE + 8 CUFHE_AMD_MAX_USER_GATES = 1000 .. 1512; capi.hip asserts it):
 *     CUFHE_AMD_TL_SEIKS_AT(j),   0 <= j < N:   2048 .. 3071
 *     CUFHE_AMD_TL_CMUX_ROTATE(e), 0 <= e < 2N: 4096 .. 6143   (what cufhe_amd_enqueue_cmux_rotate records; not an op of _enqueue_trlwe_op)
 * CUFHE_AMD_TL_SEIKS_AT(j): an op of cufhe_amd_enqueue_trlwe_op with `in` of level 2 and `out` of level 0: __SampleExtractIndex__ at
 * index j (src/bootstrap_gpu.cu:366-381: out[m] = a[j - m] for m <= j, -a[N + j - m] for m > j, out[N] = b[j]) then the key switch.
 * CUFHE_AMD_TL_SEIKS_AT(0) gives exactly the words of CUFHE_AMD_TL_SEIKS.  An id whose index is outside [0, N) lies outside the range
 * and is refused like any unknown op (-1, nothing recorded); "param_set" active: -1. */
#define CUFHE_AMD_TL_SEIKS_AT_BASE 2048
#define CUFHE_AMD_TL_SEIKS_AT(j) (CUFHE_AMD_TL_SEIKS_AT_BASE + (j))
#define CUFHE_AMD_TL_CMUX_ROTATE_BASE 4096
#define CUFHE_AMD_TL_CMUX_ROTATE(e) (CUFHE_AMD_TL_CMUX_ROTATE_BASE + (e))
/* The rotating CMUX res = c + cs [x] (X^exponent c - c), 0 <= exponent < 2N: the words of CMUXNTT(res, cs, X^exponent c, c) -- one
 * blind-rotation step against the caller's selector -- without X^exponent c ever being stored.  Recorded like cufhe_amd_enqueue_cmux:
 * res, c TRLWE handles (level 2), cs a TRGSW holder (level 3); res may be c (the d low address bits of a packed ROM are d steps on the
 * same buffer).  Needs Initialize() only.  Refused with -1 and nothing recorded: an exponent outside [0, 2N), other levels,
 * "param_set" active. */
int cufhe_amd_enqueue_cmux_rotate(int device, void* stream, int copying, cufhe_amd_ctxt* res, cufhe_amd_ctxt* cs,
                                  cufhe_amd_ctxt* c, int exponent);
/* CtxtCopyH2D / CtxtCopyD2H (include/cufhe_gpu.cuh:193-207), ordered with the recorded gates */
int cufhe_amd_enqueue_copy(int device, void* stream, cufhe_amd_ctxt* c, int to_device);
int cufhe_amd_flush(int device);                        /* launch what is recorded, do not wait */
int cufhe_amd_sched_stream_query(int device, void* stream);  /* scheduler half of StreamQuery */
/* what the scheduler did (no reference counterpart; the reference launches per gate,
 * src/bootstrap_gpu.cu:834-1292) */
typedef struct cufhe_amd_sched_stats {
    uint64_t gates;              /* gates recorded */
    uint64_t groups;             /* flushes handed to the device */
    uint64_t levels;             /* dependence levels launched */
    uint64_t launch_sequences;   /* blind-rotate + key-switch launch pairs */
    uint64_t uploads, uploads_shared, downloads;   /* ciphertext copies; _shared = unchanged inputs not copied again */
    uint64_t forced_syncs;       /* a result had to reach tlwehost before a gate could be recorded */
    uint64_t max_level_gates;
    uint64_t cross_stream_waits; /* event dependences between flushes on different internal streams */
    uint64_t record_ns, retire_ns;  /* host time on the issuing thread: recording gates, delivering results */
    uint64_t launch_ns;             /* host time on the device's launch worker */
    uint64_t renames;               /* outputs that took a fresh device buffer ("sched_rename") */
    uint64_t worker_cpus;           /* CPUs the device's launch worker is pinned to (0: not pinned; "sched_affinity") */
    uint64_t home_copies;           /* renamed values copied back to the ciphertext's own buffer before the host could look */
    uint64_t two_lane_groups;       /* flushes scheduled gate by gate on two lanes ("sched_two_lane") ... */
    uint64_t two_lane_launches;     /* ... and the launches they were cut into */
} cufhe_amd_sched_stats;
int cufhe_amd_sched_get_stats(int device, cufhe_amd_sched_stats* out, int reset);
/* Timeline of the most recent flushes of a device (oldest first, at most 64 kept): host times are std::chrono::steady_clock
 * nanoseconds (time_since_epoch), device spans milliseconds between HIP timing events (0 unless cufhe_amd_profile_enable was
 * on; marked per phase for flushes of one dependence level, as one span otherwise).  This is what the PCIe-inclusive rate of the
 * per-gate API (enqueue -> Synchronize, test/test_util.h:29-72) is made of; the reference has no counterpart. */
typedef struct cufhe_amd_group_trace {
    uint64_t id;
    uint32_t levels, gates, stream, pad;
    uint64_t in_bytes, out_bytes;    /* ciphertext words uploaded / downloaded by this flush */
    int64_t t_queued;                /* issuing thread: handed to the device's launch worker */
    int64_t t_launch_begin;          /* worker: picked up */
    int64_t t_gather_end;            /* worker: inputs copied out of tlwehost into the pinned block */
    int64_t t_submit_end;            /* worker: everything submitted to the stream */
    int64_t t_done_seen;             /* issuing thread: completion observed */
    int64_t t_delivered;             /* issuing thread: results copied into tlwehost */
    float dev_h2d_ms, dev_body_ms, dev_d2h_ms;   /* H2D copy + scatter | gates | gather + D2H copy */
    float pad2;
} cufhe_amd_group_trace;
int cufhe_amd_sched_get_trace(int device, cufhe_amd_group_trace* out, int max, int clear);

/* ---- pieces of the path (TRLWE-level primitives and parity hooks) ----
 * BootstrapTLWE2TRLWE (src/bootstrap_gpu.cu:806-815): tlwe0[count][n+1] -> acc[count][2N]
 * after `steps` CMux steps (steps < 0: all n); also the accumulator parity hook. */
int cufhe_amd_blind_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0,
                                 uint32_t* acc, int steps);
/* Bootstrap (src/bootstrap_gpu.cu:290-301,782-788): refresh lvl0 TLWEs without a gate,
 * in[count][n+1] -> blind rotate (test vector mu = lvl1 mu) -> extract -> key switch -> out[count][n+1] */
int cufhe_amd_bootstrap_batch(int device, void* stream, size_t count, uint32_t* out, const uint32_t* in);
/* SEIandKS (src/keyswitch_gpu.cu:26-40) on already extracted lvl1 TLWEs:
 * tlwe1[count][N+1] -> tlwe0[count][n+1] */
int cufhe_amd_keyswitch_batch(int device, void* stream, size_t count, const uint32_t* tlwe1,
                              uint32_t* tlwe0);
/* SampleExtractAndKeySwitch on TRLWEs (src/cufhe_gates_gpu.cu:126-146): trlwe[count][2N] -> tlwe0 */
int cufhe_amd_sample_extract_keyswitch_batch(int device, void* stream, size_t count,
                                             const uint32_t* trlwe, uint32_t* tlwe0);
/* Refresh (src/cufhe_gates_gpu.cu:106-124, SEIandBootstrap2TRLWE src/bootstrap_gpu.cu:325-364):
 * trlwe_in[count][2N] -> sample extract -> key switch -> blind rotate -> trlwe_out[count][2N]; trlwe_out may be trlwe_in */
int cufhe_amd_refresh_batch(int device, void* stream, size_t count, const uint32_t* trlwe_in,
                            uint32_t* trlwe_out);
/* TRGSW2NTT (src/bootstrap_gpu.cu:75-94): trgsw[count][(k+1)l][k+1][N] torus words ->
 * trgsw_ntt[count][(k+1)l][k+1][N] doubles (this library's NTT domain; opaque to callers) */
int cufhe_amd_trgsw_to_ntt_batch(int device, void* stream, size_t count, const uint32_t* trgsw,
                                 double* trgsw_ntt);
/* TRGSW2NTT on host memory, as the reference's wrapper runs it (H2D, kernel, D2H on `stream`, complete on return): staging
 * comes from the stream's workspace and recycled pinned blocks -- no allocation per call.  trgsw_host: (k+1)l (k+1) N
 * torus words; trgsw_ntt_host: as many doubles. */
int cufhe_amd_trgsw_to_ntt_host(int device, void* stream, const uint32_t* trgsw_host, double* trgsw_ntt_host);
/* TRGSW2NTT on a TRGSW holder (ciphertext handle of level 3, struct cuFHETRGSWNTTlvl1): fills the holder's host words (complete
 * on return) and records their upload to the stream's device, so that both CMUXNTT forms see them -- the reference leaves the
 * result in trgswhost and trgswdevices[st.device_id()] (src/bootstrap_gpu.cu:75-94).  Ordered against recorded uses of the holder. */
int cufhe_amd_trgsw_to_ntt(int device, void* stream, const uint32_t* trgsw_host, cufhe_amd_ctxt* trgswntt);
/* CMUXNTT (src/bootstrap_gpu.cu:197-285): res = c0 + trgsw [x] (c1 - c0), TRLWEs [count][2N]; res may be c0 or c1 */
int cufhe_amd_cmux_batch(int device, void* stream, size_t count, const double* trgsw_ntt,
                         const uint32_t* c1, const uint32_t* c0, uint32_t* res);
/* ---- packed ROM words (no counterpart in the reference beyond the index form of __SampleExtractIndex__) ----
 * One TRLWE holds N / w words of w bits; the low address bits rotate the wanted word to the front, the high ones pick the TRLWE with
 * CMUXNTT, and the w bits come out as lvl0 ciphertexts.  X^e p is the negacyclic product in Z_2^32[X]/(X^N + 1), 0 <= e < 2N:
 * coefficient i of X^e p is p[i - e'] for i >= e' and -p[i - e' + N] for i < e' (e' = e mod N), all negated when e >= N.
 * Default parameter set only: with "param_set" active every entry below returns -1 before any device work.  exps / src / idx are HOST
 * arrays, staged through the stream's workspace (no allocation per call); a value out of range returns -1 before any device work.
 * out[g] = X^(exps[g]) in[g] on both polynomials of TRLWEs [count][2N].  out must not overlap in (-1).  Needs no key. */
int cufhe_amd_trlwe_rotate_batch(int device, void* stream, size_t count, const uint32_t* in, const int32_t* exps, uint32_t* out);
/* The rotating CMUX: res[g] = c[g] + trgsw [x] (X^(exps[g]) c[g] - c[g]), TRLWEs [count][2N]: the words of cufhe_amd_cmux_batch with
 * c1 = X^e c and c0 = c, the rotated operand never written to memory.  ONE selector serves the launch: trgsw_ntt is a single TRGSW
 * ((k+1)l (k+1) N doubles from cufhe_amd_trgsw_to_ntt_batch), not one per item as in cufhe_amd_cmux_batch -- an address bit acts on
 * every TRLWE of a table.  res may be c.  Needs Initialize() only (the NTT tables), like cufhe_amd_cmux_batch. */
int cufhe_amd_cmux_rotate_batch(int device, void* stream, size_t count, const double* trgsw_ntt, const int32_t* exps,
                                const uint32_t* c, uint32_t* res);
/* __SampleExtractIndex__<P,index> (src/bootstrap_gpu.cu:366-381) at a caller's index: tlwe1[g] = SampleExtract(idx[g])(trlwe[src[g]]),
 * lvl1 TLWEs [count][N+1] with out[m] = a[j - m] (m <= j), -a[N + j - m] (m > j), out[N] = b[j]; 0 <= idx[g] < N.  src may be NULL
 * (src[g] = g); several outputs may name one source.  src[g] must index a TRLWE of the caller's array: the ABI carries no length, so
 * this is the caller's contract (a negative src[g] is refused).  The second form adds the key switch (SEIandKS,
 * src/keyswitch_gpu.cu:26-40): tlwe0[count][n+1]; with idx all 0 and src NULL it is cufhe_amd_sample_extract_keyswitch_batch.  Only the
 * second form uses the lvl1 -> lvl0 key: -3 before cufhe_amd_initialize. */
int cufhe_amd_sample_extract_index_batch(int device, void* stream, size_t count, const uint32_t* trlwe, const int32_t* src,
                                         const int32_t* idx, uint32_t* tlwe1);
int cufhe_amd_sample_extract_index_keyswitch_batch(int device, void* stream, size_t count, const uint32_t* trlwe, const int32_t* src,
                                                   const int32_t* idx, uint32_t* tlwe0);
/* NTT product check of test/test_polynomial_mult_1024.cu: res = a * b negacyclic mod 2^32,
 * a signed with |a| <= 128 (exactness bound of the field), all [count][N], device. */
int cufhe_amd_polymul_batch(int device, void* stream, size_t count, const int32_t* a,
                            const uint32_t* b, uint32_t* res);
/* the same check for the 512-point transform (SmallForwardNTT_512 / SmallInverseNTT_512,
 * include/ntt_gpu/ntt_gpuntt.cuh:283-329): res = a * b mod (X^512 + 1, 2^32), operands [count][512] */
int cufhe_amd_polymul512_batch(int device, void* stream, size_t count, const int32_t* a,
                               const uint32_t* b, uint32_t* res);

/* ---- tuning ----
 * "device_base": physical HIP device that logical device 0 maps to (default 0).  A process
 * that drives one GPU of a node (one rank per GPU) sets it to its local rank before Initialize.
 * Launch shape of the blind rotation (all variants produce identical words; the rules are in units of the device's CU count,
 * the numbers below are MI355X's 256 CUs).  A launch is cut into whole
 * rounds of the batch kernel's grid (2048 rotations: two per SIMD, highest throughput) plus a tail, and the
 * tail -- or a whole small launch -- takes the cheapest kernel by measured cost: up to 256 rotations (one per CU) the 16-wave
 * workgroup-per-rotation kernel with split transforms (lowest latency: 2.8 ms for one, 2.9 for 64, 3.3 for 256); up to
 * 1536 rounds of 512 on its two-rotations-per-workgroup form (5.2 ms each) plus a last round of up to 256 on the
 * single form; above that a full round (20.7 ms).  "ll2_threshold" (default -1 = by cost; 0 = never; n = for every
 * launch up to n) governs the paired form; "ll_threshold" / "half_threshold" (default -1 = by cost) force the single
 * form / the batch kernel with one rotation per SIMD up to the given count, "tail_split" 0 launches everything above
 * one round as one grid.
 * "ks_split_threshold" (default -1 = by measured cost: 32 on 256 CUs): up to that many ciphertexts per launch each key
 * switch is split over 8 workgroups (0.05 ms); above, the ciphertexts of a workgroup share each step of the key in LDS
 * (keyswitch_kernel): "ks_per_wg" ciphertexts per workgroup (1..16) and the 1024 steps of j cut into "ks_slices" runs (a
 * power of two up to 64, partial sums meeting in the output through atomics), both -1 = the cheapest shape by a model of
 * the measured times: 0.07 ms for 64, 0.12 for 256, 0.31 for 1024, 0.57 for 2048, 0.86 for 3072, 1.04 ms for 4096.
 * "ks_wg_threshold" (default -1 = never) forces one workgroup per ciphertext up to the given count (0.22 ms up to 256,
 * 0.8 ms at 1024).  All variants produce identical words.
 * "ks_mm_threshold": ciphertexts per launch from which the lvl10 key switch runs as an exact int8 matrix product on the
 * matrix cores (keyswitch_mm_kernel; the key is kept a second time in matrix form, 42 MB per device): -1 (default) = the
 * measured rule, 0 = never, n > 0 = from n ciphertexts on.  It applies only while the four "ks_*" options above are at -1,
 * and not to the N = 2048 ring or the parameter sets.  The same words as every other variant.
 * "ps_batch_threshold" (default -1 = by cost: 1025, 1281 for N = 512, 1537 for sets with key limbs): rotations per launch from which the parameter-set path
 * (cufhe_amd_ps_*) uses the wave-per-rotation kernel instead of a workgroup per rotation.
 * "lvl0_ring": 1024 (default) or 2048 -- the ring through which gates on lvl0 ciphertexts
 * bootstrap: lvl01/lvl10 (cufhe_amd_initialize) or lvl02/lvl20 (cufhe_amd_lvl2_initialize).  With 2048
 * every level-0 entry point (cufhe_amd_gate*, the recorded per-gate API, Nand<lvl0param>() ... in
 * the C++ shim) runs through the N = 2048 path.
 * "lvl2_kernel" (default -1 = by measured cost): blind-rotate kernel of the N = 2048 ring: 1 = four quarter-transform waves per rotation with
 * register sums, two rotations per CU (launches above one rotation per CU); 0 = eight half-transform waves, one rotation per CU.
 * "param_set" (default -1; "lvl0_param_set" is the same option under its old name): index of a cufhe_amd_ps_* parameter set on
 * which the whole per-gate API runs instead -- both ciphertext levels and both gate orders, and the three bootstrapping TRLWE-level
 * operations of cufhe_amd_enqueue_trlwe_op, CMUXNTT and TRGSW2NTT (cufhe_amd_enqueue_cmux / cufhe_amd_trgsw_to_ntt; not on the
 * small-modulus set, as in the reference), as the set chosen when the reference is built serves every entry point
 * (CMakeLists.txt:8-24); cufhe_amd_ps_initialize first (cufhe_amd_initialize_params does both).  Ciphertexts then have the set's sizes
 * (cufhe_amd_ctxt_words: n + 1 and k N + 1 words; include/cufhe_amd.hpp selects the matching parameter structs with
 * -DCUFHE_AMD_PARAM_SET_K2N512 / -DCUFHE_AMD_PARAM_SET_CGGI16 / -DCUFHE_AMD_PARAM_SET_SMALLMOD).  Changing it waits for everything
 * recorded; a ciphertext keeps the host buffer of the set it was created under, and using it while a set with other sizes is active is
 * refused (-1).
 * "share_devices" (default 0): 1 lets SetGPUNum(G) exceed the visible GPU count, logical devices wrapping around the
 * physical ones (every logical device keeps its own key replica, scheduler, launch thread and streams): the
 * reference's multi-GPU programs (test/test_gate_gpu_multi.cc) rehearsed on fewer GPUs.
 * "sched_streams" (default 4): internal HIP streams per device over which independent flushes of the
 * per-gate API overlap; "sched_threads" (default 1): one launch worker thread per device (0: launches
 * happen on the issuing thread).  Both before the first ciphertext is created.
 * "sched_rename" (default 1): an output whose device buffer still has recorded users (an earlier write,
 * readers of the old value) takes a fresh buffer instead of being ordered after them, so that only true data
 * dependences order a recorded program: a temporary re-used down a ripple-carry chain no longer serialises the
 * independent gates of the adders (16-bit adders: 64 dependence levels become 33).  The buffer a ciphertext was created
 * with (cufhe_amd_ctxt_device_ptr at construction = Ctxt::tlwedevices[i], include/cufhe_gpu.cuh:80-84) stays its home: a
 * value still in a renamed buffer when the caller asks for completion (Synchronize, StreamQuery of the stream that wrote
 * it) is copied home by one Copy gate in the flush that request triggers, so the published pointer holds the value
 * whenever the host may look -- results, tlwehost, tlwedevices and every API call behave as with 0 (never rename).
 * "sched_idle_gates" (default -1 = one grid round): gates of a level at which an IDLE device is handed it (never more than "sched_level_gates").
 * (Two rounds -- one flush and one key-switch launch for a burst of 4096 gates -- was measured and is no faster: the device then starts
 * 0.7 ms later, which is what the second key-switch launch costs.)
 * "sched_copy_threads" (default 4; before the first flush): host threads, the calling one included, that share the two copies on a flush's
 * latency path once it moves 1024 ciphertexts or more -- inputs out of the tlwehosts into the pinned staging block (launch worker) and
 * results back into the tlwehosts (issuing thread): 4096 NANDs' 10 MB of inputs are gathered in 0.2 ms instead of 0.7.
 * "sched_two_lane" (default 1): a flush of several dependence levels (a recorded netlist) is scheduled GATE BY GATE instead of level by
 * level when the library's cost model says that is faster: the gates on long dependence chains run as steps of the paired low-latency
 * kernel on half of the compute units while the gates nothing waits for run as chunks of the batch kernel on the other half, on two
 * internal streams (256 sixteen-bit ripple-carry adders, 32 carry levels of 256 gates behind one level of 8192: see DESIGN.md 2a).
 * Needs "sched_rename" (the recorded program is kept single-assignment); results, completion rules and tlwedevices do not change.
 * 0 = never, 2 = whenever a flush is eligible, whatever the cost model says (tests).
 * "cb_rotations" (default 3): lvl02 rotations per circuit bootstrap -- 3 = one per TRGSW row with constant test vectors, 1 = all l rows
 * from one multi-output rotation (see circuit bootstrapping below; other values -1).  Changing it waits for everything recorded.
 * "br_shape" (of the calling thread; default 0 = the launch-shape rules above): 1 / 2 / 3 put every blind rotation of the thread's
 * launches on the batch kernel / the paired low-latency kernel / the single one -- what the two lanes use, and tools/two_lane_probe.py.
 * "sched_level_gates" (default -1 = two grid rounds of the device, 16 gates per CU, while it has work -- on MI355X 4096: 32 768 gates through
 * the per-gate API 96.1 k -> 99.4 k gates/s --, one round when it is idle) / "sched_total_gates" (default 32768): a dependence level this
 * full is launched at once / bound on the recorded program.
 * "test_fail_alloc" n (default -1 = off): the (n+1)-th device allocation of an Initialize entry point fails like an exhausted device,
 * once -- a test hook for the error paths (the keys that were loaded stay loaded and usable, nothing leaks).
 * "cus_override" (default 0 = the device's own count): every launch-shape rule above and the scheduler's flush rules behave as on a
 * device with that many compute units (a partitioned device, another chip); results do not depend on it.
 * "sched_zero_copy" (default 1): the batched ciphertext traffic of a flush is read and written by the scatter / gather kernels
 * directly in pinned host memory, the inputs of a flush's first level chunk by chunk while the rest is still being gathered
 * from the tlwehosts; 0 = one H2D / D2H copy per flush through device staging buffers (the round-3 path).
 * "sched_affinity" (default 1): the launch worker thread of a device runs on the CPUs local to that GPU
 * (local_cpulist of its PCI function, intersected with the CPUs the process may use); 0 leaves it to the OS. */
int cufhe_amd_set_option(const char* key, long value);

/* ---- N = 2048 ring, 64-bit torus (BASELINE.json configs[4]; lvl2 / lvl02 / lvl20) ----
 * The reference has no N = 2048 path (its NTT is `if constexpr (N == 1024) ... else if
 * (N == 512)`, include/ntt_gpu/ntt_gpuntt.cuh, and its prime has no 4096-th root); these entry
 * points are what its gate templates compute when instantiated at brP = lvl02, iksP = lvl20:
 * __HomGate__ br -> iks (src/bootstrap_gpu.cu:402-421), the Mux of :515-588, Accumulate
 * (include/gatebootstrapping_gpu.cuh:115-285) and KeySwitchFromTLWE (include/keyswitch_gpu.cuh:
 * 83-134, 64-bit domain, 32-bit target).  Gates take and return lvl0 ciphertexts. */
typedef struct cufhe_amd_lvl2_params {
    uint32_t n, N, nbit, k, l, Bgbit, t, basebit;
    uint32_t lvl0_words, lvl2_words;   /* lvl2 TLWE: N + 1 uint64 words */
    uint64_t mu;                       /* 2^61 */
    uint64_t bk_words;                 /* n * (k+1)l * (k+1) * N uint64 words */
    uint64_t ksk_words;                /* k N * t * 2^(basebit-1) * (n+1) uint32 words */
    uint64_t bk_ntt_bytes;             /* bytes one blind rotation reads */
} cufhe_amd_lvl2_params;
int cufhe_amd_lvl2_get_params(cufhe_amd_lvl2_params* out);
/* bk: host, [n][(k+1)l][k+1][N] uint64 torus words (TRGSW of the lvl0 key bits under the lvl2
 * key); ksk: host, [kN][t][2^(basebit-1)][n+1] uint32.  Independent of cufhe_amd_initialize. */
int cufhe_amd_lvl2_initialize(const uint64_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words);
/* same contract as cufhe_amd_gate_batch at level 0 */
int cufhe_amd_lvl2_gate_batch(int device, void* stream, size_t count, const int32_t* ops, int ops_stride,
                              uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                              size_t stride_words);
/* tlwe0[count][n+1] -> acc[count][2N] (uint64) after `steps` CMux steps (< 0: all n) */
int cufhe_amd_lvl2_blind_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0,
                                      uint64_t* acc, int steps);
/* tlwe2[count][N+1] (uint64) -> tlwe0[count][n+1] */
int cufhe_amd_lvl2_keyswitch_batch(int device, void* stream, size_t count, const uint64_t* tlwe2,
                                   uint32_t* tlwe0);

/* ---- user gates on the N = 2048 ring: programmable bootstrapping with 64-bit test vectors ----
 * The ring has definitions of its own in an op-id range of its own; an op of cufhe_amd_define_gate stays refused on this ring.
 * A lvl2 user gate is defined after cufhe_amd_lvl2_initialize: integer coefficients (c0, c1, c2), c0 != 0, a 32-bit torus offset and an
 * optional test vector TV of N2 = 2048 uint64 torus words (NULL: the constant 2^61).  With lvl0 ciphertexts in0, in1, in2 and
 *     x = c0 in0 + c1 in1 + c2 in2 + (0, ..., 0, offset)   mod 2^32
 * the gate is the ring's two-input gate path on x -- lvl02 blind rotation, SampleExtract(0), lvl20 key switch -- except that the
 * accumulator starts as (0, X^bbar TV) instead of (0, X^bbar mu): bbar = 2 N2 - (b >> (32 - 1 - 11)) as for the built-in gates,
 * coefficient e reads TV[(e - bbar) mod N2], negated where (e < bbar mod N2) xor (bbar >= N2); bbar = 2 N2 is the identity and negates
 * nothing.  So (ca, cb, 0) and offset of a built-in two-input gate with TV NULL, or an all-2^61 TV, give that gate's words exactly.
 * Operands as cufhe_amd_define_gate: in0 only when c1 = c2 = 0, in0 and in1 when c2 = 0, else all three (c0 in0 + c1 in1 is formed
 * first, into a temporary).
 * Op ids: CUFHE_AMD_LVL2_USER_OP_BASE + k for the k-th definition since the last cufhe_amd_cleanup, k < CUFHE_AMD_LVL2_MAX_USER_GATES.
 * The range 8192 .. 8255 lies above every other id range (enum cufhe_amd_op, enum cufhe_amd_trlwe_op, the user gates 1000 .. 1511,
 * CUFHE_AMD_TL_SEIKS_AT 2048 .. 3071, CUFHE_AMD_TL_CMUX_ROTATE 4096 .. 6143; capi.hip asserts it).  Definitions are immutable; the test
 * vector is copied into every device's table ([64][2048] uint64, 1 MB, allocated with the first definition) before the call returns.
 * cufhe_amd_cleanup drops every definition.  Refused: c0 = 0, a full table, a null op, "param_set" active (-1); before
 * cufhe_amd_lvl2_initialize (-3).
 * Accepted, mixed freely with built-in ops: cufhe_amd_lvl2_gate_batch; and with "lvl0_ring" 2048 at level 0: cufhe_amd_gate,
 * _gate_batch, _gate_list, _enqueue_gate.  Refused with -1 before any device work: a lvl2 op on the default ring, at level 1 or with
 * "param_set" active; an id of the range without a definition; cufhe_amd_enqueue_gate_multi with a lvl2 op.
 * Not built: a level-1 form (the ring has no lvl1 gates), tables that are themselves ciphertexts (the ring has no counterpart of
 * cufhe_amd_lut_lookup_batch), cufhe_amd_enqueue_gate_multi and two-lane planning for the ring's multi-output definitions. */
#define CUFHE_AMD_LVL2_USER_OP_BASE 8192
#define CUFHE_AMD_LVL2_MAX_USER_GATES 64
int cufhe_amd_lvl2_define_gate(const int32_t coeffs[3], uint32_t offset, const uint64_t* test_vector, int* op);
/* Multi-output definitions of the ring: nout = 2^s in {2, 4, 8} functions of one x from ONE blind rotation.
 * The modulus switch rounds to multiples of 2^s (nbit = 11):
 *     abar_i = ((a_i + 2^(19+s)) >> (20+s)) << s,     bbar = 2 N2 - (((b + offset) >> (20+s)) << s)
 * and the rotation leaves nout lvl2 TLWEs, output j = SampleExtract(j) of the accumulator (a, b):
 *     out_j[m] = a[j - m] for m <= j,   out_j[m] = -a[N2 + j - m] for m > j,   out_j[N2] = b[j],
 * each with a lvl20 key switch of its own.  The test vector interleaves the functions, TV[nout q + j] = f_j at position nout q
 * (cufhe_amd_lvl2_test_vector_multi), and is required.  Every other rule is cufhe_amd_lvl2_define_gate's; a definition takes one of the
 * 64 slots.  Output j of definition `op` is the op id CUFHE_AMD_LVL2_USER_OP_OUTPUT(op, j) = op + 64 j (ids 8192 .. 8703), an ordinary
 * gate wherever lvl2 user gates are accepted; outputs of one definition on the same operand pointers in one call (one level's launch
 * of the recorded API) share the rotation, in any order, and the words never depend on that.  Refused with -1 before any device work:
 * an output id with j >= nout or on an undefined slot; nout outside {2, 4, 8}; a NULL test vector.  cufhe_amd_enqueue_gate_multi
 * stays refused for ops of this ring.  cufhe_amd_lvl2_user_rotate_batch takes output 0's id (the one accumulator);
 * cufhe_amd_lvl2_user_extract_batch takes any output id and writes that output alone (one rotation per call). */
#define CUFHE_AMD_LVL2_USER_OP_OUTPUT(op, j) ((op) + (j) * CUFHE_AMD_LVL2_MAX_USER_GATES)
int cufhe_amd_lvl2_define_gate_multi(const int32_t coeffs[3], uint32_t offset, int nout, const uint64_t* test_vector, int* op);
/* Host helper: TV[nout q + j] = values[j][m], m the box of position nout q under cufhe_amd_lvl2_test_vector's boxes; the top half-box
 * holds -values[j][0].  values: [nout][p] words; p and nout powers of two, p >= 2, nout <= 8, p nout <= N2/2; nout = 1 is
 * cufhe_amd_lvl2_test_vector. */
int cufhe_amd_lvl2_test_vector_multi(const uint64_t* values, int p, int nout, uint64_t* tv);
/* Host helper: the boxes of cufhe_amd_test_vector on N2 = 2048 coefficients with 64-bit values: coefficient j in
 * [m N2/p - N2/(2p), m N2/p + N2/(2p)) holds values[m], the top half-box [N2 - N2/(2p), N2) holds -values[0].  p a power of two,
 * 2 <= p <= N2/2; lvl0 messages encoded as m -> m 2^32 / (2p).  values: p words, tv: N2 words. */
int cufhe_amd_lvl2_test_vector(const uint64_t* values, int p, uint64_t* tv);
/* Parity hook: in0 / in1 / in2 [count][n+1] device arrays (in1 / in2 NULL where the definition's arity does not read them);
 * acc[count][2][N2] (uint64) is the accumulator of definition `op` after `steps` CMux steps (outside [0, n]: all n, as
 * cufhe_amd_lvl2_blind_rotate_batch). */
int cufhe_amd_lvl2_user_rotate_batch(int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1,
                                     const uint32_t* in2, int steps, uint64_t* acc);
/* The gate without its key switch: tlwe2[count][N2+1] (uint64) = SampleExtract(0) of the full rotation.  This is the high-precision
 * output (64-bit torus, l = 4, Bgbit = 9) and the input form of cufhe_amd_private_keyswitch_batch and cufhe_amd_lvl2_keyswitch_batch. */
int cufhe_amd_lvl2_user_extract_batch(int device, void* stream, size_t count, int op, const uint32_t* in0, const uint32_t* in1,
                                      const uint32_t* in2, uint64_t* tlwe2);

/* ---- circuit bootstrapping (CGGI17 section 4, TFHEpp's CircuitBootstrapping): lvl0 TLWE -> lvl1 TRGSW ----
 * For each input c and r = 0 .. l-1:
 *   tlwe2_r = SampleExtract(0) of the lvl02 blind rotation of c with the constant test vector mu_r = 2^(63 - (r+1) Bgbit), + mu_r on b
 *             (message bit * 2^(64 - (r+1) Bgbit));
 *   row c' l + r of the TRGSW = PrivKS_c'(tlwe2_r), c' = 0, 1, where with abar_i = tlwe2[i] + 2^(64 - t basebit - 1) (i = 0 .. N2,
 *   i = N2 the b word) and a_ij = (abar_i >> (64 - (j+1) basebit)) & (2^basebit - 1):
 *             PrivKS_u(tlwe2) = 0 - sum_i sum_j [a_ij != 0] K[u][i][j][a_ij - 1]   (word-wise mod 2^32, both polynomials).
 * The TRGSW is [(k+1) l][k+1][N] uint32 -- the layout of cufhe_amd_trgsw_to_ntt_batch -- under the default lvl1 key.
 * K is the caller's private key-switching key, TFHEpp's layout [2][N2 + 1][t][2^basebit - 1][k+1][N] uint32 (2.35 GB):
 * K[u][i][j][v-1] = TRLWE_s1(v * k2_i * 2^(32 - (j+1) basebit) * f_u), k2_i = s2[i] (i < N2), k2_N2 = -1, f_0 = -s1(X), f_1 = 1.
 * Every word is deterministic (integer arithmetic only).  Needs cufhe_amd_lvl2_initialize (the lvl02 key) and cufhe_amd_cb_initialize;
 * default parameter set only ("param_set" active: -1).
 * The one-rotation form, cufhe_amd_set_option("cb_rotations", 1) (3, the default: the above; anything else -1; switching synchronises
 * first), takes all l rows of an input from ONE rotation: the rotation of a multi-output definition with
 * s = 2 from the library's test vector TVcb[4 q + r] = 2^(63 - (r+1) Bgbit) for r < l, TVcb[4 q + 3] = 0, and
 *   tlwe2_r = SampleExtract(r) of that accumulator, + mu_r on b (the same message bit * 2^(64 - (r+1) Bgbit)).
 * Layout, private key switch, TRGSW2NTT, refusals and keys are unchanged; the option is honoured by cufhe_amd_cb_rotate_batch,
 * cufhe_amd_circuit_bootstrap_batch and the recorded CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP. */
typedef struct cufhe_amd_cb_params {
    uint32_t n, N, k, l, Bgbit;        /* output TRGSW: lvl1, l = 3, Bgbit = 6 */
    uint32_t N2, l2, Bgbit2;           /* the lvl02 rotation */
    uint32_t t, basebit;               /* private key switching lvl2 -> lvl1: t = 10, basebit = 3 */
    uint32_t lvl0_words, lvl2_words;   /* n + 1 uint32; N2 + 1 uint64 */
    uint32_t trgsw_words;              /* (k+1) l (k+1) N uint32 */
    uint32_t trgsw_ntt_doubles;        /* the same TRGSW in the NTT domain (a level-3 holder's words / 2) */
    uint64_t privksk_words;            /* 2 (N2 + 1) t (2^basebit - 1) (k+1) N uint32 */
} cufhe_amd_cb_params;
int cufhe_amd_cb_get_params(cufhe_amd_cb_params* out);
/* privksk: host words as above, copied to every device of SetGPUNum (build first, swap last: a failure leaves the keys loaded before) */
int cufhe_amd_cb_initialize(const uint32_t* privksk, size_t words);
/* stage 1: tlwe0[count][n+1] -> tlwe2[count][l][N2+1] (uint64, device), mu_r and the b offset applied */
int cufhe_amd_cb_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint64_t* tlwe2);
/* stage 2: tlwe2[count][N2+1] -> trlwe[count][2][k+1][N] (uint32, device): PrivKS_0 then PrivKS_1 of each input (no cufhe_amd_lvl2_initialize needed) */
int cufhe_amd_private_keyswitch_batch(int device, void* stream, size_t count, const uint64_t* tlwe2, uint32_t* trlwe);
/* both stages: tlwe0[count][n+1] -> trgsw[count][(k+1) l][k+1][N] torus words (may be NULL) and / or trgsw_ntt[count][trgsw_ntt_doubles]
 * (may be NULL): the words cufhe_amd_trgsw_to_ntt_batch makes of trgsw */
int cufhe_amd_circuit_bootstrap_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, uint32_t* trgsw, double* trgsw_ntt);

/* ---- TLWE packing: lvl0 ciphertexts into coefficients of a lvl1 TRLWE (no counterpart in the reference) ----
 * The way back from gate results to a packed word: the packed TRLWE can be the data operand of cufhe_amd_cmux_batch / _cmux_rotate_batch
 * (a RAM write, a table built on the device).  One exact table-sum key switch with a rotation at write-out, integer arithmetic mod 2^32
 * only.  With abar_i = a_i + 2^15 and a_ij = (abar_i >> (32 - 2 (j+1))) & 3 (t = 8 unsigned digits of basebit = 2: the library's own
 * numbers, reported by cufhe_amd_pack_get_params) for a lvl0 TLWE x = (a_0 .. a_{n-1}, b):
 *     PackKS(x) = (0, b X^0) - sum_i sum_j [a_ij != 0] K[i][j][a_ij - 1]                  a TRLWE [2][N], the a polynomial first
 *     out[o]    = sum over the inputs m with dst[m] = o of X^pos[m] PackKS(in[m])          X^e: the negacyclic product of section 11
 * An output no input names is the zero TRLWE; inputs at the same position of the same output add; all count_out outputs are written.
 * K is the caller's key, [n][t][2^basebit - 1][k+1][N] uint32 (30 965 760 words, 123.9 MB, on every device of SetGPUNum):
 * K[i][j][v-1] = TRLWE_s1(v * s0_i * 2^(32 - 2 (j+1))), a constant message, phase b - a s.  The library does not generate it.
 * Default parameter set only ("param_set" active: -1).  cufhe_amd_pack_batch works on raw device arrays and is not recorded
 * (cufhe_amd_stream_fence orders a call behind the gates recorded on its stream); cufhe_amd_enqueue_pack below is the recorded form on
 * ciphertext handles. */
typedef struct cufhe_amd_pack_params {
    uint32_t n, N;                     /* input lvl0 dimension, output ring */
    uint32_t t, basebit;               /* 8 unsigned digits of 2 bits */
    uint64_t key_words;                /* n t (2^basebit - 1) (k+1) N uint32 */
} cufhe_amd_pack_params;
int cufhe_amd_pack_get_params(cufhe_amd_pack_params* out);
/* key: host words as above, copied to every device of SetGPUNum through pinned chunks (build first, swap last: a failure leaves the key
 * loaded before in use).  -1: null pointer, wrong size, "param_set" active. */
int cufhe_amd_pack_initialize(const uint32_t* key, size_t words);
/* tlwe0[count_in][n+1] and trlwe[count_out][2][N] on the device; dst and pos HOST arrays of count_in entries (staged through the stream's
 * workspace like the exponents of section 11).  Refused before any device work: -1 for a null pointer, dst outside [0, count_out),
 * pos outside [0, N) or "param_set" active; -3 without cufhe_amd_pack_initialize.  "pack_slices" (cufhe_amd_set_option, default -1 =
 * by the rule of plan_pack) forces the number of slices the lvl0 words are cut into; the words do not depend on the shape. */
int cufhe_amd_pack_batch(int device, void* stream, size_t count_in, const uint32_t* tlwe0, const int32_t* dst, const int32_t* pos,
                         size_t count_out, uint32_t* trlwe);
/* The recorded form: a scheduler node of count_in inputs, an operation of the TRLWE kind like CUFHE_AMD_TL_REFRESH with the single id
 * CUFHE_AMD_TL_PACK (between CUFHE_AMD_TL_LUT_ROTATE 6656 .. 6659 and the lvl2 user gates 8192 ..).
 *     out = sum_m X^pos[m] PackKS(ins[m]),   0 <= m < count_in
 * word for word what cufhe_amd_pack_batch gives with count_out = 1 and dst all 0.  out is a TRLWE handle (level 2), every ins[m] a lvl0
 * handle (level 0), 1 <= count_in <= N; a handle may appear several times and positions may repeat (the terms add).  The call returns
 * at once; the scheduler orders the node behind the producers of ALL its inputs and behind the readers and the writer of out, a later
 * gate that overwrites an input is renamed or placed behind the node, and all recorded packs of one dependence level are lowered
 * together: one zeroing launch and one key-switch launch over the concatenation of their terms, reading the inputs where they lie
 * ("pack_slices" and "cus_override" as above).  copying != 0: the inputs come from their host members, the result goes to out's host
 * words (visible after Synchronize / StreamQuery); 0: device buffers only.  ins and pos are read during the call.  -1, nothing recorded:
 * a null pointer, count_in outside [1, N], pos[m] outside [0, N), wrong levels, a destroyed input, a ciphertext created under another
 * parameter set, "param_set" active; -3 when this device has no packing key.  Independent of "lvl0_ring". */
#define CUFHE_AMD_TL_PACK 6912
int cufhe_amd_enqueue_pack(int device, void* stream, int copying, cufhe_amd_ctxt* out, size_t count_in, cufhe_amd_ctxt* const* ins,
                           const int32_t* pos);

/* ---- encrypted-table lookup: blind rotation from a caller's TRLWE (no counterpart in the reference) ----
 * The blind rotation of the gates reads a PLAINTEXT table: its accumulator starts as (0, X^bbar TV).  Here it starts from a ciphertext:
 * for a TRLWE T = (A, B) ([2][N], the a polynomial first), a lvl0 TLWE x and nout = 2^s outputs,
 *     abar_i = ms_abar(x_i, s), bbar = ms_bbar(x_n, s)                      the roundings of section 9.1 (s = 0: the gates' own)
 *     acc_0 = (X^bbar A, X^bbar B)                                          the negacyclic product of section 11 on both polynomials
 *     acc_{i+1} = CMux(BK_i, X^abar_i acc_i, acc_i),  i < steps             the unchanged steps of the gates' rotation
 *     LutRotate(T, x, s) = acc_steps;   LutLookup output j = KeySwitch(SampleExtract(j)(acc_n)),  0 <= j < nout
 * so a table (0, TV) gives the words of a user gate defined on TV with coefficients (1, 0, 0) and offset 0 (nout > 1: of the
 * multi-output definition), and a table built on the device -- gates, cufhe_amd_pack_batch, cufhe_amd_trlwe_spread_batch -- is read by an
 * encrypted index in ONE rotation.  Every word is exact and independent of the launch shape.  tables[table_count][2][N], tlwe0 and the
 * outputs are device arrays; src is a HOST array of count entries (staged through the stream's workspace like the exponents of section
 * 11; NULL: src[g] = g), rotation g reads tables[src[g]] and several rotations may name one table.  Refused before any device work: -1
 * for a null pointer (src excepted), nout not 1, 2, 4 or 8, src[g] outside [0, table_count), table_count = 0 with count > 0, an output
 * array overlapping tables, or "param_set" active; -3 without cufhe_amd_initialize.  Default parameter set only; the N = 2048 ring and
 * the parameter sets have none of this.  These batch calls are not recorded (cufhe_amd_stream_fence orders one behind the gates recorded
 * on its stream) and take one address ciphertext per item; the recorded forms below -- cufhe_amd_enqueue_lookup, _enqueue_spread,
 * _enqueue_lut_rotate -- are scheduler nodes, and a lookup definition forms the address from two ciphertexts inside the rotation.  No key
 * generation. */
/* acc[count][2][N]: LutRotate after `steps` CMux steps (outside [0, n]: all n, as in cufhe_amd_blind_rotate_batch) */
int cufhe_amd_lut_rotate_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, const uint32_t* tables, size_t table_count,
                               const int32_t* src, int nout, int steps, uint32_t* acc);
/* tlwe0_out[count][nout][n+1]: all nout outputs of every item, from one rotation launch sequence and one key-switch launch (the path of
 * the multi-output gates at level 0) */
int cufhe_amd_lut_lookup_batch(int device, void* stream, size_t count, const uint32_t* tlwe0, const uint32_t* tables, size_t table_count,
                               const int32_t* src, int nout, uint32_t* tlwe0_out);
/* Spread (no key, needs no cufhe_amd_initialize): out[g] = X^(-stride floor(reps/2)) sum_{i < reps} X^(i stride) in[g] on both
 * polynomials of TRLWEs [count][2][N], mod 2^32, negacyclic.  It turns a packed TRLWE into a table whose entries fill boxes: values[m]
 * at coefficient m N / p with stride = 1, reps = N / p gives, for a trivial (0, .), cufhe_amd_test_vector(values, p) word for word (the
 * top half box holding -values[0] included); values[j][m] at m N / p + j with stride = nout, reps = N / (p nout) gives
 * cufhe_amd_test_vector_multi.  -1: a null pointer, stride < 1, reps < 1, stride * reps > N, out overlapping in, "param_set" active. */
int cufhe_amd_trlwe_spread_batch(int device, void* stream, size_t count, const uint32_t* in, int stride, int reps, uint32_t* out);

/* ---- recorded forms of the above: lookups, Spread and the table rotation as scheduler nodes ----
 * The three operations recorded like gates on ciphertext handles (cufhe_amd_ctxt_create: lvl0 ciphertexts of level 0, TRLWEs of level
 * 2): every call returns at once, the scheduler orders it by its operands and all recorded lookups, rotations and Spreads of one
 * dependence level are lowered together -- one rotation launch sequence, one key-switch launch, one Spread launch per level, whatever
 * their number and whichever streams they were issued on.  Default parameter set only: with "param_set" active every entry returns -1
 * and records nothing.
 *
 * A lookup DEFINITION is the linear part of the address and the output count: with x = c0 in0 + c1 in1 + (0, ..., 0, offset) mod 2^32
 * on lvl0 ciphertexts (c0 != 0; in1 is used only when c1 != 0),
 *     output j of Lookup(def, table, in0, in1) = LutLookup output j of (table, x, s = log2 nout),   0 <= j < nout,
 * the sum formed inside the rotation (no bootstrap of its own).  Coefficients (1, 0) and offset 0 give the words of
 * cufhe_amd_lut_lookup_batch.  Ids: CUFHE_AMD_LOOKUP_OP_BASE + k for the k-th definition since the last cufhe_amd_cleanup, k <
 * CUFHE_AMD_MAX_LOOKUPS; output j of a definition is CUFHE_AMD_LOOKUP_OP_OUTPUT(op, j), so the range is 16384 .. 16895, above every
 * other id range (lut.inc.h asserts it).  Definitions are immutable and hold no device data.  -1: c0 = 0, nout not 1, 2, 4 or 8, the
 * 65th definition, a null pointer, "param_set" active; -3 before cufhe_amd_initialize.  The ids are ops of cufhe_amd_enqueue_lookup
 * ONLY: cufhe_amd_gate, _gate_batch, _gate_list and _enqueue_gate refuse them as unknown ops. */
#define CUFHE_AMD_LOOKUP_OP_BASE 16384
#define CUFHE_AMD_MAX_LOOKUPS 64
#define CUFHE_AMD_LOOKUP_OP_OUTPUT(op, j) ((op) + (j) * CUFHE_AMD_MAX_LOOKUPS)
int cufhe_amd_define_lookup(const int32_t coeffs[2], uint32_t offset, int nout /* 1, 2, 4, 8 */, int* op);
/* The nout outputs of ONE evaluation (one rotation), recorded as one group in one dependence level: outs[j] receives output j.  outs,
 * in0, in1 have level 0, table level 2.  copying != 0: in0, in1 and table come from their host members, results go to the outputs' host
 * members (visible after Synchronize / StreamQuery); 0: device buffers only.  nout = 1: the output may be an address operand (the rotation
 * reads before the key switch writes); nout > 1: no output may be an operand.  outs[j] == NULL requests no output j: the evaluation
 * costs its one rotation and one key switch per REQUESTED output, and several calls on the same (op, in0, in1, table) in one dependence
 * level -- in any order of their outputs -- are still one rotation; at least one output must be requested.  -1, nothing recorded: op not a defined lookup (its
 * output-0 id), nout not the definition's, wrong levels, in1 missing when c1 != 0, two outputs the same handle, a ciphertext created
 * under another parameter set, "param_set" active, the N = 2048 ring ("lvl0_ring"); -3 without cufhe_amd_initialize. */
int cufhe_amd_enqueue_lookup(int device, void* stream, int op, int copying, int nout, cufhe_amd_ctxt* const* outs,
                             cufhe_amd_ctxt* table, cufhe_amd_ctxt* in0, cufhe_amd_ctxt* in1);
/* Recorded Spread and recorded table rotation, operations of the TRLWE kind like CUFHE_AMD_TL_REFRESH.  Their ids carry their numbers:
 * stride = 2^a, reps = 2^b, a + b <= 10 (every test-vector shape of cufhe_amd_test_vector[_multi]); other pairs stay on the batch call.
 *     CUFHE_AMD_TL_SPREAD(a, b):   6400 .. 6560       CUFHE_AMD_TL_LUT_ROTATE(s), s = log2 nout:   6656 .. 6659
 * (between CUFHE_AMD_TL_CMUX_ROTATE 4096 .. 6143 and the lvl2 user gates 8192 ..).
 * enqueue_spread: out = Spread(in) on TRLWE handles; needs no key.  -1: out == in, stride or reps not a power of two, stride reps > N.
 * enqueue_lut_rotate: out = LutRotate(table, addr, log2 nout) after all n steps; out and table of level 2, addr of level 0.  -1: out ==
 * table, nout not 1, 2, 4 or 8; -3 without keys.
 * Neither depends on "lvl0_ring": Spread has no key, and the rotation reads its lvl0 address with the N = 1024 key whichever ring the
 * gates use (as cufhe_amd_lut_rotate_batch does); only the lookup, whose OUTPUTS are lvl0 ciphertexts of the gates' path, is refused there.
 * The scheduler orders a writer strictly behind every recorded reader of its buffer and never renames TRLWE buffers, so out == in and
 * out == table -- an operation reading the buffer it writes -- are the only aliasing rules. */
#define CUFHE_AMD_TL_SPREAD_BASE 6400
#define CUFHE_AMD_TL_SPREAD(a, b) (CUFHE_AMD_TL_SPREAD_BASE + 16 * (a) + (b))
#define CUFHE_AMD_TL_LUT_ROTATE_BASE 6656
#define CUFHE_AMD_TL_LUT_ROTATE(s) (CUFHE_AMD_TL_LUT_ROTATE_BASE + (s))        /* s = log2 nout, 0..3 */
int cufhe_amd_enqueue_spread(int device, void* stream, int copying, cufhe_amd_ctxt* out, cufhe_amd_ctxt* in, int stride, int reps);
int cufhe_amd_enqueue_lut_rotate(int device, void* stream, int copying, int nout, cufhe_amd_ctxt* out, cufhe_amd_ctxt* table, cufhe_amd_ctxt* addr);

/* ---- linear layers: an integer matrix times a vector of ciphertexts ----
 * cufhe_amd_linear_define, _linear_get, _linear_batch, _linear_list and _linear_gate_batch: declared and documented in
 * cufhe_amd_linear.h, which this header includes. */
#include "cufhe_amd_linear.h"

/* ---- other parameter sets (CMakeLists.txt:8-24: USE_80BIT_SECURITY / USE_CGGI19 / USE_CONCRETE select TFHEpp
 * parameter headers at build time; k > 1: src/bootstrap_gpu.cu:402-421; N = 512: include/ntt_gpu/ntt_gpuntt.cuh:283-329)
 * Every set of cufhe_amd/csrc/kernels_ps.hip.h is compiled in and chosen by index: 0 = the default set (the same
 * numbers as cufhe_amd_get_params, computed by the generic kernels), 1 = "k2n512" (k = 2 over the N = 512 ring),
 * 2 = "cggi16" (the original TFHE 80-bit set; its external product exceeds the exact range of the FP64 field, so
 * the key is taken in two 16-bit limbs), 3 = "smallmod" (the default numbers through the reference's optional small NTT modulus,
 * CMakeLists.txt:12 -DUSE_SMALL_NTT_MODULUS, include/ntt_gpu/ntt_small_modulus.cuh: the bootstrapping key and every CMux increment are
 * switched between the 2^32 and the P = 625 * 2^20 + 1 discretisation of the torus -- approximate by design, word-for-word the
 * reference's arithmetic).  The numeric parameters of TFHEpp's headers are not in the reference tree
 * (SURVEY.md F3): a set is what cufhe_amd_ps_get_params reports.  Gates take and return ciphertexts of the set at
 * either level (n + 1 or k N + 1 words), keys use TFHEpp's layouts with the set's dimensions. */
typedef struct cufhe_amd_ps_params {
    char name[32];
    uint32_t n, N, nbit, k, l, Bgbit, t, basebit, key_limbs, key_limb_bits, mu;
    uint32_t lvl0_words, lvl1_words;
    uint32_t small_ntt_modulus;     /* 0: exact products; P: the set runs the reference's -DUSE_SMALL_NTT_MODULUS arithmetic mod P */
    uint64_t bk_words, ksk_words, bk_ntt_bytes;
} cufhe_amd_ps_params;
/* The numbers a caller was compiled with (TFHEpp's lvl0param::n; lvl1param::nbit, k, l, Bgbit; lvl10param::t, basebit) and whether it
 * was built with the reference's -DUSE_SMALL_NTT_MODULUS (then small_ntt_modulus = 625 * 2^20 + 1, else 0).
 * cufhe_amd_find_param_set: index of the compiled set with exactly these numbers, or -1 (text names the numbers).
 * cufhe_amd_initialize_params: Initialize(const EvalKey&) (src/cufhe_gates_gpu.cu:42-47) with the reference's single selector -- the
 * set is FOUND from the numbers, its keys are loaded on every device and the whole per-gate API runs on it (set 0 takes the
 * hand-scheduled kernels of cufhe_amd_initialize, the others cufhe_amd_ps_initialize + "param_set").  A caller whose Bgbit, t or
 * basebit differ from every compiled set is refused here instead of being served by kernels of other numbers that happen to have
 * keys of the same size.  include/cufhe_amd.hpp calls nothing else, and derives the same match at compile time. */
typedef struct cufhe_amd_param_numbers {
    uint32_t n, nbit, k, l, Bgbit, t, basebit, small_ntt_modulus;
} cufhe_amd_param_numbers;
int cufhe_amd_find_param_set(const cufhe_amd_param_numbers* numbers);
int cufhe_amd_initialize_params(const cufhe_amd_param_numbers* numbers, const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words);
int cufhe_amd_ps_count(void);
int cufhe_amd_ps_get_params(int set, cufhe_amd_ps_params* out);
int cufhe_amd_ps_initialize(int set, const uint32_t* bk, size_t bk_words, const uint32_t* ksk, size_t ksk_words);
/* words of a level-0 / level-1 ciphertext, (level 2) of a TRLWE or (level 3) of a TRGSW holder in the NTT domain (uint32 words: two per
 * double; the active set's key limbs included), of the per-gate API as configured now ("param_set") */
int cufhe_amd_ctxt_words(int level);
/* the same gates on ciphertexts of `level`: 0 = blind rotate then key switch on n + 1 words, 1 = key switch then blind rotate on
 * k N + 1 words (the reference's two __HomGate__ orders, src/bootstrap_gpu.cu:383-421, Mux :515-588 / :706-780) */
int cufhe_amd_ps_gate_batch_level(int set, int device, void* stream, int level, size_t count, const int32_t* ops, int ops_stride,
                                  uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, size_t stride_words);
/* same contract as cufhe_amd_gate_batch at level 0 */
int cufhe_amd_ps_gate_batch(int set, int device, void* stream, size_t count, const int32_t* ops, int ops_stride,
                            uint32_t* out, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2,
                            size_t stride_words);
/* tlwe0[count][n+1] -> acc[count][(k+1)N] after `steps` CMux steps (< 0: all n) */
int cufhe_amd_ps_blind_rotate_batch(int set, int device, void* stream, size_t count, const uint32_t* tlwe0,
                                    uint32_t* acc, int steps);
/* tlwe1[count][kN+1] -> tlwe0[count][n+1] */
int cufhe_amd_ps_keyswitch_batch(int set, int device, void* stream, size_t count, const uint32_t* tlwe1,
                                 uint32_t* tlwe0);
/* TRGSW2NTT / CMUXNTT on a set, device-resident (src/bootstrap_gpu.cu:75-94,197-285: in the reference the set chosen at build time
 * serves them too; the small-modulus set has none, :73-95): trgsw[count][(k+1)l][k+1][N] torus words -> trgsw_ntt[count][key_limbs]
 * [(k+1)l][k+1][N] doubles (cufhe_amd_ctxt_words(3) / 2 per TRGSW while the set is active); res = c0 + trgsw [x] (c1 - c0) on TRLWEs
 * [count][(k+1)N], res may be c0 or c1.  Need Initialize() only, like the reference. */
int cufhe_amd_ps_trgsw_to_ntt_batch(int set, int device, void* stream, size_t count, const uint32_t* trgsw, double* trgsw_ntt);
int cufhe_amd_ps_cmux_batch(int set, int device, void* stream, size_t count, const double* trgsw_ntt, const uint32_t* c1,
                            const uint32_t* c0, uint32_t* res);
/* the bootstrapping TRLWE-level operations on a set, device-resident: op = CUFHE_AMD_TL_BOOTSTRAP (in: tlwe0[count][n+1], out:
 * trlwe[count][(k+1)N]; BootstrapTLWE2TRLWE, src/bootstrap_gpu.cu:806-815), CUFHE_AMD_TL_REFRESH (trlwe -> trlwe; :325-364) or
 * CUFHE_AMD_TL_SEIKS (trlwe -> tlwe0; SEIandKS, src/keyswitch_gpu.cu:26-40) */
int cufhe_amd_ps_trlwe_op_batch(int set, int device, void* stream, int op, size_t count, uint32_t* out, const uint32_t* in);

/* ---- user gates on a parameter set: programmable bootstrapping with the set's n, N, k ----
 * cufhe_amd_define_gate word for word, over compiled set `set`: a definition is the linear part x = c0 in0 + c1 in1 + c2 in2 +
 * (0, .., 0, offset) on ciphertexts of the set (c0 != 0; c2 != 0: three operands, else c1 != 0: two, else one) and a test vector of
 * N torus words of THAT set (NULL: the constant mu = 2^29, the built-in gates' rotation).  Level 0 is blind rotate from
 * (0, .., 0, X^bbar TV) -> SampleExtract -> key switch on n + 1 words, level 1 key switch -> blind rotate -> SampleExtract on k N + 1
 * words, both with the roundings of the set's built-in gates.  The op id returned is CUFHE_AMD_PS_USER_OP_BASE + k for the k-th
 * definition since the last cufhe_amd_cleanup, over ALL sets together (k < CUFHE_AMD_PS_MAX_USER_GATES): an op of
 * cufhe_amd_ps_gate_batch[_level] on that set, mixed freely with the built-in ops (still one rotation launch per level), and of
 * cufhe_amd_gate / _gate_batch / _gate_list / _enqueue_gate while "param_set" is that set.  Definitions are immutable; cufhe_amd_cleanup
 * drops them.  A definition's test vector is copied to every logical device before the id is returned.
 * Refused with -1: c0 = 0, a null pointer, the 65th definition, an unknown set; with -3: a set that cufhe_amd_ps_initialize has not
 * loaded on every logical device.  An op of this range is refused (-1, a message naming parameter sets, before any device work) on the
 * default path, on the N = 2048 ring, on a set other than its own, and when it names no definition.  The ids of cufhe_amd_define_gate
 * and cufhe_amd_lvl2_define_gate keep their meaning and stay refused on a set.
 * On `smallmod` the accumulator holds torus words between CMux steps, so the same initial accumulator serves; the results are the
 * small-modulus path's (approximate by design, deterministic), as for its built-in gates. */
#define CUFHE_AMD_PS_USER_OP_BASE 12288      /* 12288 .. 12799: above CUFHE_AMD_TL_CMUX_ROTATE(2N - 1) = 6143 and the lvl2 range 8192 .. 8703 */
#define CUFHE_AMD_PS_MAX_USER_GATES 64
int cufhe_amd_ps_define_gate(int set, const int32_t coeffs[3], uint32_t offset, const uint32_t* test_vector /* N of the set, or NULL */, int* op);
/* Multi-output (cufhe_amd_define_gate_multi on the set): nout = 2, 4 or 8 functions from one rotation.  The modulus switch is rounded
 * to multiples of nout, the test vector is the interleaved one of cufhe_amd_ps_test_vector_multi and is required; output j is
 * SampleExtract at index j of the one accumulator and has the op id CUFHE_AMD_PS_USER_OP_OUTPUT(op, j) = op + 64 j.  Outputs of one
 * definition on the same operands in one list (or one flush of the scheduler) share the rotation, whatever their order; requesting
 * only some of them is allowed.  cufhe_amd_enqueue_gate_multi refuses these ids: record each output with cufhe_amd_enqueue_gate. */
#define CUFHE_AMD_PS_USER_OP_OUTPUT(op, j) ((op) + (j) * CUFHE_AMD_PS_MAX_USER_GATES)
int cufhe_amd_ps_define_gate_multi(int set, const int32_t coeffs[3], uint32_t offset, int nout /* 2, 4, 8 */, const uint32_t* test_vector, int* op);
/* Host only (no device, no keys): the boxes of cufhe_amd_test_vector[_multi] with the set's N.  values[p] (multi: values[nout][p]) are
 * the output torus words of messages m = 0 .. p - 1 encoded as m 2^32 / (2p) with a padding bit; coefficient j lies in the box of
 * m = round(j p / N), the top half-box is -values[0].  p a power of two, 2 <= p <= N/2; multi: nout in {1, 2, 4, 8}, p nout <= N/2. */
int cufhe_amd_ps_test_vector(int set, const uint32_t* values, int p, uint32_t* tv);
int cufhe_amd_ps_test_vector_multi(int set, const uint32_t* values, int p, int nout, uint32_t* tv);
/* Parity hook (the counterpart of cufhe_amd_lvl2_user_rotate_batch): in0/in1/in2[count][n + 1] lvl0 operands (as many as the
 * definition's arity; the others may be NULL) -> acc[count][(k+1) N], the accumulators of definition `op` (a multi-output definition:
 * output 0's id) after `steps` CMux steps (negative: all n), so that the first steps can be checked word for word. */
int cufhe_amd_ps_user_rotate(int set, int device, void* stream, size_t count, int op,
                             const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, uint32_t* acc, int steps);

/* ---- measurement ----
 * When enabled, every blind-rotate / key-switch launch is bracketed by HIP events on the
 * stream it runs on; get_profile synchronises and returns accumulated kernel time.
 * Circuit bootstrapping counts in the same fields: its lvl02 rotations as blind rotations (3 per input), its private key-switch
 * launches as key-switch launches with one key switch per lvl2 TLWE (3 per input).  To split a workload that mixes gates with
 * circuit bootstraps, profile the two in separate intervals (tools/cb_times.py profiles circuit bootstraps alone). */
typedef struct cufhe_amd_profile {
    double blind_rotate_ms; uint64_t blind_rotate_launches; uint64_t blind_rotations;
    double keyswitch_ms;    uint64_t keyswitch_launches;    uint64_t keyswitches;
} cufhe_amd_profile;
int cufhe_amd_profile_enable(int device, int on);
int cufhe_amd_profile_get(int device, cufhe_amd_profile* out, int reset);
/* Shader clock (Hz) the device holds under an FP64 load, measured now by a short calibration kernel (shader cycles over
 * the constant 100 MHz counter, median over all waves).  Measurement aid: no counterpart in the reference. */
int cufhe_amd_probe_clock(int device, double* hz);

#ifdef __cplusplus
}
#endif
#endif
