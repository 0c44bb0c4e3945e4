/* cufhe_amd_linear.h -- the linear layers of the C ABI.  Part of cufhe_amd.h, which includes it: include that header. */
#ifndef CUFHE_AMD_LINEAR_H
#define CUFHE_AMD_LINEAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- linear layers: an integer matrix times a vector of ciphertexts (no counterpart in the reference) ----
 * The leveled operation on TLWEs: a LAYER is rows x cols weights W[j][k] (int32, host, row-major) and rows bias words bias[j] (uint32
 * torus words; NULL: zeros).  For a level L in {0, 1}, words = cufhe_amd_ctxt_words(L), inputs x_0 .. x_{cols-1} and 0 <= i < words,
 *     y_j[i] = ( sum_k (uint32)W[j][k] x_k[i]  +  (i == words - 1 ? bias[j] : 0) )  mod 2^32,     0 <= j < rows
 * Integer arithmetic that wraps: one right answer for every input, random words included; no key.  The noise of y_j is the inputs'
 * variance times sum_k W[j][k]^2, and the message sum_k W[j][k] m_k + bias[j] must stay where the caller's encoding (its padding bit)
 * can hold it: both are the caller's concern, as the noise budget of a user gate's linear part is (section 9).
 * cufhe_amd_linear_define copies the weights to every logical device of SetGPUNum before it returns, as test vectors are, and brings
 * the devices up as cufhe_amd_initialize_ntt does: it needs SetGPUNum and a device, but no key.  *layer is an id in a table of its
 * own, CUFHE_AMD_LINEAR_LAYER_BASE + k for the k-th layer since the last cufhe_amd_cleanup (above every op id range, so that the gate
 * entry points refuse it as an unknown op): NOT an op id, no gate entry point accepts it.  Layers are immutable; cufhe_amd_cleanup
 * drops all of them and their ids count from 0 again.  -1: a null pointer (bias excepted), rows or cols outside [1, 16384], rows cols
 * > 2^26, the 65th layer.  cufhe_amd_linear_get reports a layer's shape (either pointer may be NULL); -1 for an unknown id. */
#define CUFHE_AMD_LINEAR_LAYER_BASE 20480
#define CUFHE_AMD_MAX_LINEAR_LAYERS 64
#define CUFHE_AMD_LINEAR_MAX_DIM 16384
#define CUFHE_AMD_LINEAR_MAX_WEIGHTS (1 << 26)
#define CUFHE_AMD_LINEAR_MAX_POINTERS (1 << 24)      /* sets * max(rows, cols) of one call */
int cufhe_amd_linear_define(size_t rows, size_t cols, const int32_t* weights, const uint32_t* bias, int* layer);
int cufhe_amd_linear_get(int layer, size_t* rows, size_t* cols);
/* `sets` independent input vectors on raw device arrays: input k of set s at in + (s cols + k) in_stride_words, output j of set s at
 * out + (s rows + j) out_stride_words; exactly `words` words are written per output and nothing between them.  Works under any active
 * parameter set, with the set's cufhe_amd_ctxt_words.  Not recorded by the scheduler (cufhe_amd_stream_fence orders a call behind the
 * gates recorded on its stream), like cufhe_amd_pack_batch.  Refused with -1 before any device work, outputs untouched: a null
 * pointer, an unknown (or dropped) layer, level outside {0, 1}, a stride below `words`, an output range that overlaps the input range,
 * sets max(rows, cols) > 2^24.  sets = 0 is not an error: 0, nothing done.  "cus_override" as for every launch shape (plan_linear); the
 * words do not depend on it. */
int cufhe_amd_linear_batch(int device, void* stream, int layer, int level, size_t sets, const uint32_t* in, size_t in_stride_words,
                           uint32_t* out, size_t out_stride_words);
/* The same with HOST arrays of DEVICE pointers, ins[s cols + k] and outs[s rows + j], as cufhe_amd_gate_list takes them: operands are
 * read where gates left them, no gather.  A pointer may appear several times among the inputs.  -1 also: a null entry, an output
 * pointer equal to an input pointer (of any set). */
int cufhe_amd_linear_list(int device, void* stream, int layer, int level, size_t sets, const uint32_t* const* ins, uint32_t* const* outs);
/* The layer fused in front of a one-input user gate -- an encrypted fully connected layer with an arbitrary activation.  Defined by
 * composition: the words of cufhe_amd_linear_batch into a temporary tmp[sets rows][words] (a pooled block of the stream, no allocation
 * per call), then the words of cufhe_amd_gate_batch(level, sets rows, &op, 0, out, tmp, NULL, NULL, ..) with output g at out + g
 * out_stride_words.  op is a user-gate id of the default path (cufhe_amd_define_gate) whose definition has c1 = c2 = 0, or an output id
 * CUFHE_AMD_USER_OP_OUTPUT(op, j) of such a multi-output definition; every launch-shape rule of the gate path applies unchanged.
 * -1 beside the refusals above: an op with a second or third coefficient, a built-in op or any id that is no defined user gate,
 * "param_set" active, "lvl0_ring" 2048 (at either level); -3 before cufhe_amd_initialize. */
int cufhe_amd_linear_gate_batch(int device, void* stream, int layer, int op, int level, size_t sets, const uint32_t* in, size_t in_stride_words,
                                uint32_t* out, size_t out_stride_words);

#ifdef __cplusplus
}
#endif

#endif
