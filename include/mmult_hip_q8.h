/* mmult_hip_q8.h -- the C ABI of libmmult_hip_q8.so: the int8 linear layer (W8A8) for the AMD Instinct MI355X (gfx950).
 *
 * A second product library beside libmmult_hip.so (same tree, same flags, its own translation units under
 * how-to-optimize-gemm_amd/csrc_q8/): it needs no mmh_handle_t and links nothing of the first one.  Status codes and
 * MMH_ACT_* are mmult_hip.h's.
 *
 * What it is for.  mmh_qgemm_f32 quantises both operands per tensor on every call.  A layer's weight never changes and
 * wants one scale per output channel; its activations want one scale per row (per token).  Here the weight is prepared
 * ONCE (mmh_q8_weight_create: torch's out x in layout in, a transposed int8 image and the channel scales out), and a
 * forward is two launches: the row quantiser (one pass over x) and the int8 MFMA GEMM with dequantisation, bias and
 * ReLU in its epilogue.
 *
 * The numeric contract (tests/qlinear_ref.py restates it in numpy).  With
 *   s(v) = 127 / max|v_i| over the FINITE elements of a vector (1 when that maximum is 0, clamped to FLT_MAX when the
 *          quotient overflows) and
 *   Q(v)_i = clamp(rint(v_i * s(v)), -127, 127), round-half-even, never -128; NaN -> 0, +-inf -> +-127
 * (both are mmh_quantize_sym_s8's rules, applied per row instead of per tensor):
 *   sx[i] = s(x[i,:])           sw[j] = s(W[j,:])
 *   rx[i] = fl(1 / sx[i])       rw[j] = fl(1 / sw[j])        IEEE division; subnormal results are kept
 *   acc[i][j] = sum_k Q(x[i,:])_k * Q(W[j,:])_k              exact in int32
 *   y[i][j] = act(fl(fl(fl((float)acc[i][j] * rx[i]) * rw[j]) + bias[j]))
 *             (float)acc rounds to nearest even; the two products and the sum round once each, nothing is contracted
 *             into an fma; without a bias there is no sum; MMH_ACT_RELU is mmh_sgemm_ex's: r if (r > 0 or r is NaN)
 *             else +0.  in == 0: the formula with acc = 0.
 * Every result is a pure function of the arguments: no atomics, no dependence on grid, path or device.
 *
 * Capture.  mmh_q8_weight_create allocates: on a capturing stream it is MMH_ERR_UNSUPPORTED and nothing is done.  The
 * activations' int8 image and row scales live in scratch the weight object owns (one mmh_q8_linear at a time per object).
 * A call on a capturing stream that would have to allocate or grow that scratch is MMH_ERR_UNSUPPORTED before anything
 * is launched or touched -- make one uncaptured call at the largest size, or mmh_q8_linear_reserve, first.  Once a
 * captured call has used the scratch, growth retires the old allocation (freed with the object), never frees it under
 * the graph.
 *
 * Every entry point leaves the caller's current device as it found it.  Known gap: shapes for which mmh_igemm_s8 would
 * pick its ping-pong kernel (igemm_s8_pp_kernel) run the 256x256 tile of igemm_s8_dma_tile here. */
#ifndef MMULT_HIP_Q8_H_
#define MMULT_HIP_Q8_H_

#include "mmult_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmh_q8_weight *mmh_q8_weight_t;

/* Text of the last error / of what the last mmh_q8_linear or mmh_q8_quantize_rows launched, on this thread ("" if none). */
const char *mmh_q8_last_error(void);
const char *mmh_q8_last_launch(void);

/* Prepare a weight: dW is out x in fp32 (torch's layout), leading dimension ldw >= in, any 4-byte aligned address (16-byte
 * loads when dW is 16-byte aligned and ldw % 4 == 0 -- same bits).  The object owns the int8 image (in rows of pitch =
 * (out + 15) & ~15 bytes: image[k][j] = Q(W[j,:])_k, columns [out, pitch) are 0), sw and rw (out floats each).  The work
 * is enqueued on `stream`; dW must stay valid until it has run.  out > 0, in >= 0.  MMH_ERR_UNSUPPORTED: a capturing
 * stream, or an image beyond the GEMM's 2 GiB buffer-descriptor window ((in + 256) * pitch >= 2^31 - 4096). */
int mmh_q8_weight_create(mmh_q8_weight_t *weight, int device, int out, int in, const float *dW, int ldw, void *stream);
int mmh_q8_weight_destroy(mmh_q8_weight_t weight);   /* NULL: MMH_OK */
/* Any out-pointer may be NULL.  The device pointers stay valid for the object's life. */
int mmh_q8_weight_info(mmh_q8_weight_t weight, int *out, int *in, int *pitch, const int8_t **dQ, const float **d_scale,
                       const float **d_inv_scale);

/* The row quantiser on caller-owned buffers: dQ[i][0..cols) = Q(x[i,:]), d_scale[i] = s(x[i,:]), d_inv_scale[i] = fl(1 / s).
 * ldq >= cols and dQ holds rows * ldq bytes: the bytes [cols, min(ldq, (cols + 15) & ~15)) of every row, the last one
 * included, are written as 0.  One pass over dX.  16-byte
 * loads when dX is 16-byte aligned, ldx % 4 == 0, dQ 4-byte aligned and ldq % 4 == 0; a scalar path otherwise -- same bits.
 * rows == 0: MMH_OK, nothing launched.  cols == 0: every scale is 1, dX and dQ are neither read nor written and may be NULL. */
int mmh_q8_quantize_rows(int device, int rows, int cols, const float *dX, int ldx, int8_t *dQ, int ldq, float *d_scale,
                         float *d_inv_scale, void *stream);

/* y (rows x out, leading dimension ldy >= out) = act(x (rows x in, ldx >= in) W^T + bias) by the contract above.  dBias:
 * out floats at any 4-byte aligned address, or NULL.  activation: MMH_ACT_NONE or MMH_ACT_RELU.  rows == 0: MMH_OK. */
int mmh_q8_linear(mmh_q8_weight_t weight, int rows, const float *dX, int ldx, const float *dBias, int activation, float *dY,
                  int ldy, void *stream);
/* mmh_q8_linear on rows that are quantised already: dXq is rows x in int8 with ldq >= in, d_inv_scale rows floats -- the rx
 * of the contract, with Q(x[i,:]) the caller's row i.  With mmh_q8_quantize_rows' outputs the result is bit-equal to
 * mmh_q8_linear on the fp32 x, and one quantisation can feed any number of weights.  One launch, the GEMM of mmh_q8_linear's
 * plan straight on dXq: no quantiser pass, no scratch, no allocation -- nothing to reserve before a capture; mmh_q8_last_launch
 * reads as the part of mmh_q8_linear_plan's text after "then ".  The tile reads dXq through a buffer descriptor in dwords: an
 * ldq that is no multiple of 4, a dXq that is not 4-byte aligned, or rows beyond the 2 GiB window (256 * ldq + in >= 2^31 -
 * 4096) are MMH_ERR_UNSUPPORTED with a message, nothing launched or touched.  Bytes of a row beyond `in` need not be zero. */
int mmh_q8_linear_s8(mmh_q8_weight_t weight, int rows, const int8_t *dXq, int ldq, const float *d_inv_scale, const float *dBias,
                     int activation, float *dY, int ldy, void *stream);
/* Size the object's scratch for calls of up to max_rows rows (see Capture above). */
int mmh_q8_linear_reserve(mmh_q8_weight_t weight, int max_rows, void *stream);

/* What mmh_q8_linear does for a shape, host arithmetic only (no device, no object): text receives what
 * mmh_q8_last_launch says after the call -- the row quantiser's form and path and the GEMM's instantiation, spelled as
 * tools/kernel_resources.py demangles it, with their grids --, *scratch_bytes the scratch the call needs.  x_mod16 /
 * y_mod16: dX's and dY's addresses modulo 16; cu_count <= 0: 256.  The tile: 256x256 where mmh_igemm_s8 would choose it
 * (csrc/igemm_plan.hpp, i8_big_tile), else 128x128; the unguarded instantiation for whole tiles with 16-byte y rows. */
int mmh_q8_linear_plan(int rows, int out, int in, int ldx, int ldy, int x_mod16, int y_mod16, int has_bias, int activation,
                       int cu_count, char *text, int text_bytes, size_t *scratch_bytes);

/* Mean milliseconds per mmh_q8_linear call: warmup calls, then reps calls between one pair of events on `stream`. */
int mmh_time_q8_linear(mmh_q8_weight_t weight, int rows, const float *dX, int ldx, const float *dBias, int activation,
                       float *dY, int ldy, int warmup, int reps, void *stream, float *ms_per_call);

/* Argument errors (every entry point): a NULL object, out-pointer or operand (dW / dX, and mmh_q8_quantize_rows' dQ, may be
 * NULL where in == 0: they are not read or written), a negative size, a leading dimension below the row length, an activation outside {MMH_ACT_NONE, MMH_ACT_RELU}: MMH_ERR_INVALID_ARG, checked before any device
 * call -- nothing is launched and no output is touched. */

#ifdef __cplusplus
}
#endif
#endif /* MMULT_HIP_Q8_H_ */
