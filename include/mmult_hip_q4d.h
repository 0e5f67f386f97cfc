/* mmult_hip_q4d.h -- the C ABI of libmmult_hip_q4d.so: the small-batch linear layer (1 - 16 rows: decode) on 4-BIT WEIGHTS and
 * int8 activations (W4A8) on the AMD Instinct MI355X (gfx950).
 *
 * A fifth product library beside libmmult_hip.so, libmmult_hip_q8.so, libmmult_hip_q8o.so and libmmult_hip_q8d.so (same tree,
 * same flags, its own translation units under how-to-optimize-gemm_amd/csrc_q4d/).  It links nothing of the others and is
 * stateless like the fourth: no handle, no object, no allocation -- raw device pointers only, the images, the scales and the
 * scratch are the caller's, so a call on a capturing stream needs nothing reserved.  Status codes and MMH_ACT_* are
 * mmult_hip.h's.
 *
 * What it is for.  At 1 - 16 rows mmh_q8d_linear's cost is reading the weight once, and its footprint is the weight.  Here the
 * weight is stored at four bits per element: half the bytes streamed, half the bytes held.  gfx950 has no int4 matrix
 * instruction: q4decode_partial_kernel streams the packed nibbles as mmh_q8d_linear's partial kernel streams bytes and feeds
 * the same int8 MFMA.
 *
 * The quantisation rule (how-to-optimize-gemm_amd/csrc_q4d/quant_rules_s4.hpp; csrc/quant_rules_s8.hpp with 7 for 127), per
 * output channel j of the fp32 weight w (out, in):
 *   s4(v)  = 7 / max|v_i| over the finite elements; 1 when that maximum is 0; clamped to FLT_MAX where the quotient overflows
 *   Q4(v)_i = clamp(rint(v_i * s4), -7, 7), round-half-even; NaN -> 0, +-inf -> +-7; the library never produces -8
 *   inv_scale = fl(1 / s4)
 *
 * The packed image.  W[k][j] = Q4(w[j, :])[k] is the transposed image mmh_q8_weight_info hands out, W[k][j] = 0 for k >= in.
 * The packed image has packed_rows = 64 * ceil(in / 128) rows of pitch_n bytes (the library's own: out rounded up to 16, pad
 * columns 0); for slice s and r in 0 .. 63
 *   P[64 s + r][j] = (W[128 s + r][j] & 15) | ((W[128 s + 64 + r][j] & 15) << 4)
 * -- the low nibbles of a slice's 64 rows are its k 0 .. 63, the high nibbles its k 64 .. 127, two's complement, -8 .. 7.
 * A CALLER-MADE image obeys the same contract: every nibble whose k is >= in is ZERO (bytes of a row of dXq beyond `in` may
 * hold anything, and the kernel multiplies them with those nibbles), all packed_rows rows are there, and -8 is allowed.
 *
 * The numeric contract is INHERITED, not new.  With one scale per output channel the int32 sums are exact, so mmh_q4d_linear on
 * P is mmh_q8d_linear on the int8 image W holding the same values, bit for bit: the partial kernel leaves the true int32
 * partials in the workspace in mmh_q8d_linear's [split][row][out rounded up to 4] layout, and the finish kernel is
 * csrc_q8d/qdecode_s8.hpp's qdecode_finish_kernel, instantiated here verbatim -- the same epilogue, the same three roundings,
 * the same int8-output requantisation (mmult_hip_q8d.h states both; tests/qchain_ref.py's qlinear_s8_ref is the reference).
 *
 * The overflow bound, derived.  The kernel feeds the MFMA 16 * W (a nibble moved into a byte's high half is that byte's signed
 * value divided by 16: -8 becomes -128) and shifts the finished sum right by 4, exactly.  |x| <= 128 and |16 W| <= 128, so a K
 * range of k_len accumulates at most 2^14 * k_len in magnitude: a range must stay below 2^17 k.  The plan keeps every range at
 * or below MMH_Q4D_MAX_RANGE_K = 65536 k (2^30), raising its split count where the occupancy rule alone would give fewer; a
 * forced split count whose ranges would be longer is MMH_ERR_INVALID_ARG.
 *
 * The plan (how-to-optimize-gemm_amd/csrc_q4d/q4decode_plan.hpp) is mmh_q8d_linear's with the weight's bytes in * out / 2 in
 * the traffic cap and that ceiling.
 *
 * Every entry point leaves the caller's current device as it found it. */
#ifndef MMULT_HIP_Q4D_H_
#define MMULT_HIP_Q4D_H_

#include <stddef.h>

#include "mmult_hip.h"

#define MMH_Q4D_MAX_ROWS 16          /* one MFMA row block */
#define MMH_Q4D_MAX_RANGE_K 65536    /* the longest K range a workgroup accumulates (the overflow bound above) */

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error / of what the last mmh_q4d_linear launched, on this thread ("" if none). */
const char *mmh_q4d_last_error(void);
const char *mmh_q4d_last_launch(void);

/* The library's own layout of a packed image, host arithmetic only: pitch_n = out rounded up to 16, packed_rows =
 * 64 * ceil(in / 128), bytes = packed_rows * pitch_n.  Negative sizes or a NULL result: MMH_ERR_INVALID_ARG. */
int mmh_q4d_weight_layout(int out, int in, int *pitch_n, int *packed_rows, size_t *bytes);

/* Prepare a layer: dW is torch's (out, in) fp32 weight on the device, read in place (ldw >= in floats).  Writes the packed
 * image into dP (packed_rows rows of pitch_n bytes; pitch_n >= out and a multiple of 16, dP 16-byte aligned; every byte of
 * every row up to pitch_n is written, pad columns and nibbles of k >= in as 0), s4 of every channel into d_scale and fl(1 / s4)
 * into d_inv_scale (out floats each).  Two kernels on `stream`: the rows' abs-max, then quantise + transpose + pack.
 * out == 0: nothing is read or written; in == 0: the scales are 1, nothing else is read or written (dW, dP may be NULL). */
int mmh_q4d_pack_weight(int device, int out, int in, const float *dW, int ldw, void *dP, int pitch_n, float *d_scale,
                        float *d_inv_scale, void *stream);

/* mmh_q8d_linear with the packed image dWp for dWq (mmult_hip_q8d.h has every other argument's rule, unchanged):
 * rows in 1..16 (0: MMH_OK, nothing launched; more: MMH_ERR_UNSUPPORTED, nothing touched); dXq / ldq / d_inv_scale the int8 rows;
 * dWp / pitch_n the packed image above (pitch_n >= out, a multiple of 4, dWp 4-byte aligned); d_w_inv_scale, dBias, activation,
 * d_out_scale, dY / ldy or dYq / ldyq as there; d_work / work_bytes the caller's scratch, at least the plan's work_bytes
 * (splits * rows * (out rounded up to 4) * 4, rounded up to 16) and 16-byte aligned; splits: 0 = the plan's choice, > 0 forces
 * that many K ranges -- MMH_ERR_INVALID_ARG where a range would be empty or longer than MMH_Q4D_MAX_RANGE_K.
 * The kernel reads dXq and dWp through buffer descriptors in dwords: a pitch that is no multiple of 4, a base that is not
 * 4-byte aligned or operands beyond the 2 GiB window (256 * ldq + in or (packed_rows + 128) * pitch_n + 256 >= 2^31 - 4096) are
 * MMH_ERR_UNSUPPORTED with a message; nothing is launched or touched.  in == 0: acc = 0, dXq, dWp and d_work are not read and
 * may be NULL.  Two launches (one when in == 0), no allocation, no state between calls. */
int mmh_q4d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const void *dWp,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits, void *stream);

/* What mmh_q4d_linear launches for a shape and the workspace it needs, host arithmetic only (no device): text receives what
 * mmh_q4d_last_launch says after the call, e.g. "q4decode_partial_kernel, 32 strips x 4 splits of 1024 k;
 * qdecode_finish_kernel<false>, 64 workgroups, wide stores".  The arguments are mmh_q8d_linear_plan's (wp_mod4: dWp's address
 * modulo 4), the operands' rules mmh_q4d_linear's, with its status codes. */
int mmh_q4d_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int out8, int ldo, int xq_mod4, int wp_mod4, int o_mod16,
                        int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes);

/* Mean milliseconds per mmh_q4d_linear call: warmup calls, then reps calls between one pair of events on `stream`. */
int mmh_time_q4d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const void *dWp, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call);

/* Argument errors (every entry point) are mmh_q8d_linear's: a negative device, size or split count, out == 0 with rows > 0, a
 * NULL operand that is read, both or neither of dY / dYq (dY with d_out_scale, dYq without), a pitch below the row length, a
 * workspace that is NULL or misaligned, a forced split count with an empty or an over-long range, an activation outside
 * {MMH_ACT_NONE, MMH_ACT_RELU}; for mmh_q4d_pack_weight also ldw < in, a pitch_n below out or no multiple of 16, a dP that is not
 * 16-byte aligned: MMH_ERR_INVALID_ARG, checked before any device call -- nothing is launched and no output is touched.  A
 * workspace smaller than a forced plan's, or than one K range's: the same, before any device call; one smaller than the plan's own
 * choice (which depends on the device's CU count): MMH_ERR_INVALID_ARG before the first launch. */

#ifdef __cplusplus
}
#endif
#endif /* MMULT_HIP_Q4D_H_ */
