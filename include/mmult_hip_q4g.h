/* mmult_hip_q4g.h -- the C ABI of libmmult_hip_q4g.so: the small-batch linear layer (1 - 16 rows: decode) on 4-BIT WEIGHTS WITH ONE
 * SCALE PER GROUP OF 128 INPUT FEATURES and int8 activations (W4A8, GPTQ / AWQ style groups) on the AMD Instinct MI355X (gfx950).
 *
 * A sixth product library beside libmmult_hip.so, libmmult_hip_q8.so, libmmult_hip_q8o.so, libmmult_hip_q8d.so and
 * libmmult_hip_q4d.so (same tree, same flags, its own translation units under how-to-optimize-gemm_amd/csrc_q4g/).  It links
 * nothing of the others and is stateless like the fourth and the fifth: no handle, no object, no allocation -- raw device pointers
 * only, the image, the scales and the scratch are the caller's, so a call on a capturing stream needs nothing reserved.  Status
 * codes and MMH_ACT_* are mmult_hip.h's.
 *
 * What it is for.  mmh_q4d_linear's weight has one scale per output channel: one outlier in a row of the weight fixes the step of
 * its other in - 1 elements, and at four bits most of them round to 0 or +-1.  Here every group of MMH_Q4G_GROUP = 128 consecutive
 * input features of a channel has its own scale: group g is k in [128 g, 128 g + 128) cut at `in`, groups = ceil(in / 128).  A
 * group is exactly one 128-k slice of the packed image, which is mmh_q4d_linear's, byte for byte.
 *
 * The quantisation rule is how-to-optimize-gemm_amd/csrc_q4d/quant_rules_s4.hpp's (scale4_of_amax, quantize4_one), unchanged,
 * applied per output channel j AND group g of the fp32 weight w (out, in):
 *   s4[g][j] = 7 / max|w[j, k]| over the group's finite elements; 1 when that maximum is 0; clamped to FLT_MAX on overflow
 *   Q4       = clamp(rint(w[j, k] * s4[g][j]), -7, 7), round-half-even; NaN -> 0, +-inf -> +-7; the library never produces -8
 *   r[g][j]  = fl(1 / s4[g][j])
 *
 * The packed image is include/mmult_hip_q4d.h's: packed_rows = 64 * ceil(in / 128) rows of pitch_n bytes (the library's own: out
 * rounded up to 16, pad columns 0), P[64 s + r][j] = (W[128 s + r][j] & 15) | ((W[128 s + 64 + r][j] & 15) << 4) -- the low
 * nibbles of a slice's 64 rows are its k 0 .. 63, the high nibbles its k 64 .. 127, two's complement.  A CALLER-MADE image obeys
 * the same contract: every nibble whose k is >= in is ZERO, all packed_rows rows are there, and -8 is allowed.
 * The scales are `groups` rows of pitch_s floats, r[g][j] at d_group_inv_scale[g * pitch_s + j] (the library's own pitch_s: out
 * rounded up to 16, pad columns 0).  A caller-made array may hold anything in its pad columns.
 *
 * THE NUMERIC CONTRACT is new: a sum of group terms is an fp32 sum, and its order is fixed here.  Row i, column j, a plan of
 * `splits` K ranges of k_len k (a multiple of 128); range p covers the groups [p k_len / 128, min((p + 1) k_len / 128, groups)).
 * Every line rounds once -- plain fp32 operators, NO fused multiply-add anywhere:
 *   S_g = sum over the group's k of xq[i][k] * W[k][j]        int32, exact; |S_g| <= 128 * 128 * 8 = 2^17: (float)S_g is exact
 *   t_g = fl((float)S_g * r[g][j])
 *   P_p = 0;  for g ascending in range p:  P_p = fl(P_p + t_g)      q4gdecode_partial_kernel; workspace [split][row][wp] fp32
 *   Z   = 0;  for p ascending:             Z   = fl(Z + P_p)        q4gdecode_finish_kernel
 *   v   = fl(Z * rx[i]);  v = fl(v + bias[j]) if bias;  ReLU: v = !(v <= 0) ? v : 0 (NaN stays)
 *   fp32 output: v.  int8 output: quantize_one(v, so[i]) as mmh_q8o_linear's (clamp(rint(fl(v * so)), -127, 127); NaN -> 0).
 * Two roundings in the epilogue where the int8 layer has three: the channel's factor lives in r[g][j].  in == 0: Z = 0, the
 * finish kernel alone.  A real group's factor of 0, a negative, a subnormal, inf or NaN follows these lines literally
 * (0 * inf = NaN).
 * THE BITS DEPEND ON THE PARTITION (splits, k_len): fp32 addition is not associative.  The partition is the plan's, and the plan
 * is host arithmetic anyone can evaluate without a device (mmh_q4g_linear_plan).  Without a forced count it depends on `rows` and
 * on the device's CU count; a caller who wants the same bits at every batch size and on every part forces `splits`.
 *
 * No range ceiling, derived.  The kernel feeds the MFMA 16 * W (a nibble moved into a byte's high half is that byte's signed
 * value divided by 16) and its int32 accumulator RESTARTS AT ZERO EVERY SLICE: |x| <= 128 and |16 W| <= 128 over 128 k is at most
 * 128 * 128 * 128 = 2^21 in magnitude, `>> 4` (arithmetic, exact: every term is a multiple of 16) gives |S_g| <= 2^17 < 2^24.
 * So MMH_Q4D_MAX_RANGE_K has no counterpart here: a range may be as long as the layer.
 *
 * The plan (how-to-optimize-gemm_amd/csrc_q4g/q4gdecode_plan.hpp) is mmh_q8d_linear's with the weight's bytes in * out / 2 in the
 * traffic cap (mmh_q4d_linear's cap) and without that library's ceiling; the workspace has the same size (fp32 partials).
 *
 * Every entry point leaves the caller's current device as it found it. */
#ifndef MMULT_HIP_Q4G_H_
#define MMULT_HIP_Q4G_H_

#include <stddef.h>

#include "mmult_hip.h"

#define MMH_Q4G_MAX_ROWS 16   /* one MFMA row block */
#define MMH_Q4G_GROUP 128     /* input features per scale: one slice of the packed image */

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error / of what the last mmh_q4g_linear launched, on this thread ("" if none). */
const char *mmh_q4g_last_error(void);
const char *mmh_q4g_last_launch(void);

/* The library's own layout, host arithmetic only: pitch_n = out rounded up to 16, packed_rows = 64 * ceil(in / 128), groups =
 * ceil(in / 128), pitch_s = out rounded up to 16 (floats), image_bytes = packed_rows * pitch_n, scale_bytes = groups * pitch_s * 4
 * (of EACH of the two scale arrays).  Negative sizes or a NULL result: MMH_ERR_INVALID_ARG. */
int mmh_q4g_weight_layout(int out, int in, int *pitch_n, int *packed_rows, int *groups, int *pitch_s, size_t *image_bytes,
                          size_t *scale_bytes);

/* Prepare a layer: dW is torch's (out, in) fp32 weight on the device, read in place (ldw >= in floats).  Writes the packed image
 * into dP (packed_rows rows of pitch_n bytes; pitch_n >= out and a multiple of 16, dP 16-byte aligned), s4[g][j] into
 * d_group_scale and fl(1 / s4[g][j]) into d_group_inv_scale (groups rows of pitch_s >= out floats each).  Every byte of every row
 * up to the pitches is written, pad columns and nibbles of k >= in as 0.  One kernel on `stream`: a workgroup holds 64 channels x
 * one slice, finds each channel's group maximum, quantises and packs.  out == 0 or in == 0: nothing is read or written (the
 * pointers may be NULL). */
int mmh_q4g_pack_weight(int device, int out, int in, const float *dW, int ldw, void *dP, int pitch_n, float *d_group_scale,
                        float *d_group_inv_scale, int pitch_s, void *stream);

/* mmh_q4d_linear with d_group_inv_scale / pitch_s in place of d_w_inv_scale (mmult_hip_q4d.h and mmult_hip_q8d.h have every other
 * argument's rule, unchanged): rows in 1..16 (0: MMH_OK, nothing launched; more: MMH_ERR_UNSUPPORTED, nothing touched); dXq / ldq /
 * d_inv_scale the int8 rows and rx; dWp / pitch_n the packed image (pitch_n >= out, a multiple of 4, dWp 4-byte aligned);
 * d_group_inv_scale / pitch_s the groups' factors r[g][j] (pitch_s >= out); dBias, activation, d_out_scale, dY / ldy or dYq / ldyq
 * as there; d_work / work_bytes the caller's scratch, at least the plan's work_bytes (splits * rows * (out rounded up to 4) * 4,
 * rounded up to 16) and 16-byte aligned; splits: 0 = the plan's choice, > 0 forces that many K ranges -- MMH_ERR_INVALID_ARG where a
 * range would be empty.
 * The partial kernel reads a lane's four factors as ONE 16-byte vector through a buffer descriptor: d_group_inv_scale must be
 * 16-BYTE ALIGNED and pitch_s a MULTIPLE OF 4 floats.  What the kernel cannot read -- that, a pitch of dXq or dWp that is no
 * multiple of 4, a base of theirs that is not 4-byte aligned, or operands beyond the 2 GiB window (256 * ldq + in,
 * (packed_rows + 128) * pitch_n + 256 or (groups + 4) * pitch_s * 4 + 1024 >= 2^31 - 4096) -- is MMH_ERR_UNSUPPORTED with a message;
 * nothing is launched or touched.  in == 0: Z = 0, dXq, dWp, d_group_inv_scale and d_work are not read and may be NULL.  Two
 * launches (one when in == 0), no allocation, no state between calls. */
int mmh_q4g_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const void *dWp,
                   int pitch_n, const float *d_group_inv_scale, int pitch_s, const float *dBias, int activation,
                   const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits,
                   void *stream);

/* What mmh_q4g_linear launches for a shape and the workspace it needs, host arithmetic only (no device): text receives what
 * mmh_q4g_last_launch says after the call, e.g. "q4gdecode_partial_kernel, 32 strips x 4 splits of 1024 k;
 * q4gdecode_finish_kernel<false>, 64 workgroups, wide stores" -- the partition (splits, k_len) the bits depend on.  The arguments
 * are mmh_q4d_linear_plan's with pitch_s behind pitch_n and gs_mod16 (d_group_inv_scale's address modulo 16) behind wp_mod4; the
 * operands' rules are mmh_q4g_linear's, with its status codes. */
int mmh_q4g_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int pitch_s, int out8, int ldo, int xq_mod4, int wp_mod4,
                        int gs_mod16, int o_mod16, int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes);

/* Mean milliseconds per mmh_q4g_linear call: warmup calls, then reps calls between one pair of events on `stream`. */
int mmh_time_q4g_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const void *dWp, int pitch_n, const float *d_group_inv_scale, int pitch_s, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call);

/* Argument errors (every entry point) are mmh_q4d_linear's: a negative device, size or split count, out == 0 with rows > 0, a
 * NULL operand that is read, both or neither of dY / dYq (dY with d_out_scale, dYq without), a pitch below the row length
 * (pitch_s < out among them), a workspace that is NULL or misaligned, a forced split count with an empty range, an activation
 * outside {MMH_ACT_NONE, MMH_ACT_RELU}; for mmh_q4g_pack_weight also ldw < in, a pitch_n below out or no multiple of 16, a dP that
 * is not 16-byte aligned: MMH_ERR_INVALID_ARG, checked before any device call -- nothing is launched and no output is touched.  A
 * workspace smaller than a forced plan's, or than one K range's: the same, before any device call; one smaller than the plan's own
 * choice (which depends on the device's CU count): MMH_ERR_INVALID_ARG before the first launch. */

#ifdef __cplusplus
}
#endif
#endif /* MMULT_HIP_Q4G_H_ */
