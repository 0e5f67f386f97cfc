/* mmult_hip_q8d.h -- the C ABI of libmmult_hip_q8d.so: the int8 linear layer for SMALL BATCHES (1 - 16 rows: decode) on the AMD
 * Instinct MI355X (gfx950).
 *
 * A fourth product library beside libmmult_hip.so, libmmult_hip_q8.so and libmmult_hip_q8o.so (same tree, same flags, its own
 * translation units under how-to-optimize-gemm_amd/csrc_q8d/).  It links nothing of the others and is stateless: no handle, no
 * object, no allocation -- raw device pointers only, the scratch is the caller's, so a call on a capturing stream needs nothing
 * reserved.  Status codes and MMH_ACT_* are mmult_hip.h's.
 *
 * What it is for.  The other two int8 libraries run 128x128 and 256x256 tiles: at 16 rows a tile does a full tile's work for 16
 * useful rows and a 4096 x 4096 layer launches 32 workgroups on 256 compute units.  Here the weight image is cut into 128-column
 * strips AND contiguous K ranges (split-K), every (strip, range) workgroup streams its slab exactly once and writes an int32
 * partial block into the caller's workspace, and a second, elementwise kernel adds the partials and applies the epilogue.
 *
 * The numeric contract is INHERITED, not new.  int32 partial sums add up exactly in any order, so the sum of the partials is the
 * accumulator acc[i][j] of the tile path, bit for bit, and on it
 *   d_out_scale == NULL   y[i][j]  = act(fl(fl(fl((float)acc * rx[i]) * rw[j]) + bias[j]))     mmult_hip_q8.h, mmh_q8_linear_s8
 *   d_out_scale != NULL   yq[i][j] = clamp(rint(fl(y[i][j] * so[i])), -127, 127)               mmult_hip_q8o.h, mmh_q8o_linear
 * (three roundings, nothing contracted; no bias: no sum; in == 0: acc = 0; round-half-even, never -128, NaN -> 0).
 * tests/qchain_ref.py (qlinear_s8_ref) is the complete reference.  Every result is a pure function of the arguments.
 *
 * The plan (how-to-optimize-gemm_amd/csrc_q8d/qdecode_plan.hpp states the rule): strips = ceil(out / 128); the K ranges are
 * multiples of 128 long, as many as bring three workgroups to every two compute units, never more than keep the partials'
 * traffic (2 * splits * rows * out * 4 bytes) at a quarter of the weight's bytes, and never one that is empty.
 *
 * Every entry point leaves the caller's current device as it found it. */
#ifndef MMULT_HIP_Q8D_H_
#define MMULT_HIP_Q8D_H_

#include <stddef.h>

#include "mmult_hip.h"

#define MMH_Q8D_MAX_ROWS 16   /* one MFMA row block */

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error / of what the last mmh_q8d_linear launched, on this thread ("" if none). */
const char *mmh_q8d_last_error(void);
const char *mmh_q8d_last_launch(void);

/* rows in 1..16 (0: MMH_OK, nothing launched; more: MMH_ERR_UNSUPPORTED, nothing touched).
 *   dXq / ldq / d_inv_scale / dWq / pitch_n / d_w_inv_scale / dBias / activation: as mmh_q8o_linear -- the rows of
 *   mmh_q8_quantize_rows or of a previous int8-output layer, the operands mmh_q8_weight_info hands out.
 *   d_out_scale == NULL: the fp32 result goes to dY (pitch ldy >= out floats), dYq must be NULL;
 *   d_out_scale != NULL: rows floats, so; the int8 result goes to dYq (pitch ldyq >= out bytes, any address), dY must be NULL.
 *   d_work / work_bytes: the caller's scratch, at least the plan's work_bytes (splits * rows * (out rounded up to 4) * 4, rounded
 *     up to 16) and 16-byte aligned.  Its contents on entry are irrelevant and on exit unspecified; nothing beyond the plan's
 *     work_bytes is written.  in == 0 needs none (NULL, 0).
 *   splits: 0 = the plan's choice; > 0 forces that many K ranges -- MMH_ERR_INVALID_ARG where a range would be empty.
 * The kernels read dXq and dWq through buffer descriptors in dwords: a pitch that is no multiple of 4, a base that is not 4-byte
 * aligned or operands beyond the 2 GiB window (256 * ldq + in or (in + 256) * pitch_n + 256 >= 2^31 - 4096) are
 * MMH_ERR_UNSUPPORTED with a message; nothing is launched or touched.  Bytes of a row of dXq beyond `in` need not be zero.  Only
 * the rows x out elements of the output are written, never the bytes up to the pitch; an output whose base and pitch allow it
 * (fp32: 16-byte base, ldy % 4 == 0; int8: 4-byte base, ldyq % 4 == 0) is written four columns at a time, any other element by
 * element -- same bits.  in == 0: acc = 0, dXq, dWq and d_work are not read and may be NULL.  Two launches (one when in == 0),
 * no allocation, no state between calls. */
int mmh_q8d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const int8_t *dWq,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits, void *stream);

/* What mmh_q8d_linear launches for a shape and the workspace it needs, host arithmetic only (no device): text receives what
 * mmh_q8d_last_launch says after the call, e.g. "qdecode_partial_kernel, 32 strips x 8 splits of 512 k;
 * qdecode_finish_kernel<false>, 64 workgroups, wide stores".  out8: 0 the fp32 output, 1 the int8 one; ldo: ldy or ldyq;
 * xq_mod4 / wq_mod4: the addresses of dXq, dWq modulo 4; o_mod16: the output's modulo 16; splits as in the call; cu_count <= 0:
 * 256.  The operands' rules are mmh_q8d_linear's, with its status codes. */
int mmh_q8d_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int out8, int ldo, int xq_mod4, int wq_mod4, int o_mod16,
                        int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes);

/* Mean milliseconds per mmh_q8d_linear call: warmup calls, then reps calls between one pair of events on `stream`. */
int mmh_time_q8d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const int8_t *dWq, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call);

/* Argument errors (every entry point): a negative device, size or split count, out == 0 with rows > 0, a NULL operand that is
 * read, both or neither of dY / dYq (dY with d_out_scale, dYq without), a pitch below the row length, a workspace that is NULL or
 * misaligned, a forced split count with an empty range, an activation outside {MMH_ACT_NONE, MMH_ACT_RELU}:
 * MMH_ERR_INVALID_ARG, checked before any device call -- nothing is launched and no output is touched.  A workspace smaller
 * than the plan's (which depends on the device's CU count): MMH_ERR_INVALID_ARG before the first launch. */

#ifdef __cplusplus
}
#endif
#endif /* MMULT_HIP_Q8D_H_ */
