/* mmult_hip_q8o.h -- the C ABI of libmmult_hip_q8o.so: the int8 linear layer with an int8 OUTPUT (W8A8 in, A8 out) for the
 * AMD Instinct MI355X (gfx950).
 *
 * A third product library beside libmmult_hip.so and libmmult_hip_q8.so (same tree, same flags, its own translation units
 * under how-to-optimize-gemm_amd/csrc_q8o/).  It links nothing of the others and is stateless: no handle, no object, no
 * scratch, no allocation -- raw device pointers only, so a call on a capturing stream needs nothing reserved.  Status codes
 * and MMH_ACT_* are mmult_hip.h's.
 *
 * What it is for.  mmh_q8_linear writes fp32; the next layer's row quantiser then reads it back to make the int8 rows its
 * GEMM wants.  Here the GEMM's epilogue writes those int8 rows itself: the activations come in as mmh_q8_quantize_rows (or a
 * previous mmh_q8o_linear) left them, the weight operands are what mmh_q8_weight_info hands out, and the output is
 * quantised with a scale per row that the CALLER gives (a constant vector: static per-tensor calibration).
 *
 * The numeric contract (tests/qchain_ref.py restates it in numpy).  With acc, rx, rw, bias, act as in
 * mmult_hip_q8.h and so[i] the caller's output scale of row i:
 *   y[i][j]  = act(fl(fl(fl((float)acc[i][j] * rx[i]) * rw[j]) + bias[j]))     mmh_q8_linear's y: three roundings, nothing
 *                                                                              contracted; in == 0: acc = 0
 *   yq[i][j] = clamp(rint(fl(y[i][j] * so[i])), -127, 127)                     round-half-even, never -128; NaN -> 0,
 *                                                                              +-inf -> +-127 (mmh_quantize_sym_s8's rule)
 * The product y * so rounds once and is not fused with the sum before it.  so[i] must be finite; for a scale that is not, the
 * bytes are unspecified but nothing outside the output window is written.  The next layer's rx[i] is fl(1 / so[i]): the
 * caller computes it, no kernel writes it.  Every result is a pure function of the arguments.
 *
 * Every entry point leaves the caller's current device as it found it. */
#ifndef MMULT_HIP_Q8O_H_
#define MMULT_HIP_Q8O_H_

#include "mmult_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Text of the last error / of what the last mmh_q8o_linear launched, on this thread ("" if none). */
const char *mmh_q8o_last_error(void);
const char *mmh_q8o_last_launch(void);

/* yq (rows x out int8, pitch ldyq >= out bytes, any address) = the contract above.
 *   dXq            rows x in int8, pitch ldq >= in; d_inv_scale: rows floats, rx
 *   dWq            in x pitch_n int8, image[k][j] of output channel j, pitch_n >= out; d_w_inv_scale: out floats, rw
 *   dBias          out floats or NULL; activation: MMH_ACT_NONE or MMH_ACT_RELU; d_out_scale: rows floats, so
 * The tile reads dXq and dWq through buffer descriptors in dwords: a pitch that is no multiple of 4, a base that is not 4-byte
 * aligned or operands beyond the 2 GiB window (256 * ldq + in or (in + 256) * pitch_n + 256 >= 2^31 - 4096) are
 * MMH_ERR_UNSUPPORTED with a message; nothing is launched or touched.  Bytes of a row of dXq beyond `in` need not be zero.
 * Only the rows x out bytes of yq are written, never the bytes up to the pitch.  A yq whose base and ldyq are multiples of 4
 * is written in dwords, any other byte by byte -- same bytes.  rows == 0: MMH_OK, nothing launched.  in == 0: acc = 0, dXq and
 * dWq are not read and may be NULL. */
int mmh_q8o_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const int8_t *dWq,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   int8_t *dYq, int ldyq, void *stream);

/* What mmh_q8o_linear launches for a shape, host arithmetic only (no device): text receives what mmh_q8o_last_launch says
 * after the call, e.g. "qlinear_s8o_kernel<128,128,4,true>, 6 workgroups".  xq_mod4 / wq_mod4 / yq_mod4: the addresses of
 * dXq, dWq, dYq modulo 4; cu_count <= 0: 256.  The tile: 256x256 where mmh_igemm_s8 would choose it (csrc/igemm_plan.hpp,
 * i8_big_tile), else 128x128; the unguarded instantiation for whole tiles with yq_mod4 == 0 and ldyq % 4 == 0.  The operands'
 * rules are mmh_q8o_linear's, with its status codes. */
int mmh_q8o_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int ldyq, int xq_mod4, int wq_mod4, int yq_mod4,
                        int cu_count, char *text, int text_bytes);

/* Mean milliseconds per mmh_q8o_linear call: warmup calls, then reps calls between one pair of events on `stream`. */
int mmh_time_q8o_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const int8_t *dWq, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, int8_t *dYq, int ldyq, int warmup, int reps, void *stream, float *ms_per_call);

/* Argument errors (every entry point): a negative device or size, out == 0 with rows > 0, a NULL operand that is read, a
 * pitch below the row length, an activation outside {MMH_ACT_NONE, MMH_ACT_RELU}: MMH_ERR_INVALID_ARG, checked before any
 * device call -- nothing is launched and no output is touched. */

#ifdef __cplusplus
}
#endif
#endif /* MMULT_HIP_Q8O_H_ */
