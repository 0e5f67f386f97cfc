"""The 4-bit small-batch layer with one scale per group of 128 input features (libmmult_hip_q4g.so, include/mmult_hip_q4g.h) as
the tests see it.  numpy only.  (Shared test code: see tests/bitcmp.py.)

The packed image, its quantiser rules and the unpacking are tests/q4_ref.py's, imported.  What is new is restated here: the
quantiser applied per channel AND group (quantize4g_ref), the scale layout (layout), the plan (plan(): q4_ref's without the
65536-k ceiling) and the NUMERIC CONTRACT, which is this library's own: want() is include/mmult_hip_q4g.h's chain in numpy
float32, group by group -- every line one float32 operation, so one rounding, and never an fma:

    S_g = sum over group g of xq[i, k] W[k, j]      exact (float64 products of small integers), |S_g| <= 2^17
    t_g = f32(S_g) * r[g, j]
    P_p = 0;  for g ascending in range p:  P_p = P_p + t_g
    Z   = 0;  for p ascending:             Z   = Z + P_p
    v   = Z * rx[i];  v = v + bias[j];  ReLU;  int8: qchain_ref.requant_ref(v, so)

The bits depend on the partition (splits, k_len): want() takes it as an argument, plan() says what the library chooses."""
import numpy as np

import q4_ref as F
import qchain_ref as Q
import qdecode_ref as D

GROUP, STRIP, SLICE, MAX_ROWS = 128, 128, 128, 16
S_BOUND = 128 * 128 * 8   # |S_g| <= 2^17: 128 k of |x| <= 128 against |W| <= 8


def groups(in_):
    return -(-in_ // GROUP)


# ---- the quantiser and the layout -------------------------------------------------------------------------------------------
def layout(out, in_):
    """(pitch_n, packed_rows, groups, pitch_s, image bytes, scale bytes) as mmh_q4g_weight_layout gives them."""
    pitch, prow, _ = F.layout(out, in_)
    return pitch, prow, groups(in_), pitch, pitch * prow, groups(in_) * pitch * 4


def quantize4g_ref(w):
    """(q int8 (out, in) in -7 .. 7, s4 float32 (groups, out), r = fl(1 / s4) float32 (groups, out)) of a float32 (out, in)
    weight: q4_ref.quantize4_ref -- quant_rules_s4.hpp's rules, unchanged -- on every group of 128 columns by itself."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    out, in_ = w.shape
    q = np.zeros((out, in_), np.int8)
    s = np.zeros((groups(in_), out), np.float32)
    r = np.zeros((groups(in_), out), np.float32)
    for g in range(groups(in_)):
        q[:, g * GROUP:(g + 1) * GROUP], s[g], r[g] = F.quantize4_ref(w[:, g * GROUP:(g + 1) * GROUP])
    return q, s, r


def dequantize_ref(q, r):
    """The fp32 (out, in) weight the layer multiplies by: q[j, k] * r[k // 128, j], one rounding."""
    with np.errstate(all="ignore"):
        return q.astype(np.float32) * np.repeat(r, GROUP, axis=0)[:q.shape[1]].T


# ---- mmh_q4g_linear_plan in Python ------------------------------------------------------------------------------------------
def plan(rows, out, in_, out8=False, ldo=0, o_mod16=0, splits=0, cus=256):
    """(text, work bytes, splits, k_len) as mmh_q4g_linear_plan gives them; None where it refuses a forced split count for an
    empty range.  qdecode_ref.plan with the weight as in * out / 2 bytes in the traffic cap (q4_ref.plan's cap) and no ceiling."""
    ldo = ldo or (((out + 15) & ~15) if out8 else out)
    strips, slices = -(-out // STRIP), -(-in_ // SLICE)
    wide = (ldo % 4 == 0 and o_mod16 % 4 == 0) if out8 else (ldo % 4 == 0 and o_mod16 == 0)
    finish = -(-out // D.FINISH_COLS) * rows
    tail = f"q4gdecode_finish_kernel<{'true' if out8 else 'false'}>"
    stores = "wide stores" if wide else "single stores"
    if in_ == 0:
        return f"{tail} alone, {finish} workgroups, {stores}", 0, 0, 0
    if splits > 0:
        if not D.valid_splits(in_, splits):
            return None
        k_len = D.ranges(in_, splits)[0]
    else:
        want_ = -(-D.WG_NUM * cus // (D.WG_DEN * strips))
        cap = in_ * D.TRAFFIC_NUM // (16 * rows * D.TRAFFIC_DEN)
        splits = max(1, min(want_, cap, slices))
        per = -(-slices // splits)
        k_len, splits = per * SLICE, -(-slices // per)
    return (f"q4gdecode_partial_kernel, {strips} strips x {splits} splits of {k_len} k; {tail}, {finish} workgroups, {stores}",
            D.work_bytes(splits, rows, out), splits, k_len)


def window_ok(ldq, pitch_n, in_, pitch_s):
    """The 2 GiB descriptor window: x and the packed image as q4_ref.window_ok holds them; the scale rows and the rows the ring
    requests behind a range's end."""
    return F.window_ok(ldq, pitch_n, in_) and (groups(in_) + 4) * pitch_s * 4 + 1024 < D.WINDOW


def largest_pitch_s(in_):
    """The largest multiple of 4 with (groups + 4) * pitch_s * 4 + 1024 < WINDOW."""
    return (D.WINDOW - 1024 - 1) // (4 * (groups(in_) + 4)) & ~3


# ---- the reference ----------------------------------------------------------------------------------------------------------
def group_sums(xq, W):
    """S[g][i][j] = sum over group g of xq[i][k] * W[k][j]: float32 (groups, rows, out) holding exact integers, |S| <= 2^17."""
    xq, W = np.asarray(xq, np.float64), np.asarray(W, np.float64)
    S = np.zeros((groups(xq.shape[1]), xq.shape[0], W.shape[1]), np.float64)
    for g in range(S.shape[0]):
        S[g] = xq[:, g * GROUP:(g + 1) * GROUP] @ W[g * GROUP:(g + 1) * GROUP]
    assert np.abs(S).max(initial=0) <= S_BOUND
    f = S.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), S)   # (float)S_g is exact
    return f


def range_groups(in_, splits, k_len):
    """[(first group, one past the last group) ...] of the partition's K ranges."""
    assert k_len % GROUP == 0
    per = k_len // GROUP
    return [(p * per, min((p + 1) * per, groups(in_))) for p in range(splits)]


def partials(xq, P, in_, r, splits, k_len):
    """What q4gdecode_partial_kernel leaves in the workspace: float32 (splits, rows, out), each range a chain from +0 in
    ascending group order of t_g = f32(S_g) * r[g]."""
    W = F.unpack_ref(P, in_)
    S = group_sums(xq, W)
    r = np.asarray(r, np.float32)[:, :W.shape[1]]
    out = np.zeros((splits, S.shape[1], W.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for p, (g0, g1) in enumerate(range_groups(in_, splits, k_len)):
            assert g0 < g1, "the partition leaves a range empty"
            for g in range(g0, g1):
                t = S[g] * r[g][None, :]       # one rounding
                out[p] = out[p] + t            # one rounding
    return out


def finish(Z, rx, bias=None, relu=False, so=None):
    """The finish kernel behind its sum: v = Z * rx; v = v + bias; ReLU (NaN stays, -0 -> +0); int8 under `so`."""
    with np.errstate(all="ignore"):
        v = Z * np.asarray(rx, np.float32)[:, None]
        if bias is not None:
            v = v + np.asarray(bias, np.float32)[None, :]
        if relu:
            v = np.where(v <= 0, np.float32(0.0), v)
    assert v.dtype == np.float32
    return v if so is None else Q.requant_ref(v, so)


def want(xq, rx, P, in_, r, bias=None, relu=False, splits=1, k_len=None, so=None):
    """The layer on int8 rows xq (rows, in), their factors rx, a packed image P (packed rows, out), the groups' factors r
    (groups, >= out) under the partition (splits, k_len): fp32 y, or int8 under the output scales so.  in == 0: splits 0."""
    xq = np.asarray(xq, np.int8)
    out = np.asarray(P).shape[1]
    Z = np.zeros((xq.shape[0], out), np.float32)
    if in_ > 0:
        k_len = k_len if k_len is not None else D.ranges(in_, splits)[0]
        with np.errstate(all="ignore"):
            for part in partials(xq, P, in_, r, splits, k_len):
                Z = Z + part                   # range order, one rounding each
    return finish(Z, rx, bias, relu, so)


# ---- inputs the tests share -------------------------------------------------------------------------------------------------
def spread_factors(rng, n_groups, out):
    """Group factors 2^e * m with e uniform in -12 .. 12 and m uniform in [1, 2): neighbouring terms differ by up to 2^24, so
    any other order, a wider accumulator or a fused multiply-add rounds differently somewhere."""
    e = rng.integers(-12, 13, (n_groups, out))
    return (np.ldexp(1.0, e) * rng.uniform(1.0, 2.0, (n_groups, out))).astype(np.float32)


def outlier_weight(rng, out, in_, factor=20.0):
    """(gaussian weight, the same weight with one element per row scaled by `factor`)."""
    w = rng.standard_normal((out, in_)).astype(np.float32)
    spiked = w.copy()
    cols = rng.integers(0, in_, out)
    spiked[np.arange(out), cols] *= np.float32(factor)
    return w, spiked
