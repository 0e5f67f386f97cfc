"""The int8-to-int8 linear layer's contract (include/mmult_hip_q8o.h) and the chain of such layers,
restated in numpy on top of tests/qlinear_ref.py.  (Shared test code: see tests/bitcmp.py.)

    y  = act(fl(fl(fl(float32(acc) * rx[i]) * rw[j]) + bias[j]))        qlinear_ref.epilogue_ref, unchanged
    yq = clamp(rint(fl(y * so[i])), -127, 127)                           one more float32 rounding, half to even, never -128;
                                                                         NaN -> 0, +-inf -> +-127
The next layer reads yq as its rows with rx[i] = fl(1 / so[i]).

Also here: plan_text_s8o -- mmh_q8o_linear_plan's arithmetic in Python -- and scale_of_amax, the quantiser's scale rule."""
import numpy as np

import qlinear_ref as R


def scale_of_amax(amax):
    """csrc/quant_rules_s8.hpp's scale_of_amax in float32."""
    a = np.float32(amax)
    if not a > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        s = np.float32(127.0) / a
    return s if s <= R.F32_MAX else R.F32_MAX


def requant_ref(y, so):
    """int8 like y: csrc/quant_rules_s8.hpp's quantize_one of every element of row i with the scale so[i].  (fmax / fmin as the
    device's fmaxf / fminf: a NaN product -- only a non-finite or zero scale makes one -- is dropped for the bound.)"""
    y = np.asarray(y, np.float32)
    so = np.asarray(so, np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        t = y * so                                   # one rounding
        t = np.where(np.isnan(y), np.float32(0.0), t)
        r = np.fmin(np.fmax(np.rint(t), np.float32(-127.0)), np.float32(127.0))
    assert t.dtype == np.float32 and r.dtype == np.float32
    q = np.empty(r.shape, np.int8)   # (a new C-ordered array: astype keeps the strides of a one-column float array)
    q[...] = r
    return q


def inv_scale_ref(so):
    with np.errstate(all="ignore"):
        return np.float32(1.0) / np.asarray(so, np.float32)


def qlinear_s8_ref(xq, rx, w, bias=None, relu=False, so=None):
    """The layer on rows that are quantised already: xq int8 (rows, in), rx float32 (rows,), w float32 (out, in).  so None:
    y float32 (mmh_q8_linear_s8); so float32 (rows,): yq int8 (mmh_q8o_linear)."""
    qw, _, rw = R.quantize_rows_ref(w)
    y = R.epilogue_ref(R.int_sums(np.ascontiguousarray(xq, dtype=np.int8), qw), np.asarray(rx, np.float32), rw, bias, relu)
    return y if so is None else requant_ref(y, so)


def chain_ref(x, layers, out_scales, relu=True, last_relu=False):
    """One row quantiser, int8 -> int8 for every hidden layer, int8 -> float32 for the last.  layers: [(w, bias or None)];
    out_scales: one scale per hidden layer (the same for every row).  Returns (y float32, [hidden yq int8 ...])."""
    assert len(out_scales) == len(layers) - 1
    xq, _, rx = R.quantize_rows_ref(x)
    hidden = []
    for (w, b), s in zip(layers[:-1], out_scales):
        so = np.full(xq.shape[0], np.float32(s), np.float32)
        xq = qlinear_s8_ref(xq, rx, w, b, relu, so)
        rx = inv_scale_ref(so)
        hidden.append(xq)
    w, b = layers[-1]
    return qlinear_s8_ref(xq, rx, w, b, last_relu), hidden


def calibrate_ref(x, layers, relu=True):
    """QMLP.calibrate: the layers with float32 outputs (every layer quantises its own input rows); per hidden layer
    scale_of_amax of the largest finite |h|."""
    h, scales = np.asarray(x, np.float32), []
    for w, b in layers[:-1]:
        h = R.qlinear_ref(h, w, b, relu)
        a = np.abs(h)
        scales.append(scale_of_amax(np.where(np.isfinite(a), a, np.float32(0)).max() if h.size else 0.0))
    return scales


# ---- mmh_q8o_linear_plan in Python ----------------------------------------------------------------------------------------
def plan_text_s8o(rows, out, ldyq=0, yq_mod4=0, cus=256):
    """The launch text as mmh_q8o_linear_plan gives it.  ldyq 0: out rounded up to 16."""
    ldyq = ldyq or (out + 15) & ~15
    tile = 256 if R.big_tile(rows, out, cus) else 128
    dwords = ldyq % 4 == 0 and yq_mod4 == 0
    edge = not (rows % tile == 0 and out % tile == 0 and dwords)
    grid = ((rows + tile - 1) // tile) * ((out + tile - 1) // tile)
    return f"qlinear_s8o_kernel<{tile},{tile},{tile // 32},{'true' if edge else 'false'}>, {grid} workgroups"
