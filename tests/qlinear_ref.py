"""The int8 linear layer's contract (include/mmult_hip_q8.h) restated in numpy.  (Shared test code: see
tests/bitcmp.py.)

Per row of x and per output channel of w the quantisation is oracle.quantize_sym_s8 on that vector alone; the sums are
oracle.ref_igemm_s8's exact int32; the epilogue is np.float32 operations in the stated order, one rounding each:
    y = act(fl(fl(fl(float32(acc) * rx[i]) * rw[j]) + bias[j])),   rx = fl(1 / sx), rw = fl(1 / sw)
float32(acc) rounds to nearest even (numpy's int32 -> float32 cast), no bias: no sum, ReLU: y if (y > 0 or y is NaN) else +0.

Also here: the special rows every test of the contract uses, plan_text -- mmh_q8_linear_plan's arithmetic in Python --, and
shapes_256 / thin_256: the smallest shapes the plan sends to the 256x256 tile on a device (the tables' and the fuzzer's)."""
import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)


def quantize_rows_ref(x):
    """(q int8 like x, scale float32 per row, inv_scale float32 per row)."""
    from oracle import oracle as O
    x = np.ascontiguousarray(x, dtype=np.float32)
    q, s = np.zeros(x.shape, np.int8), np.ones(x.shape[0], np.float32)
    if x.shape[1] > 0:
        for i in range(x.shape[0]):
            q[i], si = O.quantize_sym_s8(x[i])
            s[i] = np.float32(si)
    with np.errstate(all="ignore"):
        r = np.float32(1.0) / s
    return q, s, r


def int_sums(qx, qw):
    """acc[i][j] = sum_k qx[i][k] * qw[j][k], int32."""
    from oracle import oracle as O
    if qx.shape[1] == 0:
        return np.zeros((qx.shape[0], qw.shape[0]), np.int32)
    return O.ref_igemm_s8(np.ascontiguousarray(qx), np.ascontiguousarray(qw.T))


def epilogue_ref(acc, rx, rw, bias=None, relu=False):
    with np.errstate(all="ignore"):
        y = acc.astype(np.float32)
        y = y * rx.astype(np.float32)[:, None]
        y = y * rw.astype(np.float32)[None, :]
        if bias is not None:
            y = y + np.asarray(bias, np.float32)[None, :]
        if relu:
            y = np.where(y <= 0, np.float32(0.0), y)   # NaN <= 0 is false: NaN stays; -0 <= 0: +0
    assert y.dtype == np.float32
    return y


def qlinear_ref(x, w, bias=None, relu=False):
    qx, _, rx = quantize_rows_ref(x)
    qw, _, rw = quantize_rows_ref(w)
    return epilogue_ref(int_sums(qx, qw), rx, rw, bias, relu)


def special_rows(cols, rng):
    """Rows of `cols` >= 4 columns that meet every special rule of the quantiser, and what each must give: a list of
    (name, row float32, expected scale float32 or None, check(q) -> bool)."""
    u = rng.uniform(-1, 1, cols).astype(np.float32)
    zero = np.zeros(cols, np.float32)
    nan = u.copy()
    nan[1] = np.nan
    inf = u.copy()
    inf[0], inf[2] = np.inf, -np.inf
    amax_inf = np.abs(np.where(np.isfinite(inf), inf, 0)).max()
    tiny = np.zeros(cols, np.float32)
    tiny[3] = np.float32(1e-38)
    neg = np.full(cols, -2.5, np.float32)
    return [
        ("all zero", zero, np.float32(1.0), lambda q: not q.any()),
        ("NaN", nan, np.float32(127.0) / np.abs(np.delete(u, 1)).max(), lambda q: q[1] == 0),
        ("+-inf", inf, np.float32(127.0) / amax_inf, lambda q: q[0] == 127 and q[2] == -127),
        ("max 1e-38", tiny, F32_MAX, lambda q: q[3] == 3 and not np.delete(q, 3).any()),   # rint(1e-38 * FLT_MAX) = rint(3.4)
        ("-max", neg, np.float32(127.0) / np.float32(2.5), lambda q: bool((q == -127).all())),
    ]


# ---- mmh_q8_linear_plan in Python ----------------------------------------------------------------------------------------
def big_tile(m, n, cus):
    """csrc/igemm_plan.hpp's i8_big_tile."""
    tiles256 = ((m + 255) // 256) * ((n + 255) // 256)
    tiles128 = ((m + 127) // 128) * ((n + 127) // 128)
    r256, r128 = (tiles256 + cus - 1) // cus, (tiles128 + 2 * cus - 1) // (2 * cus)
    return r256 <= 0.6 * r128 + 1e-9


IN_256 = 192


def shapes_256(cu_count):
    """((rows, out, in) whole, ragged): the multiple-of-256 shape of the fewest elements that i8_big_tile sends to the 256x256
    tile on this device, and its neighbour three rows and five columns short (the same tiles)."""
    best = None
    for a in range(1, 33):
        for b in range(a, 65):
            if big_tile(256 * a, 256 * b, cu_count) and (best is None or a * b < best[0] * best[1]):
                best = (a, b)
    assert best, cu_count
    m, n = 256 * best[0], 256 * best[1]
    assert big_tile(m - 3, n - 5, cu_count)
    return (m, n, IN_256), (m - 3, n - 5, IN_256)


def thin_256(a, b, cu_count):
    """(rows, out) of the fewest elements that i8_big_tile sends to the 256x256 tile with a last tile `a` rows high and `b`
    columns wide.  (One tile row and column more than shapes_256's shape, not its neighbour a + 256 by b + 256 short of the
    next multiple: that one fills fewer 128x128 rounds and goes to the small tile.)"""
    best = None
    for i in range(1, 34):
        for j in range(i, 66):
            rows, out = 256 * (i - 1) + a, 256 * (j - 1) + b
            if big_tile(rows, out, cu_count) and (best is None or rows * out < best[0] * best[1]):
                best = (rows, out)
    assert best and big_tile(best[0], best[1], cu_count), (a, b, cu_count)
    return best


def plan_text(rows, out, in_, ldx=0, ldy=0, x_mod16=0, y_mod16=0, bias=False, relu=False, cus=256):
    """(text, scratch bytes) as mmh_q8_linear_plan gives them."""
    ldx, ldy = ldx or max(in_, 1), ldy or out
    b = lambda f: "true" if f else "false"
    wide, vec = in_ >= 1024, x_mod16 == 0 and ldx % 4 == 0
    qgrid = rows if wide else (rows + 3) // 4
    tile = 256 if big_tile(rows, out, cus) else 128
    edge = not (rows % tile == 0 and out % tile == 0 and ldy % 4 == 0 and y_mod16 == 0)
    grid = ((rows + tile - 1) // tile) * ((out + tile - 1) // tile)
    a16 = lambda n: (n + 15) & ~15
    scratch = a16(rows * a16(in_)) + 2 * a16(4 * rows)
    return (f"quantize_rows_s8_kernel<{b(wide)}> ({'vector' if vec else 'scalar'} path), {qgrid} workgroups, then "
            f"qlinear_s8_kernel<{tile},{tile},{tile // 32},{b(edge)},{b(bias)},{b(relu)}>, {grid} workgroups"), scratch
