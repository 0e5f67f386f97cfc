"""The small-batch int8 layer (libmmult_hip_q8d.so, include/mmult_hip_q8d.h) as the tests see it.  (Shared test code: see
tests/bitcmp.py.)

The numeric contract is inherited -- tests/qchain_ref.py's qlinear_s8_ref is the complete reference -- so what is restated here
is only what is new: plan() is csrc_q8d/qdecode_plan.hpp's arithmetic in Python, valid_splits says which forced split counts
leave no K range empty, and cases() is the table tests/test_gpu_qdecode.py runs (tests/test_q8d_coverage.py holds the classes
it promises, on the CPU); wide_deep_cases() is its second table, at the sizes the kernels are built for: outputs wider than one
finish workgroup, many K ranges, deep ranges, every row count; window_ok and its two largest_* say where the descriptor
window ends.  Also here: the tables' inputs -- problem() (a real weight; every 128-byte slice of k moves the sums),
image_problem() (a caller-made image and rows over the full int8 range, -128 included) and large_sums_problem()."""
import collections
import functools

import numpy as np

import qchain_ref as Q
import qlinear_ref as R

STRIP, SLICE, MAX_ROWS = 128, 128, 16
WG_NUM, WG_DEN = 3, 2             # kQdWgNum / kQdWgDen: three workgroups on two CUs
TRAFFIC_NUM, TRAFFIC_DEN = 1, 4   # kQdTrafficNum / kQdTrafficDen
FINISH_COLS = 1024


# ---- mmh_q8d_linear_plan in Python -----------------------------------------------------------------------------------------
def work_bytes(splits, rows, out):
    """The header's formula: splits * rows * (out rounded up to 4) * 4, rounded up to 16."""
    return (splits * rows * ((out + 3) & ~3) * 4 + 15) & ~15


def ranges(in_, splits):
    """(k_len, [(begin, end) ...]) of a forced split count, ends cut at in_; a range with begin >= end is empty."""
    slices = -(-in_ // SLICE)
    k_len = SLICE * -(-slices // splits)
    return k_len, [(s * k_len, min((s + 1) * k_len, in_)) for s in range(splits)]


def valid_splits(in_, splits):
    return in_ > 0 and splits > 0 and all(b < e for b, e in ranges(in_, splits)[1])


def plan(rows, out, in_, out8=False, ldo=0, o_mod16=0, splits=0, cus=256):
    """(text, work bytes, splits, k_len) as mmh_q8d_linear_plan gives them, or None where it refuses a forced split count.
    ldo 0: dense fp32 rows, int8 rows of pitch out rounded up to 16."""
    ldo = ldo or (((out + 15) & ~15) if out8 else out)
    strips, slices = -(-out // STRIP), -(-in_ // SLICE)
    wide = (ldo % 4 == 0 and o_mod16 % 4 == 0) if out8 else (ldo % 4 == 0 and o_mod16 == 0)
    finish = -(-out // FINISH_COLS) * rows
    tail = f"qdecode_finish_kernel<{'true' if out8 else 'false'}>"
    stores = "wide stores" if wide else "single stores"
    if in_ == 0:
        return f"{tail} alone, {finish} workgroups, {stores}", 0, 0, 0
    if splits > 0:
        if not valid_splits(in_, splits):
            return None
        k_len = ranges(in_, splits)[0]
    else:
        want = -(-WG_NUM * cus // (WG_DEN * strips))
        cap = in_ * TRAFFIC_NUM // (8 * rows * TRAFFIC_DEN)
        splits = max(1, min(want, cap, slices))
        per = -(-slices // splits)
        k_len, splits = per * SLICE, -(-slices // per)
    return (f"qdecode_partial_kernel, {strips} strips x {splits} splits of {k_len} k; {tail}, {finish} workgroups, {stores}",
            work_bytes(splits, rows, out), splits, k_len)


# ---- the descriptor window (csrc/igemm_plan.hpp: i8_window, as tests/int8_ops.py restates it) ----------------------------------------
WINDOW = (1 << 31) - 4096


def window_ok(ldq, pitch_n, in_):
    return 256 * ldq + in_ < WINDOW and (in_ + 256) * pitch_n + 256 < WINDOW


def largest_pitch_n(in_):
    """The largest multiple of 4 with (in + 256) * pitch_n + 256 < WINDOW."""
    return (WINDOW - 256 - 1) // (in_ + 256) & ~3


def largest_ldq(in_):
    """The largest multiple of 4 with 256 * ldq + in < WINDOW."""
    return (WINDOW - in_ - 1) // 256 & ~3


# ---- the GPU table ----------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 15, 16)
INS = (0, 1, 63, 64, 65, 127, 128, 129, 384, 385, 1153)
OUTS = (1, 16, 17, 127, 128, 129, 2 * STRIP + 1, 2 * STRIP + 15, 2 * STRIP + 17)
FORCED = (1, 2, 3)
X_LAYOUTS = [(pad, off) for pad in (0, 4, 8, 12) for off in (0, 4, 8, 12)]   # (ldq - in rounded up to 4, x's base past 16)
Y_LAYOUTS = [(0, 0), (1, 0), (4, 4), (2, 1), (8, 0), (3, 3), (4, 0), (5, 2)]   # (ldy - out, y's base past 16 in FLOATS): wide ones and odd ones
YQ_LAYOUTS = [(0, 0), (1, 1), (4, 0), (2, 2), (3, 3), (8, 0), (5, 0), (4, 1)]   # (ldyq - out, yq's base past 16 in bytes)
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]         # (bias, relu)

# rows, out, in_: the shape; splits: 0 the plan's choice, else forced; x_pad / x_off: X_LAYOUTS; y / yq: indices of Y_LAYOUTS /
# YQ_LAYOUTS; weight: "qweight" a real QWeight, "image" a caller-made image (its own pitch, base and row factors); bias, relu
Case = collections.namedtuple("Case", "rows out in_ splits x_pad x_off y yq weight bias relu")


def _case(i, rows, out, in_, splits):
    pad, off = X_LAYOUTS[5 * i % 16]
    bias, relu = EPILOGUES[i % 4]
    weight = "image" if i % 3 == 2 or in_ == 0 else "qweight"   # (in == 0: no weight object to prepare, NULL operands)
    return Case(rows, out, in_, splits, pad, off, i % len(Y_LAYOUTS), (3 * i) % len(YQ_LAYOUTS), weight, bias, relu)


@functools.lru_cache(maxsize=None)
def cases():
    """Every `in` at every forced split count that leaves no range empty (rows and out rotating), then every out at two row
    counts (in and the splits rotating over the deep ones), then in == 0 at every row count."""
    out, i = [], 0
    for in_ in INS[1:]:
        for s in FORCED:
            if valid_splits(in_, s):
                out.append(_case(i, ROWS[i % 4], OUTS[(2 * i + 1) % len(OUTS)], in_, s))
                i += 1
    deep = [(129, 2), (385, 2), (1153, 3), (384, 3), (1153, 2), (384, 2)]
    for j, n in enumerate(OUTS):
        for r in (0, 2):
            in_, s = deep[i % len(deep)]
            out.append(_case(i, ROWS[(j + r) % 4], n, in_, s))
            i += 1
    for rows in ROWS:
        out.append(_case(i, rows, OUTS[i % len(OUTS)], 0, 0))
        i += 1
    return tuple(out)


PLAN_SHAPE = (16, 256, 8192)   # splits = 0 here: the plan splits on the device's CU count (2 strips: 16 ranges at 256 CUs)


# ---- the second table: what the kernels are built for -------------------------------------------------------------------------
WIDE_OUTS = (FINISH_COLS, FINISH_COLS + 1, FINISH_COLS + 3, FINISH_COLS + 4, 2 * FINISH_COLS + 1, 17 * STRIP + 1, 4 * FINISH_COLS + 4)
WIDE_ROWS = (16, 1, 15, 2, 7, 3, 12, 5)                          # two neighbours per out
SHALLOW = ((129, 2), (257, 2), (385, 4), (257, 3), (385, 2))     # (in, forced ranges) behind the wide outputs
MANY_RANGES_INS = (1153, 1280)                                   # forced counts above 3, up to one range per slice
OWN_CHOICE = ((1, 130, 8192), (2, 130, 8192), (1, FINISH_COLS + 1, 4224))   # splits == 0: one slice per range at 256 CUs
DEEP = ((4224, 1), (11008, 1), (11008, 2))                       # (in, forced ranges) at 16 rows, 130 columns: 33, 86, 43 slices
LADDER = (130, 257, 2)                                           # (out, in, forced ranges) at every row count 1 - 16
RESERVE_SHAPE = (257, 1153)                                      # (out, in) whose own split count varies with the rows


@functools.lru_cache(maxsize=None)
def wide_deep_cases():
    """The finish grid (every WIDE_OUTS at two row counts behind two or three shallow ranges, then 1027 columns on the two
    layouts whose stores are wide although out is no multiple of 4), then every forced count above 3 that leaves no range of
    MANY_RANGES_INS empty, the plan's own choice where it is one slice per range, the deep ranges (the middle one on a
    caller-made image), and LADDER at every row count.  Layouts, weights and epilogues rotate as in cases()."""
    out = []

    def add(rows, n, in_, s, **fixed):
        out.append(_case(len(out), rows, n, in_, s)._replace(**fixed))

    for j, n in enumerate(WIDE_OUTS):
        for r in (0, 1):
            add(WIDE_ROWS[(2 * j + r) % len(WIDE_ROWS)], n, *SHALLOW[len(out) % len(SHALLOW)])
    # ldy = out + 1 at a 16-byte base, ldyq = out + 5 at a 4-byte base: whole rows of dwords, the last three columns one by one
    add(16, FINISH_COLS + 3, 257, 2, y=Y_LAYOUTS.index((1, 0)), yq=YQ_LAYOUTS.index((5, 0)))
    add(1, FINISH_COLS + 3, 129, 2, y=Y_LAYOUTS.index((1, 0)), yq=YQ_LAYOUTS.index((5, 0)))
    for in_ in MANY_RANGES_INS:
        for s in range(FORCED[-1] + 1, -(-in_ // SLICE) + 1):
            if valid_splits(in_, s):
                add(ROWS[len(out) % 4], OUTS[len(out) % len(OUTS)], in_, s)
    for rows, n, in_ in OWN_CHOICE:
        add(rows, n, in_, 0)
    for j, (in_, s) in enumerate(DEEP):
        add(MAX_ROWS, 130, in_, s, weight="image" if j == 1 else "qweight")
    for rows in range(1, MAX_ROWS + 1):
        add(rows, *LADDER)
    return tuple(out)


def case_id(c):
    return f"{c.rows}x{c.out}x{c.in_}-s{c.splits}-x{c.x_pad}.{c.x_off}-y{c.y}.{c.yq}-{c.weight}-{'b' if c.bias else ''}{'r' if c.relu else ''}"


# ---- inputs -------------------------------------------------------------------------------------------------------------------
Problem = collections.namedtuple("Problem", "xq rx w qw rw bias so acc")   # w: the fp32 weight, or None for a caller-made image


def out_scales(y):
    """One output scale per row: scale_of_amax of the row's largest finite |y|."""
    a = np.where(np.isfinite(y), np.abs(y), np.float32(0))
    return np.array([Q.scale_of_amax(r.max() if r.size else 0.0) for r in a], np.float32)


def int_sums(xq, qw):
    """R.int_sums; a weight of ONE channel goes in twice (its transpose, a (k, 1) array, has no row stride numpy would keep)."""
    return R.int_sums(xq, qw) if qw.shape[0] != 1 else R.int_sums(xq, np.concatenate([qw, qw]))[:, :1].copy()


def every_slice_moves_the_sums(xq, qw, acc):
    """Each 128-byte slice of k contributes a non-zero amount to at least 90 % of the sums: a slice that is dropped, read twice
    or read from the wrong range shows in the fp32 output, which keeps every bit of a sum below 2^24."""
    assert np.abs(acc).max() < 1 << 24
    for k0 in range(0, xq.shape[1], SLICE):
        part = int_sums(xq[:, k0:k0 + SLICE], qw[:, k0:k0 + SLICE])
        assert float((part != 0).mean()) >= 0.9, (xq.shape, qw.shape, k0)


@functools.lru_cache(maxsize=None)
def problem(rows, out, in_):
    """A real layer: x ~ 3 N(0, 1), w ~ U(-0.5, 0.5), the last column of every row of both plus or minus the row's maximum (so
    that a lone k tail carries the largest products); quantised by the reference quantiser."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 16)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    if in_:
        for v in (x, w):
            v[:, -1] = np.abs(v).max(axis=1) * rng.choice(np.array([-1, 1], np.float32), v.shape[0])
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    xq, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = int_sums(xq, qw)
    every_slice_moves_the_sums(xq, qw, acc)
    return Problem(xq, rx, w, qw, rw, bias, out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


def int8_full_range(rng, shape):
    """Random int8 over the full range with -128 planted at about 1 / 64 of the positions."""
    x = rng.integers(-128, 128, shape, dtype=np.int8)
    if x.size:
        x.reshape(-1)[rng.integers(0, x.size, max(1, x.size // 64))] = -128
    return x


@functools.lru_cache(maxsize=None)
def image_problem(rows, out, in_):
    """Operands no quantiser makes: rows AND image over the full int8 range with -128 planted, the last row all -128, arbitrary
    positive row and channel factors."""
    rng = np.random.default_rng(rows * 5 + out * 11 + in_ + 128)
    xq = int8_full_range(rng, (rows, in_))
    xq[-1] = -128
    qw = int8_full_range(rng, (out, in_))
    rx = rng.uniform(0.01, 0.05, rows).astype(np.float32)
    rw = rng.uniform(0.001, 0.004, out).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    acc = int_sums(xq, qw)
    if in_:
        assert (xq == -128).any() and (qw == -128).any()
        every_slice_moves_the_sums(xq, qw, acc)
    return Problem(xq, rx, None, qw, rw, bias, out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


@functools.lru_cache(maxsize=None)
def large_sums_problem():
    """(16, 64, 2048): every |element| its row's maximum but one per row of x at 2 / 127 of it, every other channel of w
    negated: odd sums beyond +-2^24, which (float)acc has to round -- after four K ranges were added exactly."""
    rng = np.random.default_rng(11)
    x = np.where(rng.random((16, 2048)) < 0.05, -1.5, 1.5).astype(np.float32) * rng.uniform(0.5, 2, (16, 1)).astype(np.float32)
    w = np.where(rng.random((64, 2048)) < 0.05, -0.25, 0.25).astype(np.float32) * rng.uniform(0.5, 2, (64, 1)).astype(np.float32)
    x[0], w[0] = 1.5, 0.25
    x[:, 5] *= np.float32(2.0 / 127.0)
    w[::2] = -w[::2]
    xq, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    inexact = acc.astype(np.float32).astype(np.int64) != acc
    assert inexact.sum() > 250 and inexact[acc > 1 << 24].sum() > 25 and inexact[acc < -(1 << 24)].sum() > 25
    bias = rng.uniform(-4, 4, 64).astype(np.float32)
    return Problem(xq, rx, w, qw, rw, bias, out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


def want(p, bias, relu, out8):
    """The reference of a Problem: fp32 y, or the int8 bytes under its output scales."""
    if p.w is not None:   # the complete reference, from the fp32 weight (one channel: twice, see int_sums)
        w, b = (p.w, p.bias) if p.w.shape[0] != 1 else (np.concatenate([p.w, p.w]), np.concatenate([p.bias, p.bias]))
        return Q.qlinear_s8_ref(p.xq, p.rx, w, b if bias else None, relu, p.so if out8 else None)[:, :p.w.shape[0]].copy()
    y = R.epilogue_ref(p.acc, p.rx, p.rw, p.bias if bias else None, relu)   # a caller-made image: the same two steps on its sums
    return Q.requant_ref(y, p.so) if out8 else y
