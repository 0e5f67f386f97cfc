"""The 4-bit-weight small-batch layer (libmmult_hip_q4d.so, include/mmult_hip_q4d.h) as the tests see it.  numpy only.  (Shared
test code: see tests/bitcmp.py.)

What is new is restated here: the 4-bit quantiser (q4_scale_of_amax, quantize4_ref: csrc_q4d/quant_rules_s4.hpp), the packed
layout (pack_ref, unpack_ref, layout), the plan (plan(): tests/qdecode_ref.py's with the halved weight bytes and the 65536-k
ceiling) and the descriptor window.  The numeric contract is INHERITED: want() is the two steps tests/qchain_ref.py's
qlinear_s8_ref takes behind its quantiser -- qlinear_ref.epilogue_ref on the exact int32 sums, then qchain_ref.requant_ref -- on
the UNPACKED int8 image, with the channels' factors the image came with.  The sums are numpy's own (float64 products of
integers below 2^53: exact), so nothing here needs a compiled helper.

Also here: the tables tests/test_gpu_q4decode.py runs -- cases() and wide_deep_cases(), the second at the grids, split counts
and row counts the first stops short of -- (tests/test_q4d_coverage.py holds the classes they promise, on the CPU) and their
inputs, ceiling_problem() among them: ranges of exactly MAX_RANGE_K k that end with the accumulator at +2^30."""
import collections
import functools

import numpy as np

import qchain_ref as Q
import qdecode_ref as D
import qlinear_ref as R

STRIP, SLICE, HALF, MAX_ROWS = 128, 128, 64, 16
MAX_RANGE_K = 65536   # MMH_Q4D_MAX_RANGE_K


# ---- the quantiser ----------------------------------------------------------------------------------------------------------
def q4_scale_of_amax(amax):
    """scale4_of_amax in float32: 7 / amax; 1 when amax is not above 0; clamped to FLT_MAX."""
    a = np.float32(amax)
    if not a > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        s = np.float32(7.0) / a
    return s if s <= R.F32_MAX else R.F32_MAX


def quantize4_ref(w):
    """(q int8 like w in -7 .. 7, scale float32 per row, inv_scale float32 per row) of a float32 (out, in) weight: per row the
    abs-max over the FINITE elements, then clamp(rint(fl(v * s)), -7, 7), half to even; NaN -> 0, +-inf -> +-7."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    a = np.abs(w)
    a = np.where(np.isfinite(a), a, np.float32(0))
    s = np.array([q4_scale_of_amax(r.max() if r.size else 0.0) for r in a], np.float32)
    with np.errstate(all="ignore"):
        t = w * s[:, None]
        t = np.where(np.isnan(w), np.float32(0), t)
        r = np.fmin(np.fmax(np.rint(t), np.float32(-7)), np.float32(7))
        inv = np.float32(1.0) / s
    assert t.dtype == np.float32
    q = np.empty(w.shape, np.int8)
    q[...] = r
    return q, s, inv


# ---- the packed image -------------------------------------------------------------------------------------------------------
def layout(out, in_):
    """(pitch_n, packed_rows, bytes) as mmh_q4d_weight_layout gives them."""
    pitch, rows = (out + 15) & ~15, HALF * -(-in_ // SLICE)
    return pitch, rows, pitch * rows


def pack_ref(W):
    """uint8 (64 * ceil(in / 128), n) of an int8 image W (in, n) with values in -8 .. 7:
    P[64 s + r][j] = (W[128 s + r][j] & 15) | ((W[128 s + 64 + r][j] & 15) << 4), W[k] = 0 for k >= in."""
    W = np.asarray(W, np.int8)
    assert W.ndim == 2 and (W.size == 0 or (W.min() >= -8 and W.max() <= 7))
    in_, n = W.shape
    slices = -(-in_ // SLICE)
    full = np.zeros((slices * SLICE, n), np.uint8)
    full[:in_] = W.view(np.uint8) & 15
    full = full.reshape(slices, 2, HALF, n)
    return (full[:, 0] | (full[:, 1] << 4)).reshape(slices * HALF, n)


def unpack_ref(P, in_):
    """The int8 image (in, n) of a packed one: pack_ref's inverse (two's-complement nibbles)."""
    P = np.asarray(P, np.uint8)
    slices, n = P.shape[0] // HALF, P.shape[1]
    assert P.shape[0] == HALF * -(-in_ // SLICE)
    p = P.reshape(slices, 1, HALF, n)
    nib = np.concatenate([p & 15, p >> 4], 1).reshape(slices * SLICE, n).astype(np.int16)
    return np.where(nib >= 8, nib - 16, nib).astype(np.int8)[:in_]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def int_sums(xq, W):
    """acc[i][j] = sum_k xq[i][k] * W[k][j], int32, exact (|sum| < 2^53 in float64)."""
    acc = np.asarray(xq, np.float64) @ np.asarray(W, np.float64)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc.astype(np.int32)


def want(xq, rx, P, in_, rw, bias=None, relu=False, so=None):
    """The layer on int8 rows xq (rows, in), their factors rx, a packed image P (packed rows, out), the channels' factors rw:
    fp32 y, or int8 under the output scales so.  qlinear_s8_ref's arithmetic on the unpacked image."""
    y = R.epilogue_ref(int_sums(xq, unpack_ref(P, in_)), np.asarray(rx, np.float32), np.asarray(rw, np.float32), bias, relu)
    return y if so is None else Q.requant_ref(y, so)


# ---- mmh_q4d_linear_plan in Python ------------------------------------------------------------------------------------------
def plan(rows, out, in_, out8=False, ldo=0, o_mod16=0, splits=0, cus=256):
    """(text, work bytes, splits, k_len) as mmh_q4d_linear_plan gives them; None where it refuses a forced split count for an
    empty range, "long" where it refuses it for a range above MAX_RANGE_K.  qdecode_ref.plan with two changes: the weight is
    in * out / 2 bytes in the traffic cap, and no range exceeds MAX_RANGE_K."""
    ldo = ldo or (((out + 15) & ~15) if out8 else out)
    strips, slices = -(-out // STRIP), -(-in_ // SLICE)
    wide = (ldo % 4 == 0 and o_mod16 % 4 == 0) if out8 else (ldo % 4 == 0 and o_mod16 == 0)
    finish = -(-out // D.FINISH_COLS) * rows
    tail = f"qdecode_finish_kernel<{'true' if out8 else 'false'}>"
    stores = "wide stores" if wide else "single stores"
    if in_ == 0:
        return f"{tail} alone, {finish} workgroups, {stores}", 0, 0, 0
    if splits > 0:
        if not D.valid_splits(in_, splits):
            return None
        k_len = D.ranges(in_, splits)[0]
        if k_len > MAX_RANGE_K:
            return "long"
    else:
        want_ = -(-D.WG_NUM * cus // (D.WG_DEN * strips))
        cap = in_ * D.TRAFFIC_NUM // (16 * rows * D.TRAFFIC_DEN)
        least = -(-slices // (MAX_RANGE_K // SLICE))
        splits = max(1, least, min(want_, cap, slices))
        per = -(-slices // splits)
        k_len, splits = per * SLICE, -(-slices // per)
    return (f"q4decode_partial_kernel, {strips} strips x {splits} splits of {k_len} k; {tail}, {finish} workgroups, {stores}",
            D.work_bytes(splits, rows, out), splits, k_len)


def window_ok(ldq, pitch_n, in_):
    """The 2 GiB descriptor window: x as the int8 layer holds it; the packed image and the slices the ring requests behind it."""
    return 256 * ldq + in_ < D.WINDOW and (layout(1, in_)[1] + 128) * pitch_n + 256 < D.WINDOW


def largest_pitch_n(in_):
    return (D.WINDOW - 256 - 1) // (layout(1, in_)[1] + 128) & ~3


def furthest_slice(nk):
    """The last slice q4decode_partial_kernel's two-stage ring requests in a range of nk slices: 0 and 1 ahead of the loop,
    then one behind each slice consumed, and the loop consumes in pairs -- nk + 2 behind an odd count, nk + 1 behind an even."""
    return nk + 2 if nk % 2 else nk + 1


def weight_offsets(in_, pitch_n, splits=1):
    """Per K range of a forced split count: (ext_w of strip 0, the largest scalar offset -- the kernel's `int` product
    kt * 64 * pitch_n --, the largest unsigned sum voff_w + soff, with voff_w <= 63 pitch_n + 112 and 16 bytes read)."""
    k_len, rs = D.ranges(in_, splits)
    got = []
    for begin, end in rs:
        nk = -(-(end - begin) // SLICE)
        soff = furthest_slice(nk) * HALF * pitch_n
        got.append(((HALF * nk - 1) * pitch_n + STRIP, soff, soff + (HALF - 1) * pitch_n + STRIP - 1))
    return got


# ---- the GPU tables ---------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 15, 16)
INS = (1, 63, 64, 65, 127, 128, 129, 384, 385, 1153)
OUTS = (1, 16, 17, 127, 128, 129, 257, 273)
FORCED = (1, 2, 3)
PACK_OUTS, PACK_INS = (1, 17, 128, 129, 273), (1, 63, 64, 65, 127, 128, 129, 385)
PLAN_SHAPE = (16, 256, 8192)    # splits = 0 here: the plan splits on the device's CU count
DEEP = (16, 130, 11008, 1)      # rows, out, in, forced ranges: 86 slices through the ring in one range
EQUAL_SHAPES = ((16, 256, 512), (5, 130, 257), (1, 128, 128))   # against qlinear_decode on the int8 image of the same values


@functools.lru_cache(maxsize=None)
def cases():
    """qdecode_ref's Case rows.  Every `in` at every forced split count that leaves no range empty (rows and out rotating), then
    every out at two row counts behind the deeper shapes, then 127 columns on the two layouts whose stores are wide although out
    is no multiple of 4.  weight "qweight": QWeight4's own image of a real weight; "image": a
    caller-made image at its own pitch and base.  Layouts and epilogues rotate as in qdecode_ref.cases()."""
    out, i = [], 0
    for in_ in INS:
        for s in FORCED:
            if D.valid_splits(in_, s):
                out.append(D._case(i, ROWS[i % 4], OUTS[(3 * i + 1) % len(OUTS)], in_, s))
                i += 1
    deep = [(129, 2), (385, 2), (1153, 3), (384, 3), (1153, 2), (384, 2)]
    for j, n in enumerate(OUTS):
        for r in (0, 2):
            in_, s = deep[i % len(deep)]
            out.append(D._case(i, ROWS[(j + r) % 4], n, in_, s))
            i += 1
    # ldy = out + 1 at a 16-byte base, ldyq = out + 5 at a 4-byte base: whole rows of dwords, the last three columns one by one
    for rows, in_ in ((16, 384), (1, 129)):
        out.append(D._case(i, rows, 127, in_, 2)._replace(y=D.Y_LAYOUTS.index((1, 0)), yq=D.YQ_LAYOUTS.index((5, 0))))
        i += 1
    # both weight kinds at a last slice that ends in its low half, one element into its high half, and inside it
    for rows, n, in_, kind in ((2, 17, 65, "image"), (15, 129, 127, "image"), (16, 16, 64, "qweight")):
        out.append(D._case(i, rows, n, in_, 1)._replace(weight=kind))
        i += 1
    return tuple(out)


case_id = D.case_id

# ---- the second table: where the kernel differs from the int8 one it was copied from -----------------------------------------
WIDE_OUTS, WIDE_ROWS, SHALLOW = D.WIDE_OUTS, D.WIDE_ROWS, D.SHALLOW   # the finish grid: qdecode_ref's, behind in <= 385
MANY_RANGES_INS = (1153, 1280)                                         # forced counts above 3, up to one range per slice
OWN_CHOICE = ((1, 130, 8192), (2, 130, 8192), (1, D.FINISH_COLS + 1, 4224))   # splits == 0: one slice per range at 256 CUs
WIDE_DEEP = ((4224, 1), (11008, 2))                                    # (in, forced ranges) at 16 rows, 130 columns: 33, 43 slices
LADDER = (130, 257, 2)                                                 # (out, in, forced ranges) at every row count 1 - 16
RESERVE_SHAPE = (257, 1153)                                            # (out, in) whose own split count varies with the rows


@functools.lru_cache(maxsize=None)
def wide_deep_cases():
    """qdecode_ref.wide_deep_cases() for the packed image: the finish grid (every WIDE_OUTS at two row counts behind two to four
    shallow ranges, then 1027 columns on the two layouts whose stores are wide although out is no multiple of 4), every forced
    count above 3 that leaves no range of MANY_RANGES_INS empty, the plan's own choice where it is one slice per range (every
    range consumes a zero second stage), the deep ranges (the second on a caller-made image) and LADDER at every row count.
    Layouts, weights and epilogues rotate as in cases()."""
    out = []

    def add(rows, n, in_, s, **fixed):
        out.append(D._case(len(out), rows, n, in_, s)._replace(**fixed))

    for j, n in enumerate(WIDE_OUTS):
        for r in (0, 1):
            add(WIDE_ROWS[(2 * j + r) % len(WIDE_ROWS)], n, *SHALLOW[len(out) % len(SHALLOW)])
    # ldy = out + 1 at a 16-byte base, ldyq = out + 5 at a 4-byte base: whole rows of dwords, the last three columns one by one
    add(16, D.FINISH_COLS + 3, 257, 2, y=D.Y_LAYOUTS.index((1, 0)), yq=D.YQ_LAYOUTS.index((5, 0)))
    add(1, D.FINISH_COLS + 3, 129, 2, y=D.Y_LAYOUTS.index((1, 0)), yq=D.YQ_LAYOUTS.index((5, 0)))
    for in_ in MANY_RANGES_INS:
        for s in range(FORCED[-1] + 1, -(-in_ // SLICE) + 1):
            if D.valid_splits(in_, s):
                add(ROWS[len(out) % 4], OUTS[len(out) % len(OUTS)], in_, s)
    for rows, n, in_ in OWN_CHOICE:
        add(rows, n, in_, 0)
    for j, (in_, s) in enumerate(WIDE_DEEP):
        add(MAX_ROWS, 130, in_, s, weight="image" if j == 1 else "qweight")
    for rows in range(1, MAX_ROWS + 1):
        add(rows, *LADDER)
    return tuple(out)


def range_slices(c, cus=256):
    """[(slices of the range, is it the last one) ...] of a case's K ranges: what the two-stage ring goes through per workgroup.
    An odd count consumes its second stage as zeros."""
    _, _, splits, k_len = plan(c.rows, c.out, c.in_, splits=c.splits, cus=cus)
    ends = [min((s + 1) * k_len, c.in_) - s * k_len for s in range(splits)]
    return [(-(-kr // SLICE), s == splits - 1) for s, kr in enumerate(ends)]


# xq int8 (rows, in); rx; w: the fp32 weight or None; W: the int8 image (in, out) in -8 .. 7; rw; bias; so; acc
Problem = collections.namedtuple("Problem", "xq rx w W rw bias so acc")


def every_half_slice_moves_the_sums(xq, W, acc):
    """Each 64-k HALF of each 128-k slice contributes a non-zero amount to at least 90 % of the sums (one sum: to it): a half
    that is dropped, swapped with its neighbour's nibbles or read from the wrong slice shows in the fp32 output, which keeps
    every bit of a sum below 2^24."""
    assert np.abs(acc).max(initial=0) < 1 << 24
    for k0 in range(0, xq.shape[1], HALF):
        part = int_sums(xq[:, k0:k0 + HALF], W[k0:k0 + HALF])
        assert float((part != 0).mean()) >= 0.9, (xq.shape, W.shape, k0)
        # ... and swapping the halves of a slice would change them (the two halves differ)
    for k0 in range(0, xq.shape[1] - HALF, SLICE):
        n = min(HALF, xq.shape[1] - k0 - HALF)
        assert not np.array_equal(W[k0:k0 + n], W[k0 + HALF:k0 + HALF + n])


def _finish(xq, rx, w, W, rw, rng):
    bias = rng.uniform(-4, 4, W.shape[1]).astype(np.float32)
    acc = int_sums(xq, W)
    if xq.shape[1]:
        every_half_slice_moves_the_sums(xq, W, acc)
    return Problem(xq, rx, w, W, rw, bias, D.out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


def _rows(rng, rows, in_):
    """int8 rows over the full range with -128 planted, no zeros in the last column (a lone k tail carries the products)."""
    xq = D.int8_full_range(rng, (rows, in_))
    if in_:
        xq[:, -1] = np.where(xq[:, -1] == 0, 127, xq[:, -1])
    return xq, rng.uniform(0.01, 0.05, rows).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(rows, out, in_):
    """A real weight: w ~ U(-0.5, 0.5), the last column of every row plus or minus the row's maximum, quantised by
    quantize4_ref; rows over the full int8 range."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 4)
    xq, rx = _rows(rng, rows, in_)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    if in_:
        w[:, -1] = np.abs(w).max(axis=1) * rng.choice(np.array([-1, 1], np.float32), out)
    q, _, rw = quantize4_ref(w)
    return _finish(xq, rx, w, np.ascontiguousarray(q.T), rw, rng)


@functools.lru_cache(maxsize=None)
def image_problem(rows, out, in_):
    """An image no quantiser makes: every nibble value -8 .. 7 in both nibble positions (zeros rare: most become -8), the last
    row of x all -128, arbitrary positive factors."""
    rng = np.random.default_rng(rows * 5 + out * 11 + in_ + 44)
    xq, rx = _rows(rng, rows, in_)
    xq[-1] = -128
    W = rng.integers(-8, 8, (in_, out), dtype=np.int8)
    W = np.where((W == 0) & (rng.random(W.shape) < 0.9), np.int8(-8), W).astype(np.int8)
    rw = rng.uniform(0.01, 0.04, out).astype(np.float32)
    return _finish(xq, rx, None, W, rw, rng)


@functools.lru_cache(maxsize=None)
def large_sums_problem():
    """(16, 64, 24576): |x| = 127 or 128 and W = 7 or -8 nearly everywhere with the signs of a row and a channel constant but
    for a few percent: odd sums beyond +-2^24, which (float)acc has to round -- after four K ranges were added exactly."""
    rng = np.random.default_rng(13)
    rows, out, in_ = 16, 64, 24576
    sx = np.where(rng.random((rows, 1)) < 0.5, -1, 1) * np.where(rng.random((rows, in_)) < 0.03, -1, 1)
    xq = np.where(sx < 0, -128, 127).astype(np.int8)
    sw = np.where(rng.random((1, out)) < 0.5, -1, 1) * np.where(rng.random((in_, out)) < 0.03, -1, 1)
    W = np.where(sw < 0, -8, 7).astype(np.int8)
    xq[:, 5] = 1
    rx = rng.uniform(0.01, 0.05, rows).astype(np.float32)
    rw = rng.uniform(0.01, 0.04, out).astype(np.float32)
    acc = int_sums(xq, W)
    inexact = acc.astype(np.float32).astype(np.int64) != acc
    assert inexact.sum() > 250 and inexact[acc > 1 << 24].sum() > 25 and inexact[acc < -(1 << 24)].sum() > 25
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    return Problem(xq, rx, None, W, rw, bias, D.out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


CEILING_SHAPE = (16, 130)   # rows, out: two strips, the second of 2 columns
CEILING_CELLS = 4           # rows {0, 1} x channels {0, 1}: the saturated sums, all that the half-slice check may leave out


def partial_of_range(xq, W, begin, end):
    """What q4decode_partial_kernel writes for the K range [begin, end): its int32 accumulator holds 16 x the sum (the
    nibbles arrive as int8 bytes 16 W), then `acc >> 4`, ARITHMETIC.  The accumulator has to fit: that is MAX_RANGE_K."""
    acc16 = 16 * (np.asarray(xq[:, begin:end], np.float64) @ np.asarray(W[begin:end], np.float64))
    assert np.abs(acc16).max(initial=0) <= 1 << 30, (begin, end)   # (+2^30 from -128 x -8; the negative extreme is smaller)
    return acc16.astype(np.int32) >> 4


@functools.lru_cache(maxsize=None)
def ceiling_problem(in_):
    """(16, 130, in_) with in_ a multiple of MAX_RANGE_K, to run in ranges of exactly MAX_RANGE_K k (512 slices): rows over
    the full int8 range with row 0 all -128 and row 1 all 127, a caller-made image over -8 .. 7 with channel 0 all -8 and
    channel 1 all 7; factors, bias and output scales as in image_problem.  In every range the accumulator of cell (0, 0) is
    +2^30 exactly -- all the contract admits -- and that of cell (1, 0) is -1 065 353 216; the shifted accumulator is the sum;
    every other sum keeps all its bits in fp32, and each half of each slice moves them."""
    rows, out = CEILING_SHAPE
    assert in_ > 0 and in_ % MAX_RANGE_K == 0
    rng = np.random.default_rng(7)
    xq = D.int8_full_range(rng, (rows, in_))
    xq[0], xq[1] = -128, 127
    W = rng.integers(-8, 8, (in_, out), dtype=np.int8)
    W[:, 0], W[:, 1] = -8, 7
    rx = rng.uniform(0.01, 0.05, rows).astype(np.float32)
    rw = rng.uniform(0.01, 0.04, out).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    acc = int_sums(xq, W)
    total = np.zeros((rows, out), np.int64)
    for begin in range(0, in_, MAX_RANGE_K):
        part = partial_of_range(xq, W, begin, begin + MAX_RANGE_K)
        assert 16 * int(part[0, 0]) == 1 << 30 and 16 * int(part[1, 0]) == -1065353216, (begin, part[:2, :2])
        assert np.array_equal(part, int_sums(xq[:, begin:begin + MAX_RANGE_K], W[begin:begin + MAX_RANGE_K])), begin
        total += part
    assert np.array_equal(total, acc)
    plain = np.ones((rows, out), bool)
    plain[:2, :2] = False
    assert plain.size - int(plain.sum()) == CEILING_CELLS
    assert np.abs(acc[plain]).max() < 1 << 24 and np.abs(acc[~plain]).min() > 1 << 24
    # each 64-k half of each slice, at once: (halves, rows, 64) @ (halves, 64, out) in float32 (|sum| <= 64 * 1024: exact)
    halves = in_ // HALF
    moved = np.matmul(xq.reshape(rows, halves, HALF).transpose(1, 0, 2).astype(np.float32), W.reshape(halves, HALF, out).astype(np.float32))
    share = (moved[:, plain] != 0).mean(axis=1)
    assert share.shape == (halves,) and float(share.min()) >= 0.9, (int(share.argmin()), float(share.min()))
    low, high = W.reshape(in_ // SLICE, 2, HALF, out)[:, 0], W.reshape(in_ // SLICE, 2, HALF, out)[:, 1]
    assert (low != high).any(axis=(1, 2)).all()   # swapping the halves of any slice would change the sums
    return Problem(xq, rx, None, W, rw, bias, D.out_scales(R.epilogue_ref(acc, rx, rw, bias, False)), acc)


def want_of(p, bias, relu, out8):
    """The reference of a Problem: through its PACKED image (pack_ref, then want's unpacking)."""
    return want(p.xq, p.rx, pack_ref(p.W), p.xq.shape[1], p.rw, p.bias if bias else None, relu, p.so if out8 else None)


def special_weight(out, in_, rng):
    """A weight that meets every special rule of the quantiser, one per row from row 0 on (out >= 5, in >= 4): all zero, a NaN,
    +-inf, a maximum whose scale overflows (1e-39: the quotient is clamped to FLT_MAX), all -max."""
    w = rng.uniform(-1, 1, (out, in_)).astype(np.float32)
    w[0] = 0
    w[1, 1] = np.nan
    w[2, 0], w[2, 2] = np.inf, -np.inf
    w[3] = 0
    w[3, 3] = np.float32(1e-39)
    w[4] = -2.5
    return w
