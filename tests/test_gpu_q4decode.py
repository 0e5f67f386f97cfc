"""The 4-bit-weight small-batch layer (libmmult_hip_q4d.so: q4_row_amax_kernel, q4_pack_weight_kernel, q4decode_partial_kernel and
qdecode_finish_kernel<false / true>) bit for bit against tests/q4_ref.py, on both output forms of every case.

run() calls mmh_q4d_linear itself, on operands laid out as a caller may, as tests/test_gpu_qdecode.py does for the int8 layer:
x's int8 rows at a pitch of `in` rounded up to 4 plus 0 - 12 bytes and a base 0 - 12 bytes past a 16-byte boundary, every byte
beyond `in`, between the rows and in the (16 - rows) rows' worth of memory behind the last row poisoned with 0x55; a weight that
is QWeight4's own image or a caller-made one (its own pitch and base, pad columns poisoned); the output inside a buffer of 0x55
that is compared WHOLE with what the reference says it holds afterwards; the workspace pre-filled with 0x7f and followed by 64
guard bytes.  The launch text is held to the Python plan at the device's CU count.  tests/q4_ref.py has the two case tables --
cases(), thorough in the small, and wide_deep_cases(): outputs wider than one finish workgroup, up to one K range per slice,
deep ranges, every row count --, tests/test_q4d_coverage.py what they promise.  Two calls run ranges of exactly
MMH_Q4D_MAX_RANGE_K k, where the accumulator ends at +2^30; three more run operands at the edge of the descriptor window (the
largest pitch_n and ldq shape_status4 admits), built on the device inside one 1.07 GB buffer of 0x55; the Python layer's timer,
its cached workspace under QWeight4's own plan and from_image's refusals follow at the end."""
import numpy as np
import pytest

import q4_ref as F
import qdecode_ref as D
from bitcmp import first_difference, same_bits

pytestmark = pytest.mark.gpu

POISON, WORK_FILL = 0x55, 0x7F


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_rows(xq, pad, off):
    """(keep-alive tensor, pointer, ldq) of x's rows in poisoned memory; 16 rows' worth of bytes lie behind the base."""
    import torch
    rows, in_ = xq.shape
    ldq = ((in_ + 3) & ~3) + pad
    host = np.full(16 + off + D.MAX_ROWS * ldq + 64, POISON, np.uint8)
    host[16 + off:16 + off + rows * ldq].reshape(rows, ldq)[:, :in_] = xq.view(np.uint8)
    flat = torch.from_numpy(host).cuda()
    return flat, flat.data_ptr() + 16 + off, ldq


def device_image(P, pad, off):
    """(keep-alive tensor, the image as a strided uint8 view, pitch_n) of a caller-made packed image in poisoned memory."""
    import torch
    prow, out = P.shape
    pitch = ((out + 3) & ~3) + pad
    host = np.full(16 + off + prow * pitch + 64, POISON, np.uint8)
    host[16 + off:16 + off + prow * pitch].reshape(prow, pitch)[:, :out] = P
    flat = torch.from_numpy(host).cuda()
    return flat, torch.as_strided(flat, (prow, out), (pitch, 1), 16 + off), pitch


class Weight:
    """The weight operands of a Problem on the device: QWeight4's own image of p.w, or a caller-made image of p.W adopted by
    QWeight4.from_image."""

    def __init__(self, p, kind, i=0):
        from how_to_optimize_gemm_amd import q8
        in_, out = p.W.shape
        if kind == "qweight":
            assert p.w is not None
            self.qweight = q8.QWeight4(dev(p.w))
        else:
            self.keep, view, _ = device_image(F.pack_ref(p.W), (0, 4, 8, 12)[i % 4], (0, 4, 8, 12)[(i // 4 + 1) % 4])
            self.qweight = q8.QWeight4.from_image(view, dev(p.rw), out, in_)
        self.ptr, _, self.rw = self.qweight._ptrs
        self.pitch = self.qweight.pitch

    def close(self):
        self.qweight.close()


def run(p, weight, bias, relu, out8, splits, cus, x_pad=0, x_off=0, o_pad=0, o_off=0, x_rows=None):
    """One mmh_q4d_linear call on the layouts above; asserts the status, the launch text, the whole output buffer, the
    workspace's guard.  Returns the launch text.  x_rows: device_rows' triple where the caller has laid x out itself."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    L = q8.lib_q4d()
    rows, in_ = p.xq.shape
    out = p.W.shape[1]
    item = 1 if out8 else 4
    ldo = out + o_pad
    keep_x, pxq, ldq = x_rows or device_rows(p.xq, x_pad, x_off)
    rx, so, db = dev(p.rx), dev(p.so), dev(p.bias)
    planned = F.plan(rows, out, in_, out8, ldo, (item * o_off) % 16, splits, cus)
    assert planned not in (None, "long"), "the table forces a split count the plan refuses"
    text, work_bytes, _, _ = planned
    work = torch.full((work_bytes + 64,), WORK_FILL, dtype=torch.uint8, device="cuda")
    front = 64 + item * o_off
    expect = np.full(front + rows * ldo * item + 64, POISON, np.uint8)
    buf = torch.from_numpy(expect.copy()).cuda()
    po = buf.data_ptr() + front
    rc = L.mmh_q4d_linear(0, rows, out, in_, pxq, ldq, rx.data_ptr(), weight.ptr, weight.pitch, weight.rw, db.data_ptr() if bias else None,
                          H.ACT_RELU if relu else H.ACT_NONE, so.data_ptr() if out8 else None, None if out8 else po, 0 if out8 else ldo,
                          po if out8 else None, ldo if out8 else 0, work.data_ptr(), work_bytes, splits,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == H.OK, (rc, L.mmh_q4d_last_error())
    launched = q8.last_launch_q4d()
    torch.cuda.synchronize()
    assert launched == text, (launched, text)
    want = F.want_of(p, bias, relu, out8)
    got = buf.cpu().numpy()
    window = got[front:front + rows * ldo * item].reshape(rows, ldo * item)[:, :out * item]
    got_values = np.ascontiguousarray(window).view(np.int8 if out8 else np.float32)
    if out8:
        assert np.array_equal(got_values, want), (launched, int((got_values != want).sum()), np.argwhere(got_values != want)[:4])
    else:
        assert same_bits(got_values, want), (launched, first_difference(got_values, want))
    expect[front:front + rows * ldo * item].reshape(rows, ldo * item)[:, :out * item] = np.ascontiguousarray(want).view(np.uint8).reshape(rows, -1)
    assert np.array_equal(got, expect), (launched, "wrote outside the rows x out window", np.argwhere(got != expect)[:4])
    assert bool((work[work_bytes:] == WORK_FILL).all()), (launched, "wrote behind the plan's work_bytes")
    return launched


def run_both(p, weight, bias, relu, splits, cus, x_pad=0, x_off=0, y=0, yq=0, x_rows=None):
    a = run(p, weight, bias, relu, False, splits, cus, x_pad, x_off, *D.Y_LAYOUTS[y], x_rows=x_rows)
    b = run(p, weight, bias, relu, True, splits, cus, x_pad, x_off, *D.YQ_LAYOUTS[yq], x_rows=x_rows)
    return a, b


# ---- 1. the packer ----------------------------------------------------------------------------------------------------------
def check_packed(qw, w):
    """QWeight4(w)'s image, scales and reciprocals against pack_ref(quantize4_ref(w)): every byte of every row up to the pitch."""
    out, in_ = w.shape
    q, s, inv = F.quantize4_ref(w)
    pitch, prow, nbytes = F.layout(out, in_)
    assert (qw.pitch, tuple(qw.p.shape), qw.nbytes) == (pitch, (prow, pitch), nbytes)
    want = np.zeros((prow, pitch), np.uint8)
    want[:, :out] = F.pack_ref(np.ascontiguousarray(q.T))
    assert np.array_equal(qw.p.cpu().numpy(), want), np.argwhere(qw.p.cpu().numpy() != want)[:4]
    assert same_bits(qw.scale.cpu().numpy(), s) and same_bits(qw.inv_scale.cpu().numpy(), inv)
    assert np.array_equal(qw.unpack().cpu().numpy()[:, :out], q.T) and not qw.unpack().cpu().numpy()[:, out:].any()
    assert tuple(qw.unpack().shape) == (in_, pitch)


@pytest.mark.parametrize("out", F.PACK_OUTS)
def test_the_packer_is_the_reference_at_every_tail(out):
    from how_to_optimize_gemm_amd import q8
    for in_ in F.PACK_INS:
        w = np.random.default_rng(out * 1000 + in_).uniform(-2, 2, (out, in_)).astype(np.float32)
        check_packed(q8.QWeight4(dev(w)), w)


def test_the_packer_on_a_strided_weight_special_values_and_no_columns():
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(9)
    big = rng.uniform(-3, 3, (129, 200)).astype(np.float32)
    check_packed(q8.QWeight4(dev(big)[:, 3:132]), big[:, 3:132])            # row stride 200, a base that is not 16-byte aligned
    w = F.special_weight(17, 129, rng)                                        # zeros, NaN, +-inf, a scale that overflows, -max
    qw = q8.QWeight4(dev(w))
    check_packed(qw, w)
    assert qw.scale[0].item() == 1.0 and qw.scale[3].item() == float(np.finfo(np.float32).max)
    assert int(qw.unpack().min()) == -7 and int(qw.unpack().max()) == 7      # the library never produces -8
    empty = q8.QWeight4(torch.zeros((5, 0), device="cuda"))                   # in == 0: the scales are 1, no image
    assert tuple(empty.p.shape) == (0, 16) and empty.nbytes == 0
    assert bool((empty.scale == 1).all()) and bool((empty.inv_scale == 1).all())
    y = q8.qlinear_decode(q8.QRows(torch.zeros((2, 0), dtype=torch.int8, device="cuda"), torch.ones(2, device="cuda")), empty,
                          torch.arange(5, dtype=torch.float32, device="cuda"))
    assert y.cpu().numpy().tolist() == [[0, 1, 2, 3, 4]] * 2 and "alone" in q8.last_launch_q4d()


# ---- 2. the kernel, the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(F.cases())), ids=[F.case_id(c) for c in F.cases()])
def test_every_case_of_the_table_is_the_contract_on_both_outputs(index, cus):
    c = F.cases()[index]
    p = (F.problem if c.weight == "qweight" else F.image_problem)(c.rows, c.out, c.in_)
    w = Weight(p, c.weight, index)
    try:
        run_both(p, w, c.bias, c.relu, c.splits, cus, c.x_pad, c.x_off, c.y, c.yq)
    finally:
        w.close()


@pytest.mark.parametrize("index", range(len(F.wide_deep_cases())), ids=[F.case_id(c) for c in F.wide_deep_cases()])
def test_every_case_of_the_second_table_is_the_contract_on_both_outputs(index, cus):
    """More than one finish workgroup per row (this library's own build of the finish kernels, blockIdx.x > 0), up to 33
    strips, up to one K range per slice -- the plan's own choice at one and two rows included, whatever it is on this device:
    every range then consumes a zero second stage --, ranges of 33 and 43 slices, every row count 1 - 16."""
    c = F.wide_deep_cases()[index]
    p = (F.problem if c.weight == "qweight" else F.image_problem)(c.rows, c.out, c.in_)
    w = Weight(p, c.weight, index)
    try:
        run_both(p, w, c.bias, c.relu, c.splits, cus, c.x_pad, c.x_off, c.y, c.yq)
    finally:
        w.close()


# ---- 2b. the 65536-k ceiling of a range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_,ranges", [(F.MAX_RANGE_K, 1), (2 * F.MAX_RANGE_K, 2)], ids=["one-range", "two-ranges"])
def test_ranges_of_exactly_65536_k_fill_the_accumulator_to_2_to_the_30(in_, ranges, cus):
    """F.ceiling_problem: every range is MMH_Q4D_MAX_RANGE_K long, 512 slices; the accumulator of cell (0, 0) ends at +2^30
    exactly (x = -128 against W = -8), that of cell (1, 0) at -1 065 353 216, and `acc >> 4` has to be arithmetic.  With two
    ranges the finish kernel adds two partials of 2^26.  One k more in a forced range is refused (no launch): the run sits ON
    the boundary."""
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode4_plan(16, 130, F.MAX_RANGE_K + 1, splits=1, cu_count=cus)
    assert e.value.status == H.ERR_INVALID_ARG and "65536" in str(e.value)
    assert F.plan(16, 130, in_, splits=ranges, cus=cus)[2:] == (ranges, F.MAX_RANGE_K)
    p = F.ceiling_problem(in_)
    w = Weight(p, "image", 6)
    try:
        for launched in run_both(p, w, True, False, ranges, cus, 4, 8, 2, 2):
            assert f"2 strips x {ranges} splits of {F.MAX_RANGE_K} k" in launched
    finally:
        w.close()


def test_the_plans_own_choice_splits_on_the_devices_cu_count(cus):
    rows, out, in_ = F.PLAN_SHAPE
    _, _, splits, k_len = F.plan(rows, out, in_, cus=cus)
    assert splits > 1 and k_len < in_, (cus, splits, k_len)
    p = F.problem(rows, out, in_)
    w = Weight(p, "qweight")
    try:
        for launched in run_both(p, w, True, False, 0, cus, 4, 8, 0, 0):
            assert f"x {splits} splits of {k_len} k" in launched
    finally:
        w.close()


@pytest.mark.parametrize("bias,relu", D.EPILOGUES, ids=["plain", "bias", "relu", "bias-relu"])
def test_bias_and_relu_all_four(bias, relu, cus):
    p = F.problem(15, 273, 385)
    assert (F.want_of(p, bias, False, False) < 0).mean() > 0.2   # ReLU has something to cut
    w = Weight(p, "qweight")
    try:
        run_both(p, w, bias, relu, 2, cus, 12, 4, 1, 1)
    finally:
        w.close()


# ---- 2c. operands at the edge of the descriptor window ----------------------------------------------------------------------
EDGE_OUT = 130
EDGE_BYTES = 16 + 12 + (F.layout(EDGE_OUT, 129)[1] - 1) * F.largest_pitch_n(129) + EDGE_OUT + 64   # the largest operand below: 1.07 GB


@pytest.fixture(scope="module")
def edge():
    """The flat 0x55 buffer the operands at the window's edge are strided views of: they are written on the device, there is
    never a host array of that size."""
    import torch
    buf = torch.full((EDGE_BYTES,), POISON, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


def edge_operand(buf, values, ld, off, rows_behind=0):
    """(keep-alive, the operand as a strided view of buf, ld) of one-byte `values` as rows of pitch ld, 16 + off bytes into
    buf; everything else of the max(its rows, rows_behind) rows' worth of bytes and 64 behind them is 0x55 (again)."""
    import torch
    rows, cols = values.shape
    end = 16 + off + max((rows - 1) * ld + cols, rows_behind * ld) + 64
    assert values.dtype.itemsize == 1 and off % 4 == 0 and ld % 4 == 0 and end <= buf.numel(), (values.shape, ld, off, buf.numel())
    buf[:end].fill_(POISON)
    view = torch.as_strided(buf, (rows, cols), (ld, 1), 16 + off)
    view.copy_(dev(values.view(np.uint8)))
    return buf, view, ld


class EdgeImage:
    """Weight's interface for a caller-made packed image of pitch `pitch` inside the edge buffer, adopted by from_image."""

    def __init__(self, buf, p, pitch, off):
        from how_to_optimize_gemm_amd import q8
        in_, out = p.W.shape
        _, view, _ = edge_operand(buf, F.pack_ref(p.W), pitch, off)
        self.qweight = q8.QWeight4.from_image(view, dev(p.rw), out, in_)
        self.ptr, _, self.rw = self.qweight._ptrs
        self.pitch = self.qweight.pitch
        assert self.pitch == pitch and self.ptr == buf.data_ptr() + 16 + off

    def close(self):
        self.qweight.close()


@pytest.mark.parametrize("splits", [0, 1])
def test_one_slice_at_the_largest_image_pitch_inside_the_window(edge, cus, splits):
    """in 1, out 130, 2 rows, pitch_n = P = 11 184 784: the largest multiple of 4 that shape_status4 admits for one slice (the
    next one is refused: tests/test_q4d_abi.py).  The image is one slice of 64 packed rows spanning 63 P + 130 bytes = 0.70 GB,
    of which 130 per packed row are written (row 0 holds k = 0 in its low nibbles; the rest of the slice is zero nibbles).

    The offsets of q4decode_partial_kernel's weight descriptor, written down before the first run.  A lane's offset is
    voff_w + soff with voff_w = r P + 16 slot, r <= 63, slot <= 7 -- at most 63 P + 112, its 16 bytes end at 63 P + 127 =
    704 641 519 -- and the scalar soff = kt 64 P, an `int` product; the extent is ext_w = (64 nk - 1) P + 128 (strip 0; 4 for
    strip 1, whose base is 128 bytes further).  One range, kr = 1, nk = 1 -- odd --, ext_w = 63 P + 128 = 704 641 520, and the
    slices issued are 0 - 3 = nk + 2:
      slice 0   offsets 0 .. 63 P + 127 < ext_w: packed rows 0 - 63, all inside the image;
      slice 1   soff 64 P = 715 826 176 >= ext_w; offsets up to 127 P + 127 = 1 420 467 695: zeros, and CONSUMED -- the second
                ring stage of an odd slice count;
      slice 2   soff 128 P = 1 431 652 352; offsets up to 191 P + 127 = 2 136 293 871 < 2^31: zeros, never consumed;
      slice 3   soff 192 P = 2 147 478 528 < 2^31 = 2 147 483 648 by 5 120 (the int product does not overflow: with one more
                ring stage, 256 P, it would); offsets 192 P .. 255 P + 127 = 2 852 120 047: above 2^31, below 2^32 -- an
                unsigned 32-bit sum that does not wrap --, all > ext_w: zeros, never consumed.
    Nothing beyond slice 0 is fetched.  x is 2 dense rows: its offsets stay below 15 ldq + 48 + 448.  The case is one the
    contract admits; every offset beyond ext_w must read zeros, and the asserts below are the arithmetic."""
    pitch, nk = F.largest_pitch_n(1), 1
    assert pitch == 11184784 and F.window_ok(4, pitch, 1) and not F.window_ok(4, pitch + 4, 1)
    ext_w = (64 * nk - 1) * pitch + 128
    assert 63 * pitch + 127 < ext_w <= 64 * pitch
    assert (nk + 2) * 64 * pitch == 2147478528 < 1 << 31 <= (nk + 3) * 64 * pitch
    assert (1 << 31) < (nk + 2) * 64 * pitch + 63 * pitch + 127 < 1 << 32
    assert F.weight_offsets(1, pitch) == [(ext_w, 2147478528, 2852120047)] and F.furthest_slice(nk) == 3
    assert F.plan(2, EDGE_OUT, 1, cus=cus)[2:] == (1, 128)
    p = F.image_problem(2, EDGE_OUT, 1)
    w = EdgeImage(edge, p, pitch, 12)
    try:
        run_both(p, w, False, True, splits, cus, 0, 4, 1, 1)
    finally:
        w.close()


@pytest.mark.parametrize("splits", [1, 2])
def test_the_largest_image_pitch_of_two_slices_inside_the_window(edge, cus, splits):
    """in 129, out 130, 16 rows, pitch_n = P = 8 388 588: the largest multiple of 4 admitted for 128 packed rows.  The image
    spans 127 P + 130 bytes = 1.065 GB, of which 130 per packed row are written.

    voff_w = r P + 16 slot, r <= 63 (its 16 bytes end at most at 63 P + 127 = 528 481 171); soff = kt 64 P;
    ext_w = (64 nk - 1) P + 128 (strip 0).  With ONE range kr = 129, nk = 2 -- even --, ext_w = 127 P + 128 = 1 065 350 804,
    and the slices issued are 0 - 3 = nk + 1:
      slice 0   offsets 0 .. 63 P + 127: packed rows 0 - 63, inside the image;
      slice 1   soff 64 P = 536 869 632; offsets .. 127 P + 127 = 1 065 350 803 < ext_w: packed rows 64 - 127, inside the image;
      slice 2   soff 128 P = 1 073 739 264 >= ext_w; offsets .. 191 P + 127: zeros, never consumed;
      slice 3   soff 192 P = 1 610 608 896 < 2^31; offsets .. 255 P + 127 = 2 139 090 067 < 2^31: zeros, never consumed.
    With TWO ranges (k_len 128) range 0 has kr = 128, nk = 1, ext_w = 63 P + 128 = 528 481 172: its slice 1 (soff 64 P >=
    ext_w) is consumed as zeros although the image's second slice lies AT those addresses -- the extent, not the memory, makes
    it zero --, and slices 2 and 3 = nk + 2 follow up to 255 P + 127 as above.  Range 1's base is 64 P further (a 64-bit
    pointer sum), kr = 1, nk = 1, ext_w = 63 P + 128: slice 0 is the image's packed rows 64 - 127, slices 1 - 3 reach
    255 P + 127 past THAT base, all beyond its extent.  x is 16 dense rows.  Every case is inside the contract."""
    pitch = F.largest_pitch_n(129)
    assert pitch == 8388588 and F.window_ok(132, pitch, 129) and not F.window_ok(132, pitch + 4, 129)
    k_len = F.plan(16, EDGE_OUT, 129, splits=splits)[3]
    assert k_len == (256, 128)[splits - 1]
    for kr in ((129,), (128, 1))[splits - 1]:
        nk = -(-kr // 128)
        last = F.furthest_slice(nk)
        ext_w = (64 * nk - 1) * pitch + 128
        assert (64 * nk - 1) * pitch + 127 < ext_w <= 64 * nk * pitch
        assert last == 3 and last * 64 * pitch == 1610608896 < 1 << 31
        assert last * 64 * pitch + 63 * pitch + 127 == 2139090067 < 1 << 31   # (so below 2^32 too)
    assert 127 * pitch + EDGE_OUT + 16 + 4 + 64 <= EDGE_BYTES
    p = F.image_problem(16, EDGE_OUT, 129)
    w = EdgeImage(edge, p, pitch, 4)
    try:
        run_both(p, w, True, False, splits, cus, 4, 8, 2, 2)
    finally:
        w.close()


def test_the_largest_row_pitch_inside_the_window(edge, cus):
    """in 129, out 130, 16 rows of x at ldq = 8 388 588, the largest multiple of 4 with 256 ldq + in < 2^31 - 4096: x spans
    134 MB; the image is QWeight4's own.  The x descriptor's extent is 15 ldq + 132 = 125 828 952; a lane's offset is
    li ldq + k_begin + 16 g + 128 kt (+ 64) <= 15 ldq + 128 + 48 + 448 = 125 829 444 with the slices issued up to 3: far
    below 2^31, and beyond the extent only in the last row's bytes past `in` (zeros).  The weight's offsets are those of a
    pitch of 144."""
    ldq = D.largest_ldq(129)
    assert ldq == 8388588 and F.window_ok(ldq, 144, 129) and not F.window_ok(ldq + 4, 144, 129)
    assert 15 * ldq + 128 + 48 + 3 * 128 + 64 < 1 << 31
    p = F.problem(16, EDGE_OUT, 129)
    w = Weight(p, "qweight")
    assert w.pitch == 144
    try:
        keep, view, _ = edge_operand(edge, p.xq, ldq, 8, F.MAX_ROWS)
        for splits in (1, 2):
            run_both(p, w, True, True, splits, cus, y=3, yq=3, x_rows=(keep, view.data_ptr(), ldq))
    finally:
        w.close()


# ---- 3. caller-made images ----------------------------------------------------------------------------------------------------
def test_a_caller_made_image_with_every_nibble_value_and_rows_that_hold_minus_128(cus):
    """Every value -8 .. 7 in both nibble positions, the last row of x all -128, 0x55 in x's bytes beyond `in` and in the image's
    pad columns; each half of each slice moves the sums (F.every_half_slice_moves_the_sums, asserted when the problem is made)."""
    p = F.image_problem(16, 271, 385)
    P = F.pack_ref(p.W)
    assert set(np.unique(P & 15)) == set(range(16)) == set(np.unique(P[:192] >> 4)) and (p.xq[-1] == -128).all()
    w = Weight(p, "image", 5)
    try:
        for relu in (False, True):
            run_both(p, w, True, relu, 2, cus, 8, 12, 3, 3)
    finally:
        w.close()


def test_sums_beyond_2_to_the_24_add_up_exactly_across_ranges(cus):
    p = F.large_sums_problem()
    w = Weight(p, "image", 0)
    try:
        for splits in (1, 4):
            run_both(p, w, True, False, splits, cus, 0, 0, 1, 1)
    finally:
        w.close()


# ---- 4. equality with the int8 path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.EQUAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_packed_image_gives_the_int8_layers_bits(shape, cus):
    """qlinear_decode on QWeight4.from_image(pack(W)) against mmh_q8d_linear on the int8 image holding the same W: both outputs."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = shape
    p = F.image_problem(rows, out, in_)
    pitch = (out + 15) & ~15
    img = np.zeros((in_, pitch), np.int8)
    img[:, :out] = p.W
    W8, rw, bias = dev(img), dev(p.rw), dev(p.bias)
    qw4 = q8.QWeight4.from_image(dev(np.pad(F.pack_ref(p.W), ((0, 0), (0, pitch - out)))), rw, out, in_)
    keep, _, ldq = device_rows(p.xq, 4, 0)
    x = q8.QRows(keep[16:16 + rows * ldq].view(torch.int8).view(rows, ldq)[:, :in_], dev(p.rx))
    L8 = q8.lib_q8d()
    for so in (None, dev(p.so)):
        got = q8.qlinear_decode(x, qw4, bias, "relu", out_scale=so)
        assert q8.last_launch_q4d() == F.plan(rows, out, in_, so is not None, cus=cus)[0]
        text, need = q8.qlinear_decode_plan(rows, out, in_, ldq, pitch, so is not None, cu_count=cus)
        work = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
        y = torch.zeros((rows, pitch if so is not None else out), dtype=torch.int8 if so is not None else torch.float32, device="cuda")
        rc = L8.mmh_q8d_linear(0, rows, out, in_, x._ptr, x._ld, x.inv_scale.data_ptr(), W8.data_ptr(), pitch, rw.data_ptr(), bias.data_ptr(),
                               H.ACT_RELU, so.data_ptr() if so is not None else None, None if so is not None else y.data_ptr(),
                               0 if so is not None else out, y.data_ptr() if so is not None else None, pitch if so is not None else 0,
                               work.data_ptr(), work.numel(), 0, torch.cuda.current_stream().cuda_stream)
        assert rc == H.OK, L8.mmh_q8d_last_error()
        torch.cuda.synchronize()
        if so is None:
            assert torch.equal(got.view(torch.int32), y.view(torch.int32))
            assert same_bits(got.cpu().numpy(), F.want_of(p, True, True, False))
        else:
            assert torch.equal(got.q, y[:, :out])
            assert np.array_equal(got.q.cpu().numpy(), F.want_of(p, True, True, True))


# ---- 5. one deep case -------------------------------------------------------------------------------------------------------
def test_one_range_of_86_slices(cus):
    rows, out, in_, splits = F.DEEP
    assert -(-in_ // 128) == 86 and F.plan(rows, out, in_, splits=splits)[3] == in_
    p = F.problem(rows, out, in_)
    w = Weight(p, "qweight")
    try:
        run_both(p, w, True, False, splits, cus, 4, 4, 2, 2)
    finally:
        w.close()


# ---- 6. capture, the module, the refusals ---------------------------------------------------------------------------------------
def qrows(p, pad=0, rows=None):
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, in_ = rows or p.xq.shape[0], p.xq.shape[1]
    keep, _, ldq = device_rows(p.xq[:rows], pad, 0)
    return q8.QRows(keep[16:16 + rows * ldq].view(torch.int8).view(rows, ldq)[:, :in_], dev(p.rx[:rows]))


def test_a_captured_call_replays_on_rewritten_rows(cus):
    """Captured after reserve_decode(); replayed twice with x rewritten in between; bit-equal to the reference each time.  Both
    launches go to the one capturing stream, so the capture is a chain of two kernel nodes -- no parallel branches."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 273, 1153
    p1, p2 = F.problem(rows, out, in_), F.problem(rows - 1, out, in_)
    x2, rx2 = np.concatenate([p2.xq, p1.xq[:1]]), np.concatenate([p2.rx, p1.rx[:1]])
    qw = q8.QWeight4(dev(p1.w))
    qw.reserve_decode()
    reserved = qw._decode_work.data_ptr()
    assert qw._decode_work.numel() >= max(F.plan(r, out, in_, cus=cus)[1] for r in range(1, 17))
    bias = dev(p1.bias)
    xbuf = torch.zeros((rows, (in_ + 15) & ~15), dtype=torch.int8, device="cuda")
    rxbuf = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    x = q8.QRows(xbuf[:, :in_], rxbuf)
    y = torch.zeros((rows, out), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q8.qlinear_decode(x, qw, bias, "relu", out=y)
    assert qw._decode_work.data_ptr() == reserved
    P = F.pack_ref(p1.W)
    for xq, rx in ((p1.xq, p1.rx), (x2, rx2)):
        xbuf[:, :in_].copy_(dev(xq))
        rxbuf.copy_(dev(rx))
        y.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y.cpu().numpy(), F.want(xq, rx, P, in_, p1.rw, p1.bias, True))
    qw.close()


def test_a_workspace_that_would_grow_while_capturing_is_refused(monkeypatch):
    """(Told that the stream is capturing: a refusal inside a real capture would leave an empty graph behind.)"""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    p = F.problem(2, 129, 129)
    qw = q8.QWeight4(dev(p.w))
    x = qrows(p)
    y = torch.full((2, 129), 7.0, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode(x, qw, out=y)
    assert e.value.status == H.ERR_UNSUPPORTED and "QWeight4.reserve_decode" in str(e.value)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    qw.reserve_decode()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    q8.qlinear_decode(x, qw, out=y)   # reserved: nothing grows
    monkeypatch.undo()
    assert same_bits(y.cpu().numpy(), F.want_of(p, False, False, False))
    qw.close()


def test_the_module_with_four_bit_weights_and_the_refusals(cus):
    """QLinear.from_float(fc, decode=True, weight_bits=4) against the reference at 16 rows (fp32 rows: quantised by the row
    quantiser first); 17 rows are refused by the module, by qlinear_decode and by the library; qlinear has no 4-bit path."""
    import torch
    import how_to_optimize_gemm_amd as H
    import qlinear_ref as R
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(4)
    fc = torch.nn.Linear(192, 130).cuda()
    layer = q8.QLinear.from_float(fc, "relu", decode=True, weight_bits=4)
    assert isinstance(layer.qweight, q8.QWeight4) and layer.weight_bits == 4
    x = torch.randn(16, 192, device="cuda")
    got = layer(x)
    assert q8.last_launch_q4d() == F.plan(16, 130, 192, cus=cus)[0]
    xq = q8.quantize(x)
    q, _, rw = F.quantize4_ref(fc.weight.detach().cpu().numpy())
    want = F.want(xq.q.cpu().numpy(), xq.inv_scale.cpu().numpy(), F.pack_ref(np.ascontiguousarray(q.T)), 192, rw,
                  fc.bias.detach().cpu().numpy(), True)
    assert same_bits(got.cpu().numpy(), want)
    assert same_bits(layer(x.reshape(2, 8, 192)).cpu().numpy().reshape(16, 130), want)
    y = torch.full((17, 130), 7.0, device="cuda")
    for call in (lambda: layer(torch.zeros((17, 192), device="cuda")),
                 lambda: q8.qlinear_decode(torch.zeros((17, 192), device="cuda"), layer.qweight, out=y),
                 lambda: q8.qlinear_decode(q8.quantize(torch.ones((17, 192), device="cuda")), layer.qweight, out=y),
                 lambda: q8.qlinear(x, layer.qweight), lambda: q8.qlinear(xq, layer.qweight),
                 lambda: q8.qlinear(xq, layer.qweight, out_scale=1.0)):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_UNSUPPORTED and ("4-bit" in str(e.value)), str(e.value)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    with pytest.raises(H.MMultError):
        q8.QLinear.from_float(fc, weight_bits=4)   # no tile path: decode=True is part of asking for 4 bits
    # the timer goes through the same entry
    ms = q8.time_qlinear_decode(xq, layer.qweight, layer.bias, "relu", warmup=1, reps=3)
    assert isinstance(ms, float) and ms > 0 and q8.last_launch_q4d() == F.plan(16, 130, 192, cus=cus)[0]


# ---- 7. the Python layer: QWeight4's own plan behind the shared workspace, the timer, from_image's refusals -----------------------
@pytest.mark.parametrize("out8", [False, True], ids=["fp32", "int8"])
def test_time_qlinear_decode_launches_the_plan_and_leaves_the_result(out8, cus):
    """mmh_time_q4d_linear behind its argument checks: one warm-up and three timed calls; no bound on the time itself."""
    import math
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 257, 385
    p = F.problem(rows, out, in_)
    qw = q8.QWeight4(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    ldo = (out + 15) & ~15 if out8 else out
    y = torch.full((rows, ldo), POISON, dtype=torch.int8, device="cuda") if out8 else torch.full((rows, ldo), float("nan"), device="cuda")
    ms = q8.time_qlinear_decode(x, qw, bias, "relu", out=y[:, :out], out_scale=dev(p.so) if out8 else None, warmup=1, reps=3)
    assert isinstance(ms, float) and math.isfinite(ms) and ms > 0, ms
    assert q8.last_launch_q4d() == F.plan(rows, out, in_, out8, ldo, cus=cus)[0]
    got, want = y.cpu().numpy(), F.want_of(p, True, True, out8)
    if out8:
        assert np.array_equal(got[:, :out], want) and bool((got[:, out:] == POISON).all())
    else:
        assert same_bits(got, want)
    qw.close()


@pytest.mark.parametrize("refusal", ["in-the-warm-up", "between-the-events", "an-empty-range", "a-long-range"])
def test_the_timing_loop_unwinds_from_a_refused_call(refusal, cus):
    """mmh_time_q4d_linear on calls it has to refuse.  A workspace one byte short of the plan's, where the plan's own count is
    above one range (so that the device-free checks, which know no CU count, let it pass): linear_on refuses it in the warm-up
    (before the timer's events exist) or in the first timed call (after they do).  A forced count that leaves a range empty,
    and one range of 65536 + 128 k (a zero image: it is never read), are refused before the loop.  Every time the status and
    the message are the call's, nothing is launched -- the output and the workspace keep their fill, the launch text is the
    earlier call's -- and a correct timed call on the same rows and output follows.  (Argument refusals: nothing invalid
    reaches the device.)"""
    import ctypes as C
    import math
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 3, 130, 1153
    p = F.problem(rows, out, in_)
    qw = q8.QWeight4(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    text, work_bytes, own, _ = F.plan(rows, out, in_, cus=cus)
    assert own > 1 and work_bytes - 1 >= D.work_bytes(1, rows, out)
    assert F.plan(rows, out, in_, splits=6) is None and F.plan(rows, out, F.MAX_RANGE_K + 128, splits=1) == "long"
    q8.qlinear_decode(qrows(p, 4, 2), qw)   # (two rows: a launch text that is not this call's)
    before = q8.last_launch_q4d()
    assert before and before != text
    y = torch.full((rows, out), 7.0, device="cuda")
    work = torch.full((work_bytes,), WORK_FILL, dtype=torch.uint8, device="cuda")
    pq, _, pr = qw._ptrs
    k, ldq, pxq, pitch, splits, given, warmup, reps = in_, x._ld, x._ptr, qw.pitch, 0, work_bytes - 1, 1, 1
    message = b"the workspace is smaller than the plan's work_bytes"
    if refusal == "between-the-events":
        warmup, reps = 0, 2
    elif refusal == "an-empty-range":
        splits, given, message = 6, work_bytes, b"the forced split count leaves a K range empty"
    elif refusal == "a-long-range":
        k = ldq = F.MAX_RANGE_K + 128
        long_x = torch.zeros((rows, k), dtype=torch.int8, device="cuda")
        long_p = torch.zeros((F.layout(out, k)[1], pitch), dtype=torch.uint8, device="cuda")
        pxq, pq, splits, given = long_x.data_ptr(), long_p.data_ptr(), 1, work_bytes
        message = b"the forced split count leaves a K range longer than 65536 k (MMH_Q4D_MAX_RANGE_K)"
    L, ms = q8.lib_q4d(), C.c_float(-1.0)
    rc = L.mmh_time_q4d_linear(0, rows, out, k, pxq, ldq, x.inv_scale.data_ptr(), pq, pitch, pr, bias.data_ptr(), H.ACT_NONE, None,
                               y.data_ptr(), out, None, 0, work.data_ptr(), given, splits, warmup, reps,
                               torch.cuda.current_stream().cuda_stream, C.byref(ms))
    assert rc == H.ERR_INVALID_ARG, (rc, L.mmh_q4d_last_error())
    assert L.mmh_q4d_last_error() == b"mmh_time_q4d_linear: " + message
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((work == WORK_FILL).all()) and ms.value == -1.0
    assert q8.last_launch_q4d() == before
    took = q8.time_qlinear_decode(x, qw, bias, out=y, warmup=1, reps=3)
    assert isinstance(took, float) and math.isfinite(took) and took > 0, took
    assert q8.last_launch_q4d() == text
    assert same_bits(y.cpu().numpy(), F.want_of(p, True, False, False))
    qw.close()


def test_the_workspace_grows_between_two_calls_that_nothing_separates(cus):
    """1 row, then 16 rows with no synchronise in between: the second call replaces the cached workspace while the first may
    still be running on it (the old tensor goes back to torch's allocator, which hands it to nobody ahead of the stream's
    work).  Then 1 row again: what is large enough stays.  (in 385 has no 3 ranges without an empty one: 4, one per slice.)"""
    import torch
    from how_to_optimize_gemm_amd import q8
    out, in_, splits = D.FINISH_COLS + 1, 385, 4
    assert D.valid_splits(in_, splits) and not D.valid_splits(in_, 3)
    assert D.work_bytes(splits, 1, out) < D.work_bytes(splits, 16, out)
    p = F.problem(16, out, in_)
    qw = q8.QWeight4(dev(p.w))
    bias = dev(p.bias)
    x1, x16 = qrows(p, 4, 1), qrows(p, 4)
    torch.cuda.synchronize()
    assert qw._decode_work is None
    y1 = q8.qlinear_decode(x1, qw, bias, splits=splits)
    first = qw._decode_work
    assert first.numel() >= D.work_bytes(splits, 1, out) and first.numel() < D.work_bytes(splits, 16, out)
    y16 = q8.qlinear_decode(x16, qw, bias, splits=splits)
    second = qw._decode_work
    assert second is not first and second.numel() >= D.work_bytes(splits, 16, out)
    assert q8.last_launch_q4d() == F.plan(16, out, in_, splits=splits, cus=cus)[0]
    torch.cuda.synchronize()
    want = F.want_of(p, True, False, False)
    assert same_bits(y1.cpu().numpy(), want[:1]) and same_bits(y16.cpu().numpy(), want)
    again = q8.qlinear_decode(x1, qw, bias, splits=splits)
    assert qw._decode_work is second
    assert same_bits(again.cpu().numpy(), want[:1])
    qw.close()


@pytest.mark.parametrize("splits", [0, 3], ids=["own-choice", "forced-3"])
def test_reserve_decode_is_enough_for_every_row_count_on_both_outputs(splits, cus):
    """After reserve_decode() no call of 1 - 16 rows replaces the workspace, on a shape whose own split count -- and with it
    the plan's work_bytes -- varies with the rows, and is not the int8 plan's (tests/test_q4d_coverage.py): QWeight4 shares
    the workspace code with QWeight and has to bring its own plan to it."""
    from how_to_optimize_gemm_amd import q8
    out, in_ = F.RESERVE_SHAPE
    mine = [F.plan(rows, out, in_, splits=splits, cus=cus)[1] for rows in range(1, F.MAX_ROWS + 1)]
    assert len(set(mine)) >= 4
    if splits == 0:
        assert mine != [D.plan(rows, out, in_, cus=cus)[1] for rows in range(1, F.MAX_ROWS + 1)]
    p = F.problem(F.MAX_ROWS, out, in_)
    P = F.pack_ref(p.W)
    qw = q8.QWeight4(dev(p.w))
    bias = dev(p.bias)
    assert qw._decode_work is None
    qw.reserve_decode(splits=splits)
    reserved = qw._decode_work
    assert reserved.numel() >= max(mine)
    for rows in range(1, F.MAX_ROWS + 1):
        x = qrows(p, 8, rows)
        y = q8.qlinear_decode(x, qw, bias, splits=splits)
        assert q8.last_launch_q4d() == F.plan(rows, out, in_, splits=splits, cus=cus)[0]
        yq = q8.qlinear_decode(x, qw, bias, out_scale=dev(p.so[:rows]), splits=splits)
        assert q8.last_launch_q4d() == F.plan(rows, out, in_, True, (out + 15) & ~15, splits=splits, cus=cus)[0]
        assert qw._decode_work is reserved and qw._decode_work.data_ptr() == reserved.data_ptr(), rows
        assert same_bits(y.cpu().numpy(), F.want(p.xq[:rows], p.rx[:rows], P, in_, p.rw, p.bias))
        assert np.array_equal(yq.q.cpu().numpy(), F.want(p.xq[:rows], p.rx[:rows], P, in_, p.rw, p.bias, False, p.so[:rows]))
    qw.close()


def test_from_image_refuses_what_the_kernel_cannot_read():
    """QWeight4.from_image on a wrong packed row count, a row pitch that is no multiple of 4, a base 2 bytes off, and factors
    on the host, of another dtype or strided: ERR_INVALID_ARG each, nothing launched; the same memory laid out right is taken."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    out, in_ = 130, 129
    prow = F.layout(out, in_)[1]
    flat = torch.zeros((16 + (prow + 1) * 136,), dtype=torch.uint8, device="cuda")
    rw = torch.ones((2 * out,), dtype=torch.float32, device="cuda")

    def image(rows=prow, pitch=136, base=16):
        return torch.as_strided(flat, (rows, out), (pitch, 1), base)

    assert prow == 128 and flat.data_ptr() % 16 == 0
    good = q8.QWeight4.from_image(image(), rw[:out], out, in_)
    assert (good.pitch, good.scale, good._ptrs[0]) == (136, None, flat.data_ptr() + 16)
    for what, p, r in (("a packed row too many", image(rows=prow + 1), rw[:out]),
                       ("a packed row short", image(rows=prow - 1), rw[:out]),
                       ("a pitch of 134", image(pitch=134), rw[:out]),
                       ("a base off by 2", image(base=18), rw[:out]),
                       ("factors on the host", image(), rw[:out].cpu()),
                       ("float64 factors", image(), rw[:out].double()),
                       ("strided factors", image(), rw[::2]),
                       ("too few factors", image(), rw[:out - 1])):
        with pytest.raises(H.MMultError) as e:
            q8.QWeight4.from_image(p, r, out, in_)
        assert e.value.status == H.ERR_INVALID_ARG, (what, str(e.value))
