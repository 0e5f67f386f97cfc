"""The small-batch int8 layer (libmmult_hip_q8d.so: qdecode_partial_kernel, qdecode_finish_kernel<false / true>) bit for bit
against tests/qchain_ref.py's qlinear_s8_ref, on both output forms of every case.

run() calls mmh_q8d_linear itself, on operands laid out as a caller may: x's int8 rows at a pitch of `in` rounded up to 4 plus
0 - 12 bytes and a base 0 - 12 bytes past a 16-byte boundary, every byte beyond `in`, between the rows and in the (16 - rows)
rows' worth of memory behind the last row poisoned with 0x55; a weight that is a real QWeight or a caller-made image (its own
pitch and base, pad columns poisoned); the output -- fp32 y and int8 yq in turn -- inside a buffer of 0x55 that is compared WHOLE
with what the reference says it holds afterwards (so the guards in front of, behind and between the rows are part of every
comparison); the workspace pre-filled with 0x7f and followed by 64 guard bytes.  The launch text is held to the Python plan
(tests/qdecode_ref.py) at the device's CU count.  tests/qdecode_ref.py has the two case tables -- cases(), thorough in the small,
and wide_deep_cases(), the sizes the kernels are built for --, tests/test_q8d_coverage.py what they promise.  Three more calls
run operands at the edge of the descriptor window (the largest pitch_n and ldq shape_status admits), built on the device inside
one 0.72 GB buffer of 0x55; the Python layer's timer and its cached workspace follow at the end."""
import ctypes as C

import numpy as np
import pytest

import qchain_ref as Q
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
    """(keep-alive tensor, pointer or None, ldq) of x's rows in poisoned memory; 16 rows' worth of bytes lie behind the base."""
    import torch
    rows, in_ = xq.shape
    if in_ == 0:
        return None, None, pad
    ldq = ((in_ + 3) & ~3) + pad
    host = np.full(16 + off + D.MAX_ROWS * ldq + 64, POISON, np.uint8)
    host[16 + off:16 + off + rows * ldq].reshape(rows, ldq)[:, :in_] = xq.view(np.uint8)
    flat = torch.from_numpy(host).cuda()
    return flat, flat.data_ptr() + 16 + off, ldq


def device_image(qw, pad, off):
    """(keep-alive tensor, pointer or None, pitch_n) of a caller-made image[k][j] = qw[j][k] in poisoned memory."""
    import torch
    out, in_ = qw.shape
    pitch = ((out + 3) & ~3) + pad
    if in_ == 0:
        return None, None, pitch
    host = np.full(16 + off + in_ * pitch + 64, POISON, np.uint8)
    host[16 + off:16 + off + in_ * pitch].reshape(in_, pitch)[:, :out] = np.ascontiguousarray(qw.T).view(np.uint8)
    flat = torch.from_numpy(host).cuda()
    return flat, flat.data_ptr() + 16 + off, pitch


class Weight:
    """The weight operands of a Problem on the device: a real QWeight's, or a caller-made image's."""

    def __init__(self, p, kind, i=0):
        from how_to_optimize_gemm_amd import q8
        self.qweight = None
        if kind == "qweight":
            assert p.w is not None
            self.qweight = q8.QWeight(dev(p.w))
            self.ptr, _, self.rw = self.qweight._ptrs
            self.pitch = self.qweight.pitch
            if p.w.shape[1] == 0:
                self.ptr = None
        else:
            self.keep, self.ptr, self.pitch = device_image(p.qw, (0, 4, 8, 12)[i % 4], (0, 4, 8, 12)[(i // 4 + 1) % 4])
            self.rw_t = dev(p.rw)
            self.rw = self.rw_t.data_ptr()

    def close(self):
        if self.qweight is not None:
            self.qweight.close()


def run(p, weight, bias, relu, out8, splits, cus, x_pad=0, x_off=0, o_pad=0, o_off=0, x_rows=None):
    """One mmh_q8d_linear call on the layouts above; asserts the status, the launch text, the whole output buffer, the
    workspace's guard.  Returns the launch text.  x_rows: device_rows' triple where the caller has laid x out itself."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    L = q8.lib_q8d()
    rows, in_ = p.xq.shape
    out = p.qw.shape[0]
    item = 1 if out8 else 4
    ldo = out + o_pad
    keep_x, pxq, ldq = x_rows or device_rows(p.xq, x_pad, x_off)
    rx, so, db = dev(p.rx), dev(p.so), dev(p.bias)
    planned = D.plan(rows, out, in_, out8, ldo, (item * o_off) % 16, splits, cus)
    assert planned is not None, "the table forces a split count the plan refuses"
    text, work_bytes, _, _ = planned
    work = torch.full((work_bytes + 64,), WORK_FILL, dtype=torch.uint8, device="cuda")
    front = 64 + item * o_off
    expect = np.full(front + rows * ldo * item + 64, POISON, np.uint8)
    buf = torch.from_numpy(expect.copy()).cuda()
    po = buf.data_ptr() + front
    rc = L.mmh_q8d_linear(0, rows, out, in_, pxq, ldq, rx.data_ptr(), weight.ptr, weight.pitch, weight.rw, db.data_ptr() if bias else None,
                          H.ACT_RELU if relu else H.ACT_NONE, so.data_ptr() if out8 else None, None if out8 else po, 0 if out8 else ldo,
                          po if out8 else None, ldo if out8 else 0, work.data_ptr() if in_ else None, work_bytes, splits,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == H.OK, (rc, L.mmh_q8d_last_error())
    launched = q8.last_launch_q8d()
    torch.cuda.synchronize()
    assert launched == text, (launched, text)
    want = D.want(p, bias, relu, out8)
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


@pytest.mark.parametrize("index", range(len(D.cases())), ids=[D.case_id(c) for c in D.cases()])
def test_every_case_of_the_table_is_the_contract_on_both_outputs(index, cus):
    c = D.cases()[index]
    p = (D.problem if c.weight == "qweight" else D.image_problem)(c.rows, c.out, c.in_)
    w = Weight(p, c.weight, index)
    try:
        run_both(p, w, c.bias, c.relu, c.splits, cus, c.x_pad, c.x_off, c.y, c.yq)
    finally:
        w.close()


@pytest.mark.parametrize("index", range(len(D.wide_deep_cases())), ids=[D.case_id(c) for c in D.wide_deep_cases()])
def test_every_case_of_the_second_table_is_the_contract_on_both_outputs(index, cus):
    """More than one finish workgroup per row (blockIdx.x of the finish kernel's column is no longer 0), up to 33 strips, up
    to one K range per slice -- the plan's own choice at one and two rows included, whatever it is on this device --, ranges
    of 33, 43 and 86 slices, every row count."""
    c = D.wide_deep_cases()[index]
    p = (D.problem if c.weight == "qweight" else D.image_problem)(c.rows, c.out, c.in_)
    w = Weight(p, c.weight, index)
    try:
        run_both(p, w, c.bias, c.relu, c.splits, cus, c.x_pad, c.x_off, c.y, c.yq)
    finally:
        w.close()


# ---- operands at the edge of the descriptor window --------------------------------------------------------------------------
EDGE_IN, EDGE_OUT = 129, 130
EDGE_BYTES = 16 + 12 + EDGE_IN * D.largest_pitch_n(EDGE_IN) + 64   # the largest of the three operands below: 0.72 GB


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
    """(keep-alive, pointer, ld) of int8 `values` as rows of pitch ld, 16 + off bytes into buf; everything else of the
    max(its rows, rows_behind) rows' worth of bytes and 64 behind them is 0x55 (again)."""
    import torch
    rows, cols = values.shape
    end = 16 + off + max((rows - 1) * ld + cols, rows_behind * ld) + 64
    assert off % 4 == 0 and ld % 4 == 0 and end <= buf.numel(), (values.shape, ld, off, buf.numel())
    buf[:end].fill_(POISON)
    torch.as_strided(buf.view(torch.int8), (rows, cols), (ld, 1), 16 + off).copy_(dev(values))
    return buf, buf.data_ptr() + 16 + off, ld


class EdgeImage:
    """Weight's interface for a caller-made image[k][j] = qw[j][k] of pitch `pitch` inside the edge buffer."""
    qweight = None

    def __init__(self, buf, p, pitch, off):
        _, self.ptr, self.pitch = edge_operand(buf, np.ascontiguousarray(p.qw.T), pitch, off)
        self.rw_t = dev(p.rw)
        self.rw = self.rw_t.data_ptr()


@pytest.mark.parametrize("splits", [1, 2])
def test_the_largest_image_pitch_inside_the_window(edge, cus, splits):
    """in 129, out 130, 16 rows, pitch_n = P = 5 577 868: the largest multiple of 4 that shape_status admits (the next one is
    refused: tests/test_q8d_abi.py).  The image spans 128 P + 130 bytes = 0.71 GB, of which 130 per k row are written.

    The offsets of qdecode_partial_kernel's weight descriptor, written down before the first run.  A lane's offset is
    voff + soff with voff = r P + 16 slot, r <= 127, and soff = kt 128 P; the descriptor's extent is ext_w = (kr - 1) P + 132
    (strip 0; 4 for strip 1, whose base is 128 bytes further).  With one range kr = 129, nk = 2, ext_w = 128 P + 132 =
    713 967 236, and the slices issued are 0 - 3:
      slice 0   offsets 0 .. 127 P + 127 = 708 389 363 < ext_w: image rows 0 - 127, all inside the image;
      slice 1   soff 128 P = 713 967 104; offsets 128 P .. 255 P + 127 = 1 422 356 467: row 128 (r = 0, 128 P + 0 .. 127) is
                below ext_w and inside the image, every r >= 1 is at or beyond 129 P > ext_w: zeros;
      slice 2   soff 256 P = 1 427 934 208; offsets .. 383 P + 127 = 2 136 323 571 < 2^31, all >= 256 P > ext_w: zeros;
      slice 3   soff 384 P = 2 141 901 312 < 2^31 (the int product does not overflow); offsets 384 P .. 511 P + 127 =
                2 850 290 675: above 2^31, below 2^32 -- an unsigned 32-bit sum that does not wrap --, all > ext_w: zeros.
    Slices 2 and 3 are issued behind the range's end and never consumed; nothing of them is fetched.  With two ranges range 0
    has kr = 128, nk = 1, ext_w = 127 P + 132, and its slice 1 (soff 128 P >= ext_w: zeros) IS consumed -- the second ring
    stage of an odd slice count; range 1's base is 128 P further, kr = 1, ext_w = 132, its slices 1 and 2 reach 383 P + 127
    past that base and are out of range from the first row on.  x is 16 dense rows: its offsets stay below 15 ldq + 512.
    The case is one the contract admits; every offset beyond ext_w must read zeros, and the asserts below are the arithmetic."""
    pitch = D.largest_pitch_n(EDGE_IN)
    assert D.window_ok(132, pitch, EDGE_IN) and not D.window_ok(132, pitch + 4, EDGE_IN)
    assert 3 * 128 * pitch < 1 << 31 and (1 << 31) < 511 * pitch + 127 < 1 << 32 and 128 * pitch + 132 < 256 * pitch
    p = D.image_problem(16, EDGE_OUT, EDGE_IN)
    w = EdgeImage(edge, p, pitch, 4)
    run_both(p, w, True, False, splits, cus, 4, 8, 2, 2)


def test_one_image_row_at_the_largest_pitch_inside_the_window(edge, cus):
    """in 1, out 130, 2 rows, pitch_n = P = 8 355 948: one image row, so the operand is 130 bytes, while the kernel's offsets
    are as large as at any depth: kr = 1, ext_w = 132 (strip 0), slice 0's rows r >= 1 start at voff = r P up to 127 P + 127 =
    1 061 205 523, the zero slices 1 and 2 add soff = 128 P = 1 069 561 344 and 256 P = 2 139 122 688 < 2^31; the largest sum is
    383 P + 127 = 3 200 328 211 < 2^32.  All of it beyond ext_w: zeros, nothing fetched."""
    pitch = D.largest_pitch_n(1)
    assert D.window_ok(4, pitch, 1) and not D.window_ok(4, pitch + 4, 1)
    assert 2 * 128 * pitch < 1 << 31 and 383 * pitch + 127 < 1 << 32
    p = D.image_problem(2, EDGE_OUT, 1)
    w = EdgeImage(edge, p, pitch, 12)
    run_both(p, w, False, True, 0, cus, 0, 4, 1, 1)


def test_the_largest_row_pitch_inside_the_window(edge, cus):
    """in 129, out 130, 16 rows of x at ldq = 8 388 588, the largest multiple of 4 with 256 ldq + in < 2^31 - 4096: x spans
    134 MB.  The x descriptor's extent is 15 ldq + 132 = 125 828 952; a lane's offset is li ldq + k + 16 g + 128 kt (+ 64) <=
    15 ldq + 48 + 448: far below 2^31, and beyond the extent only in the last row's bytes past `in` (zeros)."""
    ldq = D.largest_ldq(EDGE_IN)
    assert D.window_ok(ldq, 144, EDGE_IN) and not D.window_ok(ldq + 4, 144, EDGE_IN)
    p = D.problem(16, EDGE_OUT, EDGE_IN)
    w = Weight(p, "qweight")
    try:
        for splits in (1, 2):
            run_both(p, w, True, True, splits, cus, y=3, yq=3, x_rows=edge_operand(edge, p.xq, ldq, 8, D.MAX_ROWS))
    finally:
        w.close()


def test_the_plans_own_choice_splits_on_the_devices_cu_count(cus):
    rows, out, in_ = D.PLAN_SHAPE
    _, _, splits, k_len = D.plan(rows, out, in_, cus=cus)
    assert splits > 1 and k_len < in_, (cus, splits, k_len)
    p = D.problem(rows, out, in_)
    w = Weight(p, "qweight")
    try:
        for launched in run_both(p, w, True, False, 0, cus, 4, 8, 0, 0):
            assert f"x {splits} splits of {k_len} k" in launched
    finally:
        w.close()


@pytest.mark.parametrize("bias,relu", D.EPILOGUES, ids=["plain", "bias", "relu", "bias-relu"])
def test_bias_and_relu_all_four(bias, relu, cus):
    p = D.problem(15, 2 * D.STRIP + 17, 385)
    assert (D.want(p, bias, False, False) < 0).mean() > 0.2   # ReLU has something to cut
    w = Weight(p, "qweight")
    try:
        run_both(p, w, bias, relu, 2, cus, 12, 4, 1, 1)
    finally:
        w.close()


def test_sums_beyond_2_to_the_24_add_up_exactly_across_ranges(cus):
    p = D.large_sums_problem()
    w = Weight(p, "qweight")
    try:
        for splits in (1, 4):
            run_both(p, w, True, False, splits, cus, 0, 0, 1, 1)
    finally:
        w.close()


def test_caller_made_rows_and_image_that_hold_minus_128(cus):
    p = D.image_problem(16, 2 * D.STRIP + 15, 385)
    assert (p.xq[-1] == -128).all() and (p.qw == -128).any()
    w = Weight(p, "image", 5)
    try:
        for relu in (False, True):
            run_both(p, w, True, relu, 2, cus, 8, 12, 3, 3)
    finally:
        w.close()


# ---- the Python interface: the same bits as the tile path ---------------------------------------------------------------
def qrows(p, pad=0, rows=None):
    """The QRows of a Problem's rows (rows: of its first so many) at a pitch of `in` rounded up to 4 plus pad."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, in_ = rows or p.xq.shape[0], p.xq.shape[1]
    keep, _, ldq = device_rows(p.xq[:rows], pad, 0)
    return q8.QRows(keep[16:16 + rows * ldq].view(torch.int8).view(rows, ldq)[:, :in_], dev(p.rx[:rows]))


@pytest.mark.parametrize("shape", [(16, 256, 512), (5, 130, 257), (1, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_qlinear_decode_is_qlinear_bit_for_bit(shape, cus):
    """qlinear_decode against qlinear on the same operands -- whole 128-column tiles and ragged ones, fp32 and int8 outputs, a
    float and a per-row output scale, a QRows and an fp32 x -- and against the reference; the launch text is the plan's."""
    import torch
    from how_to_optimize_gemm_amd import q8
    p = D.problem(*shape)
    rows, out, in_ = shape
    qw = q8.QWeight(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    for act in (None, "relu"):
        tile = q8.qlinear(x, qw, bias, act)
        got = q8.qlinear_decode(x, qw, bias, act)
        assert q8.last_launch_q8d() == D.plan(rows, out, in_, cus=cus)[0]
        assert torch.equal(got.view(torch.int32), tile.view(torch.int32))
        assert same_bits(got.cpu().numpy(), Q.qlinear_s8_ref(p.xq, p.rx, p.w, p.bias, act == "relu"))
        for scale in (float(p.so[0]), dev(p.so)):
            so = np.full(rows, np.float32(scale), np.float32) if isinstance(scale, float) else p.so
            tile8 = q8.qlinear(x, qw, bias, act, out_scale=scale)
            got8 = q8.qlinear_decode(x, qw, bias, act, out_scale=scale)
            assert q8.last_launch_q8d() == D.plan(rows, out, in_, True, (out + 15) & ~15, cus=cus)[0]
            assert torch.equal(got8.q, tile8.q) and torch.equal(got8.inv_scale, tile8.inv_scale)
            assert np.array_equal(got8.q.cpu().numpy(), Q.qlinear_s8_ref(p.xq, p.rx, p.w, p.bias, act == "relu", so))
    xf = torch.from_numpy((np.random.default_rng(5).standard_normal((rows, in_)) * 2).astype(np.float32)).cuda()
    assert torch.equal(q8.qlinear_decode(xf, qw, bias).view(torch.int32), q8.qlinear(xf, qw, bias).view(torch.int32))
    for s in (2, 3):
        if D.valid_splits(in_, s):
            assert torch.equal(q8.qlinear_decode(x, qw, bias, splits=s).view(torch.int32), q8.qlinear(x, qw, bias).view(torch.int32))
    qw.close()


def test_more_than_16_rows_are_refused(cus):
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    p = D.problem(16, 128, 128)
    qw = q8.QWeight(dev(p.w))
    y = torch.full((17, 128), 7.0, device="cuda")
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode(torch.zeros((17, 128), device="cuda"), qw, out=y)
    assert e.value.status == H.ERR_UNSUPPORTED
    with pytest.raises(H.MMultError):
        q8.qlinear_decode(q8.quantize(torch.ones((17, 128), device="cuda")), qw, out=y)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    qw.close()


def test_a_captured_call_replays_on_rewritten_rows(cus):
    """Captured after reserve_decode(); replayed twice with x rewritten in between; bit-equal to the reference each time.  Both
    launches go to the one capturing stream, so the capture is a chain of two kernel nodes -- no parallel branches."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 2 * D.STRIP + 17, 1153
    p1, p2 = D.problem(rows, out, in_), D.problem(rows - 1, out, in_)
    x2 = np.concatenate([p2.xq, p1.xq[:1]])
    rx2 = np.concatenate([p2.rx, p1.rx[:1]])
    qw = q8.QWeight(dev(p1.w))
    qw.reserve_decode()
    reserved = qw._decode_work.data_ptr()
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
    for xq, rx in ((p1.xq, p1.rx), (x2, rx2)):
        xbuf[:, :in_].copy_(dev(xq))
        rxbuf.copy_(dev(rx))
        y.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y.cpu().numpy(), Q.qlinear_s8_ref(xq, rx, p1.w, p1.bias, True))
    qw.close()


def test_a_workspace_that_would_grow_while_capturing_is_refused(monkeypatch):
    """(Told that the stream is capturing: a refusal inside a real capture would leave an empty graph behind.)"""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    p = D.problem(2, 129, 129)
    qw = q8.QWeight(dev(p.w))
    x = qrows(p)
    y = torch.full((2, 129), 7.0, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode(x, qw, out=y)
    assert e.value.status == H.ERR_UNSUPPORTED and "reserve_decode" in str(e.value)
    monkeypatch.undo()
    qw.reserve_decode()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    q8.qlinear_decode(x, qw, out=y)   # reserved: nothing grows
    monkeypatch.undo()
    assert same_bits(y.cpu().numpy(), Q.qlinear_s8_ref(p.xq, p.rx, p.w))
    qw.close()


@pytest.mark.parametrize("rows", [1, 16, 17])
def test_the_modules_with_decode_give_the_tile_paths_bits(rows, cus):
    """QLinear(decode=True) and QMLP(decode=True) against decode=False at 1 and 16 rows; at 17 rows both take the tile path."""
    import torch
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(rows)
    fc1, fc2 = torch.nn.Linear(192, 272).cuda(), torch.nn.Linear(272, 130).cuda()
    x = torch.randn(rows, 192, device="cuda")
    a, b = q8.QLinear.from_float(fc1, "relu"), q8.QLinear.from_float(fc1, "relu", decode=True)
    q8.qlinear_decode(torch.randn(2, 272, device="cuda"), q8.QWeight(fc2.weight.detach()))   # (a launch text no module call below leaves)
    before = q8.last_launch_q8d()
    ya = a(x)
    assert q8.last_launch_q8d() == before                      # decode=False never goes there
    yb = b(x)
    if rows <= 16:
        assert q8.last_launch_q8d() == D.plan(rows, 272, 192, cus=cus)[0]
    else:
        assert q8.last_launch_q8d() == before and "qlinear_s8_kernel" in q8.last_launch()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    ma, mb = q8.QMLP.from_float([fc1, fc2]), q8.QMLP.from_float([fc1, fc2], decode=True)
    mb.out_scales = ma.calibrate(torch.randn(32, 192, device="cuda"))
    ya = ma(x)
    assert q8.last_launch_q8d() == (D.plan(rows, 272, 192, cus=cus)[0] if rows <= 16 else before)
    yb = mb(x)
    assert q8.last_launch_q8d() == (D.plan(rows, 130, 272, cus=cus)[0] if rows <= 16 else before)
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))


# ---- the Python layer: the timer, the cached workspace ------------------------------------------------------------------
@pytest.mark.parametrize("out8", [False, True], ids=["fp32", "int8"])
def test_time_qlinear_decode_launches_the_plan_and_leaves_the_result(out8, cus):
    """mmh_time_q8d_linear behind its argument checks: one warm-up and three timed calls; no bound on the time itself."""
    import math
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 257, 385
    p = D.problem(rows, out, in_)
    qw = q8.QWeight(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    ldo = (out + 15) & ~15 if out8 else out
    y = torch.full((rows, ldo), POISON, dtype=torch.int8, device="cuda") if out8 else torch.full((rows, ldo), float("nan"), device="cuda")
    ms = q8.time_qlinear_decode(x, qw, bias, "relu", out=y[:, :out], out_scale=dev(p.so) if out8 else None, warmup=1, reps=3)
    assert isinstance(ms, float) and math.isfinite(ms) and ms > 0, ms
    assert q8.last_launch_q8d() == D.plan(rows, out, in_, out8, ldo, cus=cus)[0]
    got = y.cpu().numpy()
    want = Q.qlinear_s8_ref(p.xq, p.rx, p.w, p.bias, True, p.so if out8 else None)
    if out8:
        assert np.array_equal(got[:, :out], want) and bool((got[:, out:] == POISON).all())
    else:
        assert same_bits(got, want)
    qw.close()


@pytest.mark.parametrize("warmup,reps", [(1, 1), (0, 2)], ids=["in-the-warm-up", "between-the-events"])
def test_the_timing_loop_unwinds_from_a_refused_call(warmup, reps, cus):
    """mmh_time_q8d_linear on a valid call whose work_bytes is one byte short of the plan's: linear_on refuses it in the warm-up
    (before the timer's events exist) or in the first timed call (after they do).  Either way the status and the message are the
    call's, nothing is launched -- the output and the workspace keep their fill, the launch text is the earlier call's -- and a
    correct timed call on the same rows and output follows.  (An argument refusal: nothing invalid reaches the device.)"""
    import math
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 3, 130, 257
    p = D.problem(rows, out, in_)
    qw = q8.QWeight(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    text, work_bytes, _, _ = D.plan(rows, out, in_, cus=cus)
    assert work_bytes > 1
    q8.qlinear_decode(qrows(p, 4, 2), qw)   # (two rows: a launch text that is not this call's)
    before = q8.last_launch_q8d()
    assert before and before != text
    y = torch.full((rows, out), 7.0, device="cuda")
    work = torch.full((work_bytes,), WORK_FILL, dtype=torch.uint8, device="cuda")
    L, ms = q8.lib_q8d(), C.c_float(-1.0)
    pq, _, pr = qw._ptrs
    rc = L.mmh_time_q8d_linear(0, rows, out, in_, x._ptr, x._ld, x.inv_scale.data_ptr(), pq, qw.pitch, pr, bias.data_ptr(), H.ACT_NONE, None,
                               y.data_ptr(), out, None, 0, work.data_ptr(), work_bytes - 1, 0, warmup, reps,
                               torch.cuda.current_stream().cuda_stream, C.byref(ms))
    assert rc == H.ERR_INVALID_ARG, (rc, L.mmh_q8d_last_error())
    assert L.mmh_q8d_last_error() == b"mmh_time_q8d_linear: the workspace is smaller than the plan's work_bytes"
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((work == WORK_FILL).all()) and ms.value == -1.0
    assert q8.last_launch_q8d() == before
    took = q8.time_qlinear_decode(x, qw, bias, out=y, warmup=1, reps=3)
    assert isinstance(took, float) and math.isfinite(took) and took > 0, took
    assert q8.last_launch_q8d() == text
    assert same_bits(y.cpu().numpy(), Q.qlinear_s8_ref(p.xq, p.rx, p.w, p.bias))
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
    p = D.problem(16, out, in_)
    qw = q8.QWeight(dev(p.w))
    bias = dev(p.bias)
    x1, x16 = qrows(p, 4, 1), qrows(p, 4)
    torch.cuda.synchronize()
    y1 = q8.qlinear_decode(x1, qw, bias, splits=splits)
    first = qw._decode_work
    assert first.numel() >= D.work_bytes(splits, 1, out) and first.numel() < D.work_bytes(splits, 16, out)
    y16 = q8.qlinear_decode(x16, qw, bias, splits=splits)
    second = qw._decode_work
    assert second is not first and second.numel() >= D.work_bytes(splits, 16, out)
    assert q8.last_launch_q8d() == D.plan(16, out, in_, splits=splits, cus=cus)[0]
    torch.cuda.synchronize()
    want = Q.qlinear_s8_ref(p.xq, p.rx, p.w, p.bias)
    assert same_bits(y1.cpu().numpy(), want[:1]) and same_bits(y16.cpu().numpy(), want)
    again = q8.qlinear_decode(x1, qw, bias, splits=splits)
    assert qw._decode_work is second
    assert same_bits(again.cpu().numpy(), want[:1])
    qw.close()


@pytest.mark.parametrize("splits", [0, 3], ids=["own-choice", "forced-3"])
def test_reserve_decode_is_enough_for_every_row_count_on_both_outputs(splits, cus):
    """After reserve_decode() no call of 1 - 16 rows replaces the workspace, on a shape whose own split count -- and with it
    rows x splits, largest in the middle of the range, not at 16 rows -- varies with the rows (tests/test_q8d_coverage.py)."""
    from how_to_optimize_gemm_amd import q8
    out, in_ = D.RESERVE_SHAPE
    p = D.problem(D.MAX_ROWS, out, in_)
    qw = q8.QWeight(dev(p.w))
    bias = dev(p.bias)
    assert qw._decode_work is None
    qw.reserve_decode(splits=splits)
    reserved = qw._decode_work
    need = max(D.plan(rows, out, in_, splits=splits, cus=cus)[1] for rows in range(1, D.MAX_ROWS + 1))
    assert reserved.numel() >= need
    for rows in range(1, D.MAX_ROWS + 1):
        x = qrows(p, 8, rows)
        y = q8.qlinear_decode(x, qw, bias, splits=splits)
        assert q8.last_launch_q8d() == D.plan(rows, out, in_, splits=splits, cus=cus)[0]
        yq = q8.qlinear_decode(x, qw, bias, out_scale=dev(p.so[:rows]), splits=splits)
        assert q8.last_launch_q8d() == D.plan(rows, out, in_, True, (out + 15) & ~15, splits=splits, cus=cus)[0]
        assert qw._decode_work is reserved and qw._decode_work.data_ptr() == reserved.data_ptr(), rows
        assert same_bits(y.cpu().numpy(), Q.qlinear_s8_ref(p.xq[:rows], p.rx[:rows], p.w, p.bias))
        assert np.array_equal(yq.q.cpu().numpy(), Q.qlinear_s8_ref(p.xq[:rows], p.rx[:rows], p.w, p.bias, False, p.so[:rows]))
    qw.close()
