"""The 4-bit-weight small-batch layer (libmmult_hip_q4d.so: q4_row_amax_kernel, q4_pack_weight_kernel, q4decode_partial_kernel and
qdecode_finish_kernel<false / true>) bit for bit against tests/q4_ref.py, on both output forms of every case.

run() calls mmh_q4d_linear itself, on operands laid out as a caller may, as tests/test_gpu_qdecode.py does for the int8 layer:
x's int8 rows at a pitch of `in` rounded up to 4 plus 0 - 12 bytes and a base 0 - 12 bytes past a 16-byte boundary, every byte
beyond `in`, between the rows and in the (16 - rows) rows' worth of memory behind the last row poisoned with 0x55; a weight that
is QWeight4's own image or a caller-made one (its own pitch and base, pad columns poisoned); the output inside a buffer of 0x55
that is compared WHOLE with what the reference says it holds afterwards; the workspace pre-filled with 0x7f and followed by 64
guard bytes.  The launch text is held to the Python plan at the device's CU count.  tests/q4_ref.py has the case table,
tests/test_q4d_coverage.py what it promises."""
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


def run(p, weight, bias, relu, out8, splits, cus, x_pad=0, x_off=0, o_pad=0, o_off=0):
    """One mmh_q4d_linear call on the layouts above; asserts the status, the launch text, the whole output buffer, the
    workspace's guard.  Returns the launch text."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    L = q8.lib_q4d()
    rows, in_ = p.xq.shape
    out = p.W.shape[1]
    item = 1 if out8 else 4
    ldo = out + o_pad
    keep_x, pxq, ldq = device_rows(p.xq, x_pad, x_off)
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


def run_both(p, weight, bias, relu, splits, cus, x_pad=0, x_off=0, y=0, yq=0):
    a = run(p, weight, bias, relu, False, splits, cus, x_pad, x_off, *D.Y_LAYOUTS[y])
    b = run(p, weight, bias, relu, True, splits, cus, x_pad, x_off, *D.YQ_LAYOUTS[yq])
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
