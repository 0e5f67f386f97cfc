"""The 4-bit small-batch layer with one scale per group of 128 input features (libmmult_hip_q4g.so: q4g_pack_weight_kernel,
q4gdecode_partial_kernel and q4gdecode_finish_kernel<false / true>) bit for bit against tests/q4g_ref.py, on both output forms
of every case.

run() calls mmh_q4g_linear itself, on operands laid out as a caller may, as tests/test_gpu_q4decode.py does for the per-channel
layer: x's int8 rows at a pitch of `in` rounded up to 4 plus 0 - 12 bytes and a base 0 - 12 bytes past a 16-byte boundary, every
byte beyond `in`, between the rows and in the (16 - rows) rows' worth of memory behind the last row poisoned with 0x55; a weight
that is QWeight4G's own image and scales or caller-made ones (the image at its own pitch and base with poisoned pad columns, the
scales at their own pitch with NaN in every pad column); the output inside a buffer of 0x55 that is compared WHOLE with what the
reference says it holds afterwards; the workspace pre-filled with 0x7f and followed by 64 guard bytes.  The launch text is held
to the Python plan at the device's CU count, and the reference is evaluated under THAT partition: the bits depend on it."""
import collections
import functools

import numpy as np
import pytest

import q4_ref as F
import q4g_ref as G
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


def device_scales(r, pad, off16=1):
    """(keep-alive tensor, the factors as a strided fp32 view, pitch_s) of a caller-made scale array: its own pitch (out rounded
    up to 4 plus `pad` floats, a multiple of 4), a base 16 * off16 bytes into the allocation, NaN in every pad column."""
    import torch
    groups, out = r.shape
    pitch = ((out + 3) & ~3) + pad
    host = np.full(4 * off16 + groups * pitch + 16, np.nan, np.float32)
    host[4 * off16:4 * off16 + groups * pitch].reshape(groups, pitch)[:, :out] = r
    flat = torch.from_numpy(host).cuda()
    return flat, torch.as_strided(flat, (groups, out), (pitch, 1), 4 * off16), pitch


# ---- inputs -------------------------------------------------------------------------------------------------------------------
# xq int8 (rows, in); rx; w: the fp32 weight or None; W: the int8 image (in, out) in -8 .. 7; r: the groups' factors (groups, out)
Problem = collections.namedtuple("Problem", "xq rx w W r bias so")


def _rows(rng, rows, in_):
    xq = D.int8_full_range(rng, (rows, in_))
    if in_:
        xq[:, -1] = np.where(xq[:, -1] == 0, 127, xq[:, -1])
    return xq, rng.uniform(0.01, 0.05, rows).astype(np.float32)


def _finish(xq, rx, w, W, r, rng):
    bias = rng.uniform(-4, 4, W.shape[1]).astype(np.float32)
    in_ = xq.shape[1]
    y = G.want(xq, rx, F.pack_ref(W), in_, r, bias, False, 1 if in_ else 0)
    return Problem(xq, rx, w, W, r, bias, D.out_scales(y))


@functools.lru_cache(maxsize=None)
def problem(rows, out, in_):
    """A real weight: w ~ U(-0.5, 0.5) times a per-group gain of 2^-3 .. 2^3 (so the groups' scales differ), quantised by
    quantize4g_ref; rows over the full int8 range."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 5)
    xq, rx = _rows(rng, rows, in_)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    gain = np.ldexp(1.0, rng.integers(-3, 4, (out, G.groups(in_)))).astype(np.float32)
    w *= np.repeat(gain, G.GROUP, axis=1)[:, :in_]
    q, _, r = G.quantize4g_ref(w)
    return _finish(xq, rx, w, np.ascontiguousarray(q.T), r, rng)


@functools.lru_cache(maxsize=None)
def image_problem(rows, out, in_):
    """Operands no quantiser makes: every nibble value -8 .. 7 in both nibble positions (zeros rare), the last row of x all
    -128, factors 2^e m with e in -12 .. 12 (G.spread_factors): any other summation order rounds differently."""
    rng = np.random.default_rng(rows * 5 + out * 11 + in_ + 45)
    xq, rx = _rows(rng, rows, in_)
    xq[-1] = -128
    W = rng.integers(-8, 8, (in_, out), dtype=np.int8)
    W = np.where((W == 0) & (rng.random(W.shape) < 0.9), np.int8(-8), W).astype(np.int8)
    return _finish(xq, rx, None, W, G.spread_factors(rng, G.groups(in_), out), rng)


class Weight:
    """The weight operands of a Problem on the device: QWeight4G's own image and scales of p.w, or a caller-made image of p.W and
    a caller-made scale array of p.r adopted by QWeight4G.from_image."""

    def __init__(self, p, kind, i=0, r=None):
        from how_to_optimize_gemm_amd import q8
        in_, out = p.W.shape
        if kind == "qweight":
            assert p.w is not None and r is None
            self.qweight = q8.QWeight4G(dev(p.w))
        else:
            self.keep, view, _ = device_image(F.pack_ref(p.W), (0, 4, 8, 12)[i % 4], (0, 4, 8, 12)[(i // 4 + 1) % 4])
            self.keep_s, sview, _ = device_scales(p.r if r is None else r, (0, 4, 8, 20)[(i + 1) % 4], 1 + i % 3)
            self.qweight = q8.QWeight4G.from_image(view, sview, out, in_)
        self.ptr, _, self.gs = self.qweight._ptrs
        self.pitch, self.pitch_s = self.qweight.pitch, self.qweight.pitch_s

    def close(self):
        self.qweight.close()


def run(p, weight, bias, relu, out8, splits, cus, x_pad=0, x_off=0, o_pad=0, o_off=0, r=None, keep_work=False):
    """One mmh_q4g_linear call on the layouts above; asserts the status, the launch text, the whole output buffer, the
    workspace's guard.  r: the factors the weight was made with where they are not p.r.  Returns the launch text (keep_work:
    and the workspace's floats as the partial kernel left them, with the plan's (splits, k_len))."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    L = q8.lib_q4g()
    rows, in_ = p.xq.shape
    out = p.W.shape[1]
    r = p.r if r is None else r
    item = 1 if out8 else 4
    ldo = out + o_pad
    keep_x, pxq, ldq = device_rows(p.xq, x_pad, x_off)
    rx, so, db = dev(p.rx), dev(p.so), dev(p.bias)
    planned = G.plan(rows, out, in_, out8, ldo, (item * o_off) % 16, splits, cus)
    assert planned is not None, "the table forces a split count the plan refuses"
    text, work_bytes, own_splits, k_len = planned
    work = torch.full((work_bytes + 64,), WORK_FILL, dtype=torch.uint8, device="cuda")
    front = 64 + item * o_off
    expect = np.full(front + rows * ldo * item + 64, POISON, np.uint8)
    buf = torch.from_numpy(expect.copy()).cuda()
    po = buf.data_ptr() + front
    rc = L.mmh_q4g_linear(0, rows, out, in_, pxq, ldq, rx.data_ptr(), weight.ptr, weight.pitch, weight.gs, weight.pitch_s,
                          db.data_ptr() if bias else None, H.ACT_RELU if relu else H.ACT_NONE, so.data_ptr() if out8 else None,
                          None if out8 else po, 0 if out8 else ldo, po if out8 else None, ldo if out8 else 0, work.data_ptr(), work_bytes,
                          splits, torch.cuda.current_stream().cuda_stream)
    assert rc == H.OK, (rc, L.mmh_q4g_last_error())
    launched = q8.last_launch_q4g()
    torch.cuda.synchronize()
    assert launched == text, (launched, text)
    want = G.want(p.xq, p.rx, F.pack_ref(p.W), in_, r, p.bias if bias else None, relu, own_splits, k_len, p.so if out8 else None)
    got = buf.cpu().numpy()
    window = got[front:front + rows * ldo * item].reshape(rows, ldo * item)[:, :out * item]
    got_values = np.ascontiguousarray(window).view(np.int8 if out8 else np.float32)
    if out8:
        assert np.array_equal(got_values, want), (launched, int((got_values != want).sum()), np.argwhere(got_values != want)[:4])
    else:
        assert same_bits(got_values, want), (launched, first_difference(got_values, want))
    # NaN payloads are the device's own: the guard bands are compared outside the window, the window through same_bits above
    expect[front:front + rows * ldo * item].reshape(rows, ldo * item)[:, :out * item] = window
    assert np.array_equal(got, expect), (launched, "wrote outside the rows x out window", np.argwhere(got != expect)[:4])
    assert bool((work[work_bytes:] == WORK_FILL).all()), (launched, "wrote behind the plan's work_bytes")
    if keep_work:
        wp = (out + 3) & ~3
        return launched, work[:own_splits * rows * wp * 4].cpu().numpy().view(np.float32).reshape(own_splits, rows, wp)[:, :, :out], own_splits, k_len
    return launched


def run_both(p, weight, bias, relu, splits, cus, x_pad=0, x_off=0, y=0, yq=0, r=None):
    a = run(p, weight, bias, relu, False, splits, cus, x_pad, x_off, *D.Y_LAYOUTS[y], r=r)
    b = run(p, weight, bias, relu, True, splits, cus, x_pad, x_off, *D.YQ_LAYOUTS[yq], r=r)
    return a, b


# ---- 1. the packer ----------------------------------------------------------------------------------------------------------
PACK_INS, PACK_OUTS = (1, 63, 64, 65, 127, 128, 129, 257, 384), (1, 5, 130)


def special_group_weight(out, in_, rng):
    """U(-2, 2) with, group by group, what the quantiser has a rule for: channel 0's FIRST group all zero (scale 1) and, from
    five channels on, F.special_weight's rows in the LAST group -- all zero, a NaN, +-inf, a maximum of 1e-39 whose scale
    overflows (clamped to FLT_MAX), all -max."""
    w = rng.uniform(-2, 2, (out, in_)).astype(np.float32)
    w[0, :G.GROUP] = 0
    k0 = G.GROUP * (G.groups(in_) - 1)
    if out >= 5 and in_ - k0 >= 4:
        w[:5, k0:] = F.special_weight(5, in_ - k0, rng)
    elif in_ - k0 >= 3:
        w[-1, k0], w[-1, k0 + 1], w[-1, k0 + 2] = np.nan, np.inf, -np.inf
    return w


def check_packed(qw, w):
    """QWeight4G(w)'s image, scales and reciprocals against quantize4g_ref(w): every byte of every row up to the pitches."""
    out, in_ = w.shape
    q, s, r = G.quantize4g_ref(w)
    pitch, prow, groups, pitch_s, image_bytes, scale_bytes = G.layout(out, in_)
    assert (qw.pitch, tuple(qw.p.shape), qw.pitch_s, tuple(qw.group_scale.shape), tuple(qw.group_inv_scale.shape)) == \
        (pitch, (prow, pitch), pitch_s, (groups, pitch_s), (groups, pitch_s))
    assert qw.nbytes == image_bytes + scale_bytes and qw.scale is None and qw.inv_scale is None
    want = np.zeros((prow, pitch), np.uint8)
    want[:, :out] = F.pack_ref(np.ascontiguousarray(q.T))
    assert np.array_equal(qw.p.cpu().numpy(), want), np.argwhere(qw.p.cpu().numpy() != want)[:4]
    for got, ref in ((qw.group_scale, s), (qw.group_inv_scale, r)):
        full = np.zeros((groups, pitch_s), np.float32)
        full[:, :out] = ref
        assert same_bits(got.cpu().numpy(), full), first_difference(got.cpu().numpy(), full)
    assert np.array_equal(qw.unpack().cpu().numpy()[:, :out], q.T) and not qw.unpack().cpu().numpy()[:, out:].any()
    assert same_bits(qw.dequantize().cpu().numpy(), G.dequantize_ref(q, r))


@pytest.mark.parametrize("out", PACK_OUTS)
def test_the_packer_is_the_reference_at_every_tail_and_special_value(out):
    from how_to_optimize_gemm_amd import q8
    for in_ in PACK_INS:
        w = special_group_weight(out, in_, np.random.default_rng(out * 1000 + in_))
        qw = q8.QWeight4G(dev(w))
        check_packed(qw, w)
        assert int(qw.unpack().min()) >= -7   # the library never produces -8
        assert qw.group_scale[0, 0].item() == 1.0   # the zero group


def test_the_packer_on_a_strided_weight_window_and_on_no_columns():
    import torch
    from how_to_optimize_gemm_amd import q8
    rng = np.random.default_rng(9)
    big = special_group_weight(130, 300, rng)
    qw = q8.QWeight4G(dev(big)[:, 3:260])             # row stride 300, a base that is not 16-byte aligned, in = 257
    check_packed(qw, big[:, 3:260])
    assert float(qw.group_scale.max()) == float(np.finfo(np.float32).max) or not (np.abs(big[:, 3:260]) == np.float32(1e-39)).any()
    empty = q8.QWeight4G(torch.zeros((5, 0), device="cuda"))     # in == 0: no group, no image
    assert tuple(empty.p.shape) == (0, 16) and tuple(empty.group_inv_scale.shape) == (0, 16) and empty.nbytes == 0
    y = q8.qlinear_decode(q8.QRows(torch.zeros((2, 0), dtype=torch.int8, device="cuda"), torch.ones(2, device="cuda")), empty,
                          torch.arange(5, dtype=torch.float32, device="cuda"))
    assert y.cpu().numpy().tolist() == [[0, 1, 2, 3, 4]] * 2
    assert q8.last_launch_q4g() == G.plan(2, 5, 0)[0] and "alone" in q8.last_launch_q4g()


# ---- 2. the kernel, the table ---------------------------------------------------------------------------------------------------
ROWS = (1, 2, 15, 16)
OUTS = (1, 4, 127, 129, 130, 257)
INS = (1, 64, 65, 128, 129, 256, 257, 640, 641)
FORCED = (1, 2, 3)
DEEP = (16, 130, 11008, 1)                         # 86 slices through the ring in one range: one long chain
OWN_CHOICE = ((16, 257, 2048), (1, 130, 8192))     # splits == 0: whatever the plan makes of the device's CU count


@functools.lru_cache(maxsize=None)
def cases():
    """qdecode_ref's Case rows (its layouts, weight kinds and epilogues rotate).  Every `in` at every forced split count that
    leaves no range empty -- 640: five slices in two ranges (3 + 2) and in three (2 + 2 + 1, an uneven last range); 257 in
    three: a last range of one k; one, two and three slices per range: both parities of the two-stage ring --, then every out at
    two row counts behind the deeper shapes, then the plan's own choice."""
    out, i = [], 0
    for in_ in INS:
        for s in FORCED:
            if D.valid_splits(in_, s):
                out.append(D._case(i, ROWS[i % 4], OUTS[(5 * i + 1) % len(OUTS)], in_, s))
                i += 1
    deep = [(129, 2), (641, 2), (640, 3), (257, 3), (640, 2), (641, 3)]
    for j, n in enumerate(OUTS):
        for k in (0, 2):
            in_, s = deep[i % len(deep)]
            out.append(D._case(i, ROWS[(j + k) % 4], n, in_, s))
            i += 1
    for rows, n, in_ in OWN_CHOICE:
        out.append(D._case(i, rows, n, in_, 0))
        i += 1
    return tuple(out)


def test_the_table_holds_what_it_promises():
    cs = cases()
    assert {c.rows for c in cs} == set(ROWS) and {c.out for c in cs} == set(OUTS) and set(INS) <= {c.in_ for c in cs}
    assert {(c.in_, c.splits) for c in cs} >= {(640, 2), (640, 3), (257, 3), (641, 2), (641, 3), (1, 1), (128, 1), (256, 2)}
    per_range = {-(-(e - b) // 128) for c in cs if c.splits for b, e in D.ranges(c.in_, c.splits)[1]}
    assert per_range >= {1, 2, 3}
    assert {c.weight for c in cs} == {"qweight", "image"} and {(c.bias, c.relu) for c in cs} == set(D.EPILOGUES)
    assert any(D.Y_LAYOUTS[c.y][0] % 4 for c in cs) and any(D.YQ_LAYOUTS[c.yq][1] % 4 for c in cs)   # single-store forms


@pytest.mark.parametrize("index", range(len(cases())), ids=[D.case_id(c) for c in cases()])
def test_every_case_of_the_table_is_the_contract_on_both_outputs(index, cus):
    c = cases()[index]
    p = (problem if c.weight == "qweight" else image_problem)(c.rows, c.out, c.in_)
    w = Weight(p, c.weight, index)
    try:
        run_both(p, w, c.bias, c.relu, c.splits, cus, c.x_pad, c.x_off, c.y, c.yq)
    finally:
        w.close()


def test_one_long_chain_of_86_groups(cus):
    rows, out, in_, splits = DEEP
    assert G.groups(in_) == 86 and G.plan(rows, out, in_, splits=splits)[3] == in_
    p = image_problem(rows, out, in_)
    w = Weight(p, "image", 3)
    try:
        run_both(p, w, True, False, splits, cus, 4, 4, 2, 2)
    finally:
        w.close()


@pytest.mark.parametrize("bias,relu", D.EPILOGUES, ids=["plain", "bias", "relu", "bias-relu"])
def test_bias_and_relu_all_four_with_per_row_output_scales(bias, relu, cus):
    p = problem(15, 257, 385)
    assert (G.want(p.xq, p.rx, F.pack_ref(p.W), 385, p.r, p.bias if bias else None, False, 2) < 0).mean() > 0.2   # ReLU has something to cut
    assert len(set(p.so.tolist())) > 1
    w = Weight(p, "qweight")
    try:
        run_both(p, w, bias, relu, 2, cus, 12, 4, 1, 1)
    finally:
        w.close()


# ---- 3. what the factors may hold ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_,splits,first", [(640, 2, 3), (257, 3, 1), (384, 3, 1)], ids=["3+2", "1+1+1k", "1+1+1"])
def test_inf_and_nan_behind_a_ranges_end_stay_out_of_its_partial(in_, splits, first, cus):
    """The trap of the two-stage ring: a range of an ODD number of slices computes one slice past its end, whose weights
    arrive as zeros -- and whose factors are the NEXT range's first group.  That group holds inf (even columns) and NaN (odd
    ones) here: 0 * inf would be NaN.  Range 0's partial, read back from the workspace, is finite and the reference's, bit for
    bit; the later partials and the final result are the reference's too (NaN or inf where the rule says so)."""
    rows, out = 16, 130
    p = image_problem(rows, out, in_)
    r = p.r.copy()
    r[first, 0::2], r[first, 1::2] = np.inf, np.nan
    k_len = G.plan(rows, out, in_, splits=splits)[3]
    ranges = G.range_groups(in_, splits, k_len)
    assert ranges[1][0] == first and (ranges[0][1] - ranges[0][0]) % 2 == 1
    w = Weight(p, "image", 2, r=r)
    try:
        launched, work, s, k = run(p, w, True, False, False, splits, cus, 4, 4, 0, 0, r=r, keep_work=True)
        assert (s, k) == (splits, k_len)
        ref = G.partials(p.xq, F.pack_ref(p.W), in_, r, splits, k_len)
        assert np.isfinite(work[0]).all() and same_bits(work[0], ref[0]), first_difference(work[0], ref[0])
        assert not np.isfinite(ref[1]).any()
        for i in range(splits):
            assert same_bits(work[i], ref[i]), (i, first_difference(work[i], ref[i]))
        run(p, w, True, True, True, splits, cus, 0, 8, 1, 1, r=r)
    finally:
        w.close()


def test_real_groups_with_zero_negative_subnormal_inf_and_nan_factors(cus):
    """A caller-made array follows the rule literally: t = f32(S) * r whatever r is (0 * inf = NaN)."""
    rows, out, in_ = 15, 129, 641
    p = image_problem(rows, out, in_)
    r = p.r.copy()
    r[0, 0], r[1, 1], r[2, 2], r[3, 3], r[4, 4], r[5, 5] = 0.0, -0.0, -3.5, 1e-40, np.inf, np.nan
    r[2, 6:9] = [-np.inf, -1e-42, np.float32(3e38)]
    r[:, 128] = -r[:, 128]
    W = p.W.copy()
    W[512:640, 4] = 0          # S_4 = 0 against inf in column 4: NaN
    p = p._replace(W=W)
    ref = G.want(p.xq, p.rx, F.pack_ref(W), in_, r, None, False, 2)
    assert np.isnan(ref[:, 4]).all() and np.isnan(ref[:, 5]).all() and np.isinf(ref[:, 6]).all() and np.isfinite(ref[:, :4]).all()
    w = Weight(p, "image", 1, r=r)
    try:
        for splits in (1, 2, 3):
            run_both(p, w, True, splits == 2, splits, cus, 8, 12, 3, 3, r=r)
    finally:
        w.close()


# ---- 4. agreement with the per-channel layer ------------------------------------------------------------------------------------
def test_power_of_two_factors_in_one_range_give_the_per_channel_layers_bits(cus):
    """What can be said exactly.  Let every group of channel j carry the same factor 2^e_j, force one range, and let every
    prefix of the channel's group sums stay below 2^24 in magnitude (always so for in < 16384: |S_g| <= 2^17).  Then every
    t_g = S_g 2^e and every running sum is 2^e times an integer below 2^24 -- exact --, so P = 2^e acc, and
    fl(P rx) = fl(2^e acc rx) = 2^e fl(acc rx) = fl(fl(acc rx) rw) with rw = 2^e (scaling by a power of two is exact away from
    overflow and subnormals): qlinear_decode on the QWeight4 holding that rw gives THE SAME BITS, on both outputs.
    It does not hold in general: beyond 2^24 the per-channel layer rounds (float)acc once where this chain rounds at every
    step, and with factors that are no powers of two the products round per group.  So the case here is constructed."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 130, 640
    assert G.groups(in_) * G.S_BOUND < 1 << 24
    p = image_problem(rows, out, in_)
    e = np.random.default_rng(2).integers(-8, 9, out)
    rw = np.ldexp(1.0, e).astype(np.float32)
    r = np.repeat(rw[None, :], G.groups(in_), axis=0)
    keep, view, _ = device_image(F.pack_ref(p.W), 4, 8)
    keep_s, sview, _ = device_scales(r, 4)
    qg = q8.QWeight4G.from_image(view, sview, out, in_)
    q4 = q8.QWeight4.from_image(view, dev(rw), out, in_)
    keep_x, _, ldq = device_rows(p.xq, 4, 0)
    x = q8.QRows(keep_x[16:16 + rows * ldq].view(torch.int8).view(rows, ldq)[:, :in_], dev(p.rx))
    bias = dev(p.bias)
    for so in (None, dev(p.so)):
        mine = q8.qlinear_decode(x, qg, bias, "relu", out_scale=so, splits=1)
        assert q8.last_launch_q4g() == G.plan(rows, out, in_, so is not None, splits=1, cus=cus)[0]
        theirs = q8.qlinear_decode(x, q4, bias, "relu", out_scale=so, splits=1)
        ref = G.want(p.xq, p.rx, F.pack_ref(p.W), in_, r, p.bias, True, 1, None, None if so is None else p.so)
        if so is None:
            assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32)) and same_bits(mine.cpu().numpy(), ref)
            assert same_bits(ref, F.want(p.xq, p.rx, F.pack_ref(p.W), in_, rw, p.bias, True))
        else:
            assert torch.equal(mine.q, theirs.q) and np.array_equal(mine.q.cpu().numpy(), ref)


# ---- 5. capture, the Python layer, the refusals -----------------------------------------------------------------------------------
def qrows(p, pad=0, rows=None):
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, in_ = rows or p.xq.shape[0], p.xq.shape[1]
    keep, _, ldq = device_rows(p.xq[:rows], pad, 0)
    return q8.QRows(keep[16:16 + rows * ldq].view(torch.int8).view(rows, ldq)[:, :in_], dev(p.rx[:rows]))


def want_of(p, rows, cus, bias=True, relu=False, out8=False, splits=0, ldo=0):
    """The reference of the first `rows` rows of a Problem under the plan's partition at this device's CU count."""
    in_, out = p.W.shape
    _, _, s, k_len = G.plan(rows, out, in_, out8, ldo, splits=splits, cus=cus)
    return G.want(p.xq[:rows], p.rx[:rows], F.pack_ref(p.W), in_, p.r, p.bias if bias else None, relu, s, k_len, p.so[:rows] if out8 else None)


def test_a_captured_call_replays_on_rewritten_rows(cus):
    """Captured after reserve_decode(); replayed twice with x rewritten in between; bit-equal to the reference each time.  Both
    launches go to the one capturing stream, so the capture is a chain of two kernel nodes -- no parallel branches."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 257, 1153
    p1, p2 = problem(rows, out, in_), image_problem(rows, out, in_)
    qw = q8.QWeight4G(dev(p1.w))
    qw.reserve_decode()
    reserved = qw._decode_work.data_ptr()
    assert qw._decode_work.numel() >= max(G.plan(r, out, in_, cus=cus)[1] for r in range(1, 17))
    bias = dev(p1.bias)
    xbuf = torch.zeros((rows, (in_ + 15) & ~15), dtype=torch.int8, device="cuda")
    rxbuf = torch.zeros((rows,), dtype=torch.float32, device="cuda")
    x = q8.QRows(xbuf[:, :in_], rxbuf)
    y = torch.zeros((rows, out), dtype=torch.float32, device="cuda")
    q8.qlinear_decode(x, qw, bias, "relu", out=y)   # (once outside: whatever the first call asks of the device is asked here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q8.qlinear_decode(x, qw, bias, "relu", out=y)
    assert qw._decode_work.data_ptr() == reserved
    for xq, rx in ((p1.xq, p1.rx), (p2.xq, p2.rx)):
        xbuf[:, :in_].copy_(dev(xq))
        rxbuf.copy_(dev(rx))
        y.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y.cpu().numpy(), want_of(p1._replace(xq=xq, rx=rx), rows, cus, True, True))
    qw.close()


def test_a_workspace_that_would_grow_while_capturing_is_refused(monkeypatch):
    """(Told that the stream is capturing: a refusal inside a real capture would leave an empty graph behind.)"""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    p = problem(2, 129, 129)
    qw = q8.QWeight4G(dev(p.w))
    x = qrows(p)
    y = torch.full((2, 129), 7.0, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode(x, qw, out=y)
    assert e.value.status == H.ERR_UNSUPPORTED and "QWeight4G.reserve_decode" in str(e.value)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    qw.close()


def test_the_workspace_grows_between_two_calls_that_nothing_separates(cus):
    """1 row, then 16 rows with no synchronise in between: the second call replaces the cached workspace while the first may
    still be running on it.  Then 1 row again: what is large enough stays."""
    import torch
    from how_to_optimize_gemm_amd import q8
    out, in_, splits = D.FINISH_COLS + 1, 385, 4
    p = problem(16, out, in_)
    qw = q8.QWeight4G(dev(p.w))
    bias = dev(p.bias)
    x1, x16 = qrows(p, 4, 1), qrows(p, 4)
    torch.cuda.synchronize()
    assert qw._decode_work is None
    y1 = q8.qlinear_decode(x1, qw, bias, splits=splits)
    first = qw._decode_work
    assert D.work_bytes(splits, 1, out) <= first.numel() < D.work_bytes(splits, 16, out)
    y16 = q8.qlinear_decode(x16, qw, bias, splits=splits)
    second = qw._decode_work
    assert second is not first and second.numel() >= D.work_bytes(splits, 16, out)
    assert q8.last_launch_q4g() == G.plan(16, out, in_, splits=splits, cus=cus)[0]
    torch.cuda.synchronize()
    want = want_of(p, 16, cus, splits=splits)
    assert same_bits(y1.cpu().numpy(), want[:1]) and same_bits(y16.cpu().numpy(), want)
    again = q8.qlinear_decode(x1, qw, bias, splits=splits)
    assert qw._decode_work is second and same_bits(again.cpu().numpy(), want[:1])
    qw.close()


@pytest.mark.parametrize("out8", [False, True], ids=["fp32", "int8"])
def test_time_qlinear_decode_launches_the_plan_and_leaves_the_result(out8, cus):
    """mmh_time_q4g_linear behind its argument checks: one warm-up and three timed calls; no bound on the time itself."""
    import math
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = 16, 257, 385
    p = problem(rows, out, in_)
    qw = q8.QWeight4G(dev(p.w))
    x, bias = qrows(p, 4), dev(p.bias)
    ldo = (out + 15) & ~15 if out8 else out
    y = torch.full((rows, ldo), POISON, dtype=torch.int8, device="cuda") if out8 else torch.full((rows, ldo), float("nan"), device="cuda")
    ms = q8.time_qlinear_decode(x, qw, bias, "relu", out=y[:, :out], out_scale=dev(p.so) if out8 else None, warmup=1, reps=3)
    assert isinstance(ms, float) and math.isfinite(ms) and ms > 0, ms
    assert q8.last_launch_q4g() == G.plan(rows, out, in_, out8, ldo, cus=cus)[0]
    got, want = y.cpu().numpy(), want_of(p, rows, cus, True, True, out8, ldo=ldo)
    if out8:
        assert np.array_equal(got[:, :out], want) and bool((got[:, out:] == POISON).all())
    else:
        assert same_bits(got, want)
    qw.close()


def test_the_module_and_a_two_layer_stack_against_a_host_chain(cus):
    """QLinear.from_float(fc, decode=True, weight_bits=4, group_size=128) at 16 rows (fp32 rows: quantised by the row quantiser
    first), then QMLP([QWeight4G, QWeight4G], decode=True): quantise, int8 -> int8 under a static scale, int8 -> fp32 -- each
    layer the reference under the plan's own partition for its shape and output form."""
    import torch
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(4)
    fc1, fc2 = torch.nn.Linear(320, 130).cuda(), torch.nn.Linear(130, 33).cuda()
    layer = q8.QLinear.from_float(fc1, "relu", decode=True, weight_bits=4, group_size=128)
    assert isinstance(layer.qweight, q8.QWeight4G) and (layer.weight_bits, layer.group_size) == (4, 128)
    x = torch.randn(16, 320, device="cuda")
    got = layer(x)
    assert q8.last_launch_q4g() == G.plan(16, 130, 320, cus=cus)[0]
    xq = q8.quantize(x)
    hx, hrx = xq.q.cpu().numpy(), xq.inv_scale.cpu().numpy()
    w1, b1 = fc1.weight.detach().cpu().numpy(), fc1.bias.detach().cpu().numpy()
    w2, b2 = fc2.weight.detach().cpu().numpy(), fc2.bias.detach().cpu().numpy()
    q1, _, r1 = G.quantize4g_ref(w1)
    q2, _, r2 = G.quantize4g_ref(w2)
    P1, P2 = F.pack_ref(np.ascontiguousarray(q1.T)), F.pack_ref(np.ascontiguousarray(q2.T))
    _, _, s, k_len = G.plan(16, 130, 320, cus=cus)
    want = G.want(hx, hrx, P1, 320, r1, b1, True, s, k_len)
    assert same_bits(got.cpu().numpy(), want)
    assert same_bits(layer(x.reshape(2, 8, 320)).cpu().numpy().reshape(16, 130), want)
    # the stack
    mlp = q8.QMLP([q8.QWeight4G(fc1.weight.detach()), q8.QWeight4G(fc2.weight.detach())], [fc1.bias.detach(), fc2.bias.detach()], decode=True)
    scales = mlp.calibrate(x)
    assert len(scales) == 1 and scales[0] == float(D.out_scales(want.reshape(1, -1))[0])
    y = mlp(x)
    so = np.full(16, scales[0], np.float32)
    _, _, s1, k1 = G.plan(16, 130, 320, True, cus=cus)
    h = G.want(hx, hrx, P1, 320, r1, b1, True, s1, k1, so)
    with np.errstate(all="ignore"):
        hr = np.float32(1.0) / so
    _, _, s2, k2 = G.plan(16, 33, 130, cus=cus)
    assert same_bits(y.cpu().numpy(), G.want(h, hr, P2, 130, r2, b2, False, s2, k2))
    assert q8.last_launch_q4g() == G.plan(16, 33, 130, cus=cus)[0]


def test_the_refusals_launch_nothing_and_touch_nothing(cus):
    """17 rows (the module, qlinear_decode on fp32 rows and on QRows, the library), qlinear on a QWeight4G, a group size other
    than 128, a scale array the kernel cannot read, from_image's shape errors: the stated status each time, the outputs keep
    their fill and the launch text stays the earlier call's."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    out, in_ = 130, 257
    p = image_problem(16, out, in_)
    fc = torch.nn.Linear(in_, out).cuda()
    layer = q8.QLinear.from_float(fc, decode=True, weight_bits=4, group_size=128)
    qw = layer.qweight
    x16 = qrows(p)
    q8.qlinear_decode(x16, qw)
    before = q8.last_launch_q4g()
    assert before == G.plan(16, out, in_, cus=cus)[0]
    y = torch.full((17, out), 7.0, device="cuda")
    xf = torch.ones((17, in_), device="cuda")
    for call in (lambda: layer(xf), lambda: q8.qlinear_decode(xf, qw, out=y), lambda: q8.qlinear_decode(q8.quantize(xf), qw, out=y),
                 lambda: q8.qlinear(xf[:16], qw, out=y[:16]), lambda: q8.qlinear(x16, qw, out=y[:16]), lambda: q8.qlinear(x16, qw, out_scale=1.0),
                 lambda: q8.time_qlinear(xf[:16], qw)):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_UNSUPPORTED and "4-bit" in str(e.value), str(e.value)
    for call in (lambda: q8.QWeight4G(fc.weight.detach(), group_size=64), lambda: q8.QWeight4G(fc.weight.detach(), group_size=0),
                 lambda: q8.QLinear.from_float(fc, decode=True, weight_bits=4, group_size=32),
                 lambda: q8.QLinear.from_float(fc, decode=True, weight_bits=8, group_size=128),
                 lambda: q8.QMLP([qw], decode=False)):
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == H.ERR_INVALID_ARG, str(e.value)
    # the library itself: 17 rows; a scale array 4 bytes off a 16-byte boundary; a pitch_s that is no multiple of 4
    L = q8.lib_q4g()
    rx, work = torch.ones(17, device="cuda"), torch.full((1 << 16,), WORK_FILL, dtype=torch.uint8, device="cuda")
    xq17 = torch.zeros((17, 260), dtype=torch.int8, device="cuda")

    def raw(rows, gs, pitch_s):
        return L.mmh_q4g_linear(0, rows, out, in_, xq17.data_ptr(), 260, rx.data_ptr(), qw.p.data_ptr(), qw.pitch, gs, pitch_s, None, H.ACT_NONE,
                                None, y.data_ptr(), out, None, 0, work.data_ptr(), work.numel(), 1, torch.cuda.current_stream().cuda_stream)

    gs = qw.group_inv_scale.data_ptr()
    assert raw(17, gs, qw.pitch_s) == H.ERR_UNSUPPORTED and b"16 rows" in L.mmh_q4g_last_error()
    assert raw(16, gs + 4, qw.pitch_s) == H.ERR_UNSUPPORTED and b"16-byte" in L.mmh_q4g_last_error()
    assert raw(16, gs, qw.pitch_s + 2) == H.ERR_UNSUPPORTED and b"16-byte" in L.mmh_q4g_last_error()
    assert raw(16, gs, out - 2) == H.ERR_INVALID_ARG
    # from_image: the scale array's shape, device, dtype, pitch and base; the image's rules are QWeight4.from_image's
    groups, prow = G.groups(in_), F.layout(out, in_)[1]
    img = torch.zeros((prow, 144), dtype=torch.uint8, device="cuda")
    flat = torch.ones((4 + (groups + 1) * 136,), dtype=torch.float32, device="cuda")

    def factors(rows=groups, pitch=136, base=4, cols=out):
        return torch.as_strided(flat, (rows, cols), (pitch, 1), base)

    good = q8.QWeight4G.from_image(img[:, :out], factors(), out, in_)
    assert (good.pitch, good.pitch_s, good.group_scale, good.scale, good._ptrs[2]) == (144, 136, None, None, flat.data_ptr() + 16)
    assert good.nbytes == prow * 144 + groups * 136 * 4
    for what, image, g in (("a group too many", img[:, :out], factors(rows=groups + 1)), ("a group short", img[:, :out], factors(rows=groups - 1)),
                           ("too few columns", img[:, :out], factors(cols=out - 1)), ("a pitch of 134", img[:, :out], factors(pitch=134)),
                           ("a base off by 4 bytes", img[:, :out], factors(base=5)), ("factors on the host", img[:, :out], factors().cpu()),
                           ("float64 factors", img[:, :out], factors().double()), ("per-channel factors", img[:, :out], flat[:out]),
                           ("a packed row short", img[:-1, :out], factors()), ("an image on the host", img[:, :out].cpu(), factors())):
        with pytest.raises(H.MMultError) as e:
            q8.QWeight4G.from_image(image, g, out, in_)
        assert e.value.status == H.ERR_INVALID_ARG, (what, str(e.value))
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((work == WORK_FILL).all()) and q8.last_launch_q4g() == before
