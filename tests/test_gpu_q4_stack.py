"""4-bit weights in a stack: q8.QMLP on q8.QWeight4s (alone and mixed with QWeights) bit for bit against a host chain --
qlinear_ref.quantize_rows_ref, then per layer tests/q4_ref.py's want on the packed quantize4_ref image of a 4-bit layer and
qchain_ref.qlinear_s8_ref for an int8 layer, with the hidden layers' static output scales --, every layer's launch text against
its own library's plan, and the refusals that keep a QWeight4 off the tile route: a stack that holds one needs decode=True, takes
at most 16 rows in forward and in calibrate, and q8._linear_s8o -- which would read the packed image as the int8 image of twice
its rows -- refuses it itself.  Only the refusals and the correct route are ever run.

The shape is small with every edge in it, 193 -> 130 -> 47: two 128-k slices with a one-k tail, two strips of which the second
is 2 columns wide, a hidden width that is neither a multiple of 128 nor of 16 (one slice whose high half holds 2 k, rows of
pitch 144)."""
import functools

import numpy as np
import pytest

import q4_ref as P4
import qchain_ref as Q
import qdecode_ref as D
import qlinear_ref as R
import test_gpu_qchain as TC
from bitcmp import first_difference, same_bits
from gpu_operands import cus_fixture, handle_fixture

pytestmark = pytest.mark.gpu

amm = handle_fixture()        # asked for the device's CU count only
cus = cus_fixture("amm")

DIMS = (193, 130, 47)
HAND_SCALE = np.float32(24.0)   # the hidden layer's output scale where it is set by hand
POISON = 0x55


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def problem(rows, seed=0):
    """(x, [(w, bias), (w, bias)]) of DIMS: test_gpu_qchain.mlp_problem's distributions."""
    return TC.mlp_problem(rows, DIMS, 100 * rows + seed)


def layer_ref(bits, xq, rx, w, bias, relu, so=None):
    """One layer on quantised rows: a 4-bit layer through its packed image, an int8 layer through qlinear_s8_ref."""
    if bits == 8:
        return Q.qlinear_s8_ref(xq, rx, w, bias, relu, so)
    q, _, rw = P4.quantize4_ref(w)
    return P4.want(xq, rx, P4.pack_ref(np.ascontiguousarray(q.T)), w.shape[1], rw, bias, relu, so)


def chain(x, layers, bits, scales):
    """(y, [hidden int8 ...]) of the stack: one row quantiser, int8 out under a constant scale and ReLU for every hidden layer,
    fp32 out and no activation for the last."""
    xq, _, rx = R.quantize_rows_ref(x)
    hidden = []
    for (w, b), n, s in zip(layers[:-1], bits, scales):
        so = np.full(xq.shape[0], np.float32(s), np.float32)
        xq, rx = layer_ref(n, xq, rx, w, b, True, so), Q.inv_scale_ref(so)
        hidden.append(xq)
    return layer_ref(bits[-1], xq, rx, *layers[-1], False), hidden


def calibrate_ref(x, layers, bits):
    """QMLP.calibrate: every hidden layer with an fp32 output on its own quantisation of the fp32 rows before it."""
    h, scales = np.asarray(x, np.float32), []
    for (w, b), n in zip(layers[:-1], bits):
        xq, _, rx = R.quantize_rows_ref(h)
        h = layer_ref(n, xq, rx, w, b, True)
        a = np.abs(h)
        scales.append(Q.scale_of_amax(np.where(np.isfinite(a), a, np.float32(0)).max()))
    return scales


def stack(layers, bits, **kw):
    from how_to_optimize_gemm_amd import q8
    return q8.QMLP([(q8.QWeight4 if n == 4 else q8.QWeight)(dev(w)) for (w, _), n in zip(layers, bits)], [dev(b) for _, b in layers], **kw)


def plan_texts(rows, bits, cus):
    """What each layer of the stack launches: the hidden layer into int8 rows of pitch 144, the last into dense fp32 rows."""
    plans = {4: P4.plan, 8: D.plan}
    return [plans[bits[0]](rows, DIMS[1], DIMS[0], True, (DIMS[1] + 15) & ~15, cus=cus)[0], plans[bits[1]](rows, DIMS[2], DIMS[1], cus=cus)[0]]


def spy_on_the_decode_calls(monkeypatch):
    """[(the weight is 4-bit, (q8d, q4d) texts before, after)] of every q8._linear_q8d call from here on."""
    from how_to_optimize_gemm_amd import q8
    real, log = q8._linear_q8d, []

    def call(what, x, qweight, *args, **kw):
        before = (q8.last_launch_q8d(), q8.last_launch_q4d())
        out = real(what, x, qweight, *args, **kw)
        log.append((isinstance(qweight, q8.QWeight4), before, (q8.last_launch_q8d(), q8.last_launch_q4d())))
        return out

    monkeypatch.setattr(q8, "_linear_q8d", call)
    return log


def check_launches(log, bits, texts):
    """Each layer went to its own library, whose text is its plan's; the other library's text stayed."""
    assert [four for four, _, _ in log] == [n == 4 for n in bits]
    for (four, before, after), text in zip(log, texts):
        assert after[four] == text, (after, text)
        assert after[not four] == before[not four], (before, after)


def all_texts():
    from how_to_optimize_gemm_amd import q8
    return q8.last_launch(), q8.last_launch_q8o(), q8.last_launch_q8d(), q8.last_launch_q4d()


def test_the_hand_set_scale_uses_the_hidden_range_without_saturating_it():
    """(The problem, not the kernel: a hidden layer that were all zeros or all 127 would hide a wrong first layer.)"""
    for rows in (1, 16):
        x, layers = problem(rows)
        for bits in ((4, 4), (8, 4)):
            _, (hidden,) = chain(x, layers, bits, [HAND_SCALE])
            assert hidden.shape == (rows, DIMS[1]) and hidden.min() == 0                 # ReLU
            assert len(np.unique(hidden)) >= (20 if rows == 1 else 50) and (hidden == 127).mean() < 0.02, (rows, bits)


@pytest.mark.parametrize("rows", [1, 16])
def test_a_4_bit_stack_is_the_chain(rows, cus, monkeypatch):
    import torch
    from how_to_optimize_gemm_amd import q8
    x, layers = problem(rows)
    mlp = stack(layers, (4, 4), decode=True)
    assert all(isinstance(q, q8.QWeight4) for q in mlp.qweights)
    mlp.out_scales = [HAND_SCALE]
    log = spy_on_the_decode_calls(monkeypatch)
    others = all_texts()[1:3]
    got = mlp(dev(x))
    torch.cuda.synchronize()
    check_launches(log, (4, 4), plan_texts(rows, (4, 4), cus))
    assert all_texts()[1:3] == others                     # neither the int8-output tiles nor the int8 decode library ran
    want, _ = chain(x, layers, (4, 4), [HAND_SCALE])
    assert tuple(got.shape) == (rows, DIMS[2]) and same_bits(got.cpu().numpy(), want), first_difference(got.cpu().numpy(), want)


@pytest.mark.parametrize("bits", [(4, 8), (8, 4)], ids=["q4-q8", "q8-q4"])
def test_a_mixed_stack_is_the_chain_and_each_layer_runs_in_its_own_library(bits, cus, monkeypatch):
    import torch
    rows = 16
    x, layers = problem(rows)
    mlp = stack(layers, bits, decode=True)
    mlp.out_scales = [HAND_SCALE]
    log = spy_on_the_decode_calls(monkeypatch)
    got = mlp(dev(x))
    torch.cuda.synchronize()
    check_launches(log, bits, plan_texts(rows, bits, cus))
    want, _ = chain(x, layers, bits, [HAND_SCALE])
    assert same_bits(got.cpu().numpy(), want), first_difference(got.cpu().numpy(), want)
    assert not same_bits(want, chain(x, layers, (4, 4), [HAND_SCALE])[0])   # (the int8 layer is not the 4-bit one)


def test_calibrate_on_a_4_bit_stack_measures_the_references_hidden_output(cus, monkeypatch):
    """16 rows: calibrate runs the hidden layer through qlinear_decode with an fp32 output -- the only route a QWeight4 has --
    and sets scale_of_amax of its largest finite value; forward afterwards is the chain under that scale."""
    import torch
    rows = 16
    x, layers = problem(rows, 1)
    mlp = stack(layers, (4, 4), decode=True)
    log = spy_on_the_decode_calls(monkeypatch)
    scales = mlp.calibrate(dev(x))
    torch.cuda.synchronize()
    check_launches(log, (4,), [P4.plan(rows, DIMS[1], DIMS[0], cus=cus)[0]])
    want_scales = calibrate_ref(x, layers, (4, 4))
    assert len(scales) == 1 and mlp.out_scales == scales
    assert same_bits(np.array(scales, np.float32), np.array(want_scales, np.float32)), (scales, want_scales)
    got = mlp(dev(x)).cpu().numpy()
    want, (hidden,) = chain(x, layers, (4, 4), want_scales)
    assert hidden.max() == 127                            # the batch's own maximum lands on 127
    assert same_bits(got, want), first_difference(got, want)


def test_the_refusals_launch_nothing(cus):
    """decode=False with a QWeight4 anywhere in the stack is refused at construction; 17 rows are refused by forward and by
    calibrate before the row quantiser runs; q8._linear_s8o refuses a QWeight4.  All four launch texts stay what they were,
    the sentinel output keeps its fill, and the next correct call gives the chain."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    x, layers = problem(16)
    mlp = stack(layers, (4, 4), decode=True)
    mixed = stack(layers, (8, 4), decode=True)
    mlp.out_scales = mixed.out_scales = [HAND_SCALE]
    xd = dev(x)
    want, _ = chain(x, layers, (4, 4), [HAND_SCALE])
    assert same_bits(mlp(xd).cpu().numpy(), want)
    xq = q8.quantize(xd)
    so, inv = q8._scale_vectors("test", float(HAND_SCALE), 16, 0)
    sentinel = torch.full((16, 144), POISON, dtype=torch.int8, device="cuda")
    wide = torch.zeros((17, DIMS[0]), device="cuda")
    torch.cuda.synchronize()
    before = all_texts()
    assert before[0] and before[3]                        # the row quantiser's and the 4-bit layer's, from the calls above
    refusals = [
        ("decode=False", H.ERR_INVALID_ARG, lambda: q8.QMLP(mlp.qweights, None)),
        ("decode=False, mixed", H.ERR_INVALID_ARG, lambda: q8.QMLP(mixed.qweights, None, decode=False)),
        ("forward, 17 rows", H.ERR_UNSUPPORTED, lambda: mlp(wide)),
        ("forward, 17 rows as 17 x 1 x in", H.ERR_UNSUPPORTED, lambda: mlp(wide.reshape(17, 1, DIMS[0]))),
        ("forward, 17 rows, mixed", H.ERR_UNSUPPORTED, lambda: mixed(wide)),
        ("calibrate, 17 rows", H.ERR_UNSUPPORTED, lambda: mlp.calibrate(wide)),
        ("calibrate, 17 rows, mixed", H.ERR_UNSUPPORTED, lambda: mixed.calibrate(wide)),
        ("_linear_s8o", H.ERR_UNSUPPORTED, lambda: q8._linear_s8o("test", xq, mlp.qweights[0], mlp.bias0, "relu", so, inv, out=sentinel[:, :DIMS[1]])),
        ("_linear_s8o, timed", H.ERR_UNSUPPORTED,
         lambda: q8._linear_s8o("test", xq, mlp.qweights[0], mlp.bias0, "relu", so, inv, out=sentinel[:, :DIMS[1]], time=(1, 1))),
    ]
    for what, status, call in refusals:
        with pytest.raises(H.MMultError) as e:
            call()
        assert e.value.status == status, (what, str(e.value))
        assert status == H.ERR_INVALID_ARG or "4-bit" in str(e.value), (what, str(e.value))
        assert all_texts() == before, what
    torch.cuda.synchronize()
    assert bool((sentinel == POISON).all())
    assert mlp.out_scales == [float(HAND_SCALE)] and mixed.out_scales == [float(HAND_SCALE)]   # a refused calibrate sets nothing
    assert same_bits(mlp(xd).cpu().numpy(), want)
    assert same_bits(mixed(xd).cpu().numpy(), chain(x, layers, (8, 4), [HAND_SCALE])[0])


def test_a_captured_4_bit_stack_replays_the_chain_on_rewritten_rows():
    """reserve_decode() on both weights and one eager forward at 16 rows on the capture stream (the scale vectors and the
    workspaces have their sizes), then forward captured and replayed twice with x rewritten in between: each replay is the
    chain.  Every launch goes to the one capturing stream: the graph is a chain of kernel nodes, no parallel branches."""
    import torch
    rows = 16
    x0, layers = problem(rows)
    mlp = stack(layers, (4, 4), decode=True)
    mlp.out_scales = [HAND_SCALE]
    for qw in mlp.qweights:
        qw.reserve_decode()
    reserved = [qw._decode_work.data_ptr() for qw in mlp.qweights]
    x = dev(x0)
    side = TC._side_stream()
    with torch.cuda.stream(side):
        mlp(x)
    side.synchronize()
    held = []
    graph = TC._capture(side, lambda: held.append(mlp(x)))
    y, = held
    assert [qw._decode_work.data_ptr() for qw in mlp.qweights] == reserved
    rng = np.random.default_rng(8)
    for rep in range(2):
        a = (rng.standard_normal((rows, DIMS[0])) * (rep + 1)).astype(np.float32)
        x.copy_(torch.from_numpy(a))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        want, _ = chain(a, layers, (4, 4), [HAND_SCALE])
        assert same_bits(got, want), (rep, first_difference(got, want))
    del graph, held, y


def test_the_4_bit_module_at_one_row_and_one_k_past_a_slice(cus):
    """QLinear(weight_bits=4, decode=True) at in = 129 -- one k in the second slice -- and one row, given as 1 x 1 x 129."""
    import torch
    from how_to_optimize_gemm_amd import q8
    in_, out = 129, 130
    rng = np.random.default_rng(129)
    w = (rng.uniform(-1, 1, (out, in_)) / np.sqrt(in_)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, out).astype(np.float32)
    x = (rng.standard_normal((1, 1, in_)) * 2).astype(np.float32)
    layer = q8.QLinear(in_, out, True, "relu", decode=True, weight_bits=4).set_weight(dev(w), dev(b))
    assert isinstance(layer.qweight, q8.QWeight4)
    got = layer(dev(x))
    assert q8.last_launch_q4d() == P4.plan(1, out, in_, cus=cus)[0]
    torch.cuda.synchronize()
    xq, _, rx = R.quantize_rows_ref(x.reshape(1, in_))
    want = layer_ref(4, xq, rx, w, b, True)
    assert (want > 0).any() and (want == 0).any()
    assert tuple(got.shape) == (1, 1, out) and same_bits(got.cpu().numpy().reshape(1, out), want), first_difference(got.cpu().numpy().reshape(1, out), want)
