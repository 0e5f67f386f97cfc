"""Int8-to-int8 linear layers on the GPU (libmmult_hip_q8o.so, mmh_q8_linear_s8, q8.QRows / q8.QMLP), bit for bit against
tests/qchain_ref.py.

Q8O_INSTANTIATIONS holds one row per kernel symbol of the third library (tests/test_q8o_kernel_census.py holds the table to the
library, both ways): qlinear_s8o_kernel at 128x128 and 256x256, whole and guarded.  Every run reads int8 rows whose pad bytes
are poisoned with 0x55 and writes into a buffer poisoned with 0x55 -- in front of the window, behind every row, behind the
last row -- of which only the rows x out bytes may change.

The 256x256 shapes are chosen by csrc/igemm_plan.hpp's i8_big_tile with the test device's CU count (qlinear_ref.big_tile):
the multiple-of-256 shape of the fewest elements that takes the big tile, and its neighbour 3 rows and 5 columns short."""
import collections
import functools

import numpy as np
import pytest

import qchain_ref as Q
import qlinear_ref as R
from bitcmp import first_difference, same_bits
from gpu_operands import cus_fixture, handle_fixture
from qlinear_ref import IN_256, shapes_256

pytestmark = pytest.mark.gpu

amm = handle_fixture()        # asked for the device's CU count only
cus = cus_fixture("amm")

Row = collections.namedtuple("Row", "symbol tile edge")
_B = {False: "false", True: "true"}
Q8O_INSTANTIATIONS = [Row(f"qlinear_s8o_kernel<{t},{t},{t // 32},{_B[e]}>", t, e) for t in (128, 256) for e in (False, True)]

SHAPES_128 = {False: [(128, 128, 128), (128, 128, 64)], True: [(129, 130, 131), (5, 3, 7), (1, 1, 1)]}
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]   # (bias, ReLU)
POISON = 0x55


@functools.lru_cache(maxsize=4)
def problem(rows, out, in_):
    """Inputs of a shape and the parts of its reference every epilogue shares: x's quantised rows and row factors, the
    integer sums, the channel factors, and one output scale per row -- chosen from the fp32 layer's |y| so that the
    quantised output uses the whole range and clamps a few elements per thousand, every row with a scale of its own."""
    rng = np.random.default_rng(rows * 7 + out * 3 + in_ + 2)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    xq, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(xq, qw)
    return w, bias, xq, rx, acc, rw, out_scales(acc, rx, rw, bias)


def out_scales(acc, rx, rw, bias):
    """problem()'s scale rule: one output scale per row from the fp32 layer's |y| (its 99.8th percentile where there are a
    thousand outputs, else just above its maximum), stepped down by up to 10 % from row to row."""
    return scales_of(R.epilogue_ref(acc, rx, rw, bias, False))


def scales_of(y):
    """out_scales of the fp32 layer's outputs themselves."""
    a = np.abs(y)
    top = np.float32(np.percentile(a, 99.8)) if a.size >= 1000 else np.float32(a.max() * 1.03 + 1e-3)
    return (np.float32(127.0) / top * (1 - 0.1 * ((np.arange(y.shape[0]) * 37) % 16) / 16)).astype(np.float32)


def want_of(p, bias, relu):
    w, b, xq, rx, acc, rw, so = p
    return Q.requant_ref(R.epilogue_ref(acc, rx, rw, b if bias else None, relu), so)


_weights = {}


def weight_of(key, w):
    """One prepared weight per shape (the epilogue variants of a shape share it)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    if key not in _weights:
        _weights.clear()
        _weights[key] = q8.QWeight(torch.from_numpy(w).cuda())
    return _weights[key]


def poisoned_rows(values, ld, off=0):
    """(flat, view): an int8 device buffer full of 0x55 and the rows x ld view `off` bytes past a 16-byte boundary of it, with
    `values` (int8, rows x cols) in its first columns -- the pad bytes of every row stay 0x55."""
    import torch
    rows, cols = values.shape
    flat = torch.full((16 + off + rows * ld + 64,), POISON, dtype=torch.int8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[16 + off:16 + off + rows * ld].view(rows, ld)
    if cols:
        view[:, :cols] = torch.from_numpy(np.ascontiguousarray(values)).cuda()
    return flat, view


def device_rows(xq, rx, pad=4, off=0):
    """The QRows of reference rows: pitch = cols rounded up to 4, plus `pad`, poisoned behind every row; the base `off` bytes
    past a 16-byte boundary."""
    import torch
    from how_to_optimize_gemm_amd import q8
    ld = ((xq.shape[1] + 3) & ~3) + pad
    _, view = poisoned_rows(xq, ld, off)
    return q8.QRows(view[:, :xq.shape[1]], torch.from_numpy(np.ascontiguousarray(rx)).cuda())


def run_s8o(qw, xq, rx, bias, relu, so, ldyq, off_y, x_pad=4, x_off=0):
    """The int8-output layer into a poisoned buffer: yq's window starts off_y bytes past a 16-byte boundary, its rows are ldyq
    bytes apart; x's rows have x_pad poisoned bytes behind them and start x_off bytes past a 16-byte boundary.  Returns (yq's
    window, nothing outside it was written, the launch text)."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, out = xq.shape[0], qw.out_features
    flat, yv = poisoned_rows(np.zeros((rows, 0), np.int8), ldyq, off_y)
    db = None if bias is None else torch.from_numpy(bias).cuda()
    got = q8.qlinear(device_rows(xq, rx, x_pad, x_off), qw, db, "relu" if relu else None, out=yv[:, :out], out_scale=torch.from_numpy(so).cuda())
    launched = q8.last_launch_q8o()
    torch.cuda.synchronize()
    assert got.q.data_ptr() == yv.data_ptr() and same_bits(got.inv_scale.cpu().numpy(), Q.inv_scale_ref(so))
    after = flat.cpu().numpy().copy()
    window = after[16 + off_y:16 + off_y + rows * ldyq].reshape(rows, ldyq)
    result = window[:, :out].copy()
    window[:, :out] = POISON
    return result, bool((after == POISON).all()), launched


def check_s8o(shape, p, qw, bias, relu, ldyq, off_y, symbol, cu_count, want=None, x_pad=4, x_off=0):
    rows, out, in_ = shape
    w, b, xq, rx, acc, rw, so = p
    want = want_of(p, bias, relu) if want is None else want
    got, untouched, launched = run_s8o(qw, xq, rx, b if bias else None, relu, so, ldyq, off_y, x_pad, x_off)
    assert launched == Q.plan_text_s8o(rows, out, ldyq, off_y % 4, cu_count) and symbol in launched, (shape, symbol, launched)
    assert np.array_equal(got, want), (shape, launched, int((got != want).sum()), np.argwhere(got != want)[:4])
    assert untouched, (shape, launched, "wrote outside yq's rows x out bytes")


@pytest.mark.parametrize("row", Q8O_INSTANTIATIONS, ids=lambda r: r.symbol)
def test_every_instantiation_is_reached_and_is_the_contract(row, cus):
    shapes = SHAPES_128[row.edge] if row.tile == 128 else [shapes_256(cus)[1 if row.edge else 0]]
    for shape in shapes:
        p = problem(*shape)
        # on the host, before any launch: the expected bytes are no constant and do not saturate (asked of the shapes that have
        # a thousand elements; (5, 3, 7) and (1, 1, 1) ride on the same scale rule)
        wants = {e: want_of(p, *e) for e in EPILOGUES}
        if shape[0] * shape[1] >= 1000:
            for e, want in wants.items():
                assert len(np.unique(want)) >= 100 and (np.abs(want) == 127).mean() < 0.01, (shape, e, len(np.unique(want)))
        qw = weight_of(shape, p[0])
        out = shape[1]
        ldyq, off = ((out + 15) & ~15, 0) if not row.edge else (out + 7 + out % 2, 1)   # guarded: an odd pitch, a base 1 byte off
        for e in EPILOGUES:
            check_s8o(shape, p, qw, *e, ldyq, off, row.symbol, cus, wants[e])


# ---- the store path ---------------------------------------------------------------------------------------------------------
THIN = (1, 3, 4, 5, 15, 16, 17)   # last tiles this wide and this high
KS = (1, 129, 257, 513)           # one to four trips of the K loop in front of the epilogue
StoreCase = collections.namedtuple("StoreCase", "rows out in_ ldyq off")


def store_cases():
    cases = []
    for i, t in enumerate(THIN):
        out = 128 + THIN[(i + 3) % 7]
        ldyq = out + 5 + (out + 5 + 1) % 2 if i % 2 == 0 else out + 4 + (2 - (out + 4) % 4) % 4   # odd; 2 modulo 4
        cases.append(StoreCase(128 + t, out, KS[i % 4], ldyq, (1, 2, 3)[i % 3]))
    cases += [StoreCase(128, 128, 257, 144, 1), StoreCase(128, 128, 129, 144, 2), StoreCase(128, 128, 513, 144, 3),   # whole tiles,
              StoreCase(128, 128, 257, 146, 0), StoreCase(128, 128, 1, 131, 0),        # guarded by the base or by the pitch alone
              StoreCase(133, 143, 129, 144, 0), StoreCase(131, 130, 257, 132, 0),      # ragged, in dwords: the last lanes in bytes
              StoreCase(129, 145, 513, 147, 0), StoreCase(144, 132, 129, 134, 2)]      # ... a pitch, a base that take bytes
    return cases


def test_the_store_cases_are_what_they_promise():
    cases = store_cases()
    assert {c.rows - 128 for c in cases[:7]} == set(THIN) == {c.out - 128 for c in cases[:7]}
    assert {c.ldyq % 4 for c in cases[:7]} == {1, 2, 3} and {c.ldyq % 2 for c in cases[:7]} == {0, 1}
    assert {c.off for c in cases} == {0, 1, 2, 3} and {c.in_ for c in cases} == set(KS)
    assert all(c.ldyq >= c.out for c in cases)
    whole = [c for c in cases if c.rows % 128 == 0 and c.out % 128 == 0]
    assert whole and all(c.ldyq % 4 or c.off for c in whole)            # guarded by misalignment alone
    assert any(c.ldyq % 4 == 0 and c.off == 0 and c.out % 4 for c in cases)


@pytest.mark.parametrize("index", range(len(store_cases())))
def test_the_store_path(index, cus):
    """Guarded 128x128 tiles with thin last tiles, pitches that are odd or 2 modulo 4, bases 1 - 3 bytes past a dword, whole
    tiles guarded by misalignment alone, behind one to four trips of the K loop."""
    import torch
    from how_to_optimize_gemm_amd import q8
    c = store_cases()[index]
    p = problem(c.rows, c.out, c.in_)
    qw = q8.QWeight(torch.from_numpy(p[0]).cuda())
    for e in ((True, True), (False, False)):
        check_s8o((c.rows, c.out, c.in_), p, qw, *e, c.ldyq, c.off, "qlinear_s8o_kernel<128,128,4,true>", cus)
    qw.close()


# ---- rounding ---------------------------------------------------------------------------------------------------------------
BIASES = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5, -126.5, 127.5, -127.5, 1e6, -1e6, np.nan, np.inf, -np.inf, -0.0,
                   1.0, 3.0, 5.0, -1.0, -3.0, 253.0, -253.0, 255.0, -255.0, 0.25, 77.3, -77.3], np.float32)


def test_rounding_of_the_requantisation(cus):
    """in == 0 and a zero x: y is the bias.  Ties of both parities, the clamp on both sides, NaN, +-inf, -0, at so = 1 and 0.5."""
    import torch
    from how_to_optimize_gemm_amd import q8
    out = len(BIASES)
    so = np.array([1.0, 0.5, 1.0, 0.5, 0.5], np.float32)
    rows = len(so)
    # on the host: the scaled values hold ties at both parities and values that clamp, at either scale
    for s in (1.0, 0.5):
        t = BIASES[np.isfinite(BIASES)].astype(np.float64) * s
        ties = t[(np.abs(t) < 127) & (t - np.floor(t) == 0.5)]
        assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any() and (t > 127).any() and (t < -127).any(), s
    qw = q8.QWeight(torch.full((out, 16), float("nan"), device="cuda")[:, :0])   # (an (out, 0) window with a row stride)
    xq = q8.QRows(torch.empty((rows, 16), dtype=torch.int8, device="cuda")[:, :0], torch.ones(rows, device="cuda"))
    acc, ones = np.zeros((rows, out), np.int32), np.ones(rows, np.float32)
    for relu in (False, True):
        want = Q.requant_ref(R.epilogue_ref(acc, ones, np.ones(out, np.float32), BIASES, relu), so)
        flat, yv = poisoned_rows(np.zeros((rows, 0), np.int8), out + 3, 1)
        q8.qlinear(xq, qw, torch.from_numpy(BIASES).cuda(), "relu" if relu else None, out=yv[:, :out], out_scale=torch.from_numpy(so).cuda())
        torch.cuda.synchronize()
        got = yv[:, :out].cpu().numpy()
        assert np.array_equal(got, want), (relu, got, want)
        assert (yv[:, out:] == POISON).all() and (flat[:17] == POISON).all()
        if not relu:
            assert list(got[0][:11]) == [0, 2, 2, 4, 0, -2, -2, 126, -126, 127, -127] and list(got[0][11:17]) == [127, -127, 0, 127, -127, 0]
            assert list(got[1][17:26]) == [0, 2, 2, 0, -2, 126, -126, 127, -127]
        else:
            assert not (got < 0).any() and got[0][14] == 127 and got[0][13] == 0
    # the fp32 output of the same rows: the bias itself (mmh_q8_linear_s8 with in == 0)
    y = q8.qlinear(xq, qw, torch.from_numpy(BIASES).cuda()).cpu().numpy()
    assert same_bits(y, R.epilogue_ref(acc, ones, np.ones(out, np.float32), BIASES, False))
    qw.close()


def test_time_qlinear_s8o_leaves_the_contract_in_yq_and_returns_a_time(cus):
    import math
    import torch
    from how_to_optimize_gemm_amd import q8
    p = problem(129, 130, 131)
    w, b, xq, rx, acc, rw, so = p
    qw = q8.QWeight(torch.from_numpy(w).cuda())
    flat, yv = poisoned_rows(np.zeros((129, 0), np.int8), 144)
    ms = q8.time_qlinear_s8o(device_rows(xq, rx), qw, torch.from_numpy(b).cuda(), "relu", out=yv[:, :130], out_scale=torch.from_numpy(so).cuda(),
                             warmup=1, reps=3)
    torch.cuda.synchronize()
    assert np.array_equal(yv[:, :130].cpu().numpy(), want_of(p, True, True)) and bool((yv[:, 130:] == POISON).all())
    assert math.isfinite(ms) and ms > 0, ms
    qw.close()


# ---- pre-quantised input, fp32 output ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(128, 128, 64), (129, 130, 131)], ids=["whole", "guarded"])
def test_a_layer_on_quantised_rows_is_the_layer_on_the_float_rows(shape, cus):
    """qlinear(quantize(x), ...) is qlinear(x, ...) bit for bit, launches the fp32 call's GEMM and nothing else, and one QRows
    feeds two different weights; rows with poisoned bytes behind `in` give the same."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    rows, out, in_ = shape
    rng = np.random.default_rng(41 + rows)
    x = (rng.standard_normal((rows, in_)) * 3).astype(np.float32)
    ws = [rng.uniform(-0.5, 0.5, (out, in_)).astype(np.float32), rng.uniform(-2, 2, (out + 16, in_)).astype(np.float32)]
    bias = rng.uniform(-4, 4, out + 16).astype(np.float32)
    dx, db = torch.from_numpy(x).cuda(), torch.from_numpy(bias).cuda()
    xq = q8.quantize(dx)
    ref_q, _, ref_rx = R.quantize_rows_ref(x)
    poisoned = device_rows(ref_q, ref_rx, pad=8)
    assert (poisoned.q.cpu().numpy() == ref_q).all() and poisoned._ld >= in_ + 8
    for w in ws:
        qw = q8.QWeight(torch.from_numpy(w).cuda())
        n = w.shape[0]
        for b, act in ((None, None), (db[:n], "relu")):
            direct = q8.qlinear(dx, qw, b, act)
            text = q8.last_launch()
            got = q8.qlinear(xq, qw, b, act)
            assert q8.last_launch() == text.split("then ")[1] == R.plan_text(rows, n, in_, 0, 0, 0, 0, b is not None, act == "relu", cus)[0].split("then ")[1]
            again = q8.qlinear(poisoned, qw, b, act)
            torch.cuda.synchronize()
            want = R.qlinear_ref(x, w, None if b is None else bias[:n], act == "relu")
            for name, y in (("the fp32 call", direct), ("quantize(x)", got), ("poisoned pad bytes", again)):
                assert same_bits(y.cpu().numpy(), want), (name, shape, first_difference(y.cpu().numpy(), want))
        # what the entry point refuses: rows shorter than `in`, an odd pitch, a base that is not dword aligned
        L, ok = q8.lib(), (rows, xq._ptr, xq._ld, xq.inv_scale.data_ptr(), None, H.ACT_NONE, got.data_ptr(), n, None)
        for i, bad, status in ((2, in_ - 1, H.ERR_INVALID_ARG), (2, xq._ld + 1, H.ERR_UNSUPPORTED), (1, xq._ptr + 1, H.ERR_UNSUPPORTED),
                               (3, None, H.ERR_INVALID_ARG), (5, 7, H.ERR_INVALID_ARG)):
            args = list(ok)
            args[i] = bad
            assert L.mmh_q8_linear_s8(qw._handle, *args) == status, (i, bad)
        torch.cuda.synchronize()
        assert same_bits(got.cpu().numpy(), want)   # (the refused calls touched nothing)
        qw.close()
    with pytest.raises(H.MMultError):
        q8.QRows(poisoned.q[:, 1:], poisoned.inv_scale)   # a base one byte past a dword


# ---- the chain --------------------------------------------------------------------------------------------------------------
def mlp_problem(rows, dims, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, dims[0])) * 2).astype(np.float32)
    layers = [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.float32(np.sqrt(i)), rng.uniform(-0.5, 0.5, o).astype(np.float32))
              for i, o in zip(dims, dims[1:])]
    return x, layers


def test_the_chain_in_place(cus):
    """Layer 1 writes int8 rows of 70 bytes at pitch 80 into a poisoned buffer; layer 2 reads that image as it is."""
    import torch
    from how_to_optimize_gemm_amd import q8
    for rows, dims, whole in ((37, (50, 70, 33), False), (128, (128, 256, 128), True)):
        x, layers = mlp_problem(rows, dims, rows)
        scale, = Q.calibrate_ref(x, layers)
        want, (hidden,) = Q.chain_ref(x, layers, [scale])
        assert len(np.unique(hidden)) >= 50 and (hidden == 127).mean() < 0.01
        qws = [q8.QWeight(torch.from_numpy(w).cuda()) for w, _ in layers]
        bs = [torch.from_numpy(b).cuda() for _, b in layers]
        pitch = (dims[1] + 15) & ~15
        flat, hv = poisoned_rows(np.zeros((rows, 0), np.int8), pitch)
        h = q8.qlinear(q8.quantize(torch.from_numpy(x).cuda()), qws[0], bs[0], "relu", out=hv[:, :dims[1]], out_scale=float(scale))
        first = q8.last_launch_q8o()
        y = q8.qlinear(h, qws[1], bs[1])
        second = q8.last_launch()
        torch.cuda.synchronize()
        assert h.q.data_ptr() == hv.data_ptr() and h._ld == pitch
        assert np.array_equal(hv[:, :dims[1]].cpu().numpy(), hidden)
        assert (hv[:, dims[1]:] == POISON).all() and (flat[:16] == POISON).all() and (flat[16 + rows * pitch:] == POISON).all()
        assert same_bits(h.inv_scale.cpu().numpy(), np.full(rows, np.float32(1) / scale, np.float32))
        got = y.cpu().numpy()
        assert same_bits(got, want), (dims, first_difference(got, want))
        assert first == Q.plan_text_s8o(rows, dims[1], pitch, 0, cus) and (f"<128,128,4,{_B[not whole]}>" in first), first
        assert f"qlinear_s8_kernel<128,128,4,{_B[not whole]},true,false>" in second, second
        # a fp32 x with an out_scale quantises first: the same bytes, in rows of the default pitch
        h2 = q8.qlinear(torch.from_numpy(x).cuda(), qws[0], bs[0], "relu", out_scale=float(scale))
        assert h2.q.stride(0) == pitch and np.array_equal(h2.q.cpu().numpy(), hidden)
        for qw in qws:
            qw.close()


def _side_stream():
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return side


def _capture(side, body):
    import torch
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def test_a_captured_chain_replays_the_contract_on_new_inputs():
    """The three launches of a two-layer QMLP -- row quantiser, int8 -> int8, int8 -> fp32 -- captured after one eager run on the
    capture stream and replayed three times on new x: each replay is the eager result and the reference.  Nothing was
    reserved: no launch of the chain uses a weight object's scratch."""
    import torch
    from how_to_optimize_gemm_amd import q8
    rows, dims = 77, (200, 130, 60)
    x0, layers = mlp_problem(rows, dims, 5)
    scale = np.float32(9.0)
    mlp = q8.QMLP([q8.QWeight(torch.from_numpy(w).cuda()) for w, _ in layers], [torch.from_numpy(b).cuda() for _, b in layers])
    mlp.out_scales = [scale]
    x = torch.from_numpy(x0).cuda()
    side = _side_stream()
    with torch.cuda.stream(side):
        mlp(x)
    side.synchronize()
    held = []
    graph = _capture(side, lambda: held.append(mlp(x)))
    y, = held
    rng = np.random.default_rng(6)
    for rep in range(3):
        a = (rng.standard_normal((rows, dims[0])) * (rep + 1)).astype(np.float32)
        x.copy_(torch.from_numpy(a))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        want, _ = Q.chain_ref(a, layers, [scale])
        assert same_bits(got, want), (rep, first_difference(got, want))
        h = q8.qlinear(q8.quantize(x.clone()), mlp.qweights[0], mlp.bias0, "relu", out_scale=float(scale))
        eager = q8.qlinear(h, mlp.qweights[1], mlp.bias1).cpu().numpy()
        assert same_bits(got, eager), rep
    del graph, held, y


def test_the_mlp_is_the_chain_and_lies_within_the_quantisation_bound():
    """QMLP.from_float of nn.Linear(96 -> 80 -> 48) with ReLU between: after calibrate(x), forward(x) equals chain_ref, and lies
    within an analytic bound of the fp32 MLP.

    The bound.  Layer 1 is the single layer of test_gpu_qlinear's module test: with d(v) = max|v| / 254 and S(v) = sum|v_k|,
        |h^_k - h_k| <= S(x) d(w1_k) + d(x) S(w1_k) + K1 d(x) d(w1_k) + (K1 + 8) 2^-24 (sum|x w1_k| (1 + 3/127) + |b1_k|) =: B1_k
    for the fp32 outputs h^ of the int8 layer against the exact hidden h (ReLU does not stretch a difference).  calibrate sets
    so = 127 / max|h^| over this batch, and forward's layer 1 forms the same h^ (same rows, same contract), so h^ so lies in
    [-127 (1 + 2^-23), 127 (1 + 2^-23)]: rint never clamps and the bytes g_k = q_k / so are off by at most half a step plus the
    product's rounding, |g_k - h^_k| <= (1/2 + 2^-16) / so =: E.  Layer 2 reads the bytes q exactly as they are (its input needs
    no quantisation) with rx = fl(1 / so); only its weights are rounded, |w2q_jk - w2_jk| <= d(w2_j).  So against the exact
    y_j = sum_k w2_jk h_k + b2_j:
        |y^_j - y_j| <= sum_k |w2_jk| (B1_k + E) + d(w2_j) sum_k |g_k| + (K2 + 8) 2^-24 (sum_k |g_k w2_jk| (1 + 3/127) + |b2_j|)
    the last term covering y^'s three roundings, the rounded reciprocals and the fp32 MLP's own K-term sums.  Both sides in
    float64."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    torch.manual_seed(4)
    fc1, fc2 = torch.nn.Linear(96, 80).cuda(), torch.nn.Linear(80, 48).cuda()
    mlp = q8.QMLP.from_float([fc1, fc2])
    x = torch.randn(2, 5, 96, device="cuda")
    with pytest.raises(H.MMultError):
        mlp(x)                                    # not calibrated
    with pytest.raises(H.MMultError):
        mlp.calibrate(x.clone().requires_grad_())
    scales = mlp.calibrate(x)
    with pytest.raises(H.MMultError):
        mlp(x.clone().requires_grad_())
    y = mlp(x)
    assert tuple(y.shape) == (2, 5, 48)
    xn = x.reshape(10, 96).cpu().numpy()
    layers = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in (fc1, fc2)]
    want_scales = Q.calibrate_ref(xn, layers)
    assert [np.float32(s) for s in scales] == want_scales and mlp.out_scales == scales
    want, (hidden,) = Q.chain_ref(xn, layers, want_scales)
    got = y.reshape(10, 48).cpu().numpy()
    assert same_bits(got, want), first_difference(got, want)
    with np.errstate(all="ignore"):
        scaled = R.qlinear_ref(xn, *layers[0], True) * want_scales[0]
    assert hidden.max() == 127 and scaled.max() < 127.5 and scaled.min() >= 0     # the batch's maximum lands on 127: nothing clamps
    with torch.no_grad():
        fp32 = fc2(torch.relu(fc1(x))).reshape(10, 48).cpu().numpy().astype(np.float64)
    (w1, b1), (w2, b2) = [(w.astype(np.float64), b.astype(np.float64)) for w, b in layers]
    ax, a1, a2 = np.abs(xn).astype(np.float64), np.abs(w1), np.abs(w2)
    dx, d1, d2 = ax.max(axis=1) / 254, a1.max(axis=1) / 254, a2.max(axis=1) / 254
    B1 = ax.sum(axis=1)[:, None] * d1[None, :] + dx[:, None] * a1.sum(axis=1)[None, :] + 96 * dx[:, None] * d1[None, :] + \
        (96 + 8) * 2.0 ** -24 * ((ax @ a1.T) * (1 + 3 / 127) + np.abs(b1)[None, :])
    so = float(want_scales[0])
    E = (0.5 + 2.0 ** -16) / so
    g = np.abs(hidden.astype(np.float64)) / so
    bound = (B1 + E) @ a2.T + g.sum(axis=1)[:, None] * d2[None, :] + (80 + 8) * 2.0 ** -24 * ((g @ a2.T) * (1 + 3 / 127) + np.abs(b2)[None, :])
    err = np.abs(got.astype(np.float64) - fp32)
    assert (err <= bound).all(), (err - bound).max()
    assert err.max() > 0 and np.isfinite(bound).all()
    # scales by hand, a last activation, no biases
    p1, p2 = torch.nn.Linear(96, 80, bias=False).cuda(), torch.nn.Linear(80, 48, bias=False).cuda()
    plain = q8.QMLP.from_float([p1, p2], last_activation="relu")
    plain.out_scales = [20.0]
    assert plain.out_scales == [20.0] and plain.bias0 is None
    want, _ = Q.chain_ref(xn, [(p1.weight.detach().cpu().numpy(), None), (p2.weight.detach().cpu().numpy(), None)], [np.float32(20.0)], True, True)
    got = plain(x).reshape(10, 48).cpu().numpy()
    assert same_bits(got, want), first_difference(got, want)
