"""The linear layer's backward captured into a hipGraph: a captured mmh_relu_grad_colsum replays the contract's bits on new
inputs; a captured call that would have to grow the partial-row workspace is refused and disturbs nothing; a graph survives a
later eager call that grows the workspace (the buffer it points at is retired, not freed); MMult.linear_backward and a training
step of autograd.Linear captured whole replay the eager bits.  Everything is captured on one side stream: no graph here has
parallel branches."""

import numpy as np
import pytest

import relu_grad_ref as ref
from built_lib import REPO
from gpu_operands import handle_fixture

pytestmark = pytest.mark.gpu

R = ref.header_block_rows(REPO)
SMALL, LARGE = (2 * R + 1, 64), (17 * R + 77, 260)     # 3 blocks; 18 blocks (a batch of 16 partial rows plus one)
FILL = -777.25


amm = handle_fixture()   # the module's own handle on MMH_KERNEL_AUTO (the session fixture's `mfma` kernel has no op forms)


def _inputs(shape, seed):
    """(g, y, old) and the contract's (dz, gated sums, ungated sums added to old) for a seed."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape).astype(np.float32)
    y = np.maximum(rng.standard_normal(shape), 0).astype(np.float32)
    old = rng.standard_normal(shape[1]).astype(np.float32)
    dz, s = ref.relu_grad_colsum(g, y, R)
    return g, y, old, dz, s, ref.blocked_colsum(g, R, old)


def _side_stream(torch):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return side


def _put(torch, t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def test_a_captured_relu_grad_colsum_replays_the_contract(amm):
    import torch
    big = _inputs(LARGE, 100)
    small = _inputs(SMALL, 200)
    g1, y1 = (torch.from_numpy(a).cuda() for a in big[:2])
    dz1, s1 = torch.empty_like(g1), torch.empty(LARGE[1], device="cuda")
    g2, acc2 = torch.from_numpy(small[0]).cuda(), torch.from_numpy(small[2].copy()).cuda()
    amm.relu_grad_colsum(g1, y1, dz=dz1, bias_grad=s1)            # the one uncaptured call at the largest size
    torch.cuda.synchronize()
    assert ref.same_bits(s1.cpu().numpy(), big[4])
    side = _side_stream(torch)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            amm.relu_grad_colsum(g1, y1, dz=dz1, bias_grad=s1)
            amm.relu_grad_colsum(g2, None, want_dz=False, bias_grad=acc2, accumulate=True)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(3):
        big, small = _inputs(LARGE, 101 + rep), _inputs(SMALL, 201 + rep)
        _put(torch, g1, big[0]), _put(torch, y1, big[1]), _put(torch, g2, small[0]), _put(torch, acc2, small[2])
        dz1.fill_(FILL), s1.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert ref.same_bits(dz1.cpu().numpy(), big[3]), rep
        assert ref.same_bits(s1.cpu().numpy(), big[4]), rep
        assert ref.same_bits(acc2.cpu().numpy(), small[5]), rep
        assert ref.same_bits(g1.cpu().numpy(), big[0]) and ref.same_bits(g2.cpu().numpy(), small[0]), rep


def test_a_captured_call_that_would_grow_the_workspace_is_refused_and_disturbs_nothing():
    import torch
    import how_to_optimize_gemm_amd as H
    small, big = _inputs(SMALL, 300), _inputs(LARGE, 301)
    g, y = (torch.from_numpy(a).cuda() for a in small[:2])
    dz, s = torch.empty_like(g), torch.empty(SMALL[1], device="cuda")
    gb, yb = (torch.from_numpy(a).cuda() for a in big[:2])
    dzb, sb = torch.full(LARGE, FILL, device="cuda"), torch.full((LARGE[1],), FILL, device="cuda")
    with H.MMult(0, "auto") as own:                                # a handle that has only ever run the small shape
        own.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
        torch.cuda.synchronize()
        dz.fill_(FILL), s.fill_(FILL)
        side = _side_stream(torch)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                own.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
                with pytest.raises(H.MMultError) as e:
                    own.relu_grad_colsum(gb, yb, dz=dzb, bias_grad=sb)
        torch.cuda.current_stream().wait_stream(side)
        assert e.value.status == H.ERR_UNSUPPORTED
        graph.replay()
        torch.cuda.synchronize()
        assert ref.same_bits(dz.cpu().numpy(), small[3]) and ref.same_bits(s.cpu().numpy(), small[4])
        assert torch.all(dzb == FILL).item() and torch.all(sb == FILL).item()
        # ... and the handle is not poisoned: the same call, uncaptured, grows the workspace and runs
        own.relu_grad_colsum(gb, yb, dz=dzb, bias_grad=sb)
        torch.cuda.synchronize()
        assert ref.same_bits(dzb.cpu().numpy(), big[3]) and ref.same_bits(sb.cpu().numpy(), big[4])
        del graph


def test_a_graph_survives_a_later_call_that_grows_the_workspace():
    """The graph points at the workspace of its capture.  A later eager call at a larger size must not free that buffer under
    it: from the first captured use on, a workspace that has to grow is retired and lives as long as the handle."""
    import torch
    import how_to_optimize_gemm_amd as H
    small, big = _inputs(SMALL, 400), _inputs(LARGE, 401)
    g, y = (torch.from_numpy(a).cuda() for a in small[:2])
    dz, s = torch.empty_like(g), torch.empty(SMALL[1], device="cuda")
    gb, yb = (torch.from_numpy(a).cuda() for a in big[:2])
    with H.MMult(0, "auto") as own:
        own.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
        torch.cuda.synchronize()
        side = _side_stream(torch)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                own.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
        torch.cuda.current_stream().wait_stream(side)
        dzb, sb = own.relu_grad_colsum(gb, yb)                     # grows the workspace
        torch.cuda.synchronize()
        assert ref.same_bits(dzb.cpu().numpy(), big[3]) and ref.same_bits(sb.cpu().numpy(), big[4])
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == 1          # retired, not freed: seen before the graph is replayed
        for rep in range(2):
            small = _inputs(SMALL, 402 + rep)
            _put(torch, g, small[0]), _put(torch, y, small[1])
            dz.fill_(FILL), s.fill_(FILL)
            graph.replay()
            torch.cuda.synchronize()
            assert ref.same_bits(dz.cpu().numpy(), small[3]), rep
            assert ref.same_bits(s.cpu().numpy(), small[4]), rep
        # the grown workspace still serves the large shape beside the graph
        dzb, sb = own.relu_grad_colsum(gb, yb)
        torch.cuda.synchronize()
        assert ref.same_bits(sb.cpu().numpy(), big[4])
        del graph


def test_linear_backward_captured_whole_replays_the_eager_bits(amm):
    """The pass, sgemm (dx), sgemm_ex with beta = 1 (grad_w += dz.t() @ x) and the finish kernel in one graph."""
    import torch
    import how_to_optimize_gemm_amd as H
    rows, n_in, n_out = 17 * R + 77, 130, 200
    rng = np.random.default_rng(500)

    def draw():
        return (rng.standard_normal((rows, n_out)).astype(np.float32), rng.standard_normal((rows, n_in)).astype(np.float32),
                rng.standard_normal((n_out, n_in)).astype(np.float32), np.maximum(rng.standard_normal((rows, n_out)), 0).astype(np.float32),
                rng.standard_normal((n_out, n_in)).astype(np.float32), rng.standard_normal(n_out).astype(np.float32))

    first = draw()
    g, x, w, y, gw, gb = (torch.from_numpy(a).cuda() for a in first)
    side = _side_stream(torch)
    amm.reserve_stream(side.cuda_stream, rows, n_in, n_out)        # dx = dz @ w
    amm.reserve_stream(side.cuda_stream, n_out, n_in, rows)        # dw = dz.t() @ x

    def eager():
        """(dx, grad_w, grad_b) of an uncaptured call on copies of the accumulators, on the side stream."""
        with torch.cuda.stream(side):
            ew, eb = gw.clone(), gb.clone()
            dx, _, _ = amm.linear_backward(g, x, w, y, grad_w=ew, grad_b=eb)
        side.synchronize()
        return dx.cpu().numpy(), ew.cpu().numpy(), eb.cpu().numpy()

    want = eager()
    assert ref.same_bits(want[2], ref.blocked_colsum(ref.gate(first[0], first[3]), R, first[5]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            dx, dw, db = amm.linear_backward(g, x, w, y, grad_w=gw, grad_b=gb)
            text = H.last_launch()
    torch.cuda.current_stream().wait_stream(side)
    assert dw is gw and db is gb and text
    assert ref.same_bits(gw.cpu().numpy(), first[4]) and ref.same_bits(gb.cpu().numpy(), first[5])   # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    for got, w_ in zip((dx, gw, gb), want):
        assert ref.same_bits(got.cpu().numpy(), w_)
    # the inputs and the accumulators rewritten in place
    second = draw()
    for t, a in zip((g, x, w, y, gw, gb), second):
        _put(torch, t, a)
    torch.cuda.synchronize()
    want = eager()
    assert ref.same_bits(want[2], ref.blocked_colsum(ref.gate(second[0], second[3]), R, second[5]))
    graph.replay()
    torch.cuda.synchronize()
    for got, w_ in zip((dx, gw, gb), want):
        assert ref.same_bits(got.cpu().numpy(), w_)
    assert amm.streamk_timeouts() == 0
    del graph


def test_a_captured_training_step_of_autograd_linear_replays_the_eager_bits(amm):
    """torch's whole-network capture recipe on 130 -> 200 (relu) -> 72 at 2253 rows: warm-up on the side stream, the grads set
    to None, forward and backward captured; .grad of the four parameters after a replay is an eager step's, bit for bit."""
    import torch
    from how_to_optimize_gemm_amd import autograd
    torch.manual_seed(23)
    rows, n_in, hidden, n_out = 17 * R + 77, 130, 200, 72
    l1 = autograd.Linear(amm, n_in, hidden, activation="relu").cuda()
    l2 = autograd.Linear(amm, hidden, n_out).cuda()
    params = (l1.weight, l1.bias, l2.weight, l2.bias)
    x1 = torch.randn((rows, n_in), device="cuda")
    x2 = torch.randn((rows, n_in), device="cuda")
    t = torch.randn((rows, n_out), device="cuda")
    static_x = x1.clone()

    def step():
        (l2(l1(static_x)) * t).sum().backward()

    side = _side_stream(torch)
    for m, n, k in ((rows, hidden, n_in), (rows, n_out, hidden), (rows, hidden, n_out), (n_out, hidden, rows), (hidden, n_in, rows)):
        amm.reserve_stream(side.cuda_stream, m, n, k)
    want = []
    with torch.cuda.stream(side):
        for xs in (x2, x1, x2, x1):                                # warm-up; the last two are the eager references
            static_x.copy_(xs)
            for p in params:
                p.grad = None
            step()
            want.append([p.grad.clone() for p in params])
        for p in params:
            p.grad = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want_x2, want_x1 = want[2], want[3]
    assert all(torch.equal(a, b) for a, b in zip(want[0], want_x2)) and all(torch.equal(a, b) for a, b in zip(want[1], want_x1))
    assert not torch.equal(want_x1[0], want_x2[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for p, w_ in zip(params, want_x1):
        assert p.grad is not None and ref.same_bits(p.grad.cpu().numpy(), w_.cpu().numpy())
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    for p, w_ in zip(params, want_x2):
        assert ref.same_bits(p.grad.cpu().numpy(), w_.cpu().numpy())
    assert amm.streamk_timeouts() == 0
    for p in params:
        p.grad = None
    del graph
