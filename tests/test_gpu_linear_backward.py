"""MMult.linear_backward and the autograd glue on the device: db against tests/relu_grad_ref.py, dx / dw against the library's own
GEMMs on the contract's dz (bit for bit: the backward is a composition of entry points that already have their bit contract),
everything against float64 within the chains' bounds, the `need` masks, accumulation into grad_w / grad_b, and a two-layer
MLP through autograd.Linear whose gradients are the hand-written sequence's bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relu_grad_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.header_block_rows(REPO)
SHAPES = [(37, 45, 70), (129, 64, 200), (1, 5, 3)]   # (rows, in, out)


@pytest.fixture(scope="module")
def amm():
    """The module's own handle on MMH_KERNEL_AUTO (the session fixture's `mfma` kernel has no transposed-operand forms)."""
    import how_to_optimize_gemm_amd as H
    h = H.MMult(0, "auto")
    yield h
    h.close()


_CASES = {}


def _case(shape, relu):
    """x, w, the incoming gradient, the forward output (ReLU only) and the contract's dz / db, computed once."""
    key = (shape, relu)
    if key not in _CASES:
        rows, n_in, n_out = shape
        rng = np.random.default_rng(rows * 131 + n_out)
        x = rng.standard_normal((rows, n_in)).astype(np.float32)
        w = rng.standard_normal((n_out, n_in)).astype(np.float32)
        g = rng.standard_normal((rows, n_out)).astype(np.float32)
        # the forward output as the gate sees it: any fp32 matrix with zeros and negatives serves (relu's image: >= 0)
        y = np.maximum(rng.standard_normal((rows, n_out)), 0).astype(np.float32) if relu else None
        dz, db = ref.relu_grad_colsum(g, y, R)
        _CASES[key] = dict(x=x, w=w, g=g, y=y, dz=dz, db=db)
        for v in _CASES[key].values():
            if v is not None:
                v.setflags(write=False)
    return _CASES[key]


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_backward_is_the_composition_bit_for_bit_and_within_the_chain_bounds(amm, shape, relu):
    import torch
    import how_to_optimize_gemm_amd as H
    rows, n_in, n_out = shape
    c = _case(shape, relu)
    x, w, g, y, dz = (_dev(torch, c[k]) for k in ("x", "w", "g", "y", "dz"))
    dx, dw, db = amm.linear_backward(g, x, w, y)
    assert dx.shape == (rows, n_in) and dw.shape == (n_out, n_in) and db.shape == (n_out,)
    # db: the contract
    assert ref.same_bits(db.cpu().numpy(), c["db"])
    # dx: the NN GEMM on the contract's dz; dw: the TN GEMM
    want_dx = amm.matmul(dz, w)
    want_dw = torch.empty((n_out, n_in), device="cuda")
    amm.sgemm_op(H.OP_T, H.OP_N, n_out, n_in, rows, dz.data_ptr(), n_out, x.data_ptr(), n_in, want_dw.data_ptr(), n_in)
    assert ref.same_bits(dx.cpu().numpy(), want_dx.cpu().numpy())
    assert ref.same_bits(dw.cpu().numpy(), want_dw.cpu().numpy())
    # against float64, the fp32 inputs taken as exact: one fma chain per element
    dz64, w64, x64 = c["dz"].astype(np.float64), c["w"].astype(np.float64), c["x"].astype(np.float64)
    assert np.all(np.abs(dx.cpu().numpy() - dz64 @ w64) <= ref.gamma(n_out) * (np.abs(dz64) @ np.abs(w64)))
    assert np.all(np.abs(dw.cpu().numpy() - dz64.T @ x64) <= ref.gamma(rows) * (np.abs(dz64).T @ np.abs(x64)))
    nblocks = (rows + R - 1) // R
    assert np.all(np.abs(db.cpu().numpy() - dz64.sum(axis=0)) <= ref.gamma(R + nblocks) * np.abs(dz64).sum(axis=0))
    # accumulation: fl(grad_w + s) with s the whole chain (sgemm_ex, beta = 1), fl(grad_b + colsum); in place
    rng = np.random.default_rng(7)
    gw0 = rng.standard_normal((n_out, n_in)).astype(np.float32)
    gb0 = rng.standard_normal(n_out).astype(np.float32)
    gw, gb = _dev(torch, gw0), _dev(torch, gb0)
    dx2, dw2, db2 = amm.linear_backward(g, x, w, y, grad_w=gw, grad_b=gb)
    assert dw2 is gw and db2 is gb
    want_gw = _dev(torch, gw0)
    amm.sgemm_ex(H.OP_T, H.OP_N, n_out, n_in, rows, 1.0, dz.data_ptr(), n_out, x.data_ptr(), n_in, 1.0, want_gw.data_ptr(), n_in)
    assert ref.same_bits(gw.cpu().numpy(), want_gw.cpu().numpy())
    assert ref.same_bits(gw.cpu().numpy(), gw0 + want_dw.cpu().numpy())          # torch's `+=` on the finished chain
    assert ref.same_bits(gb.cpu().numpy(), ref.blocked_colsum(c["dz"], R, gb0))
    assert ref.same_bits(dx2.cpu().numpy(), want_dx.cpu().numpy())
    # the inputs are untouched
    for t, k in ((x, "x"), (w, "w"), (g, "g")) + (((y, "y"),) if relu else ()):
        assert ref.same_bits(t.cpu().numpy(), c[k]), k


def test_need_masks_skip_outputs_and_launches(amm):
    import torch
    import how_to_optimize_gemm_amd as H
    shape = SHAPES[1]
    rows, n_in, n_out = shape
    c = _case(shape, True)
    x, w, g, y = (_dev(torch, c[k]) for k in ("x", "w", "g", "y"))
    full = amm.linear_backward(g, x, w, y)
    # nothing needed: nothing launched (the last launch is still the matmul's)
    amm.matmul(x, w.t())
    before = H.last_launch()
    assert "relu_grad" not in before
    assert amm.linear_backward(g, x, w, y, need=(False, False, False)) == (None, None, None)
    assert H.last_launch() == before
    # the bias gradient alone: one pass that sums and writes no dz
    dx, dw, db = amm.linear_backward(g, x, w, y, need=(False, False, True))
    assert dx is None and dw is None and ref.same_bits(db.cpu().numpy(), c["db"])
    text = H.last_launch()
    assert text.startswith("relu_grad_colsum_kernel") and "gate on" in text and "dz not written" in text and f"colsum {(rows + R - 1) // R} blocks" in text
    # without an activation and without the bias gradient there is no pass at all: dz IS the incoming gradient
    amm.relu_grad_colsum(g, y)
    dx, dw, db = amm.linear_backward(g, x, w, None, need=(True, False, False))
    assert dw is None and db is None and "relu_grad" not in H.last_launch()
    assert ref.same_bits(dx.cpu().numpy(), amm.matmul(g, w).cpu().numpy())
    # ... with the bias gradient: a pass that only sums
    dx, dw, db = amm.linear_backward(g, x, w, None, need=(False, False, True))
    text = H.last_launch()
    assert "gate off" in text and "dz not written" in text
    assert ref.same_bits(db.cpu().numpy(), ref.blocked_colsum(c["g"], R))
    # single outputs are the full call's bits
    for i in range(3):
        need = tuple(j == i for j in range(3))
        got = amm.linear_backward(g, x, w, y, need=need)
        assert [o is not None for o in got] == list(need)
        assert ref.same_bits(got[i].cpu().numpy(), full[i].cpu().numpy())
    # dx only, gated: the pass writes dz and sums nothing
    amm.linear_backward(g, x, w, y, need=(False, False, True))
    dx, _, _ = amm.linear_backward(g, x, w, y, need=(True, False, False))
    assert ref.same_bits(dx.cpu().numpy(), full[0].cpu().numpy())


def test_a_kernel_without_op_forms_refuses_before_anything_is_launched():
    import torch
    import how_to_optimize_gemm_amd as H
    c = _case(SHAPES[0], True)
    x, w, g, y = (_dev(torch, c[k]) for k in ("x", "w", "g", "y"))
    with H.MMult(0, "mfma") as mfma:
        gb = torch.full((SHAPES[0][2],), 9.0, device="cuda")
        mfma.matmul(x, w.t().contiguous())
        before = H.last_launch()
        with pytest.raises(H.MMultError) as e:
            mfma.linear_backward(g, x, w, y, grad_b=gb)
        assert e.value.status == H.ERR_UNSUPPORTED
        assert H.last_launch() == before and torch.all(gb == 9.0).item()
        # what needs no transposed operand still runs on that handle
        dx, dw, db = mfma.linear_backward(g, x, w, y, need=(True, False, True))
        assert dw is None and ref.same_bits(db.cpu().numpy(), c["db"])
    with pytest.raises(H.MMultError):
        with H.MMult(0, "auto") as a:
            a.linear_backward(g, x, w[:, :-1], y)


def test_mm_linear_itself_stays_outside_autograd(amm):
    import torch
    x = torch.randn((9, 6), device="cuda", requires_grad=True)
    w = torch.randn((4, 6), device="cuda", requires_grad=True)
    y = amm.linear(x, w, None, "relu")
    assert y.grad_fn is None and not y.requires_grad


def test_a_two_layer_mlp_through_autograd_is_the_hand_written_sequence(amm):
    import torch
    from how_to_optimize_gemm_amd import autograd
    torch.manual_seed(11)
    rows, n_in, hidden, n_out = 129, 45, 200, 70
    l1 = autograd.Linear(amm, n_in, hidden, activation="relu").cuda()
    l2 = autograd.Linear(amm, hidden, n_out).cuda()
    x = torch.randn((rows, n_in), device="cuda")
    out = l2(l1(x))
    assert out.grad_fn is not None
    out.sum().backward()                                  # an EXPANDED incoming gradient: every stride 0
    # by hand, in order
    w1, b1, w2, b2 = (p.detach() for p in (l1.weight, l1.bias, l2.weight, l2.bias))
    y1 = amm.linear(x, w1, b1, "relu")
    y2 = amm.linear(y1, w2, b2)
    assert torch.equal(out.detach(), y2)
    g2 = torch.ones((rows, n_out), device="cuda")
    dx2, dw2, db2 = amm.linear_backward(g2, y1, w2, None)
    dx1, dw1, db1 = amm.linear_backward(dx2, x, w1, y1, need=(False, True, True))
    assert dx1 is None
    first = {}
    for name, p, want in (("w1", l1.weight, dw1), ("b1", l1.bias, db1), ("w2", l2.weight, dw2), ("b2", l2.bias, db2)):
        assert ref.same_bits(p.grad.cpu().numpy(), want.cpu().numpy()), name
        first[name] = p.grad.cpu().numpy().copy()
    assert np.count_nonzero(first["w1"]) > 0 and np.count_nonzero(first["b1"]) > 0
    # a second backward accumulates into .grad
    l2(l1(x)).sum().backward()
    for name, p in (("w1", l1.weight), ("b1", l1.bias), ("w2", l2.weight), ("b2", l2.bias)):
        assert ref.same_bits(p.grad.cpu().numpy(), first[name] + first[name]), name
    # an input that requires grad gets dx; a non-contiguous incoming gradient is made contiguous
    xr = x.clone().requires_grad_(True)
    h = autograd.linear(amm, xr, w1, b1, "relu")
    h.backward(dx2.t().contiguous().t())
    want_dx, _, _ = amm.linear_backward(dx2, x, w1, y1, need=(True, False, False))
    assert ref.same_bits(xr.grad.cpu().numpy(), want_dx.cpu().numpy())
    # the backward runs outside autograd: differentiating it a second time raises instead of returning a graph-less result
    xr2 = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(autograd.linear(amm, xr2, w1, b1, "relu").sum(), xr2, create_graph=True)
    assert ref.same_bits(gx.detach().cpu().numpy(), amm.linear_backward(torch.ones_like(y1), x, w1, y1, need=(True, False, False))[0].cpu().numpy())
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # no bias, no activation
    l3 = autograd.Linear(amm, n_in, 8, bias=False).cuda()
    l3(x).sum().backward()
    _, dw3, db3 = amm.linear_backward(torch.ones((rows, 8), device="cuda"), x, l3.weight.detach(), None, need=(False, True, False))
    assert db3 is None and ref.same_bits(l3.weight.grad.cpu().numpy(), dw3.cpu().numpy())
