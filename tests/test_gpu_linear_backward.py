"""MMult.linear_backward and the autograd glue on the device: db against tests/relu_grad_ref.py, dx / dw against the library's own
GEMMs on the contract's dz (bit for bit: the backward is a composition of entry points that already have their bit contract),
everything against float64 within the chains' bounds, the `need` masks, accumulation into grad_w / grad_b, and a two-layer
MLP through autograd.Linear whose gradients are the hand-written sequence's bits -- and, within a bound computed from the data,
torch's own autograd of the same function in float64."""

import numpy as np
import pytest

import relu_grad_ref as ref
from built_lib import REPO
from gpu_operands import handle_fixture

pytestmark = pytest.mark.gpu

R = ref.header_block_rows(REPO)
# (rows, in, out); the last two leave the single tile: dw = dz.t() @ x runs 65 - 71 K-slices, dx spans dozens of tiles, db goes
# through 18 and 17 row blocks (one batch of the finish kernel's 16 partial rows plus one; exactly one batch)
SHAPES = [(37, 45, 70), (129, 64, 200), (1, 5, 3), (17 * R + 77, 130, 200), (16 * R + 1, 64, 260)]


amm = handle_fixture()   # the module's own handle on MMH_KERNEL_AUTO (the session fixture's `mfma` kernel has no op forms)


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


def test_an_expanded_gradient_of_no_rows_or_no_columns_goes_through_the_backward(amm):
    """y.sum().backward() hands back an expanded gradient (strides 0, 0); with no rows, or no output features, torch calls it
    contiguous and .contiguous() returns it as it is -- the backward raised on its strides (found by the front end's fuzz).  The
    bias gradient of no rows is +0."""
    import torch
    from how_to_optimize_gemm_amd import autograd
    for rows, n_in, n_out in ((0, 5, 7), (6, 5, 0)):
        x = torch.rand((rows, n_in), device="cuda").requires_grad_()
        w = torch.rand((n_out, n_in), device="cuda").requires_grad_()
        b = torch.rand((n_out,), device="cuda").requires_grad_()
        y = autograd.linear(amm, x, w, b, "relu")
        assert y.shape == (rows, n_out)
        y.sum().backward()
        assert x.grad.shape == x.shape and w.grad.shape == w.shape and b.grad.shape == b.shape
        assert not bool(x.grad.any()) and not bool(w.grad.any())
        assert torch.equal(b.grad.view(torch.int32), torch.zeros(n_out, dtype=torch.int32, device="cuda"))


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


def test_the_autograd_glue_against_torchs_own_autograd_in_float64(amm):
    """130 -> 200 (relu) -> 72 at 300 rows, loss = (out * t).sum() with a random t: .grad of w1, b1, w2, b2 (and of x when it
    requires grad) against torch's autograd of the same function on the CPU in float64 -- the device's fp32 parameters and x,
    layer 1's gate imposed as the constant 0 / 1 mask of the device's own forward output (y1 > 0), so that nothing hinges on
    the sign of a pre-activation next to zero.  What is saved, the `need` mask, the order of the returned gradients and the
    bias flag all show here; nothing on the reference's side comes from the library.

    No fitted tolerance.  Each bound is the first-order running error of the device's chains, on the float64 magnitudes, with
    u = 2^-24 and gamma_n = n u / (1 - n u), composed through the layers:
      e_y1  = gamma(in + 1) M (|x| |w1|^T + |b1|)       the forward output feeding dw2 (M: the mask)
      e_dz1 = M gamma(out) (|t| |w2|)                    dx2 feeding dz1
      db2: gamma(R + nblocks) sum|t|                     dw2: gamma(rows) |t|^T |y1| + |t|^T e_y1
      db1: gamma(R + nblocks) sum|dz1| + sum e_dz1       dw1: gamma(rows) |dz1|^T |x| + e_dz1^T |x|
      dx:  gamma(hidden) |dz1| |w1| + e_dz1 |w1|
    No factor for second-order terms is taken (the issue allows up to 2).  Largest error / bound ratio observed on an
    MI355X: 0.0064 (dx; dw1 0.0048, db1 0.0018, dw2 0.0022, db2 0.0049) -- worst-case bounds on random data.  On the same inputs three wrong answers exceed the bound in numpy: an ungated dz (db1 and dx),
    dw1 taken from the incoming gradient instead of dz, and db1 with one row block dropped."""
    import torch
    from how_to_optimize_gemm_amd import autograd
    torch.manual_seed(29)
    rows, n_in, hidden, n_out = 300, 130, 200, 72
    l1 = autograd.Linear(amm, n_in, hidden, activation="relu").cuda()
    l2 = autograd.Linear(amm, hidden, n_out).cuda()
    names = ("w1", "b1", "w2", "b2")
    params = dict(zip(names, (l1.weight, l1.bias, l2.weight, l2.bias)))
    x = torch.randn((rows, n_in), device="cuda")
    t = torch.randn((rows, n_out), device="cuda")
    y1 = amm.linear(x, l1.weight.detach(), l1.bias.detach(), "relu")
    mask = (y1 > 0).cpu().numpy().astype(np.float64)
    assert 0.2 < mask.mean() < 0.8

    # the reference: torch's autograd on the CPU, float64
    c = {k: p.detach().cpu().double().requires_grad_(True) for k, p in params.items()}
    cx, ct, cm = x.cpu().double().requires_grad_(True), t.cpu().double(), torch.from_numpy(mask)
    h = (cx @ c["w1"].t() + c["b1"]) * cm
    ((h @ c["w2"].t() + c["b2"]) * ct).sum().backward()
    want = {k: v.grad.numpy() for k, v in c.items()}
    want["x"] = cx.grad.numpy()

    # the bounds, float64, from the data alone
    gam = ref.gamma
    X, W1, B1, W2, T = (np.abs(a.detach().cpu().numpy().astype(np.float64)) for a in (x, l1.weight, l1.bias, l2.weight, t))
    Y1 = np.abs(h.detach().numpy())
    dz1 = (ct @ c["w2"].detach()).numpy() * mask            # float64 dz1, signed
    DZ1 = np.abs(dz1)
    nblocks = (rows + R - 1) // R
    e_y1 = gam(n_in + 1) * mask * (X @ W1.T + B1)
    e_dz1 = mask * gam(n_out) * (T @ W2)
    bound = {
        "b2": gam(R + nblocks) * T.sum(axis=0),
        "w2": gam(rows) * (T.T @ Y1) + T.T @ e_y1,
        "b1": gam(R + nblocks) * DZ1.sum(axis=0) + e_dz1.sum(axis=0),
        "w1": gam(rows) * (DZ1.T @ X) + e_dz1.T @ X,
        "x": gam(hidden) * (DZ1 @ W1) + e_dz1 @ W1,
    }
    ratios = {}

    def check(tag, got):
        for k, g_ in got.items():
            assert g_ is not None, (tag, k)
            g_ = g_.cpu().numpy().astype(np.float64)
            assert g_.shape == want[k].shape, (tag, k)
            err = np.abs(g_ - want[k])
            ratios[(tag, k)] = float(np.max(err / np.maximum(bound[k], 1e-300)))
            print("autograd vs float64 [%s] %s: largest error / bound %.4f" % (tag, k, ratios[(tag, k)]))
        for (tg, k), r in ratios.items():
            assert r <= 1.0, (tg, k, r)

    (l2(l1(x)) * t).sum().backward()                     # x does not require grad: need = (False, True, True) in layer 1
    check("x constant", {k: p.grad for k, p in params.items()})
    for p in params.values():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    (l2(l1(xr)) * t).sum().backward()
    check("x requires grad", dict({k: p.grad for k, p in params.items()}, x=xr.grad))
    # no bias: the bias flag gives no gradient slot and the others are unchanged
    l3 = autograd.Linear(amm, hidden, n_out, bias=False).cuda()
    with torch.no_grad():
        l3.weight.copy_(l2.weight)
    for p in params.values():
        p.grad = None
    ((l3(l1(x)) + l2.bias.detach()) * t).sum().backward()
    check("no bias", {"w1": l1.weight.grad, "b1": l1.bias.grad, "w2": l3.weight.grad})
    assert l2.bias.grad is None and l2.weight.grad is None

    # three wrong answers, in float64 numpy, are outside the bound on these inputs
    x64, t64 = x.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    w1_64, w2_64 = (p.detach().cpu().numpy().astype(np.float64) for p in (l1.weight, l2.weight))
    dx2 = t64 @ w2_64                                       # the incoming gradient of layer 1, ungated
    assert np.allclose(dx2 * mask, dz1, rtol=1e-12, atol=0)
    outside = lambda wrong, k: float(np.mean(np.abs(wrong - want[k]) > bound[k]))
    assert outside(dx2.sum(axis=0), "b1") > 0.9 and outside(dx2 @ w1_64, "x") > 0.9            # an ungated dz
    assert outside(dx2.T @ x64, "w1") > 0.9                                                     # dw from g instead of dz
    assert outside(np.delete(dz1, np.s_[R:2 * R], axis=0).sum(axis=0), "b1") > 0.9             # one row block dropped
