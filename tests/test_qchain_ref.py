"""tests/qchain_ref.py against a slow per-element restatement of the int8-to-int8 layer's contract (include/mmult_hip_q8o.h):
the requantisation one Python operation at a time -- ties at both parities, the clamp at +-127.5 and beyond, NaN, +-inf, -0 --
and the chain of layers on tiny shapes."""
import numpy as np
import pytest

import qchain_ref as Q
import qlinear_ref as R
from bitcmp import first_difference, same_bits

f32 = np.float32


def slow_scale(v):
    amax = f32(0.0)
    for e in v:
        a = abs(f32(e))
        if np.isfinite(a) and a > amax:
            amax = a
    if not amax > 0:
        return f32(1.0)
    with np.errstate(over="ignore"):
        s = f32(127.0) / amax
    return s if s <= R.F32_MAX else R.F32_MAX


def slow_q(e, s):
    """The row quantiser's element rule."""
    if np.isnan(e):
        return 0
    with np.errstate(over="ignore"):
        y = f32(e) * s
    return int(min(max(np.rint(y), f32(-127.0)), f32(127.0)))


def slow_requant(v, s):
    """quantize_one, spelled differently from requant_ref: Python's round() (half to even on the exact double of the float32
    product) and integer clamps."""
    if np.isnan(v):
        return 0
    with np.errstate(all="ignore"):
        t = f32(v) * f32(s)
    if np.isinf(t):
        return 127 if t > 0 else -127
    return max(-127, min(127, round(float(t))))


SPECIAL = [0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5, -126.5, 127.5, -127.5, 127.49, 128.0, -128.0, 1e6, -1e6, 3e38, -3e38,
           np.nan, np.inf, -np.inf, -0.0, 0.0, 0.49999997, 1e-40, -1e-40]


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0, 3.0, 0.1])
def test_requant_ref_is_the_slow_rule_on_the_special_values(scale):
    y = np.array([SPECIAL, SPECIAL[::-1]], f32)
    so = np.array([scale, scale], f32)
    got = Q.requant_ref(y, so)
    want = np.array([[slow_requant(v, scale) for v in row] for row in y], np.int64)
    assert got.dtype == np.int8 and np.array_equal(got, want), (got, want)
    assert got.min() >= -127
    if scale == 1.0:
        by = dict(zip(SPECIAL[:23], got[0][:23]))
        assert [by[v] for v in (0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5)] == [0, 2, 2, 4, 0, -2, -2]       # ties: to even, both parities
        assert [by[v] for v in (126.5, -126.5, 127.5, -127.5, 128.0, -128.0, 1e6, -1e6)] == [126, -126, 127, -127, 127, -127, 127, -127]
        assert got[0][18] == 0 and got[0][19] == 127 and got[0][20] == -127 and got[0][21] == 0         # NaN, +inf, -inf, -0


def test_requant_ref_scales_each_row_with_its_own_scale():
    rng = np.random.default_rng(3)
    y = (rng.standard_normal((7, 33)) * 40).astype(f32)
    so = rng.uniform(0.2, 4, 7).astype(f32)
    got = Q.requant_ref(y, so)
    want = np.array([[slow_requant(v, so[i]) for v in y[i]] for i in range(7)])
    assert np.array_equal(got, want)
    assert (np.abs(got) == 127).any() and (np.abs(got) < 127).any()


def test_requant_ref_at_the_edges_of_the_scale():
    """What quantize_one gives where the header's "so must be finite" still holds but the product is not a number of the
    range -- written down value by value, so that the reference's own edge behaviour can be reviewed: rintf keeps a NaN, fmaxf
    and fminf return their other argument for one, so a NaN PRODUCT (inf * 0) leaves the lower bound, -127; a NaN y is 0."""
    inf, nan, fmax = np.inf, np.nan, R.F32_MAX
    y = np.array([inf, -inf, nan, 0.0, -0.0, 1.5, -2.5, 1e-38, -1e-38, 3e38], f32)
    table = [
        (0.0,         [-127, -127, 0, 0, 0, 0, 0, 0, 0, 0]),                 # inf * 0 is NaN: -127; finite * 0: 0
        (-0.0,        [-127, -127, 0, 0, 0, 0, 0, 0, 0, 0]),
        (fmax,        [127, -127, 0, 0, 0, 127, -127, 3, -3, 127]),          # overflow to +-inf clamps; 1e-38 * FLT_MAX = 3.4
        (-fmax,       [-127, 127, 0, 0, 0, -127, 127, -3, 3, -127]),
        (-1.0,        [-127, 127, 0, 0, 0, -2, 2, 0, 0, -127]),              # a negative scale mirrors: ties still go to even
        (-0.5,        [-127, 127, 0, 0, 0, -1, 1, 0, 0, -127]),              # -0.75 -> -1, 1.25 -> 1
        (2.0 ** -140, [127, -127, 0, 0, 0, 0, 0, 0, 0, 0]),                  # a denormal scale: inf stays inf, the rest underflows
        (1e30,        [127, -127, 0, 0, 0, 127, -127, 0, 0, 127]),
        (1e-30,       [127, -127, 0, 0, 0, 0, 0, 0, 0, 127]),               # 3e38 * 1e-30 = 3e8
    ]
    for scale, want in table:
        got = Q.requant_ref(y[None, :], np.array([scale], f32))[0]
        assert list(got) == want, (scale, list(got), want)
        # the per-element rule agrees wherever the product is not NaN (it has no fmaxf to ask)
        with np.errstate(all="ignore"):
            number = ~np.isnan(y * f32(scale)) | np.isnan(y)
        assert [slow_requant(v, scale) for v in y[number]] == list(got[number]), scale
    # a scale that is not finite is outside the contract; requant_ref is not asked about it


def test_the_scale_rule_is_the_quantisers():
    for v in ([0.0], [1e-38], [2.5, -7.0], [np.inf, 3.0], [np.nan, 0.25]):
        a = np.abs(np.array(v, f32))
        amax = np.where(np.isfinite(a), a, 0).max()
        assert Q.scale_of_amax(amax) == slow_scale(np.array(v, f32)), v


def slow_chain(x, layers, out_scales, relu, last_relu):
    """The chain, element by element: the row quantiser, then per hidden layer the integer sums of the previous layer's bytes,
    the three float32 roundings, the requantisation; the reciprocal of the output scale as the next row factor."""
    rows = len(x)
    sx = [slow_scale(r) for r in x]
    q = [[slow_q(e, sx[i]) for e in x[i]] for i in range(rows)]
    with np.errstate(all="ignore"):
        rx = [f32(1.0) / s for s in sx]
        for li, (w, b) in enumerate(layers):
            last = li == len(layers) - 1
            sw = [slow_scale(r) for r in w]
            qw = [[slow_q(e, sw[j]) for e in w[j]] for j in range(len(w))]
            nxt = [[None] * len(w) for _ in range(rows)]
            for i in range(rows):
                for j in range(len(w)):
                    acc = sum(a * c for a, c in zip(q[i], qw[j]))
                    v = f32(f32(f32(acc) * rx[i]) * (f32(1.0) / sw[j]))
                    if b is not None:
                        v = f32(v + b[j])
                    if (last_relu if last else relu) and not (v > 0 or np.isnan(v)):
                        v = f32(0.0)
                    nxt[i][j] = v if last else slow_requant(v, out_scales[li])
            if last:
                return np.array(nxt, f32)
            q, rx = nxt, [f32(1.0) / f32(out_scales[li])] * rows


@pytest.mark.parametrize("dims", [(3, 5, 4, 2), (2, 7, 2, 3), (4, 0, 3, 2), (1, 6, 5, 5, 2)])
@pytest.mark.parametrize("bias,relu", [(False, False), (True, True)])
def test_chain_ref_is_the_slow_loop(oracle, dims, bias, relu):
    rng = np.random.default_rng(sum(dims))
    rows, widths = dims[0], dims[1:]
    x = (rng.standard_normal((rows, widths[0])) * 2).astype(f32)
    layers = [(rng.uniform(-1, 1, (o, i)).astype(f32), rng.uniform(-1, 1, o).astype(f32) if bias else None)
              for i, o in zip(widths, widths[1:])]
    scales = [f32(s) for s in rng.uniform(10, 60, len(layers) - 1)]
    got, hidden = Q.chain_ref(x, layers, scales, relu, False)
    want = slow_chain(x, layers, scales, relu, False)
    assert same_bits(got, want), first_difference(got, want)
    assert len(hidden) == len(layers) - 1 and all(h.dtype == np.int8 for h in hidden)


def test_a_layer_on_quantised_rows_is_the_layer_on_the_float_rows(oracle):
    """qlinear_s8_ref on quantize_rows_ref's outputs is qlinear_ref."""
    rng = np.random.default_rng(8)
    x, w = rng.standard_normal((4, 9)).astype(f32), rng.uniform(-1, 1, (3, 9)).astype(f32)
    b = rng.uniform(-1, 1, 3).astype(f32)
    xq, _, rx = R.quantize_rows_ref(x)
    assert same_bits(Q.qlinear_s8_ref(xq, rx, w, b, True), R.qlinear_ref(x, w, b, True))
    assert same_bits(Q.qlinear_s8_ref(xq, rx, w, b, True), slow_chain(x, [(w, b)], [], False, True))


def test_calibration_takes_the_largest_finite_hidden_value(oracle):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 6)).astype(f32)
    layers = [(rng.uniform(-1, 1, (4, 6)).astype(f32), None), (rng.uniform(-1, 1, (3, 4)).astype(f32), None)]
    s, = Q.calibrate_ref(x, layers)
    h = R.qlinear_ref(x, layers[0][0], None, True)
    assert s == f32(127.0) / h.max() and not (np.abs(Q.requant_ref(h, np.full(5, s, f32))) > 127).any()
    assert (Q.requant_ref(h, np.full(5, s, f32)) == 127).sum() >= 1   # the maximum itself lands on 127: nothing clamps


def test_the_plan_restatement_knows_the_guard_rule():
    assert Q.plan_text_s8o(128, 128) == "qlinear_s8o_kernel<128,128,4,false>, 1 workgroups"
    assert Q.plan_text_s8o(128, 128, ldyq=130) == "qlinear_s8o_kernel<128,128,4,true>, 1 workgroups"     # a pitch of 2 mod 4: bytes
    assert Q.plan_text_s8o(128, 128, yq_mod4=1) == "qlinear_s8o_kernel<128,128,4,true>, 1 workgroups"
    assert Q.plan_text_s8o(129, 130) == "qlinear_s8o_kernel<128,128,4,true>, 4 workgroups"
    assert Q.plan_text_s8o(4096, 11008) == "qlinear_s8o_kernel<256,256,8,false>, 688 workgroups"
    assert Q.plan_text_s8o(4093, 11003) == "qlinear_s8o_kernel<256,256,8,true>, 688 workgroups"
