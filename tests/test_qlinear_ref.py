"""tests/qlinear_ref.py against a slow per-element restatement of the int8 linear layer's contract (include/mmult_hip_q8.h):
every rule written out once more, one Python float32 operation at a time, on tiny shapes -- and the special rows."""
import numpy as np
import pytest

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
    if np.isnan(e):
        return 0
    with np.errstate(over="ignore"):
        y = f32(e) * s
    return int(min(max(np.rint(y), f32(-127.0)), f32(127.0)))   # np.rint: half to even


def slow_qlinear(x, w, bias, relu):
    sx, sw = [slow_scale(r) for r in x], [slow_scale(r) for r in w]
    y = np.zeros((len(x), len(w)), f32)
    with np.errstate(all="ignore"):
        for i in range(len(x)):
            for j in range(len(w)):
                acc = sum(slow_q(x[i][k], sx[i]) * slow_q(w[j][k], sw[j]) for k in range(x.shape[1]))
                v = f32(f32(f32(acc) * (f32(1.0) / sx[i])) * (f32(1.0) / sw[j]))
                if bias is not None:
                    v = f32(v + bias[j])
                if relu and not (v > 0 or np.isnan(v)):
                    v = f32(0.0)
                y[i, j] = v
    return y


@pytest.mark.parametrize("rows,out,in_", [(1, 1, 1), (3, 2, 5), (4, 5, 0), (5, 3, 17)])
@pytest.mark.parametrize("bias,relu", [(False, False), (True, False), (False, True), (True, True)])
def test_the_restatement_is_the_slow_loop(oracle, rows, out, in_, bias, relu):
    rng = np.random.default_rng(rows * 100 + out * 10 + in_)
    x = (rng.standard_normal((rows, in_)) * 3).astype(f32)
    w = rng.uniform(-0.5, 0.5, (out, in_)).astype(f32)
    b = rng.uniform(-2, 2, out).astype(f32) if bias else None
    if bias:
        b[0] = f32(-0.0)
    got, want = R.qlinear_ref(x, w, b, relu), slow_qlinear(x, w, b, relu)
    assert same_bits(got, want), first_difference(got, want)


def test_special_rows_follow_the_quantisers_rules(oracle):
    rng = np.random.default_rng(7)
    rows = R.special_rows(9, rng)
    x = np.stack([r for _, r, _, _ in rows])
    q, s, r = R.quantize_rows_ref(x)
    for i, (name, row, scale, check) in enumerate(rows):
        assert s[i] == scale, (name, s[i], scale)
        assert s[i] == slow_scale(row) and list(q[i]) == [slow_q(e, s[i]) for e in row], name
        assert check(q[i]), (name, q[i])
        assert q[i].min() >= -127, name
    by = {name: i for i, (name, *_) in enumerate(rows)}
    assert s[by["all zero"]] == 1 and r[by["all zero"]] == 1
    tiny = by["max 1e-38"]
    assert s[tiny] == R.F32_MAX and 0 < r[tiny] < np.finfo(f32).tiny, "the clamped scale's reciprocal is subnormal, and kept"
    assert r[tiny] == f32(2.0) ** -128
    # the same rows as weight channels, through the whole layer
    w = rng.uniform(-1, 1, (4, 9)).astype(f32)
    for a, b in ((x, w), (w, x)):
        got, want = R.qlinear_ref(a, b, None, True), slow_qlinear(a, b, None, True)
        assert same_bits(got, want), first_difference(got, want)


def test_large_sums_round_to_nearest_even(oracle):
    """Every |element| is its row's maximum: every q is +-127 and |acc| = 127^2 k passes 2^24 -- float32(acc) rounds."""
    k = 2048
    x, w = np.full((2, k), 1.5, f32), np.full((2, k), -0.25, f32)
    x[1, ::2] = -1.5   # (row 1: the sum cancels to 0)
    qx, _, rx = R.quantize_rows_ref(x)
    qw, _, rw = R.quantize_rows_ref(w)
    acc = R.int_sums(qx, qw)
    assert acc[0, 0] == -127 * 127 * k and abs(int(acc[0, 0])) > 1 << 24 and acc[1, 0] == 0
    odd = np.array([[(1 << 24) + 1, (1 << 24) + 3, -(1 << 25) - 2]], np.int32)   # ties: to even
    y = R.epilogue_ref(odd, np.ones(1, f32), np.ones(3, f32))
    assert list(y[0]) == [f32(1 << 24), f32((1 << 24) + 4), f32(-(1 << 25))]


def test_the_plan_restatement_knows_the_tile_rule():
    assert R.plan_text(128, 128, 64)[0].endswith("qlinear_s8_kernel<128,128,4,false,false,false>, 1 workgroups")
    assert "qlinear_s8_kernel<256,256,8,false,true,true>, 256 workgroups" in R.plan_text(4096, 4096, 4096, bias=True, relu=True)[0]
    assert "qlinear_s8_kernel<128,128,4,true," in R.plan_text(2048, 2048, 192, ldy=2049)[0]
    assert not R.big_tile(2048, 2048, 256) and R.big_tile(2560, 3328, 256)
