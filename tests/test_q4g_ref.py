"""CPU tests of tests/q4g_ref.py, the numpy restatement of include/mmult_hip_q4g.h's contract: the group sums convert exactly at
their bound, the reference tells each plausible WRONG kernel from the right one in at least one bit, and per-group scales do what
they are for -- a strictly smaller error than per-channel scales on a weight with one outlier per row."""
import numpy as np

import q4_ref as F
import q4g_ref as G
import qlinear_ref as R
from bitcmp import same_bits


def test_the_group_sum_converts_exactly_at_its_bound():
    """|S_g| <= 128 * 128 * 8 = 2^17, reached by x = -128 against W = -8; the negative extreme is 127 * 128 * -8 ... both far
    below 2^24, and the kernel's accumulator, 16 x that, is at most 2^21."""
    assert G.S_BOUND == 1 << 17 and 16 * G.S_BOUND == 1 << 21 < 1 << 31
    xq = np.full((2, 256), -128, np.int8)
    xq[1] = 127
    W = np.full((256, 3), -8, np.int8)
    W[:, 1] = 7
    S = G.group_sums(xq, W)
    assert S.dtype == np.float32 and S.shape == (2, 2, 3)
    assert S[0, 0, 0] == 1 << 17 and S[1, 0, 1] == -128 * 128 * 7 and S[0, 1, 0] == -127 * 128 * 8
    odd = np.float32(G.S_BOUND - 1)
    assert int(odd) == G.S_BOUND - 1   # every integer up to the bound is a float32


def case(seed=5, rows=4, out=24, in_=1100, splits=2):
    rng = np.random.default_rng(seed)
    xq = rng.integers(-128, 128, (rows, in_), dtype=np.int8)
    W = rng.integers(-8, 8, (in_, out), dtype=np.int8)
    r = G.spread_factors(rng, G.groups(in_), out)
    rx = rng.uniform(0.01, 0.05, rows).astype(np.float32)
    bias = rng.uniform(-4, 4, out).astype(np.float32)
    k_len = G.plan(rows, out, in_, splits=splits)[3]
    return xq, W, r, rx, bias, k_len


def chain(terms):
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc


def pairwise(terms):
    terms = list(terms)
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


def test_the_reference_tells_every_wrong_kernel_from_the_right_one():
    """Nine groups in two ranges of five and four (a pairwise sum of three terms IS the chain), factors spread over
    2^-12 .. 2^13.  Each mutant is a kernel somebody could write; each differs from want() in at least one bit of the fp32
    output."""
    xq, W, r, rx, bias, k_len = case()
    rows, in_ = xq.shape
    out, splits = W.shape[1], 2
    assert G.groups(in_) == 9 >= 5 and k_len == 640
    P = F.pack_ref(W)
    right = G.want(xq, rx, P, in_, r, bias, False, splits, k_len)
    assert same_bits(right, G.want(xq, rx, P, in_, np.pad(r, ((0, 0), (0, 7)), constant_values=np.nan), bias, False, splits, k_len))
    S = G.group_sums(xq, W)
    t = [S[g] * r[g][None, :] for g in range(9)]                       # float32 terms, one rounding each
    ranges = G.range_groups(in_, splits, k_len)
    assert ranges == [(0, 5), (5, 9)]
    f32, f64 = np.float32, np.float64

    def fin(Z):
        return G.finish(Z.astype(f32), rx, bias)

    mutants = {
        "descending group order": fin(chain([chain(t[a:b][::-1]) for a, b in ranges])),
        "pairwise order": fin(chain([pairwise(t[a:b]) for a, b in ranges])),
        "one chain across the range boundary": fin(chain(t)),
        "a float64 accumulator rounded once per range": fin(chain([sum(S[g].astype(f64) * r[g].astype(f64)[None, :] for g in range(a, b)).astype(f32)
                                                                  for a, b in ranges])),
        "rx applied per group": (lambda Z: Z + bias[None, :])(chain([chain([tg * rx[:, None] for tg in t[a:b]]) for a, b in ranges])),
    }
    # an fma chain, emulated in float64: the product of a 18-bit and a 24-bit number is exact there, the sum rounds once to
    # float64 and once more to float32 -- as close to a fused multiply-add as numpy gets
    parts = []
    for a, b in ranges:
        acc = np.zeros((rows, out), f32)
        for g in range(a, b):
            acc = (S[g].astype(f64) * r[g].astype(f64)[None, :] + acc.astype(f64)).astype(f32)
        parts.append(acc)
    mutants["an fma chain"] = fin(chain(parts))
    # the int8 layer's finish kernel on this workspace: it adds the partials as INTEGERS and has three roundings,
    # (float)acc * rx * rw.  With rw = 1 the third is exact, so what is left of the mutant is its integer accumulator.
    with np.errstate(all="ignore"):
        acc = sum(np.rint(p).astype(np.int64) for p in G.partials(xq, P, in_, r, splits, k_len))
    mutants["the three-rounding int8 epilogue with rw = 1"] = R.epilogue_ref(acc, rx, np.ones(out, f32), bias, False)
    for name, got in mutants.items():
        assert got.dtype == f32 and got.shape == right.shape, name
        assert not same_bits(got, right), name + ": the reference cannot tell this kernel from the right one"
    # ... and the partition is part of the contract: the same operands under another one give other bits
    assert not same_bits(G.want(xq, rx, P, in_, r, bias, False, 3, 384), right)
    # the int8 output follows the fp32 one
    so = np.full(rows, 3.0, f32)
    import qchain_ref as Q
    assert np.array_equal(G.want(xq, rx, P, in_, r, bias, True, splits, k_len, so),
                          Q.requant_ref(G.want(xq, rx, P, in_, r, bias, True, splits, k_len), so))


def test_an_empty_layer_is_the_bias():
    y = G.want(np.zeros((2, 0), np.int8), np.ones(2, np.float32), np.zeros((0, 3), np.uint8), 0, np.zeros((0, 3), np.float32),
               np.arange(3, dtype=np.float32), False, 0, 0)
    assert y.tolist() == [[0, 1, 2]] * 2
    assert G.plan(2, 3, 0)[1:] == (0, 0, 0) and "alone" in G.plan(2, 3, 0)[0]


def test_special_factors_follow_the_rule_literally():
    """A real group whose factor is 0, negative, subnormal, inf or NaN: t = f32(S) * r as numpy computes it (0 * inf = NaN)."""
    xq = np.ones((1, 256), np.int8)
    W = np.ones((256, 6), np.int8)
    W[:128, 4] = 0                                  # S_0 = 0 in column 4: 0 * inf
    r = np.ones((2, 6), np.float32)
    r[0] = [0.0, -2.0, 1e-40, np.inf, np.inf, np.nan]
    y = G.want(xq, np.ones(1, np.float32), F.pack_ref(W), 256, r, None, False, 1, 256)[0]
    assert y[0] == 128 and y[1] == -128 and y[2] == np.float32(128) + np.float32(128) * np.float32(1e-40) and np.isinf(y[3])
    assert np.isnan(y[4]) and np.isnan(y[5])


def rel_error(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want.astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))


def test_group_scales_beat_channel_scales_on_a_weight_with_outliers():
    """One element per row 20 times its Gaussian value: the channel's scale is the outlier's, and the other 1023 elements round to
    a handful of levels; only the outlier's own group pays with group scales.  Both errors come from the two references -- a fact
    about the rules, not a tolerance."""
    rng = np.random.default_rng(3)
    plain, spiked = G.outlier_weight(rng, 64, 1024)
    x = rng.standard_normal((16, 1024))
    errors = {}
    for name, w in (("gaussian", plain), ("outlier", spiked)):
        q, _, inv = F.quantize4_ref(w)
        channel = q.astype(np.float32) * inv[:, None]
        qg, _, r = G.quantize4g_ref(w)
        group = G.dequantize_ref(qg, r)
        errors[name] = (rel_error(channel, w), rel_error(group, w), rel_error(x @ channel.T.astype(np.float64), x @ w.T.astype(np.float64)),
                        rel_error(x @ group.T.astype(np.float64), x @ w.T.astype(np.float64)))
    cw, gw, cy, gy = errors["outlier"]
    assert gw < cw and gy < cy, errors
    assert errors["gaussian"][1] < errors["gaussian"][0]    # (a group's maximum is never above its channel's)


def test_the_group_quantiser_is_the_channel_quantiser_per_group():
    rng = np.random.default_rng(8)
    w = F.special_weight(6, 300, rng)
    q, s, r = G.quantize4g_ref(w)
    assert q.shape == (6, 300) and s.shape == r.shape == (3, 6) and int(q.min()) == -7 and int(q.max()) == 7
    for g in range(3):
        qq, ss, rr = F.quantize4_ref(w[:, 128 * g:128 * g + 128])
        assert np.array_equal(q[:, 128 * g:128 * g + 128], qq) and same_bits(s[g], ss) and same_bits(r[g], rr)
    assert s[1, 0] == 1.0 and s[0, 3] == np.finfo(np.float32).max and s[1, 3] == 1.0   # a zero group; an overflowing one
    assert G.layout(130, 257) == (144, 192, 3, 144, 144 * 192, 3 * 144 * 4) and G.layout(5, 0) == (16, 0, 0, 16, 0, 0)
