"""The seeded case list of the int8 layers' fuzz (tests/q8_fuzz.py: cases(64, 2026, cus), run by tests/test_gpu_q8_fuzz.py) is
what it promises, checked on the CPU at 256 (the MI355X), 304 and 64 compute units: deterministic; every kernel instantiation and
launch form of the three libraries is reached -- judged by the libraries' own plan functions on the layouts run_case() uses, which
run_case() holds the device's last_launch texts to --; the Python restatements of the plans agree with the libraries on every
call; the list is not vacuous (few refusals, saturated and unsaturated int8 outputs, every special value visible in the
expectation where it was planted); and the oracle tells wrong kernels apart: for each mutant of the reference below at least one
case's expectation differs from the true one.

Cases of the 64 whose expectation differs, per mutant, at 256 / 304 / 64 compute units (printed by the mutant test):
    drop the last byte of k                                    57 / 57 / 57
    add the bias before multiplying by rw                      26 / 26 / 26
    ReLU sends NaN to 0                                         3 /  3 /  3
    requant rounds half away from zero                         11 / 12 / 11
    requant clamps at -128                                     16 / 16 / 16
    decode sums only the first split                           13 / 13 / 13
    inv_scale kept as a double reciprocal of the rounded scale 58 / 58 / 58
    4-bit: clamp to -8 .. 7                                     2 /  2 /  2    (of the 22 cases of at most 16 rows, which run F7)
    4-bit: scale 8 / amax                                      20 / 20 / 20
    4-bit: round half away from zero                           20 / 20 / 20    (q8_fuzz.W4_TIES; 2 without that channel)
    4-bit: the nibble halves of a slice swapped in the image   20 / 20 / 20
    4-bit: nibbles zero-extended                               20 / 20 / 20
    4-bit: inf quantised to 0                                   2 /  2 /  2
    4-bit: abs-max over non-finite elements too                 6 /  6 /  6
F7 -- the 4-bit weight (libmmult_hip_q4d.so) on the list's decode cases -- has its own section at the end: the launch forms its
texts reach, the two weight windows and both answers of QWeight4.from_image, its expectation against tests/q4_ref.py's want.
The inv_scale mutant is read as: rx = 1 / (double)sx used unrounded in the epilogue's first product.  Rounded to float32 first, the double
reciprocal IS the float32 quotient (53 >= 2 * 24 + 2 bits: the second rounding is innocuous) -- q8._scale_vectors relies on it --
and that reading is asserted to differ nowhere."""
import types

import numpy as np
import pytest

import built_lib
import q4_ref as P4
import q8_fuzz as F
import qchain_ref as Q
import qdecode_ref as D
import qlinear_ref as R
import test_gpu_qchain as TC
import test_gpu_qlinear as T
from bitcmp import same_bits

N, SEED = 64, 2026
CU_COUNTS = (256, 304, 64)


@pytest.fixture(scope="module", params=CU_COUNTS, ids=lambda n: f"{n}cus")
def cus(request):
    return request.param


@pytest.fixture(scope="module")
def table(cus, oracle):
    """[(case, inputs, memoising rules, expectation)] of the list at a CU count, computed once (pytest runs the module's tests
    CU count by CU count, so one table is alive at a time)."""
    out = []
    for c in F.cases(N, SEED, cus):
        inp, rules = F.inputs(c), memoised()
        out.append((c, inp, rules, F.expected(c, inp, rules)))
    return out


def memoised(**swapped):
    """F.RULES whose quantiser and integer sums remember what they gave for the same arrays (a mutant of a later rule reuses
    them), with `swapped` rules in place of the true ones."""
    memo = {}

    def remember(fn):
        def call(*arrays):
            key = (fn.__name__,) + tuple(id(a) for a in arrays)
            if key not in memo:
                memo[key] = (arrays, fn(*arrays))   # (the arrays are kept: an id stays theirs)
            return memo[key][1]
        return call

    rules = types.SimpleNamespace(**vars(F.RULES))
    rules.quantize_rows_ref, rules.int_sums = remember(R.quantize_rows_ref), remember(R.int_sums)
    for name, fn in swapped.items():
        setattr(rules, name, fn)
    return rules


def mutate(rules, **swapped):
    """The case's memoising rules with some swapped (the memo is shared)."""
    m = types.SimpleNamespace(**vars(rules))
    for name, fn in swapped.items():
        setattr(m, name, fn)
    return m


def launching(c, cus, plan=F.python_plan):
    return [(k, plan(k, cus)[0]) for k in F.calls(c)]


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_the_list_is_deterministic(cus):
    a, b = F.cases(N, SEED, cus), F.cases(N, SEED, cus)
    assert a == b and len(a) == N and len(set(a)) == N
    assert F.cases(16, SEED, cus) == a[:16], "a shorter list is a prefix"
    assert F.cases(N, SEED + 1, cus) != a
    for n in (0, 7, 12, 63, -8):
        with pytest.raises(ValueError):
            F.cases(n, SEED, cus)
    for c in a[:8]:
        x, y = F.inputs(c), F.inputs(c)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x[:5], y[:5])) and x.planted == y.planted


def test_the_strata_are_what_the_module_says(cus):
    cases = F.cases(N, SEED, cus)
    by = lambda s: cases[s::F.STRATA]
    aligned = lambda c: F.layout(c).ldx % 4 == 0 and c.off_x % 4 == 0 and F.layout(c).ldy % 4 == 0 and c.off_y % 4 == 0 and \
        F.layout(c).ldyq % 4 == 0 and c.off_yq % 4 == 0 and F.layout(c).ldq % 4 == 0 and c.off_q % 4 == 0
    for s in range(F.STRATA):
        assert [(c.bias, c.relu) for c in by(s)] == F.EPILOGUES * 2, s
    assert all(c.rows % 128 == 0 and c.out % 128 == 0 and aligned(c) for c in by(0))
    assert all(aligned(c) for c in by(1) + by(4)) and not any(aligned(c) for c in by(2) + by(5))
    for s in (3, 6):
        assert sum(map(aligned, by(s))) == 4, s
        assert {(c.bias, c.relu) for c in by(s) if aligned(c)} == set(F.EPILOGUES) == {(c.bias, c.relu) for c in by(s) if not aligned(c)}
    assert sum(c.in_ == 0 for c in by(1)) >= 2 and sum(c.in_ == 0 for c in by(2)) >= 2           # once per 32 cases, each
    assert all(1 <= c.rows <= 16 for c in by(4) + by(5)) and {c.rows for c in by(4) + by(5)} == set(range(1, 17))
    refused = [c for c in by(4) + by(5) if not F.layout(c).splits_ok]
    assert len(refused) == N // 16 and all(c.in_ > 0 and c.splits > 0 and not D.valid_splits(c.in_, c.splits) for c in refused)
    assert all(sum(not F.layout(c).splits_ok for c in cases[i:i + 16]) == 1 for i in range(0, N, 16))
    assert all(c.in_ >= 1024 and c.rows < 20 and c.out < 80 for c in by(6))
    (m, n, _), _ = R.shapes_256(cus)
    assert [(c.rows, c.out) == (m, n) for c in by(7)] == [True] * 4 + [False] * 4
    assert all(R.big_tile(c.rows, c.out, cus) and 0 <= m - c.rows < 240 and 0 <= n - c.out < 240 and c.in_ < 200 for c in by(7))
    assert all(c.splits == 0 for s in (0, 1, 2, 3, 6, 7) for c in by(s))
    assert sum(not c.specials for c in cases) == N // 8 and {c.scale_factor for c in cases} == set(F.FACTORS)
    assert {(c.scale_kind, c.scale_factor) for c in cases} == {(k, f) for k in ("float", "rows") for f in F.FACTORS}


# ---- coverage, through the Python restatements (the next test holds them to the libraries) ----------------------------------------
def test_every_instantiation_and_launch_form_is_reached(cus):
    cases = F.cases(N, SEED, cus)
    texts = [(c, k, text) for c in cases for k, text in launching(c, cus)]
    q8, q8o, q8d = ([(c, k, t) for c, k, t in texts if k.lib == lib] for lib in ("q8", "q8o", "q8d"))
    want = {f"q8: {r.symbol}": any(r.symbol in t for _, _, t in q8) for r in T.Q8_INSTANTIATIONS if r.kind == "gemm"}
    assert len(want) == 16
    for r in T.Q8_INSTANTIATIONS:
        if r.kind == "rows":
            for path in ("vector", "scalar"):
                want[f"q8: {r.symbol} ({path} path)"] = any(f"{r.symbol} ({path} path)" in t for _, _, t in q8)
                want[f"q8: {r.symbol} ({path} path) alone"] = any(f"{r.symbol} ({path} path)" in t for _, k, t in q8 if k.form == "F1")
    want.update({f"q8o: {r.symbol}": any(r.symbol in t for _, _, t in q8o) for r in TC.Q8O_INSTANTIATIONS})
    assert len(TC.Q8O_INSTANTIATIONS) == 4
    for out8 in ("false", "true"):
        for stores in ("wide", "single"):
            want[f"q8d: qdecode_finish_kernel<{out8}>, {stores} stores"] = any(
                f"qdecode_finish_kernel<{out8}>," in t and t.endswith(f"{stores} stores") for _, _, t in q8d)
        want[f"q8d: qdecode_finish_kernel<{out8}> alone"] = any(f"qdecode_finish_kernel<{out8}> alone" in t and c.in_ == 0 for c, _, t in q8d)
    splits_of = lambda t: int(t.split(" strips x ")[1].split(" splits")[0]) if "partial" in t else 0
    want["q8d: one split"] = any(splits_of(t) == 1 for _, _, t in q8d)
    want["q8d: the plan's own choice above one split"] = any(c.splits == 0 and splits_of(t) > 1 for c, _, t in q8d)
    want["q8d: two splits forced"] = any(c.splits == 2 and splits_of(t) == 2 for c, _, t in q8d)
    want["q8d: three splits forced"] = any(c.splits == 3 and splits_of(t) == 3 for c, _, t in q8d)
    want["q8d: several strips"] = any("partial" in t and not t.startswith("qdecode_partial_kernel, 1 strips") for _, _, t in q8d)
    missing = [name for name, reached in want.items() if not reached]
    assert not missing, f"{cus} CUs: the list does not reach {missing}"


@built_lib.needs_library
def test_the_libraries_plans_say_the_same_of_every_call(cus):
    """mmh_q8_linear_plan, mmh_q8o_linear_plan, mmh_q8d_linear_plan (host arithmetic in the three libraries) against
    qlinear_ref.plan_text, qchain_ref.plan_text_s8o and qdecode_ref.plan, text and bytes: the coverage above is the libraries'."""
    if not built_lib.library_loads():
        pytest.skip("the libraries (or the HIP runtime they link) are not loadable here")
    calls = [(c, k) for c in F.cases(N, SEED, cus) for k in F.calls(c)]
    assert len(calls) > 5 * N
    for c, k in calls:
        assert F.library_plan(k, cus) == F.python_plan(k, cus), (c, k)


# ---- the list is not vacuous ------------------------------------------------------------------------------------------------------
def test_no_case_is_skipped_and_few_end_in_a_refusal(cus, table):
    rows = table
    for c, inp, _, exp in rows:
        L, forms = F.layout(c), [k.form for k in F.calls(c)]
        assert forms[:2] == ["F1", "F2"] and "F4 default rows" in forms, c
        assert ("F3" in forms) == ("F4 F1's rows" in forms) == L.rows_ok and ("F5" in forms) == L.chain_ok, c
        assert ("F6 fp32" in forms) == ("F6 int8" in forms) == (c.rows <= 16 and L.splits_ok), c
        assert (exp["F6"] is not None) == (c.rows <= 16) and all(exp[f] is not None for f in ("F1", "F2", "F3", "F4", "F5")), c
        assert exp["F2"].shape == (c.rows, c.out) and exp["F4"][0].shape == (c.rows, c.out) and exp["F5"].shape == (c.rows, c.out2), c
        assert exp["F4"][0].dtype == np.int8 and np.isfinite(exp["F4"][2]).all() and (exp["F4"][2] > 0).all(), c
    assert sum(not F.layout(c).rows_ok for c, *_ in rows) <= N // 3
    assert sum(not F.layout(c).chain_ok for c, *_ in rows) <= N // 3
    assert sum(not F.layout(c).rows_ok for c, *_ in rows) >= 4 and sum(not F.layout(c).chain_ok for c, *_ in rows) >= 4
    # one-row windows that carry their own stride: accepted by QRows at an odd pitch, refused by _rows_args at one
    assert any(c.rows == 1 for c, *_ in rows)


def test_the_int8_expectations_saturate_in_some_cases_and_not_in_others(cus, table):
    holds_127 = [bool((np.abs(exp["F4"][0].astype(np.int16)) == 127).any()) for *_, exp in table]
    assert sum(holds_127) >= N // 4, sum(holds_127)
    assert holds_127.count(False) >= N // 4, holds_127.count(False)
    assert not any((exp["F4"][0] == -128).any() for *_, exp in table)
    # ... and most expectations use the range (a +-1e6 bias under a per-matrix scale, or in == 0 without a bias, leave few values)
    assert sum(np.count_nonzero(np.bincount(exp["F4"][0].view(np.uint8).ravel(), minlength=256)) > 64 for *_, exp in table) >= N // 2


def test_every_special_value_reaches_the_expectation_where_it_is_planted(cus, table):
    seen = set()
    for c, inp, rules, exp in table:
        assert set(inp.planted) == set(c.specials), c
        y, (yq, _, so) = exp["F2"], exp["F4"]
        for name, at in inp.planted.items():
            where, kind = name.split(":")
            seen.add(name)
            if where in ("x", "w"):
                q, s, _ = exp["F1"] if where == "x" else rules.quantize_rows_ref(inp.w)
                v = inp.x if where == "x" else inp.w
                (_, _, scale, check), = [r for r in R.special_rows(c.in_, np.random.default_rng(0)) if r[0] == kind]
                assert check(q[at]), (c, name)
                finite = np.abs(np.where(np.isfinite(v[at]), v[at], np.float32(0))).max()
                assert same_bits(s[at:at + 1], [Q.scale_of_amax(finite)]) and (kind in ("NaN", "+-inf") or s[at] == scale), (c, name)
            elif kind == "NaN":
                assert np.isnan(inp.bias[at]).all() and np.isnan(y[:, at]).all() and not yq[:, at].any(), (c, name)
            elif kind == "+-inf":
                assert (y[:, at[0]] == np.inf).all() and (yq[:, at[0]] == 127).all(), (c, name)
                if len(at) > 1:
                    assert (y[:, at[1]] == (0 if c.relu else -np.inf)).all() and (yq[:, at[1]] == (0 if c.relu else -127)).all(), (c, name)
            elif kind == "-0.0":   # +0 (the sum's) + -0 is +0: the column is what no bias gives, and never -0
                assert np.signbit(inp.bias[at]).all() and not inp.bias[at].any()
                assert not np.signbit(y[:, at][y[:, at] == 0]).any(), (c, name)
            elif kind == "+-1e6":
                assert (y[:, at[0]] > 9e5).all(), (c, name)
                if len(at) > 1:
                    assert (y[:, at[1]] == 0).all() if c.relu else (y[:, at[1]] < -9e5).all(), (c, name)
            else:   # ties: y is the bias, its largest element 127, so the scale is scale_factor and the scaled values are halves
                assert kind == "ties" and c.in_ == 0 and (so == np.float32(c.scale_factor)).all(), (c, name, so[:4])
                t = np.maximum(inp.bias[at[1:]], 0) * so[0] if c.relu else inp.bias[at[1:]] * so[0]
                assert same_bits(y[0, at], np.maximum(inp.bias[at], 0) if c.relu else inp.bias[at]), (c, name)
                assert len(at) >= 2 and (np.abs(t[t != 0]) % 1 == 0.5).all() and (t != 0).any(), (c, name, t)
    kinds = {f"{w}:{k}" for w in ("x", "w") for k in F.ROW_KINDS} | {f"bias:{k}" for k in F.BIAS_KINDS} | {"bias:ties"}
    assert seen == kinds, kinds - seen


# ---- the oracle tells wrong kernels apart -------------------------------------------------------------------------------------------
def _bias_before_rw(acc, rx, rw, bias=None, relu=False):
    with np.errstate(all="ignore"):
        y = acc.astype(np.float32) * rx.astype(np.float32)[:, None]
        if bias is not None:
            y = y + np.asarray(bias, np.float32)[None, :]
        y = y * rw.astype(np.float32)[None, :]
        return np.where(y <= 0, np.float32(0.0), y) if relu else y


def _relu_drops_nan(acc, rx, rw, bias=None, relu=False):
    y = R.epilogue_ref(acc, rx, rw, bias, False)
    with np.errstate(all="ignore"):
        return np.where(y > 0, y, np.float32(0.0)) if relu else y


def _requant(rounding, low):
    def requant(y, so):
        y, so = np.asarray(y, np.float32), np.asarray(so, np.float32).reshape(-1, 1)
        with np.errstate(all="ignore"):
            t = np.where(np.isnan(y), np.float32(0.0), y * so)
            r = np.fmin(np.fmax(rounding(t), np.float32(low)), np.float32(127.0))
        q = np.empty(r.shape, np.int8)
        q[...] = r
        return q
    return requant


def _half_away(t):
    return (np.sign(t) * np.floor(np.abs(t.astype(np.float64)) + 0.5)).astype(np.float32)


def _double_reciprocal(rounded):
    """The quantiser whose inv_scale is 1 / (double)scale: rounded to float32 (the innocuous reading), or kept in double."""
    def quantize(x):
        q, s, _ = R.quantize_rows_ref(x)
        with np.errstate(all="ignore"):
            r = 1.0 / s.astype(np.float64)
        return q, s, r.astype(np.float32) if rounded else r
    return quantize


def _epilogue_on_double_rx(acc, rx, rw, bias=None, relu=False):
    with np.errstate(all="ignore"):
        y = (acc.astype(np.float32).astype(np.float64) * np.asarray(rx, np.float64)[:, None]).astype(np.float32)
    return R.epilogue_ref(y, np.ones(len(rx), np.float32), rw, bias, relu)   # (y is exact in float32: the first product is done)


def _differs(a, b):
    """Two expectations differ in some form's bits."""
    flat = lambda e: [np.asarray(v) for f in ("F1", "F2", "F4", "F5", "F6", "F7") if e[f] is not None for v in (e[f] if isinstance(e[f], tuple) else (e[f],))]
    return any(not (np.array_equal(p, q) if p.dtype in (np.int8, np.uint8) else same_bits(p, q)) for p, q in zip(flat(a), flat(b)))


# ---- mutants of the 4-bit rules (tests/q4_ref.py: quantize4_ref, pack_ref, unpack_ref) ----------------------------------------------
def _quantize4(low=-7.0, numerator=7.0, rounding=np.rint, inf_to_zero=False, finite_amax=True):
    """quantize4_ref with one rule changed."""
    def quantize(w):
        w = np.ascontiguousarray(w, dtype=np.float32)
        a = np.abs(w)
        if finite_amax:
            a = np.where(np.isfinite(a), a, np.float32(0))
        with np.errstate(all="ignore"):
            amax = [np.float32(r.max()) if r.size else np.float32(0) for r in a]
            s = np.array([np.minimum(np.float32(numerator) / m, R.F32_MAX) if m > 0 else np.float32(1) for m in amax], np.float32)
            t = w * s[:, None]
            t = np.where(np.isnan(w) | (np.isinf(w) & inf_to_zero), np.float32(0), t)
            r = np.fmin(np.fmax(rounding(t), np.float32(low)), np.float32(7))
            inv = np.float32(1.0) / s
        q = np.empty(w.shape, np.int8)
        q[...] = r
        return q, s, inv
    return quantize


def _pack_halves_swapped(W):
    """pack_ref with the low nibble holding the second half of each slice."""
    W = np.asarray(W, np.int8)
    in_, n = W.shape
    full = np.zeros((-(-in_ // P4.SLICE) * P4.SLICE, n), np.int8)
    full[:in_] = W
    swapped = full.reshape(-1, 2, P4.HALF, n)[:, ::-1].reshape(-1, n)
    return P4.pack_ref(swapped)


def _unpack_zero_extended(P, in_):
    P = np.asarray(P, np.uint8)
    p = P.reshape(P.shape[0] // P4.HALF, 1, P4.HALF, P.shape[1])
    return np.concatenate([p & 15, p >> 4], 1).reshape(-1, P.shape[1]).astype(np.int8)[:in_]


MUTANTS = {
    "drop the last byte of k": lambda r: dict(int_sums=lambda qx, qw: R.int_sums(qx[:, :max(qx.shape[1] - 1, 0)], qw[:, :max(qw.shape[1] - 1, 0)])),
    "add the bias before multiplying by rw": lambda r: dict(epilogue_ref=_bias_before_rw),
    "ReLU sends NaN to 0": lambda r: dict(epilogue_ref=_relu_drops_nan),
    "requant rounds half away from zero": lambda r: dict(requant_ref=_requant(_half_away, -127.0)),
    "requant clamps at -128": lambda r: dict(requant_ref=_requant(np.rint, -128.0)),
    "inv_scale kept as a double reciprocal of the rounded scale": lambda r: dict(quantize_rows_ref=_double_reciprocal(False), epilogue_ref=_epilogue_on_double_rx),
    "4-bit: clamp to -8 .. 7": lambda r: dict(quantize4_ref=_quantize4(low=-8.0)),
    "4-bit: scale 8 / amax": lambda r: dict(quantize4_ref=_quantize4(numerator=8.0)),
    "4-bit: round half away from zero": lambda r: dict(quantize4_ref=_quantize4(rounding=_half_away)),
    "4-bit: the nibble halves of a slice swapped in the image": lambda r: dict(pack_ref=_pack_halves_swapped),
    "4-bit: nibbles zero-extended": lambda r: dict(unpack_ref=_unpack_zero_extended),
    "4-bit: inf quantised to 0": lambda r: dict(quantize4_ref=_quantize4(inf_to_zero=True)),
    "4-bit: abs-max over non-finite elements too": lambda r: dict(quantize4_ref=_quantize4(finite_amax=False)),
}
RULES_4BIT = {"quantize4_ref", "pack_ref", "unpack_ref"}   # a mutant of these alone changes F7 only: cases without F7 are not recomputed


def _first_split_only(c, inp, rules, cus):
    """The expectation of a decode whose finish kernel reads only the first K range's partials, or None where the case's decode
    call has one range or none."""
    L = F.layout(c)
    if not (L.decode and L.splits_ok and c.in_ > 0):
        return None
    _, _, splits, k_len = D.plan(c.rows, c.out, c.in_, False, L.ldy, L.y16, c.splits, cus)
    if splits < 2:
        return None
    return F.expected(c, inp, mutate(rules, int_sums=lambda qx, qw: R.int_sums(qx[:, :k_len], qw[:, :k_len])))


def test_every_mutant_of_the_reference_differs_from_it_in_some_case(cus, table):
    counts = {}
    for name, swap in MUTANTS.items():
        rows = [t for t in table if t[3]["F7"] is not None] if set(swap(None)) <= RULES_4BIT else table
        counts[name] = sum(_differs(F.expected(c, inp, mutate(rules, **swap(rules))), exp) for c, inp, rules, exp in rows)
    name = "decode sums only the first split"
    counts[name] = 0
    for c, inp, rules, exp in table:
        wrong = _first_split_only(c, inp, rules, cus)
        if wrong is not None:
            assert exp["F6"] is not None
            counts[name] += not (same_bits(wrong["F6"][0], exp["F6"][0]) and np.array_equal(wrong["F6"][1], exp["F6"][1]))
    for name, n in counts.items():
        print(f"{cus} CUs: {name}: {n} of {N} cases differ")
    assert all(n > 0 for n in counts.values()), counts
    # the innocuous reading of the last one: the double reciprocal rounded to float32 is the float32 quotient, everywhere
    same = dict(quantize_rows_ref=_double_reciprocal(True))
    assert not any(_differs(F.expected(c, inp, mutate(rules, **same)), exp) for c, inp, rules, exp in table[:24])
    # requant's two mutants are told apart by their own rules: a tie of even integer part, a product at or below -127.5
    for c, inp, rules, exp in table:
        if "bias:ties" in c.specials:
            wrong = F.expected(c, inp, mutate(rules, requant_ref=_requant(_half_away, -127.0)))
            assert not np.array_equal(wrong["F4"][0], exp["F4"][0]), c


# ---- F7: the 4-bit weight on the decode cases ----------------------------------------------------------------------------------------
def _eligible(rows):
    """The cases (or table rows) that run F7: at most 16 rows."""
    return [r for r in rows if (r if isinstance(r, F.Case) else r[0]).rows <= D.MAX_ROWS]


def test_the_4_bit_launches_reach_every_form_of_their_library(cus):
    """The F7 launch texts of the list (q4_ref.plan; the test above holds it to mmh_q4d_linear_plan on every call): both finish
    kernels, both store forms, the finish kernel alone, forced counts 1 - 3 and the plan's own choice above one range."""
    el = _eligible(F.cases(N, SEED, cus))
    assert len(el) >= 16 and all(c.rows <= 16 for c in el)                  # strata 4 and 5 whole, and what stratum 6 draws
    q4d = [(c, k, t) for c in el for k, t in launching(c, cus) if k.lib == "q4d"]
    assert all(k.form in ("F7 fp32", "F7 int8") for _, k, _ in q4d) and not any(k.lib == "q4d" for c in F.cases(N, SEED, cus)
                                                                               if c.rows > 16 for k in F.calls(c))
    splits_of = lambda t: int(t.split(" strips x ")[1].split(" splits")[0]) if "partial" in t else 0
    want = {}
    for out8 in ("false", "true"):
        for stores in ("wide", "single"):
            want[f"qdecode_finish_kernel<{out8}>, {stores} stores"] = any(
                f"qdecode_finish_kernel<{out8}>," in t and t.endswith(f"{stores} stores") for _, _, t in q4d)
        want[f"qdecode_finish_kernel<{out8}> alone"] = any(f"qdecode_finish_kernel<{out8}> alone" in t and c.in_ == 0 for c, _, t in q4d)
    for forced in (1, 2, 3):
        want[f"{forced} ranges forced"] = any(c.splits == forced and splits_of(t) == forced for c, _, t in q4d)
    want["q4decode_partial_kernel"] = any(t.startswith("q4decode_partial_kernel, ") for _, _, t in q4d)
    want["several strips"] = any("partial" in t and not t.startswith("q4decode_partial_kernel, 1 strips") for _, _, t in q4d)
    missing = [name for name, reached in want.items() if not reached]
    assert not missing, f"{cus} CUs: F7 does not reach {missing}"
    own = {c for c, _, t in q4d if c.splits == 0 and splits_of(t) > 1}
    assert len(own) >= 4, (cus, len(own))
    both = [c for c in el if {k.form for k in F.calls(c)} >= {"F7 fp32", "F7 int8"}]
    assert len(both) >= 16 and all(F.layout(c).splits_ok for c in both), len(both)
    assert all(("F7 fp32" in {k.form for k in F.calls(c)}) == F.layout(c).splits_ok for c in el)


def test_the_4_bit_forms_meet_both_weight_windows_and_both_answers_of_from_image(cus):
    el = _eligible(F.cases(N, SEED, cus))
    adopted = [c for c in el if F.layout(c).image_ok]
    assert 2 * len(adopted) >= len(el) and len(el) - len(adopted) >= 4, (len(el), len(adopted))
    # a refused window has a pitch or a base that is no multiple of 4; an adopted one of in > 0 has neither
    for c in el:
        L = F.layout(c)
        assert L.image_ok == (c.in_ == 0 or ((c.out + c.ldyq_pad) % 4 == 0 and c.off_yq % 4 == 0)), c
    assert any((c.out + c.ldyq_pad) % 4 and c.off_yq % 4 == 0 for c in el) and any(c.off_yq % 4 and (c.out + c.ldyq_pad) % 4 == 0 for c in el)
    # the weight is read dense in one half and through a row-strided window in the other: exactly in turn in strata 4 and 5
    decode = [c for i, c in enumerate(F.cases(N, SEED, cus)) if i % F.STRATA in (4, 5)]
    assert [F.layout(c).w4_strided for c in decode] == [False, True] * (len(decode) // 2)
    strided = [c for c in el if F.layout(c).w4_strided and c.in_ > 0]
    assert len(strided) >= 6 and any(c.off_x % 4 for c in strided) and any(c.ldx_pad % 4 for c in strided) and \
        any(c.off_x % 4 == 0 and (c.in_ + c.ldx_pad) % 4 == 0 for c in strided)
    assert not any(F.layout(c).w4_strided for c in F.cases(N, SEED, cus) if c.rows > 16)


def test_the_4_bit_expectation_is_q4_refs_want_on_the_references_image(cus, table):
    """expected()'s F7 takes q4_ref.want's steps through the named rules, so that mutants can replace them; with the true rules it
    IS q4_ref.want of the reference's rows and packed image (the int8 output under the scales of the 4-bit fp32 result), and its
    image is the packed quantise4_ref of w."""
    el = _eligible(table)
    for c, inp, rules, exp in el:
        qx, _, rx = exp["F1"]
        image, s4, r4, y4, yq4, so4 = exp["F7"]
        q, s, inv = P4.quantize4_ref(inp.w)
        assert np.array_equal(image, P4.pack_ref(np.ascontiguousarray(q.T))) and image.dtype == np.uint8, c
        assert image.shape == (P4.layout(c.out, c.in_)[1], c.out) and same_bits(s4, s) and same_bits(r4, inv), c
        bias = inp.bias if c.bias else None
        assert same_bits(y4, P4.want(qx, rx, image, c.in_, r4, bias, c.relu)), c
        assert same_bits(so4, F.out_scales(c, y4)) and np.isfinite(so4).all() and (so4 > 0).all(), c
        assert np.array_equal(yq4, P4.want(qx, rx, image, c.in_, r4, bias, c.relu, so4)) and yq4.dtype == np.int8, c
        assert int(np.abs(q).max(initial=0)) <= 7, c
    assert all(exp["F7"] is None for c, _, _, exp in table if c.rows > 16)
    # the 4-bit result is not the 8-bit one: its own scales matter
    assert sum(not same_bits(exp["F7"][5], exp["F4"][2]) for *_, exp in el) >= len(el) // 2
    # the mutants' common base is the reference
    for c, inp, _, exp in el[:6]:
        q, s, inv = _quantize4()(inp.w)
        assert np.array_equal(q, P4.unpack_ref(exp["F7"][0], c.in_).T) and same_bits(s, exp["F7"][1]) and same_bits(inv, exp["F7"][2])


def test_the_4_bit_int8_expectation_saturates_where_the_scale_factor_says(cus, table):
    """so4 is scale_factor x 127 / (the largest finite |y4| of the row or the matrix): at a factor of 1 or more that maximum
    lands on +-127 (or is clamped there), at 0.5 no finite value passes 64.  A row (matrix) without a finite non-zero value has
    no maximum to land anywhere, and a scale that was clamped to FLT_MAX brings it nowhere near."""
    el = _eligible(table)
    holds_127 = []
    for c, _, _, exp in el:
        y4, yq4 = exp["F7"][3], exp["F7"][4]
        top = int(np.abs(yq4.astype(np.int16)).max())
        holds_127.append(top == 127)
        assert not (yq4 == -128).any(), c
        if not (np.isfinite(y4) & (y4 != 0)).any() or (exp["F7"][5] == R.F32_MAX).any():
            continue
        if c.scale_factor >= 1:
            assert top == 127, (c, top)
        elif not np.isinf(y4).any():
            assert top <= 64, (c, top)
    assert sum(holds_127) >= 4 and holds_127.count(False) >= 2, holds_127


def test_the_4_bit_special_values_reach_the_packed_image(cus, table):
    """The case's "w:<kind>" channel and the W4_TIES channel as quantize4_ref must leave them, read back out of the image."""
    seen, ties = set(), 0
    for c, inp, _, exp in _eligible(table):
        image, s4 = exp["F7"][0], exp["F7"][1]
        W = P4.unpack_ref(image, c.in_)   # (in, out)
        for name, at in inp.planted.items():
            where, kind = name.split(":")
            if where != "w":
                continue
            seen.add(kind)
            q, v = W[:, at], inp.w[at]
            finite = np.abs(np.where(np.isfinite(v), v, np.float32(0))).max()
            assert same_bits(s4[at:at + 1], [P4.q4_scale_of_amax(finite)]), (c, name)
            if kind == "all zero":
                assert not q.any() and s4[at] == 1
            elif kind == "NaN":
                assert q[1] == 0 and np.abs(q).max() == 7
            elif kind == "+-inf":
                assert q[0] == 7 and q[2] == -7
            elif kind == "max 1e-38":   # rint(1e-38 * FLT_MAX) = rint(3.4)
                assert s4[at] == R.F32_MAX and q[3] == 3 and not np.delete(q, 3).any()
            else:
                assert kind == "-max" and (q == -7).all()
        if inp.ties4 is not None:
            ties += 1
            assert inp.ties4 not in [r for n, r in inp.planted.items() if n.startswith("w:")] and s4[inp.ties4] == 2, c
            assert W[:4, inp.ties4].tolist() == [7, 0, -2, 2], (c, W[:4, inp.ties4])      # 7, 0.5, -1.5, 2.5: half to even
        else:
            assert c.in_ < len(F.W4_TIES) or c.out == 1, c
    assert seen == set(F.ROW_KINDS), set(F.ROW_KINDS) - seen
    assert ties >= 12, ties
    assert all(inp.ties4 is None for c, inp, _, _ in table if c.rows > 16)
