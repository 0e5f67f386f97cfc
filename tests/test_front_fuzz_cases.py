"""The seeded case list of the fp32 tensor front end's fuzz (tests/front_fuzz.py: cases(64, 2026, cus), run by
tests/test_gpu_front_fuzz.py) is what it promises, checked on the CPU at 256 (the MI355X), 304 and 64 compute units:
deterministic; every stratum has its cases and every view class occurs on every operand that admits it; every entry point, `need`
mask and `input` kind occurs; by the library's plan functions on the addressing model's launches the three tiles run guarded and
whole, all four operand pairs occur and AUTO folds a batch and runs one as one launch, plain and `ex`; the model reproduces every
view's logical contents from the flat storage; and the list is not vacuous: at most eight refusals, the planted NaN and -0.0
reach the expectations, and for each wrong front end below the expectation gathered through it differs from the true one.

Cases of the 64 whose expectation differs, per wrong front end, at 256 / 304 / 64 compute units (printed by the mutant test):
    ld taken as cols instead of stride(0)                              43 / 43 / 43
    storage offset dropped                                             52 / 52 / 52
    a transposed view read row-major, ld unchanged                     21 / 21 / 21
    an expanded operand's batch stride taken as packed                  8 /  8 /  8
    a batch of one's rule (no batch stride) applied to a batch of more  8 /  8 /  8
    a per-matrix bias read as shared                                   11 / 11 / 11
    beta input lost when out is not input                              28 / 28 / 28
    (n,) input with beta != 1 added unscaled as a bias                 22 / 22 / 22
    grad_w= as a chain started at grad_w                               11 / 11 / 11
    an expanded grad_out read with its strides as given                12 / 12 / 12
The fifth is read as: the front end passes batch stride 0 for a batch of one, whatever stride(0) says; the wrong front end does
so for A in a batch of more, so every matrix of the batch reads A[0]."""
import numpy as np
import pytest

import built_lib
import front_fuzz as F
from bitcmp import same_bits

N, SEED = 64, 2026
CU_COUNTS = (256, 304, 64)
READ_SIDE = {"a": "a", "b": "b", "c0": "c", "inp": "inp", "g": "g", "y": "y", "x": "x", "w": "w", "gw": "gw"}   # logical array -> its view


@pytest.fixture(scope="module", params=CU_COUNTS, ids=lambda n: f"{n}cus")
def cus(request):
    return request.param


_TABLE = {}


@pytest.fixture(scope="module")
def table(cus, oracle):
    """[(case, inputs, expectation)] of the list at a CU count; a case the CU counts share is computed once."""
    out = []
    for c in F.cases(N, SEED, cus):
        key = repr(c)
        if key not in _TABLE:
            v = F.inputs(c)
            _TABLE[key] = (c, v, F.expected(c, v) if c.family != "refuse" else {})
        out.append(_TABLE[key])
    return out


def by(cases, s):
    return cases[s::F.STRATA]


def stored(view):
    """(rows, cols, s0, s1) of a view's matrices."""
    return view.shape[-2:] + view.strides[-2:]


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_the_list_is_deterministic(cus):
    a, b = F.cases(N, SEED, cus), F.cases(N, SEED, cus)
    assert a == b and len(a) == N and [c.index for c in a] == list(range(N)) and [c.stratum for c in a] == [i % 8 for i in range(N)]
    assert F.cases(16, SEED, cus) == a[:16], "a shorter list is a prefix"
    assert F.cases(N, SEED + 1, cus) != a
    for n in (0, 7, 12, 63, -8):
        with pytest.raises(ValueError):
            F.cases(n, SEED, cus)
    for c in a[:16]:
        x, y = F.inputs(c), F.inputs(c)
        assert x.keys() == y.keys() and x["planted"] == y["planted"]
        assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in x if k != "planted")


# ---- strata and view classes ------------------------------------------------------------------------------------------------------
def test_the_strata_and_view_classes_are_what_the_module_says(cus):
    cases = F.cases(N, SEED, cus)
    assert [[c.family for c in by(cases, s)] for s in range(8)] == [[f] * 8 for f in ("2d", "2d", "2d", "3d", "3d", "back", "back", "refuse")]
    assert sum(c.side_stream for c in cases) == N // 2 and all(sum(c.side_stream for c in by(cases, s)) == 4 for s in range(8))
    assert all({c.ab for c in by(cases, s)} == set(F.AB) for s in range(5))
    # 0: whole tiles, everything 16-byte aligned; all four operand pairs
    for c in by(cases, 0):
        assert c.m % 128 == 0 and c.n % 128 == 0 and c.k % 32 == 0 and 128 <= c.m <= 384 and 128 <= c.n <= 384, c
        for name in ("a", "b", "c", "inp"):
            r = F.read(c.views[name], name in "ab")
            assert r.ld % 4 == 0 and r.offset % 4 == 0, (c, name)
    assert {(F.read(c.views["a"]).op, F.read(c.views["b"]).op) for c in by(cases, 0)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # 1: every 2-D class on A and on B, every window class on out and input; sizes from the issue's list
    one = by(cases, 1)
    assert {c.kinds["a"] for c in one} == set(F.K2) == {c.kinds["b"] for c in one}
    assert {c.kinds["c"] for c in one} == set(F.KC) == {c.kinds["inp"] for c in one}
    assert all(x in F.SIZES + F.RAGGED for c in one for x in (c.m, c.n, c.k)) and any(x in F.RAGGED for c in one for x in (c.m, c.n, c.k))
    for name in ("a", "b", "c", "inp"):
        views = [c.views[name] for c in one]
        lds = {max(v.strides[-2:]) - (v.shape[1] if v.strides[1] == 1 else v.shape[0]) for v in views}
        assert lds >= {0} and lds & set(F.PADS), (name, lds)                      # contiguous and row-strided
        assert {(v.offset - F.FRONT) for v in views} >= {0} and any(1 <= v.offset - F.FRONT <= 3 for v in views), name   # 4-byte bases
    assert all(v.offset >= F.FRONT for c in cases for v in c.views.values())       # a guard band in front of every view
    # 2: each of m, n, k zero; 1 x 1; one row and one column
    two = by(cases, 2)
    assert [(c.m == 0, c.n == 0, c.k == 0) for c in two[:3]] == [(True, False, False), (False, True, False), (False, False, True)]
    assert any((c.m, c.n, c.k) == (1, 1, 1) for c in two) and any(c.m == 1 and c.n == 1 and c.k > 1 for c in two)
    # one row / one column of an operand, reached both ways: as a window of a larger matrix (N: row stride ld > cols) and as the
    # .t() of the other (strides (1, ld)) -- over the 2-D operands and the matrices of the 3-D ones
    ops = [stored(c.views[name]) for c in cases if c.family in ("2d", "3d") for name in ("a", "b")]
    row_window = [v for v in ops if v[0] == 1 and v[1] > 1 and v[3] == 1 and v[2] > v[1]]
    row_as_t = [v for v in ops if v[0] == 1 and v[1] > 1 and v[2] == 1 and v[3] > 1]
    col_window = [v for v in ops if v[1] == 1 and v[0] > 1 and v[2] > 1 and v[3] == 1]
    col_as_t = [v for v in ops if v[1] == 1 and v[0] > 1 and v[2] == 1 and v[3] > v[0]]
    assert row_window and row_as_t and col_window and col_as_t, (len(row_window), len(row_as_t), len(col_window), len(col_as_t))
    for name in ("a", "b"):
        mine = [stored(c.views[name]) for c in cases if c.family in ("2d", "3d")]
        assert any(v[0] == 1 and v[1] > 1 for v in mine) and any(v[1] == 1 and v[0] > 1 for v in mine) and any(v[:2] == (1, 1) for v in mine), name
    # the model reads every such view N where both readings address it
    assert all(F.read2(v[:2], v[2:], 0, True).op == 0 for v in row_window + col_window)
    # 3: batch strides: expanded A, B and both; gapped; no multiple of 4; transposed matrices
    three = by(cases, 3)
    pairs = {(c.kinds["a"].split("/")[1], c.kinds["b"].split("/")[1]) for c in three}
    assert {(x == "expand", y == "expand") for x, y in pairs} == {(True, False), (False, True), (True, True), (False, False)}
    assert {k for p in pairs for k in p} >= {"gapped", "odd", "expand"} and {c.batch for c in three} == set(F.BATCHES)
    assert any(c.views[n].strides[0] % 4 for c in three for n in ("a", "b", "c")) and any(c.kinds["a"].startswith("t") for c in three)
    assert {c.kinds["bias"] for c in three} == {"strided", "packed", "shared", "None"}
    # 4: batch 0, a batch of one that keeps a larger tensor's stride, k == 0
    four = by(cases, 4)
    assert any(c.batch == 0 for c in four) and any(c.k == 0 and c.batch > 1 for c in four)
    sliced = [c for c in four if c.batch == 1]
    assert sliced and all(c.views[n].strides[0] > 0 and F.read(c.views[n], n != "c").bstride == 0 for c in sliced for n in ("a", "b", "c"))
    # 5 / 6: the backward's windows; rows, in_features, out_features of 0 and of 1; more than one row block
    assert {c.kinds[n] for c in by(cases, 5) for n in ("g", "y", "x", "w")} == set(F.KC)
    six = by(cases, 6)
    assert [(c.m == 0, c.k == 0, c.n == 0) for c in six[:3]] == [(True, False, False), (False, True, False), (False, False, True)]
    assert [(c.m == 1, c.k == 1, c.n == 1) for c in six[3:6]] == [(True, False, False), (False, True, False), (False, False, True)]
    assert any(c.m > 2 * F.R_BLOCK for c in six)
    assert {c.relu for c in by(cases, 5)} == {True, False} == {c.bias for c in by(cases, 6)}
    # 7: the refusals, each once
    assert [c.refusal for c in by(cases, 7)] == list(F.REFUSALS) and all(c.refusal is None for c in cases if c.stratum != 7)
    assert sum(c.family == "refuse" for c in cases) <= 8


def test_every_entry_point_need_mask_and_input_kind_occurs(cus):
    cases = F.cases(N, SEED, cus)
    forms = [(c, f) for c in cases for f in F.forms(c)]
    assert {f.entry for _, f in forms} == {"matmul", "addmm", "linear", "bmm", "baddbmm", "batched_linear", "relu_grad_colsum",
                                          "linear_backward", "autograd.linear", "refusal"}
    names = {f.name for _, f in forms}
    assert names >= {f"linear_backward need={need}" for need in F.NEEDS} and len(F.NEEDS) == 8
    assert names >= {"addmm " + k for k in F.ADDMM_INPUTS} | {"baddbmm " + k for k in F.BADDBMM_INPUTS}
    assert names >= {"autograd " + k for k in ("contiguous", "expanded", "transposed")} | {"matmul accumulate", "bmm accumulate"}
    # the (n,) and (batch, 1, n) inputs are the kernel's bias where beta == 1 and a scaled copy elsewhere, both in the list
    for key in ("vec", "pm", "pe"):
        kinds = {F.bias_reading(c.views[key], c.batch, c.n, F.bias_beta(c), False)[0] for c in cases if c.family == "3d"}
        assert kinds == {"bias", "copy"}, (key, kinds)
    per_matrix = {F.bias_reading(c.views["pm"], c.batch, c.n, 1.0, False)[2] for c in cases if c.family == "3d"}
    assert 0 in per_matrix and any(s > 0 for s in per_matrix)          # (a batch of one: no bias stride)
    assert {F.bias_reading(c.views["pe"], c.batch, c.n, 1.0, False)[2] for c in cases if c.family == "3d"} == {0}
    assert all(F.bias_reading(c.views["vec"], None, c.n, be, False)[0] == ("bias" if bias else "copy")
               for c in cases if c.family == "2d" and c.n > 0 for bias in (True, False) for be in [F.vec_ab(c, bias)[1]])
    assert any(c.ab[1] == 0 for c in cases)                            # beta == 0 runs over a NaN input
    # every form of a case takes the next of the seven kernel configurations; all seven meet every entry point
    seen = {(f.entry, F.config_of(c, number)) for c in cases for number, f in enumerate(F.forms(c)) if c.family != "refuse"}
    for entry in ("matmul", "addmm", "linear", "bmm", "baddbmm", "batched_linear", "linear_backward", "autograd.linear"):
        assert {cfg for e, cfg in seen if e == entry} == set(F.CONFIGS), entry


@built_lib.needs_library
def test_the_plan_functions_say_the_list_reaches_the_tiles_pairs_and_batched_forms(cus):
    if not built_lib.library_loads():
        pytest.skip("the library (or the HIP runtime it links) is not loadable here")
    cases = F.cases(N, SEED, cus)
    tiles, pairs, batched = set(), set(), set()
    for c in cases:
        for number, f in enumerate(F.forms(c)):
            L = f.launch
            if L is None:
                continue
            kernel, _ = F.config_of(c, number)
            name, form = F.plan_of(L, cus)         # (every launch the model predicts is one the plan functions accept)
            run = name if kernel == "auto" else kernel
            if run in F.FAMILY:
                tiles.add((run, F.whole(L, F.tile_of(run))))
            pairs.add((L.call, L.ta, L.tb))
            if L.batch is not None and kernel == "auto":
                batched.add((L.call, form))
    assert tiles == {(t, w) for t in F.TILES for w in (True, False)}, tiles
    assert pairs >= {(call, ta, tb) for call in ("ex", "batched", "batched_ex") for ta in (0, 1) for tb in (0, 1)}
    assert pairs >= {("nn", 0, 0), ("op", 0, 1), ("op", 1, 0), ("op", 1, 1)}
    assert batched >= {(call, form) for call in ("batched", "batched_ex") for form in ("fold", "one_launch")}, batched


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_the_model_gathers_every_views_logical_contents_from_the_flat_storage(cus, table):
    checked = 0
    for c, v, _ in table:
        for name, view in c.views.items():
            if len(view.shape) == 1 or name in ("pm", "pe", "m1", "1n", "b11") or (name == "bias" and c.family in ("3d", "refuse")):
                continue
            addr = F.read(view, name in ("a", "b"))
            assert addr is not None, (c.index, name, view)
            assert same_bits(F.gather(F.lay(view, v[name]), F.model_indices(addr, view.shape)).reshape(-1, 1), v[name].reshape(-1, 1)), (c.index, name)
            assert addr.ld >= 1 and (view.shape[0] > 1 or len(view.shape) == 2 or addr.bstride == 0), (c.index, name)
            checked += 1
    assert checked > 4 * N
    # what the front end must refuse: no unit stride, rows that overlap, a transposed output
    assert F.read2((4, 6), (12, 2), 0, True) is None and F.read2((4, 6), (5, 1), 0, True) is None and F.read2((4, 6), (0, 1), 0, True) is None
    assert F.read2((4, 6), (1, 4), 0, True).op == 1 and F.read2((4, 6), (1, 4), 0, False) is None and F.read2((4, 6), (1, 3), 0, True) is None


# ---- the list is not vacuous ------------------------------------------------------------------------------------------------------
def test_the_planted_values_reach_the_expectations(cus, table):
    nan_rows = neg_zero = gated = 0
    for c, v, e in table:
        zr, nan = v["planted"]["zero row"], v["planted"]["nan"]
        if c.family in ("2d", "3d") and nan is not None and c.n > 0 and c.batch != 0:
            product = e["matmul" if c.family == "2d" else "bmm"]
            assert np.isnan(product[..., nan[0], :]).all() and not np.isnan(np.delete(product, nan[0], axis=-2)).any(), c.index
            nan_rows += 1
            if c.ab == (-1.3, 1.0):      # s = +0 on the row of zeros, alpha s = -0, beta input = -0: the sum keeps the sign
                for form in ("addmm 2-D", "addmm out is input") if c.family == "2d" else ("baddbmm full", "baddbmm out is input"):
                    row = e[form][..., zr, :]
                    assert (row == 0).all() and np.signbit(row).all(), (c.index, form)
                neg_zero += 1
            linear = e["linear" if c.family == "2d" else "batched_linear"]
            assert np.isnan(linear[..., nan[0], :]).all(), (c.index, "ReLU keeps NaN")
        if c.family == "back" and nan is not None:
            dz = e["relu_grad_colsum"][0]
            open_gate = not c.relu or not v["y"][nan] <= 0
            assert bool(np.isnan(dz[nan])) == open_gate, c.index
            gated += open_gate
            row = dz[zr, ::2]
            assert (row == 0).all() and (np.signbit(row) == (~(v["y"][zr, ::2] <= 0) if c.relu else True)).all(), c.index
            neg_zero += bool(np.signbit(row).any())
    assert nan_rows >= 20 and neg_zero >= 8 and gated >= 4, (nan_rows, neg_zero, gated)
    # a batch's matrices, and a bias' rows, differ from each other
    for c, v, e in table:
        if c.family == "3d" and c.batch > 1 and c.m * c.n * c.k > 0:
            both = c.views["a"].strides[0] == 0 and c.views["b"].strides[0] == 0      # (one matrix each: one product)
            assert same_bits(e["bmm"][0], e["bmm"][1]) == both, c.index
            assert not same_bits(v["pm"][0], v["pm"][1]) and same_bits(v["pe"][0], v["pe"][1]), c.index


def _mutated(c, v, change):
    """The case's logical arrays as a front end reads them whose Addr of each read-side view is change(name, view, addr)."""
    out = dict(v)
    for name, view_name in READ_SIDE.items():
        if name in v and view_name in c.views:
            view = c.views[view_name]
            addr = change(name, view, F.read(view, name in ("a", "b")))
            out[name] = F.gather(F.lay(view, v[name]), F.model_indices(addr, view.shape))
    return out


def _stored_row(view, addr):
    rows, cols = view.shape[-2:]
    return (rows, cols) if addr.op == 0 else (cols, rows)


def _shared_bias(c, v):
    out = dict(v)
    for name in ("pm",) + (("bias",) if c.family == "3d" and c.kinds["bias"] in ("packed", "strided") else ()):
        if name in v and v[name].shape[0] > 0:
            out[name] = np.broadcast_to(v[name][:1], v[name].shape).copy()
    return out


ADDRESS_MUTANTS = {
    "ld taken as cols instead of stride(0)": lambda name, view, a: a._replace(ld=max(_stored_row(view, a)[1], 1)),
    "storage offset dropped": lambda name, view, a: a._replace(offset=0),
    "a transposed view read row-major, ld unchanged": lambda name, view, a: a._replace(op=0),
    "an expanded operand's batch stride taken as packed":
        lambda name, view, a: a._replace(bstride=_stored_row(view, a)[0] * a.ld) if len(view.shape) == 3 and view.shape[0] > 1 and view.strides[0] == 0 else a,
    "a batch of one's rule (no batch stride) applied to a batch of more": lambda name, view, a: a._replace(bstride=0) if name == "a" else a,
}
RULE_MUTANTS = ("beta input lost", "(n,) unscaled as a bias", "grad_w= as a chain started at grad_w",
                "an expanded grad_out read with its strides as given")
MUTANT_NAMES = list(ADDRESS_MUTANTS) + ["a per-matrix bias read as shared", "beta input lost when out is not input",
                                        "(n,) input with beta != 1 added unscaled as a bias", "grad_w= as a chain started at grad_w",
                                        "an expanded grad_out read with its strides as given"]


def _differs(a, b):
    for form in a:
        for x, y in zip(a[form] if isinstance(a[form], tuple) else (a[form],), b[form] if isinstance(b[form], tuple) else (b[form],)):
            if x is not None and not same_bits(np.asarray(x).reshape(-1, 1), np.asarray(y).reshape(-1, 1)):
                return True
    return False


def test_every_wrong_front_end_differs_from_the_true_one_in_some_case(cus, table):
    counts = dict.fromkeys(MUTANT_NAMES, 0)
    for c, v, e in table:
        if c.family == "refuse":
            continue
        for name, change in ADDRESS_MUTANTS.items():
            counts[name] += _differs(F.expected(c, _mutated(c, v, change)), e)
        counts["a per-matrix bias read as shared"] += _differs(F.expected(c, _shared_bias(c, v)), e)
        for name, wrong in zip(MUTANT_NAMES[6:], RULE_MUTANTS):
            counts[name] += _differs(F.expected(c, v, wrong), e)
    for name, n in counts.items():
        print(f"{cus} CUs: {name}: {n} of {N} cases differ")
    assert all(n > 0 for n in counts.values()), counts
    # ... and the true front end, through the same machinery, differs nowhere
    assert not any(_differs(F.expected(c, _mutated(c, v, lambda name, view, a: a)), e) for c, v, e in table[:16] if c.family != "refuse")
