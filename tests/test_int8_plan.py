"""The int8 plan (csrc/igemm_plan.hpp: the mode table and plan_igemm_s8, through mmh_igemm_plan / igemm_plan) against the
independent restatement of the launchers' host arithmetic in tests/int8_ops.py (`reach`), on the CPU: every case of the
exact-reference table and of the graph module, a seeded sweep over shapes, leading dimensions, base residues, modes, entry
points and CU counts, the scratch sizes restated once below, and the modes the build accepts.  What a real call then launches is
held to the plan, character for character, by tests/test_gpu_int8_plan.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import built_lib
import int8_ops
from int8_ops import Case, inplace_ok, reach

pytestmark = [built_lib.needs_library, built_lib.needs_loadable_library()]

CUS = 256
GEMM = re.compile(r"igemm_s8_(?:simple_|dma_|pp_)?kernel<[^>]*>")
PRODUCT_MODES = (0, 2, 5, 6, 7, 8, 9)
QS_BYTES = (4 * 64 + 16) * 4 + 2 * 64 * 4   # abs-max words of A and B, scales, the quantiser's words; the zero block


def plan_of(entry, mode, c, cus, cap=0):
    """igemm_plan with the arguments the call of `c` would have: byte residues of the bases (Case offsets are elements)."""
    import how_to_optimize_gemm_amd as H
    lda, ldb, ldc = c.lds(entry)
    unit = 1 if entry == "igemm" else 4
    return H.igemm_plan(entry, mode, c.m, c.n, c.k, lda, ldb, ldc, unit * c.oa % 16, unit * c.ob % 16, 4 * c.oc % 16, cus, cap)


def scratch_of(entry, mode, c):
    """igemm.hip's sizes restated: mmh_qgemm_f32 keeps int8 images of A (m x ka) and B (k x nb), its words in qs, and the int32
    image m x nb when it is not fused; mmh_igemm_s8 keeps an image only of an operand that mode 0 copies because it is not
    dword-aligned (padded to 16 columns) -- also where the images then lie beyond the descriptors' window and the simple kernel
    reads the operands themselves.  bt: the tools build's."""
    lda, ldb, _ = c.lds(entry)
    m, n, k = c.m, c.n, c.k
    need = dict(qa=0, qb=0, qc=0, qs=0, bt=0)
    if entry == "qgemm":
        ka, nb = (k + 15) & ~15, (n + 3) & ~3
        need.update(qa=m * ka, qb=k * nb, qs=QS_BYTES)
        if not (mode == 0 and inplace_ok(ka, 0, nb, 0, k)):
            need["qc"] = 4 * m * nb
    elif mode == 0 and not inplace_ok(lda, c.oa, ldb, c.ob, k):
        a_ok, b_ok = lda % 4 == 0 and c.oa % 4 == 0, ldb % 4 == 0 and c.ob % 4 == 0
        need.update(qa=0 if a_ok else m * ((k + 15) & ~15), qb=0 if b_ok else k * ((n + 15) & ~15))
    return need


def holds(entry, mode, c, cus, cap=0):
    """The containment the GPU helpers assert on mmh_last_launch, on the plan's text; one GEMM instantiation; the sizes."""
    text, sizes = plan_of(entry, mode, c, cus, cap)
    syms, words = reach(entry, mode, c, cus, cap)
    what = f"{entry} mode {mode} {c} at {cus} CUs, cap {cap}: {text}"
    for w in list(syms) + list(words):
        assert w in text, f"{what}: '{w}' not in the plan's text"
    named = GEMM.findall(text)
    assert len(named) == 1 and named[0] in syms, (what, named)
    assert ("igemm_s8_simple_kernel" in text) == any(s.startswith("igemm_s8_simple_kernel") for s in syms), what
    assert sizes == scratch_of(entry, mode, c), (what, sizes, scratch_of(entry, mode, c))
    # no buffer that the text does not use -- but for the copies mode 0 makes of a misaligned operand whose images then lie
    # beyond the window too (the simple kernel reads the operands; its text says nothing of copies)
    unused = entry == "igemm" and "igemm_s8_simple_kernel" in text
    assert (sizes["qa"] > 0) == (entry == "qgemm" or "A copied to workspace" in text) or unused, what
    assert (sizes["qb"] > 0) == (entry == "qgemm" or "B copied to workspace" in text) or unused, what
    if "copied to workspace" in text:
        assert "igemm_s8_dma_kernel" in text, what
    assert (sizes["qc"] > 0) == ("into int32 workspace, then dequantize_kernel" in text), what
    assert (sizes["qs"] > 0) == text.startswith("qgemm: absmax_kernel + quantize_kernel"), what
    if "dequantised in the epilogue" in text:
        assert sizes["qc"] == 0, what
    return text, sizes


def _table_cases():
    import test_gpu_int8_parity as T
    out = []
    for inst in T.INSTANTIATIONS:
        for c in inst.cases(CUS) + ([inst.worst(CUS)] if inst.worst else []):
            entry = c.entry or inst.entry
            if entry != "quantize":
                out.append((entry, inst.mode if c.mode is None else c.mode, c, 0, inst.symbol))
        if inst.persistent:
            out += [(inst.entry, inst.mode, c, T.GRID_CAP, inst.symbol) for c in T._persistent_cases(inst, CUS)]
    return out


def test_every_case_of_the_exact_reference_table_is_planned_as_reach_says():
    cases = _table_cases()
    assert len(cases) > 150
    for entry, mode, c, cap, symbol in cases:
        text, _ = holds(entry, mode, c, CUS, cap)
        assert symbol in text, (symbol, c, text)
        if cap:
            assert "persistent: 8 workgroups walk" in text, (c, text)


def test_every_case_of_the_graph_module_is_planned_as_reach_says():
    import test_gpu_int8_graph as G
    s = int8_ops._big_side(CUS)
    cases = [("qgemm", 0, G.RAGGED), ("qgemm", 5, G.MID), ("qgemm", 5, Case(4096, 3, 8, ldb=4)), ("igemm", 8, Case(300, 700, 1000)),
             ("igemm", 8, Case(512, 256, 129, lda=132)), ("igemm", 5, Case(131, 133, 257, lda=260, ldb=136, ldc=134, oc=1)),
             ("igemm", 0, G.MISALIGNED_LARGE), ("qgemm", 0, G.THIN_K), ("qgemm", 5, G.THIN_K), ("qgemm", 5, G.DEEP), ("qgemm", 0, G.COLUMN),
             ("qgemm", 0, G.MID), ("qgemm", 0, Case(s, s, 272)), ("qgemm", 5, G.RAGGED), ("qgemm", 5, Case(1, 1, 1)),
             ("qgemm", 0, Case(1283, 1027, 129, lda=132, ldb=1028))]
    cases += [("igemm", 0, c) for c in G.MISALIGNED]
    for k in (64, 129):
        cases += [("qgemm", 0, Case(s - 5, s + 3, k, ldc=s + 4, oc=1)), ("qgemm", 0, Case(s, s, k))]
    # every shape the module names, through both entry points in the modes the module uses (so that a shape added there is
    # planned here); the (entry, mode, shape) triples above are the calls its tests make
    named = [v for v in vars(G).values() if isinstance(v, Case)]
    named += [c for v in vars(G).values() if isinstance(v, tuple) for c in v if isinstance(c, Case)]
    assert len(named) >= 9 and all(any(c == x for _, _, x in cases) for c in named), named
    cases += [(entry, mode, c) for c in named for entry in ("igemm", "qgemm") for mode in (0, 5, 8)]
    for entry, mode, c in cases:
        holds(entry, mode, c, CUS)


def test_the_persistent_launch_form_changes_between_k_5120_and_5121():
    """Mode 0 runs K3p persistent up to k = 5120 and one workgroup per tile beyond; with more tiles than CUs the text shows it:
    mmh_igemm_s8 and the fused mmh_qgemm_f32 on 8 x 8 tiles at 4 CUs and on 32 x 32 (the last ones ragged) at 256."""
    for cus, c in ((4, Case(2048, 2048, 0)), (256, Case(8192, 8189, 0, ldb=8192, ldc=8192))):
        for entry in ("igemm", "qgemm"):
            for k in (5119, 5120, 5121):
                ck = Case(c.m, c.n, k, lda=k + 3 if entry == "qgemm" else k + (-k % 4), ldb=c.ldb, ldc=c.ldc)
                text, _ = holds(entry, 0, ck, cus)
                assert "igemm_s8_pp_kernel" in text and ("persistent: " in text) == (k <= 5120), (entry, ck, text)
                assert (f"persistent: {cus} workgroups walk" in text) == (k <= 5120), (entry, ck, text)


def test_a_seeded_sweep_is_planned_as_reach_says():
    """Shapes around the tiles' and slices' sizes; at most one dimension of a draw is large, and the large values carry an
    operand across the descriptors' 2 GiB window (256 * lda + k, (k + 256) * ldb + 256) while the tile counts stay in an int."""
    rng = np.random.default_rng(20261019)
    small = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4096, 8192]
    deep = [5119, 5120, 5121]   # k only: either side of where mode 0's K3p stops being persistent
    large = [(1 << 19) + 5, 1 << 23, (1 << 23) + 4, 1 << 24]
    seen, beyond, draws = set(), 0, 4000
    for _ in range(draws):
        dims = [int(rng.choice(small)) for _ in range(3)]
        if rng.random() < 0.15:
            dims[int(rng.integers(3))] = int(rng.choice(large))
        if rng.random() < 0.1:
            dims[2] = int(rng.choice(deep))
        m, n, k = dims
        pad = [int(rng.choice([0, 1, 3, 4, 16])) for _ in range(3)]
        res = [int(rng.choice([0, 1, 2, 3, 4, 8])) for _ in range(3)]
        entry = ("igemm", "qgemm")[int(rng.integers(2))]
        mode = int(rng.choice(PRODUCT_MODES))
        cus = int(rng.choice([1, 8, 256, 304]))
        cap = int(rng.choice([0, 0, 0, 3, 8]))
        c = Case(m, n, k, lda=k + pad[0], ldb=n + pad[1], ldc=n + pad[2], oa=res[0], ob=res[1], oc=res[2] % 4)
        text, _ = holds(entry, mode, c, cus, cap)
        seen.add((entry, mode, GEMM.findall(text)[0].split("<")[0], "copied" in text, "persistent" in text))
        lda, ldb, _ = c.lds(entry)
        beyond += 256 * lda + k >= (1 << 31) - 4096 or (k + 256) * ldb + 256 >= (1 << 31) - 4096
    kinds = {(e, mo, fam) for e, mo, fam, _, _ in seen}
    for mode in PRODUCT_MODES:
        assert ("igemm", mode, "igemm_s8_simple_kernel") in kinds and ("qgemm", mode, "igemm_s8_simple_kernel") in kinds, mode
    assert {("igemm", 0, "igemm_s8_pp_kernel"), ("igemm", 0, "igemm_s8_dma_kernel"), ("qgemm", 0, "igemm_s8_pp_kernel"),
            ("qgemm", 0, "igemm_s8_dma_kernel"), ("igemm", 7, "igemm_s8_pp_kernel"), ("qgemm", 6, "igemm_s8_dma_kernel")} <= kinds
    assert any(copied for _, _, _, copied, _ in seen) and any(walks for _, _, _, _, walks in seen)
    assert beyond > 20, f"{beyond} aligned operands beyond the window in {draws} draws"


def test_the_product_plans_exactly_the_product_modes():
    import how_to_optimize_gemm_amd as H
    for mode in range(-1, 15):
        if mode in PRODUCT_MODES:
            assert GEMM.search(H.igemm_plan("igemm", mode, 256, 256, 64)[0]), mode
            assert H.igemm_plan("qgemm", mode, 256, 256, 64)[1]["bt"] == 0, mode
        else:
            for entry in ("igemm", "qgemm"):
                with pytest.raises(H.MMultError) as e:
                    H.igemm_plan(entry, mode, 256, 256, 64)
                assert e.value.status == H.ERR_INVALID_ARG, mode


def test_the_tools_library_plans_modes_0_to_13_where_it_is_built():
    """(loaded beside the product library, for this one host function; nothing builds it here)"""
    import how_to_optimize_gemm_amd as H
    if not os.path.exists(H.AB_LIB_PATH):
        pytest.skip("libmmult_hip_ab.so has not been built")
    ab = C.CDLL(H.AB_LIB_PATH)
    ab.mmh_igemm_plan.argtypes = [C.c_int] * 13 + [C.c_char_p, C.c_int, C.POINTER(C.c_size_t)]
    text, sizes = C.create_string_buffer(256), (C.c_size_t * 5)()

    def plan(mode, m=256, n=256, k=64, lda=64):
        return ab.mmh_igemm_plan(0, mode, m, n, k, lda, n, n, 0, 0, 0, CUS, 0, text, len(text), sizes)

    for mode in range(-1, 15):
        assert plan(mode) == (H.OK if 0 <= mode <= 13 else H.ERR_INVALID_ARG), mode
    # the tools build's rungs leave no launch marker; bt is stated for the packed-B modes whatever the operands then allow
    for mode in (3, 4, 10, 11, 12, 13):
        assert plan(mode) == H.OK and text.value == b"" and sizes[4] == 256 * 256, mode
    assert plan(3, 130, 100, 300, 304) == H.OK and text.value == b"" and sizes[4] == 128 * 512
    assert plan(1) == H.OK and text.value == b"" and sizes[4] == 0
    assert plan(3, lda=67) == H.OK and b"igemm_s8_simple_kernel<true>" in text.value and sizes[4] == 256 * 256   # A: no dword rows
    assert plan(5) == H.OK and b"igemm_s8_dma_kernel<128,128,4,false,0,true>" in text.value and sizes[4] == 0
