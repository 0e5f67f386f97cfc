"""A census of libmmult_hip.so: every kernel in its code objects (tools/kernel_resources.py) is claimed by exactly one entry of
CENSUS -- one of the eight per-instantiation tables, which must then hold a row for it, or the GPU test that runs a kernel that
has no table (the naive kernels, the ReLU-gate / column-sum pair, the peak probes).  A new kernel family that ships without an
entry fails here by name, on the CPU; so does an entry that matches no kernel of the library any more."""
import importlib
import inspect
import os
import re

import built_lib
from built_lib import LIB, REPO

pytestmark = built_lib.needs_library

ANONYMOUS = "_ZN3mmh12_GLOBAL__N_1"   # a kernel of an unnamed namespace inside mmh: kernel_resources reads no further than this


def symbol_of(row):
    """kernel_resources' demangled head; for a kernel in an unnamed namespace its identifier with the template arguments as
    they stand in the mangled name (probe_lds_read_kernel<16>, probe_valu_kernel<true>; n8 = -8).  Only integer and bool
    template arguments are read, as in kernel_resources; a name with anything else comes back mangled, whole, so that it is
    the real symbol that fails as unclaimed."""
    name = row["name"]
    if not name.startswith(ANONYMOUS):
        return row["kernel"]
    rest = name[len(ANONYMOUS):]
    digits = re.match(r"\d+", rest)
    if not digits:
        return name
    digits = digits[0]
    ident, rest = rest[len(digits):len(digits) + int(digits)], rest[len(digits) + int(digits):]
    if rest.startswith("E") and not rest.startswith("EE"):      # no template arguments: E, then the parameter types
        return ident
    g = re.fullmatch(r"I((?:L[ib]n?\d+E)+)EEv.+", rest)         # I <Li..E | Lb..E>+ E, E, the void return type, the parameter types
    if not g:
        return name
    args = [(tok[2:] if tok[1] == "i" else ("true" if tok[2:] == "1" else "false")) for tok in re.findall(r"L[ib]n?\d+", g[1])]
    return f"{ident}<{','.join(args)}>"


def table(pattern, module, name):
    return {"pattern": re.compile(pattern), "table": (module, name)}


def single(pattern, test, mentions):
    """A kernel (or the instantiations of one template) without a table: the GPU test that runs it, and a word of that test's
    module that shows it -- the kernel id, the launch marker or the entry point."""
    return {"pattern": re.compile(pattern), "test": test, "mentions": mentions}


CENSUS = [
    # ---- the eight tables: one row per instantiation, the row's shapes proved to reach it, bit for bit against the oracle
    # (split-K: against the restatement of its own contract, tests/splitk_ref.py, which is built from the oracle's chains)
    table(r"^(sgemm_mfma_dma_kernel|sgemm_dma_streamk_kernel|sgemm_mfma_dma5_kernel|sgemm_dma5_streamk_kernel|sgemm_valu_dma5_kernel|"
          r"sgemm_valu_dma5_streamk_kernel|sgemm_mfma_dma5_op_kernel|sgemm_dma5_op_streamk_kernel)<", "test_gpu_lds_dma_parity", "INSTANTIATIONS"),
    table(r"^(igemm_s8_simple_kernel|igemm_s8_dma_kernel|igemm_s8_pp_kernel)<|^(absmax_kernel|quantize_kernel|dequantize_kernel)$",
          "test_gpu_int8_parity", "INSTANTIATIONS"),
    table(r"^sgemm_(mfma_dma5_ex|dma5_ex_streamk)_kernel<", "test_gpu_ex_parity", "EX_INSTANTIATIONS"),
    table(r"^sgemm_mfma_dma5_batched_ex_kernel<", "test_gpu_batched_ex", "BATCHED_EX_INSTANTIATIONS"),
    table(r"^(sgemm_mfma_kernel|sgemm_mfma_streamk_kernel|sgemm_mfma_simple_kernel)<", "test_gpu_reg_parity", "REG_INSTANTIATIONS"),
    table(r"^sgemm_mfma_splitk_kernel<", "test_gpu_splitk_parity", "SPLITK_INSTANTIATIONS"),
    table(r"^sgemm_mfma_dma5_batched_kernel<", "test_gpu_batched_parity", "BATCHED_INSTANTIATIONS"),
    table(r"^sgemm_valu_kernel<", "test_gpu_k1_parity", "K1_INSTANTIATIONS"),
    # ---- the naive kernels: the bottom rung, and the independent on-device reference of the fuzzers
    single(r"^sgemm_naive_kernel$", "tests/test_gpu_parity.py::test_golden_fixtures_device_flavour", '"naive"'),
    single(r"^sgemm_naive_op_kernel$", "tests/test_gpu_op.py::test_op_form_fuzz_against_the_naive_op_kernel", "sgemm_naive_op_kernel"),
    single(r"^sgemm_naive_ex_kernel$", "tests/test_gpu_ex_parity.py::test_special_values_follow_the_epilogue_contract", "sgemm_naive_ex_kernel"),
    single(r"^sgemm_naive_batched_kernel$", "tests/test_gpu_batched.py::test_every_matrix_is_the_fused_chain", "sgemm_naive_batched_kernel"),
    single(r"^sgemm_naive_batched_ex_kernel$", "tests/test_gpu_batched_ex.py::test_strides_broadcasts_and_shared_biases",
           "sgemm_naive_batched_ex_kernel"),
    # ---- the linear layer's backward: every mode (the three template flags) on the vector and the scalar path, and the finish
    single(r"^relu_grad_colsum_kernel<[14],(true|false),(true|false),(true|false)>$",
           "tests/test_gpu_relu_grad.py::test_every_mode_and_layout_is_bit_equal_to_the_contract", "relu_grad_colsum_kernel (%s path)"),
    single(r"^colsum_finish_kernel$", "tests/test_gpu_relu_grad.py::test_every_mode_and_layout_is_bit_equal_to_the_contract", "colsum {nblocks} block"),
    # ---- the peak probes
    single(r"^probe_mfma_kernel$", "tests/test_gpu_parity.py::test_peak_probes_are_sane", "probe_mfma_f32("),
    single(r"^probe_copy_kernel$", "tests/test_gpu_parity.py::test_peak_probes_are_sane", "probe_hbm_copy("),
    single(r"^probe_read_kernel$", "tests/test_gpu_parity.py::test_entry_points_restore_the_callers_device", "probe_hbm_read("),
    single(r"^probe_lds_read_kernel<(16|8|n8|4)>$", "tests/test_gpu_parity.py::test_lds_probe_reads_a_plausible_rate", "probe_lds_read("),
    single(r"^probe_valu_kernel<(true|false)>$", "tests/test_gpu_probes.py::test_the_vector_alu_probes_read_a_rate_under_their_roofs",
           "probe_valu_f32("),
    single(r"^probe_mfma_i8(_random)?_kernel$", "tests/test_gpu_probes.py::test_the_int8_mfma_probes_read_a_rate_under_their_roof",
           "probe_mfma_i8_sustained("),
]


def _symbols(lib=LIB):
    return sorted({symbol_of(r) for r in built_lib.resources(lib)})


def census(symbols):
    """(symbols no entry claims, symbols more than one entry claims, entries that claim nothing, entry index by symbol)"""
    by = {s: [i for i, e in enumerate(CENSUS) if e["pattern"].search(s)] for s in symbols}
    unclaimed = sorted(s for s, hits in by.items() if not hits)
    twice = sorted(s for s, hits in by.items() if len(hits) > 1)
    idle = [CENSUS[i]["pattern"].pattern for i in range(len(CENSUS)) if not any(i in hits for hits in by.values())]
    return unclaimed, twice, idle, {s: hits[0] for s, hits in by.items() if len(hits) == 1}


def test_every_kernel_of_the_library_is_claimed_by_exactly_one_entry():
    symbols = _symbols()
    assert len(symbols) > 200 and not any(s.startswith("_") for s in symbols), [s for s in symbols if s.startswith("_")]
    unclaimed, twice, idle, _ = census(symbols)
    assert not unclaimed, f"kernels in libmmult_hip.so that no table and no test of tests/test_kernel_census.py::CENSUS claims: {unclaimed}"
    assert not twice, f"kernels that two entries of CENSUS claim: {twice}"
    assert not idle, f"entries of CENSUS that match no kernel of libmmult_hip.so: {idle}"


def test_a_kernel_without_an_entry_fails_by_name():
    """The census on the library's symbols plus one that nothing claims, and minus a family."""
    symbols = _symbols()
    unclaimed, _, _, _ = census(symbols + ["sgemm_grouped_kernel<64,64,32,false>"])
    assert unclaimed == ["sgemm_grouped_kernel<64,64,32,false>"]
    _, _, idle, _ = census([s for s in symbols if not s.startswith("sgemm_valu_kernel<")])
    assert idle == [r"^sgemm_valu_kernel<"]


def test_a_table_entry_holds_a_row_for_each_of_its_kernels():
    _, _, _, entry_of = census(_symbols())
    eight = [e for e in CENSUS if "table" in e]
    assert len(eight) == 8 and len({e["table"] for e in eight}) == 8
    rows = {}
    for e in eight:
        module, name = e["table"]
        assert os.path.exists(os.path.join(REPO, "tests", module + ".py")), module
        rows[e["table"]] = {r.symbol for r in getattr(importlib.import_module(module), name)}
    missing = sorted(s for s, i in entry_of.items() if "table" in CENSUS[i] and s not in rows[CENSUS[i]["table"]])
    assert not missing, f"kernels whose table holds no row for them: {missing}"
    # ... and the tables hold nothing of another entry's: 30 rows in the three newest
    assert len(rows[("test_gpu_batched_parity", "BATCHED_INSTANTIATIONS")]) == 24 and len(rows[("test_gpu_k1_parity", "K1_INSTANTIATIONS")]) == 4
    assert len(rows[("test_gpu_splitk_parity", "SPLITK_INSTANTIATIONS")]) == 2


def test_a_single_entry_names_a_gpu_test_that_runs_its_kernel():
    for e in CENSUS:
        if "test" not in e:
            continue
        path, name = e["test"].split("::")
        assert os.path.exists(os.path.join(REPO, path)), e["test"]
        module = importlib.import_module(os.path.splitext(os.path.basename(path))[0])
        test = getattr(module, name, None)
        assert callable(test), e["test"]
        marks = getattr(module, "pytestmark", [])
        marks = list(marks) if isinstance(marks, (list, tuple)) else [marks]
        marks += list(getattr(test, "pytestmark", []))
        assert any(getattr(m, "name", None) == "gpu" or getattr(getattr(m, "mark", None), "name", None) == "gpu" for m in marks), \
            (e["test"], "is not marked gpu")
        assert e["mentions"] in inspect.getsource(module), (e["test"], e["mentions"])
