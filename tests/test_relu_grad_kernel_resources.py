"""The kernels of mmh_relu_grad_colsum (csrc/relu_grad.hpp) in the built product library, read on the CPU
(tools/kernel_resources.py): the twelve instantiations of the pass -- {vector, scalar} x {gate, no gate} x {dz + colsum, dz,
colsum} -- and the finish kernel exist under their own names, and none uses scratch or spills a vector or scalar register."""
import re

from built_lib import rows as _rows

PASS = [f"relu_grad_colsum_kernel<{w},{g},{z},{s}>" for w in (4, 1) for g in ("true", "false")
        for z, s in (("true", "true"), ("true", "false"), ("false", "true"))]
# the family patterns the existing coverage and resource tests count
OTHER_FAMILIES = r"sgemm_|igemm_s8_|absmax_kernel|quantize_kernel|dequantize_kernel"


def test_the_kernels_exist_under_their_own_names():
    rows = _rows()
    assert len(PASS) == 12
    missing = [k for k in PASS + ["colsum_finish_kernel"] if k not in rows]
    assert missing == [], missing
    mine = [k for k in rows if "relu_grad" in k or "colsum" in k]
    assert sorted(mine) == sorted(PASS + ["colsum_finish_kernel"]), mine
    for k in mine:
        assert not re.search(OTHER_FAMILIES, k) and not re.search(OTHER_FAMILIES, rows[k]["name"]), k


def test_no_scratch_and_no_spills():
    rows = _rows()
    for k in PASS + ["colsum_finish_kernel"]:
        r = rows[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["threads"] == (64 if k == "colsum_finish_kernel" else 256), r
        assert r["vgpr"] + r["agpr"] <= 256, r      # two workgroups of the pass per CU at the least
