"""What an int8 call launches is what its plan says.  After a real mmh_igemm_s8 / mmh_qgemm_f32 call, mmh_last_launch equals
igemm_plan's text for that call's arguments character for character (tests/test_int8_plan.py holds the plan to `reach` on the
CPU), on the smallest shape of every plan kind; and the handle's scratch grows by what the plan states: on a fresh handle the
same call into a capturing stream is refused, with nothing recorded, exactly when one of the plan's sizes is not zero (a handle
without scratch cannot allocate under capture), and is otherwise recorded and replays exactly."""
import numpy as np
import pytest

from test_gpu_int8_graph import _Igemm, _Qgemm, _capture, _captured_nodes, _eager, _replays, _side_stream   # (that module's ops and capture helpers)
from int8_ops import Case, _cus

pytestmark = pytest.mark.gpu

KINDS = [
    ("simple, whole", "igemm", 2, Case(128, 128, 64), "igemm_s8_simple_kernel<false>"),
    ("simple, guarded", "igemm", 2, Case(129, 127, 65), "igemm_s8_simple_kernel<true>"),
    ("K3t 128", "igemm", 5, Case(128, 128, 64), "igemm_s8_dma_kernel<128,128,4,false,0,true>"),
    ("K3t 256", "igemm", 6, Case(256, 256, 64), "igemm_s8_dma_kernel<256,256,8,false,0,true>"),
    ("K3p persistent", "igemm", 8, Case(256, 256, 64), "igemm_s8_pp_kernel<false,false,64>"),
    ("K3p per tile", "igemm", 9, Case(256, 256, 64), "igemm_s8_pp_kernel<false,false,64>"),
    ("K3p on the 32-deep MFMA", "igemm", 7, Case(256, 256, 64), "igemm_s8_pp_kernel<false,false,32>"),
    ("copied operand", "igemm", 0, Case(128, 128, 65, lda=67), "A copied to workspace"),
    ("qgemm fused", "qgemm", 0, Case(128, 128, 64), "dequantised in the epilogue"),
    ("qgemm two-pass", "qgemm", 2, Case(128, 128, 64), "dequantize_kernel (two-pass)"),
]


def _plan(op):
    import how_to_optimize_gemm_amd as H
    c = op.c
    lda, ldb, ldc = c.lds(op.entry)
    return H.igemm_plan(op.entry, op.mode, c.m, c.n, c.k, lda, ldb, ldc, op.av.data_ptr() % 16, op.bv.data_ptr() % 16,
                        op.cv.data_ptr() % 16, _cus(), 0)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k[0])
def test_a_call_launches_its_plan_and_grows_the_scratch_the_plan_states(mm, kind):
    import torch
    import how_to_optimize_gemm_amd as H
    _, entry, mode, c, word = kind
    op = (_Igemm if entry == "igemm" else _Qgemm)(c, mode)
    text, sizes = _plan(op)
    assert word in text, text
    rng = np.random.default_rng(len(text))
    side = _side_stream()
    # an eager call (on the session's handle): the marker is the plan's text
    op.fill(rng)
    with torch.cuda.stream(side):
        op.call(mm)
        launched = H.last_launch()
    side.synchronize()
    op.check("eager")
    assert launched == text
    # a fresh handle, capturing: refused exactly when the plan needs scratch
    with H.MMult(0, "auto") as own:
        op.fill(rng)
        mark = torch.zeros(4, device="cuda")
        seen = []

        def body():
            mark.fill_(1.0)   # (so that the graph is never empty)
            seen.append(_captured_nodes(side))
            if any(sizes.values()):
                with pytest.raises(H.MMultError) as e:
                    op.call(own)
                assert e.value.status == H.ERR_UNSUPPORTED
                del e   # (tests/test_gpu_int8_graph.py _capture: no dead cycle may hold this capture's graph)
            else:
                op.call(own)
            seen.append(_captured_nodes(side))

        graph = _capture(side, body)
        if any(sizes.values()):
            assert seen[1] == seen[0], f"the refused call recorded {seen[1] - seen[0]} nodes"
            graph.replay()
            torch.cuda.synchronize()
            assert op.untouched()
            _eager(own, side, [op], rng, "uncaptured after the refusal")
            assert H.last_launch() == text
        else:
            assert seen[1] > seen[0]
            _replays(graph, [op], rng, 1)
        assert own.get_option(H.OPT_RETIRED_BUFFERS) == 0
        del graph


def test_set_option_and_the_plan_accept_the_same_modes(mm):
    import how_to_optimize_gemm_amd as H
    try:
        for mode in range(-1, 15):
            planned = True
            try:
                H.igemm_plan("igemm", mode, 256, 256, 64)
            except H.MMultError:
                planned = False
            taken = H.lib().mmh_set_option(mm._h, H.OPT_IGEMM_MODE, mode) == H.OK
            assert planned == taken == (mode in (0, 2, 5, 6, 7, 8, 9)), mode
    finally:
        mm.set_igemm_mode(0)
