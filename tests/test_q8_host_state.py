"""CPU test of the state the three int8 layer libraries keep: their host sides share one header (csrc_q8/q8_host.hpp), but each
.so has its own per-thread error and launch texts -- a refusal in one library never shows in another's mmh_*_last_error, and a
thread that has called nothing reads "" from all of them."""
import ctypes as C
import threading

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, q8


def in_fresh_thread(fn):
    """fn()'s result, run on a thread of its own (an exception there is raised here)."""
    box = []

    def run():
        try:
            box.append((fn(), None))
        except BaseException as e:   # noqa: BLE001 -- handed to the caller's thread
            box.append((None, e))

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box[0][1] is not None:
        raise box[0][1]
    return box[0][0]


def test_each_library_keeps_its_own_error_text():
    def refusals():
        L8, Lo, Ld = q8.lib(), q8.lib_q8o(), q8.lib_q8d()
        assert (L8.mmh_q8_last_error(), Lo.mmh_q8o_last_error(), Ld.mmh_q8d_last_error()) == (b"", b"", b"")
        # the int8-output library refuses rows of pitch 130 (no multiple of 4) before any device call, with a message
        text, work = C.create_string_buffer(192), C.c_size_t(0)
        assert Lo.mmh_q8o_linear_plan(8, 8, 129, 130, 16, 8, 0, 0, 0, 256, text, 128) == H.ERR_UNSUPPORTED
        q8o_text = (b"mmh_q8o_linear_plan: the tile reads the int8 rows and the weight image in dwords -- their pitches and base "
                    b"addresses must be multiples of 4")
        assert Lo.mmh_q8o_last_error() == q8o_text
        assert L8.mmh_q8_last_error() == b"" and Ld.mmh_q8d_last_error() == b""
        # ... and the small-batch library 17 rows: its text is its own, the others are as they were
        assert Ld.mmh_q8d_linear_plan(17, 8, 256, 256, 16, 0, 8, 0, 0, 0, 0, 256, text, 192, C.byref(work)) == H.ERR_UNSUPPORTED
        assert Ld.mmh_q8d_last_error() == b"mmh_q8d_linear_plan: at most 16 rows (MMH_Q8D_MAX_ROWS) -- larger batches are the tile path's"
        assert L8.mmh_q8_last_error() == b"" and Lo.mmh_q8o_last_error() == q8o_text
        return True

    assert in_fresh_thread(refusals)

    def every_text():
        out = {}
        for header, lib in ((q8.HEADER, q8.lib), (q8.Q8O_HEADER, q8.lib_q8o), (q8.Q8D_HEADER, q8.lib_q8d)):
            for name in abi_header.parse(header)[1]:
                if "_last_" in name:
                    out[name] = getattr(lib(), name)()
        return out

    texts = in_fresh_thread(every_text)
    assert len(texts) >= 5 and {n.split("_last_")[0] for n in texts} == {"mmh_q8", "mmh_q8o", "mmh_q8d"}, texts
    assert set(texts.values()) == {b""}, texts
