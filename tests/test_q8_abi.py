"""CPU tests of the second product library's boundary: build_all builds libmmult_hip_q8.so, the library exports exactly what
include/mmult_hip_q8.h declares, every prototype binds from the parsed header, mmh_q8_linear_plan is the Python restatement
(tests/qlinear_ref.py, plan_text) over a grid of shapes, and argument errors are refused before any device call."""
import ctypes as C
import itertools
import os
import threading

import pytest

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, build, q8
import qlinear_ref as R
from built_lib import dynamic_exports
from conftest import REPO


def test_build_all_builds_the_library_after_the_product_library(monkeypatch):
    assert os.path.exists(build.Q8_LIB), "libmmult_hip_q8.so has not been built: build_all() builds it"
    assert build.Q8_LIB == q8.LIB_PATH == os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q8.so")
    calls = []
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=False: calls.append("product"))
    monkeypatch.setattr(build, "build_q8_library", lambda force=False, verbose=False: calls.append("q8"))
    monkeypatch.setattr(build, "build_harness", lambda force=False: calls.append("harness"))
    build.build_all()
    assert calls[:2] == ["product", "q8"], calls


def test_the_library_exports_exactly_the_headers_prototypes():
    constants, prototypes = abi_header.parse(q8.HEADER)
    assert constants == {} and list(prototypes) == q8.EXPORTS and len(q8.EXPORTS) >= 10
    assert dynamic_exports(q8.LIB_PATH) == sorted(q8.EXPORTS)
    # ... and the first library's header and exports are as they were: nothing of this one is declared there
    assert not [n for n in H.EXPORTS if "q8" in n] and abi_header.PROTOTYPES is not prototypes
    assert abi_header.parse(abi_header.HEADER) == (abi_header.CONSTANTS, abi_header.PROTOTYPES)


def test_every_prototype_binds():
    L = q8.lib()
    for name, (restype, argtypes) in q8.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    _I, _P, _S = C.c_int, C.c_void_p, C.c_char_p
    assert q8.PROTOTYPES["mmh_q8_weight_info"] == (_I, [_P] * 7)                              # mmh_q8_weight_t, int *, const int8_t **
    assert q8.PROTOTYPES["mmh_q8_weight_create"] == (_I, [_P, _I, _I, _I, _P, _I, _P])        # mmh_q8_weight_t *
    assert q8.PROTOTYPES["mmh_q8_linear_plan"] == (_I, [_I] * 10 + [_S, _I, _P])
    assert q8.PROTOTYPES["mmh_q8_last_launch"] == (_S, [])
    # (the launch text is per thread: a thread that has launched nothing reads "", whatever this one ran before)
    fresh = []
    reader = threading.Thread(target=lambda: fresh.append(L.mmh_q8_last_launch()))
    reader.start()
    reader.join()
    assert fresh == [b""] and b"gfx950" in open(q8.LIB_PATH, "rb").read()


ROWS = (1, 5, 128, 129, 512, 2048, 2560, 4096)
OUTS = (1, 3, 128, 130, 2048, 3328, 4096, 11008)
INS = (0, 1, 7, 64, 1023, 1024, 4096)


@pytest.mark.parametrize("cus", [256, 64])
def test_the_plan_is_the_python_restatement(cus):
    seen = set()
    for rows, out, in_ in itertools.product(ROWS, OUTS, INS):
        for (ldx, ldy, x16, y16), (bias, act) in itertools.product(((0, 0, 0, 0), (in_ + 4, out + 4, 0, 0), (in_ + 3, out + 1, 4, 0), (0, 0, 0, 8)),
                                                                    ((False, None), (True, None), (False, "relu"), (True, "relu"))):
            want = R.plan_text(rows, out, in_, ldx, ldy, x16, y16, bias, act == "relu", cus)
            assert q8.qlinear_plan(rows, out, in_, ldx, ldy, x16, y16, bias, act, cus) == want, (rows, out, in_, ldx, ldy, x16, y16)
            seen.add(want[0].split("then ")[1].split(">")[0])
    assert len(seen) == 16, sorted(seen)   # the grid reaches every instantiation of the GEMM
    assert q8.qlinear_plan(4096, 4096, 4096, cu_count=0) == q8.qlinear_plan(4096, 4096, 4096, cu_count=256)


def test_argument_errors_are_refused_without_a_device():
    L, INV = q8.lib(), H.ERR_INVALID_ARG
    h, x = C.c_void_p(), 4096   # (a non-NULL address that is never read)
    # mmh_q8_weight_create: NULL out-pointer, negative device / sizes, out == 0, ldw < in, NULL dW
    assert L.mmh_q8_weight_create(None, 0, 4, 4, x, 4, None) == INV
    for device, out, in_, dw, ldw in ((-1, 4, 4, x, 4), (0, 0, 4, x, 4), (0, -1, 4, x, 4), (0, 4, -1, x, 4), (0, 4, 4, x, 3), (0, 4, 4, None, 4)):
        assert L.mmh_q8_weight_create(C.byref(h), device, out, in_, dw, ldw, None) == INV and not h.value
    assert L.mmh_q8_weight_destroy(None) == H.OK
    assert L.mmh_q8_weight_info(None, None, None, None, None, None, None) == INV
    # mmh_q8_quantize_rows: negative sizes, NULL operands, ldx / ldq below the row length; rows == 0 is MMH_OK
    ok = (0, 2, 8, x, 8, x, 8, x, x, None)
    assert L.mmh_q8_quantize_rows(0, 0, 8, None, 0, None, 0, None, None, None) == H.OK
    for i, bad in ((0, -1), (1, -1), (2, -1), (3, None), (4, 7), (5, None), (6, 7), (7, None), (8, None)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q8_quantize_rows(*args) == INV, (i, bad)
    # the calls on an object: a NULL object
    y = C.c_float(0)
    assert L.mmh_q8_linear(None, 1, x, 4, None, H.ACT_NONE, x, 4, None) == INV
    assert L.mmh_q8_linear_reserve(None, 1, None) == INV
    assert L.mmh_time_q8_linear(None, 1, x, 4, None, H.ACT_NONE, x, 4, 1, 1, None, C.byref(y)) == INV
    # mmh_q8_linear_plan: the entry points' own rules
    text, scratch = C.create_string_buffer(256), C.c_size_t(0)
    good = [8, 8, 8, 8, 8, 0, 0, 0, H.ACT_NONE, 256, text, 256, C.byref(scratch)]
    assert L.mmh_q8_linear_plan(*good) == H.OK
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, -1), (3, 7), (4, 7), (5, 16), (6, -1), (8, 2), (8, -1), (10, None), (11, 0), (12, None)):
        args = list(good)
        args[i] = bad
        assert L.mmh_q8_linear_plan(*args) == INV, (i, bad)
    assert L.mmh_q8_linear_plan(8, 65536, 40000, 40000, 65536, 0, 0, 0, 0, 256, text, 256, C.byref(scratch)) == H.ERR_UNSUPPORTED   # beyond the window
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_plan(8, 8, 8, activation="gelu")
    assert e.value.status == INV


def test_a_device_that_is_not_there_fails_loudly():
    h, n = C.c_void_p(), H.device_count()
    assert q8.lib().mmh_q8_weight_create(C.byref(h), n, 4, 4, 4096, 4, None) == H.ERR_NO_DEVICE and not h.value
    assert b"no such device" in q8.lib().mmh_q8_last_error()
