"""CPU tests of the third product library's boundary: build_all builds libmmult_hip_q8o.so after the second library, it
exports exactly what include/mmult_hip_q8o.h declares, every prototype binds from the parsed header, mmh_q8o_linear_plan is the
Python restatement (tests/qchain_ref.py, plan_text_s8o) over a grid that reaches all four instantiations, argument errors and
operands the tile cannot read are refused before any device call -- and mmh_q8_linear_s8 is among the second library's exports."""
import ctypes as C
import itertools
import os
import threading

import pytest

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, build, q8
import qchain_ref as Q
from built_lib import dynamic_exports
from conftest import REPO


def test_build_all_builds_the_library_after_the_second_library(monkeypatch):
    assert os.path.exists(build.Q8O_LIB), "libmmult_hip_q8o.so has not been built: build_all() builds it"
    assert build.Q8O_LIB == q8.Q8O_LIB_PATH == os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q8o.so")
    calls = []
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=False: calls.append("product"))
    monkeypatch.setattr(build, "build_q8_library", lambda force=False, verbose=False: calls.append("q8"))
    monkeypatch.setattr(build, "build_q8o_library", lambda force=False, verbose=False: calls.append("q8o"))
    monkeypatch.setattr(build, "build_harness", lambda force=False: calls.append("harness"))
    build.build_all()
    assert calls == ["product", "q8", "q8o", "harness"], calls


def test_the_recipe_is_the_second_librarys_with_its_own_directory(monkeypatch):
    """build_q8o_library's compile lines: the q8 library's flags, -I csrc_q8o -I csrc_q8 -I csrc, objects under build/q8o/, at
    most 16 jobs at a time, its own version script on the link line."""
    import concurrent.futures
    lines, workers = [], []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: lines.append(cmd))
    real = concurrent.futures.ThreadPoolExecutor

    def pool(max_workers=None):
        workers.append(max_workers)
        return real(max_workers=max_workers)

    monkeypatch.setattr(concurrent.futures, "ThreadPoolExecutor", pool)
    monkeypatch.setattr(build.os, "cpu_count", lambda: 192)
    build.build_q8o_library(force=True)
    compiles, link = lines[:-1], lines[-1]
    assert len(compiles) == 5 and workers == [5] and max(workers) <= 16
    for cmd in compiles:
        inc = [a for a in cmd if a.startswith("-I")]
        assert inc == ["-I" + build.CSRC_Q8O, "-I" + build.CSRC_Q8, "-I" + build.CSRC], cmd
        assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and "-fPIC" in cmd
        assert os.path.dirname(cmd[cmd.index("-o") + 1]) == os.path.join(build.PKG_DIR, "build", "q8o")
    assert "-shared" in link and link[link.index("-o") + 1] == build.Q8O_LIB
    assert "-Wl,--version-script=" + os.path.join(build.CSRC_Q8O, "exports_q8o.map") in link
    assert not [a for a in link if "libmmult_hip" in a and a != build.Q8O_LIB], "links nothing of the other libraries"
    # the one recipe caps every library's pool: the second library's five units, 16 of the first library's more than 16
    del workers[:]
    build.build_q8_library(force=True)
    build.build_library(force=True)
    assert len(build.translation_units()) > 16 and workers == [5, 16] and max(workers) <= 16


def test_the_library_exports_exactly_the_headers_prototypes():
    constants, prototypes = abi_header.parse(q8.Q8O_HEADER)
    assert constants == {} and sorted(prototypes) == ["mmh_q8o_last_error", "mmh_q8o_last_launch", "mmh_q8o_linear", "mmh_q8o_linear_plan",
                                                      "mmh_time_q8o_linear"]
    assert dynamic_exports(q8.Q8O_LIB_PATH) == sorted(prototypes)
    # ... the second library gained one entry point, declared in its own header; the first is as it was
    assert "mmh_q8_linear_s8" in q8.EXPORTS and "mmh_q8_linear_s8" in dynamic_exports(q8.LIB_PATH)
    assert not [n for n in q8.EXPORTS if "q8o" in n] and not [n for n in H.EXPORTS if "q8" in n]


def test_every_prototype_binds():
    L = q8.lib_q8o()
    _, prototypes = abi_header.parse(q8.Q8O_HEADER)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    _I, _P, _S = C.c_int, C.c_void_p, C.c_char_p
    assert prototypes["mmh_q8o_linear"] == (_I, [_I] * 4 + [_P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P])
    assert prototypes["mmh_q8o_linear_plan"] == (_I, [_I] * 10 + [_S, _I])
    assert prototypes["mmh_q8o_last_launch"] == (_S, [])
    assert q8.PROTOTYPES["mmh_q8_linear_s8"] == (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P])
    fresh = []
    reader = threading.Thread(target=lambda: fresh.append((L.mmh_q8o_last_launch(), L.mmh_q8o_last_error())))
    reader.start()
    reader.join()
    assert fresh == [(b"", b"")] and b"gfx950" in open(q8.Q8O_LIB_PATH, "rb").read()


ROWS = (1, 5, 128, 129, 512, 2048, 2560, 4096)
OUTS = (1, 3, 128, 130, 2048, 3328, 4096, 11008)


@pytest.mark.parametrize("cus", [256, 64])
def test_the_plan_is_the_python_restatement(cus):
    seen = set()
    for rows, out in itertools.product(ROWS, OUTS):
        p16 = (out + 15) & ~15
        for in_, (ldyq, y4) in itertools.product((0, 7, 4096), ((0, 0), (p16 + 4, 0), (out + 1, 0), (((out + 3) & ~3) + 2, 0),
                                                              (p16, 1), (p16, 2), (p16 + 2, 3))):
            want = Q.plan_text_s8o(rows, out, ldyq, y4, cus)
            assert q8.qlinear_s8o_plan(rows, out, in_, ldyq=ldyq, yq_mod4=y4, cu_count=cus) == want, (rows, out, in_, ldyq, y4)
            seen.add(want.split(">")[0])
    assert len(seen) == 4, sorted(seen)   # the grid reaches every instantiation
    assert q8.qlinear_s8o_plan(4096, 4096, 4096, cu_count=0) == q8.qlinear_s8o_plan(4096, 4096, 4096, cu_count=256)
    # whole tiles are unguarded only in dwords: a pitch of 2 modulo 4 or a base off a dword takes the guarded kernel
    assert q8.qlinear_s8o_plan(128, 128, 64) == "qlinear_s8o_kernel<128,128,4,false>, 1 workgroups"
    assert q8.qlinear_s8o_plan(128, 128, 64, ldyq=130) == q8.qlinear_s8o_plan(128, 128, 64, yq_mod4=2) == "qlinear_s8o_kernel<128,128,4,true>, 1 workgroups"


def test_argument_errors_are_refused_without_a_device():
    L, INV, UNS = q8.lib_q8o(), H.ERR_INVALID_ARG, H.ERR_UNSUPPORTED
    x = 4096   # (a non-NULL, dword-aligned address that is never read)
    # device, rows, out, in, dXq, ldq, d_inv_scale, dWq, pitch_n, d_w_inv_scale, dBias, activation, d_out_scale, dYq, ldyq, stream
    good = [0, 8, 8, 8, x, 8, x, x, 16, x, None, H.ACT_NONE, x, x, 8, None]
    assert L.mmh_q8o_linear(0, 0, 8, 8, None, 0, None, None, 0, None, None, 0, None, None, 0, None) == H.OK   # rows == 0
    bad_args = ((0, -1), (1, -1), (2, 0), (2, -1), (3, -1), (4, None), (5, 7), (6, None), (7, None), (8, 7), (9, None), (11, 2), (11, -1),
                (12, None), (13, None), (14, 7))
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert L.mmh_q8o_linear(*args) == INV, (i, bad)
        assert L.mmh_time_q8o_linear(*args[:15], 1, 1, None, C.byref(C.c_float(0))) == INV, (i, bad)
    # operands the tile cannot read in dwords, or beyond its window: refused with a message, nothing launched
    for i, bad in ((5, 9), (5, 10), (4, x + 1), (4, x + 2), (8, 18), (7, x + 3)):
        args = list(good)
        args[i] = bad
        assert L.mmh_q8o_linear(*args) == UNS and b"multiples of 4" in L.mmh_q8o_last_error(), (i, bad)
    far = list(good)
    far[1], far[2], far[3], far[5], far[8], far[14] = 8, 65536, 40000, 40000, 65536, 65536
    assert L.mmh_q8o_linear(*far) == UNS and b"window" in L.mmh_q8o_last_error()
    y = C.c_float(0)
    assert L.mmh_time_q8o_linear(*good[:15], 1, 0, None, C.byref(y)) == INV and L.mmh_time_q8o_linear(*good[:15], 1, 1, None, None) == INV
    assert L.mmh_time_q8o_linear(0, 0, 8, 8, x, 8, x, x, 16, x, None, 0, x, x, 8, 1, 1, None, C.byref(y)) == INV   # nothing to time
    # the plan: its own rules, and the call's
    text = C.create_string_buffer(128)
    ok = [8, 8, 8, 8, 16, 8, 0, 0, 0, 256, text, 128]   # rows, out, in, ldq, pitch_n, ldyq, xq_mod4, wq_mod4, yq_mod4, cus, text, bytes
    assert L.mmh_q8o_linear_plan(*ok) == H.OK and text.value == b"qlinear_s8o_kernel<128,128,4,true>, 1 workgroups"
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, -1), (3, 7), (4, 7), (5, 7), (6, 4), (7, -1), (8, 4), (10, None), (11, 0)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q8o_linear_plan(*args) == INV, (i, bad)
    for i, bad in ((3, 9), (4, 18), (6, 1), (7, 2)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q8o_linear_plan(*args) == UNS, (i, bad)
    assert L.mmh_q8o_linear_plan(8, 65536, 40000, 40000, 65536, 65536, 0, 0, 0, 256, text, 128) == UNS
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_s8o_plan(8, 8, 8, ldq=9)
    assert e.value.status == UNS
    # in == 0 reads neither operand: NULL rows and image, any pitch
    assert L.mmh_q8o_linear_plan(8, 8, 0, 0, 9, 9, 1, 1, 1, 256, text, 128) == H.OK


def test_the_second_librarys_new_entry_point_refuses_a_null_object():
    """(What it refuses of a real object's rows -- ldq < in, an odd ldq -- needs an object, so a device: tests/test_gpu_qchain.py.)"""
    L = q8.lib()
    assert L.mmh_q8_linear_s8(None, 1, 4096, 4, 4096, None, H.ACT_NONE, 4096, 4, None) == H.ERR_INVALID_ARG
    assert L.mmh_q8_linear_s8(None, 0, None, 0, None, None, H.ACT_NONE, None, 0, None) == H.ERR_INVALID_ARG
