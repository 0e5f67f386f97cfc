"""CPU tests of the fourth product library's boundary: build_all builds libmmult_hip_q8d.so after the third library with the
third's flags and its own directory in front, it exports exactly what include/mmult_hip_q8d.h declares, every prototype binds
from the parsed header, mmh_q8d_linear_plan is the Python restatement (tests/qdecode_ref.py) over a grid of shapes, CU counts and
forced split counts, work_bytes is the header's formula, and argument errors are refused before any device call."""
import ctypes as C
import itertools
import os
import threading

import pytest

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, build, q8
import qdecode_ref as D
from built_lib import REPO, dynamic_exports


def test_build_all_builds_the_library_after_the_third(monkeypatch):
    assert os.path.exists(build.Q8D_LIB), "libmmult_hip_q8d.so has not been built: build_all() builds it"
    assert build.Q8D_LIB == q8.Q8D_LIB_PATH == os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q8d.so")
    calls = []
    monkeypatch.setattr(build, "build_library", lambda force=False, verbose=False: calls.append("product"))
    monkeypatch.setattr(build, "build_q8_library", lambda force=False, verbose=False: calls.append("q8"))
    monkeypatch.setattr(build, "build_q8o_library", lambda force=False, verbose=False: calls.append("q8o"))
    monkeypatch.setattr(build, "build_q8d_library", lambda force=False, verbose=False: calls.append("q8d"))
    monkeypatch.setattr(build, "build_harness", lambda force=False: calls.append("harness"))
    build.build_all()
    assert calls == ["product", "q8", "q8o", "q8d", "harness"], calls


def test_the_recipe_is_the_third_librarys_with_its_own_directory_in_front(monkeypatch):
    import concurrent.futures
    lines, workers = [], []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: lines.append(cmd))
    real = concurrent.futures.ThreadPoolExecutor

    def pool(max_workers=None):
        workers.append(max_workers)
        return real(max_workers=max_workers)

    monkeypatch.setattr(concurrent.futures, "ThreadPoolExecutor", pool)
    monkeypatch.setattr(build.os, "cpu_count", lambda: 192)
    build.build_q8d_library(force=True)
    compiles, link = lines[:-1], lines[-1]
    tus = [f for f in os.listdir(build.CSRC_Q8D) if f.endswith(".hip")]
    assert len(compiles) == len(tus) >= 1 and workers == [len(tus)] and max(workers) <= 16
    third = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: third.append(cmd))
    build.build_q8o_library(force=True)
    q8o_flags = [a for a in third[0][1:third[0].index("-c")]]
    for cmd in compiles:
        flags = cmd[1:cmd.index("-c")]
        assert [a for a in flags if a != "-I" + build.CSRC_Q8D] == q8o_flags, cmd          # the third library's flags ...
        assert [a for a in flags if a.startswith("-I")][0] == "-I" + build.CSRC_Q8D, cmd   # ... plus -I csrc_q8d, in front
        assert os.path.dirname(cmd[cmd.index("-o") + 1]) == os.path.join(build.PKG_DIR, "build", "q8d")
    assert "-shared" in link and link[link.index("-o") + 1] == build.Q8D_LIB
    assert "-Wl,--version-script=" + os.path.join(build.CSRC_Q8D, "exports_q8d.map") in link
    assert not [a for a in link if "libmmult_hip" in a and a != build.Q8D_LIB], "links nothing of the other libraries"
    # the one recipe caps every library's pool (cpu_count is 192 here): the second library's units, 16 of the first library's
    del workers[:]
    build.build_q8_library(force=True)
    build.build_library(force=True)
    assert len(workers) == 2 and max(workers) <= 16 and workers[1] == 16 < len(build.translation_units())


def test_the_header_parses_and_the_library_exports_exactly_its_prototypes():
    constants, prototypes = abi_header.parse(q8.Q8D_HEADER)
    assert constants == {"MMH_Q8D_MAX_ROWS": 16} and q8.Q8D_MAX_ROWS == D.MAX_ROWS == 16
    assert sorted(prototypes) == ["mmh_q8d_last_error", "mmh_q8d_last_launch", "mmh_q8d_linear", "mmh_q8d_linear_plan", "mmh_time_q8d_linear"]
    assert dynamic_exports(q8.Q8D_LIB_PATH) == sorted(prototypes)
    # the map names the same families and nothing else; the other libraries declare and export nothing of this one
    text = open(os.path.join(build.CSRC_Q8D, "exports_q8d.map")).read()
    assert "global: mmh_q8d_*; mmh_time_q8d_*;" in text and "local: *;" in text
    assert not [n for n in list(q8.EXPORTS) + list(H.EXPORTS) + list(abi_header.parse(q8.Q8O_HEADER)[1]) if "q8d" in n]


def test_every_prototype_binds():
    L = q8.lib_q8d()
    _, prototypes = abi_header.parse(q8.Q8D_HEADER)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    _I, _P, _S, _Z = C.c_int, C.c_void_p, C.c_char_p, C.c_size_t
    call = [_I] * 4 + [_P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _I, _P, _Z, _I]
    assert prototypes["mmh_q8d_linear"] == (_I, call + [_P])
    assert prototypes["mmh_time_q8d_linear"] == (_I, call + [_I, _I, _P, _P])
    assert prototypes["mmh_q8d_linear_plan"] == (_I, [_I] * 12 + [_S, _I, _P])
    assert prototypes["mmh_q8d_last_launch"] == (_S, [])
    fresh = []
    reader = threading.Thread(target=lambda: fresh.append((L.mmh_q8d_last_launch(), L.mmh_q8d_last_error())))
    reader.start()
    reader.join()
    assert fresh == [(b"", b"")] and b"gfx950" in open(q8.Q8D_LIB_PATH, "rb").read()


ROWS = (1, 2, 7, 15, 16)
OUTS = (1, 17, 128, 129, 273, 4096, 11008)
INS = (0, 1, 128, 129, 385, 1153, 4096, 8192, 11008)


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
def test_the_plan_is_the_python_restatement(cus):
    forms = set()
    for rows, out, in_ in itertools.product(ROWS, OUTS, INS):
        for splits in (0, 1, 2, 3, 7, 32, 87):
            for out8, ldo, o16 in ((False, 0, 0), (False, out + 1, 0), (False, (out + 3) & ~3, 4), (True, 0, 0), (True, out + 2, 0),
                                   (True, (out + 3) & ~3, 1), (True, (out + 3) & ~3, 12)):
                want = D.plan(rows, out, in_, out8, ldo, o16, splits, cus)
                if want is None:
                    with pytest.raises(H.MMultError) as e:
                        q8.qlinear_decode_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus)
                    assert e.value.status == H.ERR_INVALID_ARG and "empty" in str(e.value)
                    continue
                text, work, s, k_len = want
                assert q8.qlinear_decode_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus) == (text, work), \
                    (rows, out, in_, out8, ldo, o16, splits)
                # the header's formula, ranges that are multiples of the slice, none empty, the traffic bound
                assert work == D.work_bytes(s, rows, out) and work % 16 == 0 and (in_ == 0) == (work == 0)
                if in_:
                    assert k_len % 128 == 0 and (s - 1) * k_len < in_ <= s * k_len
                    if splits == 0 and s > 1:
                        assert 2 * s * rows * out * 4 * D.TRAFFIC_DEN <= in_ * out * D.TRAFFIC_NUM
                        assert (s - 1) * -(-out // 128) * D.WG_DEN < D.WG_NUM * cus
                forms.add((text.split(",")[0], "wide" in text, out8))
    assert len(forms) == 8, sorted(forms)   # with and without partials x wide and single stores x both outputs
    assert q8.qlinear_decode_plan(16, 4096, 4096, cu_count=0) == q8.qlinear_decode_plan(16, 4096, 4096, cu_count=256)
    assert q8.qlinear_decode_plan(16, 4096, 4096)[0] == \
        "qdecode_partial_kernel, 32 strips x 8 splits of 512 k; qdecode_finish_kernel<false>, 64 workgroups, wide stores"


def test_the_windows_edge_is_where_the_formula_puts_it():
    """shape_status admits the largest pitch_n and the largest ldq of i8_window's formula and refuses the next multiple of 4
    (tests/test_gpu_qdecode.py runs the admitted ones)."""
    L = q8.lib_q8d()
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    lim = (1 << 31) - 4096

    def status(in_, ldq, pitch_n):
        return L.mmh_q8d_linear_plan(16, 130, in_, ldq, pitch_n, 0, 130, 0, 0, 0, 1, 256, text, 192, C.byref(work))

    for in_ in (129, 1):
        pitch = D.largest_pitch_n(in_)
        assert pitch % 4 == 0 and (in_ + 256) * pitch + 256 < lim <= (in_ + 256) * (pitch + 4) + 256, (in_, pitch)
        assert D.window_ok(132, pitch, in_) and not D.window_ok(132, pitch + 4, in_)
        assert status(in_, 132, pitch) == H.OK, (in_, pitch, L.mmh_q8d_last_error())
        assert status(in_, 132, pitch + 4) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q8d_last_error(), (in_, pitch)
    assert (D.largest_pitch_n(129), D.largest_pitch_n(1)) == (5577868, 8355948)
    ldq = D.largest_ldq(129)
    assert ldq % 4 == 0 and 256 * ldq + 129 < lim <= 256 * (ldq + 4) + 129 and ldq == 8388588
    assert D.window_ok(ldq, 132, 129) and not D.window_ok(ldq + 4, 132, 129)
    assert status(129, ldq, 132) == H.OK, L.mmh_q8d_last_error()
    assert status(129, ldq + 4, 132) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q8d_last_error()
    # both at once are admitted too: the two conditions are independent
    assert status(129, ldq, D.largest_pitch_n(129)) == H.OK


def test_argument_errors_are_refused_without_a_device():
    L, INV, UNS = q8.lib_q8d(), H.ERR_INVALID_ARG, H.ERR_UNSUPPORTED
    x = 4096   # (a non-NULL, 16-byte aligned address that is never read)
    # 0 device, 1 rows, 2 out, 3 in, 4 dXq, 5 ldq, 6 d_inv_scale, 7 dWq, 8 pitch_n, 9 d_w_inv_scale, 10 dBias, 11 activation,
    # 12 d_out_scale, 13 dY, 14 ldy, 15 dYq, 16 ldyq, 17 d_work, 18 work_bytes, 19 splits, 20 stream
    f32 = [0, 8, 8, 256, x, 256, x, x, 16, x, None, H.ACT_NONE, None, x, 8, None, 0, x, 1 << 20, 0, None]
    s8 = list(f32)
    s8[12], s8[13], s8[14], s8[15], s8[16] = x, None, 0, x, 8
    ms = C.c_float(0)
    timed = lambda a: L.mmh_time_q8d_linear(*a[:20], 1, 1, None, C.byref(ms))
    assert L.mmh_q8d_linear(0, 0, 8, 8, None, 0, None, None, 0, None, None, 0, None, None, 0, None, 0, None, 0, 0, None) == H.OK   # rows == 0
    for good, o, ld in ((f32, 13, 14), (s8, 15, 16)):
        bad_args = ((0, -1), (1, -1), (2, 0), (2, -1), (3, -1), (4, None), (5, 252), (6, None), (7, None), (8, 4), (9, None), (11, 2), (11, -1),
                    (o, None), (ld, 7), (17, None), (17, x + 8), (19, -1), (19, 3))   # (3 ranges of 128 k: the third is empty)
        for i, bad in bad_args:
            args = list(good)
            args[i] = bad
            assert L.mmh_q8d_linear(*args) == INV, (i, bad)
            assert timed(args) == INV, (i, bad)
        # rows 17: refused as unsupported, with a message
        args = list(good)
        args[1] = 17
        assert L.mmh_q8d_linear(*args) == UNS and b"16 rows" in L.mmh_q8d_last_error() and timed(args) == UNS
        # operands the kernel cannot read in dwords, or beyond its window
        for i, bad in ((5, 257), (5, 258), (4, x + 1), (4, x + 2), (8, 18), (7, x + 3)):
            args = list(good)
            args[i] = bad
            assert L.mmh_q8d_linear(*args) == UNS and b"multiples of 4" in L.mmh_q8d_last_error(), (i, bad)
        far = list(good)
        far[2], far[3], far[5], far[8], far[ld] = 65536, 40000, 40000, 65536, 65536
        assert L.mmh_q8d_linear(*far) == UNS and b"window" in L.mmh_q8d_last_error()
    # both output pointers, neither, and the wrong one for the scale
    for y, yq, so in ((x, x, None), (x, x, x), (None, None, None), (None, None, x), (None, x, None), (x, None, x)):
        args = list(f32)
        args[12], args[13], args[15], args[16] = so, y, yq, 8
        assert L.mmh_q8d_linear(*args) == INV and timed(args) == INV, (y, yq, so)
    assert L.mmh_time_q8d_linear(*f32[:20], 1, 0, None, C.byref(ms)) == INV and L.mmh_time_q8d_linear(*f32[:20], 1, 1, None, None) == INV
    zero = list(f32)
    zero[1] = 0
    assert timed(zero) == INV   # nothing to time
    # the plan: its own rules, and the call's
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    # 0 rows, 1 out, 2 in, 3 ldq, 4 pitch_n, 5 out8, 6 ldo, 7 xq_mod4, 8 wq_mod4, 9 o_mod16, 10 splits, 11 cus, 12 text, 13 bytes, 14 work
    ok = [8, 8, 256, 256, 16, 0, 8, 0, 0, 0, 2, 256, text, 192, C.byref(work)]
    assert L.mmh_q8d_linear_plan(*ok) == H.OK and work.value == 2 * 8 * 8 * 4
    assert text.value == b"qdecode_partial_kernel, 1 strips x 2 splits of 128 k; qdecode_finish_kernel<false>, 8 workgroups, wide stores"
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, -1), (3, 252), (4, 4), (5, 2), (6, 7), (7, 4), (8, -1), (9, 16), (10, -1), (10, 3), (12, None),
                   (13, 0), (14, None)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q8d_linear_plan(*args) == INV, (i, bad)
    for i, bad in ((0, 17), (3, 257), (4, 18), (7, 1), (8, 2)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q8d_linear_plan(*args) == UNS, (i, bad)
    assert L.mmh_q8d_linear_plan(8, 65536, 40000, 40000, 65536, 0, 65536, 0, 0, 0, 0, 256, text, 192, C.byref(work)) == UNS
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode_plan(17, 8, 8)
    assert e.value.status == UNS
    # in == 0 reads neither operand: any pitch, any residue, no workspace
    assert L.mmh_q8d_linear_plan(8, 8, 0, 0, 9, 1, 9, 1, 1, 1, 0, 256, text, 192, C.byref(work)) == H.OK and work.value == 0
