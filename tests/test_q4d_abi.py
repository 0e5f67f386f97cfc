"""CPU tests of the fifth product library's boundary: build_all builds libmmult_hip_q4d.so after the fourth library with the
fourth's flags and its own directory in front, it exports exactly what include/mmult_hip_q4d.h declares, every prototype binds
from the parsed header, mmh_q4d_linear_plan is the Python restatement (tests/q4_ref.py) over a grid of shapes, CU counts and
forced split counts -- the 65536-k ceiling included --, mmh_q4d_weight_layout is its restatement, and every stated refusal
returns its code before any device call."""
import ctypes as C
import itertools
import os
import threading

import pytest

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, build, q8
import q4_ref as F
import qdecode_ref as D
from built_lib import REPO, dynamic_exports

NAMES = ["mmh_q4d_last_error", "mmh_q4d_last_launch", "mmh_q4d_linear", "mmh_q4d_linear_plan", "mmh_q4d_pack_weight",
         "mmh_q4d_weight_layout", "mmh_time_q4d_linear"]


def test_build_all_builds_the_library_after_the_fourth(monkeypatch):
    assert os.path.exists(build.Q4D_LIB), "libmmult_hip_q4d.so has not been built: build_all() builds it"
    assert build.Q4D_LIB == q8.Q4D_LIB_PATH == os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q4d.so")
    calls = []
    for name in ("library", "q8_library", "q8o_library", "q8d_library", "q4d_library"):
        monkeypatch.setattr(build, "build_" + name, lambda force=False, verbose=False, name=name: calls.append(name))
    monkeypatch.setattr(build, "build_harness", lambda force=False: calls.append("harness"))
    build.build_all()
    assert calls == ["library", "q8_library", "q8o_library", "q8d_library", "q4d_library", "harness"], calls


def test_the_recipe_is_the_fourth_librarys_with_its_own_directory_in_front(monkeypatch):
    lines = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: lines.append(cmd))
    build.build_q4d_library(force=True)
    compiles, link = lines[:-1], lines[-1]
    tus = [f for f in os.listdir(build.CSRC_Q4D) if f.endswith(".hip")]
    assert len(compiles) == len(tus) >= 1
    fourth = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: fourth.append(cmd))
    build.build_q8d_library(force=True)
    q8d_flags = [a for a in fourth[0][1:fourth[0].index("-c")]]
    for cmd in compiles:
        flags = cmd[1:cmd.index("-c")]
        assert [a for a in flags if a != "-I" + build.CSRC_Q4D] == q8d_flags, cmd          # the fourth library's flags ...
        assert [a for a in flags if a.startswith("-I")][0] == "-I" + build.CSRC_Q4D, cmd   # ... plus -I csrc_q4d, in front
        assert os.path.dirname(cmd[cmd.index("-o") + 1]) == os.path.join(build.PKG_DIR, "build", "q4d")
    assert "-shared" in link and link[link.index("-o") + 1] == build.Q4D_LIB
    assert "-Wl,--version-script=" + os.path.join(build.CSRC_Q4D, "exports_q4d.map") in link
    assert not [a for a in link if "libmmult_hip" in a and a != build.Q4D_LIB], "links nothing of the other libraries"
    # the older directories gained nothing
    assert sorted(os.listdir(build.CSRC_Q8D)) == ["exports_q8d.map", "q8d.hip", "qdecode_plan.hpp", "qdecode_s8.hpp"]


def test_the_header_parses_and_the_library_exports_exactly_its_prototypes():
    constants, prototypes = abi_header.parse(q8.Q4D_HEADER)
    assert constants == {"MMH_Q4D_MAX_ROWS": 16, "MMH_Q4D_MAX_RANGE_K": 65536} and q8.Q4D_MAX_ROWS == F.MAX_ROWS == 16
    assert F.MAX_RANGE_K == constants["MMH_Q4D_MAX_RANGE_K"]
    assert sorted(prototypes) == NAMES
    assert dynamic_exports(q8.Q4D_LIB_PATH) == NAMES
    text = open(os.path.join(build.CSRC_Q4D, "exports_q4d.map")).read()
    assert "global: mmh_q4d_*; mmh_time_q4d_*;" in text and "local: *;" in text
    others = list(q8.EXPORTS) + list(H.EXPORTS) + list(abi_header.parse(q8.Q8O_HEADER)[1]) + list(abi_header.parse(q8.Q8D_HEADER)[1])
    assert not [n for n in others if "q4d" in n]
    for older in (q8.LIB_PATH, q8.Q8O_LIB_PATH, q8.Q8D_LIB_PATH):
        assert not [n for n in dynamic_exports(older) if "q4d" in n]


def test_every_prototype_binds():
    L = q8.lib_q4d()
    _, prototypes = abi_header.parse(q8.Q4D_HEADER)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    _I, _P, _S, _Z = C.c_int, C.c_void_p, C.c_char_p, C.c_size_t
    call = [_I] * 4 + [_P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _I, _P, _Z, _I]
    assert prototypes["mmh_q4d_linear"] == (_I, call + [_P])                         # mmh_q8d_linear's, argument for argument
    assert prototypes["mmh_q4d_linear"][1] == abi_header.parse(q8.Q8D_HEADER)[1]["mmh_q8d_linear"][1]
    assert prototypes["mmh_time_q4d_linear"] == (_I, call + [_I, _I, _P, _P])
    assert prototypes["mmh_q4d_linear_plan"] == (_I, [_I] * 12 + [_S, _I, _P])
    assert prototypes["mmh_q4d_pack_weight"] == (_I, [_I, _I, _I, _P, _I, _P, _I, _P, _P, _P])
    assert prototypes["mmh_q4d_weight_layout"] == (_I, [_I, _I, _P, _P, _P])
    assert prototypes["mmh_q4d_last_launch"] == (_S, [])
    fresh = []
    reader = threading.Thread(target=lambda: fresh.append((L.mmh_q4d_last_launch(), L.mmh_q4d_last_error())))
    reader.start()
    reader.join()
    assert fresh == [(b"", b"")] and b"gfx950" in open(q8.Q4D_LIB_PATH, "rb").read()


def test_the_layout_is_its_restatement():
    for out, in_ in itertools.product((0, 1, 15, 16, 17, 128, 273, 4096, 11008), (0, 1, 64, 65, 127, 128, 129, 385, 4096, 11008, 65664)):
        assert q8.weight4_layout(out, in_) == F.layout(out, in_), (out, in_)
    assert q8.weight4_layout(4096, 4096) == (4096, 2048, 4096 * 4096 // 2)
    L = q8.lib_q4d()
    a, b, z = C.c_int(0), C.c_int(0), C.c_size_t(0)
    assert L.mmh_q4d_weight_layout(-1, 1, C.byref(a), C.byref(b), C.byref(z)) == H.ERR_INVALID_ARG
    assert L.mmh_q4d_weight_layout(1, -1, C.byref(a), C.byref(b), C.byref(z)) == H.ERR_INVALID_ARG
    assert L.mmh_q4d_weight_layout(1, 1, None, C.byref(b), C.byref(z)) == H.ERR_INVALID_ARG
    assert L.mmh_q4d_weight_layout(1, 1, C.byref(a), C.byref(b), None) == H.ERR_INVALID_ARG


ROWS = (1, 2, 7, 15, 16)
OUTS = (1, 17, 128, 129, 273, 4096, 11008)
INS = (0, 1, 128, 129, 385, 1153, 4096, 8192, 11008, 65536, 65664)


@pytest.mark.parametrize("cus", [256, 304, 64, 1])
def test_the_plan_is_the_python_restatement(cus):
    forms, long_ = set(), 0
    for rows, out, in_ in itertools.product(ROWS, OUTS, INS):
        for splits in (0, 1, 2, 3, 7, 32, 87):
            for out8, ldo, o16 in ((False, 0, 0), (False, out + 1, 0), (False, (out + 3) & ~3, 4), (True, 0, 0), (True, out + 2, 0),
                                   (True, (out + 3) & ~3, 1), (True, (out + 3) & ~3, 12)):
                want = F.plan(rows, out, in_, out8, ldo, o16, splits, cus)
                if want is None or want == "long":
                    with pytest.raises(H.MMultError) as e:
                        q8.qlinear_decode4_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus)
                    assert e.value.status == H.ERR_INVALID_ARG and ("empty" if want is None else "longer than 65536 k") in str(e.value)
                    long_ += want == "long"
                    continue
                text, work, s, k_len = want
                assert q8.qlinear_decode4_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus) == (text, work), \
                    (rows, out, in_, out8, ldo, o16, splits)
                assert work == D.work_bytes(s, rows, out) and work % 16 == 0 and (in_ == 0) == (work == 0)
                if in_:
                    assert k_len % 128 == 0 and (s - 1) * k_len < in_ <= s * k_len and k_len <= F.MAX_RANGE_K
                    assert text.startswith("q4decode_partial_kernel, ")
                    if splits == 0 and s > 1 and k_len < F.MAX_RANGE_K // 2:   # (not raised by the ceiling: the int8 plan's bounds, halved bytes)
                        assert 2 * s * rows * out * 4 * D.TRAFFIC_DEN <= in_ * out // 2 * D.TRAFFIC_NUM
                        assert (s - 1) * -(-out // 128) * D.WG_DEN < D.WG_NUM * cus
                forms.add((text.split(",")[0], "wide" in text, out8))
    assert len(forms) == 8, sorted(forms)   # with and without partials x wide and single stores x both outputs
    assert long_ > 0                        # in = 65664 in one forced range
    assert q8.qlinear_decode4_plan(16, 4096, 4096, cu_count=0) == q8.qlinear_decode4_plan(16, 4096, 4096, cu_count=256)
    assert q8.qlinear_decode4_plan(16, 4096, 4096)[0] == \
        "q4decode_partial_kernel, 32 strips x 4 splits of 1024 k; qdecode_finish_kernel<false>, 64 workgroups, wide stores"


def test_the_plan_holds_the_overflow_bound_where_the_occupancy_rule_would_not():
    """in = 65536 + 128 at ONE compute unit.  One strip: the occupancy rule asks for ceil(3 / 2) = 2 ranges, each within the
    bound.  Two strips: it asks for ceil(3 / 4) = 1 range of 65664 k, above the ceiling -- the plan makes it two.  Forcing one
    range is refused; forcing two is what the plan chose."""
    in_ = F.MAX_RANGE_K + 128
    for out, alone in ((100, 2), (200, 1)):
        strips = -(-out // 128)
        assert -(-D.WG_NUM * 1 // (D.WG_DEN * strips)) == alone
        for rows in (1, 16):
            text, work, s, k_len = F.plan(rows, out, in_, cus=1)
            assert (s, k_len) == (2, 32896) and k_len <= F.MAX_RANGE_K and (1 << 14) * k_len < 1 << 31
            assert q8.qlinear_decode4_plan(rows, out, in_, cu_count=1) == (text, work)
            assert f"{strips} strips x 2 splits of 32896 k" in text
            assert q8.qlinear_decode4_plan(rows, out, in_, splits=2, cu_count=1) == (text, work)
            with pytest.raises(H.MMultError) as e:
                q8.qlinear_decode4_plan(rows, out, in_, splits=1, cu_count=1)
            assert e.value.status == H.ERR_INVALID_ARG and "65536" in str(e.value)
    # exactly at the ceiling one range is allowed; the int8 plan, which has no ceiling, keeps one range beyond it
    assert F.plan(16, 200, F.MAX_RANGE_K, cus=1)[2:] == (1, F.MAX_RANGE_K) == q8_plan_tail(16, 200, F.MAX_RANGE_K)
    assert D.plan(16, 200, in_, cus=1)[2:] == (1, in_)


def q8_plan_tail(rows, out, in_):
    text, _ = q8.qlinear_decode4_plan(rows, out, in_, cu_count=1)
    s, k = text.split(" x ")[1].split(" splits of ")
    return int(s), int(k.split(" k")[0])


def test_the_windows_edge_is_where_the_formula_puts_it():
    L = q8.lib_q4d()
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    lim = (1 << 31) - 4096

    def status(in_, ldq, pitch_n):
        return L.mmh_q4d_linear_plan(16, 130, in_, ldq, pitch_n, 0, 130, 0, 0, 0, 1, 256, text, 192, C.byref(work))

    for in_ in (129, 1, 128):
        pitch, packed = F.largest_pitch_n(in_), F.layout(1, in_)[1]
        assert pitch % 4 == 0 and (packed + 128) * pitch + 256 < lim <= (packed + 128) * (pitch + 4) + 256, (in_, pitch)
        assert F.window_ok(132, pitch, in_) and not F.window_ok(132, pitch + 4, in_)
        assert status(in_, 132, pitch) == H.OK, (in_, pitch, L.mmh_q4d_last_error())
        assert status(in_, 132, pitch + 4) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q4d_last_error(), (in_, pitch)
    ldq = D.largest_ldq(129)
    assert status(129, ldq, 132) == H.OK and status(129, ldq + 4, 132) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q4d_last_error()


def test_argument_errors_are_refused_without_a_device():
    L, INV, UNS = q8.lib_q4d(), H.ERR_INVALID_ARG, H.ERR_UNSUPPORTED
    x = 4096   # (a non-NULL, 16-byte aligned address that is never read)
    # 0 device, 1 rows, 2 out, 3 in, 4 dXq, 5 ldq, 6 d_inv_scale, 7 dWp, 8 pitch_n, 9 d_w_inv_scale, 10 dBias, 11 activation,
    # 12 d_out_scale, 13 dY, 14 ldy, 15 dYq, 16 ldyq, 17 d_work, 18 work_bytes, 19 splits, 20 stream
    f32 = [0, 8, 8, 256, x, 256, x, x, 16, x, None, H.ACT_NONE, None, x, 8, None, 0, x, 1 << 20, 0, None]
    s8 = list(f32)
    s8[12], s8[13], s8[14], s8[15], s8[16] = x, None, 0, x, 8
    ms = C.c_float(0)
    timed = lambda a: L.mmh_time_q4d_linear(*a[:20], 1, 1, None, C.byref(ms))
    assert L.mmh_q4d_linear(0, 0, 8, 8, None, 0, None, None, 0, None, None, 0, None, None, 0, None, 0, None, 0, 0, None) == H.OK   # rows == 0
    for good, o, ld in ((f32, 13, 14), (s8, 15, 16)):
        bad_args = ((0, -1), (1, -1), (2, 0), (2, -1), (3, -1), (4, None), (5, 252), (6, None), (7, None), (8, 4), (9, None), (11, 2), (11, -1),
                    (o, None), (ld, 7), (17, None), (17, x + 8), (19, -1), (19, 3))   # (3 ranges of 128 k: the third is empty)
        for i, bad in bad_args:
            args = list(good)
            args[i] = bad
            assert L.mmh_q4d_linear(*args) == INV, (i, bad)
            assert timed(args) == INV, (i, bad)
        args = list(good)
        args[19] = 3
        assert L.mmh_q4d_linear(*args) == INV and b"empty" in L.mmh_q4d_last_error()
        # a forced range above 65536 k
        args = list(good)
        args[3], args[5], args[19] = 65664, 65664, 1
        assert L.mmh_q4d_linear(*args) == INV and b"longer than 65536 k" in L.mmh_q4d_last_error() and timed(args) == INV
        # a workspace below the forced plan's, and below one range's whatever the device would choose
        for splits, short in ((2, 2 * 8 * 8 * 4 - 1), (0, 8 * 8 * 4 - 1), (1, 0)):
            args = list(good)
            args[18], args[19] = short, splits
            assert L.mmh_q4d_linear(*args) == INV and b"workspace is smaller" in L.mmh_q4d_last_error() and timed(args) == INV, splits
        # rows 17: refused as unsupported, with a message
        args = list(good)
        args[1] = 17
        assert L.mmh_q4d_linear(*args) == UNS and b"16 rows" in L.mmh_q4d_last_error() and timed(args) == UNS
        # operands the kernel cannot read in dwords, or beyond its window
        for i, bad in ((5, 257), (5, 258), (4, x + 1), (4, x + 2), (8, 18), (7, x + 3)):
            args = list(good)
            args[i] = bad
            assert L.mmh_q4d_linear(*args) == UNS and b"multiples of 4" in L.mmh_q4d_last_error(), (i, bad)
        far = list(good)
        far[2], far[3], far[5], far[8], far[ld] = 65536, 80000, 80000, 65536, 65536
        assert L.mmh_q4d_linear(*far) == UNS and b"window" in L.mmh_q4d_last_error()
    for y, yq, so in ((x, x, None), (x, x, x), (None, None, None), (None, None, x), (None, x, None), (x, None, x)):
        args = list(f32)
        args[12], args[13], args[15], args[16] = so, y, yq, 8
        assert L.mmh_q4d_linear(*args) == INV and timed(args) == INV, (y, yq, so)
    assert L.mmh_time_q4d_linear(*f32[:20], 1, 0, None, C.byref(ms)) == INV and L.mmh_time_q4d_linear(*f32[:20], 1, 1, None, None) == INV
    zero = list(f32)
    zero[1] = 0
    assert timed(zero) == INV   # nothing to time
    # the plan: its own rules, and the call's
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    ok = [8, 8, 256, 256, 16, 0, 8, 0, 0, 0, 2, 256, text, 192, C.byref(work)]
    assert L.mmh_q4d_linear_plan(*ok) == H.OK and work.value == 2 * 8 * 8 * 4
    assert text.value == b"q4decode_partial_kernel, 1 strips x 2 splits of 128 k; qdecode_finish_kernel<false>, 8 workgroups, wide stores"
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, -1), (3, 252), (4, 4), (5, 2), (6, 7), (7, 4), (8, -1), (9, 16), (10, -1), (10, 3), (12, None),
                   (13, 0), (14, None)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q4d_linear_plan(*args) == INV, (i, bad)
    for i, bad in ((0, 17), (3, 257), (4, 18), (7, 1), (8, 2)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q4d_linear_plan(*args) == UNS, (i, bad)
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode4_plan(17, 8, 8)
    assert e.value.status == UNS
    assert L.mmh_q4d_linear_plan(8, 8, 0, 0, 9, 1, 9, 1, 1, 1, 0, 256, text, 192, C.byref(work)) == H.OK and work.value == 0
    # the packer: 0 device, 1 out, 2 in, 3 dW, 4 ldw, 5 dP, 6 pitch_n, 7 d_scale, 8 d_inv_scale, 9 stream
    pack = [0, 8, 256, x, 256, x, 16, x, x, None]
    for i, bad in ((0, -1), (1, -1), (2, -1), (3, None), (4, 255), (5, None), (5, x + 4), (6, 4), (6, 20), (7, None), (8, None)):
        args = list(pack)
        args[i] = bad
        assert L.mmh_q4d_pack_weight(*args) == INV, (i, bad)
    assert L.mmh_q4d_pack_weight(0, 0, 256, None, 0, None, 0, None, None, None) == H.OK   # out == 0: nothing to do
