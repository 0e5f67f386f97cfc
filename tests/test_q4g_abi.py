"""CPU tests of the sixth product library's boundary: build_all builds libmmult_hip_q4g.so after the fifth library with the
fifth's flags and its own directory in front, it exports exactly what include/mmult_hip_q4g.h declares, every prototype binds
from the parsed header, mmh_q4g_linear_plan is the Python restatement (tests/q4g_ref.py) over a grid of shapes, CU counts and
forced split counts -- with no ceiling on a range --, mmh_q4g_weight_layout is its restatement, and every stated refusal returns
its code before any device call."""
import ctypes as C
import itertools
import os
import threading

import pytest

import how_to_optimize_gemm_amd as H
from how_to_optimize_gemm_amd import abi_header, build, q8
import q4_ref as F
import q4g_ref as G
import qdecode_ref as D
from built_lib import REPO, dynamic_exports

NAMES = ["mmh_q4g_last_error", "mmh_q4g_last_launch", "mmh_q4g_linear", "mmh_q4g_linear_plan", "mmh_q4g_pack_weight",
         "mmh_q4g_weight_layout", "mmh_time_q4g_linear"]


def test_build_all_builds_the_library_after_the_fifth(monkeypatch):
    assert os.path.exists(build.Q4G_LIB), "libmmult_hip_q4g.so has not been built: build_all() builds it"
    assert build.Q4G_LIB == q8.Q4G_LIB_PATH == os.path.join(REPO, "how-to-optimize-gemm_amd", "libmmult_hip_q4g.so")
    calls = []
    for name in ("library", "q8_library", "q8o_library", "q8d_library", "q4d_library", "q4g_library"):
        monkeypatch.setattr(build, "build_" + name, lambda force=False, verbose=False, name=name: calls.append(name))
    monkeypatch.setattr(build, "build_harness", lambda force=False: calls.append("harness"))
    build.build_all()
    assert calls == ["library", "q8_library", "q8o_library", "q8d_library", "q4d_library", "q4g_library", "harness"], calls


def test_the_recipe_is_the_fifth_librarys_with_its_own_directory_in_front(monkeypatch):
    lines = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: lines.append(cmd))
    build.build_q4g_library(force=True)
    compiles, link = lines[:-1], lines[-1]
    tus = [f for f in os.listdir(build.CSRC_Q4G) if f.endswith(".hip")]
    assert len(compiles) == len(tus) >= 1
    fifth = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: fifth.append(cmd))
    build.build_q4d_library(force=True)
    q4d_flags = [a for a in fifth[0][1:fifth[0].index("-c")]]
    for cmd in compiles:
        flags = cmd[1:cmd.index("-c")]
        assert [a for a in flags if a != "-I" + build.CSRC_Q4G] == q4d_flags, cmd          # the fifth library's flags ...
        assert [a for a in flags if a.startswith("-I")][0] == "-I" + build.CSRC_Q4G, cmd   # ... plus -I csrc_q4g, in front
        assert os.path.dirname(cmd[cmd.index("-o") + 1]) == os.path.join(build.PKG_DIR, "build", "q4g")
    assert "-shared" in link and link[link.index("-o") + 1] == build.Q4G_LIB
    assert "-Wl,--version-script=" + os.path.join(build.CSRC_Q4G, "exports_q4g.map") in link
    assert not [a for a in link if "libmmult_hip" in a and a != build.Q4G_LIB], "links nothing of the other libraries"
    assert not [a for a in link if a.startswith("-l")], "links nothing else"
    # the older directories gained nothing
    assert sorted(os.listdir(build.CSRC_Q8D)) == ["exports_q8d.map", "q8d.hip", "qdecode_plan.hpp", "qdecode_s8.hpp"]
    assert sorted(os.listdir(build.CSRC_Q4D)) == ["exports_q4d.map", "q4d.hip", "q4decode_plan.hpp", "q4decode_s4.hpp", "quant_rules_s4.hpp"]
    assert sorted(os.listdir(build.CSRC_Q4G)) == ["exports_q4g.map", "q4g.hip", "q4gdecode_plan.hpp", "q4gdecode_s4.hpp"]


def test_the_header_parses_and_the_library_exports_exactly_its_prototypes():
    constants, prototypes = abi_header.parse(q8.Q4G_HEADER)
    assert constants == {"MMH_Q4G_MAX_ROWS": 16, "MMH_Q4G_GROUP": 128} and q8.Q4G_GROUP == G.GROUP == 128 and G.MAX_ROWS == 16
    assert sorted(prototypes) == NAMES
    assert dynamic_exports(q8.Q4G_LIB_PATH) == NAMES
    text = open(os.path.join(build.CSRC_Q4G, "exports_q4g.map")).read()
    assert "global: mmh_q4g_*; mmh_time_q4g_*;" in text and "local: *;" in text
    others = list(q8.EXPORTS) + list(H.EXPORTS) + list(abi_header.parse(q8.Q8O_HEADER)[1]) + list(abi_header.parse(q8.Q8D_HEADER)[1]) + \
        list(abi_header.parse(q8.Q4D_HEADER)[1])
    assert not [n for n in others if "q4g" in n]
    for older in (q8.LIB_PATH, q8.Q8O_LIB_PATH, q8.Q8D_LIB_PATH, q8.Q4D_LIB_PATH):
        assert not [n for n in dynamic_exports(older) if "q4g" in n]


def test_every_prototype_binds():
    L = q8.lib_q4g()
    _, prototypes = abi_header.parse(q8.Q4G_HEADER)
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    _I, _P, _S, _Z = C.c_int, C.c_void_p, C.c_char_p, C.c_size_t
    call = [_I] * 4 + [_P, _I, _P, _P, _I, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _Z, _I]
    assert prototypes["mmh_q4g_linear"] == (_I, call + [_P])
    # mmh_q4d_linear's, argument for argument, with pitch_s behind the scales
    theirs = list(abi_header.parse(q8.Q4D_HEADER)[1]["mmh_q4d_linear"][1])
    assert prototypes["mmh_q4g_linear"][1] == theirs[:10] + [_I] + theirs[10:]
    assert prototypes["mmh_time_q4g_linear"] == (_I, call + [_I, _I, _P, _P])
    assert prototypes["mmh_q4g_linear_plan"] == (_I, [_I] * 14 + [_S, _I, _P])
    assert prototypes["mmh_q4g_pack_weight"] == (_I, [_I, _I, _I, _P, _I, _P, _I, _P, _P, _I, _P])
    assert prototypes["mmh_q4g_weight_layout"] == (_I, [_I, _I, _P, _P, _P, _P, _P, _P])
    assert prototypes["mmh_q4g_last_launch"] == (_S, [])
    fresh = []
    reader = threading.Thread(target=lambda: fresh.append((L.mmh_q4g_last_launch(), L.mmh_q4g_last_error())))
    reader.start()
    reader.join()
    assert fresh == [(b"", b"")] and b"gfx950" in open(q8.Q4G_LIB_PATH, "rb").read()


def test_the_layout_is_its_restatement():
    for out, in_ in itertools.product((0, 1, 15, 16, 17, 128, 273, 4096, 11008), (0, 1, 64, 65, 127, 128, 129, 385, 4096, 11008, 65664)):
        assert q8.weight4g_layout(out, in_) == G.layout(out, in_), (out, in_)
        assert q8.weight4g_layout(out, in_)[:2] == q8.weight4_layout(out, in_)[:2]   # the image is the fifth library's
    assert q8.weight4g_layout(4096, 4096) == (4096, 2048, 32, 4096, 4096 * 4096 // 2, 32 * 4096 * 4)
    L = q8.lib_q4g()
    v = [C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)]
    refs = [C.byref(a) for a in v]
    assert L.mmh_q4g_weight_layout(-1, 1, *refs) == H.ERR_INVALID_ARG and L.mmh_q4g_weight_layout(1, -1, *refs) == H.ERR_INVALID_ARG
    for i in range(6):
        args = list(refs)
        args[i] = None
        assert L.mmh_q4g_weight_layout(1, 1, *args) == H.ERR_INVALID_ARG, i


ROWS = (1, 2, 7, 15, 16)
OUTS = (1, 17, 128, 129, 273, 4096, 11008)
INS = (0, 1, 128, 129, 385, 1153, 4096, 8192, 11008, 65536, 65664)


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_the_plan_is_the_python_restatement(cus):
    forms, beyond = set(), 0
    for rows, out, in_ in itertools.product(ROWS, OUTS, INS):
        for splits in (0, 1, 2, 3, 7, 32, 87):
            for out8, ldo, o16 in ((False, 0, 0), (False, out + 1, 0), (False, (out + 3) & ~3, 4), (True, 0, 0), (True, out + 2, 0),
                                   (True, (out + 3) & ~3, 1), (True, (out + 3) & ~3, 12)):
                want = G.plan(rows, out, in_, out8, ldo, o16, splits, cus)
                if want is None:
                    with pytest.raises(H.MMultError) as e:
                        q8.qlinear_decode4g_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus)
                    assert e.value.status == H.ERR_INVALID_ARG and "empty" in str(e.value)
                    continue
                text, work, s, k_len = want
                assert q8.qlinear_decode4g_plan(rows, out, in_, out8=out8, ldo=ldo, o_mod16=o16, splits=splits, cu_count=cus) == (text, work), \
                    (rows, out, in_, out8, ldo, o16, splits)
                assert work == D.work_bytes(s, rows, out) and work % 16 == 0 and (in_ == 0) == (work == 0)
                if in_:
                    assert k_len % 128 == 0 and (s - 1) * k_len < in_ <= s * k_len
                    assert text.startswith("q4gdecode_partial_kernel, ") and "q4gdecode_finish_kernel<" in text
                    beyond += k_len > F.MAX_RANGE_K
                    if splits == 0 and s > 1:   # the int8 plan's bounds, halved bytes
                        assert 2 * s * rows * out * 4 * D.TRAFFIC_DEN <= in_ * out // 2 * D.TRAFFIC_NUM
                        assert (s - 1) * -(-out // 128) * D.WG_DEN < D.WG_NUM * cus
                    # where the fifth library's ceiling does not bind, the partition is the fifth library's
                    theirs = F.plan(rows, out, in_, out8, ldo, o16, splits, cus)
                    if theirs not in (None, "long") and in_ <= F.MAX_RANGE_K:
                        assert theirs[1:] == want[1:]
                forms.add((text.split(",")[0], "wide" in text, out8))
    assert len(forms) == 8, sorted(forms)   # with and without partials x wide and single stores x both outputs
    assert beyond > 0                       # in = 65664 in one range: no ceiling here
    assert q8.qlinear_decode4g_plan(16, 4096, 4096, cu_count=0) == q8.qlinear_decode4g_plan(16, 4096, 4096, cu_count=256)
    assert q8.qlinear_decode4g_plan(16, 4096, 4096)[0] == \
        "q4gdecode_partial_kernel, 32 strips x 4 splits of 1024 k; q4gdecode_finish_kernel<false>, 64 workgroups, wide stores"


def test_the_windows_edge_is_where_the_formula_puts_it():
    L = q8.lib_q4g()
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    lim = (1 << 31) - 4096

    def status(in_, ldq, pitch_n, pitch_s):
        return L.mmh_q4g_linear_plan(16, 130, in_, ldq, pitch_n, pitch_s, 0, 130, 0, 0, 0, 0, 1, 256, text, 192, C.byref(work))

    for in_ in (129, 1, 128):
        pitch, packed = F.largest_pitch_n(in_), F.layout(1, in_)[1]
        assert status(in_, 132, pitch, 132) == H.OK, (in_, pitch, L.mmh_q4g_last_error())
        assert status(in_, 132, pitch + 4, 132) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q4g_last_error(), (in_, pitch)
        ps, groups = G.largest_pitch_s(in_), G.groups(in_)
        assert ps % 4 == 0 and (groups + 4) * ps * 4 + 1024 < lim <= (groups + 4) * (ps + 4) * 4 + 1024, (in_, ps)
        assert G.window_ok(132, 132, in_, ps) and not G.window_ok(132, 132, in_, ps + 4)
        assert status(in_, 132, 132, ps) == H.OK, (in_, ps, L.mmh_q4g_last_error())
        assert status(in_, 132, 132, ps + 4) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q4g_last_error(), (in_, ps)
    ldq = D.largest_ldq(129)
    assert status(129, ldq, 132, 132) == H.OK and status(129, ldq + 4, 132, 132) == H.ERR_UNSUPPORTED and b"window" in L.mmh_q4g_last_error()
    # in == 0: no scale is read, its pitch is not looked at
    assert L.mmh_q4g_linear_plan(8, 8, 0, 0, 9, 0, 1, 9, 1, 1, 5, 1, 0, 256, text, 192, C.byref(work)) == H.OK and work.value == 0
    assert text.value == b"q4gdecode_finish_kernel<true> alone, 8 workgroups, single stores"


def test_argument_errors_are_refused_without_a_device():
    L, INV, UNS = q8.lib_q4g(), H.ERR_INVALID_ARG, H.ERR_UNSUPPORTED
    x = 4096   # (a non-NULL, 16-byte aligned address that is never read)
    # 0 device, 1 rows, 2 out, 3 in, 4 dXq, 5 ldq, 6 d_inv_scale, 7 dWp, 8 pitch_n, 9 d_group_inv_scale, 10 pitch_s, 11 dBias,
    # 12 activation, 13 d_out_scale, 14 dY, 15 ldy, 16 dYq, 17 ldyq, 18 d_work, 19 work_bytes, 20 splits, 21 stream
    f32 = [0, 8, 8, 256, x, 256, x, x, 16, x, 16, None, H.ACT_NONE, None, x, 8, None, 0, x, 1 << 20, 0, None]
    s8 = list(f32)
    s8[13], s8[14], s8[15], s8[16], s8[17] = x, None, 0, x, 8
    ms = C.c_float(0)
    timed = lambda a: L.mmh_time_q4g_linear(*a[:21], 1, 1, None, C.byref(ms))
    assert L.mmh_q4g_linear(0, 0, 8, 8, None, 0, None, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, 0, None) == H.OK   # rows == 0
    for good, o, ld in ((f32, 14, 15), (s8, 16, 17)):
        bad_args = ((0, -1), (1, -1), (2, 0), (2, -1), (3, -1), (4, None), (5, 252), (6, None), (7, None), (8, 4), (9, None), (10, 4), (12, 2),
                    (12, -1), (o, None), (ld, 7), (18, None), (18, x + 8), (20, -1), (20, 3))   # (3 ranges of 128 k: the third is empty)
        for i, bad in bad_args:
            args = list(good)
            args[i] = bad
            assert L.mmh_q4g_linear(*args) == INV, (i, bad)
            assert timed(args) == INV, (i, bad)
        args = list(good)
        args[20] = 3
        assert L.mmh_q4g_linear(*args) == INV and b"empty" in L.mmh_q4g_last_error()
        # a workspace below the forced plan's, and below one range's whatever the device would choose
        for splits, short in ((2, 2 * 8 * 8 * 4 - 1), (0, 8 * 8 * 4 - 1), (1, 0)):
            args = list(good)
            args[19], args[20] = short, splits
            assert L.mmh_q4g_linear(*args) == INV and b"workspace is smaller" in L.mmh_q4g_last_error() and timed(args) == INV, splits
        # rows 17: refused as unsupported, with a message
        args = list(good)
        args[1] = 17
        assert L.mmh_q4g_linear(*args) == UNS and b"16 rows" in L.mmh_q4g_last_error() and timed(args) == UNS
        # operands the kernel cannot read in dwords ...
        for i, bad in ((5, 257), (5, 258), (4, x + 1), (4, x + 2), (8, 18), (7, x + 3)):
            args = list(good)
            args[i] = bad
            assert L.mmh_q4g_linear(*args) == UNS and b"multiples of 4" in L.mmh_q4g_last_error(), (i, bad)
        # ... a scale array it cannot read in 16-byte vectors ...
        for i, bad in ((9, x + 4), (9, x + 8), (9, x + 1), (10, 18), (10, 17)):
            args = list(good)
            args[i] = bad
            assert L.mmh_q4g_linear(*args) == UNS and b"16-byte" in L.mmh_q4g_last_error() and timed(args) == UNS, (i, bad)
        # ... or operands beyond its window: the image's, then the scales' alone
        far = list(good)
        far[2], far[3], far[5], far[8], far[10], far[ld] = 65536, 80000, 80000, 65536, 65536, 65536
        assert L.mmh_q4g_linear(*far) == UNS and b"window" in L.mmh_q4g_last_error()
        far = list(good)
        far[10] = G.largest_pitch_s(256) + 4
        assert L.mmh_q4g_linear(*far) == UNS and b"window" in L.mmh_q4g_last_error()
    for y, yq, so in ((x, x, None), (x, x, x), (None, None, None), (None, None, x), (None, x, None), (x, None, x)):
        args = list(f32)
        args[13], args[14], args[16], args[17] = so, y, yq, 8
        assert L.mmh_q4g_linear(*args) == INV and timed(args) == INV, (y, yq, so)
    assert L.mmh_time_q4g_linear(*f32[:21], 1, 0, None, C.byref(ms)) == INV and L.mmh_time_q4g_linear(*f32[:21], 1, 1, None, None) == INV
    zero = list(f32)
    zero[1] = 0
    assert timed(zero) == INV   # nothing to time
    # a range as long as the layer is no error here: the fifth library refuses one above 65536 k
    text, work = C.create_string_buffer(192), C.c_size_t(0)
    assert L.mmh_q4g_linear_plan(8, 8, 65664, 65664, 16, 16, 0, 8, 0, 0, 0, 0, 1, 256, text, 192, C.byref(work)) == H.OK
    assert b"1 strips x 1 splits of 65664 k" in text.value
    # the plan: its own rules, and the call's.  0 rows, 1 out, 2 in, 3 ldq, 4 pitch_n, 5 pitch_s, 6 out8, 7 ldo, 8 xq_mod4, 9 wp_mod4,
    # 10 gs_mod16, 11 o_mod16, 12 splits, 13 cu_count, 14 text, 15 text_bytes, 16 work_bytes
    ok = [8, 8, 256, 256, 16, 16, 0, 8, 0, 0, 0, 0, 2, 256, text, 192, C.byref(work)]
    assert L.mmh_q4g_linear_plan(*ok) == H.OK and work.value == 2 * 8 * 8 * 4
    assert text.value == b"q4gdecode_partial_kernel, 1 strips x 2 splits of 128 k; q4gdecode_finish_kernel<false>, 8 workgroups, wide stores"
    for i, bad in ((0, 0), (0, -1), (1, 0), (2, -1), (3, 252), (4, 4), (5, 4), (6, 2), (7, 7), (8, 4), (9, -1), (10, 16), (11, 16), (12, -1), (12, 3),
                   (14, None), (15, 0), (16, None)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q4g_linear_plan(*args) == INV, (i, bad)
    for i, bad in ((0, 17), (3, 257), (4, 18), (5, 18), (8, 1), (9, 2), (10, 4)):
        args = list(ok)
        args[i] = bad
        assert L.mmh_q4g_linear_plan(*args) == UNS, (i, bad)
    with pytest.raises(H.MMultError) as e:
        q8.qlinear_decode4g_plan(17, 8, 8)
    assert e.value.status == UNS
    # the packer: 0 device, 1 out, 2 in, 3 dW, 4 ldw, 5 dP, 6 pitch_n, 7 d_group_scale, 8 d_group_inv_scale, 9 pitch_s, 10 stream
    pack = [0, 8, 256, x, 256, x, 16, x, x, 16, None]
    for i, bad in ((0, -1), (1, -1), (2, -1), (3, None), (4, 255), (5, None), (5, x + 4), (6, 4), (6, 20), (7, None), (8, None), (9, 7)):
        args = list(pack)
        args[i] = bad
        assert L.mmh_q4g_pack_weight(*args) == INV, (i, bad)
    assert L.mmh_q4g_pack_weight(0, 0, 256, None, 0, None, 0, None, None, 0, None) == H.OK   # out == 0: nothing to do
    assert L.mmh_q4g_pack_weight(0, 8, 0, None, 0, None, 0, None, None, 0, None) == H.OK     # in == 0: no group, no packed row


def test_the_python_layer_refuses_without_a_device():
    """What needs no GPU of the Python layer: the group size, and group_size with 8-bit weights."""
    with pytest.raises(H.MMultError) as e:
        q8.QWeight4G(None, group_size=64)
    assert e.value.status == H.ERR_INVALID_ARG and "128" in str(e.value)
    assert issubclass(q8.QWeight4G, q8.QWeight4)
    for kwargs in ({"weight_bits": 8, "group_size": 128}, {"weight_bits": 4, "decode": True, "group_size": 64}, {"group_size": 128}):
        with pytest.raises(H.MMultError) as e:
            q8.QLinear(8, 8, **kwargs)
        assert e.value.status == H.ERR_INVALID_ARG, kwargs
    assert q8.QLinear(8, 8, decode=True, weight_bits=4, group_size=128).group_size == 128
    assert q8.QLinear(8, 8, decode=True, weight_bits=4).group_size is None and q8.QLinear(8, 8).group_size is None
