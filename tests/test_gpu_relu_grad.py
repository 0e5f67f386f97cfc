"""mmh_relu_grad_colsum on the device against tests/relu_grad_ref.py, bit for bit (NaN equal to NaN): every mode -- gate on /
off, dz written / not, column sum on / off, accumulate, in place -- on dense operands, padded leading dimensions (a multiple of
four: the vector path, ragged column counts included; odd: the scalar path) and bases one float off (the scalar path), the
path asserted from mmh_last_launch; the floats between the rows and around the windows are canaries that must survive; the
special values of the gate; the argument checks; and one rate floor against torch's where + sum(0)."""
import ctypes as C
import statistics

import numpy as np
import pytest

import relu_grad_ref as ref
from built_lib import REPO
from gpu_operands import handle_fixture

pytestmark = pytest.mark.gpu

R = ref.header_block_rows(REPO)
ROWS = [1, R - 1, R, R + 1, 2 * R + 44]
COLS = [1, 3, 4, 255, 256, 257, 1028]
# the finish kernel adds the partial rows RG_FU = 16 at a time, behind p_0: one full batch with a one-row last block, a batch plus
# one block, two full batches, two batches plus one block (tests/test_relu_grad_ref.py: at these very inputs other orders,
# other block heights and dropped blocks give other bits)
MANY_BLOCK_ROWS = [16 * R + 1, 17 * R + 77, 32 * R + 1, 33 * R + 77]
MANY_BLOCK_COLS = [5, 260]      # one quad and a leftover column; more than one chunk of 256 scalar items, 65 quads
CANARY = np.float32(-777.25)
FRONT = 8   # canary floats in front of a window (a multiple of 4: the window's base stays 16-byte aligned)


amm = handle_fixture()   # the module's own handle on MMH_KERNEL_AUTO (the session fixture's `mfma` kernel has no op forms)


_CASES = {}


def _case(rows, cols):
    """Inputs and the contract's results for a shape, computed once: g with -0 and subnormals sprinkled in, y with +-0."""
    key = (rows, cols)
    if key not in _CASES:
        g, y, old = ref.case_inputs(rows, cols)
        z_on, s_on = ref.relu_grad_colsum(g, y, R)
        z_off, s_off = ref.relu_grad_colsum(g, None, R)
        _CASES[key] = dict(g=g, y=y, old=old, z_on=z_on, s_on=s_on, z_off=z_off, s_off=s_off,
                           s_on_acc=ref.blocked_colsum(z_on, R, old), s_off_acc=ref.blocked_colsum(z_off, R, old))
        for v in _CASES[key].values():
            v.setflags(write=False)
    return _CASES[key]


LAYOUTS = {
    #             ld(cols),                         base offset in floats
    "dense":      (lambda c: c,                     0),
    "padded4":    (lambda c: (c + 3) // 4 * 4 + 4,  0),     # the vector path, ragged column counts included
    "padded_odd": (lambda c: (c + 4) | 1,           0),     # the scalar path
    "offset1":    (lambda c: (c + 3) // 4 * 4 + 4,  1),     # the scalar path
}


class Window:
    """A rows x cols window with leading dimension ld inside a canary-filled device buffer."""

    def __init__(self, torch, rows, cols, ld, off, host=None):
        self.rows, self.cols, self.ld, self.start = rows, cols, ld, FRONT + off
        n = self.start + rows * ld + FRONT
        self.image = np.full(n, CANARY, dtype=np.float32)
        if host is not None:
            self.view(self.image)[:] = host
        self.buf = torch.from_numpy(self.image.copy()).cuda()
        self.t = self.buf.as_strided((rows, cols), (ld, 1), self.start)

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.start:], (self.rows, self.cols), (self.ld * 4, 4))

    def expect(self, host):
        """The whole buffer with `host` in the window and every other float as it was."""
        want = self.image.copy()
        self.view(want)[:] = host
        return want

    def whole(self):
        return self.buf.cpu().numpy()


def _run(torch, H, amm, c, layout, gate, dz, colsum, accumulate, inplace):
    rows, cols = c["g"].shape
    ld_of, off = LAYOUTS[layout] if isinstance(layout, str) else layout
    ld = ld_of(cols)
    vector = off == 0 and (ld if rows > 1 else cols) % 4 == 0    # (a one-row tensor's leading dimension is its length)
    g = Window(torch, rows, cols, ld, off, c["g"])
    y = Window(torch, rows, cols, ld, off, c["y"]) if gate else None
    z = g if inplace else (Window(torch, rows, cols, ld, off) if dz else None)
    cs = None
    if colsum:
        cs_buf = torch.from_numpy(np.concatenate([np.full(FRONT + off, CANARY), c["old"], np.full(FRONT, CANARY)]).astype(np.float32)).cuda()
        cs = cs_buf[FRONT + off:FRONT + off + cols]
    got_z, got_s = amm.relu_grad_colsum(g.t, y.t if gate else None, dz=z.t if z is not None else None, want_dz=dz,
                                        bias_grad=cs, want_colsum=colsum, accumulate=accumulate)
    text = H.last_launch()
    torch.cuda.synchronize()
    tag = (rows, cols, layout, gate, dz, colsum, accumulate, inplace, text)
    assert text.startswith("relu_grad_colsum_kernel (%s path)" % ("vector" if vector else "scalar")), tag
    assert ("gate on" if gate else "gate off") in text and ("dz written" if dz else "dz not written") in text, tag
    nblocks = (rows + R - 1) // R
    if colsum:
        assert f"colsum {nblocks} block" in text and f"of {R} rows" in text, tag
        assert ("+ finish" in text) == (nblocks > 1) and ("accumulated" in text) == accumulate, tag
    else:
        assert "no colsum" in text, tag
    want_z = c["z_on"] if gate else c["z_off"]
    if dz:
        assert got_z is z.t, tag
        assert ref.same_bits(z.whole(), z.expect(want_z)), tag          # the window's bits, and every canary around it
    else:
        assert got_z is None, tag
    if not inplace:
        assert ref.same_bits(g.whole(), g.expect(c["g"])), tag              # inputs are not written
    if gate:
        assert ref.same_bits(y.whole(), y.expect(c["y"])), tag
    if colsum:
        want_s = c[("s_on" if gate else "s_off") + ("_acc" if accumulate else "")]
        got = cs_buf.cpu().numpy()
        assert ref.same_bits(got[FRONT + off:FRONT + off + cols], want_s), tag
        assert np.all(got[:FRONT + off] == CANARY) and np.all(got[FRONT + off + cols:] == CANARY), tag
    else:
        assert got_s is None, tag


#        gate   dz     colsum accumulate inplace
MODES = [(True, True, True, False, False),
         (False, True, True, True, False),
         (True, False, True, False, False),
         (True, True, False, False, False),
         (True, True, True, True, True),
         (False, False, True, False, False),
         (False, True, False, False, True)]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_every_mode_and_layout_is_bit_equal_to_the_contract(amm, rows, cols):
    import torch
    import how_to_optimize_gemm_amd as H
    c = _case(rows, cols)
    for layout in LAYOUTS:
        for mode in MODES:
            _run(torch, H, amm, c, layout, *mode)


@pytest.mark.parametrize("cols", MANY_BLOCK_COLS)
@pytest.mark.parametrize("rows", MANY_BLOCK_ROWS)
def test_every_mode_and_layout_at_the_finish_kernels_batch_boundaries(amm, rows, cols):
    import torch
    import how_to_optimize_gemm_amd as H
    c = _case(rows, cols)
    for layout in LAYOUTS:
        for mode in MODES:
            _run(torch, H, amm, c, layout, *mode)


def _wide_case(rows, cols):
    """_case for a two-vector-operation reference: at most R rows, so every sum is one chain."""
    assert rows <= R
    g, y, old = ref.case_inputs(rows, cols)
    z_on = ref.gate(g, y)
    s_on, s_off = ref.chain(z_on), ref.chain(g)
    return dict(g=g, y=y, old=old, z_on=z_on, z_off=g, s_on=s_on, s_off=s_off, s_on_acc=old + s_on, s_off_acc=old + s_off)


def test_the_strided_column_loop_of_the_scalar_path(amm):
    """65535 * 256 + 256 + 3 columns on the scalar path: more than 65535 chunks of 256 items, so grid.y stops at 65535 and the
    blockIdx.y loop takes a second step -- a whole chunk and a ragged one."""
    import torch
    import how_to_optimize_gemm_amd as H
    rows, cols = 2, 65535 * 256 + 256 + 3
    assert (cols + 255) // 256 == 65535 + 2
    c = _wide_case(rows, cols)
    for layout in (LAYOUTS["padded_odd"], (lambda n: n, 1)):         # an odd leading dimension; dense, the base one float off
        _run(torch, H, amm, c, layout, True, True, True, False, False)
        _run(torch, H, amm, c, layout, False, False, True, True, False)


def test_the_strided_column_loop_of_the_vector_path(amm):
    """4 (65535 * 256 + 256) + 3 columns in one 16-byte aligned row: 65535 + 2 chunks of quads, the three columns past them on
    the last chunk's scalar walk.  Through the C entry point, which takes a one-row window's leading dimension as given (the
    torch glue passes the row's length, which is odd here)."""
    import torch
    import how_to_optimize_gemm_amd as H
    cols = 4 * 65535 * 256 + 4 * 256 + 3
    assert (cols // 4 + cols % 4 + 255) // 256 == 65535 + 2
    rng = np.random.default_rng(cols)
    g, y = rng.standard_normal(cols, dtype=np.float32), rng.standard_normal(cols, dtype=np.float32)
    y[::7] = np.float32(-0.0)
    want = ref.gate(g, y)
    pad = np.full(FRONT, CANARY, dtype=np.float32)
    dg, dy = (torch.from_numpy(np.concatenate([pad, a, pad])).cuda() for a in (g, y))
    dz, ds = torch.full_like(dg, float(CANARY)), torch.full_like(dg, float(CANARY))
    ptr = lambda t: C.c_void_p(t.data_ptr() + 4 * FRONT)
    assert H.lib().mmh_relu_grad_colsum(amm._h, 1, cols, ptr(dg), cols + 1, ptr(dy), cols + 1, ptr(dz), cols + 1, ptr(ds), 0, None) == H.OK
    text = H.last_launch()
    torch.cuda.synchronize()
    assert text == "relu_grad_colsum_kernel (vector path), gate on, dz written, colsum 1 block of %d rows, written by the pass" % R, text
    for got in (dz, ds):                      # one row: the sums are the row
        got = got.cpu().numpy()
        assert ref.same_bits(got[FRONT:FRONT + cols], want)
        assert np.all(got[:FRONT] == CANARY) and np.all(got[FRONT + cols:] == CANARY)
    assert ref.same_bits(dg.cpu().numpy()[FRONT:FRONT + cols], g) and ref.same_bits(dy.cpu().numpy()[FRONT:FRONT + cols], y)


def test_the_workspace_across_calls_of_changing_size():
    """One handle of its own (the workspace starts empty), one stream, no synchronisation between the calls: the partial-row
    workspace grows twice, its row length changes from call to call, and a larger buffer serves a smaller call.  Every call
    once more accumulating, without a gate."""
    import torch
    import how_to_optimize_gemm_amd as H
    shapes = [(2 * R + 1, 64), (17 * R + 77, 260), (2 * R + 1, 1028), (33 * R + 77, 5), (2 * R + 1, 64)]
    steps = []
    for rows, cols in shapes:
        c = _case(rows, cols)
        steps.append((c, torch.from_numpy(c["g"].copy()).cuda(), torch.from_numpy(c["y"].copy()).cuda(), torch.full((rows, cols), float(CANARY), device="cuda"),
                      torch.full((cols,), float(CANARY), device="cuda"), torch.from_numpy(c["old"].copy()).cuda()))
    texts = []
    with H.MMult(0, "auto") as own:
        torch.cuda.synchronize()
        for c, g, y, dz, s, s_acc in steps:
            own.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
            texts.append(H.last_launch())
            own.relu_grad_colsum(g, None, want_dz=False, bias_grad=s_acc, accumulate=True)
            texts.append(H.last_launch())
        torch.cuda.synchronize()
        for i, (c, g, y, dz, s, s_acc) in enumerate(steps):
            rows = c["g"].shape[0]
            assert f"colsum {(rows + R - 1) // R} blocks of {R} rows + finish" in texts[2 * i], (i, texts[2 * i])
            assert texts[2 * i + 1].endswith("+ finish, accumulated") and "gate off, dz not written" in texts[2 * i + 1], (i, texts[2 * i + 1])
            assert ref.same_bits(dz.cpu().numpy(), c["z_on"]), i
            assert ref.same_bits(s.cpu().numpy(), c["s_on"]), i
            assert ref.same_bits(s_acc.cpu().numpy(), c["s_off_acc"]), i


def test_mixed_alignment_takes_the_scalar_path(amm):
    """One operand off the 16-byte grid is enough: an aligned g with a y one float off."""
    import torch
    import how_to_optimize_gemm_amd as H
    c = _case(R + 1, 256)
    g = Window(torch, R + 1, 256, 260, 0, c["g"])
    y = Window(torch, R + 1, 256, 260, 1, c["y"])
    dz, s = amm.relu_grad_colsum(g.t, y.t)
    assert H.last_launch().startswith("relu_grad_colsum_kernel (scalar path)")
    assert ref.same_bits(dz.cpu().numpy(), c["z_on"]) and ref.same_bits(s.cpu().numpy(), c["s_on"])
    dz, s = amm.relu_grad_colsum(g.t, None)
    assert H.last_launch().startswith("relu_grad_colsum_kernel (vector path)")
    assert ref.same_bits(dz.cpu().numpy(), c["z_off"]) and ref.same_bits(s.cpu().numpy(), c["s_off"])


@pytest.mark.parametrize("reps", [1, 30])
def test_special_values(amm, reps):
    """y in {+0, -0, -1, +-subnormal, NaN, +-Inf, 1} crossed with g in {NaN, +-Inf, +-0, +-subnormal, 1.5}: one block
    (written by the pass) and, tiled to 270 rows, three blocks and the finish kernel -- with and without a gate."""
    import torch
    sub = np.float32(1e-45)
    ys = np.array([0.0, -0.0, -1.0, sub, -sub, np.nan, np.inf, -np.inf, 1.0], dtype=np.float32)
    gs = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub, 1.5], dtype=np.float32)
    y, g = np.meshgrid(ys, gs, indexing="ij")
    y, g = np.tile(y, (reps, 1)).copy(), np.tile(g, (reps, 1)).copy()
    for yy, gg in ((y, g), (y.T.copy(), g.T.copy())):
        for gated in (True, False):
            want_z, want_s = ref.relu_grad_colsum(gg, yy if gated else None, R)
            dz, s = amm.relu_grad_colsum(torch.from_numpy(gg).cuda(), torch.from_numpy(yy).cuda() if gated else None)
            assert ref.same_bits(dz.cpu().numpy(), want_z), (reps, gated)
            assert ref.same_bits(s.cpu().numpy(), want_s), (reps, gated, s.cpu().numpy(), want_s)
    # a column of -0 sums to -0: the chains start at their first element, not at +0
    z = np.full((2 * R + 3, 4), -0.0, dtype=np.float32)
    _, s = amm.relu_grad_colsum(torch.from_numpy(z).cuda(), None, want_dz=False)
    assert np.all(np.signbit(s.cpu().numpy()))


def test_rows_zero_and_cols_zero(amm):
    import torch
    s = torch.full((5,), 3.0, device="cuda")
    dz, out = amm.relu_grad_colsum(torch.empty((0, 5), device="cuda"), None, bias_grad=s)
    assert out is s and dz.shape == (0, 5) and np.array_equal(s.cpu().numpy(), np.zeros(5, np.float32))
    s.fill_(3.0)
    amm.relu_grad_colsum(torch.empty((0, 5), device="cuda"), None, bias_grad=s, accumulate=True)
    assert np.array_equal(s.cpu().numpy(), np.full(5, 3.0, np.float32))
    dz, out = amm.relu_grad_colsum(torch.empty((4, 0), device="cuda"), None)
    assert dz.shape == (4, 0) and out.shape == (0,)
    # the C entry point itself: rows == 0 writes +0 (not when accumulating), cols == 0 launches nothing
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    s.fill_(3.0)
    p = C.c_void_p(s.data_ptr())
    assert L.mmh_relu_grad_colsum(amm._h, 0, 5, p, 5, None, 5, None, 5, p, 1, None) == H.OK
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), np.full(5, 3.0, np.float32))
    assert L.mmh_relu_grad_colsum(amm._h, 0, 5, p, 5, None, 5, None, 5, p, 0, None) == H.OK
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), np.zeros(5, np.float32))
    s.fill_(3.0)
    assert L.mmh_relu_grad_colsum(amm._h, 7, 0, p, 0, None, 0, None, 0, p, 0, None) == H.OK
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), np.full(5, 3.0, np.float32))


def test_invalid_arguments_are_refused_with_the_outputs_untouched(amm):
    import torch
    import how_to_optimize_gemm_amd as H
    L = H.lib()
    rows, cols = 6, 8
    g = torch.ones((rows, cols), device="cuda")
    y = torch.ones((rows, cols), device="cuda")
    z = torch.full((rows, cols), 5.0, device="cuda")
    s = torch.full((cols,), 7.0, device="cuda")
    pg, py, pz, ps = (C.c_void_p(t.data_ptr()) for t in (g, y, z, s))
    call = lambda *a: L.mmh_relu_grad_colsum(amm._h, *a, None)
    assert call(rows, cols, None, cols, py, cols, pz, cols, ps, 0) == H.ERR_INVALID_ARG       # NULL dG
    assert call(rows, cols, pg, cols, py, cols, None, cols, None, 0) == H.ERR_INVALID_ARG     # both outputs NULL
    assert call(rows, cols, pg, cols - 1, py, cols, pz, cols, ps, 0) == H.ERR_INVALID_ARG     # leading dimensions below cols
    assert call(rows, cols, pg, cols, py, cols - 1, pz, cols, ps, 0) == H.ERR_INVALID_ARG
    assert call(rows, cols, pg, cols, py, cols, pz, cols - 1, ps, 0) == H.ERR_INVALID_ARG
    assert call(-1, cols, pg, cols, py, cols, pz, cols, ps, 0) == H.ERR_INVALID_ARG           # negative sizes
    assert call(rows, -1, pg, cols, py, cols, pz, cols, ps, 0) == H.ERR_INVALID_ARG
    assert L.mmh_relu_grad_colsum(None, rows, cols, pg, cols, py, cols, pz, cols, ps, 0, None) == H.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(z == 5.0).item() and torch.all(s == 7.0).item()
    # the torch glue: wrong dtype / device / shape, an expanded (overlapping) gradient, nothing wanted
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g.double(), None)
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g.cpu(), None)
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g, y[:, :4])
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(torch.ones((1, cols), device="cuda").expand(rows, cols), None)
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g, None, want_dz=False, want_colsum=False)
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g, None, accumulate=True)
    with pytest.raises(H.MMultError):
        amm.relu_grad_colsum(g, None, bias_grad=torch.zeros(cols + 1, device="cuda"))
    with pytest.raises(H.MMultError):
        amm.time_relu_grad_colsum(torch.empty((0, cols), device="cuda"), None)
    assert torch.all(z == 5.0).item() and torch.all(s == 7.0).item()


def test_time_relu_grad_colsum_runs_the_same_call(amm):
    import torch
    c = _case(2 * R + 44, 256)
    g, y = torch.from_numpy(c["g"]).cuda(), torch.from_numpy(c["y"]).cuda()
    dz, s = torch.empty_like(g), torch.empty(256, device="cuda")
    ms = amm.time_relu_grad_colsum(g, y, dz=dz, bias_grad=s, warmup=1, reps=3)
    assert ms > 0.0
    assert ref.same_bits(dz.cpu().numpy(), c["z_on"]) and ref.same_bits(s.cpu().numpy(), c["s_on"])


def test_rate_floor_against_torch_where_and_sum(amm):
    """At 4096 x 4096 the full primitive (gate + dz + column sum: g and y read, dz written -- three passes over the matrix) is
    not slower than what it replaces, torch.where(y > 0, g, 0) then .sum(0) (four passes).  Median of five interleaved
    passes of 20 calls each; the floor is 1.0, the byte ratio 4 / 3 is the margin for noise.  The printed ratio is not a pure
    4 / 3 byte-count result: torch's side also materialises the mask `y > 0` (one more launch, a byte per element written and
    read again) and is issued from Python, ours from C -- at some 100 us per call neither moves the floor."""
    import torch
    n = 4096
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn((n, n), device="cuda", generator=gen)
    y = torch.randn((n, n), device="cuda", generator=gen)
    dz, s = torch.empty_like(g), torch.empty(n, device="cuda")
    zero = torch.zeros((), device="cuda")

    def torch_ms(reps=20):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            torch.where(y > 0, g, zero).sum(0)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    torch_ms(3)
    amm.time_relu_grad_colsum(g, y, dz=dz, bias_grad=s, warmup=3, reps=3)
    ours, theirs = [], []
    for _ in range(5):
        ours.append(amm.time_relu_grad_colsum(g, y, dz=dz, bias_grad=s, warmup=0, reps=20))
        theirs.append(torch_ms())
    ratio = statistics.median(theirs) / statistics.median(ours)
    print(f"relu_grad_colsum 4096x4096: {statistics.median(ours) * 1e3:.1f} us, torch where+sum {statistics.median(theirs) * 1e3:.1f} us, "
          f"ratio {ratio:.3f}")
    assert ratio >= 1.0, (ours, theirs)
    # (and the same answer to fp32 summation accuracy -- the orders differ)
    want = torch.where(y > 0, g, zero)
    assert torch.equal(dz, want)
    assert torch.allclose(s, want.sum(0), rtol=0, atol=float(ref.gamma(R + n // R) * want.abs().sum(0).max()) * 2)
