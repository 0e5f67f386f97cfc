"""A seeded, stratified differential fuzz of the three int8 layer libraries (libmmult_hip_q8.so, _q8o.so, _q8d.so), of the 4-bit
decode library (libmmult_hip_q4d.so) and of the Python objects above them (q8.QWeight, QWeight4, QRows, qlinear, qlinear_decode)
against the numpy contracts the tables already use: tests/qlinear_ref.py, tests/qchain_ref.py, tests/qdecode_ref.py,
tests/q4_ref.py.  (Shared test code: see tests/bitcmp.py.)

The tables (tests/test_gpu_qlinear.py, test_gpu_qchain.py, test_gpu_q8o_table.py, test_gpu_qdecode.py) are thorough along each
axis but rotate their axes in lock-step; here the axes meet: shapes, the layouts of five windows, epilogues, forced split
counts, output scales and special values are combined per case.  cases() is a deterministic list -- case i belongs to stratum
i % 8, epilogues, layouts, split counts and special values cycle, only sizes and pads are drawn --, inputs() and expected()
are the host side of a case, calls() says which launches a case makes on which layouts (so that tests/test_q8_fuzz_cases.py can
prove the list's coverage on the CPU, through the libraries' own plan functions), and run_case() is the GPU runner that
tests/test_gpu_q8_fuzz.py and tools/fuzz_q8.py share.

The strata: 0 whole 128 tiles; 1 / 2 ragged small, aligned / not; 3 around the 128 tile's edges; 4 / 5 decode (1 - 16 rows),
aligned / not; 6 wide rows (the quantiser's workgroup-per-row form); 7 the 256 tile, whole or 1 - 239 rows and columns short.

The forms of a case (run_case):
  F1  q8.quantize_rows(x, out=window)                    q, scale, inv_scale; the zeroed bytes behind each row; nothing else
  F2  q8.qlinear(x, qw, bias, act, out=window)           the contract, nothing written outside the window
  F3  q8.qlinear(QRows of F1's rows, ...)                F2's bits -- or QRows' refusal of rows the GEMM cannot read in dwords
  F4  q8.qlinear(QRows, ..., out=int8 window, out_scale) requant_ref and inv_scale_ref; on quantize(x)'s default rows and on F1's
  F5  F4's QRows in place into QWeight(w2)               qlinear_s8_ref of the reference's bytes -- or _rows_args' refusal
  F6  q8.qlinear_decode (rows <= 16), both outputs       the same bits; a forced split count with an empty range is refused
  F7  the 4-bit weight (rows <= 16, libmmult_hip_q4d.so), on F6's rows, windows and split count:
      pack   q8.QWeight4(w) -- w a row-strided window in every second decode case -- every byte of the image, scale, inv_scale
      fp32 / int8   q8.qlinear_decode on it              tests/q4_ref.py's contract on the reference's packed image; the int8
                                                         output under out_scales() of the 4-bit reference's OWN fp32 result
      image  the packed bytes in a poisoned uint8 window through QWeight4.from_image: F7 fp32's and int8's bits, the window
             unchanged -- or from_image's refusal of a pitch or base the kernel cannot read in dwords
After every launching call the library's last_launch text is the text of its own plan function for that layout."""
import collections
import types
import zlib

import numpy as np

import q4_ref as P4
import qchain_ref as Q
import qdecode_ref as D
import qlinear_ref as R
from bitcmp import first_difference, same_bits

# ldx_pad / off_x, ldy_pad / off_y: floats behind a row of x / y, floats between the allocation and the base; ldyq_pad / off_yq,
# ldq_pad / off_q: the same in bytes for the int8 output window and for the stand-alone quantiser's out= (bases past a 16-byte
# boundary); bias_off: floats between the bias' allocation and its base; splits: 0 the plan's choice; scale_kind "float" / "rows":
# out_scale as a Python float / a (rows,) tensor; scale_factor: times the reference's own scale; specials: names, see inputs()
Case = collections.namedtuple("Case", "rows out in_ out2 ldx_pad off_x ldy_pad off_y ldyq_pad off_yq ldq_pad off_q bias relu bias_off "
                                      "splits scale_kind scale_factor specials")

STRATA = 8
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]   # (bias, relu)
FACTORS = (0.5, 1.0, 2.0, 8.0)
ROW_KINDS = ("all zero", "NaN", "+-inf", "max 1e-38", "-max")             # qlinear_ref.special_rows' names
BIAS_KINDS = ("NaN", "+-inf", "-0.0", "+-1e6")
# scaled values of the "ties" bias (in == 0: y is the bias): halves whose integer part is even -- where round-half-even and
# round-half-away part -- and odd; the bias also holds 127 as its maximum, so that the reference's scale is scale_factor exactly
TIES = (0.5, -2.5, 2.5, 1.5, -0.5, 4.5, -1.5)
POISON = 0x55

# the layouts that are not aligned: (leading dimension a multiple of 4, base aligned) of x, y (16-byte bases) and of the two int8
# windows (4-byte bases).  The cycles have different lengths so that the four windows' forms meet in every combination
X_FORMS = [(False, False), (True, False), (False, True)]
Y_FORMS = [(True, False), (False, True), (False, False)]
Q_FORMS = [(False, True), (True, True), (True, False), (True, True)]
YQ_FORMS = [(True, True), (False, True), (True, False)]
# the decode strata's split counts by the case's index in its stratum: "own" the plan's choice (an `in` at which it is above one),
# "in0" in == 0, "refused" a forced count that leaves a range empty -- one per 16 cases
SPLITS = {4: ("own", 2, 3, "refused", 1, "in0", 2, "refused"), 5: ("refused", 3, 1, "in0", 2, "refused", 3, "own")}


# ---- the case list ------------------------------------------------------------------------------------------------------------
def _pad(rng, n, whole):
    """Elements behind a row of n: n + pad is a multiple of 4, or is none."""
    return -n % 4 + 4 * int(rng.integers(0, 3)) + (0 if whole else int(rng.integers(1, 4)))


def _layout(rng, out, in_, aligned, u):
    """The ten layout fields.  aligned: every leading dimension a multiple of 4, fp32 bases 16-byte and int8 bases 4-byte aligned;
    else the u-th combination of the *_FORMS."""
    (xl, xb), (yl, yb) = ((True, True),) * 2 if aligned else (X_FORMS[u % 3], Y_FORMS[u % 3])
    (ql, qb), (ol, ob) = ((True, True),) * 2 if aligned else (Q_FORMS[u % 4], YQ_FORMS[u % 3])
    f32_base = lambda ok: 4 * int(rng.integers(0, 3)) if ok else int(rng.integers(1, 4)) + 4 * int(rng.integers(0, 2))
    i8_base = lambda ok: 4 * int(rng.integers(0 if aligned else 1, 4)) if ok else int(rng.integers(1, 4)) + 4 * int(rng.integers(0, 3))
    return dict(ldx_pad=_pad(rng, in_, xl), off_x=f32_base(xb), ldy_pad=_pad(rng, out, yl), off_y=f32_base(yb),
                ldyq_pad=_pad(rng, out, ol), off_yq=i8_base(ob), ldq_pad=_pad(rng, in_, ql), off_q=i8_base(qb),
                bias_off=4 * int(rng.integers(0, 2)) if aligned else int(rng.integers(1, 4)))


def _refused_splits(rng, in_):
    slices = -(-in_ // D.SLICE)
    return int(rng.choice([s for s in range(1, slices + 3) if not D.valid_splits(in_, s)]))


def _shape(rng, s, j, cus, decode_index):
    """(rows, out, in_, splits, aligned or None for "alternate") of case j of stratum s."""
    splits = 0
    if s == 0:
        rows, out = (128 * int(rng.integers(1, 4)) for _ in range(2))
        in_ = 64 * int(rng.integers(1, 6)) + (int(rng.integers(1, 4)) * (1, -1)[int(rng.integers(0, 2))] if j % 2 else 0)
        return rows, out, in_, 0, True
    if s in (1, 2):
        rows, out, in_ = int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.integers(0, 700))
        if j % 4 == (1 if s == 1 else 3):   # in == 0, once per 32 cases in each of the two strata, under a bias that holds ties
            out, in_ = max(out, 8), 0
        return rows, out, in_, 0, s == 1
    if s == 3:
        rows, out = (128 * int(rng.integers(1, 3)) + int(rng.integers(-3, 18)) for _ in range(2))
        return rows, out, 128 * int(rng.integers(1, 5)) + int(rng.integers(-3, 4)), 0, None
    if s in (4, 5):
        rows = (7 * decode_index) % D.MAX_ROWS + 1        # every count once per 16 decode cases
        out, in_ = int(rng.integers(1, 1200)), int(rng.integers(0, 1400))
        kind = SPLITS[s][j % 8]
        if kind == "in0":
            out, in_ = max(out, 8), 0
        elif kind == "own":
            in_ = int(rng.integers(max(257, 64 * rows), 1400))   # the traffic cap in / (32 rows) and the slices allow two ranges
        elif kind == "refused":
            in_ = max(in_, 1)
            splits = _refused_splits(rng, in_)
        else:
            while not D.valid_splits(in_, kind):
                in_ = int(rng.integers(1, 1400))
            splits = kind
        return rows, out, in_, splits, s == 4
    if s == 6:
        return int(rng.integers(1, 20)), int(rng.integers(1, 80)), int(rng.integers(1024, 1300)), 0, None
    (m, n, _), _ = R.shapes_256(cus)
    in_ = int(rng.integers(1, 200))
    if (j // 4) % 2 == 0:             # whole, on aligned layouts: the only way to the unguarded 256 tile, in all four epilogues
        return m, n, in_, 0, True
    for _ in range(64):
        a, b = int(rng.integers(1, 240)), int(rng.integers(1, 240))
        if R.big_tile(m - a, n - b, cus):
            return m - a, n - b, in_, 0, None
    return m - 3, n - 5, in_, 0, None   # (shapes_256's own neighbour: the same tiles)


def cases(n, seed, cus):
    """The deterministic list of n cases (a multiple of 8) for a device of `cus` compute units."""
    if n <= 0 or n % STRATA:
        raise ValueError(f"the case count is a positive multiple of {STRATA}, not {n}")
    rng = np.random.default_rng(seed)
    out, carrying = [], 0
    for i in range(n):
        s, j = i % STRATA, i // STRATA
        bias, relu = EPILOGUES[j % 4]
        rows, cols, in_, splits, aligned = _shape(rng, s, j, cus, 2 * j + (s - 4))
        if aligned is None:              # alternate, the other way round in the second four: every epilogue meets both
            aligned = (j + j // 4) % 2 == 0
        u = j if s in (2, 5) else j // 2   # which combination of the forms: every unaligned case of a stratum takes the next one
        lay = _layout(rng, cols, in_, aligned, u)
        out2 = int(rng.integers(1, 41 if s == 7 else 97))
        specials = []
        if (j + s) % 8:                  # every eighth case carries none
            t, carrying = carrying, carrying + 1
            if in_ >= 4:
                specials += ["x:" + ROW_KINDS[t % 5], "w:" + ROW_KINDS[(t + t // 5) % 5]]
            if bias and not (in_ == 0 and BIAS_KINDS[(t + t // 4) % 4] == "+-1e6"):   # (1e6 beside the ties would set the scale)
                specials.append("bias:" + BIAS_KINDS[(t + t // 4) % 4])
            if in_ == 0 and bias:
                specials.append("bias:ties")
        out.append(Case(rows, cols, in_, out2, bias=bias, relu=relu, splits=splits, scale_kind=("float", "rows")[(j // 2 + s) % 2],
                        scale_factor=FACTORS[(j + s) % 4], specials=tuple(specials), **lay))
    return out


# ---- a case's layouts and the launches it makes ---------------------------------------------------------------------------------
def layout(c):
    """The leading dimensions and base residues run_case uses, as the binding passes them on (a one-row tensor has no row stride:
    MMult._tensor_args passes its width; the int8 output of one row keeps its view's), and which forms end in a refusal."""
    L = types.SimpleNamespace()
    one = c.rows == 1
    p16 = lambda n: (n + 15) & ~15
    L.ldx = c.in_ + c.ldx_pad if c.in_ else 4          # the views' row strides
    L.ldy, L.ldy2 = c.out + c.ldy_pad, c.out2 + 4
    L.ldq = c.in_ + c.ldq_pad if c.in_ else 4
    L.ldyq = c.out + c.ldyq_pad
    L.ldx_call, L.ldq_call = (max(c.in_, 1),) * 2 if one else (L.ldx, L.ldq)        # what the calls are given
    L.ldy_call, L.ldy2_call = (c.out, c.out2) if one else (L.ldy, L.ldy2)
    # (in == 0: x and q have no bytes, and torch gives an empty tensor the address NULL whatever view it is)
    L.x16, L.y16, L.yq16 = 4 * c.off_x % 16 if c.in_ else 0, 4 * c.off_y % 16, c.off_yq % 16
    L.quant_vector = L.x16 == 0 and L.ldx_call % 4 == 0 and (c.in_ == 0 or (c.off_q % 4 == 0 and L.ldq_call % 4 == 0))
    # QRows: a row stride that is a multiple of 4 (one row: its view's where that is one, else its length rounded up) and a base that is
    L.rows_ok = c.in_ == 0 or (c.off_q % 4 == 0 and (one or L.ldq % 4 == 0))
    L.rows_ld = 0 if c.in_ == 0 else L.ldq if L.ldq % 4 == 0 else (c.in_ + 3) & ~3
    L.default_ld = p16(c.in_)
    L.chain_ok = L.ldyq % 4 == 0 and c.off_yq % 4 == 0                               # F5: the int8 window read in place
    L.decode = c.rows <= D.MAX_ROWS
    L.splits_ok = not (c.in_ > 0 and c.splits > 0 and not D.valid_splits(c.in_, c.splits))
    L.decode_ld = L.rows_ld if L.rows_ok else L.default_ld
    # F7: QWeight4 reads w in a row-strided window (x's: ldx_pad, off_x) in every second decode case -- strata 4 and 5 draw their
    # row counts 1, 8, 15, 6, ... in turn, so an even count is every second of them; the packed image goes into a uint8 window
    # of the int8 output's pitch and base, which from_image adopts where the kernel can read it in dwords (in == 0: no packed
    # rows, nothing is read, any window is taken)
    L.w4_strided = L.decode and c.rows % 2 == 0
    L.image_ok = c.in_ == 0 or (L.ldyq % 4 == 0 and c.off_yq % 4 == 0)
    return L


# form: F1 ... F7 and which call of it; lib: "q8" / "q8o" / "q8d" / "q4d"; args: the plan function's; part: "quantiser" / "gemm" / "all" of
# mmh_q8_linear_plan's text
Call = collections.namedtuple("Call", "form lib args part")


def calls(c):
    """Every launching call of run_case(c) with the arguments its library's plan function takes for the layout it runs on."""
    L = layout(c)
    # (the stand-alone quantiser takes 16-byte loads only where q's window allows dwords too: a plan with x one float off says scalar)
    quant_x16 = L.x16 if L.quant_vector or L.x16 else 4
    out = [Call("F1", "q8", (c.rows, c.out, c.in_, L.ldx_call, c.out, quant_x16, 0, False, False), "quantiser"),
           Call("F2", "q8", (c.rows, c.out, c.in_, L.ldx_call, L.ldy_call, L.x16, L.y16, c.bias, c.relu), "all")]
    if L.rows_ok:
        out.append(Call("F3", "q8", (c.rows, c.out, c.in_, max(c.in_, 1), L.ldy_call, 0, L.y16, c.bias, c.relu), "gemm"))
    out.append(Call("F4 default rows", "q8o", (c.rows, c.out, c.in_, L.default_ld, L.ldyq, c.off_yq % 4), "all"))
    if L.rows_ok:
        out.append(Call("F4 F1's rows", "q8o", (c.rows, c.out, c.in_, L.rows_ld, L.ldyq, c.off_yq % 4), "all"))
    if L.chain_ok:
        out.append(Call("F5", "q8", (c.rows, c.out2, c.out, c.out, L.ldy2_call, 0, L.y16, c.bias, c.relu), "gemm"))
    if L.decode and L.splits_ok:
        out += [Call("F6 fp32", "q8d", (c.rows, c.out, c.in_, L.decode_ld, False, L.ldy, L.y16, c.splits), "all"),
                Call("F6 int8", "q8d", (c.rows, c.out, c.in_, L.decode_ld, True, L.ldyq, L.yq16, c.splits), "all"),
                # (the image F7 runs a second time on has its own pitch; the plan's text does not depend on it)
                Call("F7 fp32", "q4d", (c.rows, c.out, c.in_, L.decode_ld, False, L.ldy, L.y16, c.splits), "all"),
                Call("F7 int8", "q4d", (c.rows, c.out, c.in_, L.decode_ld, True, L.ldyq, L.yq16, c.splits), "all")]
    return out


def _part(text, part):
    return text if part == "all" else text.split(", then ")[0 if part == "quantiser" else 1]


def library_plan(call, cus):
    """(launch text, bytes of scratch or workspace -- None for q8o, which has none) from the library's own plan function."""
    from how_to_optimize_gemm_amd import q8
    a = call.args
    if call.lib == "q8":
        text, scratch = q8.qlinear_plan(*a[:7], a[7], "relu" if a[8] else None, cus)
        return _part(text, call.part), scratch
    if call.lib == "q8o":
        return q8.qlinear_s8o_plan(a[0], a[1], a[2], ldq=a[3], ldyq=a[4], yq_mod4=a[5], cu_count=cus), None
    plan = q8.qlinear_decode4_plan if call.lib == "q4d" else q8.qlinear_decode_plan
    return plan(a[0], a[1], a[2], ldq=a[3], out8=a[4], ldo=a[5], o_mod16=a[6], splits=a[7], cu_count=cus)


def python_plan(call, cus):
    """library_plan from the Python restatements: qlinear_ref.plan_text, qchain_ref.plan_text_s8o, qdecode_ref.plan, q4_ref.plan."""
    a = call.args
    if call.lib == "q8":
        text, scratch = R.plan_text(*a, cus)
        return _part(text, call.part), scratch
    if call.lib == "q8o":
        return Q.plan_text_s8o(a[0], a[1], a[4], a[5], cus), None
    return (P4.plan if call.lib == "q4d" else D.plan)(a[0], a[1], a[2], a[4], a[5], a[6], a[7], cus)[:2]


# ---- inputs and expectations ------------------------------------------------------------------------------------------------------
# planted: special name -> the row / channel / positions; ties4: the channel of w that holds W4_TIES, or None
Inputs = collections.namedtuple("Inputs", "x w w2 bias bias2 planted ties4")
# a channel of w for the 4-bit quantiser (decode cases of in >= 4): its maximum 3.5, so that the scale is 7 / 3.5 = 2 exactly, and
# values that come to halves -- 0.5 and 2.5, where round-half-even and round-half-away part, and -1.5, where they agree
W4_TIES = (3.5, 0.25, -0.75, 1.25)


def inputs(c):
    """x ~ 3 N(0, 1), w and w2 ~ U(-0.5, 0.5), the biases ~ U(-4, 4) (test_gpu_qlinear.problem's distributions), seeded by the case's
    fields; then c.specials at random positions: "x:<kind>" / "w:<kind>" one of qlinear_ref.special_rows as a row of x / a channel of
    w; "bias:NaN", "bias:+-inf", "bias:-0.0", "bias:+-1e6" those values in the bias; "bias:ties" (in == 0, where y is the bias) 127
    and values that scale_factor brings to halves.  Last, drawing nothing: W4_TIES in the first columns of one other channel of w
    where the case runs F7 (rows <= 16, in >= 4, a channel free of the "w:" special)."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    x = (rng.standard_normal((c.rows, c.in_)) * 3).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (c.out, c.in_)).astype(np.float32)
    w2 = rng.uniform(-0.5, 0.5, (c.out2, c.out)).astype(np.float32)
    bias = rng.uniform(-4, 4, c.out).astype(np.float32)
    bias2 = rng.uniform(-4, 4, c.out2).astype(np.float32)
    free = [int(p) for p in rng.permutation(c.out)]
    planted = {}
    for name in c.specials:
        where, kind = name.split(":")
        if where in ("x", "w"):
            v = x if where == "x" else w
            r = int(rng.integers(0, v.shape[0]))
            v[r] = {n: row for n, row, _, _ in R.special_rows(c.in_, rng)}[kind]
            planted[name] = r
        else:
            values = {"NaN": [np.nan], "+-inf": [np.inf, -np.inf], "-0.0": [-0.0], "+-1e6": [1e6, -1e6],
                      "ties": [127.0] + [t / c.scale_factor for t in TIES]}[kind]
            at = [free.pop() for _ in values[:len(free)]]
            bias[at] = values[:len(at)]
            planted[name] = at
    ties4 = None
    if c.rows <= D.MAX_ROWS and c.in_ >= len(W4_TIES):
        taken = [r for n, r in planted.items() if n.startswith("w:")]
        ties4 = next((ch for ch in (free[::-1] if free else range(c.out)) if ch not in taken), None)
        if ties4 is not None:
            w[ties4, :len(W4_TIES)] = W4_TIES
    return Inputs(x, w, w2, bias, bias2, planted, ties4)


# the reference's rules, by name: a test swaps one for a wrong one to show that the case list tells the two apart
RULES = types.SimpleNamespace(quantize_rows_ref=R.quantize_rows_ref, int_sums=R.int_sums, epilogue_ref=R.epilogue_ref,
                              requant_ref=Q.requant_ref, inv_scale_ref=Q.inv_scale_ref, qlinear_s8_ref=Q.qlinear_s8_ref,
                              quantize4_ref=P4.quantize4_ref, pack_ref=P4.pack_ref, unpack_ref=P4.unpack_ref)


def _sums(rules, qx, qw):
    """rules.int_sums; a weight of ONE channel goes in twice (qdecode_ref.int_sums: its transpose has no row stride numpy would keep)."""
    return rules.int_sums(qx, qw) if qw.shape[0] != 1 else rules.int_sums(qx, np.concatenate([qw, qw]))[:, :1].copy()


def out_scales(c, y):
    """F4's output scale per row, from the reference alone: qchain_ref.scale_of_amax of the largest finite |y| -- of the row for
    "rows", of the matrix for "float" -- times scale_factor, kept finite (the header asks for a finite scale)."""
    a = np.where(np.isfinite(y), np.abs(y), np.float32(0))
    amax = a.max(axis=1) if c.scale_kind == "rows" else np.full(c.rows, a.max(), np.float32)
    with np.errstate(all="ignore"):
        so = np.array([Q.scale_of_amax(v) for v in amax], np.float32) * np.float32(c.scale_factor)
    return np.minimum(so, R.F32_MAX).astype(np.float32)


def expected(c, inp, rules=RULES):
    """One entry per form: F1 (q, scale, inv_scale); F2 y, F3 the same array; F4 (yq, inv_scale, so); F5 y2; F6 (y, yq) -- decode
    promises the tile path's bits -- or None above 16 rows; F7 (image uint8 (packed rows, out), scale, inv_scale, y4, yq4, so4) or
    None above 16 rows: q4_ref.want's steps, rule by rule (tests/test_q8_fuzz_cases.py holds the two to each other), on the
    reference's rows and the reference's packed image, so4 = out_scales() of y4 itself."""
    qx, sx, rx = rules.quantize_rows_ref(inp.x)
    qw, _, rw = rules.quantize_rows_ref(inp.w)
    y = rules.epilogue_ref(_sums(rules, qx, qw), rx, rw, inp.bias if c.bias else None, c.relu)
    so = out_scales(c, y)
    yq, inv = rules.requant_ref(y, so), rules.inv_scale_ref(so)
    w2, b2 = (inp.w2, inp.bias2) if c.out2 != 1 else (np.concatenate([inp.w2, inp.w2]), np.concatenate([inp.bias2, inp.bias2]))
    y2 = rules.qlinear_s8_ref(yq, inv, w2, b2 if c.bias else None, c.relu)[:, :c.out2].copy()
    f7 = None
    if c.rows <= D.MAX_ROWS:
        q4, s4, r4 = rules.quantize4_ref(inp.w)
        image = rules.pack_ref(np.ascontiguousarray(q4.T))
        w4 = np.ascontiguousarray(rules.unpack_ref(image, c.in_).T)   # (out, in): int_sums' layout
        y4 = rules.epilogue_ref(_sums(rules, qx, w4), rx, r4, inp.bias if c.bias else None, c.relu)
        so4 = out_scales(c, y4)
        f7 = (image, s4, r4, y4, rules.requant_ref(y4, so4), so4)
    return {"F1": (qx, sx, rx), "F2": y, "F3": y, "F4": (yq, inv, so), "F5": y2, "F6": (y, yq) if c.rows <= D.MAX_ROWS else None, "F7": f7}


# ---- the GPU runner ---------------------------------------------------------------------------------------------------------------
def _f32_window(rows, cols, ld, off, fill=None):
    """(flat, view): a NaN buffer and the rows x ld view `off` floats into it (slack behind it), `fill` in its first columns."""
    import torch
    flat = torch.full((off + rows * ld + 8,), float("nan"), device="cuda")
    view = flat[off:off + rows * ld].view(rows, ld)
    if fill is not None and cols:
        view[:, :cols] = torch.from_numpy(np.ascontiguousarray(fill)).cuda()
    return flat, view


def _i8_window(rows, ld, off):
    """(flat, view): a buffer of 0x55 and the rows x ld view `off` bytes past a 16-byte boundary of it (slack behind it)."""
    import torch
    flat = torch.full((16 + off + rows * ld + 64,), POISON, dtype=torch.int8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat, flat[16 + off:16 + off + rows * ld].view(rows, ld)


def _f32_result(flat, view, cols):
    """(the window's values on the host, nothing but the window was written); the window is NaN again afterwards."""
    import torch
    got = view[:, :cols].cpu().numpy()
    view[:, :cols] = float("nan")
    return got, bool(torch.isnan(flat).all())


def _i8_result(flat, view, cols):
    got = view[:, :cols].cpu().numpy()
    view[:, :cols] = POISON
    return got, bool((flat == POISON).all())


def _bytes_differ(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first [{bad[0][0]},{bad[0][1]}] = {got[tuple(bad[0])]}, oracle {want[tuple(bad[0])]}"


def run_case(c, cus, tally=None):
    """Run every form of the case on the current device.  Returns the list of failures (strings), never stopping at the first;
    tally, a dict, counts "forms" run, "F7" those of them that are a layer call on a 4-bit weight, and "refusals" checked.  A HIP
    error is not a failure of a form: it is raised."""
    import torch
    import how_to_optimize_gemm_amd as H
    from how_to_optimize_gemm_amd import q8
    fails = []
    tally = tally if tally is not None else {}
    L, inp = layout(c), inputs(c)
    exp = expected(c, inp)
    plans = {k.form: library_plan(k, cus)[0] for k in calls(c)}
    act = "relu" if c.relu else None

    def fail(form, *what):
        fails.append(f"{form}: " + " ".join(str(w) for w in what))

    def ran(n=1, key="forms"):
        tally[key] = tally.get(key, 0) + n

    def launched(form, text, plan=None):
        if text != plans[plan or form]:
            fail(form, f"launched {text!r}, the plan says {plans[plan or form]!r}")

    def refusal(form, call, texts_before):
        """`call` must raise MMultError(ERR_INVALID_ARG) and launch nothing: texts_before are the four last_launch texts."""
        ran(key="refusals")
        try:
            call()
        except H.MMultError as e:
            if e.status == H.ERR_HIP:
                raise
            if e.status != H.ERR_INVALID_ARG:
                fail(form, f"refused with status {e.status}, not MMH_ERR_INVALID_ARG: {e}")
        else:
            fail(form, "was not refused")
        if texts() != texts_before:
            fail(form, "a refused call changed a last_launch text")

    def attempt(form, call):
        """call(), or None after recording an MMultError that is no HIP error."""
        try:
            return call()
        except H.MMultError as e:
            if e.status == H.ERR_HIP:
                raise
            fail(form, f"raised {e}")
            return None

    def texts():
        return q8.last_launch(), q8.last_launch_q8o(), q8.last_launch_q8d(), q8.last_launch_q4d()

    def device_bias(values, n):
        if not c.bias:
            return None
        b = torch.full((c.bias_off + n + 4,), float("nan"), device="cuda")[c.bias_off:c.bias_off + n]
        b.copy_(torch.from_numpy(values))
        return b

    def scale_arg(so):
        return float(so[0]) if c.scale_kind == "float" else torch.from_numpy(so).cuda()

    def check_f32(form, flat, view, cols, want, same_as=None):
        got, clean = _f32_result(flat, view, cols)
        if not same_bits(got, want):
            fail(form, first_difference(got, want))
        if same_as is not None and not same_bits(got, same_as[1]):
            fail(form, f"differs from {same_as[0]}:", first_difference(got, same_as[1]))
        if not clean:
            fail(form, "wrote outside the window")
        return got

    def f7_ran():
        ran()
        ran(key="F7")

    def check_i8(form, flat, view, got_rows, want, want_inv, same_as=None):
        if got_rows.q.data_ptr() != view.data_ptr():
            fail(form, "the returned QRows is not the window")
        if not same_bits(got_rows.inv_scale.cpu().numpy(), want_inv):
            fail(form, "inv_scale:", first_difference(got_rows.inv_scale.cpu().numpy()[None, :], want_inv[None, :]))
        got, clean = _i8_result(flat, view, c.out)
        if not np.array_equal(got, want):
            fail(form, _bytes_differ(got, want))
        if same_as is not None and not np.array_equal(got, same_as[1]):
            fail(form, f"differs from {same_as[0]}:", _bytes_differ(got, same_as[1]))
        if not clean:
            fail(form, "wrote outside the window")
        return got

    qw = qw2 = qw4 = None
    try:
        empty = lambda n: torch.full((n, 4), float("nan"), device="cuda")[:, :0]   # an (n, 0) window with a row stride
        qw = q8.QWeight(torch.from_numpy(inp.w).cuda() if c.in_ else empty(c.out))
        _, xv = _f32_window(c.rows, c.in_, L.ldx, c.off_x, inp.x)
        x = xv[:, :c.in_]
        db, db2 = device_bias(inp.bias, c.out), device_bias(inp.bias2, c.out2)

        # F1: the stand-alone row quantiser into its own window
        want_q, want_s, want_r = exp["F1"]
        qflat, qv = _i8_window(c.rows, L.ldq, c.off_q)
        f1 = attempt("F1", lambda: q8.quantize_rows(x, out=qv[:, :c.in_]))
        rows_r = None
        if f1 is not None:
            ran()
            launched("F1", q8.last_launch())
            torch.cuda.synchronize()
            _, got_s, rows_r = f1
            want = np.full(qflat.numel(), POISON, np.int8)
            window = want[16 + c.off_q:16 + c.off_q + c.rows * L.ldq].reshape(c.rows, L.ldq)
            window[:, :c.in_] = want_q
            window[:, c.in_:min(L.ldq_call, (c.in_ + 15) & ~15)] = 0   # the header: up to 15 bytes behind each row, inside the stride
            got = qflat.cpu().numpy()
            if not np.array_equal(got, want):
                at = int(np.argwhere(got != want)[0][0]) - 16 - c.off_q
                fail("F1", f"{int((got != want).sum())} bytes of the allocation differ, first at row {at // L.ldq} column {at % L.ldq}")
            for name, g, w_ in (("scale", got_s, want_s), ("inv_scale", rows_r, want_r)):
                if not same_bits(g.cpu().numpy(), w_):
                    fail("F1", f"{name}:", first_difference(g.cpu().numpy()[None, :], w_[None, :]))

        # F2: the layer on the fp32 rows
        yflat, yv = _f32_window(c.rows, c.out, L.ldy, c.off_y)
        got_y = None
        if attempt("F2", lambda: q8.qlinear(x, qw, db, act, out=yv[:, :c.out])) is not None:
            ran()
            launched("F2", q8.last_launch())
            torch.cuda.synchronize()
            got_y = check_f32("F2", yflat, yv, c.out, exp["F2"])
        same_y = None if got_y is None else ("F2", got_y)

        # F3: the layer on F1's rows -- or QRows' refusal
        xq = None
        if rows_r is not None and L.rows_ok:
            xq = attempt("F3", lambda: q8.QRows(qv[:, :c.in_], rows_r))
            if xq is not None and attempt("F3", lambda: q8.qlinear(xq, qw, db, act, out=yv[:, :c.out])) is not None:
                ran()
                launched("F3", q8.last_launch())
                torch.cuda.synchronize()
                check_f32("F3", yflat, yv, c.out, exp["F3"], same_y)
        elif rows_r is not None:
            refusal("F3", lambda: q8.QRows(qv[:, :c.in_], rows_r), texts())

        # F4: the int8 output, on quantize(x)'s default rows and on F1's
        want_yq, want_inv, so = exp["F4"]
        oflat, ov = _i8_window(c.rows, L.ldyq, c.off_yq)
        default_rows = attempt("F4 default rows", lambda: q8.quantize(x))
        got_yq = hidden = None
        for form, rows_in in (("F4 default rows", default_rows), ("F4 F1's rows", xq)):
            if rows_in is None:
                continue
            if got_yq is not None:
                ov[:, :c.out] = POISON
            hidden = attempt(form, lambda: q8.qlinear(rows_in, qw, db, act, out=ov[:, :c.out], out_scale=scale_arg(so)))
            if hidden is None:
                continue
            ran()
            launched(form, q8.last_launch_q8o())
            torch.cuda.synchronize()
            got_yq = check_i8(form, oflat, ov, hidden, want_yq, want_inv)
            ov[:, :c.out] = torch.from_numpy(got_yq).cuda()   # (check_i8 poisoned the window: F5 reads it in place)
        same_yq = None if got_yq is None else ("F4", got_yq)

        # F5: F4's rows in place into a second layer -- or _rows_args' refusal
        if hidden is not None:
            qw2 = q8.QWeight(torch.from_numpy(inp.w2).cuda())
            y2flat, y2v = _f32_window(c.rows, c.out2, L.ldy2, c.off_y)
            if L.chain_ok:
                if attempt("F5", lambda: q8.qlinear(hidden, qw2, db2, act, out=y2v[:, :c.out2])) is not None:
                    ran()
                    launched("F5", q8.last_launch())
                    torch.cuda.synchronize()
                    # (on the reference's bytes: where F4 is wrong this form does not fail a second time for it)
                    if np.array_equal(got_yq, want_yq):
                        check_f32("F5", y2flat, y2v, c.out2, exp["F5"])
            else:
                refusal("F5", lambda: q8.qlinear(hidden, qw2, db2, act, out=y2v[:, :c.out2]), texts())
                torch.cuda.synchronize()
                if not bool(torch.isnan(y2flat).all()):
                    fail("F5", "the refused call wrote to its output")

        # F6: the small-batch layer on the same rows, both outputs -- or the refusal of a forced split count with an empty range
        rows_in = xq if xq is not None else default_rows
        if L.decode and rows_in is not None:
            if L.splits_ok:
                if attempt("F6 fp32", lambda: q8.qlinear_decode(rows_in, qw, db, act, out=yv[:, :c.out], splits=c.splits)) is not None:
                    ran()
                    launched("F6 fp32", q8.last_launch_q8d())
                    torch.cuda.synchronize()
                    check_f32("F6 fp32", yflat, yv, c.out, exp["F6"][0], same_y)
                ov[:, :c.out] = POISON
                got = attempt("F6 int8", lambda: q8.qlinear_decode(rows_in, qw, db, act, out=ov[:, :c.out], out_scale=scale_arg(so),
                                                                   splits=c.splits))
                if got is not None:
                    ran()
                    launched("F6 int8", q8.last_launch_q8d())
                    torch.cuda.synchronize()
                    check_i8("F6 int8", oflat, ov, got, exp["F6"][1], want_inv, same_yq)
            else:   # include/mmult_hip_q8d.h: MMH_ERR_INVALID_ARG where a range would be empty, no output touched
                ov[:, :c.out] = POISON
                refusal("F6 fp32", lambda: q8.qlinear_decode(rows_in, qw, db, act, out=yv[:, :c.out], splits=c.splits), texts())
                refusal("F6 int8", lambda: q8.qlinear_decode(rows_in, qw, db, act, out=ov[:, :c.out], out_scale=scale_arg(so),
                                                             splits=c.splits), texts())
                torch.cuda.synchronize()
                if not bool(torch.isnan(yflat).all()) or not bool((oflat == POISON).all()):
                    fail("F6", "a refused call wrote to its output")

        # F7: the 4-bit weight -- the packer, the layer on F6's rows and windows, the same image adopted from a poisoned window
        if L.decode:
            image, want_s4, want_r4, want_y4, want_yq4, so4 = exp["F7"]
            want_inv4 = RULES.inv_scale_ref(so4)
            if c.in_ == 0:
                w_dev = empty(c.out)
            elif L.w4_strided:
                w_dev = _f32_window(c.out, c.in_, L.ldx, c.off_x, inp.w)[1][:, :c.in_]
            else:
                w_dev = torch.from_numpy(inp.w).cuda()
            qw4 = attempt("F7 pack", lambda: q8.QWeight4(w_dev))
            if qw4 is not None:
                ran()
                torch.cuda.synchronize()
                pitch, prow, nbytes = P4.layout(c.out, c.in_)
                want_p = np.zeros((prow, pitch), np.uint8)
                want_p[:, :c.out] = image
                if (qw4.pitch, tuple(qw4.p.shape), qw4.nbytes) != (pitch, (prow, pitch), nbytes):
                    fail("F7 pack", f"pitch {qw4.pitch}, image {tuple(qw4.p.shape)}, {qw4.nbytes} bytes; the layout is {(pitch, prow, nbytes)}")
                elif not np.array_equal(qw4.p.cpu().numpy(), want_p):
                    fail("F7 pack", _bytes_differ(qw4.p.cpu().numpy(), want_p))
                for name, g, w_ in (("scale", qw4.scale, want_s4), ("inv_scale", qw4.inv_scale, want_r4)):
                    if not same_bits(g.cpu().numpy(), w_):
                        fail("F7 pack", f"{name}:", first_difference(g.cpu().numpy()[None, :], w_[None, :]))

            # the same bytes as a caller's image: from_image takes a window the kernel can read in dwords, and no other
            prow = image.shape[0]
            host = np.full(16 + c.off_yq + prow * L.ldyq + 64, POISON, np.uint8)
            host[16 + c.off_yq:16 + c.off_yq + prow * L.ldyq].reshape(prow, L.ldyq)[:, :c.out] = image
            pflat = torch.from_numpy(host).cuda()
            assert pflat.data_ptr() % 16 == 0
            pview = pflat[16 + c.off_yq:16 + c.off_yq + prow * L.ldyq].view(prow, L.ldyq)[:, :c.out]
            r4_dev = torch.from_numpy(want_r4).cuda()
            adopted = None
            if L.image_ok:
                adopted = attempt("F7 image", lambda: q8.QWeight4.from_image(pview, r4_dev, c.out, c.in_))
            else:
                refusal("F7 image", lambda: q8.QWeight4.from_image(pview, r4_dev, c.out, c.in_), texts())

            def decode4(weight, out8):
                if out8:
                    return q8.qlinear_decode(rows_in, weight, db, act, out=ov[:, :c.out], out_scale=scale_arg(so4), splits=c.splits)
                return q8.qlinear_decode(rows_in, weight, db, act, out=yv[:, :c.out], splits=c.splits)

            first = {}   # F7 fp32's and F7 int8's bits: the adopted image has to give the same
            for form, weight in (("F7", qw4), ("F7 image", adopted)):
                if weight is None or rows_in is None:
                    continue
                if L.splits_ok:
                    if attempt(form + " fp32", lambda: decode4(weight, False)) is not None:
                        f7_ran()
                        launched(form + " fp32", q8.last_launch_q4d(), "F7 fp32")
                        torch.cuda.synchronize()
                        got = check_f32(form + " fp32", yflat, yv, c.out, want_y4, first.get("fp32"))
                        first.setdefault("fp32", ("F7 fp32", got))
                    ov[:, :c.out] = POISON
                    got = attempt(form + " int8", lambda: decode4(weight, True))
                    if got is not None:
                        f7_ran()
                        launched(form + " int8", q8.last_launch_q4d(), "F7 int8")
                        torch.cuda.synchronize()
                        got = check_i8(form + " int8", oflat, ov, got, want_yq4, want_inv4, first.get("int8"))
                        first.setdefault("int8", ("F7 int8", got))
                elif weight is qw4:   # include/mmult_hip_q4d.h: MMH_ERR_INVALID_ARG where a range would be empty, no output touched
                    ov[:, :c.out] = POISON
                    refusal("F7 fp32", lambda: decode4(weight, False), texts())
                    refusal("F7 int8", lambda: decode4(weight, True), texts())
                    torch.cuda.synchronize()
                    if not bool(torch.isnan(yflat).all()) or not bool((oflat == POISON).all()):
                        fail("F7", "a refused call wrote to its output")
            torch.cuda.synchronize()
            if not np.array_equal(pflat.cpu().numpy(), host):
                fail("F7 image", "the image's window changed")
    finally:
        for weight in (qw, qw2, qw4):
            if weight is not None:
                weight.close()
    return fails
