"""Vocabulary that several per-instantiation tables share: the tile configurations the launchers instantiate, the shape
generators more than one table runs, the launchers' host arithmetic restated (window_ok, per_cu_by_lds, tail_split, dma5_form)
and the special-value inputs.  Each table, its row builder and the shapes only it runs stay in its own test_gpu_*.py.
(Shared test code: see tests/bitcmp.py.)"""
import dataclasses
import functools
import math
import re
from typing import Callable, Optional

import numpy as np

from ex_ref import COL, NONE, RELU, ROW, expected

# ---- tiles --------------------------------------------------------------------------------------------------------------
# The tile configurations the launchers instantiate (launch_dma.hip, launch_dma5.hip, launch_op.hip, launch_valu.hip);
# the symbols are spelled as tools/kernel_resources.py demangles them.
K2L_TILES = ("64,64,32,2,2,3", "128,64,32,4,2,3", "128,128,32,4,4,3")
K2W_TILES = {"64,64,32,2,2,3": "2,2", "128,64,32,4,2,3": "4,2", "128,128,32,4,4,3": "4,2",        # NL,D; with a stream-K form
             "96,96,32,3,3,3": "1,2", "96,64,32,3,2,3": "4,2", "160,160,32,5,5,3": "4,2"}        # one workgroup per tile only
K2W_SK = ("64,64,32,2,2,3", "128,64,32,4,2,3", "128,128,32,4,4,3")
OP_LAYOUTS = {1: (1, 0), 2: (0, 1), 3: (1, 1)}   # the OP template argument = transa | transb << 1
# forced kernel -> BM, BN, WTN, WTM, KB (csrc/internal.hpp reg_tiles; mfma256 is launch_reg's launch_mfma<256, 128>)
REG_TILES = {"mfma": (128, 128, 4, 4, 32), "mfma_256x256": (256, 256, 4, 8, 32), "mfma_128x64": (128, 64, 2, 4, 32),
             "mfma_64x64": (64, 64, 2, 2, 128), "mfma256": (256, 128, 4, 4, 32)}
# the K2W tiles with op, `ex` and batched forms, by forced kernel, and how a launch string spells each
OPS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}
TILES = ["mfma_64x64_dma5", "mfma_128x64_dma5", "mfma_128x128_dma5"]
FAMILY = {"mfma_64x64_dma5": "<64,64>", "mfma_128x64_dma5": "<128,64>", "mfma_128x128_dma5": "<128,128>"}
SPLIT_MARKER = "(the last round as a launch of its own)"
# the shapes of the op-form and epilogue sweeps (tests/test_gpu_op.py, tests/test_gpu_ex.py)
OP_SHAPES = [(256, 256, 256), (512, 384, 1024), (1024, 1024, 1024), (2176, 2176, 2176), (4096, 4096, 4096), (1000, 1030, 999),
             (1025, 1025, 1025), (33, 17, 5), (1, 1, 1), (7, 300, 1)]


def pair_name(ops):
    return "NT"[ops[0]] + "NT"[ops[1]]


def ex_tag(ops, alpha, beta, mode, act):
    """What the description of an `ex` launch ends in (ex_tag, csrc/launch_dma5.hpp)."""
    words = [w for on, w in ((np.float32(alpha) != 1, "alpha"), (np.float32(beta) != 0, "beta"), (mode == COL, "bias(col)"),
                             (mode == ROW, "bias(row)"), (act == RELU, "relu")) if on]
    return f", operands {pair_name(ops)}, epilogue " + (" ".join(words) or "identity")


# ---- the launchers' host arithmetic, restated ---------------------------------------------------------------------------
LIM = (1 << 31) - 4096          # csrc/internal.hpp window_ok: every byte offset of a tile below this


def window_ok(bm, bn, k, lda, ldb) -> bool:
    """csrc/internal.hpp window_ok: the buffer-descriptor path needs every byte offset of a tile inside the 2 GiB window."""
    return (bm * lda + k) * 4 < LIM and (k * ldb + bn) * 4 < LIM


def _parity(ld, guarded) -> bool:
    return ld % 2 == 1 if guarded else ld % 4 == 0


def smallest_beyond(side, bm, bn, k, guarded) -> int:
    q = LIM // 4 - 1
    ld = ((q - k) // bm if side == "a" else (q - bn) // k) + 1
    while not _parity(ld, guarded):
        ld += 1
    return ld


def per_cu_by_lds(bm, bn, kb):
    """launch_common.hpp resident_per_cu's upper bound: persistent workgroups per CU the 160 KiB of LDS allow."""
    return (160 * 1024) // (2 * kb * (bm + bn) * 4)


def tail_split(tiles, w, cus, k):
    """dma5_tail_split (csrc/internal.hpp)."""
    rem = tiles - w * cus
    return w >= 2 and k >= 512 and 100 * rem > 85 * cus and rem <= cus and (w * cus) % 8 == 0


def tail_split_case(cus):
    """(m, n, k, batch) on the 64x64 tile whose batch x tiles takes the tail split: three workgroups per CU (the 48 KiB ring) and a
    last round of one tile per CU -- batch = CUs matrices of 2 x 2 tiles.  k = 512: the rule's floor (a second launch has to be
    small beside a tile), the shallowest contraction that splits."""
    m, n, k, batch = 128, 128, 512, cus
    assert tail_split(batch * 4, 3, cus, k) and not tail_split(batch * 4, 3, cus, k - 32), ("no tail split at", m, n, k, batch)
    return m, n, k, batch


def _whole(bm, bn, ta, tb, m, n, k, batch, extra):
    """dma5_form == 0 for the batch as tests/gpu_operands.py `Batch` lays it out (device allocations are 256-byte aligned):
    whole tiles, leading dimensions, strides and bases multiples of 4 floats."""
    ra, ca = (k, m) if ta else (m, k)
    rb, cb = (n, k) if tb else (k, n)
    lda, ldb, ldc = extra.get("lda") or ca, extra.get("ldb") or cb, extra.get("ldc") or n
    sa, sb, sc = extra.get("sa", ra * lda), extra.get("sb", rb * ldb), extra.get("sc", m * ldc)
    offs = extra.get("offs", (0, 0, 0))
    tiles = m % bm == 0 and n % bn == 0 and k % 32 == 0
    return tiles and all(x % 4 == 0 for x in (lda, ldb, ldc) + tuple(offs)) and (batch == 1 or all(s % 4 == 0 for s in (sa, sb, sc)))


# ---- shapes of the LDS-DMA tiles (the NN, op and `ex` tables run them) -----------------------------------------------------
def _whole_shapes(bm, bn):
    return [(bm, bn, 32), (2 * bm, 3 * bn, 224), (8 * bm, 5 * bn, 512)]


def _edge_shapes(bm, bn):
    """Ragged m / n / k on every K-tail class, and a last tile row / column of 1, 15, 16 and 17 (K2W's thin edge tiles)."""
    return [(1, 1, 1), (bm - 1, bn + 1, 31), (bm + 1, 2 * bn - 1, 33)] + \
           [(2 * bm + r, 3 * bn + c, k) for r, c, k in ((1, 17, 64), (15, 16, 95), (16, 15, 130), (17, 1, 257))]


# the shapes the reference sweep sends to the two odd-blocked K2W tiles (mmh_auto_plan picks them there)
EXTRA = {(160, 160, False): [(2560, 2560, 2560)], (160, 160, True): [(161, 159, 33), (2561, 2559, 777)],
         (96, 64, False): [(1152, 1152, 1152)], (96, 64, True): [(97, 65, 31), (1153, 1151, 1000)]}


def _plain_shapes(bm, bn, edge):
    def shapes(cus):
        base = _edge_shapes(bm, bn) + [(bm, bn, 32)] if edge else _whole_shapes(bm, bn)
        return [(m, n, k, False) for m, n, k in base + EXTRA.get((bm, bn, edge), [])]
    return shapes


def _streamk_shapes(bm, bn, edge, persist):
    """Ragged tile counts above one per CU (forced stream-K hands tiles over between workgroups) and, with MMH_OPT_PERSIST,
    6 tiles per CU: a whole number (>= 2) of rounds of every grid the launcher can pick (1, 2 or 3 workgroups per CU)."""
    def shapes(cus):
        r = math.isqrt(cus) + 1                                  # r * r tiles: more than one per CU, fewer than two
        if edge:
            out = [((r - 1) * bm + 7, r * bn - 3, 100), (2 * r * bm + 1, (r + 1) * bn + 17, 257)]
            rounds = (6 * bm - 3, cus * bn - 1, 97)
        else:
            out = [(r * bm, r * bn, 160), ((2 * r + 1) * bm, (r + 2) * bn, 96)]
            rounds = (6 * bm, cus * bn, 96)
        return [(m, n, k, False) for m, n, k in out] + ([rounds + (True,)] if persist else [])
    return shapes


# ---- cases of the register-staged tiles (the register-staged and K1 tables run them) ---------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    m: int
    n: int
    k: int
    lda: int = 0                      # 0: run_gemm's small padded leading dimension; else A is a view of the NaN buffer
    ldb: int = 0                      # likewise B
    whole_rounds: bool = False        # stream-K rows: a whole number (>= 2) of rounds of the persistent grid (MMH_OPT_PERSIST)


def _k_tails(kb):
    """k of the four ragged shapes: a whole number of K-slices, tails of KB - 1, 1 and 2 behind two and more slices."""
    return (2 * kb, 3 * kb - 1, 2 * kb + 1, 4 * kb + 2)


def _edge_cases(bm, bn, kb):
    """_edge_shapes with K tails for the tile's own KB (the 64x64 tile's slices are 128 deep: k % 128 of 1, 127, 1, 0, 127, 1,
    2), and one whole-tile shape that only its operands' alignment makes guarded."""
    return [Case(1, 1, 1), Case(bm - 1, bn + 1, kb - 1), Case(bm + 1, 2 * bn - 1, kb + 1)] + \
           [Case(2 * bm + r, 3 * bn + c, k) for (r, c), k in zip(((1, 17), (15, 16), (16, 15), (17, 1)), _k_tails(kb))] + \
           [Case(bm, bn, kb)]


# ---- special values -------------------------------------------------------------------------------------------------------
def _special_shapes(kernel):
    """One whole-tile shape and one guarded one whose k leaves a K tail (k % 32 != 0); both reach C[70, 100]."""
    t = re.search(r"_(\d+)x(\d+)", kernel)
    bm, bn = (int(t[1]), int(t[2])) if t else (64, 64)
    wm, wn = bm * (-(-128 // bm)), bn * (-(-192 // bn))
    return [(wm, wn, 96, False), (wm + 3, wn - 5, 77, True)]


def _signed_zero_inputs(a, b):
    """Rows of A that are +0 and -0 against columns of B that are all negative and all positive: every product of
    C[+0 row, negative column] and of C[-0 row, positive column] is -0.  C0 is -0 there; the chain keeps it."""
    a, b = a.copy(), b.copy()
    m, n = a.shape[0], b.shape[1]
    rows_p, rows_n = np.arange(0, m, 5), np.arange(2, m, 5)
    cols_neg = np.arange(n) % 3 == 0
    a[rows_p] = 0.0
    a[rows_n] = -0.0
    b[:, cols_neg] = -np.abs(b[:, cols_neg]) - 0.25
    b[:, ~cols_neg] = np.abs(b[:, ~cols_neg]) + 0.25
    neg_zero = np.zeros((m, n), dtype=bool)
    neg_zero[np.ix_(rows_p, np.flatnonzero(cols_neg))] = True
    neg_zero[np.ix_(rows_n, np.flatnonzero(~cols_neg))] = True
    c0 = np.random.default_rng(5).uniform(-1, 1, (m, n)).astype(np.float32)
    c0[neg_zero] = -0.0
    return a, b, c0, neg_zero


TINY = np.finfo(np.float32).tiny


def _is_subnormal(x):
    return (x != 0) & (np.abs(x) < TINY)


def _neg_zero(x):
    return (x == 0) & np.signbit(x)


def _pos_zero(x):
    return (x == 0) & ~np.signbit(x)


@dataclasses.dataclass
class Block:
    name: str
    a: np.ndarray
    b: np.ndarray
    alpha: float
    beta: float
    c: Optional[np.ndarray]      # None: C's window is NaN (beta == 0 must not read it)
    bias: Optional[np.ndarray]
    mode: int
    act: int
    want: np.ndarray = None
    reaches: Callable = None     # reaches(want) asserts on the expectation alone that the block's class of values is really there

    def check_expectation(self):
        self.reaches(self.want)


@functools.lru_cache(maxsize=4)
def special_blocks(oracle, m, n, k):
    """The special-value blocks of one shape (m > 70, n > 100, k > 20), each with its expectation and a check of it.  The GPU
    tests of the `ex` and batched `ex` kernels run them; tests/test_ex_coverage.py checks every expectation on a machine
    without a GPU.  (This is no test module, so every assert names its block and carries the counts it judged.)"""
    f32 = np.float32
    a, b = oracle.harness_inputs(m, n, k, seed=1234 + m + n + k)
    rng = np.random.default_rng(m * n + k)
    c0 = rng.uniform(-1, 1, (m, n)).astype(f32)
    bias_n, bias_m = rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, m).astype(f32)

    def chain(x, y):
        with np.errstate(over="ignore", invalid="ignore"):
            return oracle.ref_mmult(x, y, fma=True)

    def block(name, x, y, s, alpha, beta=0.0, c=None, bias=None, mode=NONE, act=0):
        blk = Block(name, x, y, alpha, beta, c, bias, mode, act)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            blk.want = expected(s, alpha, beta, c, bias, mode, act)
        return blk

    s = chain(a, b)
    assert np.isfinite(s).all(), ("the plain chain is not finite", (m, n, k), int((~np.isfinite(s)).sum()))
    blocks = []

    # alpha == 0 is not special: 0 * s -- NaN where s is not finite, a zero of s's sign elsewhere
    a_p, b_p = a.copy(), b.copy()
    a_p[3, 5], a_p[70, 10], b_p[5, 7], b_p[20, 100] = np.inf, -np.inf, 0.0, np.nan
    s_p = chain(a_p, b_p)
    blk = block("alpha == 0", a_p, b_p, s_p, 0.0)

    def reaches(w):
        what = ("alpha == 0", (m, n, k))
        wild = ~np.isfinite(s_p)
        assert np.isnan(s_p[3, 7]) and np.isnan(s_p[:, 100]).all() and np.isinf(s_p[3]).any() and np.isinf(s_p[70]).any(), \
            (what, "the planted inf / NaN did not reach the chain", s_p[3, 7], int(np.isnan(s_p[:, 100]).sum()))
        assert np.isnan(w[wild]).all() and np.isnan(w).sum() == wild.sum() >= m + n - 1, \
            (what, "NaN where s is not finite", int(np.isnan(w).sum()), int(wild.sum()), m + n - 1)
        assert (w[~wild] == 0).all() and np.array_equal(np.signbit(w[~wild]), np.signbit(s_p[~wild])), \
            (what, "a zero of s's sign elsewhere", int((w[~wild] != 0).sum()), int((np.signbit(w[~wild]) != np.signbit(s_p[~wild])).sum()))
        assert _neg_zero(w).sum() > n and _pos_zero(w).sum() > n, (what, "zeros of both signs", int(_neg_zero(w).sum()), int(_pos_zero(w).sum()))
    blk.reaches = reaches
    blocks.append(blk)

    # signed zero through skipped operations: rows of A all +0 give s = +0 and, with alpha = -1, r1 = -0
    zero_rows = np.arange(1, m, 4)
    a_z = a.copy()
    a_z[zero_rows] = 0.0
    s_z = chain(a_z, b)
    assert _pos_zero(s_z[zero_rows]).all(), ("rows of +0 in A must give +0", (m, n, k), int((~_pos_zero(s_z[zero_rows])).sum()))
    zero_cols = np.arange(n) % 3 == 0
    bias_neg = bias_m.copy()
    bias_neg[zero_rows] = -0.0
    bias_pos = bias_n.copy()
    bias_pos[zero_cols] = 0.0
    blk = block("signed zero, nothing switched on", a_z, b, s_z, -1.0)
    blk.reaches = lambda w: _assert(_neg_zero(w[zero_rows]).all(), "signed zero, nothing switched on", (m, n, k))
    blocks.append(blk)
    blk = block("signed zero, bias -0", a_z, b, s_z, -1.0, bias=bias_neg, mode=ROW)
    blk.reaches = lambda w: _assert(_neg_zero(w[zero_rows]).all(), "signed zero, bias -0", (m, n, k))
    blocks.append(blk)
    blk = block("signed zero, bias +0", a_z, b, s_z, -1.0, bias=bias_pos, mode=COL)
    blk.reaches = lambda w: _assert(_pos_zero(w[zero_rows][:, zero_cols]).all() and zero_cols.sum() * len(zero_rows) > 0
                                             and (w[zero_rows][:, ~zero_cols] != 0).all(), "signed zero, bias +0", (m, n, k))
    blocks.append(blk)
    blk = block("signed zero, relu", a_z, b, s_z, -1.0, act=RELU)
    blk.reaches = lambda w: _assert(_pos_zero(w[zero_rows]).all(), "signed zero, relu", (m, n, k))
    blocks.append(blk)

    # beta = -0.0 is zero: C (all NaN) is not read
    blk = block("beta == -0", a, b, s, 0.7, beta=-0.0)
    blk.reaches = lambda w: _assert(not np.isnan(w).any() and (w != 0).any(), "beta == -0", (m, n, k))
    blocks.append(blk)

    # ReLU's classes, from C and the bias: alpha = -1 on the +0 rows gives r1 = -0, beta = 1 adds C's planted value, the bias -0
    # keeps it -- r3 is NaN, -inf, +inf, a negative subnormal, a positive subnormal, -0 by column
    planted = np.array([np.nan, -np.inf, np.inf, -2.0 ** -140, 3 * 2.0 ** -149, -0.0], dtype=f32)
    c_r = c0.copy()
    c_r[zero_rows] = planted[np.arange(n) % 6][None, :]
    blk = block("relu classes from C", a_z, b, s_z, -1.0, beta=1.0, c=c_r, bias=np.full(n, -0.0, f32), mode=COL, act=RELU)
    with np.errstate(invalid="ignore"):
        pre = expected(s_z, -1.0, 1.0, c_r, np.full(n, -0.0, f32), COL, 0)
    blk.reaches = lambda w: _relu_classes(pre, w)
    blocks.append(blk)

    # ... and from the product, ReLU alone switched on: r3 = -s with s = +0 (rows of +0), subnormals of both signs (a row whose
    # one nonzero element is 2^-100 against a row of B scaled by 2^-35), +inf, -inf and NaN (inf in A against a zero in B)
    a_q, b_q = a_z.copy(), b.copy()
    i_sub, i_inf, p_sub, p_inf = 2, 6, 4, 9
    a_q[i_sub] = 0.0
    a_q[i_sub, p_sub] = 2.0 ** -100
    b_q[p_sub] = b[p_sub] * f32(2.0 ** -35)
    a_q[i_inf, p_inf] = np.inf
    b_q[p_inf, 11] = 0.0
    s_q = chain(a_q, b_q)
    blk = block("relu classes from the product", a_q, b_q, s_q, -1.0, act=RELU)
    blk.reaches = lambda w: _relu_classes(-s_q, w)
    blocks.append(blk)

    # overflow inside the epilogue: fl(alpha s) = +-inf where s is finite; C (beta = 1) holds the opposite infinity on every 7th of
    # those elements, the bias holds +inf on every 5th column and -inf on every 5th + 1: NaN exactly where opposite infinities meet
    big = 3e38
    with np.errstate(over="ignore"):
        r1 = f32(big) * s
    over = np.isinf(r1)
    c_o = c0.copy()
    pick = np.zeros(m * n, bool)
    pick[np.flatnonzero(over.ravel())[::7]] = True
    pick = pick.reshape(m, n)
    c_o[pick] = -r1[pick]
    bias_o = bias_n.copy()
    bias_o[0::5], bias_o[1::5] = np.inf, -np.inf
    blk = block("overflow in the epilogue", a, b, s, big, beta=1.0, c=c_o, bias=bias_o, mode=COL)

    def reaches(w):
        what = ("overflow in the epilogue", (m, n, k))
        assert over.sum() > s.size // 2 and (r1[over] > 0).any() and (r1[over] < 0).any(), (what, "alpha s overflows", int(over.sum()), s.size)
        r2_inf = np.isinf(r1) | np.isinf(bias_o)[None, :]
        nan = pick | (over & np.isinf(bias_o)[None, :] & (np.sign(r1) != np.sign(bias_o)[None, :]))
        assert pick.sum() > 0 and (nan & ~pick).sum() > 0, (what, "opposite infinities meet", int(pick.sum()), int((nan & ~pick).sum()))
        assert np.array_equal(np.isnan(w), nan), (what, "NaN exactly there", int(np.isnan(w).sum()), int(nan.sum()))
        assert np.isinf(w[r2_inf & ~nan]).all() and np.isinf(w[over & ~nan]).sum() > 0, \
            (what, "inf elsewhere", int((~np.isinf(w[r2_inf & ~nan])).sum()), int(np.isinf(w[over & ~nan]).sum()))
    blk.reaches = reaches
    blocks.append(blk)

    # subnormal beta c beside alpha s of its size: fl(beta c) rounds (a subnormal keeps fewer bits than c has), then the sum
    # rounds -- not the one rounding of fma(beta, c, r1)
    alpha_t, beta_t = 2.0 ** -126, 2.0 ** -10
    c_t = (c0 * f32(2.0 ** -120)).astype(f32)
    blk = block("subnormal beta c", a, b, s, alpha_t, beta=beta_t, c=c_t)

    def reaches(w):
        what = ("subnormal beta c", (m, n, k))
        bc = f32(beta_t) * c_t
        r1_t = f32(alpha_t) * s
        assert _is_subnormal(bc).sum() > s.size // 2 and _is_subnormal(r1_t).sum() > 0 and (np.abs(r1_t) >= TINY).sum() > 0, \
            (what, "subnormal beta c, alpha s of both kinds", int(_is_subnormal(bc).sum()), int(_is_subnormal(r1_t).sum()), s.size)
        rounded = (bc.astype(np.float64) != np.float64(beta_t) * c_t.astype(np.float64)).sum()
        assert rounded > s.size // 4, (what, "the product rounded", int(rounded), s.size)
        rounded = (r1_t.astype(np.float64) != np.float64(alpha_t) * s.astype(np.float64)).sum()
        assert rounded > 0, (what, "alpha s rounded", int(rounded))
        # fma(beta, c, r1): exact in fp64, rounded once.  It differs from the two roundings only where the sum is normal (subnormals
        # add exactly) and fl(beta c) lands on a tie of the sum's coarser grid: one to three bits coarser here, so 1/4 .. 1/16 of
        # the elements with a normal sum -- a few percent of all
        fused = (np.float64(beta_t) * c_t.astype(np.float64) + r1_t.astype(np.float64)).astype(f32)
        assert (fused != w).sum() > s.size // 64, (what, "differs from one rounding", int((fused != w).sum()), s.size // 64)
        assert _is_subnormal(w).sum() > 0, (what, "no subnormal result")
    blk.reaches = reaches
    blocks.append(blk)
    return blocks


def _assert(ok, *what):
    assert ok, what + ("the expectation does not hold the block's class of values",)


def _relu_classes(pre, want):
    """`pre`, the value in front of ReLU, takes every class, and `want` is what the contract makes of each."""
    nan, ninf, pinf = np.isnan(pre), np.isneginf(pre), np.isposinf(pre)
    with np.errstate(invalid="ignore"):
        nsub, psub, nz = _is_subnormal(pre) & (pre < 0), _is_subnormal(pre) & (pre > 0), _neg_zero(pre)
    for name, cls in (("NaN", nan), ("-inf", ninf), ("+inf", pinf), ("negative subnormal", nsub), ("positive subnormal", psub), ("-0", nz)):
        assert cls.sum() > 0, f"no {name} in front of ReLU"
    assert np.array_equal(np.isnan(want), nan), ("NaN goes through ReLU", int(np.isnan(want).sum()), int(nan.sum()))
    assert _pos_zero(want[ninf | nsub | nz]).all(), ("-inf, negative subnormals and -0 give +0", int((~_pos_zero(want[ninf | nsub | nz])).sum()))
    assert np.isposinf(want[pinf]).all(), ("+inf stays", int((~np.isposinf(want[pinf])).sum()))
    assert np.array_equal(want[psub].view(np.uint32), pre[psub].view(np.uint32)) and _is_subnormal(want[psub]).all(), \
        ("positive subnormals stay, bit for bit", int((want[psub].view(np.uint32) != pre[psub].view(np.uint32)).sum()))
