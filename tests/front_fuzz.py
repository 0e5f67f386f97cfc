"""A seeded, stratified differential fuzz of the fp32 TENSOR front end -- the code of api.py and autograd.py that turns a torch
tensor into (pointer, leading dimension, op, batch stride, bias stride): MMult._tensor_args, _operand_args, _batched_args, _ex,
_batched_ex, addmm, baddbmm, batched_linear, relu_grad_colsum, linear_backward and autograd._LinearFn.backward -- against numpy:
the oracle's fused chain (oracle.ref_mmult, fma=True), ex_ref.expected and relu_grad_ref.  (Shared test code: see tests/bitcmp.py.)

tools/fuzz.py fuzzes the C ABI on raw pointers; here every operand is a VIEW (shape, strides, storage offset) carved from
NaN-filled storage, so a wrong stride or a dropped offset reaches C as NaN or as a neighbour's value, and every output's storage
is compared whole: the window with the expectation, the guard floats before, behind and between its rows and matrices with NaN,
bit for bit.  cases() is a deterministic list -- case i belongs to stratum i % 8 --, inputs() / expected() are the host side,
forms() names every call a case makes with the launch the addressing model below predicts for it, and run_case() is the GPU
runner tests/test_gpu_front_fuzz.py and tools/fuzz_front.py share.  tests/test_front_fuzz_cases.py proves the list's coverage.

The strata: 0 whole, 16-byte aligned tiles (2-D); 1 ragged 2-D views; 2 2-D edges: sizes 0 and 1, one row / one column read both
ways; 3 ragged batches: expanded, gapped, odd batch strides; 4 batches AUTO folds / runs as one launch, a batch of 1 cut from a
larger tensor, batch 0, k 0; 5 the backward on row-strided windows; 6 the backward's edges: rows / in / out of 0 and 1, more than one
row block; 7 refusals -- calls the host refuses before any launch.  The `loop` form of a batch needs cubes from 2176 up (half a
minute of CPU chain per matrix): it stays out and is held by test_auto_loops_over_two_large_matrices.

THE ADDRESSING MODEL (read2 / read3 / bias_reading) restates the front end's decision from shape, strides and storage offset alone,
from the header's contract and not from api.py: element (i, j) of an operand read MMH_OP_N lies at offset + i ld + j with
ld >= max(cols, 1), read MMH_OP_T at offset + j ld + i with ld >= max(rows, 1); a view both readings address (one row, one
column) is read N; one that neither addresses is refused; a batch of one has no batch stride."""
import collections
import re
import zlib

import numpy as np

import ex_ref
import relu_grad_ref as G
from bitcmp import first_difference, same_bits
from built_lib import REPO
from kernel_tables import FAMILY, TILES, ex_tag

F32 = np.float32
STRATA = 8
STRATUM_NAMES = ["whole aligned tiles", "ragged 2-D views", "2-D edges", "ragged batches", "batch forms and edges",
                 "backward on windows", "backward edges", "refusals"]
SIZES = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129)       # (0 is dealt by name in the edge strata)
RAGGED = (77, 100, 200, 257, 300)
BATCHES = (2, 3, 7)
AB = ((1.0, 1.0), (0.7, -0.5), (2.0, 0.0), (-1.3, 1.0))             # addmm / baddbmm's (alpha, beta)
PADS = (1, 3, 4, 8)                                                 # ld = cols + one of these
FRONT, BACK = 4, 8                                                  # guard floats before (a multiple of 4) and behind a view
# the kernel a form runs on: AUTO; the three K2W tiles forced, plain (stream-K off); the same with set_streamk(2)
CONFIGS = [("auto", 1)] + [(t, 0) for t in TILES] + [(t, 2) for t in TILES]
NEEDS = [(x, w, b) for x in (True, False) for w in (True, False) for b in (True, False)]
ADDMM_INPUTS = ("2-D", "2-D out=", "out is input", "(n,) bias", "(n,) copy")
BADDBMM_INPUTS = ("full", "out is input", "(n,)", "(batch,1,n) strided", "(batch,1,n) expanded", "(m,1)", "(1,n)", "(batch,1,1)")
REFUSALS = ("no unit stride", "overlapping rows of out", "overlapping matrices of out", "wrong dtype", "CPU tensor",
            "non-dense bias", "inner dimensions disagree", "batch dimensions disagree")
R_BLOCK = G.header_block_rows(REPO)

# shape, strides (floats), offset (floats into the storage), size (floats of storage)
View = collections.namedtuple("View", "shape strides offset size")
# a case: kinds -- operand name -> the view class's name (for the coverage test); views -- operand name -> View
Case = collections.namedtuple("Case", "index stratum family batch m n k ab relu bias side_stream kinds views refusal")
# what the model says a tensor is read as; op 0 = N, 1 = T
Addr = collections.namedtuple("Addr", "offset ld op bstride")
# the launch the model predicts for a form: call "nn" / "op" / "ex" / "batched" / "batched_ex"; bases: the three operands' float
# offsets (None: address 0); epilogue (alpha, beta, bias mode, act) or None
Launch = collections.namedtuple("Launch", "call ta tb m n k lda ldb ldc bases batch sa sb sc sbias epilogue")
Form = collections.namedtuple("Form", "name entry launch")


# ---- views ----------------------------------------------------------------------------------------------------------------------
def _window(rng, rows, cols, kind):
    """(ld, off) of a row-major (rows, cols) window: kind "c" contiguous, "a" row-strided and aligned (ld = cols + 4 or 8), "r"
    row-strided (any of PADS), "o" a storage offset of 1 - 3 floats, "ro" both."""
    pad = PADS[int(rng.integers(0, 4))] if "r" in kind else (4, 8)[int(rng.integers(0, 2))] if "a" in kind else 0
    return max(cols, 1) + pad, int(rng.integers(1, 4)) if "o" in kind else 0


def view2(rng, rows, cols, kind):
    """A 2-D view of the kind; "t" + kind: the .t() of such a (cols, rows) window."""
    t = kind.startswith("t")
    r, c = (cols, rows) if t else (rows, cols)
    ld, off = _window(rng, r, c, kind[1:] if t else kind)
    return View((rows, cols), (1, ld) if t else (ld, 1), FRONT + off, FRONT + off + max(r - 1, 0) * ld + c + BACK)


def view3(rng, batch, rows, cols, kind, bkind):
    """A 3-D view: every matrix a view2 of `kind`; bkind "packed", "gapped" (a multiple of 4 floats between matrices), "odd" (a
    batch stride that is no multiple of 4), "expand" (stride 0), "slice1" (a batch of one that keeps a larger tensor's stride)."""
    v = view2(rng, rows, cols, kind)
    t = kind.startswith("t")
    r, c = (cols, rows) if t else (rows, cols)
    ld = v.strides[1] if t else v.strides[0]
    packed = r * ld
    if bkind == "odd":
        sb = packed + 1 + (1 if (packed + 1) % 4 == 0 else 0)
    else:
        sb = {"packed": packed, "gapped": packed + 4 * int(rng.integers(1, 4)), "expand": 0, "slice1": packed + 5}[bkind]
    return View((batch,) + v.shape, (sb,) + v.strides, v.offset, v.offset + max(batch - 1, 0) * sb + max(r - 1, 0) * ld + c + BACK)


def vector(rng, shape, strides, off=None):
    """A view of any rank with the given strides, `off` (1 - 3 drawn if None) floats past the front guard."""
    off = int(rng.integers(1, 4)) if off is None else off
    reach = sum(max(n - 1, 0) * s for n, s in zip(shape, strides)) + 1
    return View(tuple(shape), tuple(strides), FRONT + off, FRONT + off + reach + BACK)


def indices(shape, strides, offset):
    """The flat index of every element of a view."""
    idx = np.full(shape, offset, np.int64)
    for axis, (n, s) in enumerate(zip(shape, strides)):
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape([n if a == axis else 1 for a in range(len(shape))])
    return idx


def lay(view, values=None):
    """The view's storage on the host: NaN, `values` at the view's elements."""
    flat = np.full(view.size, np.nan, F32)
    if values is not None and np.asarray(values).size:
        flat[indices(*view[:3])] = values
    return flat


def gather(flat, idx):
    """flat[idx] with NaN for every index outside the storage."""
    ok = (idx >= 0) & (idx < flat.size)
    return np.where(ok, flat[np.where(ok, idx, 0)], F32(np.nan)).astype(F32)


# ---- the addressing model ---------------------------------------------------------------------------------------------------------
def read2(shape, strides, offset, operand):
    """Addr of a 2-D tensor (bstride 0), None where the front end must refuse it.  operand: a transposed reading is allowed."""
    (rows, cols), (s0, s1) = shape, strides
    if (cols <= 1 or s1 == 1) and (rows <= 1 or s0 >= max(cols, 1)):
        return Addr(offset, s0 if rows > 1 else max(cols, 1), 0, 0)
    if operand and (rows <= 1 or s0 == 1) and (cols <= 1 or s1 >= max(rows, 1)):
        return Addr(offset, s1 if cols > 1 else max(rows, 1), 1, 0)
    return None


def read3(shape, strides, offset, operand):
    """Addr of a 3-D tensor: the matrices as read2 reads them, the batch stride as given -- none for a batch of one."""
    a = read2(shape[1:], strides[1:], offset, operand)
    return None if a is None else a._replace(bstride=strides[0] if shape[0] > 1 else 0)


def read(view, operand=True):
    return (read2 if len(view.shape) == 2 else read3)(view.shape, view.strides, view.offset, operand)


def model_indices(addr, shape):
    """The flat indices the kernels read for a tensor of `shape` through the model's reading."""
    batch, rows, cols = (1,) + tuple(shape) if len(shape) == 2 else shape
    i, r, c = np.ogrid[:batch, :rows, :cols]
    idx = addr.offset + i * addr.bstride + (c * addr.ld + r if addr.op else r * addr.ld + c)
    return idx.reshape(shape).astype(np.int64)


def bias_reading(view, batch, n, beta, out_is_input):
    """addmm / baddbmm's `input` as the front end must take it: ("bias", offset, bias stride) -- the kernel's column bias, read
    in place -- or ("copy",): broadcast into out and scaled by beta -- or ("in place",)."""
    if out_is_input:
        return ("in place",)
    shape = view.shape
    if beta == 1.0 and n >= 1 and (shape == (n,) or (batch is not None and shape == (batch, 1, n))):
        return ("bias", view.offset, view.strides[0] if len(shape) == 3 and batch > 1 else 0)
    return ("copy",)


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def _draw(rng, pool):
    return int(pool[int(rng.integers(0, len(pool)))])


K2 = ("c", "r", "o", "ro", "tc", "tr", "to", "tro")      # an operand's 2-D view classes
KC = ("c", "r", "o", "ro")                                # a row-major window's (out, input, g, y, x, w)
BK = ("packed", "gapped", "odd", "expand")


def _case2d(rng, m, n, k, ka, kb, kc, kin):
    views = {"a": view2(rng, m, k, ka), "b": view2(rng, k, n, kb), "c": view2(rng, m, n, kc), "inp": view2(rng, m, n, kin),
             "vec": vector(rng, (n,), (1,)), "bias": vector(rng, (n,), (1,))}
    return dict(family="2d", batch=None, m=m, n=n, k=k, kinds={"a": ka, "b": kb, "c": kc, "inp": kin}, views=views)


def _case3d(rng, batch, m, n, k, ka, kb, kc, ba, bb, bc, lb):
    """lb: batched_linear's bias -- "packed" / "strided" (batch, n), "shared" (n,) or None."""
    views = {"a": view3(rng, batch, m, k, ka, ba), "b": view3(rng, batch, k, n, kb, bb), "c": view3(rng, batch, m, n, kc, bc),
             "inp": view3(rng, batch, m, n, KC[(m + n) % 4], ("packed", "gapped", "odd")[(m + k) % 3] if batch != 1 else "slice1"),
             "vec": vector(rng, (n,), (1,)), "pm": vector(rng, (batch, 1, n), (n + 3, n, 1)),
             "pe": vector(rng, (batch, 1, n), (0, n, 1)), "m1": vector(rng, (m, 1), (1, 1)), "1n": vector(rng, (1, n), (n, 1)),
             "b11": vector(rng, (batch, 1, 1), (1, 1, 1))}
    if lb is not None:
        views["bias"] = vector(rng, (n,), (1,)) if lb == "shared" else vector(rng, (batch, n), (n + (3 if lb == "strided" else 0), 1))
    return dict(family="3d", batch=batch, m=m, n=n, k=k, views=views,
                kinds={"a": ka + "/" + ba, "b": kb + "/" + bb, "c": kc + "/" + bc, "bias": str(lb)})


def _caseback(rng, rows, n_in, n_out, kg, ky, kx, kw):
    views = {"g": view2(rng, rows, n_out, kg), "y": view2(rng, rows, n_out, ky), "x": view2(rng, rows, n_in, kx),
             "w": view2(rng, n_out, n_in, kw), "dz": view2(rng, rows, n_out, KC[(rows + n_in) % 4]),
             "gw": view2(rng, n_out, n_in, KC[(rows + n_out) % 4]), "gb": vector(rng, (n_out,), (1,)),
             "bias": vector(rng, (n_out,), (1,)), "t": view2(rng, n_out, rows, "c"), "G": view2(rng, rows, n_out, "c")}
    return dict(family="back", batch=None, m=rows, n=n_out, k=n_in, views=views, kinds={"g": kg, "y": ky, "x": kx, "w": kw})


def _fold_or_one_launch(rng, want, ex, cus):
    """A batch mmh_auto_plan_batched(_ex) plans as `want`, found among a few drawn shapes by the plan function itself (host
    arithmetic); the shape drawn last if the library is not there to ask."""
    for _ in range(32):
        batch, m, n, k = _draw(rng, BATCHES), _draw(rng, (33, 64, 65, 127, 128)), _draw(rng, (63, 64, 129)), _draw(rng, (31, 64, 65))
        tb = int(rng.integers(0, 2))
        try:
            import how_to_optimize_gemm_amd as H
            plan = H.auto_plan_batched_ex if ex else H.auto_plan_batched
            form = plan(0, tb, m, n, k, stride_b=0 if want == "fold" else -1, batch=batch, cu_count=cus)[1]
        except Exception:   # (no library: the GPU run and the coverage test, which need it, see the real plan)
            break
        if form == want:
            break
    return batch, m, n, k, tb


def cases(count, seed, cus):
    """The deterministic list of `count` cases (a multiple of 8) for a device of `cus` compute units (only stratum 4 asks)."""
    if count <= 0 or count % STRATA:
        raise ValueError(f"the case count is a positive multiple of {STRATA}, not {count}")
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        s, j = i % STRATA, i // STRATA
        refusal = None
        if s == 0:      # whole tiles, 16-byte aligned: contiguous or ld = cols + 4 / 8, row-major and transposed
            m, n, k = 128 * int(rng.integers(1, 4)), 128 * int(rng.integers(1, 4)), 32 * int(rng.integers(1, 7))
            kk = ("c", "a", "tc", "ta")
            c = _case2d(rng, m, n, k, kk[j % 4], kk[(j // 2 + j) % 4], ("c", "a")[j % 2], ("a", "c")[j % 2])
        elif s == 1:
            m, n, k = (_draw(rng, SIZES[1:] + RAGGED) for _ in range(3))
            c = _case2d(rng, m, n, k, K2[j % 8], K2[(3 * j + 1 + j // 8) % 8], KC[(j + 1) % 4], KC[(j + j // 4) % 4])
        elif s == 2:    # sizes 0 and 1; one row and one column, each as a window of a larger matrix and as the .t() of one
            m, n, k = (_draw(rng, SIZES[:8]) for _ in range(3))
            e = j % 8
            m, n, k = [(0, n, k), (m, 0, k), (m, n, 0), (1, 1, 1), (1, n, k), (m, 1, k), (m, n, 1), (1, 1, k)][e]
            ka, kb = [("r", "tr"), ("tr", "ro"), ("r", "tr"), ("ro", "tr"), ("tr", "r"), ("ro", "tr"), ("r", "tr"), ("r", "r")][e]
            if j % 16 >= 8:
                ka, kb = ("tr" if ka == "r" else "r" if ka == "tr" else ka), ("tr" if kb == "r" else "r" if kb == "tr" else kb)
            c = _case2d(rng, m, n, k, ka, kb, KC[(j + 1) % 4], KC[j % 4])
        elif s == 3:
            batch, (m, n, k) = BATCHES[j % 3], (_draw(rng, SIZES[2:] + RAGGED[:2]) for _ in range(3))
            ba, bb = [("expand", "odd"), ("gapped", "expand"), ("expand", "expand"), ("odd", "gapped"), ("packed", "odd")][j % 5]
            ka, kb = K2[(j + 2) % 8], K2[(3 * j) % 8]
            if j % 8 == 1:      # the readings stratum 2 has no room for: A's matrices one column as the .t() of a row, B's one row
                k, ka, kb = 1, "tr", "r"
            c = _case3d(rng, batch, m, n, k, ka, kb, KC[j % 4], ba, bb, ("odd", "gapped", "packed")[j % 3],
                        ("strided", "packed", "shared", None)[j % 4])
        elif s == 4:
            e = j % 8
            if e in (0, 1, 4, 5):   # fold: B shared, A and C packed; one launch: a matrix each
                want = "fold" if e in (0, 4) else "one_launch"
                batch, m, n, k, tb = _fold_or_one_launch(rng, want, e >= 4, cus)
                if e == 5:          # ... whole and aligned
                    m, n, k = 128, 128, 64
                c = _case3d(rng, batch, m, n, k, "c", "tc" if tb else "c", "c", "packed", "expand" if want == "fold" else "packed",
                            "packed", ("shared", None)[e // 4] if want == "fold" else "packed")
            else:
                batch, (m, n, k) = {2: 1, 3: 0, 6: 1, 7: 2}[e], (_draw(rng, SIZES[2:9]) for _ in range(3))
                if e == 7:
                    k = 0
                bk = "slice1" if batch == 1 else "packed"
                c = _case3d(rng, batch, m, n, k, K2[(j + e) % 8], K2[(j + 3) % 8], KC[j % 4], bk, bk, bk, ("packed", "strided")[e % 2])
        elif s in (5, 6):
            rows, n_in, n_out = (_draw(rng, SIZES[1:] + RAGGED[:3]) for _ in range(3))
            if s == 6:
                e = j % 8
                rows, n_in, n_out = [(0, n_in, n_out), (rows, 0, n_out), (rows, n_in, 0), (1, n_in, n_out), (rows, 1, n_out),
                                     (rows, n_in, 1), (1, 1, 1), (2 * R_BLOCK + 5, 33, 17)][e]
            c = _caseback(rng, rows, n_in, n_out, KC[j % 4], KC[(j + 1 + j // 4) % 4], KC[(j + 2) % 4], KC[(3 * j + 1) % 4])
        else:
            refusal = REFUSALS[j % 8]
            m, n, k = (_draw(rng, SIZES[2:8]) for _ in range(3))
            c = _case3d(rng, 3, m, n, k, "c", "c", "r", "packed", "packed", "gapped", "packed")
            c["family"] = "refuse"
        out.append(Case(index=i, stratum=s, ab=AB[(j + s) % 4], relu=bool((j + s // 2) % 2), bias=bool((j // 2 + s) % 2),
                        side_stream=bool((j + s) % 2), refusal=refusal, **c))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """name -> logical float32 array for every view of the case, seeded by the case: U(-1, 1), every matrix and every bias row
    different (an expanded view: one matrix, broadcast).  Planted: in `a` (`g` for the backward) a row of zeros of both signs and
    one NaN in another row; in `inp` / `c0` -0.0 under the row of zeros (alpha < 0, beta = 1 keeps it: -0 + -0); the backward's `y`
    is a ReLU image (zeros of both signs).  "planted": {"zero row": r or None, "nan": (r, p) or None}."""
    rng = np.random.default_rng(zlib.crc32(repr((c.index, c.family, c.batch, c.m, c.n, c.k, c.views)).encode()))
    v = {}
    for name, view in c.views.items():
        shape = tuple(1 if s == 0 and n > 1 else n for n, s in zip(view.shape, view.strides))
        v[name] = np.broadcast_to(rng.uniform(-1, 1, shape).astype(F32), view.shape).copy()
    if c.family in ("2d", "3d", "refuse"):
        v["c0"] = rng.uniform(-1, 1, c.views["c"].shape).astype(F32)
    planted = {"zero row": None, "nan": None}
    main = v["g" if c.family == "back" else "a"]
    rows, cols = main.shape[-2:]
    if rows >= 3 and cols >= 1 and main.size:
        zr, nr, p = int(rng.integers(0, rows)), int(rng.integers(0, rows)), int(rng.integers(0, cols))
        nr = nr if nr != zr else (zr + 1) % rows
        if c.family == "back":
            main[zr, ::2] = F32(-0.0)
        else:
            main[..., zr, :] = F32(0.0)
            main[..., zr, ::2] = F32(-0.0)
            for name in ("inp", "c0"):
                v[name][..., zr, :] = F32(-0.0)
        main[..., nr, p] = F32(np.nan)
        planted = {"zero row": zr, "nan": (nr, p)}
    if c.family == "back":
        y = np.maximum(v["y"], 0).astype(F32)
        y[..., 1::3] = np.where(y[..., 1::3] == 0, F32(-0.0), y[..., 1::3])
        v["y"] = y
    v["planted"] = planted
    return v


# ---- expectations -----------------------------------------------------------------------------------------------------------------
def chain(a, b, c0=None):
    """The oracle's fused chain of a @ b (started at c0); an empty contraction is +0 (c0); an empty result is empty."""
    from oracle import oracle as O
    (m, k), n = a.shape, b.shape[1]
    if m == 0 or n == 0 or k == 0:
        return np.zeros((m, n), F32) if c0 is None else np.array(c0, F32)
    with np.errstate(all="ignore"):
        fresh = lambda x: np.array(x, F32, order="C")    # (a copy: a fresh array's strides are the packed ones, a view's .T's are not)
        return O.ref_mmult(fresh(a), fresh(b), None if c0 is None else fresh(c0), fma=True)


def _ex(s, alpha, beta, c, bias, act):
    with np.errstate(all="ignore"):
        return ex_ref.expected(s, alpha, beta, c, bias, ex_ref.NONE if bias is None else ex_ref.COL, ex_ref.RELU if act else 0)


def vec_ab(c, bias_path):
    """(alpha, beta) of addmm's (n,) forms: beta = 1 for the bias path, the case's beta -- -0.5 where that is 1 -- for the copy."""
    alpha, beta = c.ab
    return (alpha, 1.0) if bias_path else (alpha, beta if beta != 1.0 else -0.5)


def bias_beta(c):
    """beta of baddbmm's bias-shaped inputs: 1 (the bias path) in even cases, the case's own (a copy unless it is 1) in odd ones."""
    return 1.0 if (c.index // STRATA) % 2 == 0 else c.ab[1]


def expected(c, v, wrong=None):
    """form name -> expectation (float32 arrays; tuples for the backward), from the logical arrays `v` alone.  wrong: one of the
    wrong rules tests/test_front_fuzz_cases.py tells from the true ones ("beta input lost", "(n,) unscaled as a bias", "grad_w= as a
    chain started at grad_w", "an expanded grad_out read with its strides as given")."""
    e = {}
    alpha, beta = c.ab
    if c.family in ("2d", "3d"):
        mats = [None] if c.family == "2d" else range(c.batch)
        at = lambda x, i: x if i is None else x[i]
        s = [chain(at(v["a"], i), at(v["b"], i)) for i in mats]
        acc = [chain(at(v["a"], i), at(v["b"], i), at(v["c0"], i)) for i in mats]
        pack = lambda xs: xs[0] if c.family == "2d" else (np.stack(xs) if xs else np.zeros(v["c0"].shape, F32))
        shape = v["c0"].shape

        def full(al, be, inp, in_place=False):      # `input` broadcast to the output; beta == 0: not read
            if be == 0 or (wrong == "beta input lost" and not in_place):
                return pack([_ex(s[j], al, 0.0, None, None, 0) for j, i in enumerate(mats)])
            b3 = np.broadcast_to(inp, shape)
            return pack([_ex(s[j], al, be, at(b3, i), None, 0) for j, i in enumerate(mats)])

        def biased(al, bias_of, act=0):
            return pack([_ex(s[j], al, 0.0, None, bias_of(i), act) for j, i in enumerate(mats)])
    if c.family == "2d":
        e["matmul"] = e["matmul out="] = s[0]
        e["matmul accumulate"] = acc[0]
        e["addmm 2-D"] = e["addmm 2-D out="] = full(alpha, beta, v["inp"])
        e["addmm out is input"] = full(alpha, beta, v["inp"], in_place=True)
        al, be = vec_ab(c, True)
        e["addmm (n,) bias"] = biased(al, lambda i: v["vec"])
        al, be = vec_ab(c, False)
        e["addmm (n,) copy"] = biased(al, lambda i: v["vec"]) if wrong == "(n,) unscaled as a bias" else full(al, be, v["vec"][None, :])
        e["linear"] = biased(1.0, lambda i: v["bias"] if c.bias else None, c.relu)
    elif c.family == "3d":
        e["bmm"] = e["bmm out="] = pack(s)
        e["bmm accumulate"] = pack(acc)
        e["baddbmm full"] = full(alpha, beta, v["inp"])
        e["baddbmm out is input"] = full(alpha, beta, v["inp"], in_place=True)
        bb = bias_beta(c)
        for name, key, bias_of in (("(n,)", "vec", lambda i: v["vec"]), ("(batch,1,n) strided", "pm", lambda i: v["pm"][i, 0]),
                                   ("(batch,1,n) expanded", "pe", lambda i: v["pe"][i, 0])):
            e["baddbmm " + name] = biased(alpha, bias_of) if bb == 1.0 else full(alpha, bb, v[key])
        for name, key in (("(m,1)", "m1"), ("(1,n)", "1n"), ("(batch,1,1)", "b11")):
            e["baddbmm " + name] = full(alpha, beta, v[key])
        lb = c.kinds["bias"]
        e["batched_linear"] = biased(1.0, lambda i: None if lb == "None" else v["bias"] if lb == "shared" else v["bias"][i], c.relu)
    elif c.family == "back":
        g, y, x, w = v["g"], (v["y"] if c.relu else None), v["x"], v["w"]
        dz = G.gate(g, y)
        e["relu_grad_colsum"] = (dz, G.blocked_colsum(dz, R_BLOCK))
        e["relu_grad_colsum dz=g"] = (dz, G.blocked_colsum(dz, R_BLOCK))
        e["relu_grad_colsum want_dz=False accumulate"] = (None, G.blocked_colsum(dz, R_BLOCK, v["gb"]))
        e["relu_grad_colsum want_colsum=False"] = (dz, None)
        dx, dw, db = chain(dz, w), chain(dz.T, x), G.blocked_colsum(dz, R_BLOCK)
        for need in NEEDS:
            e[f"linear_backward need={need}"] = tuple(r if on else None for r, on in zip((dx, dw, db), need))
        with np.errstate(all="ignore"):
            gw = chain(dz.T, x, v["gw"]) if wrong == "grad_w= as a chain started at grad_w" else v["gw"] + dw
        e["linear_backward grad_w= grad_b="] = (dx, gw, G.blocked_colsum(dz, R_BLOCK, v["gb"]))
        fwd = _ex(chain(x, w.T), 1.0, 0.0, None, v["bias"] if c.bias else None, c.relu)
        ones = np.ones(g.shape, F32)
        if wrong == "an expanded grad_out read with its strides as given":   # one float of storage, both strides 0, read as packed rows
            ones = gather(np.ones(1, F32), model_indices(Addr(0, max(g.shape[1], 1), 0, 0), g.shape))
        for kind, grad in (("contiguous", v["G"]), ("expanded", ones), ("transposed", v["t"].T)):
            z = G.gate(grad, fwd if c.relu else None)
            e["autograd " + kind] = (fwd, chain(z, w), chain(z.T, x), G.blocked_colsum(z, R_BLOCK) if c.bias else None)
    return e


# ---- the calls of a case and the launches the model predicts -------------------------------------------------------------------------
def config_of(c, number):
    """(kernel, stream-K option) of the case's form `number`: the seven CONFIGS in turn."""
    return CONFIGS[(c.index + c.index // STRATA + number) % len(CONFIGS)]


def _launch(call, a, b, cv, m, n, k, batch=None, sbias=0, epilogue=None):
    """The Launch of a GEMM on views a (m, k), b (k, n), out cv, or None where the call launches nothing (an empty size) or the
    kernel's text is not the tiles' (k == 0)."""
    ra, rb, rc = read(a), read(b), read(cv, False)
    if 0 in (m, n, k) or batch == 0:
        return None
    return Launch(call, ra.op, rb.op, m, n, k, ra.ld, rb.ld, rc.ld, (ra.offset, rb.offset, rc.offset), batch, ra.bstride, rb.bstride,
                  rc.bstride, sbias, epilogue)


def packed_view(shape):
    """What torch.empty(shape) is: contiguous, at the start of its own allocation."""
    strides, s = [], 1
    for n in reversed(shape):
        strides.insert(0, s)
        s *= max(n, 1)
    return View(tuple(shape), tuple(strides), 0, max(s, 1))


def forms(c):
    """Every form run_case(c) runs, in order, with the launch its LAST GEMM is predicted to be (None: no tile launch to hold)."""
    V, out = c.views, []
    add = lambda name, entry, launch=None: out.append(Form(name, entry, launch))
    alpha, beta = c.ab
    m, n, k = c.m, c.n, c.k
    if c.family == "2d":
        new = packed_view((m, n))
        plain = lambda cv: _launch("nn" if (read(V["a"]).op, read(V["b"]).op) == (0, 0) else "op", V["a"], V["b"], cv, m, n, k)
        ex = lambda cv, al, be, mode, act=0: _launch("ex", V["a"], V["b"], cv, m, n, k, epilogue=(al, be, mode, act))
        add("matmul", "matmul", plain(new))
        add("matmul out=", "matmul", plain(V["c"]))
        add("matmul accumulate", "matmul", plain(V["c"]))
        add("addmm 2-D", "addmm", ex(new, alpha, beta, 0))
        add("addmm 2-D out=", "addmm", ex(V["c"], alpha, beta, 0))
        add("addmm out is input", "addmm", ex(V["inp"], alpha, beta, 0))
        add("addmm (n,) bias", "addmm", ex(V["c"], vec_ab(c, True)[0], 0.0, 1))
        add("addmm (n,) copy", "addmm", ex(new, *vec_ab(c, False), 0))
        add("linear", "linear", ex(V["c"] if c.index % 3 else new, 1.0, 0.0, 1 if c.bias else 0, int(c.relu)))
    elif c.family == "3d":
        new = packed_view((c.batch, m, n))
        plain = lambda cv: _launch("batched", V["a"], V["b"], cv, m, n, k, c.batch)
        ex = lambda cv, al, be, mode, sbias=0, act=0: _launch("batched_ex", V["a"], V["b"], cv, m, n, k, c.batch, sbias, (al, be, mode, act))
        add("bmm", "bmm", plain(new))
        add("bmm out=", "bmm", plain(V["c"]))
        add("bmm accumulate", "bmm", plain(V["c"]))
        add("baddbmm full", "baddbmm", ex(V["c"], alpha, beta, 0))
        add("baddbmm out is input", "baddbmm", ex(V["inp"], alpha, beta, 0))
        bb = bias_beta(c)
        for name, key in (("(n,)", "vec"), ("(batch,1,n) strided", "pm"), ("(batch,1,n) expanded", "pe")):
            kind = bias_reading(V[key], c.batch, n, bb, False)
            add("baddbmm " + name, "baddbmm", ex(new, alpha, 0.0, 1, kind[2]) if kind[0] == "bias" else ex(new, alpha, bb, 0))
        for name in ("(m,1)", "(1,n)", "(batch,1,1)"):
            add("baddbmm " + name, "baddbmm", ex(V["c"], alpha, beta, 0))
        lb = c.kinds["bias"]
        sbias = V["bias"].strides[0] if lb in ("packed", "strided") and c.batch > 1 else 0
        add("batched_linear", "batched_linear", ex(V["c"] if c.index % 3 else new, 1.0, 0.0, 0 if lb == "None" else 1, sbias, int(c.relu)))
    elif c.family == "back":
        for name in ("relu_grad_colsum", "relu_grad_colsum dz=g", "relu_grad_colsum want_dz=False accumulate", "relu_grad_colsum want_colsum=False"):
            add(name, "relu_grad_colsum")
        for need in NEEDS:
            add(f"linear_backward need={need}", "linear_backward")
        add("linear_backward grad_w= grad_b=", "linear_backward")
        for kind in ("contiguous", "expanded", "transposed"):
            add("autograd " + kind, "autograd.linear")
    else:
        add("refusal: " + c.refusal, "refusal")
    return out


def base_align(bases):
    """16 where every operand's base is 16-byte aligned (storage is; an empty tensor's address is 0), else 4."""
    return 16 if all(b is None or b % 4 == 0 for b in bases) else 4


def plan_of(L, cus):
    """(short kernel name, batched form or None) of the model's launch on AUTO, from the library's own plan functions."""
    import how_to_optimize_gemm_amd as H
    kw = dict(lda=L.lda, ldb=L.ldb, ldc=L.ldc, base_align=base_align(L.bases), cu_count=cus)
    if L.call == "nn":
        return H.auto_plan(L.m, L.n, L.k, **kw)[0], None
    if L.call in ("op", "ex"):
        return (H.auto_plan_op if L.call == "op" else H.auto_plan_ex)(L.ta, L.tb, L.m, L.n, L.k, **kw)[0], None
    kw.update(stride_a=L.sa, stride_b=L.sb, stride_c=L.sc, batch=L.batch)
    if L.call == "batched":
        return H.auto_plan_batched(L.ta, L.tb, L.m, L.n, L.k, **kw)[:2]
    return H.auto_plan_batched_ex(L.ta, L.tb, L.m, L.n, L.k, stride_bias=L.sbias, bias_mode=L.epilogue[2], **kw)[:2]


def tile_of(name):
    """(bm, bn) a short kernel name says, None where it says none ("mfma": the 128x128 register-staged tile)."""
    t = re.search(r"_(\d+)x(\d+)", name)
    return (int(t[1]), int(t[2])) if t else (128, 128) if name == "mfma" else None


def whole(L, tile):
    """The launch needs no guards on the tile: whole tiles, leading dimensions, bases and a batch's strides multiples of 4 floats."""
    ok = L.m % tile[0] == 0 and L.n % tile[1] == 0 and L.k % 32 == 0 and base_align(L.bases) == 16 and \
        all(x % 4 == 0 for x in (L.lda, L.ldb, L.ldc))
    return ok and (L.batch in (None, 1) or all(x % 4 == 0 for x in (L.sa, L.sb, L.sc)))


def text_tail(L, form):
    """What last_launch() ends in for the model's launch: kernel_tables.ex_tag / launch_dma5.hpp's op tag, then the batch."""
    pair = "NT"[L.ta] + "NT"[L.tb]
    tag = ex_tag((L.ta, L.tb), *L.epilogue) if L.epilogue is not None else "" if pair == "NN" else ", operands " + pair
    if L.batch is None:
        return tag
    if form == "fold":
        return tag + f", batch {L.batch} folded into one {L.batch * L.m}-row GEMM"
    if form == "loop":
        return tag + f", batch {L.batch} as a loop of {L.batch} per-matrix launches"
    return tag + f", batch {L.batch}"


def text_failures(L, text, kernel, cus):
    """How `text`, last_launch() after the form, departs from the model's launch `L` run on `kernel` (a forced tile or "auto")."""
    bad = []
    name, form = plan_of(L, cus) if kernel == "auto" else (kernel, None)
    if kernel != "auto" and L.batch is not None:
        form = "one_launch"
    tail = text_tail(L, form)
    if not text.endswith(tail) or (tail == "" and ", operands" in text):
        bad.append(f"the launch text does not end in {tail!r}")
    tile = tile_of(name)
    if tile is not None and "<%d,%d" % tile not in text:
        bad.append(f"the launch text does not name the tile <{tile[0]},{tile[1]}> of {name}")
    if name in FAMILY and not whole(L, tile) and "guarded" not in text:
        bad.append("the launch is not the guarded form")
    return [f"{b}: {text!r}" for b in bad]


# ---- the GPU runner ---------------------------------------------------------------------------------------------------------------
class Stored:
    """A view's storage on the device: NaN but for `values` at the view's elements; .t the torch view."""

    def __init__(self, view, values=None):
        import torch
        self.view, self.before = view, lay(view, values)
        self.flat = torch.from_numpy(self.before).cuda()
        self.t = torch.as_strided(self.flat, view.shape, view.strides, view.offset)

    def reset(self, values=None):
        import torch
        self.before = lay(self.view, values)
        self.flat.copy_(torch.from_numpy(self.before))

    def failures(self, want=None):
        """The storage against `want` in the window (None: untouched) and its former bits everywhere else."""
        got = self.flat.cpu().numpy()
        bad = []
        if want is not None and np.asarray(want).size:
            idx = indices(*self.view[:3])
            w2 = np.asarray(want, F32).reshape(-1, want.shape[-1]) if np.asarray(want).ndim else np.asarray(want, F32).reshape(1, 1)
            g2 = got[idx].reshape(w2.shape)
            if not same_bits(g2, w2):
                bad.append(first_difference(g2, w2))
            inside = np.zeros(got.size, bool)
            inside[idx] = True
        else:
            inside = np.zeros(got.size, bool)
        if not np.array_equal(got.view(np.uint32)[~inside], self.before.view(np.uint32)[~inside]):
            bad.append("wrote outside the window" if want is not None else "the output was touched")
        return bad


def _as_rows(x):
    x = np.asarray(x, F32)
    return x.reshape(-1, x.shape[-1]) if x.ndim else x.reshape(1, 1)


def run_case(c, cus, tally=None, H=None, handle=None):
    """Run every form of the case on the current device with `handle` (an MMult on AUTO; its kernel and stream-K option are put
    back).  Returns the list of failures (strings), never stopping at the first; tally, a dict, counts "forms" run and "refusals"
    checked.  A HIP error is not a failure of a form: it is raised."""
    import torch
    if H is None:
        import how_to_optimize_gemm_amd as H
    tally = tally if tally is not None else {}
    fails, v = [], inputs(c)
    exp = expected(c, v) if c.family != "refuse" else {}
    todo = {f.name: f for f in forms(c)}
    V = c.views
    side = torch.cuda.Stream() if c.side_stream else None

    def fail(form, *what):
        fails.append(f"{form}: " + " ".join(str(w) for w in what))

    def ran(form, call, outs, number):
        """Run `call` under the form's kernel configuration; outs: [(Stored or tensor, expectation or None)] checked afterwards."""
        f = todo.pop(form)
        kernel, sk = config_of(c, number)
        handle.set_kernel(kernel)
        handle.set_streamk(sk)
        try:
            result = call()
            text = H.last_launch()
        except H.MMultError as err:
            if err.status == H.ERR_HIP:
                raise
            fail(form, f"on {kernel}: raised {err}")
            return None
        finally:
            handle.set_kernel("auto")
            handle.set_streamk(1)
        torch.cuda.synchronize()
        tally["forms"] = tally.get("forms", 0) + 1
        for bad in (text_failures(f.launch, text, kernel, cus) if f.launch is not None else []):
            fail(form, f"on {kernel}:", bad)
        for target, want in outs(result) if callable(outs) else outs:
            if isinstance(target, Stored):
                for bad in target.failures(want):
                    fail(form, f"on {kernel}:", bad, f"[{text}]")
            elif want is None:
                if target is not None:
                    fail(form, "returned a tensor where None is the contract")
            elif target is None or tuple(target.shape) != tuple(np.asarray(want).shape):
                fail(form, f"on {kernel}: returned {None if target is None else tuple(target.shape)}, expected shape {np.asarray(want).shape}")
            elif np.asarray(want).size and not same_bits(_as_rows(target.detach().cpu().numpy()), _as_rows(want)):
                fail(form, f"on {kernel}:", first_difference(_as_rows(target.detach().cpu().numpy()), _as_rows(want)), f"[{text}]")
        return result

    def body():
        S = lambda name, values=True: Stored(V[name], v[name] if values is True else values)
        alpha, beta = c.ab
        nan_like = lambda name: np.full(V[name].shape, np.nan, F32)
        if c.family in ("2d", "3d"):
            a, b = S("a"), S("b")
            out = S("c", None)
            mm, addmm = (handle.matmul, handle.addmm) if c.family == "2d" else (handle.bmm, handle.baddbmm)
            p = "matmul" if c.family == "2d" else "bmm"
            ran(p, lambda: mm(a.t, b.t), lambda r: [(r, exp[p])], 0)
            ran(p + " out=", lambda: mm(a.t, b.t, out=out.t), [(out, exp[p + " out="])], 1)
            out.reset(v["c0"])
            ran(p + " accumulate", lambda: mm(a.t, b.t, out=out.t, accumulate=True), [(out, exp[p + " accumulate"])], 2)
            # beta == 0 runs over a NaN input
            inp = S("inp", v["inp"] if beta != 0 else nan_like("inp"))
            vec = S("vec")
        if c.family == "2d":
            ran("addmm 2-D", lambda: addmm(inp.t, a.t, b.t, beta=beta, alpha=alpha), lambda r: [(r, exp["addmm 2-D"]), (inp, None)], 3)
            out.reset()
            ran("addmm 2-D out=", lambda: addmm(inp.t, a.t, b.t, beta=beta, alpha=alpha, out=out.t), [(out, exp["addmm 2-D out="]), (inp, None)], 4)
            inp.reset(v["inp"] if beta != 0 else None)
            ran("addmm out is input", lambda: addmm(inp.t, a.t, b.t, beta=beta, alpha=alpha, out=inp.t), [(inp, exp["addmm out is input"])], 5)
            out.reset()
            al, be = vec_ab(c, True)
            ran("addmm (n,) bias", lambda: addmm(vec.t, a.t, b.t, beta=be, alpha=al, out=out.t), [(out, exp["addmm (n,) bias"]), (vec, None)], 6)
            al2, be2 = vec_ab(c, False)
            if be2 == 0:
                vec.reset(nan_like("vec"))
            ran("addmm (n,) copy", lambda: addmm(vec.t, a.t, b.t, beta=be2, alpha=al2), lambda r: [(r, exp["addmm (n,) copy"]), (vec, None)], 7)
            bias = S("bias")
            w = b.t.t()
            act = "relu" if c.relu else None
            if c.index % 3:
                out.reset()
                ran("linear", lambda: handle.linear(a.t, w, bias.t if c.bias else None, act, out=out.t), [(out, exp["linear"]), (bias, None)], 8)
            else:
                ran("linear", lambda: handle.linear(a.t, w, bias.t if c.bias else None, act), lambda r: [(r, exp["linear"])], 8)
        elif c.family == "3d":
            out.reset()
            ran("baddbmm full", lambda: addmm(inp.t, a.t, b.t, beta=beta, alpha=alpha, out=out.t), [(out, exp["baddbmm full"]), (inp, None)], 3)
            inp.reset(v["inp"] if beta != 0 else None)
            ran("baddbmm out is input", lambda: addmm(inp.t, a.t, b.t, beta=beta, alpha=alpha, out=inp.t), [(inp, exp["baddbmm out is input"])], 4)
            bb = bias_beta(c)
            for number, (name, key) in enumerate((("(n,)", "vec"), ("(batch,1,n) strided", "pm"), ("(batch,1,n) expanded", "pe")), 5):
                src = S(key, v[key] if bb != 0 else nan_like(key))
                ran("baddbmm " + name, lambda: addmm(src.t, a.t, b.t, beta=bb, alpha=alpha), lambda r: [(r, exp["baddbmm " + name]), (src, None)], number)
            for number, (name, key) in enumerate((("(m,1)", "m1"), ("(1,n)", "1n"), ("(batch,1,1)", "b11")), 8):
                src = S(key, v[key] if beta != 0 else nan_like(key))
                out.reset()
                ran("baddbmm " + name, lambda: addmm(src.t, a.t, b.t, beta=beta, alpha=alpha, out=out.t), [(out, exp["baddbmm " + name]), (src, None)], number)
            lb = c.kinds["bias"]
            bias = None if lb == "None" else S("bias")
            # w: (batch, out, in) whose transpose is b -- or, where b is one expanded matrix, the 2-D weight the batch shares
            w = b.t[0].t() if (V["b"].strides[0] == 0 and c.batch > 0) else b.t.transpose(1, 2)
            act = "relu" if c.relu else None
            checks = [] if bias is None else [(bias, None)]
            if c.index % 3:
                out.reset()
                ran("batched_linear", lambda: handle.batched_linear(a.t, w, None if bias is None else bias.t, act, out=out.t),
                    [(out, exp["batched_linear"])] + checks, 11)
            else:
                ran("batched_linear", lambda: handle.batched_linear(a.t, w, None if bias is None else bias.t, act),
                    lambda r: [(r, exp["batched_linear"])] + checks, 11)
        elif c.family == "back":
            g, x, w = S("g"), S("x"), S("w")
            y = S("y") if c.relu else None
            yt = None if y is None else y.t
            dz, gb = S("dz", None), S("gb")
            name = "relu_grad_colsum"
            ran(name, lambda: handle.relu_grad_colsum(g.t, yt, dz=dz.t), lambda r: [(dz, exp[name][0]), (r[1], exp[name][1]), (g, None)], 0)
            ran(name + " want_dz=False accumulate", lambda: handle.relu_grad_colsum(g.t, yt, want_dz=False, bias_grad=gb.t, accumulate=True),
                lambda r: [(r[0], None), (gb, exp[name + " want_dz=False accumulate"][1]), (g, None)], 1)
            dz.reset()
            ran(name + " want_colsum=False", lambda: handle.relu_grad_colsum(g.t, yt, dz=dz.t, want_colsum=False),
                lambda r: [(dz, exp[name][0]), (r[1], None)], 2)
            for number, need in enumerate(NEEDS, 3):
                ran(f"linear_backward need={need}", lambda: handle.linear_backward(g.t, x.t, w.t, yt, need=need),
                    lambda r: list(zip(r, exp[f"linear_backward need={need}"])) + [(g, None), (x, None), (w, None)], number)
            gw = S("gw")
            gb.reset(v["gb"])
            want = exp["linear_backward grad_w= grad_b="]
            ran("linear_backward grad_w= grad_b=", lambda: handle.linear_backward(g.t, x.t, w.t, yt, grad_w=gw.t, grad_b=gb.t),
                lambda r: [(r[0], want[0]), (gw, want[1]), (gb, want[2])], 11)
            ran(name + " dz=g", lambda: handle.relu_grad_colsum(g.t, yt, dz=g.t), lambda r: [(g, exp[name][0]), (r[1], exp[name][1])], 12)
            from how_to_optimize_gemm_amd import autograd as AG
            bias, Gd, td = S("bias"), S("G"), S("t")
            act = "relu" if c.relu else None
            for number, kind in enumerate(("contiguous", "expanded", "transposed"), 13):
                xl, wl = x.t.detach().requires_grad_(), w.t.detach().requires_grad_()
                bl = bias.t.detach().requires_grad_() if c.bias else None

                def step():
                    yl = AG.linear(handle, xl, wl, bl, act)
                    loss = {"contiguous": lambda: (yl * Gd.t).sum(), "expanded": yl.sum, "transposed": lambda: (yl.t() * td.t).sum()}[kind]()
                    loss.backward()
                    return yl
                ran("autograd " + kind, step, lambda r: list(zip((r, xl.grad, wl.grad, None if bl is None else bl.grad), exp["autograd " + kind]))
                    + [(x, None), (w, None)], number)
        else:
            refuse()

    def refuse():
        """One call the host refuses before any launch: MMH_ERR_INVALID_ARG, no output touched, no launch recorded."""
        todo.pop("refusal: " + c.refusal)
        a, b, out = Stored(V["a"], v["a"]), Stored(V["b"], v["b"]), Stored(V["c"], v["c0"])
        inp, vec = Stored(V["inp"], v["inp"]), Stored(V["vec"], v["vec"])
        a2, b2, o2 = a.t[0], b.t[0], out.t[0]
        (batch, m, n), k = out.t.shape, c.k
        ldc = V["c"].strides[1]
        overlap_rows = torch.as_strided(out.flat, (m, n), (n - 1, 1), V["c"].offset)
        overlap_mats = torch.as_strided(out.flat, (batch, m, n), ((m - 1) * ldc + n - 1, ldc, 1), V["c"].offset)
        gapped = torch.as_strided(vec.flat, ((n + 1) // 2,), (2,), V["vec"].offset)
        calls = {
            "no unit stride": [lambda: handle.matmul(a2[:, ::2], b2[:(k + 1) // 2], out=o2), lambda: handle.bmm(a.t, b.t[:, :, ::2], out=out.t[:, :, :(n + 1) // 2]),
                               lambda: handle.addmm(inp.t[0], a2, b2, out=torch.as_strided(out.flat, (m, n), (ldc, 2), FRONT))],
            "overlapping rows of out": [lambda: handle.matmul(a2, b2, out=overlap_rows), lambda: handle.addmm(inp.t[0], a2, b2, out=overlap_rows),
                                        lambda: handle.linear(a2, b2.t(), out=overlap_rows)],
            "overlapping matrices of out": [lambda: handle.bmm(a.t, b.t, out=overlap_mats), lambda: handle.baddbmm(inp.t, a.t, b.t, beta=0.5, out=overlap_mats),
                                            lambda: handle.baddbmm(vec.t, a.t, b.t, out=overlap_mats)],
            "wrong dtype": [lambda: handle.matmul(a2.double(), b2.double(), out=o2), lambda: handle.matmul(a2, b2, out=o2.double()),
                            lambda: handle.bmm(a.t.half(), b.t.half(), out=out.t), lambda: handle.linear(a2, b2.t(), vec.t.double(), out=o2)],
            "CPU tensor": [lambda: handle.matmul(a2.cpu(), b2, out=o2), lambda: handle.matmul(a2, b2, out=o2.cpu()),
                           lambda: handle.baddbmm(inp.t, a.t, b.t.cpu(), out=out.t), lambda: handle.linear(a2, b2.t(), vec.t.cpu(), out=o2)],
            "non-dense bias": [lambda: handle.linear(a2, b2[:, :(n + 1) // 2].t(), gapped, out=o2[:, :(n + 1) // 2]),
                               lambda: handle.batched_linear(a.t, b.t.transpose(1, 2), torch.as_strided(inp.flat, (batch, n), (2 * n, 2), FRONT), out=out.t),
                               lambda: handle.relu_grad_colsum(o2[:, :(n + 1) // 2], None, want_dz=False, bias_grad=gapped)],
            "inner dimensions disagree": [lambda: handle.matmul(a2, b2[:k - 1], out=o2), lambda: handle.addmm(o2, a2[:, :k - 1], b2, out=o2),
                                          lambda: handle.bmm(a.t[:, :, :k - 1], b.t, out=out.t), lambda: handle.linear(a2, b2.t()[:, :k - 1], out=o2)],
            "batch dimensions disagree": [lambda: handle.bmm(a.t[:2], b.t, out=out.t), lambda: handle.baddbmm(inp.t, a.t, b.t[:2], out=out.t),
                                          lambda: handle.batched_linear(a.t, b.t.transpose(1, 2)[:2], out=out.t), lambda: handle.bmm(a.t, b.t, out=out.t[:2])],
        }[c.refusal]
        before = H.last_launch()
        for number, call in enumerate(calls):
            tally["refusals"] = tally.get("refusals", 0) + 1
            try:
                call()
            except H.MMultError as err:
                if err.status == H.ERR_HIP:
                    raise
                if err.status != H.ERR_INVALID_ARG:
                    fail(f"refusal {number}", f"refused with status {err.status}, not MMH_ERR_INVALID_ARG: {err}")
            else:
                fail(f"refusal {number}", "was not refused")
            if H.last_launch() != before:
                fail(f"refusal {number}", "a refused call launched something")
        torch.cuda.synchronize()
        for name, st in (("out", out), ("input", inp), ("vec", vec), ("a", a), ("b", b)):
            for bad in st.failures(None):
                fail("refusal", name + ":", bad)

    try:
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body()
            torch.cuda.current_stream().wait_stream(side)
        else:
            body()
    finally:
        handle.set_kernel("auto")
        handle.set_streamk(1)
        torch.cuda.synchronize()
    for name in todo:
        fail(name, "forms() lists the form, run_case did not run it")
    return fails
