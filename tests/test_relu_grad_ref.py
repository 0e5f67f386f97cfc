"""tests/relu_grad_ref.py, the numpy restatement of mmh_relu_grad_colsum's contract, checked on the CPU: against float64 within
the bound of its own summation order, and that the order really is pinned -- moving a row across a block boundary changes
bits -- and the condition that gives the many-block cases of tests/test_gpu_relu_grad.py their teeth: on the very arrays that
table runs at (rows, 260), blocks added in descending order, each batch of 16 partial rows summed first, R = 64, R = 256 and
one chain over all rows each agree with the contract in fewer than half of the columns, and so does a dropped block (index 16,
index 17, the last) at the two row counts whose last block is 77 rows.  The shares are conditions on the reference; nothing
here has seen a kernel's output.  Observed: the largest agreeing share of an order or block-height variant is 0.435 (batches
first, 17R + 77 rows, no gate: a margin of 0.065 under the 0.5), the next 0.381 and 0.350 (batches first, gated, 18 and 17
blocks); descending order 0.131 - 0.304; R = 64 / 256 at most 0.154; one chain at most 0.077; every dropped block at the + 77
row counts 0.0."""
import os

import numpy as np
import pytest

import relu_grad_ref as ref
from built_lib import REPO

R = ref.header_block_rows(REPO)


@pytest.mark.parametrize("rows,cols", [(1, 5), (R - 1, 7), (R, 4), (R + 1, 9), (2 * R + 44, 33), (5 * R + 3, 16)])
@pytest.mark.parametrize("gated", [False, True])
def test_blocked_colsum_is_within_its_chain_bound_of_float64(rows, cols, gated):
    """A chain of n adds is within gamma_(n-1) sum|z| of the exact sum; a column's value passes through at most R - 1 adds
    inside its block and nblocks - 1 across the blocks: gamma_(R + nblocks) covers it."""
    rng = np.random.default_rng(rows * 1000 + cols)
    g = rng.standard_normal((rows, cols)).astype(np.float32)
    y = rng.standard_normal((rows, cols)).astype(np.float32) if gated else None
    z, s = ref.relu_grad_colsum(g, y, R)
    if gated:
        assert np.array_equal(z, np.where(y > 0, g, np.float32(0)))
        assert 0 < np.count_nonzero(z) < z.size or rows * cols < 8
    else:
        assert np.array_equal(z.view(np.uint32), g.view(np.uint32))
    assert s.dtype == np.float32 and s.shape == (cols,)
    z64 = z.astype(np.float64)
    nblocks = (rows + R - 1) // R
    bound = ref.gamma(R + nblocks) * np.abs(z64).sum(axis=0)
    assert np.all(np.abs(s.astype(np.float64) - z64.sum(axis=0)) <= bound)
    old = rng.standard_normal(cols).astype(np.float32)
    assert np.array_equal(ref.blocked_colsum(z, R, old), old + s)


def test_the_order_is_pinned_across_a_block_boundary():
    """Column 0 of 2R rows: block 0 holds 2^24 and R - 1 ones, block 1 zeros.  In order, every 1 is absorbed by 2^24 (half an
    ulp, ties to even): the sum is 2^24.  With the 2^24 row swapped into block 1, block 0 sums its R - 1 ones exactly and the
    last add rounds the exact 2^24 + R - 1 once (spacing 2 up there) -- other bits.  The exact sum is the same."""
    z = np.zeros((2 * R, 2), dtype=np.float32)
    z[0, 0] = 2.0 ** 24
    z[1:R, 0] = 1.0
    z[:, 1] = 1.0
    s = ref.blocked_colsum(z, R)
    assert s[0] == np.float32(2.0 ** 24) and s[1] == np.float32(2 * R)
    perm = np.arange(2 * R)
    perm[0], perm[R] = R, 0                     # swap row 0 with the first row of block 1
    t = ref.blocked_colsum(z[perm], R)
    assert t[1] == s[1]
    assert t[0] == np.float32(np.float64(2.0 ** 24) + (R - 1)) and t[0] != s[0]
    assert not ref.same_bits(s, t)
    assert z[perm].astype(np.float64).sum(axis=0)[0] == z.astype(np.float64).sum(axis=0)[0]
    # ... and a permutation INSIDE a block that keeps every partial exact leaves the bits alone
    inside = np.arange(2 * R)
    inside[R + 1], inside[R + 2] = R + 2, R + 1
    assert ref.same_bits(ref.blocked_colsum(z[inside], R), s)


def test_gate_special_values():
    sub = np.float32(1e-45)
    ys = np.array([0.0, -0.0, -1.0, sub, -sub, np.nan, np.inf, -np.inf, 1.0], dtype=np.float32)
    gs = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub, 1.5], dtype=np.float32)
    y, g = np.meshgrid(ys, gs, indexing="ij")
    z = ref.gate(g, y)
    open_ = np.array([False, False, False, True, False, True, True, False, True])
    for i, o in enumerate(open_):
        want = gs if o else np.zeros_like(gs)
        assert ref.same_bits(z[i], want), (ys[i], z[i])
        if not o:
            assert not np.any(np.signbit(z[i]))      # +0, never -0 or NaN
    assert ref.same_bits(ref.gate(g), g)


def test_rows_zero_and_same_bits():
    assert ref.same_bits(ref.blocked_colsum(np.zeros((0, 3), np.float32), R), np.zeros(3, np.float32))
    old = np.array([1.0, -0.0, np.nan], np.float32)
    assert ref.same_bits(ref.blocked_colsum(np.zeros((0, 3), np.float32), R, old), old)
    assert not ref.same_bits(np.float32([0.0]), np.float32([-0.0]))
    assert ref.same_bits(np.float32([np.nan, 1.0]), np.float32([-np.nan, 1.0]))


# ---- the condition that gives the GPU table's many-block cases their teeth ---------------------------------------------
FU = 16   # colsum_finish_kernel adds the partial rows this many at a time (RG_FU, csrc/relu_grad.hpp)
MANY_BLOCK_ROWS = [16 * R + 1, 17 * R + 77, 32 * R + 1, 33 * R + 77]   # tests/test_gpu_relu_grad.py::MANY_BLOCK_ROWS
_SHARES = []


def test_the_many_block_rows_are_the_gpu_tables():
    import test_gpu_relu_grad as T
    assert T.MANY_BLOCK_ROWS == MANY_BLOCK_ROWS and 260 in T.MANY_BLOCK_COLS
    src = open(os.path.join(REPO, "how-to-optimize-gemm_amd", "csrc", "relu_grad.hpp")).read()
    assert "constexpr int RG_FU = %d;" % FU in src
    assert [(r + R - 1) // R for r in MANY_BLOCK_ROWS] == [17, 18, 33, 34]


def wrong_sums(z):
    """What a finish kernel, or a pass, that is subtly wrong would give: name -> column sums."""
    parts = ref.block_partials(z, R)
    n = len(parts)
    with np.errstate(invalid="ignore", over="ignore"):
        batch_first = parts[0].copy()
        for b in range(1, n, FU):
            batch_first = batch_first + ref.chain(parts[b:b + FU])
    orders = {
        "descending": ref.chain(parts[::-1]),
        "batch first": batch_first,
        "R = 64": ref.blocked_colsum(z, 64),
        "R = 256": ref.blocked_colsum(z, 256),
        "one chain": ref.chain(z),
    }
    dropped = {
        "block 16 dropped": ref.chain(np.delete(parts, 16, axis=0)),
        "block 17 dropped": ref.chain(np.delete(parts, 17, axis=0)),
        "last block dropped": ref.chain(parts[:-1]),
    } if n > 17 else {}
    return orders, dropped


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("rows", MANY_BLOCK_ROWS)
def test_at_the_many_block_cases_other_orders_and_dropped_blocks_give_other_bits(rows, gated):
    """On the very arrays the GPU table runs at (rows, 260): each wrong order or block height agrees with the contract in
    fewer than half of the columns, and so does a dropped block where the last block is more than one row (a one-row last
    block under a gate is zero in most columns: dropping it changes little, and that is the data's property)."""
    g, y, _ = ref.case_inputs(rows, 260)
    z, s = ref.relu_grad_colsum(g, y if gated else None, R)
    orders, dropped = wrong_sums(z)
    for name, other in orders.items():
        share = ref.agreeing_share(s, other)
        _SHARES.append((share, name, rows, gated))
        assert share < 0.5, (name, share)
    if rows % R == 77:
        for name, other in dropped.items():
            share = ref.agreeing_share(s, other)
            _SHARES.append((share, name, rows, gated))
            assert share < 0.5, (name, share)
    print("largest agreeing share so far: %.3f (%s, %d rows, gated %s)" % max(_SHARES))
