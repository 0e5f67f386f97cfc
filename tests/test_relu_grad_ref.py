"""tests/relu_grad_ref.py, the numpy restatement of mmh_relu_grad_colsum's contract, checked on the CPU: against float64 within
the bound of its own summation order, and that the order really is pinned -- moving a row across a block boundary changes
bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relu_grad_ref as ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
