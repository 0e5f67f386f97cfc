"""The numpy restatement of mmh_relu_grad_colsum's contract (include/mmult_hip.h): the gate as a select, the column sum in
row blocks of R = MMH_COLSUM_BLOCK_ROWS -- every block a sequential fp32 chain started at its first row, the blocks' partials
a sequential fp32 chain started at block 0.  Vectorised over the columns: every np.float32 array addition below is one
correctly rounded fp32 add per column, the operation the kernels perform.  A helper, not a test module."""
import numpy as np

from bitcmp import same_bits  # noqa: F401 (bit equality with every NaN equal to every NaN: ref.same_bits)


def header_block_rows(repo):
    """MMH_COLSUM_BLOCK_ROWS as include/mmult_hip.h defines it."""
    import os
    import re
    text = open(os.path.join(repo, "include", "mmult_hip.h")).read()
    return int(re.search(r"^#define\s+MMH_COLSUM_BLOCK_ROWS\s+(\d+)\s*$", text, re.M).group(1))


def gate(g, y=None):
    """z = g without y; z = +0 where y <= 0, else g's bits (y = NaN: the gate stays open)."""
    g = np.asarray(g, dtype=np.float32)
    if y is None:
        return g.copy()
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y, dtype=np.float32) <= 0, np.float32(0), g).astype(np.float32)


def blocked_colsum(z, R, old=None):
    """The column sums of z (rows, cols) in the contract's order; `old`: accumulate -- fl(old + s)."""
    z = np.asarray(z, dtype=np.float32)
    rows, cols = z.shape
    with np.errstate(invalid="ignore", over="ignore"):
        s = None
        for r0 in range(0, rows, R):
            p = z[r0].copy()
            for r in range(r0 + 1, min(r0 + R, rows)):
                p = p + z[r]
            s = p if s is None else s + p
        if s is None:
            s = np.zeros(cols, dtype=np.float32)
            return s if old is None else np.asarray(old, dtype=np.float32).copy()
        assert s.dtype == np.float32
        return s if old is None else (np.asarray(old, dtype=np.float32) + s)


def case_inputs(rows, cols):
    """(g, y, old) of the GPU table's case (rows, cols), tests/test_gpu_relu_grad.py: normal variates with -0 and subnormals
    sprinkled into g and +-0 into y; `old` is what an accumulating call finds in the sums."""
    rng = np.random.default_rng(rows * 4099 + cols)
    g = rng.standard_normal((rows, cols)).astype(np.float32)
    y = rng.standard_normal((rows, cols)).astype(np.float32)
    pick = rng.random((rows, cols))
    g[pick < 0.03] = np.float32(-0.0)
    g[(pick >= 0.03) & (pick < 0.06)] = np.float32(3e-42)
    y[(pick >= 0.5) & (pick < 0.55)] = np.float32(0.0)
    y[(pick >= 0.55) & (pick < 0.6)] = np.float32(-0.0)
    old = rng.standard_normal(cols).astype(np.float32)
    return g, y, old


def block_partials(z, R):
    """p_b of the contract for every row block: (nblocks, cols)."""
    z = np.asarray(z, dtype=np.float32)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, z.shape[0], R):
            p = z[r0].copy()
            for r in range(r0 + 1, min(r0 + R, z.shape[0])):
                p = p + z[r]
            parts.append(p)
    return np.array(parts, dtype=np.float32).reshape(len(parts), z.shape[1])


def chain(parts):
    """parts[0], then fl(s + parts[b]) for b ascending."""
    s = parts[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p in parts[1:]:
            s = s + p
    return s


def agreeing_share(a, b):
    """The share of elements whose bits are equal."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return float(np.mean(a.view(np.uint32) == b.view(np.uint32)))


def relu_grad_colsum(g, y, R, old=None):
    """(dz, colsum) of the contract."""
    z = gate(g, y)
    return z, blocked_colsum(z, R, old)


def gamma(n):
    """Higham's gamma_n for fp32: n u / (1 - n u), u = 2^-24."""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)
