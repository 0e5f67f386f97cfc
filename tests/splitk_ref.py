"""The restatement of the opt-in split-K kernels' bit contract (csrc/sgemm_mfma.hpp, the K2s block; include/mmult_hip.h,
MMH_KERNEL_MFMA_SPLITK), built from the oracle's chains alone.  With nk = k / kb K-slices, part s of S is the ascending-k fp32
fma chain over the slices [nk s / S, nk (s + 1) / S); parts 1 .. S - 1 start from zero, part 0 from C when accumulating, else
from zero; the tile is ((P0 + P1) + P2) + ... in plain fp32 adds.  Every such chain is one oracle.ref_mmult(..., fma=True)
reproduces bit for bit for the chain kernels.  A helper, not a test module."""
import numpy as np


def parts_launched(requested, nk):
    """csrc/launch_reg.hip try_launch_splitk's first clamp: never more parts than K-slices.  Fewer than 2: no split."""
    return min(requested, nk)


def auto_parts(cus, tiles, k):
    """csrc/policy.hip splitk_auto_parts: two workgroups per CU, at least 8 K-slices (256 of k) per part, at most 8 parts."""
    return min((2 * cus) // max(tiles, 1), k // 256, 8)


def boundaries(nk, S):
    """The K-slice at which each part starts, and nk behind the last: floor(nk s / S)."""
    return [nk * s // S for s in range(S + 1)]


def partials(oracle, a, b, c0, S, kb=32):
    """[P0, P1, ...]: each part one oracle chain over contiguous copies of its K range (oracle._base wants a view that starts
    at its parent's origin); part 0 is given a copy of c0 when accumulating."""
    m, k = a.shape
    assert k % kb == 0 and 1 <= S <= k // kb, (k, kb, S)
    cut = boundaries(k // kb, S)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            k0, k1 = cut[s] * kb, cut[s + 1] * kb
            start = None if s or c0 is None else np.array(c0, dtype=np.float32, order="C", copy=True)
            out.append(oracle.ref_mmult(np.ascontiguousarray(a[:, k0:k1]), np.ascontiguousarray(b[k0:k1]), start, fma=True))
    return out


def fold(parts, descending=False):
    """((P0 + P1) + P2) + ... : one correctly rounded fp32 add per element and part.  (descending: the parts taken from the
    last one down -- what the contract is NOT; the CPU tests measure how far apart the two are.)"""
    seq = parts[::-1] if descending else parts
    acc = seq[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for p in seq[1:]:
            acc = acc + p
    assert acc.dtype == np.float32
    return acc


def splitk_ref(oracle, a, b, c0, S, kb=32):
    """C = A B (c0 None) or c0 + A B as a split-K launch of S parts returns it."""
    return fold(partials(oracle, a, b, c0, S, kb))


def c_added_last(oracle, a, b, c0, S, kb=32):
    """What the contract is NOT: every part started from zero, C added behind the fold."""
    with np.errstate(over="ignore", invalid="ignore"):
        return fold(partials(oracle, a, b, None, S, kb)) + np.asarray(c0, dtype=np.float32)


def differing_share(x, y):
    """The share of elements whose bits differ (NaN equal to NaN)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    bad = (nx != ny) | (~nx & ~ny & (x.view(np.uint32) != y.view(np.uint32)))
    return float(bad.mean())
