"""The fused epilogue's contract restated in numpy (mmh_sgemm_ex, include/mmult_hip.h): C = act(alpha s + beta C + bias) on
the oracle's fused chain s, float32 throughout, one rounding per numpy operation.  Built from numpy alone, never from the
library; tests/test_gpu_ex.py, tests/test_gpu_ex_parity.py and tests/test_gpu_batched_ex.py hold the kernels to it."""
import numpy as np

NONE, COL, ROW = 0, 1, 2   # bias modes
RELU = 1                   # activations


def expected(s, alpha, beta, c, bias, bias_mode, act):
    """The contract, restated: float32 arrays throughout, one rounding per numpy operation."""
    assert s.dtype == np.float32, s.dtype
    r = np.float32(alpha) * s
    if beta != 0:
        r = r + np.float32(beta) * c.astype(np.float32)
    if bias_mode == COL:
        r = r + bias.astype(np.float32)[None, :]
    elif bias_mode == ROW:
        r = r + bias.astype(np.float32)[:, None]
    if act == RELU:
        r = np.where((r > 0) | np.isnan(r), r, np.float32(0))
    assert r.dtype == np.float32, r.dtype
    return r
