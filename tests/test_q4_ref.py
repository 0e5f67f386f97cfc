"""The 4-bit layer's numpy restatement (tests/q4_ref.py) held to itself, and the arithmetic q4decode_partial_kernel stands on made
a held fact: the packing round trip at every nibble value, position and k tail; the unpacking of a dword of packed bytes into two
int8 vectors of 16 x the nibbles for all 256 byte values, carries between bytes included; the exact shift of the finished sum;
the overflow bound of a K range; the quantiser's special values."""
import numpy as np
import pytest

import q4_ref as F
import qlinear_ref as R


@pytest.mark.parametrize("in_", [1, 63, 64, 65, 127, 128, 129, 256, 385])
def test_packing_round_trips_at_every_tail(in_):
    rng = np.random.default_rng(in_)
    W = rng.integers(-8, 8, (in_, 19), dtype=np.int8)
    P = F.pack_ref(W)
    assert P.dtype == np.uint8 and P.shape == (64 * -(-in_ // 128), 19) == (F.layout(19, in_)[1], 19)
    assert np.array_equal(F.unpack_ref(P, in_), W)
    # the formula, element by element; nibbles of k >= in are zero
    for s in range(P.shape[0] // 64):
        for r in (0, 1, 31, 63):
            lo = W[128 * s + r] if 128 * s + r < in_ else np.zeros(19, np.int8)
            hi = W[128 * s + 64 + r] if 128 * s + 64 + r < in_ else np.zeros(19, np.int8)
            assert np.array_equal(P[64 * s + r], (lo.view(np.uint8) & 15) | ((hi.view(np.uint8) & 15) << 4)), (s, r)


def test_every_value_at_every_nibble_position():
    """All 16 x 16 (low, high) pairs, at every row of a slice's low and high half."""
    lo, hi = np.meshgrid(np.arange(-8, 8, dtype=np.int8), np.arange(-8, 8, dtype=np.int8))
    W = np.zeros((128, 256), np.int8)
    for r in range(64):
        W[r], W[64 + r] = np.roll(lo.reshape(-1), r), np.roll(hi.reshape(-1), 3 * r)
    P = F.pack_ref(W)
    assert len(np.unique(P)) == 256 and np.array_equal(F.unpack_ref(P, 128), W)
    assert F.pack_ref(np.full((1, 1), -8, np.int8))[0, 0] == 0x08 and F.pack_ref(np.full((65, 1), -8, np.int8))[0, 0] == 0x88
    assert F.pack_ref(np.full((65, 1), -1, np.int8))[0, 0] == 0xFF and F.pack_ref(np.full((65, 1), 7, np.int8))[1, 0] == 0x07


def test_the_kernels_unpacking_is_exact_for_all_256_byte_values():
    """v & 0xF0F0F0F0 and (v << 4) & 0xF0F0F0F0 on DWORDS, viewed as int8, are 16 x the high and 16 x the low nibbles: every
    byte value at every byte position, beside every neighbour (what the shift carries over a byte boundary is masked away)."""
    b = np.arange(256, dtype=np.uint32)
    a, c = np.meshgrid(b, b)                       # every pair of neighbouring bytes
    for pos in range(3):
        v = ((a << (8 * pos)) | (c << (8 * pos + 8))).astype(np.uint32).reshape(-1)
        v |= np.uint32(0x5A) << np.uint32(8 * ((pos + 2) % 4))     # (the other bytes hold something too)
        hi = (v & np.uint32(0xF0F0F0F0)).view(np.int8).reshape(-1, 4)
        lo = ((v << np.uint32(4)) & np.uint32(0xF0F0F0F0)).view(np.int8).reshape(-1, 4)
        bytes_ = v.view(np.uint8).reshape(-1, 4).astype(np.int16)
        nib = lambda x: np.where(x >= 8, x - 16, x)
        assert np.array_equal(lo, 16 * nib(bytes_ & 15)) and np.array_equal(hi, 16 * nib(bytes_ >> 4)), pos
    assert np.array([0x80], np.uint8).view(np.int8)[0] == -128 == 16 * -8 and (0x08 << 4) & 0xF0 == 0x80   # nibble 8 -> byte 0x80


def test_the_shifted_sum_is_the_sum_for_every_x_and_every_nibble():
    """sum x * (16 W) >> 4 == sum x * W with x over -128 .. 127 and W over -8 .. 7: every product, and sums of both signs."""
    x = np.arange(-128, 128, dtype=np.int64)
    W = np.arange(-8, 8, dtype=np.int64)
    prod16 = x[:, None] * (16 * W)[None, :]
    assert np.array_equal(prod16 >> 4, x[:, None] * W[None, :])
    rng = np.random.default_rng(4)
    xs, Ws = rng.integers(-128, 128, (64, 4096)), rng.integers(-8, 8, (4096, 32))
    acc16 = (xs @ (16 * Ws)).astype(np.int32)
    assert np.array_equal(acc16 >> 4, xs @ Ws) and (acc16 < 0).any() and (acc16 > 0).any()


def test_the_overflow_bound():
    """|x| <= 128, |16 W| <= 128: a range of k_len accumulates at most 2^14 k_len -- int32 holds 65536 k (2^30) and any range
    below 2^17 k; at 2^17 k the all -128 x -8 range reaches 2^31."""
    assert 128 * 128 == 1 << 14 and (1 << 14) * F.MAX_RANGE_K == 1 << 30 < (1 << 31) - 1
    assert (1 << 14) * ((1 << 17) - 1) <= (1 << 31) - 1 < (1 << 14) * (1 << 17)
    worst = np.int64(-128) * np.int64(16 * -8) * F.MAX_RANGE_K
    assert worst == 1 << 30 and np.int32(worst) >> 4 == 128 * 8 * F.MAX_RANGE_K
    assert F.MAX_RANGE_K % F.SLICE == 0


def test_the_quantisers_rule_and_its_special_values():
    assert F.q4_scale_of_amax(0.0) == 1 and F.q4_scale_of_amax(np.float32(3.5)) == np.float32(2.0)
    assert F.q4_scale_of_amax(np.float32(1e-39)) == R.F32_MAX and F.q4_scale_of_amax(np.nan) == 1
    w = F.special_weight(6, 8, np.random.default_rng(2))
    q, s, inv = F.quantize4_ref(w)
    assert q.dtype == np.int8 and q.min() >= -7 and q.max() <= 7
    assert not q[0].any() and s[0] == 1 and inv[0] == 1
    assert q[1, 1] == 0 and s[1] == np.float32(7.0) / np.abs(np.delete(w[1], 1)).max()
    assert q[2, 0] == 7 and q[2, 2] == -7 and np.isfinite(s[2])
    assert s[3] == R.F32_MAX and q[3, 3] == np.rint(np.float32(1e-39) * R.F32_MAX) and not np.delete(q[3], 3).any()
    assert (q[4] == -7).all() and s[4] == np.float32(7.0) / np.float32(2.5)
    assert np.abs(q[5]).max() == 7 and np.array_equal(inv, np.float32(1.0) / s)
    # half to even: 0.5, 1.5, 2.5 of a row whose scale is 1 (max 7)
    q, s, _ = F.quantize4_ref(np.array([[7.0, 0.5, 1.5, 2.5, -0.5, -2.5, 6.5]], np.float32))
    assert s[0] == 1 and q[0].tolist() == [7, 0, 2, 2, 0, -2, 6]
    q, s, inv = F.quantize4_ref(np.zeros((3, 0), np.float32))
    assert q.shape == (3, 0) and (s == 1).all() and (inv == 1).all()


def test_want_is_the_int8_layers_arithmetic_on_the_unpacked_image():
    import qchain_ref as Q
    p = F.problem(5, 130, 257)
    P = F.pack_ref(p.W)
    assert np.array_equal(F.unpack_ref(P, 257), p.W) and np.array_equal(F.int_sums(p.xq, p.W), p.acc)
    y = F.want(p.xq, p.rx, P, 257, p.rw, p.bias, True)
    assert y.dtype == np.float32 and np.array_equal(y, R.epilogue_ref(p.acc, p.rx, p.rw, p.bias, True))
    assert np.array_equal(F.want(p.xq, p.rx, P, 257, p.rw, p.bias, True, p.so), Q.requant_ref(y, p.so))
    assert np.array_equal(F.want_of(p, True, True, False), y)
