"""The peak probes no other GPU test launches (csrc/probes.hip): the vector-ALU loops, packed and not, and the two int8 MFMA
loops.  A probe is a denominator -- what a rung's rate is quoted against -- so what is held here is that
each one runs and reads a rate that is positive and under its roof: the specification's figure at the peak engine clock, with
the 5 % of tests/test_gpu_parity.py::test_lds_probe_reads_a_plausible_rate for the event timers' granularity.  The vector
ALU's roof is 157.3 TFLOP/s for BOTH loops: a CDNA4 SIMD is 32 lanes wide and issues a wave64 v_fma_f32 in two cycles -- 64 lanes
x 2 flops / 2 cycles = the 64 flops per clock and SIMD that v_pk_fma_f32 (twice the work, four cycles) reaches as well; packing
saves issue slots, not time.  The int8 MFMA's is 5.03 POP/s.  tests/test_kernel_census.py names these tests for the probe kernels.

Floors, in the style of that test's (50 % of the roof for the read a kernel leans on): two waves per SIMD are what it takes to
fill the two-cycle issue (MI355X: one wave alone issues a vector instruction every four cycles), so at two waves either loop
must reach half the roof; and since both loops have the same roof and the same 64 FMAs per lane and iteration, neither may
read under half the other at the same wave count -- a loop that compiles to something else, or a flop count off by the factor
of two that packing suggests, shows there.

The unpacked loop is spelled in inline asm: as two __builtin_fmaf per accumulator pair hipcc paired them into v_pk_fma_f32 and
the "v_fma_f32" probe was a second packed one.  With the instruction spelled out the two loops read the same rate (77 TFLOP/s at
one wave per SIMD, 104 at two), which is what the two-cycle issue says they should."""
import pytest

pytestmark = pytest.mark.gpu

VALU_ROOF = 157.3             # TFLOP/s: 256 CUs x 4 SIMDs x 32 lanes x 2 (FMA) x 2.4 GHz, packed or not
INT8_MFMA_ROOF = 5033.0       # TOP/s: twice the BF16 MFMA rate


def test_the_vector_alu_probes_read_a_rate_under_their_roofs(mm):
    import how_to_optimize_gemm_amd as H
    for waves in (1, 2):
        packed = mm.probe_valu_f32(True, waves)
        plain = mm.probe_valu_f32(False, waves)
        print(f"probe_valu_f32, {waves} wave(s) per SIMD: packed {packed:.1f}, unpacked {plain:.1f} TFLOP/s")
        assert 0 < packed < 1.05 * VALU_ROOF, (waves, packed)
        assert 0 < plain < 1.05 * VALU_ROOF, (waves, plain)
        assert 0.5 * packed < plain < 2.0 * packed, (waves, packed, plain)
        if waves == 2:
            assert packed > 0.5 * VALU_ROOF and plain > 0.5 * VALU_ROOF, (packed, plain)
    for waves in (0, 5):
        with pytest.raises(H.MMultError):
            mm.probe_valu_f32(True, waves)


def test_the_int8_mfma_probes_read_a_rate_under_their_roof(mm):
    constant = mm.probe_mfma_i8()
    sustained = mm.probe_mfma_i8_sustained(True, 5.0)
    sustained_constant = mm.probe_mfma_i8_sustained(False, 5.0)
    print(f"probe_mfma_i8 {constant:.0f}, sustained (random operands) {sustained:.0f}, (constant operands) {sustained_constant:.0f} TOP/s")
    for v in (constant, sustained, sustained_constant):
        assert 0 < v < 1.05 * INT8_MFMA_ROOF, v
