// ab_kernels.hpp -- kernel ids of the tools build (libmmult_hip_ab.so) that name whole tile families; the product library
// neither defines nor accepts them.  Their catalogue rows, and those of the A/B ids that carry bare numbers: ab_kernels.inc.
// K2M (sgemm_dma32.hpp, round 4): the LDS-DMA ring feeding v_mfma_f32_32x32x2_f32 -- 64-cycle matrix instructions, one
// conflict-free ds_read_b128 + two v_permlane32_swap per eight k's of A -- and the two-block form
// v_mfma_f32_32x32x1_2b_f32; measured slower than the 16x16x4 tiles (profiles/r04_notes.md).
#pragma once
#define MMH_KERNEL_MFMA32_64X64_DMA 48
#define MMH_KERNEL_MFMA32_128X64_DMA 49
#define MMH_KERNEL_MFMA32_128X128_DMA 50
#define MMH_KERNEL_MFMA32_64X128_DMA 51
#define MMH_KERNEL_MFMA32B_128X64_DMA 60
#define MMH_KERNEL_MFMA32B_64X128_DMA 61
#define MMH_KERNEL_MFMA32B_128X128_DMA 62
