// What the kernels of the three-product fp16 scheme (gemm_x6.hip, gemm_dw.hip, angle.hip) must agree on, and the
// DMA-to-LDS staging primitives of the two pipelined GEMMs.  The slicers stay with their kernels: their operand forms differ.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));    // accumulator of a 32 x 32 MFMA
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));   // one operand of v_mfma_f32_32x32x16_f16

// power-of-two scale that puts a tensor with the given max|x| just below 2^15 (fp16 max is 65504); 1 for an
// all-zero / denormal / non-finite tensor (nothing to protect; inf and nan propagate through the fp16 slices).
// The weight images and the activations are scaled by this ONE function: a copy that drifts is a silent factor of two.
__device__ __forceinline__ float f16_scale(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 255u);  // amax < 2^(e-126)
    if (e == 0 || e == 255) return 1.0f;
    int se = 268 - e;                                           // 2^(141-e)
    se = se > 254 ? 254 : se;
    return __uint_as_float((unsigned)se << 23);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_barrier without the vmcnt(0)/lgkmcnt(0) drain that __syncthreads() implies: DMA stages stay in flight across it
__device__ __forceinline__ void block_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// 64 lanes x 16 B -> 1 KiB of LDS at lds_wave_base (wave-uniform) + lane*16, from sbase (wave-uniform, scalar
// registers) + lane_off (+ OFF).  Written as the instruction itself: through __builtin_amdgcn_global_load_lds hipcc
// builds a 64-bit vector address per piece and k-step (v_lshl_add_u64) and, in the pipelined loop, answered a ds_read
// whose destination landed on such an address pair with s_waitcnt vmcnt(0) - a wait for the DMA issued just before.
// The compiler neither sees these loads (every vmcnt wait on them is explicit, see wait_vmcnt) nor uses M0 for
// anything else on gfx950.  (Default cache policy: nt on the read-once activation tile measured 10 % slower.)
template <int OFF = 0>
__device__ __forceinline__ void dma16(const void* sbase, unsigned lane_off, unsigned char* lds_wave_base) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%3"
                 :
                 : "s"((unsigned)(size_t)lds_wave_base), "v"(lane_off), "s"(sbase), "n"(OFF)
                 : "memory");
}
