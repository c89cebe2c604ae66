// What the baselines' row kernels (hgr_dgp.hip, hgr_dgp_train.hip, hgr_free.hip, hgr_cnzsl.hip) share: the counter mix, the block
// reductions of a 256-thread workgroup, the coupled-decay Adam update and the fp32-row argument check; their slices-per-thread
// ladder is hgr_by_nv4 (hgr_launch.h).  hgr_train.hip keeps its own reductions (they associate as (s0 + s1) + (s2 + s3): other bits)
// and its own AdamW.
#pragma once
#include "hgr_launch.h"

// murmur3's 32-bit finaliser: the mix of hgr_dropout_counter and of the counter normal (host twin: baseline/_shared.py fmix32)
__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// Reductions over a workgroup of 256 threads; every thread gets the result.  red: [4].  A shuffle tree over the wave, then the four
// waves in order, ((red0 + red1) + red2) + red3.  The leading barrier lets a kernel call them back to back on the same `red`.
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// torch.optim.Adam with coupled weight decay on one element: the decay is part of the gradient the moments see.
// step_size = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t).
__device__ __forceinline__ void adam_l2_update(float &p, float g, float &m, float &v, float beta1, float beta2, float eps, float wd,
                                               float step_size, float inv_sqrt_bc2) {
    const float pi = p;
    const float gi = g + wd * pi;
    const float mi = m + (gi - m) * (1.f - beta1);
    const float vi = v * beta2 + (1.f - beta2) * gi * gi;
    m = mi;
    v = vi;
    p = pi - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

// fp32 rows read and written as float4: 16-byte aligned, the leading dimension a multiple of 4 and at least C.  A null pointer
// passes: an entry point that needs the operand asks for it by name first.
static inline bool rows_f32_ok(const void *p, int64_t ld, int C) { return hgr_aligned(p, 16) && ld % 4 == 0 && ld >= C; }
