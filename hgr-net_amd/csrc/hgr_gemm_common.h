// Shared pieces of the NT GEMM family (hgr_gemm_128 / _256 / _duo .hip + the host entry points in hgr_gemm.hip):
// the argument block, the epilogue helpers and the wait / barrier macros of the counted-vmcnt pipelines.
//
// C[M,N] = epilogue(A[M,K] . W[N,K]^T) on the gfx950 matrix cores.  Both operands are K-contiguous (activations row-major,
// nn.Linear weights [out, in]), so a lane's MFMA fragment (8 consecutive k of one row) is one 16-byte LDS read for either operand.
// W is fed as the MFMA "A" operand and the activations as "B", i.e. a wave computes C^T tiles: the 4 accumulator registers of a
// lane are 4 CONSECUTIVE n of one output row m, so bias / residual / stores are 8- or 16-byte vector accesses.
// Staging is LDS-DMA (global_load_lds_dwordx4) into a lane-linear image of 128-byte rows; the bank-conflict swizzle
// chunk' = chunk ^ (row & 7) is applied on the per-lane SOURCE address and again on the ds_read address (cdna_hip_programming.md
// rule 21).  Block -> tile maps are XCD-aware (blocks b, b + 8 share an L2) with a grouped raster.
#pragma once
#include "hgr_common.h"
#include <stdlib.h>
#include <type_traits>

namespace hgr_gemm {

constexpr int BK = 64;

struct GemmArgs {
    const char *A = nullptr; int64_t lda = 0;
    const char *W = nullptr; int64_t ldw = 0;
    void *C = nullptr; int64_t ldc = 0;
    const float *bias = nullptr;
    const float *res = nullptr; int64_t ldr = 0;
    int M = 0, N = 0, K = 0;
    int tiles_m = 0, tiles_n = 0;
    int m_fastest = 0;   // 1: consecutive tile ids walk M first (W panel shared), 0: walk N first
    int vec_ok = 0;  // C / residual rows allow 4-element vector access
    int dbg = 0;     // diagnostics only (HGR_GEMM_DBG): 1 = skip MFMAs, 2 = skip LDS-DMA issue, 3 = skip epilogue
    // implicit-GEMM 3x3 convolution (CONV kernels only): A is an NHWC image [B, H, W, C], pad 1
    int cH = 0, cW = 0, cC = 0, cStride = 0, cHo = 0, cWo = 0;
    unsigned cMagic = 0;  // ceil(2^32 / cC): __umulhi(k, cMagic) == k / cC for every k < 9 * cC + 64 (k * cC < 2^32)
    int cUni = 0;     // cC % 64 == 0: a 64-deep K-tile lies inside ONE tap, so tap / kernel offset are wave-uniform per K-tile (scalar ALU)
    // split-K (gemm_nt_128 only): blockIdx.y = split s works on K columns [s * kc, min(K, (s + 1) * kc)) and writes its own
    // fp32 partial C + s * csplit elements; 0 = off
    int kc = 0; int64_t csplit = 0;
    // LayerNorm folded into the GEMMs around it (gemm_nt_duo only, LN template parameter):
    //   producer (LN = 1, x += A W^T + b): the residual stream is kept as a 16-bit pair (hi, lo) with x = hi + lo - 4 bytes per
    //            element like fp32, and hi IS the next GEMM's A operand; per row and 64-column slot it also emits the partial
    //            (sum, sum of squares) of the new values -> ln_stats [M][ln_slots][2]
    //   consumer (LN = 2, y = LN(x) W^T + b): A is the un-normalised 16-bit x, W the gamma-folded weight,
    //            y = rstd_m (acc - mean_m ln_s[n]) + ln_c[n] with row statistics from ln_stats (K = row width)
    float *ln_stats = nullptr; int ln_slots = 0; float ln_eps = 0.f;
    void *ln_xh = nullptr, *ln_xl = nullptr; int64_t ln_ldx = 0;      // producer: the residual stream as a 16-bit PAIR, x = hi + lo (hi in the MFMA type, lo f16)
    const float *ln_s = nullptr, *ln_c = nullptr;
    // producer range guard: when a 64-column slot's sum of squares exceeds ln_guard (or is inf / NaN) its bit pattern is
    // atomicMax'ed into *ln_flag (0 = the stream stayed in range); null = no guard
    unsigned *ln_flag = nullptr; float ln_guard = 0.f;
    int group = 0;   // gemm_nt_duo: row (or column) panels per raster group (HGR_GEMM_GROUP, default 4)
    // gemm_nt_duo tail plan (duo_plan): blocks [0, nbig) = full 256 x 128 tiles on row panels [0, big_panels), the remaining blocks =
    // 128 x 128 half tiles on the rows behind them (tiles_m_half panels of 128 rows).  No tail: nbig = grid, big_panels = tiles_m.
    int nbig = 0, big_panels = 0, tiles_m_half = 0;
    // HGR_EPI_QGELU_GRAD16 on gemm_nt_duo only (hgr_gemm_nt_qgelu_grad_colsum): column sums of the ROUNDED 16-bit outputs per 64-row
    // unit, colsum[unit][n] for unit < colsum_units = ceil(M / 64) - the bias gradient of the layer below without a second pass over C
    float *colsum = nullptr; int colsum_units = 0;
    int total = 0;   // gemm_nt_duo, persistent form: number of virtual blocks (0 = gridDim.x, one tile per workgroup)
};

// The part of the argument block every host entry point fills alike; the entry point then sets only what is specific to it.
// m_fastest: each XCD owns a contiguous range of tile ids; the operand indexed by the slow tile index is fetched ~once, the other one
// once per XCD.  Make the bigger operand the once-fetched one.
inline int gemm_m_fastest(int M, int N, int K) { return (int64_t)N * K > (int64_t)M * K ? 1 : 0; }
inline GemmArgs gemm_args(const void *A, int64_t lda, const void *W, int64_t ldw, void *C, int64_t ldc, int M, int N, int K, bool vec_ok, int dbg) {
    GemmArgs a;
    a.A = (const char *)A; a.lda = lda; a.W = (const char *)W; a.ldw = ldw; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K;
    a.m_fastest = gemm_m_fastest(M, N, K); a.vec_ok = vec_ok ? 1 : 0; a.dbg = dbg;
    return a;
}


// 16 zero bytes every out-of-bounds conv tap (and the K padding) is loaded from; one copy per translation unit (no -fgpu-rdc)
static __device__ __attribute__((aligned(16))) unsigned int hgr_zero_page[4] = {0u, 0u, 0u, 0u};

// x * sigmoid(1.702 x) with v_exp_f32 + v_rcp_f32 (1 ulp each): an IEEE fp32 divide costs ~10 VALU ops per
// element and, at 128 elements per lane, dominated the c_fc epilogue (measured 88 us of a 206 us launch).
__device__ __forceinline__ float quick_gelu(float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * v));
}


// QuickGELU to 16 bits, the product rounded once (mul16: hipcc merges a product with its conversion in some kernel forms and not in
// others - every form goes through these)
template <int DT> __device__ __forceinline__ typename T16<DT>::elem quick_gelu16(float v) {
    return mul16<DT>(v, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * v)));
}
// the expression hgr_quickgelu16 (hgr_train.hip) evaluates, operation for operation: the dual-output forward must give its bits
template <int DT> __device__ __forceinline__ typename T16<DT>::elem quick_gelu_train16(float x) {
    const float z = 1.702f * x;
    return mul16<DT>(x, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z)));
}
// d/dx of quick_gelu: s (1 + 1.702 x (1 - s)), s = sigmoid(1.702 x) - the expression of hgr_quickgelu16's backward
__device__ __forceinline__ float quick_gelu_grad(float x) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * x));
    return s * (1.0f + 1.702f * x * (1.0f - s));
}
// The folded LayerNorm's arithmetic, written with explicit fused multiply-adds: every kernel that finalises row statistics or applies
// them (the consumer epilogues of gemm_nt_duo, hgr_gemm_nt_ln_mha) must round identically, and left to -ffp-contract the compiler is
// free to contract `s2 * inv - mean * mean` and `acc - mean * s` differently from one kernel to the next (the in_proj + attention kernel
// differed from gemm_nt_ln + hgr_mha in 578 of 19.7 M f16 outputs by one ulp before this).
__device__ __forceinline__ float2 ln_finalize(float s1, float s2, float inv_k, float eps) {
    const float mean = s1 * inv_k;
    const float msq = mean * mean;
    return make_float2(mean, rsqrtf(fmaxf(__builtin_fmaf(s2, inv_k, -msq), 0.f) + eps));
}
// rstd * (acc - mean * s_n) + c_n
__device__ __forceinline__ float ln_apply(float2 mr, float acc, float s_n, float c_n) {
    return __builtin_fmaf(mr.y, __builtin_fmaf(-mr.x, s_n, acc), c_n);
}

// four consecutive outputs of a folded-LayerNorm consumer, rounded to the MFMA type: rstd (acc - mean s_n) + c_n [through QuickGELU]
template <int DT, bool GELU> __device__ __forceinline__ u32x2 ln_out16(float2 mr, f32x4 acc, f32x4 s4, f32x4 c4);

// The folded LayerNorm's output through QuickGELU in 4 plain + 2 quarter-rate vector instructions per element (round 6; ln_apply +
// quick_gelu: 5 + 2).  With k = -1.702 log2(e) and the row's rstd and the column's c pre-multiplied by k (once per row / column):
//     w = k v  straight out of the second FMA,   e = 2^w,   v sigmoid(1.702 v) = v / (1 + e) = w / (k + k e)
// Every folded-LayerNorm consumer with QuickGELU (gemm_nt_duo, gemm_nt_p8) goes through this function, so they keep
// rounding alike.
constexpr float QG_K = -1.702f * 1.4426950408889634f;
__device__ __forceinline__ float ln_apply_gelu(float2 mr, float acc, float s_n, float c_n) {
    const float w = __builtin_fmaf(mr.y * QG_K, __builtin_fmaf(-mr.x, s_n, acc), c_n * QG_K);
    return w * __builtin_amdgcn_rcpf(__builtin_fmaf(QG_K, __builtin_amdgcn_exp2f(w), QG_K));
}

template <int DT, bool GELU> __device__ __forceinline__ u32x2 ln_out16(float2 mr, f32x4 acc, f32x4 s4, f32x4 c4) {
    u32x2 o;
    if (GELU) {
        const float rk = mr.y * QG_K;
        float w[4], r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = __builtin_fmaf(rk, __builtin_fmaf(-mr.x, s4[e], acc[e]), c4[e] * QG_K);
            r[e] = __builtin_amdgcn_rcpf(__builtin_fmaf(QG_K, __builtin_amdgcn_exp2f(w[e]), QG_K));
        }
        o[0] = mul_pack16<DT>(w[0], r[0], w[1], r[1]);
        o[1] = mul_pack16<DT>(w[2], r[2], w[3], r[3]);
    } else {
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = __builtin_fmaf(-mr.x, s4[e], acc[e]);
        o[0] = fma_pack16<DT>(mr.y, u[0], c4[0], mr.y, u[1], c4[1]);
        o[1] = fma_pack16<DT>(mr.y, u[2], c4[2], mr.y, u[3], c4[3]);
    }
    return o;
}

__host__ __device__ constexpr bool epi_has_bias(int epi) { return epi != HGR_EPI_NONE && epi != HGR_EPI_ACCUM && epi != HGR_EPI_QGELU_GRAD16; }
__host__ __device__ constexpr bool epi_has_idn16(int epi) { return epi == HGR_EPI_BIAS_ADD16_RELU || epi == HGR_EPI_QGELU_GRAD16; }

// One lane's 4 consecutive outputs C[m][n .. n+3] of an accumulator tile: bias / QuickGELU / residual,
// then a 16-byte (fp32) or 8-byte (16-bit) store; scalar tail only at the N edge or for odd strides.
template <int DT, int EPI, bool OUT32>
__device__ __forceinline__ void store_quad(const GemmArgs &p, f32x4 v, int m, int n) {
    typedef typename T16<DT>::elem E;
    if (n + 3 < p.N && p.vec_ok) {
        if (epi_has_bias(EPI)) v += *(const f32x4 *)(p.bias + n);
        if (EPI == HGR_EPI_ACCUM) v += *(const f32x4 *)((const float *)p.C + (int64_t)m * p.ldc + n);
        const f32x4 v0 = v;                 // before the last product (QuickGELU / its gradient): the 16-bit forms round that product once
        f32x4 gq = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (EPI == HGR_EPI_BIAS_QUICKGELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = quick_gelu(v[e]);
        }
        if (EPI == HGR_EPI_BIAS_RESIDUAL) v += *(const f32x4 *)(p.res + (int64_t)m * p.ldr + n);
        if (epi_has_idn16(EPI)) {
            const typename T16<DT>::vec4 idn = *(const typename T16<DT>::vec4 *)((const E *)(const void *)p.res + (int64_t)m * p.ldr + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (EPI == HGR_EPI_QGELU_GRAD16) { gq[e] = quick_gelu_grad((float)idn[e]); v[e] = v[e] * gq[e]; }
                else v[e] = v[e] + (float)idn[e];
            }
        }
        if (EPI == HGR_EPI_BIAS_RELU || EPI == HGR_EPI_BIAS_ADD16_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (OUT32) *(f32x4 *)((float *)p.C + (int64_t)m * p.ldc + n) = v;
        else if (EPI == HGR_EPI_BIAS_QUICKGELU || EPI == HGR_EPI_QGELU_GRAD16) {
            typename T16<DT>::vec4 o;                      // the last product and the rounding as ONE operation (v0 = its first factor)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = EPI == HGR_EPI_BIAS_QUICKGELU ? quick_gelu16<DT>(v0[e]) : mul16<DT>(v0[e], gq[e]);
            *(typename T16<DT>::vec4 *)((E *)p.C + (int64_t)m * p.ldc + n) = o;
        } else *(typename T16<DT>::vec4 *)((E *)p.C + (int64_t)m * p.ldc + n) = cvt4<DT>(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int e = 0; e < 4 && n + e < p.N; ++e) {
        float x = v[e];
        if (epi_has_bias(EPI)) x += p.bias[n + e];
        if (EPI == HGR_EPI_ACCUM) x += ((const float *)p.C)[(int64_t)m * p.ldc + n + e];
        const float x0 = x;
        float gx = 0.f;
        if (EPI == HGR_EPI_BIAS_QUICKGELU) x = quick_gelu(x);
        if (EPI == HGR_EPI_BIAS_RESIDUAL) x += p.res[(int64_t)m * p.ldr + n + e];
        if (EPI == HGR_EPI_BIAS_ADD16_RELU) x += (float)((const E *)(const void *)p.res)[(int64_t)m * p.ldr + n + e];
        if (EPI == HGR_EPI_QGELU_GRAD16) { gx = quick_gelu_grad((float)((const E *)(const void *)p.res)[(int64_t)m * p.ldr + n + e]); x *= gx; }
        if (EPI == HGR_EPI_BIAS_RELU || EPI == HGR_EPI_BIAS_ADD16_RELU) x = fmaxf(x, 0.f);
        if (OUT32) ((float *)p.C)[(int64_t)m * p.ldc + n + e] = x;
        else if (EPI == HGR_EPI_BIAS_QUICKGELU) ((E *)p.C)[(int64_t)m * p.ldc + n + e] = quick_gelu16<DT>(x0);
        else if (EPI == HGR_EPI_QGELU_GRAD16) ((E *)p.C)[(int64_t)m * p.ldc + n + e] = mul16<DT>(x0, gx);
        else ((E *)p.C)[(int64_t)m * p.ldc + n + e] = (E)x;
    }
}

// Interior-tile forms (the caller guarantees vec_ok and that the whole quad is inside C).  The quad's second addend
// (fp32 residual, 16-bit identity or the old C for ACCUM) is loaded by load_addend() and handed to store_quad_full():
// callers fetch a batch of addends, then store the batch.  Interleaved load / store pairs serialise completely -
// residual and C may alias, so hipcc keeps every load behind the previous store with a vmcnt(0) between them.
template <int DT, int EPI>
__device__ __forceinline__ f32x4 load_addend(const GemmArgs &p, int m, int n) {
    typedef typename T16<DT>::elem E;
    if (EPI == HGR_EPI_ACCUM) return *(const f32x4 *)((const float *)p.C + (int64_t)m * p.ldc + n);
    if (EPI == HGR_EPI_BIAS_RESIDUAL) return *(const f32x4 *)(p.res + (int64_t)m * p.ldr + n);
    if (epi_has_idn16(EPI)) {
        const typename T16<DT>::vec4 idn = *(const typename T16<DT>::vec4 *)((const E *)(const void *)p.res + (int64_t)m * p.ldr + n);
        return (f32x4){(float)idn[0], (float)idn[1], (float)idn[2], (float)idn[3]};
    }
    return (f32x4){0.f, 0.f, 0.f, 0.f};
}

template <int DT, int EPI, bool OUT32>
__device__ __forceinline__ void store_quad_full(const GemmArgs &p, f32x4 v, f32x4 bq, f32x4 addend, int m, int n) {
    typedef typename T16<DT>::elem E;
    if (epi_has_bias(EPI)) v += bq;
    if (!OUT32 && (EPI == HGR_EPI_BIAS_QUICKGELU || EPI == HGR_EPI_QGELU_GRAD16)) {
        typename T16<DT>::vec4 o;                          // the last product rounded once (mul16)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = EPI == HGR_EPI_BIAS_QUICKGELU ? quick_gelu16<DT>(v[e]) : mul16<DT>(v[e], quick_gelu_grad(addend[e]));
        *(typename T16<DT>::vec4 *)((E *)p.C + (int64_t)m * p.ldc + n) = o;
        return;
    }
    if (EPI == HGR_EPI_BIAS_QUICKGELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = quick_gelu(v[e]);
    }
    if (EPI == HGR_EPI_ACCUM || EPI == HGR_EPI_BIAS_RESIDUAL || EPI == HGR_EPI_BIAS_ADD16_RELU) v += addend;
    if (EPI == HGR_EPI_QGELU_GRAD16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= quick_gelu_grad(addend[e]);
    }
    if (EPI == HGR_EPI_BIAS_RELU || EPI == HGR_EPI_BIAS_ADD16_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (OUT32) *(f32x4 *)((float *)p.C + (int64_t)m * p.ldc + n) = v;
    else *(typename T16<DT>::vec4 *)((E *)p.C + (int64_t)m * p.ldc + n) = cvt4<DT>(v[0], v[1], v[2], v[3]);
}


// LDS-DMA in its BUFFER form (buffer_load_dwordx4 ... offen lds): the per-lane source is a 32-bit byte offset into a buffer resource
// (128-bit descriptor in SGPRs: base, no stride, 4 GB of records, raw dword format) and the K-tile advance rides in the scalar offset
// operand - one address VGPR per instruction and no VALU, where the global form (global_load_lds_dwordx4) needs a 64-bit per-lane
// pointer, i.e. a 64-bit add (two VALU) and two address VGPRs per instruction.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dma_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)0xFFFFFFFFu, 0x00020000);
}
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff, char *lds_dst) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (AS3 void *)lds_dst, 16, (int)voff, soff, 0, 0);
}

// R interval end: my share of the piece the NEXT read interval needs has landed (counted vmcnt), my own
// ds_reads are complete (so the slot they read may be refilled), then the barrier.  M interval end: barrier.
// rwait<N>(): the count as a constant expression (a loop shared by two tile shapes waits for MT + 4); HGR_RWAIT(N) is the same call.
template <int N> __device__ __forceinline__ void rwait() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
#define HGR_RWAIT(N) hgr_gemm::rwait<N>()
#define HGR_RBAR() do { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define HGR_MBAR() do { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_barrier" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)


// 16 MFMAs of a phase interleaved with NR LDS reads, NW LDS writes and NV vector-memory instructions (LDS-DMAs) that do not depend on
// them: the scheduler is told to issue them in the gaps between MFMAs instead of in a block in front (the fragment-prefetch loop of
// gemm_nt_duo's LayerNorm consumers)
template <int NR, int NW, int NV, int M_, int NM = 16>
__device__ __forceinline__ void mfma16_interleave_step() {
    if constexpr (M_ < NM) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        constexpr int DR = (M_ + 1) * NR / NM - M_ * NR / NM, DW = (M_ + 1) * NW / NM - M_ * NW / NM, DV = (M_ + 1) * NV / NM - M_ * NV / NM;
        if constexpr (DR > 0) __builtin_amdgcn_sched_group_barrier(0x100, DR, 0);
        if constexpr (DW > 0) __builtin_amdgcn_sched_group_barrier(0x200, DW, 0);
        if constexpr (DV > 0) __builtin_amdgcn_sched_group_barrier(0x020, DV, 0);
        mfma16_interleave_step<NR, NW, NV, M_ + 1, NM>();
    }
}
template <int NR, int NW, int NV>
__device__ __forceinline__ void mfma16_interleave() { mfma16_interleave_step<NR, NW, NV, 0>(); }
// the same over 8 MFMAs (one k half of a phase)
template <int NR, int NW, int NV>
__device__ __forceinline__ void mfma8_interleave() { mfma16_interleave_step<NR, NW, NV, 0, 8>(); }

// ---- pieces more than one kernel of the family is built from: one copy each, so that what must round alike does --------------------

// Tiles -> XCDs.  Workgroups b, b + 8, b + 16, ... run on XCD b & 7 and share its L2; the rasters give every XCD a CONTIGUOUS range of
// the ntiles tile (or workgroup) ids, the first ntiles % 8 XCDs one more than the others: the first id of XCD xcd's range, and its length.
__device__ __forceinline__ int xcd_first_tile(int ntiles, int xcd) {
    const int q8 = ntiles >> 3, r8 = ntiles & 7;
    return xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
}
__device__ __forceinline__ int xcd_tile_count(int ntiles, int xcd) { return (ntiles >> 3) + (xcd < (ntiles & 7) ? 1 : 0); }

// LayerNorm consumers: (sum, sum of squares) of one row from the producer's per-slot partial sums, sp = the row's `slots` pairs (two per
// 16-byte load), summed in slot order.  The usual row widths get all their loads issued back to back (a load inside a run-time loop is
// waited for on the spot: six dependent L2 round trips for width 768).  Callers clamp the row and call ln_finalize themselves.
__device__ __forceinline__ void ln_row_sums(const f32x4 *sp, int slots, float &s1, float &s2) {
    float a1 = 0.f, a2 = 0.f;
    auto fixed = [&](auto nq_tag) {
        constexpr int NQ = decltype(nq_tag)::value;
        f32x4 t[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) t[i] = sp[i];
#pragma unroll
        for (int i = 0; i < NQ; ++i) { a1 += t[i][0] + t[i][2]; a2 += t[i][1] + t[i][3]; }
    };
    switch (slots) {
        case 4: fixed(std::integral_constant<int, 2>()); break;      // width 256
        case 8: fixed(std::integral_constant<int, 4>()); break;      // 512
        case 10: fixed(std::integral_constant<int, 5>()); break;     // 640
        case 12: fixed(std::integral_constant<int, 6>()); break;     // 768
        case 16: fixed(std::integral_constant<int, 8>()); break;     // 1024
        default:
            for (int i = 0; i < slots / 2; ++i) { const f32x4 t = sp[i]; a1 += t[0] + t[2]; a2 += t[1] + t[3]; }
    }
    s1 = a1; s2 = a2;
}

// Residual producers (gemm_nt_duo with LN = 1, gemm_nt_res_wide): one pass of the epilogue on a lane's 8 consecutive columns of a row.
// The kernels keep their own loads, stores, buffer ring and pass order; the arithmetic is here.
// new x = (acc + bias) + old x, the old x decoded from the pair (pair_dec4: hi's bits + the low byte's 8 mantissa bits)
template <int DT> __device__ __forceinline__ void pair_pass_values(f32x4 lo4, f32x4 hi4, f32x4 b8lo, f32x4 b8hi, typename T16<DT>::vec8 oh, u32x2 ol, float (&v)[8]) {
    v[0] = (lo4[0] + b8lo[0]) + pair_dec4<DT, 0>(oh[0], ol[0]); v[1] = (lo4[1] + b8lo[1]) + pair_dec4<DT, 1>(oh[1], ol[0]);
    v[2] = (lo4[2] + b8lo[2]) + pair_dec4<DT, 2>(oh[2], ol[0]); v[3] = (lo4[3] + b8lo[3]) + pair_dec4<DT, 3>(oh[3], ol[0]);
    v[4] = (hi4[0] + b8hi[0]) + pair_dec4<DT, 0>(oh[4], ol[1]); v[5] = (hi4[1] + b8hi[1]) + pair_dec4<DT, 1>(oh[5], ol[1]);
    v[6] = (hi4[2] + b8hi[2]) + pair_dec4<DT, 2>(oh[6], ol[1]); v[7] = (hi4[3] + b8hi[3]) + pair_dec4<DT, 3>(oh[7], ol[1]);
}
// the new pair of those 8 values: pair_split()'s bits through pair_split2 / pair_put_q (hgr_common.h), ~5 instead of ~8 vector
// instructions per element
template <int DT> __device__ __forceinline__ void pair_pass_split(const float (&v)[8], u32x4 &nh, u32x2 &nl) {
    unsigned tq[8];
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) nh[e2] = pair_split2<DT>(v[2 * e2], v[2 * e2 + 1], tq[2 * e2], tq[2 * e2 + 1]);
    unsigned n0, n1;
    pair_put_q<DT, 0>(n0, tq[0]); pair_put_q<DT, 1>(n0, tq[1]); pair_put_q<DT, 2>(n0, tq[2]); pair_put_q<DT, 3>(n0, tq[3]);
    pair_put_q<DT, 0>(n1, tq[4]); pair_put_q<DT, 1>(n1, tq[5]); pair_put_q<DT, 2>(n1, tq[6]); pair_put_q<DT, 3>(n1, tq[7]);
    nl = (u32x2){n0, n1};
}
// their share of the slot's (sum, sum of squares): the pairing of the 4-column form, stage by stage
__device__ __forceinline__ void pair_pass_sums(const float (&v)[8], float &s1, float &s2) {
    s1 = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    s2 = (__builtin_fmaf(v[0], v[0], v[1] * v[1]) + __builtin_fmaf(v[2], v[2], v[3] * v[3])) +
         (__builtin_fmaf(v[4], v[4], v[5] * v[5]) + __builtin_fmaf(v[6], v[6], v[7] * v[7]));
}
// ... and the slot's totals over the 8 lanes of a row (64 columns), for the two rows of a pass: three DPP stages, the four chains
// advancing together (DPP latencies overlap); every lane of the row ends with the totals
template <int CTRL> __device__ __forceinline__ void pair_pass_dpp_stage(float (&s1)[2], float (&s2)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        s1[q] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s1[q]), CTRL, 0xF, 0xF, true));
        s2[q] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s2[q]), CTRL, 0xF, 0xF, true));
    }
}
__device__ __forceinline__ void pair_pass_reduce(float (&s1)[2], float (&s2)[2]) {
    pair_pass_dpp_stage<0xB1>(s1, s2); pair_pass_dpp_stage<0x4E>(s1, s2); pair_pass_dpp_stage<0x141>(s1, s2);
}

// One K-tile of the 8-wave ping-pong loop whose phases split a wave's 128 columns (gemm_nt_p8: MT = 4 m tiles per wave, gemm_nt_res_wide:
// MT = 5).  st = the K-tile's stage; PA / PW0 / PW1 = the pieces' offsets inside a stage; issue1 / issue2 = the caller's LDS-DMA issue
// for the phases (PW1(t+1), MT-independent 2 instructions; PA(t+2) + PW0(t+2), MT + 2): a count = "my N youngest may still be in flight".
//     ph1(t): reads A (2 MT x ds_read_b128), W columns 0-63 (8 x)    issue1 behind the reads    waits vmcnt(MT + 4): PW1(t) landed
//     ph2(t): reads W columns 64-127 (8 x), A fragments stay          issue2 behind the reads    waits vmcnt(MT + 4): PA(t+1), PW0(t+1) landed
// MODE 0: steady state (t + 2 < nk), 1: second-last K-tile (issue1 only), 2: last K-tile (no issue)
template <int DT, int MT, int MODE, int PA, int PW0, int PW1, typename Issue1, typename Issue2>
__device__ __forceinline__ void pingpong_ktile(const char *st, int offA, int offW, int sw0, int sw1, f32x4 (&acc)[MT][8],
                                               typename T16<DT>::vec8 (&wf)[4][2], typename T16<DT>::vec8 (&af)[MT][2], Issue1 issue1, Issue2 issue2) {
    typedef typename T16<DT>::vec8 vec8;
    // ---- ph1: all rows of the wave x its columns 0-63 ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        wf[j][0] = *(const vec8 *)(st + PW0 + offW + j * 2048 + sw0);
        wf[j][1] = *(const vec8 *)(st + PW0 + offW + j * 2048 + sw1);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        af[i][0] = *(const vec8 *)(st + PA + offA + i * 2048 + sw0);
        af[i][1] = *(const vec8 *)(st + PA + offA + i * 2048 + sw1);
    }
    if (MODE <= 1) issue1();                                   // behind the reads; its slot was last read in ph2(t - 1), two barriers ago
    if (MODE <= 1) rwait<MT + 4>(); else rwait<0>();           // PW1(t) landed
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = T16<DT>::mfma16(wf[j][kk], af[i][kk], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    HGR_MBAR();
    // ---- ph2: columns 64-127, the A fragments stay ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        wf[j][0] = *(const vec8 *)(st + PW1 + offW + j * 2048 + sw0);
        wf[j][1] = *(const vec8 *)(st + PW1 + offW + j * 2048 + sw1);
    }
    if (MODE == 0) issue2();                                   // read in ph1(t), two barriers ago
    if (MODE == 0) rwait<MT + 4>(); else if (MODE == 1) rwait<2>(); else HGR_RBAR();      // PA(t+1), PW0(t+1) landed
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][4 + j] = T16<DT>::mfma16(wf[j][kk], af[i][kk], acc[i][4 + j]);
    __builtin_amdgcn_s_setprio(0);
    HGR_MBAR();
}

// ---- launchers, one per translation unit (the kernels are templates; host code selects by value) ------------------------
enum { V128_PLAIN = 0, V128_TALL = 1, V128_CONV = 2, V128_CONV_TALL = 3 };
// gemm_nt_128 family.  PLAIN: epi any (K == 64 with 16-bit bias epilogues takes the one-stage variant); TALL: 256 x 64 tiles,
// epi = BIAS_RELU, 16-bit out; CONV / CONV_TALL: implicit-GEMM 3x3 convolution, epi = BIAS_RELU or NONE, 16-bit out.
void launch_128(const GemmArgs &a, int dtype, int epi, bool out32, int variant, dim3 grid, hipStream_t s);
// gemm_nt_256: plain (any epi) or the implicit-GEMM convolution (BIAS_RELU, 16-bit out)
void launch_256(const GemmArgs &a, int dtype, int epi, bool out32, bool conv, dim3 grid, hipStream_t s);
// gemm_nt_duo: ln = 0 plain (any epi), 1 LayerNorm producer, 2 LayerNorm consumer (epi BIAS / BIAS_QUICKGELU), 4 dual output
// (pre-activation + QuickGELU), 5 the 3 x 3 convolution.  ln = 1 walks a.total > grid.x virtual blocks (plan_duo, hgr_gemm.hip)
void launch_duo(const GemmArgs &a, int dtype, int epi, bool out32, int ln, dim3 grid, hipStream_t s);
// hgr_gemm_p8.hip: the LayerNorm-folded consumer as one persistent 512-thread workgroup per CU on 256 x 256 tiles
bool p8_covers(int M, int N, int K);
void launch_p8(const GemmArgs &a, int dtype, int act, dim3 grid, hipStream_t s);

// first stage of hgr_logits_eval (hgr_logits_slab.hip): 512-row x 96-column tiles, one per CU, evaluation consumers in the epilogue
struct SlabArgs {
    const char *A = nullptr; int64_t lda = 0;          // features [M, K] 16-bit
    const char *W = nullptr; int64_t ldw = 0;          // level-sorted class matrix [Np, K] 16-bit, Np % 96 == 0
    int M = 0, K = 0, Np = 0;
    const int *tpos = nullptr, *epos = nullptr;              // [Np] train / test position of every permuted column (-1 = not in the subset / padding)
    unsigned long long *ev_key = nullptr;          // [M][S]      S = Np / 32
    float *ev_tmax = nullptr, *ev_m2 = nullptr; int *ev_p1 = nullptr;  // [M][S][2]
    int S = 0;
    int dbg = 0;                             // HGR_LS_DBG (timing experiments only, wrong results): 1 skip the MFMAs, 2 skip the feature DMAs, 4 skip the class-row DMAs, 8 skip the epilogue, 16 skip the warm-up touches
};
void launch_logits_slab(const SlabArgs &a, int dtype, hipStream_t s);

}  // namespace hgr_gemm
