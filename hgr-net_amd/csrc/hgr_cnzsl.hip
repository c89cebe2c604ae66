// CNZSL baseline (baseline/CNZSL/cnzsl.py:139-219): what the attribute -> prototype network needs beside the fp32 products,
// hgr_l2norm_rows / hgr_l2norm_bwd, hgr_ce_rows and hgr_adam_l2.  With u = z + b, z = h1 W2^T [S, H], and the reference's
// ClassStandardization over the class dimension - (x - mean_0(x)) / (var_0(x) + eps): UNBIASED variance, and a division by
// the variance, not by a standard deviation -
//
//     hgr_cnzsl_std_chain_fwd   a = relu((u - m1) / (v1 + eps)),  c = (a - m2) / (v2 + eps)     modules 2 (bias) .. 5
//     hgr_cnzsl_std_chain_bwd   dz = d loss / d z from dc, through layer 5, the ReLU mask a > 0 and layer 3;  dbias = colsum(dz)
//     hgr_bias_relu_f32         y = relu(x + b)                                                  modules 0/1 and 6/7
//     hgr_relu_bwd_colsum_f32   dx = dy [y > 0],  db = colsum(dx)
//
// The chain is column-local: a workgroup (1024 threads forward, 512 backward) owns a STRIP of 16 columns and all S rows.  Thread t holds the float4
// column quad t & 3 of the rows t >> 2, t >> 2 + threads / 4, ...; a strip row is 64 contiguous bytes.  Up to CN_RES_ROWS rows the strip
// lives in LDS (64 B per row), so the statistics passes - mean first, then the centred second moment, as torch.var does - read
// memory once; beyond that every pass re-reads the strip from L2 (a thread only ever re-reads what it wrote itself).
// Summation order: per thread its rows in ascending order, then a shuffle tree over the 16 row slots of a wave, then the
// workgroup's waves in order - a function of S alone, never of the grid.  No atomics, nothing allocated.
#include "hgr_rows.h"

namespace {

constexpr int NT = 256;
constexpr int CN_NT = 1024;                     // the chain forward: 16 waves, so that a thread walks S / 256 rows per pass
constexpr int CB_NT = 512;                      // the chain backward: 8 waves (at 1024 threads its registers would spill)
constexpr int CN_COLS = 16;                     // strip width: 4 quads
constexpr int CN_SLOTS = CN_NT / 4;             // 256 row slots
constexpr int CN_RES_ROWS = 2048;               // resident strip: 2048 rows x 64 B = 128 KiB of the CU's 160 KiB
constexpr int RB_ROWS = 256;                    // rows per partial of hgr_relu_bwd_colsum_f32

__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// sum over the threads that hold the same column quad (all rows of the strip); every thread gets the result.  red: [WAVES * 4]
template <int WAVES>
__device__ __forceinline__ f32x4 strip_sum(f32x4 v, f32x4 *red) {
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane < 4) red[wave * 4 + lane] = v;
    __syncthreads();
    const int q = threadIdx.x & 3;
    f32x4 s = red[q];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w * 4 + q];
    return s;
}

__device__ __forceinline__ f32x4 relu4(f32x4 x) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = x[e] > 0.f ? x[e] : 0.f;
    return r;
}

template <bool RES, bool TRAIN>
__global__ __launch_bounds__(CN_NT) void std_chain_fwd(const float *__restrict__ z, int64_t ldz, const float *__restrict__ bias,
                                                    float *__restrict__ rm1, float *__restrict__ rv1, float *__restrict__ rm2,
                                                    float *__restrict__ rv2, float *c, int64_t ldc, float *a, int64_t lda,
                                                    float *__restrict__ stats, int S, int H, float eps, float mom) {
    extern __shared__ __attribute__((aligned(16))) char cn_dyn[];
    __shared__ f32x4 red[CN_NT / 16];
    f32x4 *strip = (f32x4 *)cn_dyn;             // [S][4] quads, RES only
    const int q = threadIdx.x & 3, rs = threadIdx.x >> 2;
    const int col = blockIdx.x * CN_COLS + q * 4;
    const bool active = col < H;                // H % 4 == 0: a quad is inside or outside as a whole
    const f32x4 b = active ? *(const f32x4 *)(bias + col) : zero4();
    if (!TRAIN) {                               // running statistics in place of the batch's: one pass, nothing reduced
        if (!active) return;
        const f32x4 m1 = *(const f32x4 *)(rm1 + col), d1 = *(const f32x4 *)(rv1 + col) + eps;
        const f32x4 m2 = *(const f32x4 *)(rm2 + col), d2 = *(const f32x4 *)(rv2 + col) + eps;
        for (int r = rs; r < S; r += CN_SLOTS) {
            const f32x4 u = *(const f32x4 *)(z + (int64_t)r * ldz + col) + b;
            const f32x4 av = relu4((u - m1) / d1);
            if (a) *(f32x4 *)(a + (int64_t)r * lda + col) = av;
            *(f32x4 *)(c + (int64_t)r * ldc + col) = (av - m2) / d2;
        }
        return;
    }
    const float inv_s = 1.f / (float)S, inv_s1 = 1.f / (float)(S - 1);
    auto load_u = [&](int r) { return active ? *(const f32x4 *)(z + (int64_t)r * ldz + col) + b : zero4(); };
    f32x4 s = zero4();
    for (int r = rs; r < S; r += CN_SLOTS) {
        const f32x4 u = load_u(r);
        if (RES) strip[r * 4 + q] = u;
        s += u;
    }
    const f32x4 m1 = strip_sum<CN_NT / 64>(s, red) * inv_s;
    s = zero4();
    for (int r = rs; r < S; r += CN_SLOTS) {
        const f32x4 dl = (RES ? strip[r * 4 + q] : load_u(r)) - m1;
        s += dl * dl;
    }
    const f32x4 v1 = strip_sum<CN_NT / 64>(s, red) * inv_s1, d1 = v1 + eps;
    s = zero4();
    for (int r = rs; r < S; r += CN_SLOTS) {
        const f32x4 u = RES ? strip[r * 4 + q] : load_u(r);
        const f32x4 av = relu4((u - m1) / d1);
        if (active) *(f32x4 *)(a + (int64_t)r * lda + col) = av;
        if (RES) strip[r * 4 + q] = av;
        s += av;
    }
    const f32x4 m2 = strip_sum<CN_NT / 64>(s, red) * inv_s;
    auto load_a = [&](int r) { return RES ? strip[r * 4 + q] : (active ? *(const f32x4 *)(a + (int64_t)r * lda + col) : zero4()); };
    s = zero4();
    for (int r = rs; r < S; r += CN_SLOTS) {
        const f32x4 dl = load_a(r) - m2;
        s += dl * dl;
    }
    const f32x4 v2 = strip_sum<CN_NT / 64>(s, red) * inv_s1, d2 = v2 + eps;
    if (!active) return;
    for (int r = rs; r < S; r += CN_SLOTS) *(f32x4 *)(c + (int64_t)r * ldc + col) = (load_a(r) - m2) / d2;
    if (rs == 0) {
        *(f32x4 *)(stats + col) = m1;
        *(f32x4 *)(stats + (int64_t)H + col) = v1;
        *(f32x4 *)(stats + 2 * (int64_t)H + col) = m2;
        *(f32x4 *)(stats + 3 * (int64_t)H + col) = v2;
        const float keep = 1.f - mom;
        *(f32x4 *)(rm1 + col) = *(const f32x4 *)(rm1 + col) * keep + m1 * mom;
        *(f32x4 *)(rv1 + col) = *(const f32x4 *)(rv1 + col) * keep + v1 * mom;
        *(f32x4 *)(rm2 + col) = *(const f32x4 *)(rm2 + col) * keep + m2 * mom;
        *(f32x4 *)(rv2 + col) = *(const f32x4 *)(rv2 + col) * keep + v2 * mom;
    }
}

// One standardisation y = xt / d, xt = x - m, d = v + eps, v = sum xt^2 / (S - 1):
//     dx_j = (g_j - mean(g)) / d - 2 xt_j (sum_i g_i xt_i) / ((S - 1) d^2)
// Layer 5 (x = a), the mask a > 0, layer 3 (x = z + b).  The resident strip holds a, then the masked gradient gt.
template <bool RES>
__global__ __launch_bounds__(CB_NT) void std_chain_bwd(const float *__restrict__ dc, int64_t lddc, const float *__restrict__ a, int64_t lda,
                                                    const float *__restrict__ z, int64_t ldz, const float *__restrict__ bias,
                                                    const float *__restrict__ stats, float *dz, int64_t lddz,
                                                    float *__restrict__ dbias, int S, int H, float eps) {
    extern __shared__ __attribute__((aligned(16))) char cn_dyn[];
    __shared__ f32x4 red[CB_NT / 16];
    f32x4 *strip = (f32x4 *)cn_dyn;
    const int q = threadIdx.x & 3, rs = threadIdx.x >> 2;
    const int col = blockIdx.x * CN_COLS + q * 4;
    const bool active = col < H;
    const f32x4 one = (f32x4){1.f, 1.f, 1.f, 1.f};
    f32x4 b = zero4(), m1 = zero4(), d1 = one, m2 = zero4(), d2 = one;
    if (active) {
        b = *(const f32x4 *)(bias + col);
        m1 = *(const f32x4 *)(stats + col);
        d1 = *(const f32x4 *)(stats + (int64_t)H + col) + eps;
        m2 = *(const f32x4 *)(stats + 2 * (int64_t)H + col);
        d2 = *(const f32x4 *)(stats + 3 * (int64_t)H + col) + eps;
    }
    const float inv_s = 1.f / (float)S, two_s1 = 2.f / (float)(S - 1);
    auto load = [&](const float *p, int64_t ld, int r) { return active ? *(const f32x4 *)(p + (int64_t)r * ld + col) : zero4(); };
    f32x4 sg = zero4(), sgx = zero4();
    for (int r = rs; r < S; r += CB_NT / 4) {
        const f32x4 g = load(dc, lddc, r), av = load(a, lda, r);
        if (RES) strip[r * 4 + q] = av;
        sg += g;
        sgx += g * (av - m2);
    }
    const f32x4 gm2 = strip_sum<CB_NT / 64>(sg, red) * inv_s;
    const f32x4 k2 = strip_sum<CB_NT / 64>(sgx, red) * two_s1 / (d2 * d2);
    sg = zero4(); sgx = zero4();
    for (int r = rs; r < S; r += CB_NT / 4) {
        const f32x4 g = load(dc, lddc, r), av = RES ? strip[r * 4 + q] : load(a, lda, r);
        const f32x4 da = (g - gm2) / d2 - (av - m2) * k2;
        f32x4 gt;
#pragma unroll
        for (int e = 0; e < 4; ++e) gt[e] = av[e] > 0.f ? da[e] : 0.f;
        if (RES) strip[r * 4 + q] = gt;
        else if (active) *(f32x4 *)(dz + (int64_t)r * lddz + col) = gt;
        sg += gt;
        sgx += gt * ((load(z, ldz, r) + b) - m1);
    }
    const f32x4 gm1 = strip_sum<CB_NT / 64>(sg, red) * inv_s;
    const f32x4 k1 = strip_sum<CB_NT / 64>(sgx, red) * two_s1 / (d1 * d1);
    sg = zero4();
    for (int r = rs; r < S; r += CB_NT / 4) {
        const f32x4 gt = RES ? strip[r * 4 + q] : load(dz, lddz, r);
        const f32x4 du = (gt - gm1) / d1 - ((load(z, ldz, r) + b) - m1) * k1;
        if (active) *(f32x4 *)(dz + (int64_t)r * lddz + col) = du;
        sg += du;
    }
    const f32x4 db = strip_sum<CB_NT / 64>(sg, red);
    if (active && rs == 0) *(f32x4 *)(dbias + col) = db;
}

__global__ __launch_bounds__(NT) void bias_relu_f32(const float *x, int64_t ldx, const float *__restrict__ bias, float *y, int64_t ldy,
                                                    int rows, int C) {
    const int64_t per_row = C / 4, quads = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < quads; i += (int64_t)gridDim.x * NT) {
        const int64_t r = i / per_row;
        const int c = (int)(i - r * per_row) * 4;
        *(f32x4 *)(y + r * ldy + c) = relu4(*(const f32x4 *)(x + r * ldx + c) + *(const f32x4 *)(bias + c));
    }
}

// workgroup (strip, chunk): rows [256 chunk, 256 chunk + 256) of 16 columns; partial[chunk][C] = their column sums
__global__ __launch_bounds__(NT) void relu_bwd_colsum_f32(const float *dy, int64_t lddy, const float *__restrict__ y, int64_t ldy, float *dx,
                                                          int64_t lddx, float *__restrict__ partial, int rows, int C) {
    __shared__ f32x4 red[16];
    const int q = threadIdx.x & 3, rs = threadIdx.x >> 2;
    const int col = blockIdx.x * CN_COLS + q * 4;
    const bool active = col < C;
    const int r0 = blockIdx.y * RB_ROWS, r1 = min(rows, r0 + RB_ROWS);
    f32x4 s = zero4();
    if (active) {
        for (int r = r0 + rs; r < r1; r += NT / 4) {
            const f32x4 g = *(const f32x4 *)(dy + (int64_t)r * lddy + col), yy = *(const f32x4 *)(y + (int64_t)r * ldy + col);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = yy[e] > 0.f ? g[e] : 0.f;
            *(f32x4 *)(dx + (int64_t)r * lddx + col) = o;
            s += o;
        }
    }
    s = strip_sum<NT / 64>(s, red);
    if (active && rs == 0) *(f32x4 *)(partial + (int64_t)blockIdx.y * C + col) = s;
}

// db[c] = the partials of column c in chunk order
__global__ __launch_bounds__(NT) void colsum_finish_f32(const float *__restrict__ partial, int chunks, int C, float *__restrict__ db) {
    const int c = (blockIdx.x * NT + threadIdx.x) * 4;
    if (c >= C) return;
    f32x4 s = *(const f32x4 *)(partial + c);
    for (int k = 1; k < chunks; ++k) s += *(const f32x4 *)(partial + (int64_t)k * C + c);
    *(f32x4 *)(db + c) = s;
}

// LDS of a launch: the resident strip, or nothing beyond CN_RES_ROWS; the grant beyond 64 KB is asked for once per kernel
template <typename K>
int cn_lds(K kernel, bool &granted, int S, size_t &bytes, const char *name) {
    bytes = S <= CN_RES_ROWS ? (size_t)S * CN_COLS * sizeof(float) : 0;
    if (bytes > 65536 && !granted) {
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CN_RES_ROWS * CN_COLS * (int)sizeof(float));
        if (e != hipSuccess) return hgr_set_error(HGR_ELAUNCH, "%s: cannot reserve %d B of LDS: %s", name, CN_RES_ROWS * CN_COLS * 4, hipGetErrorString(e));
        granted = true;
    }
    return HGR_OK;
}

}  // namespace

extern "C" int hgr_cnzsl_std_chain_fwd(const float *z, int64_t ld_z, const float *bias, float *running_mean1, float *running_var1,
                                       float *running_mean2, float *running_var2, float *c, int64_t ld_c, float *a, int64_t ld_a,
                                       float *stats, int S, int H, int train, float eps, float momentum, void *stream) {
    HGR_REQUIRE(z && bias && running_mean1 && running_var1 && running_mean2 && running_var2 && c, "hgr_cnzsl_std_chain_fwd: null operand");
    HGR_REQUIRE(H >= 4 && H % 4 == 0, "hgr_cnzsl_std_chain_fwd: H=%d must be a multiple of 4", H);
    HGR_REQUIRE(train ? S >= 2 : S >= 1, "hgr_cnzsl_std_chain_fwd: S=%d (training needs two classes for the unbiased variance, evaluation one)", S);
    HGR_REQUIRE(!train || (a && stats), "hgr_cnzsl_std_chain_fwd: training writes a and stats");
    HGR_REQUIRE(rows_f32_ok(z, ld_z, H) && rows_f32_ok(c, ld_c, H) && (!a || rows_f32_ok(a, ld_a, H)),
                "hgr_cnzsl_std_chain_fwd: z / c / a must be 16-byte aligned, leading dimensions multiples of 4 and >= H");
    HGR_REQUIRE(hgr_aligned(bias, 16) && hgr_aligned(running_mean1, 16) && hgr_aligned(running_var1, 16) && hgr_aligned(running_mean2, 16) &&
                hgr_aligned(running_var2, 16) && hgr_aligned(stats, 16), "hgr_cnzsl_std_chain_fwd: vectors must be 16-byte aligned");
    const dim3 grid((H + CN_COLS - 1) / CN_COLS), block(CN_NT);
    hipStream_t s = (hipStream_t)stream;
    if (!train) {
        hipLaunchKernelGGL((std_chain_fwd<false, false>), grid, block, 0, s, z, ld_z, bias, running_mean1, running_var1, running_mean2,
                           running_var2, c, ld_c, a, ld_a, stats, S, H, eps, momentum);
    } else if (S <= CN_RES_ROWS) {
        static bool granted = false;
        size_t bytes;
        if (int rc = cn_lds(std_chain_fwd<true, true>, granted, S, bytes, "hgr_cnzsl_std_chain_fwd")) return rc;
        hipLaunchKernelGGL((std_chain_fwd<true, true>), grid, block, bytes, s, z, ld_z, bias, running_mean1, running_var1, running_mean2,
                           running_var2, c, ld_c, a, ld_a, stats, S, H, eps, momentum);
    } else {
        hipLaunchKernelGGL((std_chain_fwd<false, true>), grid, block, 0, s, z, ld_z, bias, running_mean1, running_var1, running_mean2,
                           running_var2, c, ld_c, a, ld_a, stats, S, H, eps, momentum);
    }
    HGR_CHECK_LAUNCH("hgr_cnzsl_std_chain_fwd");
    return HGR_OK;
}

extern "C" int hgr_cnzsl_std_chain_bwd(const float *dc, int64_t ld_dc, const float *a, int64_t ld_a, const float *z, int64_t ld_z,
                                       const float *bias, const float *stats, float *dz, int64_t ld_dz, float *dbias, int S, int H,
                                       float eps, void *stream) {
    HGR_REQUIRE(dc && a && z && bias && stats && dz && dbias, "hgr_cnzsl_std_chain_bwd: null operand");
    HGR_REQUIRE(H >= 4 && H % 4 == 0 && S >= 2, "hgr_cnzsl_std_chain_bwd: S=%d H=%d (S >= 2, H a multiple of 4)", S, H);
    HGR_REQUIRE(rows_f32_ok(dc, ld_dc, H) && rows_f32_ok(a, ld_a, H) && rows_f32_ok(z, ld_z, H) && rows_f32_ok(dz, ld_dz, H),
                "hgr_cnzsl_std_chain_bwd: dc / a / z / dz must be 16-byte aligned, leading dimensions multiples of 4 and >= H");
    HGR_REQUIRE(hgr_aligned(bias, 16) && hgr_aligned(stats, 16) && hgr_aligned(dbias, 16), "hgr_cnzsl_std_chain_bwd: vectors must be 16-byte aligned");
    HGR_REQUIRE(dz != dc && dz != a && dz != z, "hgr_cnzsl_std_chain_bwd: dz must not alias an input");
    const dim3 grid((H + CN_COLS - 1) / CN_COLS), block(CB_NT);
    hipStream_t s = (hipStream_t)stream;
    if (S <= CN_RES_ROWS) {
        static bool granted = false;
        size_t bytes;
        if (int rc = cn_lds(std_chain_bwd<true>, granted, S, bytes, "hgr_cnzsl_std_chain_bwd")) return rc;
        hipLaunchKernelGGL((std_chain_bwd<true>), grid, block, bytes, s, dc, ld_dc, a, ld_a, z, ld_z, bias, stats, dz, ld_dz, dbias, S, H, eps);
    } else {
        hipLaunchKernelGGL((std_chain_bwd<false>), grid, block, 0, s, dc, ld_dc, a, ld_a, z, ld_z, bias, stats, dz, ld_dz, dbias, S, H, eps);
    }
    HGR_CHECK_LAUNCH("hgr_cnzsl_std_chain_bwd");
    return HGR_OK;
}

extern "C" int hgr_bias_relu_f32(const float *x, int64_t ld_x, const float *bias, float *y, int64_t ld_y, int rows, int C, void *stream) {
    HGR_REQUIRE(x && bias && y && rows >= 1 && C >= 4 && C % 4 == 0, "hgr_bias_relu_f32: bad arguments (C=%d must be a multiple of 4)", C);
    HGR_REQUIRE(rows_f32_ok(x, ld_x, C) && rows_f32_ok(y, ld_y, C) && hgr_aligned(bias, 16),
                "hgr_bias_relu_f32: x / y / bias must be 16-byte aligned, leading dimensions multiples of 4 and >= C");
    int64_t blocks = ((int64_t)rows * (C / 4) + NT - 1) / NT;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bias_relu_f32, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, ld_x, bias, y, ld_y, rows, C);
    HGR_CHECK_LAUNCH("hgr_bias_relu_f32");
    return HGR_OK;
}

extern "C" int hgr_relu_bwd_colsum_f32(const float *dy, int64_t ld_dy, const float *y, int64_t ld_y, float *dx, int64_t ld_dx, float *db,
                                       float *scratch, int rows, int C, void *stream) {
    HGR_REQUIRE(dy && y && dx && db && rows >= 1 && C >= 4 && C % 4 == 0, "hgr_relu_bwd_colsum_f32: bad arguments (C=%d must be a multiple of 4)", C);
    HGR_REQUIRE(rows_f32_ok(dy, ld_dy, C) && rows_f32_ok(y, ld_y, C) && rows_f32_ok(dx, ld_dx, C) && hgr_aligned(db, 16) && hgr_aligned(scratch, 16),
                "hgr_relu_bwd_colsum_f32: operands must be 16-byte aligned, leading dimensions multiples of 4 and >= C");
    const int chunks = (rows + RB_ROWS - 1) / RB_ROWS;
    HGR_REQUIRE(chunks <= 65535, "hgr_relu_bwd_colsum_f32: rows=%d beyond %d", rows, 65535 * RB_ROWS);
    HGR_REQUIRE(chunks == 1 || scratch, "hgr_relu_bwd_colsum_f32: more than %d rows need scratch [ceil(rows / %d), C]", RB_ROWS, RB_ROWS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(relu_bwd_colsum_f32, dim3((C + CN_COLS - 1) / CN_COLS, chunks), dim3(NT), 0, s, dy, ld_dy, y, ld_y, dx, ld_dx,
                       chunks == 1 ? db : scratch, rows, C);
    if (chunks > 1) hipLaunchKernelGGL(colsum_finish_f32, dim3((C / 4 + NT - 1) / NT), dim3(NT), 0, s, scratch, chunks, C, db);
    HGR_CHECK_LAUNCH("hgr_relu_bwd_colsum_f32");
    return HGR_OK;
}
