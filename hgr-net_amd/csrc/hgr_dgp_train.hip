// DGP baseline training (baseline/DGP/train_gcn_dense_att.py:96-102): what the backward pass of GCN_Dense_Att needs beside
// the forward gather of hgr_dgp.hip and the fp32 products.  Per layer and side, with a = softmax(att), S = Xd W and
// O[i] = sum_e a[grp_e] inv_e (S[col_e] + b):
//
//     hgr_csr_group_att_grad   dO[i] = G[i] * (Y[i] > 0 ? 1 : slope) (or dO given), and the attention gradient's rows
//                              P[i, d] = dO[i] . sum_{e in (i, d)} inv_e (S[col_e] + b);     da = colsum(P)
//     hgr_dgp_loss_head        the masked L2 loss of utils.l2_loss on F.normalize(O) and its gradient with respect to O
//     hgr_dropout_counter      y = x * keep * 2, keep a pure function of (seed, step, layer, element index)
//     hgr_adam_l2              torch.optim.Adam with coupled weight decay
//
// The adjoint gather T[j] = sum_{e: col_e = j} a[grp_e] inv_e dO[row_e] is hgr_csr_group_aggregate on the transposed CSR.
// Same structure as the forward gather: a workgroup owns one work item (at most CHUNK edges of one row), its 256 threads
// own float4 column slices, edge data is block-uniform, rows cut into several items leave fp32 partials that a finish
// kernel adds in item order.  No atomics: a launch repeated on the same inputs gives bit-equal output.
#include "hgr_rows.h"

namespace {

constexpr int NT = 256;

// dO slices of one row: G * (Y > 0 ? 1 : slope), or G itself without Y (the last layer, whose dO the loss head made)
template <int NV>
__device__ __forceinline__ void load_dout(f32x4 (&d)[NV], const float *__restrict__ g, const float *__restrict__ y, int C, float slope) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (v * NT + threadIdx.x) * 4;
        d[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            d[v] = *(const f32x4 *)(g + c);
            if (y) {
                const f32x4 yy = *(const f32x4 *)(y + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[v][e] *= yy[e] > 0.f ? 1.f : slope;
            }
        }
    }
}

template <int NV>
__global__ __launch_bounds__(NT) void csr_att_grad(const float *__restrict__ support, int64_t lds_, const float *__restrict__ bias,
                                                   const float *g, int64_t ldg, const float *__restrict__ y, int64_t ldy,
                                                   float *dout, int64_t ldd, const int *__restrict__ item_row,
                                                   const int *__restrict__ item_e0, const int *__restrict__ item_e1,
                                                   const int *__restrict__ item_slot, const int *__restrict__ col,
                                                   const float *__restrict__ inv_deg, const unsigned char *__restrict__ grp, int D,
                                                   float *__restrict__ P, float *__restrict__ partial, int C, float slope) {
    __shared__ float s_p[32];
    __shared__ float red[4];
    if (threadIdx.x < 32) s_p[threadIdx.x] = 0.f;          // groups without an edge in this item contribute 0
    const int it = blockIdx.x;
    const int row = item_row[it], e0 = item_e0[it], e1 = item_e1[it], slot = item_slot[it];
    f32x4 d[NV], acc[NV];
    load_dout<NV>(d, g + (int64_t)row * ldg, y ? y + (int64_t)row * ldy : nullptr, C, slope);
    if (slot < 0 && dout) {                                // rows cut into several items get their dO from the finish kernel
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = (v * NT + threadIdx.x) * 4;
            if (c < C) *(f32x4 *)(dout + (int64_t)row * ldd + c) = d[v];
        }
    }
    float bd = 0.f;                                        // dO[i] . b, the bias part of every group's aggregate
    if (bias) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = (v * NT + threadIdx.x) * 4;
            if (c < C) {
                const f32x4 b = *(const f32x4 *)(bias + c);
                bd += (d[v][0] * b[0] + d[v][1] * b[1]) + (d[v][2] * b[2] + d[v][3] * b[3]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float isum = 0.f;
    int cur = e0 < e1 ? (int)grp[e0] : 0;
    // the group's aggregate is complete (or the item ends inside it): reduce dO . aggregate over the block
    auto flush = [&](int grp_id) {
        float s = bd * isum;
#pragma unroll
        for (int v = 0; v < NV; ++v) s += (d[v][0] * acc[v][0] + d[v][1] * acc[v][1]) + (d[v][2] * acc[v][2] + d[v][3] * acc[v][3]);
        s = block_sum(s, red);
        if (threadIdx.x == 0) s_p[grp_id & 31] = s;
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        isum = 0.f;
    };
    int e = e0;
    while (e < e1) {                                       // edge data is block-uniform: scalar loads, uniform branches
        const int gid = grp[e];
        if (gid != cur) { flush(cur); cur = gid; }
        if (e + 4 <= e1 && grp[e + 3] == gid) {            // edges are sorted by group inside a row: all four are of group gid
            const int j0 = col[e], j1 = col[e + 1], j2 = col[e + 2], j3 = col[e + 3];
            const float w0 = inv_deg[e], w1 = inv_deg[e + 1], w2 = inv_deg[e + 2], w3 = inv_deg[e + 3];
            isum += (w0 + w1) + (w2 + w3);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = (v * NT + threadIdx.x) * 4;
                if (c < C) {
                    const f32x4 s0 = *(const f32x4 *)(support + (int64_t)j0 * lds_ + c), s1 = *(const f32x4 *)(support + (int64_t)j1 * lds_ + c);
                    const f32x4 s2 = *(const f32x4 *)(support + (int64_t)j2 * lds_ + c), s3 = *(const f32x4 *)(support + (int64_t)j3 * lds_ + c);
                    acc[v] += (s0 * w0 + s1 * w1) + (s2 * w2 + s3 * w3);
                }
            }
            e += 4;
        } else {
            const int j = col[e];
            const float w = inv_deg[e];
            isum += w;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int c = (v * NT + threadIdx.x) * 4;
                if (c < C) acc[v] += *(const f32x4 *)(support + (int64_t)j * lds_ + c) * w;
            }
            e += 1;
        }
    }
    if (e0 < e1) flush(cur);
    __syncthreads();
    float *dst = slot < 0 ? P + (int64_t)row * D : partial + (int64_t)slot * D;
    if (threadIdx.x < D) dst[threadIdx.x] = s_p[threadIdx.x];
}

// rows cut into several items: P[row] = sum of its [D] partials in item order, and the row's dO
template <int NV>
__global__ __launch_bounds__(NT) void csr_att_grad_finish(const int *__restrict__ split_row, const int *__restrict__ split_slot0,
                                                          const int *__restrict__ split_n, const float *__restrict__ partial,
                                                          float *__restrict__ P, int D, const float *g, int64_t ldg,
                                                          const float *__restrict__ y, int64_t ldy, float *dout, int64_t ldd, int C, float slope) {
    const int row = split_row[blockIdx.x], s0 = split_slot0[blockIdx.x], ns = split_n[blockIdx.x];
    if (threadIdx.x < D) {
        float s = 0.f;
        for (int k = 0; k < ns; ++k) s += partial[(int64_t)(s0 + k) * D + threadIdx.x];
        P[(int64_t)row * D + threadIdx.x] = s;
    }
    if (dout) {
        f32x4 d[NV];
        load_dout<NV>(d, g + (int64_t)row * ldg, y ? y + (int64_t)row * ldy : nullptr, C, slope);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = (v * NT + threadIdx.x) * 4;
            if (c < C) *(f32x4 *)(dout + (int64_t)row * ldd + c) = d[v];
        }
    }
}

// one selected row: y = o / max(|o|, 1e-12); loss term |y - f|^2 / (2 n_t); dO = (gy - y (y . gy)) / max(|o|, 1e-12), gy = (y - f) / n_t
template <int NV>
__global__ __launch_bounds__(NT) void loss_head(const float *__restrict__ O, int64_t ldo, const int *__restrict__ rows,
                                                const float *__restrict__ F, int64_t ldf, int n_t, float *__restrict__ loss_rows,
                                                float *__restrict__ dout, int64_t ldd, int C) {
    __shared__ float red[4];
    const int k = blockIdx.x, row = rows[k];
    const float *o = O + (int64_t)row * ldo, *f = F + (int64_t)k * ldf;
    f32x4 yv[NV], gv[NV];
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (v * NT + threadIdx.x) * 4;
        yv[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < C) yv[v] = *(const f32x4 *)(o + c);
        ss += (yv[v][0] * yv[v][0] + yv[v][1] * yv[v][1]) + (yv[v][2] * yv[v][2] + yv[v][3] * yv[v][3]);
    }
    const float scale = 1.f / fmaxf(sqrtf(block_sum(ss, red)), 1e-12f);
    const float inv_nt = 1.f / (float)n_t;
    float l = 0.f, yg = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (v * NT + threadIdx.x) * 4;
        gv[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            const f32x4 ff = *(const f32x4 *)(f + c);
            yv[v] = yv[v] * scale;
            const f32x4 df = yv[v] - ff;
            l += (df[0] * df[0] + df[1] * df[1]) + (df[2] * df[2] + df[3] * df[3]);
            gv[v] = df * inv_nt;
            yg += (yv[v][0] * gv[v][0] + yv[v][1] * gv[v][1]) + (yv[v][2] * gv[v][2] + yv[v][3] * gv[v][3]);
        }
    }
    l = block_sum(l, red);
    yg = block_sum(yg, red);
    if (threadIdx.x == 0) loss_rows[k] = l * (0.5f * inv_nt);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (v * NT + threadIdx.x) * 4;
        if (c < C) *(f32x4 *)(dout + (int64_t)row * ldd + c) = (gv[v] - yv[v] * yg) * scale;
    }
}

// loss = sum of the per-row terms in a fixed order (thread t takes rows t, t + 256, ...; then the block tree)
__global__ __launch_bounds__(NT) void loss_sum(const float *__restrict__ loss_rows, int n_t, float *__restrict__ loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < n_t; k += NT) s += loss_rows[k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *loss = s;
}

__global__ __launch_bounds__(NT) void dropout_counter(const float *x, int64_t ldx, float *y, int64_t ldy, int rows, int C, unsigned key) {
    const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x, per_row = C / 4;
    if (q >= (int64_t)rows * per_row) return;
    const int64_t r = q / per_row;
    const int c = (int)(q - r * per_row) * 4;
    const f32x4 xv = *(const f32x4 *)(x + r * ldx + c);
    const unsigned idx = (unsigned)((uint64_t)r * (uint64_t)C + (uint64_t)c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (fmix32((idx + (unsigned)e) ^ key) >> 31) ? xv[e] * 2.f : 0.f;
    *(f32x4 *)(y + r * ldy + c) = o;
}

__global__ __launch_bounds__(NT) void adam_l2(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                              int64_t n, float beta1, float beta2, float eps, float wd, float step_size, float inv_sqrt_bc2) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        float pi = p[i];
        adam_l2_update(pi, g[i], m[i], v[i], beta1, beta2, eps, wd, step_size, inv_sqrt_bc2);
        p[i] = pi;
    }
}

}  // namespace

extern "C" int hgr_csr_group_att_grad(const float *support, int64_t ld_support, const float *bias, const float *g, int64_t ld_g,
                                      const float *y, int64_t ld_y, float *dout, int64_t ld_dout, const int *item_row,
                                      const int *item_e0, const int *item_e1, const int *item_slot, int n_items, const int *col,
                                      const float *inv_deg, const unsigned char *grp, int D, const int *split_row,
                                      const int *split_slot0, const int *split_n, int n_split, float *partial, float *P, int C,
                                      float slope, void *stream) {
    HGR_REQUIRE(support && g && item_row && item_e0 && item_e1 && item_slot && col && inv_deg && grp && P, "hgr_csr_group_att_grad: null operand");
    HGR_REQUIRE(n_items >= 1 && D >= 1 && D <= 32, "hgr_csr_group_att_grad: bad sizes n_items=%d D=%d (D <= 32)", n_items, D);
    HGR_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4 * NT * 4, "hgr_csr_group_att_grad: C=%d must be a multiple of 4, at most %d", C, 4 * NT * 4);
    HGR_REQUIRE(ld_support % 4 == 0 && ld_support >= C && ld_g % 4 == 0 && ld_g >= C && (!y || (ld_y % 4 == 0 && ld_y >= C)) &&
                (!dout || (ld_dout % 4 == 0 && ld_dout >= C)), "hgr_csr_group_att_grad: leading dimensions must be multiples of 4 and >= C");
    HGR_REQUIRE(hgr_aligned(support, 16) && hgr_aligned(g, 16) && hgr_aligned(y, 16) && hgr_aligned(dout, 16) && hgr_aligned(bias, 16),
                "hgr_csr_group_att_grad: support / bias / g / y / dout must be 16-byte aligned");
    HGR_REQUIRE(!y || dout, "hgr_csr_group_att_grad: the LeakyReLU mode (y given) writes dout");
    HGR_REQUIRE(n_split == 0 || (split_row && split_slot0 && split_n && partial), "hgr_csr_group_att_grad: split rows need their tables and the partial buffer");
    hipStream_t s = (hipStream_t)stream;
    const int nv = (C + 4 * NT - 1) / (4 * NT);
    hgr_by_nv4(nv, [&](auto NV) {
        hipLaunchKernelGGL(csr_att_grad<NV.value>, dim3(n_items), dim3(NT), 0, s, support, ld_support, bias, g, ld_g, y, ld_y, dout,
                           ld_dout, item_row, item_e0, item_e1, item_slot, col, inv_deg, grp, D, P, partial, C, slope);
        if (n_split > 0)
            hipLaunchKernelGGL(csr_att_grad_finish<NV.value>, dim3(n_split), dim3(NT), 0, s, split_row, split_slot0, split_n, partial, P,
                               D, g, ld_g, y, ld_y, dout, ld_dout, C, slope);
    });
    HGR_CHECK_LAUNCH("hgr_csr_group_att_grad");
    return HGR_OK;
}

extern "C" int hgr_dgp_loss_head(const float *O, int64_t ld_o, const int *rows, const float *F, int64_t ld_f, int n_t, int n,
                                 float *loss_rows, float *loss, float *dout, int64_t ld_dout, int C, void *stream) {
    HGR_REQUIRE(O && rows && F && loss_rows && loss && dout, "hgr_dgp_loss_head: null operand");
    HGR_REQUIRE(n_t >= 1 && n >= n_t, "hgr_dgp_loss_head: bad sizes n_t=%d n=%d (distinct rows: n_t <= n)", n_t, n);
    HGR_REQUIRE(C >= 4 && C % 4 == 0 && C <= 4 * NT * 4, "hgr_dgp_loss_head: C=%d must be a multiple of 4, at most %d", C, 4 * NT * 4);
    HGR_REQUIRE(ld_o % 4 == 0 && ld_f % 4 == 0 && ld_dout % 4 == 0 && ld_o >= C && ld_f >= C && ld_dout >= C,
                "hgr_dgp_loss_head: leading dimensions must be multiples of 4 and >= C");
    HGR_REQUIRE(hgr_aligned(O, 16) && hgr_aligned(F, 16) && hgr_aligned(dout, 16), "hgr_dgp_loss_head: O / F / dout must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemset2DAsync(dout, (size_t)ld_dout * sizeof(float), 0, (size_t)C * sizeof(float), (size_t)n, s) != hipSuccess)
        return hgr_set_error(HGR_ELAUNCH, "hgr_dgp_loss_head: clearing dout failed");
    const int nv = (C + 4 * NT - 1) / (4 * NT);
    hgr_by_nv4(nv, [&](auto NV) { hipLaunchKernelGGL(loss_head<NV.value>, dim3(n_t), dim3(NT), 0, s, O, ld_o, rows, F, ld_f, n_t, loss_rows, dout, ld_dout, C); });
    hipLaunchKernelGGL(loss_sum, dim3(1), dim3(NT), 0, s, loss_rows, n_t, loss);
    HGR_CHECK_LAUNCH("hgr_dgp_loss_head");
    return HGR_OK;
}

extern "C" int hgr_dropout_counter(const float *x, int64_t ld_x, float *y, int64_t ld_y, int rows, int C, int seed, int step, int layer,
                                   void *stream) {
    HGR_REQUIRE(x && y && rows >= 1 && C >= 4 && C % 4 == 0, "hgr_dropout_counter: bad arguments (C=%d must be a multiple of 4)", C);
    HGR_REQUIRE(ld_x % 4 == 0 && ld_y % 4 == 0 && ld_x >= C && ld_y >= C && hgr_aligned(x, 16) && hgr_aligned(y, 16),
                "hgr_dropout_counter: leading dimensions must be multiples of 4 and >= C, x / y 16-byte aligned");
    HGR_REQUIRE((int64_t)rows * C <= 0xFFFFFFFFll, "hgr_dropout_counter: rows * C must fit the 32-bit element index");
    // the key of (seed, step, layer), block-uniform: dgp.dropout_keep is the host twin of these two lines and of the kernel's mix
    unsigned key = fmix32((unsigned)seed + 0x9E3779B9u * ((unsigned)step + 1u));
    key = fmix32(key ^ ((unsigned)layer * 0x85EBCA6Bu + 0xC2B2AE35u));
    const int64_t quads = (int64_t)rows * (C / 4);
    hipLaunchKernelGGL(dropout_counter, dim3((unsigned)((quads + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, x, ld_x, y, ld_y, rows, C, key);
    HGR_CHECK_LAUNCH("hgr_dropout_counter");
    return HGR_OK;
}

extern "C" int hgr_adam_l2(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1, float beta2, float eps, float wd,
                           int step, void *stream) {
    HGR_REQUIRE(p && g && m && v && n >= 1 && step >= 1, "hgr_adam_l2: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    int64_t blocks = (n + NT - 1) / NT;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adam_l2, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n, beta1, beta2, eps, wd,
                       (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)));
    HGR_CHECK_LAUNCH("hgr_adam_l2");
    return HGR_OK;
}
