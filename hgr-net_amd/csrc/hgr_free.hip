// FREE baseline, validation route (baseline/FREE/validate.py, classifier.py, model.py): what synthesising features, fitting the
// softmax classifier on cat(x, hidden, h) and scoring it need beside hgr_gemm_nt, hgr_gemm_tn_splitk, hgr_colsum, hgr_adam_l2 and
// hgr_dot_f32 -
//
//     hgr_normal_counter     z[r, c] ~ N(0, 1), a pure function of (seed, stream, row0 + r, c)            (test entry of normal_at)
//     hgr_free_gen_input     cat(z, attribute[classes[row / num]]) - the generator's input                  classifier.py:30-38
//     hgr_bias_act_rows      y = lrelu_0.2(x + b) or sigmoid(x + b), into a strided destination            model.py:59-60, :109
//     hgr_free_fr_tail       y = sigmoid(mu + eps sigmoid(sd)) from lantent = (mu, sd)                      model.py:110-121, :130
//     hgr_nll_rows16         NLLLoss(LogSoftmax): loss rows, 16-bit (softmax - onehot), fp32 log-softmax    classifier.py:81, :369
//     hgr_adam_l2_cast16     slice sum -> hgr_adam_l2's update -> the 16-bit operand, one pass              classifier.py:86, :121
//
// All of them are bound by memory: a lane moves 16 bytes per access, a 16-bit value is ONE rounding of the fp32 value, sums run in
// a fixed order (per thread ascending, a shuffle tree over the wave, the waves in order) and nothing is atomic - a launch
// repeated on the same input writes the same bits.
#include "hgr_rows.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int OUT_F32 = 2;                      // `out_type`: HGR_BF16, HGR_F16 or fp32
constexpr int NLL_RES = HGR_NLL_RESIDENT_COLS;  // a row of up to this many fp32 logits stays in LDS (72 KiB: two workgroups per CU)

// ---- the counter normal: free.normal_host is the float64 twin of these three functions ---------------------------------------------
unsigned normal_key(int seed, int stream) {
    const unsigned key = fmix32((unsigned)seed + 0x9E3779B9u * ((unsigned)stream + 1u));
    return fmix32(key ^ 0xC2B2AE35u);
}
__device__ __forceinline__ unsigned normal_row_key(unsigned key, int64_t row) {
    const unsigned k = fmix32(key ^ (unsigned)(uint64_t)row);
    return fmix32(k + 0x9E3779B9u * ((unsigned)((uint64_t)row >> 32) + 1u));
}
// Box-Muller on the two draws of column c: u1 = ((a >> 9) + 1/2) 2^-23 in (0, 1) and 2 u2 = (b >> 8) 2^-23 in [0, 2) are exact in
// fp32; logf / cospif are the library functions (the fast intrinsics are 2^-21 off near u1 = 1)
__device__ __forceinline__ float normal_at(unsigned rk, int c, unsigned &a, unsigned &b) {
    a = fmix32(rk ^ (2u * (unsigned)c));
    b = fmix32(rk ^ (2u * (unsigned)c + 1u));
    const float u1 = ((float)(a >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float t = (float)(b >> 8) * 1.1920928955078125e-07f;
    return sqrtf(-2.f * logf(u1)) * cospif(t);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// The fp32 value as the conversion sees it: handed over through an opaque register copy, so that the compiler cannot merge the
// arithmetic in front of it with the conversion (v_fma_mix*_f16 rounds an fp32 product or sum ONCE, straight to f16 - not the bits
// hgr_cast16 gives for the fp32 result)
__device__ __forceinline__ float rounded32(float x) {
    asm("" : "+v"(x));
    return x;
}

// 8 consecutive values to y: 16 bytes in the 16-bit types, two 16-byte stores in fp32
template <int OT> __device__ __forceinline__ void store8(void *y, int64_t at, const float (&o)[8]) {
    if (OT == OUT_F32) {
        f32x4 *p = (f32x4 *)((float *)y + at);
        p[0] = (f32x4){o[0], o[1], o[2], o[3]};
        p[1] = (f32x4){o[4], o[5], o[6], o[7]};
    } else {
        constexpr int DT = OT == OUT_F32 ? HGR_BF16 : OT;
        typedef typename T16<DT>::elem E;
        typename T16<DT>::vec8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (E)rounded32(o[e]);
        *(typename T16<DT>::vec8 *)((E *)y + at) = v;
    }
}
__device__ __forceinline__ void load8(const float *x, float (&o)[8]) {
    const f32x4 a = ((const f32x4 *)x)[0], b = ((const f32x4 *)x)[1];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
}

__global__ __launch_bounds__(NT) void normal_counter(float *z, int64_t ldz, unsigned *bits, int rows, int C, unsigned key, int64_t row0) {
    const int64_t per_row = C / 4, quads = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < quads; i += (int64_t)gridDim.x * NT) {
        const int64_t r = i / per_row;
        const int c = (int)(i - r * per_row) * 4;
        const unsigned rk = normal_row_key(key, row0 + r);
        f32x4 o;
        u32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned a, b;
            o[e] = normal_at(rk, c + e, a, b);
            if (e < 2) { lo[2 * e] = a; lo[2 * e + 1] = b; }
            else { hi[2 * e - 4] = a; hi[2 * e - 3] = b; }
        }
        *(f32x4 *)(z + r * ldz + c) = o;
        if (bits) {
            u32x4 *bp = (u32x4 *)(bits + (r * C + c) * 2);
            bp[0] = lo;
            bp[1] = hi;
        }
    }
}

// item = 8 columns of one row: columns [0, nz) the noise, [nz, nz + A) the class's attribute row
template <int OT>
__global__ __launch_bounds__(NT) void gen_input(void *out, int64_t ldo, const float *__restrict__ z, int64_t ldz, const float *__restrict__ att,
                                                int64_t lda, int att_rows, const int32_t *__restrict__ classes, int n_classes, int num, int rows,
                                                int nz, int A, unsigned key, int64_t row0) {
    const int64_t per_row = (nz + A) / 8, items = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < items; i += (int64_t)gridDim.x * NT) {
        const int64_t r = i / per_row, gr = row0 + r;
        const int c = (int)(i - r * per_row) * 8;
        float o[8];
        if (c < nz) {
            if (z) load8(z + r * ldz + c, o);
            else {
                const unsigned rk = normal_row_key(key, gr);
#pragma unroll
                for (int e = 0; e < 8; ++e) { unsigned a, b; o[e] = normal_at(rk, c + e, a, b); }
            }
        } else {
            const int64_t k = gr / num;
            const int cls = k < n_classes ? classes[k] : -1;
            if ((unsigned)cls < (unsigned)att_rows) load8(att + (int64_t)cls * lda + (c - nz), o);
            else {                                  // a class outside the table: NaN, never a read out of bounds
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = __builtin_nanf("");
            }
        }
        store8<OT>(out, r * ldo + c, o);
    }
}

template <int OT, int ACT>
__global__ __launch_bounds__(NT) void bias_act_rows(const float *__restrict__ x, int64_t ldx, const float *__restrict__ bias, void *y, int64_t ldy,
                                                    int rows, int C) {
    const int64_t per_row = C / 8, items = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < items; i += (int64_t)gridDim.x * NT) {
        const int64_t r = i / per_row;
        const int c = (int)(i - r * per_row) * 8;
        float v[8], b[8], o[8];
        load8(x + r * ldx + c, v);
        load8(bias + c, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float u = v[e] + b[e];
            o[e] = ACT == 0 ? (u > 0.f ? u : 0.2f * u) : sigmoidf(u);
        }
        store8<OT>(y, r * ldy + c, o);
    }
}

template <int OT>
__global__ __launch_bounds__(NT) void fr_tail(const float *__restrict__ lat, int64_t ldl, const float *__restrict__ bias, const float *__restrict__ eps,
                                              int64_t lde, void *y, int64_t ldy, float *__restrict__ mus, int64_t ldm, int rows, int A, unsigned key,
                                              int64_t row0) {
    const int64_t per_row = A / 8, items = (int64_t)rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < items; i += (int64_t)gridDim.x * NT) {
        const int64_t r = i / per_row;
        const int c = (int)(i - r * per_row) * 8;
        float mu[8], sd[8], n[8], o[8];
        load8(lat + r * ldl + c, mu);
        load8(lat + r * ldl + A + c, sd);
        if (bias) {
            float bm[8], bs[8];
            load8(bias + c, bm);
            load8(bias + A + c, bs);
#pragma unroll
            for (int e = 0; e < 8; ++e) { mu[e] += bm[e]; sd[e] += bs[e]; }
        }
        if (eps) load8(eps + r * lde + c, n);
        else {
            const unsigned rk = normal_row_key(key, row0 + r);
#pragma unroll
            for (int e = 0; e < 8; ++e) { unsigned a, b; n[e] = normal_at(rk, c + e, a, b); }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = sigmoidf(n[e] * sigmoidf(sd[e]) + mu[e]);
        store8<OT>(y, r * ldy + c, o);
        if (mus) {
            f32x4 *mp = (f32x4 *)(mus + r * ldm + c);
            mp[0] = (f32x4){mu[0], mu[1], mu[2], mu[3]};
            mp[1] = (f32x4){mu[4], mu[5], mu[6], mu[7]};
        }
    }
}

// ---- hgr_nll_rows16: one workgroup per row -------------------------------------------------------------------------------------------
// two running (max, sum of exp(x - max)) states into one; symmetric, so both lanes of an exchange hold the same bits
__device__ __forceinline__ void online_merge(float &m, float &s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * (m == mn ? 1.f : __expf(m - mn)) + s2 * (m2 == mn ? 1.f : __expf(m2 - mn));
    m = mn;
}

// RES: the row is read from memory ONCE into LDS (max on the way in, then the sum and the write pass from LDS).  Otherwise two passes
// over memory: a running (max, sum) pass, then the write pass - which may overwrite the logits with their log-softmax, a thread
// only ever re-reads in pass two what no other thread writes.
template <int DT, bool RES>
__global__ __launch_bounds__(NT) void nll_rows16(const float *logits, int64_t ld, const int32_t *__restrict__ labels, int n, float *__restrict__ loss_rows,
                                                 typename T16<DT>::elem *__restrict__ dlogits, int64_t ldd, int dcols, float *logsm, int64_t ldl) {
    extern __shared__ __attribute__((aligned(16))) char nll_dyn[];
    __shared__ float red[4];
    float *row = (float *)nll_dyn;                 // RES: [npad]
    const int r = blockIdx.x, t = threadIdx.x;
    const float *x = logits + (int64_t)r * ld;
    const int nq = (n + 3) / 4;                     // quads with at least one valid column (ld % 8 == 0: the whole quad is readable)
    const int lab = labels ? labels[r] : -1;
    // read before anything is written: the write pass may replace the logits by their log-softmax
    const float xlab = t == 0 && (unsigned)lab < (unsigned)n ? x[lab] : __builtin_nanf("");
    float mx, sum;
    if (RES) {
        float m = -INFINITY;
        for (int q = t; q < nq; q += NT) {
            const f32x4 v = ((const f32x4 *)x)[q];
            ((f32x4 *)row)[q] = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (4 * q + e < n) m = fmaxf(m, v[e]);
        }
        mx = block_max(m, red);                     // its barrier also publishes the row
        float s = 0.f;
        for (int q = t; q < nq; q += NT) {
            const f32x4 v = ((const f32x4 *)row)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) if (4 * q + e < n) s += __expf(v[e] - mx);
        }
        sum = block_sum(s, red);
    } else {
        float m = -INFINITY, s = 0.f;
        for (int q = t; q < nq; q += NT) {
            const f32x4 v = ((const f32x4 *)x)[q];
            float cm = -INFINITY;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (4 * q + e < n) cm = fmaxf(cm, v[e]);
            const float mn = fmaxf(m, cm);
            float cs = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (4 * q + e < n) cs += __expf(v[e] - mn);
            s = s * (m == mn ? 1.f : __expf(m - mn)) + cs;
            m = mn;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) online_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
        __shared__ float redm[4], reds[4];
        if ((t & 63) == 0) { redm[t >> 6] = m; reds[t >> 6] = s; }
        __syncthreads();
        m = redm[0]; s = reds[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) online_merge(m, s, redm[w], reds[w]);
        mx = m; sum = s;
    }
    const float lse = mx + __logf(sum);
    const float *src = RES ? row : x;
    if (loss_rows && t == 0) loss_rows[r] = lse - xlab;      // NaN for a label outside [0, n)
    const int chunks = dlogits ? dcols / 8 : (n + 7) / 8;
    float *lo = logsm ? logsm + (int64_t)r * ldl : nullptr;
    for (int c8 = t; c8 < chunks; c8 += NT) {
        const int c = c8 * 8;
        float v[8], d[8];
        if (c < n) load8(src + c, v);               // c < n: the chunk lies inside [0, round_up(n, 8)), which is inside the row
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = c + e < n ? __expf(v[e] - lse) - (c + e == lab ? 1.f : 0.f) : 0.f;
        if (dlogits) store8<DT>(dlogits, (int64_t)r * ldd + c, d);
        if (lo && c < n) {
            if (c + 8 <= n) {
                ((f32x4 *)(lo + c))[0] = (f32x4){v[0] - lse, v[1] - lse, v[2] - lse, v[3] - lse};
                ((f32x4 *)(lo + c))[1] = (f32x4){v[4] - lse, v[5] - lse, v[6] - lse, v[7] - lse};
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) if (c + e < n) lo[c + e] = v[e] - lse;
            }
        }
    }
}

// g' = alpha (g[0] + g[1] + ...), then hgr_adam_l2's update (adam_l2_update) on it (the product is handed over through an opaque register copy, so
// that it is rounded before the decay term meets it, as a gradient read from memory is), then the 16-bit copy of the new parameter
template <int DT>
__global__ __launch_bounds__(NT) void adam_l2_cast16(float *__restrict__ p, const float *__restrict__ g, int64_t slice_stride, int S, float alpha,
                                                     float *__restrict__ m, float *__restrict__ v, typename T16<DT>::elem *__restrict__ w16, int64_t n4,
                                                     float beta1, float beta2, float eps, float wd, float step_size, float inv_sqrt_bc2) {
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        f32x4 gs = ((const f32x4 *)g)[i];
        for (int s = 1; s < S; ++s) gs += ((const f32x4 *)(g + (int64_t)s * slice_stride))[i];
        f32x4 pv = ((const f32x4 *)p)[i], mv = ((const f32x4 *)m)[i], vv = ((const f32x4 *)v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float ga = alpha * gs[e];
            asm volatile("" : "+v"(ga));
            float pe = pv[e], me = mv[e], ve = vv[e];         // a vector element does not bind to a float &
            adam_l2_update(pe, ga, me, ve, beta1, beta2, eps, wd, step_size, inv_sqrt_bc2);
            pv[e] = pe;
            mv[e] = me;
            vv[e] = ve;
        }
        ((f32x4 *)m)[i] = mv;
        ((f32x4 *)v)[i] = vv;
        ((f32x4 *)p)[i] = pv;
        ((typename T16<DT>::vec4 *)w16)[i] = cvt4<DT>(rounded32(pv[0]), rounded32(pv[1]), rounded32(pv[2]), rounded32(pv[3]));
    }
}

bool out_ok(const void *y, int64_t ld, int C) {
    return y && ld % 8 == 0 && ld >= C && hgr_aligned(y, 16);
}

#define HGR_OT_OK(name) HGR_REQUIRE(out_type == HGR_BF16 || out_type == HGR_F16 || out_type == OUT_F32, name ": out_type must be HGR_BF16, HGR_F16 or 2 (fp32)")

}  // namespace

extern "C" int hgr_normal_counter(float *z, int64_t ld_z, uint32_t *bits, int rows, int C, int seed, int stream_id, int64_t row0, void *stream) {
    HGR_REQUIRE(z && rows >= 1 && C >= 4 && C % 4 == 0 && row0 >= 0, "hgr_normal_counter: bad arguments (C=%d must be a multiple of 4, row0 >= 0)", C);
    HGR_REQUIRE(rows_f32_ok(z, ld_z, C) && hgr_aligned(bits, 16), "hgr_normal_counter: z / bits must be 16-byte aligned, ld_z a multiple of 4 and >= C");
    hipLaunchKernelGGL(normal_counter, dim3(hgr_grid1((int64_t)rows * (C / 4), hgr_cu_count() * 16, NT)), dim3(NT), 0, (hipStream_t)stream, z, ld_z, (unsigned *)bits, rows, C,
                       normal_key(seed, stream_id), row0);
    HGR_CHECK_LAUNCH("hgr_normal_counter");
    return HGR_OK;
}

extern "C" int hgr_free_gen_input(void *out, int64_t ld_out, int out_type, const float *z, int64_t ld_z, const float *att, int64_t ld_att,
                                  int att_rows, const int32_t *classes, int n_classes, int num, int rows, int nz, int A, int seed,
                                  int stream_id, int64_t row0, void *stream) {
    HGR_REQUIRE(out && att && classes, "hgr_free_gen_input: null operand");
    HGR_OT_OK("hgr_free_gen_input");
    HGR_REQUIRE(rows >= 1 && num >= 1 && n_classes >= 1 && att_rows >= 1 && row0 >= 0 && row0 + rows <= (int64_t)n_classes * num,
                "hgr_free_gen_input: rows [%lld, %lld) outside the %d x %d synthetic rows", (long long)row0, (long long)(row0 + rows), n_classes, num);
    HGR_REQUIRE(nz >= 8 && nz % 8 == 0 && A >= 8 && A % 8 == 0, "hgr_free_gen_input: nz=%d and A=%d must be multiples of 8", nz, A);
    HGR_REQUIRE(out_ok(out, ld_out, nz + A) && rows_f32_ok(att, ld_att, A) && (!z || rows_f32_ok(z, ld_z, nz)),
                "hgr_free_gen_input: out / att / z must be 16-byte aligned, ld_out a multiple of 8 and >= nz + A, ld_att / ld_z multiples of 4 and >= A / nz");
    const dim3 grid(hgr_grid1((int64_t)rows * ((nz + A) / 8), hgr_cu_count() * 16, NT)), block(NT);
    hgr_by_out_type(out_type, [&](auto ot) {
        hipLaunchKernelGGL((gen_input<ot.value>), grid, block, 0, (hipStream_t)stream, out, ld_out, z, ld_z, att, ld_att, att_rows, classes, n_classes, num, rows, nz, A,
                           normal_key(seed, stream_id), row0); });
    HGR_CHECK_LAUNCH("hgr_free_gen_input");
    return HGR_OK;
}

extern "C" int hgr_bias_act_rows(const float *x, int64_t ld_x, const float *bias, void *y, int64_t ld_y, int64_t col0, int out_type, int act,
                                 int rows, int C, void *stream) {
    HGR_REQUIRE(x && bias && y, "hgr_bias_act_rows: null operand");
    HGR_OT_OK("hgr_bias_act_rows");
    HGR_REQUIRE(act == HGR_ACT_LRELU02 || act == HGR_ACT_SIGMOID, "hgr_bias_act_rows: act=%d (0 LeakyReLU(0.2), 1 sigmoid)", act);
    HGR_REQUIRE(rows >= 1 && C >= 8 && C % 8 == 0 && col0 >= 0 && col0 % 8 == 0, "hgr_bias_act_rows: C=%d and col0=%lld must be multiples of 8", C, (long long)col0);
    HGR_REQUIRE(rows_f32_ok(x, ld_x, C) && hgr_aligned(bias, 16) && out_ok(y, ld_y, 0) && ld_y >= col0 + C,
                "hgr_bias_act_rows: x / bias / y must be 16-byte aligned, ld_x a multiple of 4 and >= C, ld_y a multiple of 8 and >= col0 + C");
    void *yo = out_type == OUT_F32 ? (void *)((float *)y + col0) : (void *)((unsigned short *)y + col0);
    const dim3 grid(hgr_grid1((int64_t)rows * (C / 8), hgr_cu_count() * 16, NT)), block(NT);
    hipStream_t s = (hipStream_t)stream;
    hgr_by_out_type(out_type, [&](auto ot) { hgr_by_flag(act == HGR_ACT_LRELU02, [&](auto lrelu) { constexpr int ACT = lrelu.value ? 0 : 1;
        hipLaunchKernelGGL((bias_act_rows<ot.value, ACT>), grid, block, 0, s, x, ld_x, bias, yo, ld_y, rows, C); }); });
    HGR_CHECK_LAUNCH("hgr_bias_act_rows");
    return HGR_OK;
}

extern "C" int hgr_free_fr_tail(const float *lantent, int64_t ld_l, const float *bias, const float *eps, int64_t ld_eps, void *y, int64_t ld_y,
                                int64_t col0, int out_type, float *mus, int64_t ld_mus, int rows, int A, int seed, int stream_id, int64_t row0,
                                void *stream) {
    HGR_REQUIRE(lantent && y, "hgr_free_fr_tail: null operand");
    HGR_OT_OK("hgr_free_fr_tail");
    HGR_REQUIRE(rows >= 1 && A >= 8 && A % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && row0 >= 0, "hgr_free_fr_tail: A=%d and col0=%lld must be multiples of 8", A, (long long)col0);
    HGR_REQUIRE(rows_f32_ok(lantent, ld_l, 2 * A) && hgr_aligned(bias, 16) && (!eps || rows_f32_ok(eps, ld_eps, A)) && (!mus || rows_f32_ok(mus, ld_mus, A)) &&
                out_ok(y, ld_y, 0) && ld_y >= col0 + A,
                "hgr_free_fr_tail: operands must be 16-byte aligned, ld_l / ld_eps / ld_mus multiples of 4 and >= 2A / A / A, ld_y a multiple of 8 and >= col0 + A");
    void *yo = out_type == OUT_F32 ? (void *)((float *)y + col0) : (void *)((unsigned short *)y + col0);
    const dim3 grid(hgr_grid1((int64_t)rows * (A / 8), hgr_cu_count() * 16, NT)), block(NT);
    hgr_by_out_type(out_type, [&](auto ot) {
        hipLaunchKernelGGL((fr_tail<ot.value>), grid, block, 0, (hipStream_t)stream, lantent, ld_l, bias, eps, ld_eps, yo, ld_y, mus, ld_mus, rows, A,
                           normal_key(seed, stream_id), row0); });
    HGR_CHECK_LAUNCH("hgr_free_fr_tail");
    return HGR_OK;
}

extern "C" int hgr_nll_rows16(const float *logits, int64_t ld, const int32_t *labels, int rows, int n, float *loss_rows, void *dlogits,
                              int64_t ld_d, float *logsm, int64_t ld_ls, int dtype, void *stream) {
    HGR_REQUIRE(logits && rows >= 1 && n >= 1, "hgr_nll_rows16: null logits or empty shape (rows=%d n=%d)", rows, n);
    HGR_REQUIRE(loss_rows || dlogits || logsm, "hgr_nll_rows16: nothing to write");
    HGR_REQUIRE(labels || !(loss_rows || dlogits), "hgr_nll_rows16: the loss and the gradient need labels");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_nll_rows16: dtype must be HGR_BF16 or HGR_F16");
    HGR_REQUIRE(ld >= n && ld % 8 == 0 && hgr_aligned(logits, 16), "hgr_nll_rows16: ld=%lld must be a multiple of 8 and >= n=%d, logits 16-byte aligned", (long long)ld, n);
    HGR_REQUIRE(!dlogits || (ld_d % 8 == 0 && ld_d >= ld && ld <= 0x7fffffff && hgr_aligned(dlogits, 16)),
                "hgr_nll_rows16: ld_d=%lld must be a multiple of 8 and >= ld=%lld, dlogits 16-byte aligned", (long long)ld_d, (long long)ld);
    HGR_REQUIRE(!logsm || (ld_ls % 4 == 0 && ld_ls >= n && hgr_aligned(logsm, 16)), "hgr_nll_rows16: ld_ls=%lld must be a multiple of 4 and >= n, logsm 16-byte aligned", (long long)ld_ls);
    const int npad = (n + 7) & ~7;
    const dim3 grid(rows), block(NT);
    hipStream_t s = (hipStream_t)stream;
    const bool resident = npad <= NLL_RES;
    const size_t bytes = resident ? (size_t)npad * sizeof(float) : 0;
    if (bytes > 65536) {                            // asked for at every such launch: the grant belongs to the current device's copy of the kernel
        const void *k = dtype == HGR_BF16 ? (const void *)nll_rows16<HGR_BF16, true> : (const void *)nll_rows16<HGR_F16, true>;
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, NLL_RES * (int)sizeof(float));
        if (e != hipSuccess) return hgr_set_error(HGR_ELAUNCH, "hgr_nll_rows16: cannot reserve %d B of LDS: %s", NLL_RES * 4, hipGetErrorString(e));
    }
    hgr_by_flag(resident, [&](auto res) { hgr_by_dtype(dtype, [&](auto dt) { typedef typename decltype(dt)::elem E;
        hipLaunchKernelGGL((nll_rows16<dt.value, res.value>), grid, block, bytes, s, logits, ld, labels, n, loss_rows, (E *)dlogits, ld_d, (int)ld, logsm, ld_ls); }); });
    HGR_CHECK_LAUNCH("hgr_nll_rows16");
    return HGR_OK;
}

extern "C" int hgr_adam_l2_cast16(float *p, const float *g, int64_t slice_stride, int n_slices, float alpha, float *m, float *v, void *w16,
                                  int64_t n, float lr, float beta1, float beta2, float eps, float wd, int step, int dtype, void *stream) {
    HGR_REQUIRE(p && g && m && v && w16, "hgr_adam_l2_cast16: null operand");
    HGR_REQUIRE(n >= 4 && n % 4 == 0 && step >= 1 && n_slices >= 1, "hgr_adam_l2_cast16: n=%lld must be a multiple of 4, step and n_slices >= 1", (long long)n);
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_adam_l2_cast16: dtype must be HGR_BF16 or HGR_F16");
    HGR_REQUIRE(n_slices == 1 || (slice_stride >= n && slice_stride % 4 == 0), "hgr_adam_l2_cast16: slice_stride=%lld must be a multiple of 4 and >= n", (long long)slice_stride);
    HGR_REQUIRE(hgr_aligned(p, 16) && hgr_aligned(g, 16) && hgr_aligned(m, 16) && hgr_aligned(v, 16) && hgr_aligned(w16, 8),
                "hgr_adam_l2_cast16: p / g / m / v must be 16-byte aligned, w16 8-byte aligned");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const dim3 grid(hgr_grid1(n / 4, hgr_cu_count() * 16, NT)), block(NT);
    hipStream_t s = (hipStream_t)stream;
    const float step_size = (float)((double)lr / bc1), isb = (float)(1.0 / sqrt(bc2));
    hgr_by_dtype(dtype, [&](auto dt) { typedef typename decltype(dt)::elem E;
        hipLaunchKernelGGL((adam_l2_cast16<dt.value>), grid, block, 0, s, p, g, slice_stride, n_slices, alpha, m, v, (E *)w16, n / 4, beta1, beta2, eps, wd, step_size, isb); });
    HGR_CHECK_LAUNCH("hgr_adam_l2_cast16");
    return HGR_OK;
}
