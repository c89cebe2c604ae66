// Kernels of the torchvision-style ResNet (baseline/resnet.py, the DGP baseline's feature extractor): the 7 x 7 / stride 2 stem with its
// 3 x 3 / stride 2 max-pool, the row gather of the strided 1 x 1 `downsample` convolution and the global mean.  The rest of the net runs
// on hgr_gemm_nt and hgr_conv3x3_nhwc.  Activations NHWC in the 16-bit MFMA type, fp32 accumulation.
//
// Rounding contract of the stem, shared by the fused kernel and the unfused route (hgr_stem7_im2col -> hgr_gemm_nt(BIAS_RELU) ->
// hgr_maxpool3s2_nhwc): relu(conv + bias) is rounded to 16 bit ONCE and the max is taken over those 16-bit values.  A max-pool tap outside
// the conv map is IGNORED (never a padded 0), so the kernels stay right for inputs that are not preceded by a ReLU.
#include "hgr_launch.h"

namespace {

// ---- fused stem -------------------------------------------------------------------------------------------------------------------
// A workgroup owns an 8 x 8 tile of POOLED outputs of one image = 17 x 17 conv outputs = a 39 x 40 x 3 input patch, which is converted
// to 16 bit once on its way into LDS (zero outside the image = the conv's padding).  K is ordered (ky, c, kx) with kx padded to 8: the 8
// values of one (ky, c) chunk are 8 consecutive patch columns, 16 contiguous, 4-byte aligned bytes of LDS (the 8th meets a zero weight) -
// 21 chunks + 3 zero chunks = 6 k-steps of v_mfma_f32_16x16x32.  The folded weights never touch LDS: every lane keeps its 4 x 6 A fragments
// (all 64 output channels) in 96 registers for the whole persistent launch.  Each wave walks over 16-pixel groups of the 289 conv outputs;
// results are staged as 16-bit values (stride 144 B per pixel) and the pool reads the staged tile, so only the pooled tensor is written.
// Measured (batch 256, 224 x 224, f16, profiles/NOTES.md "DGP ResNet-50"): 0.235 ms against 1.22 ms for the unfused route and a byte
// floor of 0.04 ms.  The MFMA loop is not what bounds it: 32 channels per wave with the next group's fragments read ahead ran in the
// same time.  Nor is it the count of vector-ALU instructions: a fetch in which a thread keeps one patch column (no division per load)
// together with a packed 16-bit max in the pool took 188 registers instead of 253 and ran SLOWER, 0.338 ms.  What bounds the kernel is
// not known; it has not been looked at with counters.
constexpr int S7_TP = 8;                       // pooled tile edge
constexpr int S7_TC = 2 * S7_TP + 1;           // conv tile edge (17)
constexpr int S7_ROWS = 2 * S7_TC + 5;         // input patch rows (39)
constexpr int S7_RS = 48;                      // patch row stride in elements (40 live columns)
constexpr int S7_PIX = S7_TC * S7_TC;          // 289
constexpr int S7_GROUPS = (S7_PIX + 15) / 16;  // 19
constexpr int S7_STG = 144;                    // staged bytes per conv pixel (128 live)
constexpr int S7_PATCH_BYTES = S7_ROWS * 3 * S7_RS * 2;   // 11232

struct Stem7Args {
    const float *img; const char *w; const float *bias; char *out;
    int B, R, Hc, Hp, Kp, tiles;               // tiles per image edge
};

template <int DT>
__global__ __launch_bounds__(256, 2) void stem7_pool(Stem7Args p) {
    typedef typename T16<DT>::vec8 vec8;
    typedef typename T16<DT>::vec4 vec4;
    typedef typename T16<DT>::elem E;
    __shared__ __attribute__((aligned(16))) char smem[S7_PATCH_BYTES + S7_PIX * S7_STG];
    E *patch = (E *)smem;
    char *stg = smem + S7_PATCH_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int R = p.R;
    const int ntiles = p.B * p.tiles * p.tiles;

    // ---- weights: fragment (i, s) = output channel i * 16 + r, chunk q = 4 s + g = (ky, c), element e = kx
    vec8 wf[4][6];
    f32x4 bq[4];
    const E *wg = (const E *)p.w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = i * 16 + r;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int q = s * 4 + g, qc = min(q, 20), ky = qc / 3, c = qc - ky * 3;
            // unconditional (clamped) loads, then a select: behind a branch each of the 168 loads of a lane waited for the one before it
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const E v = wg[co * p.Kp + (ky * 7 + min(e, 6)) * 3 + c];
                wf[i][s][e] = (q < 21 && e < 7) ? v : (E)0.f;
            }
        }
        bq[i] = *(const f32x4 *)(p.bias + i * 16 + g * 4);
    }

    // ---- patch of a tile: [row][c][40 columns] of fp32 pixels, zero outside the image, into registers: S7_LD unconditional (clamped)
    // loads per thread issued back to back, then a select.  The NEXT tile's patch is fetched while the current tile computes - taken one
    // at a time behind a branch the 19 loads of a thread cost 19 memory round trips per tile (first build: 0.39 ms per batch-256 launch).
    constexpr int S7_LIVE = S7_ROWS * 3 * 40, S7_LD = (S7_LIVE + 255) / 256;
    float pre[S7_LD];
    auto fetch = [&](int t) {
        const int tx = t % p.tiles; t /= p.tiles;
        const int ty = t % p.tiles; const int b = t / p.tiles;
        const int iy0 = 4 * ty * S7_TP - 5, ix0 = 4 * tx * S7_TP - 5;       // first input row / column of the patch
        const char *img = (const char *)(p.img + (int64_t)b * 3 * R * R);   // wave-uniform; one image is < 4 GB (R <= 16384): 32-bit lane offsets
#pragma unroll
        for (int i = 0; i < S7_LD; ++i) {
            const int id = min(i * 256 + tid, S7_LIVE - 1);
            const int col = id % 40, rc = id / 40, c = rc % 3, row = rc / 3;
            const int yi = iy0 + row, xi = ix0 + col;
            const bool ok = yi >= 0 && yi < R && xi >= 0 && xi < R;
            const unsigned off = ((unsigned)(c * R + min(max(yi, 0), R - 1)) * (unsigned)R + (unsigned)min(max(xi, 0), R - 1)) * 4u;
            const float v = *(const float *)(img + off);
            pre[i] = ok ? v : 0.f;
        }
    };
    fetch(blockIdx.x);                                         // gridDim.x <= ntiles

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int t = tile;
        const int tx = t % p.tiles; t /= p.tiles;
        const int ty = t % p.tiles; const int b = t / p.tiles;
        const int py0 = ty * S7_TP, px0 = tx * S7_TP;
        const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;        // first conv row / column of the tile (may be -1)

        // ---- the fetched patch -> 16 bit -> LDS (every wave is behind the previous tile's conv: the barrier in front of its pool)
#pragma unroll
        for (int i = 0; i < S7_LD; ++i) {
            const int id = i * 256 + tid;
            if (id < S7_LIVE) patch[(id / 40) * S7_RS + id % 40] = (E)pre[i];
        }
        // both barriers of the loop order LDS traffic only, so they are raw: __syncthreads() would also wait for the previous tile's
        // output stores here, and for the next tile's loads at the barrier below
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (tile + (int)gridDim.x < ntiles) fetch(tile + (int)gridDim.x);

        // ---- conv: 16 pixels x 64 channels per group; pixel index beyond 288 is clamped (computed again, stored to the same place)
        for (int grp = wave; grp < S7_GROUPS; grp += 4) {
            const int px = min(grp * 16 + r, S7_PIX - 1);
            const int ly = px / S7_TC, lx = px - ly * S7_TC;
            const unsigned *base = (const unsigned *)(patch + (2 * ly * 3) * S7_RS + 2 * lx);      // even element offset: 4-byte aligned
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int q = min(s * 4 + g, 20);              // chunks 21 .. 23 meet zero weights: read live (finite) data
                const unsigned *src = base + q * (S7_RS / 2);
                u32x4 raw;
                raw[0] = src[0]; raw[1] = src[1]; raw[2] = src[2]; raw[3] = src[3];
                const vec8 af = __builtin_bit_cast(vec8, raw);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = T16<DT>::mfma16(wf[i][s], af, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 v = acc[i] + bq[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                *(vec4 *)(stg + px * S7_STG + (i * 16 + g * 4) * 2) = cvt4<DT>(v[0], v[1], v[2], v[3]);
            }
        }
        // the staged tile is complete
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

        // ---- pool: 64 pooled pixels x 8 chunks of 8 channels; taps outside the conv map are skipped (the centre tap is always inside)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int id = it * 256 + tid;
            const int ch = id & 7, pp = id >> 3, plx = pp & 7, ply = pp >> 3;
            const int py = py0 + ply, pxg = px0 + plx;
            if (py < p.Hp && pxg < p.Hp) {
                float m[8];
                {
                    const vec8 v = *(const vec8 *)(stg + ((2 * ply + 1) * S7_TC + 2 * plx + 1) * S7_STG + ch * 16);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = (float)v[e];
                }
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        if (dy == 1 && dx == 1) continue;
                        const int cy = cy0 + 2 * ply + dy, cx = cx0 + 2 * plx + dx;
                        if (cy >= 0 && cy < p.Hc && cx >= 0 && cx < p.Hc) {
                            const vec8 v = *(const vec8 *)(stg + ((2 * ply + dy) * S7_TC + 2 * plx + dx) * S7_STG + ch * 16);
#pragma unroll
                            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
                        }
                    }
                vec8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (E)m[e];
                *(vec8 *)(p.out + ((((int64_t)b * p.Hp + py) * p.Hp + pxg) * 64 + ch * 8) * 2) = o;
            }
        }
        // the next tile's patch is written to LDS by waves that are done with their pool (nobody reads the patch any more); the staging
        // area is written only behind the next tile's first barrier, which every wave reaches after its pool reads
    }
}

// ---- unfused route: im2col of the 7 x 7 stem, K order (ky, kx, c) = the folded weight's -------------------------------------------
// one thread per (output pixel, 8 K columns): eight clamped loads + select, one 16-byte store
template <int DT>
__global__ __launch_bounds__(256) void stem7_im2col(const float *__restrict__ img, typename T16<DT>::elem *__restrict__ out, int B, int R, int Kp) {
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::vec8 vec8;
    const int Hc = (R - 1) / 2 + 1, kc = Kp / 8;
    const int64_t total = (int64_t)B * Hc * Hc * kc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ch = (int)(i % kc);
        const int64_t row = i / kc;
        const int wo = (int)(row % Hc), ho = (int)((row / Hc) % Hc), b = (int)(row / ((int64_t)Hc * Hc));
        vec8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = ch * 8 + e, kk = min(k, 146);
            const int tap = kk / 3, c = kk - tap * 3, ky = tap / 7, kx = tap - ky * 7;
            const int hi = ho * 2 - 3 + ky, wi = wo * 2 - 3 + kx;
            const bool ok = k < 147 && hi >= 0 && hi < R && wi >= 0 && wi < R;
            const int hc = min(max(hi, 0), R - 1), wc = min(max(wi, 0), R - 1);
            const float x = img[(((int64_t)b * 3 + c) * R + hc) * R + wc];
            v[e] = (E)(ok ? x : 0.f);
        }
        *(vec8 *)(out + i * 8) = v;
    }
}

// 3 x 3 / stride 2 / pad 1 max-pool, one thread per (output pixel, 8 channels); taps outside the map are skipped
template <int DT>
__global__ __launch_bounds__(256) void maxpool3s2(const typename T16<DT>::elem *__restrict__ x, typename T16<DT>::elem *__restrict__ out,
                                                  int B, int H, int W, int C) {
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::vec8 vec8;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, cv = C / 8;
    const int64_t total = (int64_t)B * Ho * Wo * cv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv);
        int64_t t = i / cv;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const E *img = x + (int64_t)b * H * W * C + c * 8;
        float m[8];
        {
            const vec8 v = *(const vec8 *)(img + ((int64_t)(2 * ho) * W + 2 * wo) * C);      // the centre tap is always inside
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = (float)v[e];
        }
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const int hi = 2 * ho + dy, wi = 2 * wo + dx;
                if (hi >= 0 && hi < H && wi >= 0 && wi < W) {
                    const vec8 v = *(const vec8 *)(img + ((int64_t)hi * W + wi) * C);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
                }
            }
        vec8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (E)m[e];
        *(vec8 *)(out + i * 8) = o;
    }
}

// out[b, yo, xo, :] = x[b, 2 yo, 2 xo, :]: the A operand of a 1 x 1 / stride 2 convolution; 16-byte pieces, no arithmetic
__global__ __launch_bounds__(256) void subsample2(const u32x4 *__restrict__ x, u32x4 *__restrict__ out, int B, int H, int W, int cv) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t total = (int64_t)B * Ho * Wo * cv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv);
        int64_t t = i / cv;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho);
        const int b = (int)(t / Ho);
        out[i] = x[(((int64_t)b * H + 2 * ho) * W + 2 * wo) * cv + c];
    }
}

// global mean over the H W cells: one thread per (image, 8 channels), fp32 sum in cell order, one true division, one rounding
template <int DT, bool OUT32>
__global__ __launch_bounds__(256) void meanpool(const typename T16<DT>::elem *__restrict__ x, void *__restrict__ out, int B, int G, int C) {
    typedef typename T16<DT>::elem E;
    typedef typename T16<DT>::vec8 vec8;
    const int cv = C / 8;
    const int64_t total = (int64_t)B * cv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cv), b = (int)(i / cv);
        float sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const E *src = x + (int64_t)b * G * C + c * 8;
        for (int g = 0; g < G; ++g) {
            const vec8 v = *(const vec8 *)(src + (int64_t)g * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum[e] += (float)v[e];
        }
        if (OUT32) {
            f32x4 *o = (f32x4 *)((float *)out + i * 8);
            o[0] = (f32x4){sum[0] / (float)G, sum[1] / (float)G, sum[2] / (float)G, sum[3] / (float)G};
            o[1] = (f32x4){sum[4] / (float)G, sum[5] / (float)G, sum[6] / (float)G, sum[7] / (float)G};
        } else {
            vec8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (E)(sum[e] / (float)G);
            *(vec8 *)((E *)out + i * 8) = o;
        }
    }
}

}  // namespace


extern "C" int hgr_stem7_pool(const float *image, const void *w, const float *bias, void *out, int B, int R, int Kp, int dtype, void *stream) {
    HGR_REQUIRE(image && w && bias && out && B >= 1 && R >= 1 && R <= 16384, "hgr_stem7_pool: bad arguments B=%d R=%d", B, R);
    HGR_REQUIRE(Kp >= 147 && Kp <= 65536, "hgr_stem7_pool: Kp=%d must lie in [147, 65536]", Kp);
    HGR_REQUIRE(hgr_aligned(image, 4) && hgr_aligned(w, 2) && hgr_aligned(bias, 16) && hgr_aligned(out, 16), "hgr_stem7_pool: misaligned operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_stem7_pool: bad dtype %d", dtype);
    Stem7Args a;
    a.img = image; a.w = (const char *)w; a.bias = bias; a.out = (char *)out;
    a.B = B; a.R = R; a.Hc = (R - 1) / 2 + 1; a.Hp = (a.Hc - 1) / 2 + 1; a.Kp = Kp; a.tiles = (a.Hp + S7_TP - 1) / S7_TP;
    const int64_t ntiles = (int64_t)B * a.tiles * a.tiles;
    HGR_REQUIRE(ntiles < (1ll << 31), "hgr_stem7_pool: too many tiles");
    dim3 grid((unsigned)std::min<int64_t>(ntiles, 2 * (int64_t)hgr_cu_count()));     // persistent: two workgroups per compute unit
    hipStream_t s = (hipStream_t)stream;
    hgr_by_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((stem7_pool<dt.value>), grid, dim3(256), 0, s, a); });
    HGR_CHECK_LAUNCH("hgr_stem7_pool");
    return HGR_OK;
}

extern "C" int hgr_stem7_im2col(const float *image, void *out, int B, int R, int Kp, int dtype, void *stream) {
    HGR_REQUIRE(image && out && B >= 1 && R >= 1 && R <= 16384, "hgr_stem7_im2col: bad arguments B=%d R=%d", B, R);
    HGR_REQUIRE(Kp >= 152 && Kp % 8 == 0 && Kp <= 4096, "hgr_stem7_im2col: Kp=%d must be a multiple of 8 in [152, 4096]", Kp);
    HGR_REQUIRE(hgr_aligned(image, 4) && hgr_aligned(out, 16), "hgr_stem7_im2col: misaligned operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_stem7_im2col: bad dtype %d", dtype);
    const int Hc = (R - 1) / 2 + 1;
    const int64_t total = (int64_t)B * Hc * Hc * (Kp / 8);
    hgr_by_dtype(dtype, [&](auto dt) { typedef typename decltype(dt)::elem E;
        hipLaunchKernelGGL((stem7_im2col<dt.value>), dim3(hgr_grid1(total, 16384)), dim3(256), 0, (hipStream_t)stream, image, (E *)out, B, R, Kp); });
    HGR_CHECK_LAUNCH("hgr_stem7_im2col");
    return HGR_OK;
}

extern "C" int hgr_maxpool3s2_nhwc(const void *x, void *out, int B, int H, int W, int C, int dtype, void *stream) {
    HGR_REQUIRE(x && out && B >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "hgr_maxpool3s2_nhwc: bad geometry B=%d H=%d W=%d C=%d", B, H, W, C);
    HGR_REQUIRE(hgr_aligned(x, 16) && hgr_aligned(out, 16), "hgr_maxpool3s2_nhwc: misaligned operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_maxpool3s2_nhwc: bad dtype %d", dtype);
    const int64_t total = (int64_t)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (C / 8);
    hgr_by_dtype(dtype, [&](auto dt) { typedef typename decltype(dt)::elem E;
        hipLaunchKernelGGL((maxpool3s2<dt.value>), dim3(hgr_grid1(total, 16384)), dim3(256), 0, (hipStream_t)stream, (const E *)x, (E *)out, B, H, W, C); });
    HGR_CHECK_LAUNCH("hgr_maxpool3s2_nhwc");
    return HGR_OK;
}

extern "C" int hgr_subsample2_nhwc(const void *x, void *out, int B, int H, int W, int C, int dtype, void *stream) {
    HGR_REQUIRE(x && out && x != out && B >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "hgr_subsample2_nhwc: bad geometry B=%d H=%d W=%d C=%d", B, H, W, C);
    HGR_REQUIRE(hgr_aligned(x, 16) && hgr_aligned(out, 16), "hgr_subsample2_nhwc: misaligned operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_subsample2_nhwc: bad dtype %d", dtype);
    const int64_t total = (int64_t)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (C / 8);
    hipLaunchKernelGGL(subsample2, dim3(hgr_grid1(total, 16384)), dim3(256), 0, (hipStream_t)stream, (const u32x4 *)x, (u32x4 *)out, B, H, W, C / 8);
    HGR_CHECK_LAUNCH("hgr_subsample2_nhwc");
    return HGR_OK;
}

extern "C" int hgr_meanpool_nhwc(const void *x, void *out, int B, int H, int W, int C, int dtype, int out_f32, void *stream) {
    HGR_REQUIRE(x && out && B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W < (1 << 24) && C >= 8 && C % 8 == 0, "hgr_meanpool_nhwc: bad geometry B=%d H=%d W=%d C=%d", B, H, W, C);
    HGR_REQUIRE(hgr_aligned(x, 16) && hgr_aligned(out, 16), "hgr_meanpool_nhwc: misaligned operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_meanpool_nhwc: bad dtype %d", dtype);
    HGR_REQUIRE(out_f32 == 0 || out_f32 == 1, "hgr_meanpool_nhwc: out_f32=%d must be 0 or 1", out_f32);
    const int64_t total = (int64_t)B * (C / 8);
    const dim3 grid(hgr_grid1(total, 16384));
    hipStream_t s = (hipStream_t)stream;
    hgr_by_dtype(dtype, [&](auto dt) { hgr_by_flag(out_f32, [&](auto f32) { typedef typename decltype(dt)::elem E;
        hipLaunchKernelGGL((meanpool<dt.value, f32.value>), grid, dim3(256), 0, s, (const E *)x, out, B, H * W, C); }); });
    HGR_CHECK_LAUNCH("hgr_meanpool_nhwc");
    return HGR_OK;
}
