// =================================================================================================
// vit_patch_embed_ln: the front of the ViT tower (clip/model.py:219-226: conv1 as a GEMM over the patches, class token, positional
// embedding, ln_pre) in ONE launch, from fp32 NCHW pixels to the residual pair + slot statistics of the first block - the bits of
// hgr_im2col_patches -> hgr_gemm_nt (fp32 out) -> hgr_vit_embed_ln_stats, without the unfolded 16-bit patch matrix and without the
// fp32 patch embedding in memory.
//
// Tile: the patches of TWO images (2 gg <= 112 rows = 7 MFMA row tiles, rows behind 2 gg are padding: computed, never stored) x ALL
// 768 output columns; one 512-thread workgroup per tile, one per CU.  A tile that owns the whole row fetches its pixels ONCE (the
// 128-column tiles of gemm_nt_duo fetch a row panel six times, which is what an fp32 A operand could not afford there) and has the
// whole row for ln_pre.  8 waves, wave w owns all 112 rows x columns [96 w, 96 w + 96) = 7 x 6 accumulator tiles (168 registers).
//
// K-tile = 32 = one pixel row (channel, py) of every patch: for one image and one patch that is 128 contiguous bytes of fp32, so the
// A piece of a K-tile is 128 rows x 128 B (16 KB; rows 112-127 only keep the LDS-DMA count per wave uniform) and the W piece is
// 768 x 64 B = 48 KB, cut in two by the phase that reads it: W0 = columns [0, 48) of every wave's 96, W1 = columns [48, 96).
// Two stages of (A | W0) = 40 KB and of W1 = 24 KB: 128 KB of LDS.  Counted-vmcnt loop, every piece refilled for K-tile t + 2 in the
// phase after the barrier that follows its last read (8 LDS-DMA instructions per thread in flight behind every wait):
//     ph1(t): reads A(t) (14 x ds_read_b128, fp32 -> MFMA type in registers), W0(t) (3 x)   issues W1(t+1) x3        waits vmcnt(8): W1(t) landed
//     ph2(t): reads W1(t) (3 x), the A fragments stay                                      issues A(t+2) x2, W0(t+2) x3  waits vmcnt(8): A(t+1), W0(t+1) landed
// (one loop body for all 96 K-tiles: behind the last one the refills re-request K-tile 95 into slots nothing reads any more)
// 21 MFMAs per wave and phase; waves 0-3 and 4-7 (one of each per SIMD) run one barrier interval apart, so that one group's fragment
// reads sit under the other one's MFMAs (the ping-pong of gemm_nt_p8).  W is the MFMA "A" operand and the pixels "B", K ascends in MFMA steps of 32 from a zero accumulator
// and the pixels are rounded with the conversion of im2col_vec8 ((E)x, nearest even): the accumulator chain of gemm_nt_duo, bit for bit.
//
// LDS images (lane-linear 1 KB per LDS-DMA wave-instruction, the swizzle applied on the per-lane SOURCE address and on the read):
//   A : row = 128 B = 8 chunks of 4 pixels; chunk c of row p sits in slot (((c >> 1) ^ (p >> 1 & 3)) << 1) | ((c & 1) ^ ((p + 4) >> 3 & 1));
//       lane (r, g) reads chunks 2 g and 2 g + 1 of row 16 i + r: the 16 lanes of every ds_read_b128 lane group hit 16 distinct
//       16-byte bank groups of the 256-byte LDS row.
//   W : line = 128 B = piece rows 2 l, 2 l + 1 (64 B each); chunk8 = (row & 1) * 4 + k chunk sits in slot chunk8 ^ (l & 7).
//
// Epilogue: the accumulators go through LDS as fp32 rows, 48 tile rows (3 MFMA row tiles) per pass, row stride 3072 + 16 B; every wave
// then runs vit_ln_row() (hgr_common.h: the row routine of vit_embed_ln, one copy of the text) on 6 rows per pass with the lane-to-
// element assignment of that kernel, v = patch embedding + positional embedding, and stores the pair and the statistics of the rows
// that exist.  The class-token rows of the tile's images are written by waves 0 / 1 straight from cls + pos[0].
// No workgroup depends on another one.
// =================================================================================================
#include "hgr_gemm_common.h"
#include "hgr_launch.h"

namespace hgr_gemm {
namespace {
constexpr int PE_NT = 512;
constexpr int PE_W = 768, PE_P = 32, PE_K = 3 * PE_P * PE_P, PE_NK = PE_K / 32;      // 96 K-tiles
constexpr int PE_MT = 7, PE_ROWS = 16 * PE_MT;               // 112 tile rows
constexpr int PE_A = 0, PE_W0 = 32768, PE_W1 = 81920;        // A: 2 x 16 KB | W0: 2 x 24 KB | W1: 2 x 24 KB
constexpr int PE_ASZ = 16384, PE_WSZ = 24576;
constexpr int PE_RS = PE_W * 4 + 16, PE_PR = 48;             // epilogue: fp32 row stride, tile rows per pass
constexpr int PE_LDS = PE_PR * PE_RS;                        // 148 224 B (the main loop uses 131 072)
static_assert(PE_W1 + 2 * PE_WSZ <= PE_LDS, "the stages fit under the epilogue's rows");

template <int DT>
__global__ __launch_bounds__(PE_NT) void vit_patch_embed_ln(const float *__restrict__ image, const char *__restrict__ conv_w, const float *__restrict__ cls,
                                                            const float *__restrict__ pos, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            void *__restrict__ xh, void *__restrict__ xl, float *__restrict__ stats,
                                                            int B, int R, int gs, float eps) {
    typedef typename T16<DT>::vec8 vec8;
    typedef typename T16<DT>::elem E;
    __shared__ __attribute__((aligned(1024))) char smem[PE_LDS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                                // waves w and w + 4 share a SIMD: one of each ping-pong group
    const int r = lane & 15, g = lane >> 4;
    const int gg = gs * gs;
    const int img0 = blockIdx.x * 2;
    const bool two = img0 + 1 < B;                            // an odd last tile has one image: the second one's rows read the first one's pixels
    const int64_t img_elems = (int64_t)3 * R * R;
    const char *const abase = (const char *)(image + (int64_t)img0 * img_elems);     // the tile's own images: 32-bit offsets stay below 2 images

    // per-lane source offsets (bytes) of one K-tile's LDS-DMA instructions: A 2, W 3 (W1 = the rows 48 behind W0's: the constant rides
    // in the scalar offset with the K advance)
    unsigned oA[2], oW[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int id = (i * 8 + wave) * 64 + lane;
        const int line = id >> 3, slot = id & 7;
        if (i < 2) {
            const int pr = line;                              // A piece row = tile row
            const int c = ((((slot >> 1) ^ ((pr >> 1) & 3)) << 1) | ((slot & 1) ^ (((pr + 4) >> 3) & 1)));
            int tr = pr < 2 * gg ? pr : 0;                    // padding rows: a valid address, never stored
            const int im = tr >= gg ? 1 : 0;
            const int patch = tr - im * gg;
            const int gy = patch / gs, gx = patch - gy * gs;
            oA[i] = (unsigned)((((int64_t)((im && two) ? 1 : 0) * img_elems + (int64_t)gy * PE_P * R + gx * PE_P) * 4) + c * 16);
        }
        const int c8 = slot ^ (line & 7);
        const int q = 2 * line + (c8 >> 2);                   // piece row (0 .. 383): wave q / 48, its column q % 48 (+ 48 in W1)
        const int n = 96 * (q / 48) + q % 48;
        oW[i] = (unsigned)(n * (PE_K * 2) + (c8 & 3) * 16);
    }
    char *const ldsw = smem + wave * 1024;
    const __amdgpu_buffer_rsrc_t rA = dma_rsrc(abase), rW = dma_rsrc(conv_w);
    const int RR4 = R * R * 4, R4 = R * 4;
    auto issueA = [&](int t) {                                // K-tile t = pixel row (channel t / 32, py t % 32) of every patch
        char *dst = ldsw + PE_A + (t & 1) * PE_ASZ;
        const int ts = min(t, PE_NK - 1);                       // (behind the last K-tile: see the loop)
        const int soff = (ts >> 5) * RR4 + (ts & 31) * R4;
#pragma unroll
        for (int i = 0; i < 2; ++i) dma16(rA, oA[i], soff, dst + i * 8192);
    };
    auto issueW = [&](int half, int t) {                      // half 0 = piece W0, 1 = W1
        char *dst = ldsw + (half ? PE_W1 : PE_W0) + (t & 1) * PE_WSZ;
#pragma unroll
        for (int i = 0; i < 3; ++i) dma16(rW, oW[i], min(t, PE_NK - 1) * 64 + half * (48 * PE_K * 2), dst + i * 8192);
    };

    // fragment addresses (see the LDS images above)
    const int offA = r * 128 + ((g ^ ((r >> 1) & 3)) << 5);                   // + m tile * 2048; the two chunks of the lane's 32 bytes:
    const int hsA = (((r + 4) >> 3) & 1) << 4;                                // chunk 2 g at + hsA, chunk 2 g + 1 at + (16 - hsA)
    const int offW = (24 * wave + (r >> 1)) * 128 + ((((r & 1) * 4 + g) ^ (r >> 1)) << 4);      // + n tile * 1024

    f32x4 acc[PE_MT][6];        // [m tile][n tile]: C[16 i + r][96 wave + 16 j + 4 g .. + 3]
#pragma unroll
    for (int i = 0; i < PE_MT; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    vec8 af[PE_MT], wf[3];

    // prologue in steady-state order: A(0), W0(0) | W1(0) | A(1), W0(1)
    issueA(0); issueW(0, 0);
    issueW(1, 0);
    issueA(1); issueW(0, 1);
    HGR_RWAIT(8);               // A(0), W0(0) landed
    if (grp) HGR_MBAR();        // ping-pong: group 1 runs one barrier interval behind group 0

    // One loop body for every K-tile, the last two included: behind the last K-tile the refills re-request K-tile PE_NK - 1 into slots
    // that nothing reads any more (2 of 96 K-tiles of extra fill), so the counts of the waits stay what they are in the steady state
    // and no accumulator register changes its place in peeled copies of the body.
    for (int t = 0; t < PE_NK; ++t) {
        const char *sa = smem + PE_A + (t & 1) * PE_ASZ, *sw0 = smem + PE_W0 + (t & 1) * PE_WSZ, *sw1 = smem + PE_W1 + (t & 1) * PE_WSZ;
        // ---- ph1: all rows x the wave's columns 0-47 ----
#pragma unroll
        for (int j = 0; j < 3; ++j) wf[j] = *(const vec8 *)(sw0 + offW + j * 1024);
#pragma unroll
        for (int i = 0; i < PE_MT; ++i) {
            const f32x4 lo = *(const f32x4 *)(sa + offA + i * 2048 + hsA);
            const f32x4 hi = *(const f32x4 *)(sa + offA + i * 2048 + (16 - hsA));
            vec8 a;
            a[0] = (E)lo[0]; a[1] = (E)lo[1]; a[2] = (E)lo[2]; a[3] = (E)lo[3];
            a[4] = (E)hi[0]; a[5] = (E)hi[1]; a[6] = (E)hi[2]; a[7] = (E)hi[3];
            af[i] = a;
        }
        issueW(1, t + 1);                                       // its slot was last read in ph2(t - 1), by both groups before the last barrier
        HGR_RWAIT(8);                                           // W1(t) landed
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < PE_MT; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i][j] = T16<DT>::mfma16(wf[j], af[i], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
        HGR_MBAR();
        // ---- ph2: columns 48-95, the A fragments stay ----
#pragma unroll
        for (int j = 0; j < 3; ++j) wf[j] = *(const vec8 *)(sw1 + offW + j * 1024);
        issueA(t + 2); issueW(0, t + 2);                        // read in ph1(t)
        HGR_RWAIT(8);                                           // A(t+1), W0(t+1) landed
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < PE_MT; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i][3 + j] = T16<DT>::mfma16(wf[j], af[i], acc[i][3 + j]);
        __builtin_amdgcn_s_setprio(0);
        HGR_MBAR();
    }
    if (!grp) HGR_MBAR();       // group 0 waits for group 1's last interval: every fragment read is done
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the refills behind the last K-tile have landed before the epilogue's rows overwrite the stages

    const int L = gg + 1;
    constexpr int nv = PE_W >> 2;
    // (opaque copy: every lane-derived term of the epilogue is computed here instead of being kept live - and spilled - across the main loop)
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int lane_e = tid_e & 63, r_e = lane_e & 15, g_e = lane_e >> 4;
    // ---- patch rows, 48 tile rows per pass through LDS ----
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        __syncthreads();                                        // the main loop's reads / the previous pass's rows are done
        if (pass * PE_PR < 2 * gg) {
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) {
                const int i = pass * 3 + ii;
                if (i < PE_MT) {
#pragma unroll
                    for (int j = 0; j < 6; ++j)
                        *(f32x4 *)(smem + (ii * 16 + r_e) * PE_RS + (96 * wave + 16 * j + 4 * g_e) * 4) = acc[i < PE_MT ? i : 0][j];
                }
            }
        }
        __syncthreads();
        int ln = lane_e;                                         // opaque per pass: nothing lane-derived of the row phase (gamma / beta, addresses)
        asm volatile("" : "+v"(ln));                           // is hoisted in front of the passes, where every accumulator is still live
        // the wave's 6 rows of the pass as independent chains (loads, two wave reductions, stores): unrolled so that they overlap
#pragma unroll
        for (int k = 0; k < PE_PR / 8; ++k) {
            const int lr = k * 8 + wave, tr = pass * PE_PR + lr;          // wave-uniform
            const int im = tr >= gg ? 1 : 0;
            if (tr < 2 * gg && tr < PE_ROWS && (!im || two)) {
                const int patch = tr - im * gg;
                const f32x4 *src = (const f32x4 *)(smem + lr * PE_RS), *pr = (const f32x4 *)(pos + (int64_t)(1 + patch) * PE_W);
                f32x4 v[4];
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = i * 64 + ln;
                    if (i * 64 < nv) {
                        v[i] = (c < nv) ? (src[c] + pr[c]) : (f32x4){0.f, 0.f, 0.f, 0.f};
                        s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
                    }
                }
                vit_ln_row<4, DT, true>(v, s, ln, nv, PE_W, eps, gamma, beta, nullptr, (img0 + im) * L + 1 + patch, xh, xl, stats);
            }
        }
    }

    // ---- class-token rows: waves 0 / 1, image img0 / img0 + 1 (behind the patch rows: no accumulator is live any more) ----
    if (wave < 2 && (wave == 0 || two)) {
        const f32x4 *src = (const f32x4 *)cls, *pr = (const f32x4 *)pos;
        f32x4 v[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 64 + lane_e;
            if (i * 64 < nv) {
                v[i] = (c < nv) ? (src[c] + pr[c]) : (f32x4){0.f, 0.f, 0.f, 0.f};
                s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
            }
        }
        vit_ln_row<4, DT, true>(v, s, lane_e, nv, PE_W, eps, gamma, beta, nullptr, (img0 + wave) * L, xh, xl, stats);
    }
}

}  // namespace
}  // namespace hgr_gemm

// Shape contract of hgr_vit_patch_embed_ln (1 = this launch covers the geometry): patch 32, grid side a whole number with at most 56
// patches per image (two images inside the 112 tile rows), width 768, a 16-bit MFMA type.
extern "C" int hgr_vit_patch_embed_ln_ok(int B, int R, int P, int W, int dtype) {
    if (B < 1 || P != hgr_gemm::PE_P || R < P || R % P != 0 || W != hgr_gemm::PE_W) return 0;
    const int gs = R / P;
    if (gs * gs > hgr_gemm::PE_ROWS / 2) return 0;
    if ((int64_t)B * (gs * gs + 1) >= (int64_t)1 << 31) return 0;      // row indices are 32-bit
    return dtype == HGR_BF16 || dtype == HGR_F16;
}

extern "C" int hgr_vit_patch_embed_ln(const float *image, const void *conv_w, const float *class_embedding, const float *positional_embedding,
                                      const float *gamma, const float *beta, void *xh, void *xl, float *stats,
                                      int B, int R, int P, int W, float eps, int dtype, void *stream) {
    using namespace hgr_gemm;
    HGR_REQUIRE(image && conv_w && class_embedding && positional_embedding && gamma && beta && xh && xl && stats, "hgr_vit_patch_embed_ln: null operand");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_vit_patch_embed_ln: bad dtype %d", dtype);
    HGR_REQUIRE(P == PE_P, "hgr_vit_patch_embed_ln: patch size P=%d unsupported (32)", P);
    HGR_REQUIRE(W == PE_W, "hgr_vit_patch_embed_ln: width W=%d unsupported (768)", W);
    HGR_REQUIRE(B >= 1 && R >= P && R % P == 0, "hgr_vit_patch_embed_ln: B=%d R=%d unsupported (R a multiple of %d)", B, R, P);
    const int gs = R / P, gg = gs * gs;
    HGR_REQUIRE(gg <= PE_ROWS / 2, "hgr_vit_patch_embed_ln: %d patches per image exceed %d (two images per 112-row tile)", gg, PE_ROWS / 2);
    HGR_REQUIRE((int64_t)B * (gg + 1) < ((int64_t)1 << 31), "hgr_vit_patch_embed_ln: B=%d: %lld rows exceed 32-bit row indices", B, (long long)B * (gg + 1));
    // LDS-DMA addresses its operands with 32-bit byte offsets: the pixels from the tile's own two images, the weight from its base
    HGR_REQUIRE((int64_t)2 * 3 * R * R * 4 < ((int64_t)1 << 31) && (int64_t)PE_W * PE_K * 2 < ((int64_t)1 << 31), "hgr_vit_patch_embed_ln: operand offsets exceed 32 bits");
    HGR_REQUIRE(hgr_aligned(image, 16) && hgr_aligned(conv_w, 16) && hgr_aligned(class_embedding, 16) && hgr_aligned(positional_embedding, 16) &&
                hgr_aligned(gamma, 16) && hgr_aligned(beta, 16) && hgr_aligned(xh, 16) && hgr_aligned(xl, 16) && hgr_aligned(stats, 16),
                "hgr_vit_patch_embed_ln: operands must be 16-byte aligned");
    const dim3 grid((B + 1) / 2), block(PE_NT);
    hgr_by_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((vit_patch_embed_ln<dt.value>), grid, block, 0, (hipStream_t)stream, image, (const char *)conv_w, class_embedding, positional_embedding, gamma, beta, xh, xl, stats, B, R, gs, eps); });
    HGR_CHECK_LAUNCH("hgr_vit_patch_embed_ln");
    return HGR_OK;
}
