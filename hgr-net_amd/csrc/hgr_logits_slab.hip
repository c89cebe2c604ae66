// =================================================================================================
// First stage of hgr_logits_eval: logits = feat . zsl_perm^T (model/clip_tree.py:331) with the evaluation consumers of main.test
// (main.py:136-176) in the epilogue - nothing [B, N] is written.
//
// north_star asks >= 40 % of the MFMA peak of this product ([512 x 512] . [512 x 21 841]: 11.45 GFLOP = 11.5 us).  Rounds 2 / 3 ran
// it on gemm_nt_duo's 128 x 128 half tiles: 712 workgroups on 512 slots, every one a prologue + 8 K-tiles + an epilogue with nothing
// to overlap - 29.9 us.  This kernel gives every CU ONE tile of the whole batch:
//
//   tile = 512 rows (the batch) x 96 columns x K;  grid = N' / 96 slabs (230 at N = 21 841: one round on 256 CUs, every CU the same
//   work) x ceil(rows / 512);  512 threads = 8 waves, wave w owns rows 64 w .. 64 w + 63 x all 96 columns = 4 x 6 MFMA tiles.
//
// The class matrix streams through each CU exactly once (96 rows x 2 D bytes per CU, 22 MB chip-wide from HBM); the 512 x D feature
// matrix (written microseconds earlier by l2norm_rows) is re-read by every CU out of its XCD's L2.  Staging and main loop are those
// of hgr_gemm_nt_ln_mha (hgr_qkv_attn.hip): LDS-DMA pieces cut by the phase that reads them - PA0 (rows 0-31 of every wave, 32 KB),
// PW (the 96 class rows, padded to 16 KB), PA1 (rows 32-63, 32 KB) - two stages of 80 KB = the CU's whole LDS, counted vmcnt(10)
// waits, one barrier per interval, waves 0-3 / 4-7 one interval apart (ping-pong):
//     ph1(t): issues PA1(t+1) x4               reads W (12 x ds_read_b128), A rows 0-31 (4 x)    24 MFMAs
//     ph2(t): issues PA0(t+2) x4, PW(t+2) x2   reads A rows 32-63 (4 x)                           24 MFMAs
//
// Epilogue: the class matrix is LEVEL-SORTED and level-aligned to 32 columns (ops.LogitsEvalPlan), so every 32-column slice - two of
// a lane's n tiles - lies inside one hierarchy level.  Per (row, slice): the best train column as an orderable 64-bit key
// (value, then smaller train position - the tie rule of logits[:, train_index].topk); per 16-column group the largest test value, the
// test position of an element attaining it and the second largest value.  96 bytes per (row, slab), written as ONE 8-byte store per
// lane and slice (lane group g = 0 .. 3 writes key / maxima / positions / second values) into the slab's own contiguous block.  hgr_logits_eval's row stage (hgr_select.hip) turns
// them into the level arg-max, the top-1 and the top-k.
// =================================================================================================
#include "hgr_gemm_common.h"
#include "hgr_launch.h"

namespace hgr_gemm {

namespace {
constexpr int LS_NT = 512;
constexpr int LS_PA0 = 0, LS_PA1 = 32768, LS_PW = 65536, LS_STAGE = 81920, LS_LDS = 2 * LS_STAGE;     // 163 840 B: all of the CU's LDS

template <int DT>
__global__ __launch_bounds__(LS_NT) void logits_slab(SlabArgs p) {
    typedef typename T16<DT>::vec8 vec8;
    __shared__ __attribute__((aligned(1024))) char smem[LS_LDS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = wave >> 2;                      // waves w and w + 4 share a SIMD: the ping-pong group
    const int r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 96, m0 = blockIdx.y * 512;

    // per-lane source offsets of one K-tile's LDS-DMA instructions (bytes from A / W; operands < 4 GB, checked on the host)
    unsigned oA0[4], oA1[4], oW[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = (i * 8 + wave) * 64 + lane;
        const int pr = id >> 3, c = (id & 7) ^ (pr & 7);
        const int tr = (pr >> 5) * 64 + (pr & 31);              // PA0 piece row pr = rows 0-31 of wave pr / 32
        oA0[i] = (unsigned)(((int64_t)min(m0 + tr, p.M - 1) * p.lda + c * 8) * 2);
        oA1[i] = (unsigned)(((int64_t)min(m0 + tr + 32, p.M - 1) * p.lda + c * 8) * 2);
        if (i < 2) oW[i] = (unsigned)(((int64_t)(n0 + min(pr, 95)) * p.ldw + c * 8) * 2);      // piece rows 96-127: padding (row 95 again)
    }
    // The class rows of this slab come from HBM, 12 KB per K-tile, and the pipeline below requests a piece ~1.5 K-tiles (~1 us) before it
    // is read - less than a loaded HBM round trip, so every K-tile would wait for memory (first version: 26 us per launch, slower than
    // the tiled GEMM it replaces).  The whole slab is only 96 x 2 K bytes: touch every 64-byte sector of it ONCE, up front, with plain
    // loads whose values are never looked at before the kernel's last instruction - one HBM latency for the slab, after which every
    // LDS-DMA of it is an L2 hit.  Likewise this workgroup's share of the feature matrix (every XCD's L2 fetches it once from the
    // Infinity Cache; the 29 - 32 workgroups of an XCD - blocks b, b + 8, ... - touch a 1 / 32 share each).
    // (unconditional loads into separate registers, ids clamped: a load under a branch or feeding a running sum is waited for at once)
    unsigned tw[6], ta;
    {
        const int spr = p.K >> 5;                               // 64-byte sectors per row (K <= 1024: at most 6 touches of W per thread)
        const int nw = 96 * spr;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int id = min(tid + u * LS_NT, nw - 1);
            tw[u] = HGR_LAB_ON(p.dbg & 16) ? 0u : *(const unsigned *)(p.W + ((int64_t)(n0 + id / spr) * p.ldw) * 2 + (id % spr) * 64);
        }
        const int rows_here = min(512, p.M - m0), na = rows_here * spr;
        const int id = min((int)(blockIdx.x >> 3) * LS_NT + tid, na - 1);
        ta = *(const unsigned *)(p.A + ((int64_t)(m0 + id / spr) * p.lda) * 2 + (id % spr) * 64);
    }
    char *const ldsw = smem + wave * 1024;
    const __amdgpu_buffer_rsrc_t rA = dma_rsrc(p.A), rW = dma_rsrc(p.W);
    auto issueA = [&](const unsigned (&off)[4], int piece, int t) {
        if (HGR_LAB_ON(p.dbg & 2)) return;
        char *dst = ldsw + (t & 1) * LS_STAGE + piece;
#pragma unroll
        for (int i = 0; i < 4; ++i) dma16(rA, off[i], t * 128, dst + i * 8192);
    };
    auto issueW = [&](int t) {
        if (HGR_LAB_ON(p.dbg & 4)) return;
        char *dst = ldsw + (t & 1) * LS_STAGE + LS_PW;
#pragma unroll
        for (int i = 0; i < 2; ++i) dma16(rW, oW[i], t * 128, dst + i * 8192);
    };

    f32x4 acc[4][6];            // [m tile][n tile]: logits[m0 + 64 wave + 16 i + r][n0 + 16 j + 4 g .. + 3]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / 64;    // >= 2 (host guarantees)
    const int offA = (wave * 32 + r) * 128;        // + m tile (0, 1) * 2048 within PA0 / PA1
    const int offW = r * 128;                      // + n tile * 2048 within PW
    const int sw0 = ((0 + g) ^ (r & 7)) * 16, sw1 = ((4 + g) ^ (r & 7)) * 16;
    vec8 wf[6][2], af[2][2];

    // prologue in steady-state order: PA0(0), PW(0) | PA1(0) | PA0(1), PW(1)
    issueA(oA0, LS_PA0, 0); issueW(0);
    issueA(oA1, LS_PA1, 0);
    issueA(oA0, LS_PA0, 1); issueW(1);
    HGR_RWAIT(10);              // PA0(0), PW(0) landed
    if (pg) HGR_MBAR();         // ping-pong: group 1 runs one barrier interval behind group 0

    // MODE 0: steady state (t + 2 < nk), 1: second-last K-tile, 2: last K-tile
    auto ktile = [&](int t, auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
        const char *st = smem + (t & 1) * LS_STAGE;
        // ---- ph1: rows 0-31 of the wave x all 96 columns ----
        if (MODE <= 1) issueA(oA1, LS_PA1, t + 1);              // its slot was last read in ph2(t - 1), two barriers ago
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            wf[j][0] = *(const vec8 *)(st + LS_PW + offW + j * 2048 + sw0);
            wf[j][1] = *(const vec8 *)(st + LS_PW + offW + j * 2048 + sw1);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            af[i][0] = *(const vec8 *)(st + LS_PA0 + offA + i * 2048 + sw0);
            af[i][1] = *(const vec8 *)(st + LS_PA0 + offA + i * 2048 + sw1);
        }
        if (MODE <= 1) HGR_RWAIT(10); else HGR_RWAIT(0);        // PA1(t) landed
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) if (!HGR_LAB_ON(p.dbg & 1)) acc[i][j] = T16<DT>::mfma16(wf[j][kk], af[i][kk], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
        HGR_MBAR();
        // ---- ph2: rows 32-63 ----
        if (MODE == 0) { issueA(oA0, LS_PA0, t + 2); issueW(t + 2); }     // read in ph1(t), two barriers ago
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            af[i][0] = *(const vec8 *)(st + LS_PA1 + offA + i * 2048 + sw0);
            af[i][1] = *(const vec8 *)(st + LS_PA1 + offA + i * 2048 + sw1);
        }
        if (MODE == 0) HGR_RWAIT(10); else if (MODE == 1) HGR_RWAIT(4); else HGR_RBAR();     // PA0(t+1), PW(t+1) landed
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) if (!HGR_LAB_ON(p.dbg & 1)) acc[2 + i][j] = T16<DT>::mfma16(wf[j][kk], af[i][kk], acc[2 + i][j]);
        __builtin_amdgcn_s_setprio(0);
        HGR_MBAR();
    };
    for (int t = 0; t < nk - 2; ++t) ktile(t, std::integral_constant<int, 0>());
    ktile(nk - 2, std::integral_constant<int, 1>());
    ktile(nk - 1, std::integral_constant<int, 2>());
    if (!pg) HGR_MBAR();        // (barrier counts of the two groups balanced; nothing below touches LDS)

    if (HGR_LAB_ON(p.dbg & 8)) { if (acc[0][0][0] == 123.456f && acc[3][5][3] == 1.f) p.ev_key[0] = 1ull; return; }
    // ---- evaluation consumers.  Lane (r, g) holds, of row m = m0 + 64 wave + 16 i + r, the columns n0 + 16 j + 4 g + e (e = 0..3)
    // of n tile j; a 32-column slice = n tiles 2 s, 2 s + 1, the other 3/4 of its columns sit in the lanes r + 16, r + 32, r + 48 ----
    int tp[6][4], ep[6][4];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int n = n0 + j * 16 + g * 4;
        const int4 t4 = *(const int4 *)(p.tpos + n), e4 = *(const int4 *)(p.epos + n);
        tp[j][0] = t4.x; tp[j][1] = t4.y; tp[j][2] = t4.z; tp[j][3] = t4.w;
        ep[j][0] = e4.x; ep[j][1] = e4.y; ep[j][2] = e4.z; ep[j][3] = e4.w;
    }
    // records of this slab: [row][96 bytes] = keys of the 3 slices | (m1, m1') x 3 | (p1, p1') x 3 | (m2, m2') x 3, contiguous per
    // workgroup (48 KB: whole lines from one CU; the first version wrote [row][slice] arrays, i.e. 8-byte pieces of lines shared by
    // CUs of different XCDs).  Lane group g writes the g-th 24-byte part.
    char *const rec = (char *)p.ev_key + (int64_t)blockIdx.x * p.M * 96 + g * 24;
    // Cross-lane steps: the four lane groups g = lane >> 4 of a row meet through v_permlane16_swap / v_permlane32_swap (gfx950: VALU, no
    // LDS crossbar).  swap(x, x) returns (a, b) = for the lane pair (L, L ^ 16) [resp. ^ 32] the even row's and the odd row's value, the
    // SAME pair in both lanes, so max(a, b) etc. leave both lanes with the same result.  (First version: 64-bit keys per element and 16
    // __shfl_xor = ds_bpermute per (row, slice): the epilogue took 13 of the launch's 26 us.)
#define LS_SWAP16(x) __builtin_amdgcn_permlane16_swap((unsigned)(x), (unsigned)(x), false, false)
#define LS_SWAP32(x) __builtin_amdgcn_permlane32_swap((unsigned)(x), (unsigned)(x), false, false)
    auto xmaxf = [&](float v) {
        auto a = LS_SWAP16(__float_as_uint(v));
        v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
        auto b = LS_SWAP32(__float_as_uint(v));
        return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
    };
    auto xmini = [&](int v) {
        auto a = LS_SWAP16(v);
        v = min((int)a[0], (int)a[1]);
        auto b = LS_SWAP32(v);
        return min((int)b[0], (int)b[1]);
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wave * 64 + i * 16 + r;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            float m1[2], m2[2];
            int p1[2];
            // ---- train columns of the slice: value first, position second (ties in the value: the smaller train position) ----
            float tv[2][4];
            float V = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tv[jj][e] = tp[2 * s + jj][e] >= 0 ? acc[i][2 * s + jj][e] + 0.0f : -INFINITY;    // -0 -> +0, as the row sweep of hgr_eval_rows does
                    V = fmaxf(V, tv[jj][e]);
                }
            V = xmaxf(V);
            int P = 0x7fffffff;
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) P = min(P, (tp[2 * s + jj][e] >= 0 && tv[jj][e] == V) ? tp[2 * s + jj][e] : 0x7fffffff);
            P = xmini(P);
            // (no train column in the slice: P stays INT_MAX -> key 0, which loses against every real key)
            const unsigned long long vkey = key_of(V, P);                   // formed ahead of the select, as the kernel always did: same code
            const unsigned long long key = P == 0x7fffffff ? 0ull : vkey;
            // ---- test columns: per 16-column group the largest value, the position of an element attaining it, the runner-up ----
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = 2 * s + jj;
                float x[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = ep[j][e] >= 0 ? acc[i][j][e] + 0.0f : -INFINITY;
                const float hi01 = fmaxf(x[0], x[1]), lo01 = fminf(x[0], x[1]), hi23 = fmaxf(x[2], x[3]), lo23 = fminf(x[2], x[3]);
                float t1 = fmaxf(hi01, hi23);
                float t2 = fmaxf(fminf(hi01, hi23), fmaxf(lo01, lo23));
                int q1 = x[0] == t1 ? ep[j][0] : x[1] == t1 ? ep[j][1] : x[2] == t1 ? ep[j][2] : ep[j][3];
                {
                    auto a1 = LS_SWAP16(__float_as_uint(t1)); auto a2 = LS_SWAP16(__float_as_uint(t2)); auto ap = LS_SWAP16(q1);
                    const float e1 = __uint_as_float(a1[0]), o1 = __uint_as_float(a1[1]);
                    t2 = fmaxf(fminf(e1, o1), fmaxf(__uint_as_float(a2[0]), __uint_as_float(a2[1])));
                    q1 = o1 > e1 ? (int)ap[1] : (int)ap[0];
                    t1 = fmaxf(e1, o1);
                }
                {
                    auto a1 = LS_SWAP32(__float_as_uint(t1)); auto a2 = LS_SWAP32(__float_as_uint(t2)); auto ap = LS_SWAP32(q1);
                    const float e1 = __uint_as_float(a1[0]), o1 = __uint_as_float(a1[1]);
                    t2 = fmaxf(fminf(e1, o1), fmaxf(__uint_as_float(a2[0]), __uint_as_float(a2[1])));
                    q1 = o1 > e1 ? (int)ap[1] : (int)ap[0];
                    t1 = fmaxf(e1, o1);
                }
                m1[jj] = t1; m2[jj] = t2; p1[jj] = q1;
            }
            // (the warm-up loads' values are consumed here, at the very end; the extra condition never holds)
            if (m < p.M || ((tw[0] ^ tw[1] ^ tw[2]) + (tw[3] ^ tw[4] ^ tw[5]) + ta == 0x9E3779B9u && m == 0x7fffffff)) {
                const unsigned long long v8 = g == 0 ? key
                    : g == 1 ? ((unsigned long long)__float_as_uint(m1[1]) << 32) | __float_as_uint(m1[0])
                    : g == 2 ? ((unsigned long long)(unsigned)p1[1] << 32) | (unsigned)p1[0]
                             : ((unsigned long long)__float_as_uint(m2[1]) << 32) | __float_as_uint(m2[0]);
                *(unsigned long long *)(rec + (int64_t)m * 96 + s * 8) = v8;
            }
        }
    }
#undef LS_SWAP16
#undef LS_SWAP32
}
}  // namespace

void launch_logits_slab(const SlabArgs &a, int dtype, hipStream_t s) {
    const dim3 grid((unsigned)(a.Np / 96), (unsigned)((a.M + 511) / 512)), block(LS_NT);
    hgr_by_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((logits_slab<dt.value>), grid, block, 0, s, a); });
}

}  // namespace hgr_gemm
