// =================================================================================================
// gemm_nt_res_wide: the residual producer (hgr_gemm_nt_res_stats: (xh, xl) += A W^T + bias on the 16-bit-plus-byte pair, + the slot
// statistics of the new rows) on 320 (M) x 256 (N) tiles, ONE 512-thread workgroup per tile and per CU, one round - the K-tile loop
// gemm_nt_p8 runs (pingpong_ktile, hgr_gemm_common.h) with a fifth m tile per wave, and the producer pass of gemm_nt_duo (pair_pass_*).
//
// Why a third form of this product: ViT-B/32's c_proj at batch 512 is 25 600 x 768 x 3 072.  On gemm_nt_duo's 256 x 128 tiles that is
// 600 tiles for 512 workgroup slots - a full round, then a tail of half tiles on a third of the slots (duo_plan, hgr_gemm.hip) - and a
// 256 x 128 tile stages 96 KB per pair of K-tiles and CU, more clocks of L2 -> LDS fill than of MFMA issue.  25 600 / 320 x 768 / 256
// = 240 tiles = one workgroup on 240 of the 256 CUs, every workgroup the same work, no tail; and a 320 x 256 tile stages
// (320 + 256) x 128 B = 72 KB per K-tile for 80 MFMAs per wave: fill / MFMA issue 0.87 (gemm_nt_p8 0.97, gemm_nt_duo 1.42).
//
// 8 waves as 4 (M) x 2 (N); a wave owns 80 x 128 = 5 x 8 MFMA tiles = 160 accumulator registers.  A K-tile (64 deep) is staged as PA
// (the 320 activation rows, 40 KB) and PW0 / PW1 (the weight rows of columns 0-63 / 64-127 of every wave column, 16 KB each); two
// stages of 72 KB.  Per wave and K-tile 9 LDS-DMA instructions (A 5, W0 2, W1 2), every piece refilled for K-tile t + 2 as soon as both
// ping-pong groups have read it:
//     ph1(t): reads A (10 x ds_read_b128), W columns 0-63 (8 x)    issues PW1(t+1) x2               waits vmcnt(9): PW1(t) landed
//     ph2(t): reads W columns 64-127 (8 x), A fragments stay        issues PA(t+2) x5, PW0(t+2) x2   waits vmcnt(9): PA(t+1), PW0(t+1) landed
// (issue order ... PW1(t) | PA(t+1), PW0(t+1) | PW1(t+1) | PA(t+2), PW0(t+2): a count = "my N youngest may still be in flight")
// 40 MFMAs per wave and phase; waves 0-3 and 4-7 (one of each per SIMD) run one barrier interval apart.  Same operand roles and the
// same ascending K walk from a zero accumulator as gemm_nt_duo, hence its accumulator bits.
//
// One instruction of a piece reads 64 piece rows, 8 per wave: instruction i of PA = tile rows 64 i + 8 wave + lane / 8, of PW0 = tile
// columns 128 i + 8 wave + lane / 8 (PW1: + 64) - rows that differ from instruction 0's by a wave-uniform constant, which rides in the
// scalar offset with the K advance.  The buffer descriptors start at the TILE's first row, so a lane keeps two offsets (A, W) in all.
//
// One tile per workgroup, no next-tile request: behind the last K-tile no DMA is in flight, and the epilogue is plain C++ over the
// stage memory.  Its arithmetic is gemm_nt_duo's producer pass, the same functions (pair_pass_*, hgr_gemm_common.h): passes of 16 rows x 64 columns through a
// wave-private LDS slice, a lane then owns 8 consecutive columns of a row (8 lanes per row, 8 rows per instruction), 16-byte accesses
// on xh, 8-byte ones on xl over whole lines, the old pair requested two passes ahead.  A wave's 128 columns are two whole statistic
// slots (n tiles 0-3 and 4-7); inside a slot the values are paired exactly as in gemm_nt_duo, where a wave's 64 columns are one slot.
// =================================================================================================
#include "hgr_gemm_common.h"
#include "hgr_launch.h"

namespace hgr_gemm {
namespace {
constexpr int WD_NT = 512;
constexpr int WD_BM = 320, WD_BN = 256;
constexpr int WD_PA = 0, WD_PW0 = 40960, WD_PW1 = 57344;     // PA 40 K | PW0 16 K | PW1 16 K
constexpr int WD_STAGE = 73728;
constexpr int WD_LDS = 2 * WD_STAGE;                         // 147 456 B
constexpr int WD_RS = 272;                                   // epilogue staging row: 64 fp32 columns + 16 B pad; 8 waves x 16 rows x 272 B = 34 816 B

template <int DT>
__global__ __launch_bounds__(WD_NT) void gemm_nt_res_wide(GemmArgs p) {
    typedef typename T16<DT>::vec8 vec8;
    __shared__ __attribute__((aligned(1024))) char smem[WD_LDS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 2, wm = wave & 3;          // waves w and w + 4 share a SIMD: wn is also the ping-pong group
    const int r = lane & 15, g = lane >> 4;

    // tile id = row tile * tiles_n + column tile; every XCD (blocks b, b + 8, ... share an L2) owns a contiguous range of ids, column
    // tiles fastest: the column tiles of a row panel sit on one L2.  grid = number of tiles.
    const int ntiles = p.tiles_m * p.tiles_n, orig = blockIdx.x;
    const int tile = xcd_first_tile(ntiles, orig & 7) + (orig >> 3);
    if (tile >= ntiles) return;
    const int tm = tile / p.tiles_n;
    const int m0 = tm * WD_BM, n0 = (tile - tm * p.tiles_n) * WD_BN;

    // LDS-DMA sources: descriptors at the tile's first A row / W row, one lane offset per operand (piece row 8 wave + lane / 8, source
    // chunk ^= row & 7: rule 21), the 64-row (A) / 128-row (W) step of an instruction in the scalar offset (host: < 2^31 per tile)
    const char *const At = p.A + (int64_t)m0 * p.lda * 2, *const Wt = p.W + (int64_t)n0 * p.ldw * 2;
    const __amdgpu_buffer_rsrc_t rA = dma_rsrc(At), rW = dma_rsrc(Wt);
    const int pr0 = wave * 8 + (lane >> 3), c0 = (lane & 7) ^ (pr0 & 7);
    const unsigned laneA = (unsigned)(pr0 * (int)p.lda + c0 * 8) * 2u, laneW = (unsigned)(pr0 * (int)p.ldw + c0 * 8) * 2u;
    const int stepA = 64 * (int)p.lda * 2, stepW = 128 * (int)p.ldw * 2, w1off = 64 * (int)p.ldw * 2;
    char *const ldsw = smem + wave * 1024;
    auto issueA = [&](int t) {
        char *dst = ldsw + (t & 1) * WD_STAGE + WD_PA;
#pragma unroll
        for (int i = 0; i < 5; ++i) dma16(rA, laneA, t * 128 + i * stepA, dst + i * 8192);
    };
    auto issueW = [&](int half, int t) {
        char *dst = ldsw + (t & 1) * WD_STAGE + (half ? WD_PW1 : WD_PW0);
#pragma unroll
        for (int i = 0; i < 2; ++i) dma16(rW, laneW, t * 128 + i * stepW + half * w1off, dst + i * 8192);
    };

    const int nk = p.K / 64;    // even, >= 4 (host)
    const int offA = (wm * 80 + r) * 128;          // + m tile (0 .. 4) * 2048 within PA
    const int offW = (wn * 64 + r) * 128;          // + n tile (0 .. 3) * 2048 within PW0 / PW1
    const int sw0 = ((0 + g) ^ (r & 7)) * 16, sw1 = ((4 + g) ^ (r & 7)) * 16;
    vec8 wf[4][2], af[5][2];

    // prologue in steady-state order: PA(0), PW0(0) | PW1(0) | PA(1), PW0(1)
    issueA(0); issueW(0, 0);
    issueW(1, 0);
    issueA(1); issueW(0, 1);
    f32x4 acc[5][8];            // [m tile][n tile]: C[wm*80 + 16 i + r][wn*128 + 16 j + 4 g .. + 3]
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    HGR_RWAIT(9);               // PA(0), PW0(0) landed: my 9 youngest are PW1(0) x2, PA(1) x5, PW0(1) x2
    if (wn) HGR_MBAR();         // ping-pong: group 1 runs one barrier interval behind group 0

    // the shared K-tile (pingpong_ktile, hgr_gemm_common.h) with five m tiles: ph1 issues PW1(t+1), ph2 PA(t+2) and PW0(t+2)
    auto ktile = [&](int t, auto mode_tag) {
        pingpong_ktile<DT, 5, decltype(mode_tag)::value, WD_PA, WD_PW0, WD_PW1>(smem + (t & 1) * WD_STAGE, offA, offW, sw0, sw1, acc, wf, af,
            [&]() { issueW(1, t + 1); }, [&]() { issueA(t + 2); issueW(0, t + 2); });
    };
    for (int t = 0; t < nk - 2; ++t) ktile(t, std::integral_constant<int, 0>());
    ktile(nk - 2, std::integral_constant<int, 1>());
    ktile(nk - 1, std::integral_constant<int, 2>());
    if (!wn) HGR_MBAR();        // group 0 waits for group 1's last interval: every LDS read is done, no DMA in flight

    // ---- epilogue: gemm_nt_duo's residual producer (duo_tile, LN == 1), 10 passes of 16 rows x 64 columns per wave ----
    // (opaque copy: every lane-derived term of the epilogue is computed here instead of being kept live across the main loop)
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int le = tid_e & 63, re = le & 15, ge = le >> 4;
    const int r8e = le >> 3, c8 = le & 7;
    char *my = smem + wave * (16 * WD_RS);
    const int64_t wrow = m0 + wm * 80;
    const unsigned ldxB = (unsigned)p.ln_ldx * 2u, ldsB = (unsigned)p.ln_slots * 8u, ldlB = (unsigned)p.ln_ldx;
    const unsigned xo = r8e * ldxB + c8 * 16, so = r8e * ldsB, lo8 = r8e * ldlB + c8 * 8;
    constexpr int NP = 10;      // pass ps: column half ps / 5 (one statistic slot), m tile ps % 5
    // bases of column half h: + 64 columns = 128 B of xh, 64 B of xl, one slot (8 B) of stats, 256 B of bias
    char *const hw0 = (char *)p.ln_xh + (wrow * p.ln_ldx + n0 + wn * 128) * 2;
    char *const lw0 = (char *)p.ln_xl + (wrow * p.ln_ldx + n0 + wn * 128);
    char *const sw = (char *)(p.ln_stats + (wrow * p.ln_slots + ((n0 + wn * 128) >> 6)) * 2);
    const float *const bw = p.bias + n0 + wn * 128 + c8 * 8;
    u32x4 ohb[3][2];
    u32x2 olb[3][2];
    auto pair_load = [&](int buf, int ps) {
        const int h = ps / 5, rl = (ps % 5) * 16;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ohb[buf][q] = *(const u32x4 *)(hw0 + h * 128 + (xo + (rl + q * 8) * ldxB));
            olb[buf][q] = *(const u32x2 *)(lw0 + h * 64 + (lo8 + (rl + q * 8) * ldlB));
        }
    };
    pair_load(0, 0);        // (pass 1's request waits for pass 0's accumulators to leave their registers: all 160 are live here)
    unsigned gbits = 0u;                              // range guard: largest slot sum of squares seen (as bits: inf / NaN rank highest)
    f32x4 b8lo = (f32x4){0.f, 0.f, 0.f, 0.f}, b8hi = b8lo;
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        const int h = ps / 5, i = ps % 5;
        const int rl = i * 16;
        const int pb = ps % 3;
        // the bias of this lane's 8 output columns of the half, added behind the LDS transpose
        if (i == 0) { b8lo = *(const f32x4 *)(bw + h * 64); b8hi = *(const f32x4 *)(bw + h * 64 + 4); }
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4 *)(my + re * WD_RS + (j * 16 + ge * 4) * 4) = acc[i][h * 4 + j];
        __builtin_amdgcn_sched_barrier(0);           // the requests below stay behind the writes that free the pass's 16 accumulator registers
        // the old pair two passes ahead (a ring of three 12-register buffers), one pass ahead while most accumulators are still live
        if (ps == 0) pair_load(1, 1);
        if (ps == 1) pair_load(2, 2);
        if (ps >= 1 && ps + 2 < NP) pair_load((ps + 2) % 3, ps + 2);
        float s1[2], s2[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 lo4 = *(const f32x4 *)(my + (q * 8 + r8e) * WD_RS + c8 * 32);
            const f32x4 hi4 = *(const f32x4 *)(my + (q * 8 + r8e) * WD_RS + c8 * 32 + 16);
            const vec8 oh = __builtin_bit_cast(vec8, ohb[pb][q]);
            const u32x2 ol = olb[pb][q];
            float v[8];
            pair_pass_values<DT>(lo4, hi4, b8lo, b8hi, oh, ol, v);
            u32x4 nh;
            u32x2 nl;
            pair_pass_split<DT>(v, nh, nl);
            *(u32x4 *)(hw0 + h * 128 + (xo + (rl + q * 8) * ldxB)) = nh;
            *(u32x2 *)(lw0 + h * 64 + (lo8 + (rl + q * 8) * ldlB)) = nl;
            pair_pass_sums(v, s1[q], s2[q]);
        }
        pair_pass_reduce(s1, s2);
        if (c8 == 0) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                *(float2 *)(sw + h * 8 + (so + (rl + q * 8) * ldsB)) = make_float2(s1[q], s2[q]);
                gbits = max(gbits, __float_as_uint(s2[q]));
            }
        }
    }
    if (p.ln_flag && gbits > __float_as_uint(p.ln_guard)) atomicMax(p.ln_flag, gbits);
}

// the shape contract of hgr_gemm_nt_res_stats_wide, message of the first rule broken (nullptr = covered)
const char *wide_reject(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldx, int dtype) {
    if (dtype != HGR_BF16 && dtype != HGR_F16) return "bad dtype";
    if (M < WD_BM || M % WD_BM || N < WD_BN || N % WD_BN || N >= (1 << 20)) return "M must be a multiple of 320, N a multiple of 256 below 2^20";
    if (K < 256 || K % 128) return "K must be a multiple of 128, at least 256 (an even number >= 4 of K-tiles)";
    if ((M / WD_BM) * (N / WD_BN) > hgr_cu_count()) return "more tiles than compute units (one workgroup per tile, one round)";
    // a tile's rows are addressed at 32-bit byte offsets from the tile's first row: 320 * lda * 2 and 256 * ldw * 2 stay below 2^31
    if (lda < K || ldw < K || lda % 8 || ldw % 8 || lda >= (1 << 21) || ldw >= (1 << 21)) return "lda / ldw must be >= K, multiples of 8 and < 2^21";
    if (ldx < N || ldx % 8 || ldx >= (1 << 23)) return "ldx must be >= N, a multiple of 8 and < 2^23";
    if (M * lda * 2 >= (1ll << 32) || N * ldw * 2 >= (1ll << 32) || M * ldx * 2 >= (1ll << 32)) return "operands beyond 4 GB";
    return nullptr;
}
}  // namespace
}  // namespace hgr_gemm

using namespace hgr_gemm;

extern "C" int hgr_gemm_nt_res_stats_wide_ok(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldx, int dtype) {
    return wide_reject(M, N, K, lda, ldw, ldx, dtype) == nullptr ? 1 : 0;
}

extern "C" int hgr_gemm_nt_res_stats_wide(const void *A, int64_t lda, const void *W, int64_t ldw, void *xh, void *xl, int64_t ldx,
                                          const float *bias, float *stats, float guard_sumsq, uint32_t *flag,
                                          int M, int N, int K, int dtype, void *stream) {
    const char *why = wide_reject(M, N, K, lda, ldw, ldx, dtype);
    HGR_REQUIRE(!why, "hgr_gemm_nt_res_stats_wide: M=%d N=%d K=%d lda=%lld ldw=%lld ldx=%lld dtype=%d: %s", M, N, K, (long long)lda, (long long)ldw, (long long)ldx, dtype, why);
    HGR_REQUIRE(A && W && xh && xl && bias && stats, "hgr_gemm_nt_res_stats_wide: null operand");
    HGR_REQUIRE(!flag || (guard_sumsq > 0.f && hgr_aligned(flag, 4)), "hgr_gemm_nt_res_stats_wide: flag needs guard_sumsq > 0 and 4-byte alignment");
    HGR_REQUIRE(hgr_aligned(A, 16) && hgr_aligned(W, 16) && hgr_aligned(xh, 16) && hgr_aligned(xl, 16) && hgr_aligned(bias, 16) && hgr_aligned(stats, 8),
                "hgr_gemm_nt_res_stats_wide: A, W, xh, xl and bias must be 16-byte, stats 8-byte aligned");
    GemmArgs a = gemm_args(A, lda, W, ldw, nullptr, 0, M, N, K, true, 0);
    a.bias = bias;
    a.ln_stats = stats; a.ln_slots = N / 64; a.ln_xh = xh; a.ln_xl = xl; a.ln_ldx = ldx;
    a.ln_flag = flag; a.ln_guard = guard_sumsq;
    a.tiles_m = M / WD_BM; a.tiles_n = N / WD_BN;
    const dim3 grid((unsigned)(a.tiles_m * a.tiles_n)), block(WD_NT);
    hgr_by_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL((gemm_nt_res_wide<dt.value>), grid, block, 0, (hipStream_t)stream, a); });
    HGR_CHECK_LAUNCH("hgr_gemm_nt_res_stats_wide");
    return HGR_OK;
}
