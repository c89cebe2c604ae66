// Host entry points of the NT GEMM family (kernels: hgr_gemm_128 / _256 / _duo / _p8 .hip, hgr_conv_direct.hip).  Every entry point is
// validate -> plan -> launch: the plan functions below are plain host code that decide kernel, tile plan and grid (GemmLaunch) and launch
// nothing; gemm_run() hands a plan to the launchers, which only select a template instantiation - or, when hgr_gemm_plan_capture armed
// the calling thread, writes it out instead (tests/golden/gemm_plans.json pins the plan of every route on a machine without a GPU).
#include "hgr_gemm_common.h"

using namespace hgr_gemm;

int hgr_conv3x3_c32_launch(const void *x, const void *w, const float *bias, void *out, int B, int H, int W, int Cout, int Kp,
                           int dtype, int relu, void *stream, int pool, int C);      // hgr_conv_direct.hip

namespace {
constexpr int BM = 128, BN = 128;

// ---- development knobs (HgrKnob, hgr_common.h: the environment gives the initial value, the hgr_gemm_set_* setters win from then on) ----
HgrKnob<> k_group{"HGR_GEMM_GROUP", 0, [](int v) { return v < 0 ? 0 : v; }};      // raster group of gemm_nt_duo; 0 = by shape (duo_group_for)
HgrKnob<> k_tail{"HGR_DUO_TAIL", 1}, k_pb{"HGR_DUO_PB", -1};                       // hgr_gemm_set_tail: tail plan on / off, forced full panels
HgrKnob<double> k_half_cost{"HGR_DUO_HALF_COST", 0.55, [](double v) { return v > 0.1 ? v : 0.55; }};
HgrKnob<> k_tile{"HGR_GEMM_TILE", 0};                                              // hgr_gemm_set_tile: 0 | 128 | 256 | 2
HgrKnob<> k_split{"HGR_GEMM_SPLIT", 1};                                            // the two-launch split plan of hgr_gemm_nt
HgrKnob<> k_conv_direct{"HGR_CONV_DIRECT", 1}, k_conv_duo{"HGR_CONV_DUO", 1};      // 0 keeps the implicit GEMM / the 128 and 256 kernels
// Persistent form of the residual producers.  Default: at most two workgroups per CU, each walking its share of the tiles (see gemm_nt_duo);
// HGR_DUO_PERSIST=0 = one workgroup per tile (A/B runs).  Measured on the ViT-B/32 evaluation step, interleaved pairs on one box: every
// launch persistent 5.064 -> 5.008 ms (-1.1 %; by shape proj 128.6 -> 123.5 us, out 50.1 -> 48.5, fc unchanged), the producers only
// 5.137 -> 5.104 (-0.6 %).  Bit-identical.
HgrKnob<> k_persist{"HGR_DUO_PERSIST", 1, hgr_knob_bool};                          // hgr_gemm_set_persist
HgrKnob<> k_p8{"HGR_P8", 2, [](int v) { return v >= 0 && v <= 2 ? v : 2; }};       // hgr_gemm_set_p8: 0 never, 1 wherever p8_covers, 2 by shape (p8_wanted)

int duo_group() { return k_group.get() ? k_group.get() : 4; }          // m-fastest rasters of gemm_nt_duo, and the group field of a gemm_nt_p8 plan
// Row panels per raster group of a gemm_nt_duo launch (plan_duo).  By shape unless HGR_GEMM_GROUP=n forces n: 4 (64 tiles in flight per
// XCD = 4 row panels x 16 column panels), but ONE for launches of at most 8 column panels - the few tiles that share an activation
// panel are then dispatched back to back instead of 4 slots apart.  Measured (tools/raster_split_ab.sh, FETCH_SIZE per launch, ViT-B/32
// step): the N = 768 producers 250 -> 222 MB (group 2: 232, 8: 280), patch GEMM 345 -> < 300; c_fc (24 column panels) 207 MB at 4,
// 241 / 270 at 2 / 1, 219 at 8.  Step times of all three BASELINE configurations unchanged (tools/group_ab.sh: 4.953 vs 4.949 ms,
// 10.08 vs 10.09 ms, 224.1 vs 224.8 ms): this trims fabric traffic, not time.
int duo_group_for(int tiles_n) { return k_group.get() ? k_group.get() : (tiles_n <= 8 ? 1 : 4); }
int duo_dbg() {
    static const int d = hgr_lab_env("HGR_GEMM_DBG");    // lab builds only (hgr_common.h): 0 in libhgr.so; bit 8: sc1 output stores
    return d;
}

// One launch as the plan step decides it: which kernel and instantiation, the grid, the plan fields of GemmArgs and the rows of the
// call it covers (hgr_gemm_nt's split plan makes two launches over disjoint row ranges)
struct GemmLaunch {
    int kernel = 0;               // HGR_KERNEL_* (hgr.h); 0 = no launch
    int variant = 0;              // V128_* | conv of gemm_nt_256 | ln form of gemm_nt_duo | input channels of the direct convolution
    int epilogue = HGR_EPI_NONE; bool out32 = false;
    int act = 0;                  // gemm_nt_p8: 0 none, 1 QuickGELU
    unsigned grid_x = 0, grid_y = 1;
    int tiles_m = 0, tiles_n = 0, total = 0, nbig = 0, big_panels = 0, tiles_m_half = 0, group = 0;      // -> GemmArgs
    int row0 = 0, rows = 0;
};

// gemm_nt_128 / gemm_nt_256 on TM x TN tiles, one per workgroup
GemmLaunch plan_tiles(int kernel, int variant, int epi, bool out32, int M, int N, int TM, int TN, unsigned grid_y = 1) {
    GemmLaunch L;
    L.kernel = kernel; L.variant = variant; L.epilogue = epi; L.out32 = out32; L.rows = M;
    L.tiles_m = (M + TM - 1) / TM; L.tiles_n = (N + TN - 1) / TN;
    L.grid_x = (unsigned)(L.tiles_m * L.tiles_n); L.grid_y = grid_y;
    return L;
}

// Tail plan of gemm_nt_duo.  The chip runs 512 of its workgroups at a time (2 per CU); a launch of T > 512 full tiles that is not
// a whole number of rounds ends in a partly empty round: the N = 768 residual producers of ViT-B/32 at batch 512 (600 tiles) spent
// 25 - 29 % of their time with 88 workgroups on the chip (tools/round_staircase.py).  The plan gives the LAST row panels to half
// tiles (128 x 128, dispatched after the full tiles): work of half the size fills the slots the full tiles free first.  Chosen by
// list-scheduling the two tile kinds on 512 slots (a half tile priced at HGR_DUO_HALF_COST = 0.55 of a full one: half the MFMAs, the
// same per-tile overhead) over the candidate panel counts; HGR_DUO_TAIL=0 switches it off, HGR_DUO_PB=n forces n full panels.
struct DuoPlan { int big_panels, nbig, tiles_m_half, grid; };
DuoPlan duo_plan(int M, int N) {
    const int tail = k_tail.get(), pb_forced = k_pb.get();
    const double half_cost = k_half_cost.get();
    const int tiles_m = (M + 255) / 256, tiles_n = (N + 127) / 128, S = 512;
    const int64_t T = (int64_t)tiles_m * tiles_n;
    DuoPlan best{tiles_m, (int)T, 0, (int)T};
    if (tail && pb_forced < 0 && M > 128 && (T <= S / 4 || (tiles_m <= 2 && T <= S))) {
        // a launch that covers a fraction of the chip (the class-token GEMMs of a ViT's last block: 512 rows) is bound by what ONE
        // workgroup can pull per K-tile, not by the matrix cores: all half tiles = twice the workgroups, 2/3 of the bytes per K-tile each.
        // Likewise at most two row panels on fewer tiles than slots (the class-logits GEMM and hgr_logits_eval at batch 512: 356
        // full tiles on 256 CUs -> 712 half tiles; measured 48.0 -> 46.2 us fused, 21.6 -> 21.0 us plain, bit-identical)
        best.big_panels = 0; best.nbig = 0; best.tiles_m_half = (M + 127) / 128; best.grid = best.tiles_m_half * tiles_n;
        return best;
    }
    if (!tail || T <= S || T % S == 0) return best;
    // measured (tools/tail_sweep.py, ViT-B/32 tower launches at batch 512, cold operands): last round 15 - 17 % full (out, proj, patch:
    // 600 / 588 tiles) -13 %, -14.5 %, -11 %; last round 52 % full (qkv, 1800 tiles) +-0; 69 % full (fc, 2400 tiles) +2 %: a
    // half-full last round already overlaps well, and half tiles stage fewer flops per byte
    if (pb_forced < 0 && (T % S) * 100 > 45 * (int64_t)S) return best;
    auto makespan = [&](int pb) {
        const int64_t nb = (int64_t)pb * tiles_n;
        const int mh = M - pb * 256;
        int64_t nh = mh > 0 ? (int64_t)((mh + 127) / 128) * tiles_n : 0;
        const int64_t q = nb / S, rem = nb % S;
        double tE = (double)q, tL = (double)q + 1.0;         // S - rem slots are free at q, rem slots at q + 1
        int64_t nE = S - rem, nL = rem;
        double end = rem ? tL : tE;
        if (!nb) end = 0.0;
        while (nh > 0) {
            const bool useE = nE > 0 && (nL == 0 || tE <= tL);
            double &t = useE ? tE : tL;
            const int64_t k = useE ? nE : nL;
            t += half_cost;
            if (t > end) end = t;
            nh -= k;
        }
        return end;
    };
    int pick = tiles_m;
    double bm = makespan(tiles_m);
    if (pb_forced >= 0) pick = pb_forced < tiles_m ? pb_forced : tiles_m;
    else
        for (int pb = tiles_m - 1; pb >= 0 && pb >= tiles_m - 96; --pb) {
            const double m = makespan(pb);
            // (forced panel counts, tools/producer_ab.py with warm clocks and interleaved arms, out_proj K = 768 / c_proj K = 3072 of
            // ViT-B/32 at batch 512, us: no tail 61.7 / 150.0, 85 full panels - this loop's pick - 55.7 / 132.6, 70: 57.6 / 141.4,
            // 55: 57.4 / 142.5: more half tiles than the last round needs cost time even on the epilogue-bound K = 768 launch)
            if (m < bm - 1e-9) { bm = m; pick = pb; }
        }
    if (pick == tiles_m) return best;
    const int mh = M - pick * 256;
    best.big_panels = pick; best.nbig = pick * tiles_n; best.tiles_m_half = (mh + 127) / 128;
    best.grid = best.nbig + best.tiles_m_half * tiles_n;
    return best;
}

// gemm_nt_duo: 256 x 128 tiles with the tail plan, raster group by shape; ln = the form (launch_duo)
GemmLaunch plan_duo(const GemmArgs &a, int ln, int epi, bool out32) {
    GemmLaunch L;
    L.kernel = HGR_KERNEL_DUO; L.variant = ln; L.epilogue = epi; L.out32 = out32; L.rows = a.M;
    L.tiles_m = (a.M + 255) / 256; L.tiles_n = (a.N + 127) / 128;
    const DuoPlan pl = duo_plan(a.M, a.N);
    L.nbig = pl.nbig; L.big_panels = pl.big_panels; L.tiles_m_half = pl.tiles_m_half;
    L.group = a.m_fastest ? duo_group() : duo_group_for(L.tiles_n);
    if (duo_dbg() & 64) fprintf(stderr, "[duo_plan] M=%d N=%d K=%d -> %d full panels (%d tiles) + %d half panels, grid %d\n",
                                     a.M, a.N, a.K, pl.big_panels, pl.nbig, pl.tiles_m_half, pl.grid);
    L.grid_x = (unsigned)pl.grid;
    // The persistent form (k_persist) for the residual producers (ln == 1, the only instantiations compiled with the tile loop) on launches
    // of up to two rounds of the chip's slots - the launches that gain (their epilogue's read-modify-write drains beside the next tile's
    // first operand loads).  Launches of many rounds LOSE with the static deal (ViT-L/14 training step 221.2 -> 223.6 ms, RN50 step
    // 9.58 -> 9.66 ms with every launch persistent): the dispatcher's first-free-slot order balances the slots' drifting speeds, the
    // fixed stride does not; the consumer / plain launches of one to two rounds measured neutral to slightly negative (RN50 9.97 -> 10.03 ms).
    int slots = 2 * hgr_cu_count() & ~7;         // whole multiples of the 8 XCDs: virtual block v and physical block v % grid sit on the same XCD
    if (slots < 8) slots = 8;
    if (k_persist.get() && ln == 1 && pl.grid > slots && pl.grid <= 2 * slots) { L.total = pl.grid; L.grid_x = (unsigned)slots; }
    return L;
}

// gemm_nt_p8: whole 256 x 256 tiles (p8_covers), one persistent workgroup per CU walks them
GemmLaunch plan_p8(int M, int N, int act) {
    GemmLaunch L;
    L.kernel = HGR_KERNEL_P8; L.epilogue = act ? HGR_EPI_BIAS_QUICKGELU : HGR_EPI_BIAS; L.act = act; L.rows = M;
    L.tiles_m = M / 256; L.tiles_n = N / 256; L.group = duo_group();
    const int tiles = L.tiles_m * L.tiles_n;
    L.grid_x = (unsigned)(tiles < hgr_cu_count() ? tiles : hgr_cu_count());
    return L;
}

// By shape: measured against gemm_nt_duo (tools/p8_bench.py, back to back, one MI355X, bit-identical): 25 600 x 3 072 x 3 072
// 436 -> 394 us (1 108 -> 1 228 TF/s), ViT-L/14's c_fc 65 536 x 4 096 x 1 024 543 -> 519, ViT-B/32's c_fc (K = 768, 4.7 tiles per CU)
// 128.0 -> 126.2 back to back and 132.5 -> 131.8 in the step (the step itself unchanged), its k / v projection (2.3 tiles per CU)
// 70.9 -> 74.3: a K-tile of this form takes ~3 400 clocks where fill, matrix and LDS time are ~2 000 each (ablation builds at
// K = 3 072: 390 us; no fragment reads 378; no LDS-DMA behind the prologue 318; neither 274 - the fill that does not overlap is
// added), and a tile's prologue and epilogue run beside nothing - so it pays with long K and many tiles per CU only.
bool p8_wanted(int M, int N, int K) {
    const int m = k_p8.get();
    if (!m || !p8_covers(M, N, K)) return false;
    return m == 1 || (K >= 1024 && (int64_t)(M / 256) * (N / 256) >= 4 * hgr_cu_count());
}

// ---- plan capture (hgr_gemm_plan_capture) and the launch step -----------------------------------------------------------
thread_local hgr_gemm_launch *cap_out = nullptr;
thread_local int cap_max = 0;
// every covered entry point holds one: whichever way the call ends (planned or rejected), the calling thread is disarmed
struct CaptureScope { ~CaptureScope() { cap_out = nullptr; cap_max = 0; } };

// rows [row0, row0 + rows) of the call `a` describes (csz / rsz: element sizes of C and of the second operand)
GemmArgs gemm_rows(GemmArgs a, int row0, int rows, size_t csz, size_t rsz) {
    a.A += (size_t)row0 * a.lda * 2;
    a.C = (char *)a.C + (size_t)row0 * a.ldc * csz;
    if (a.res) a.res = (const float *)((const char *)a.res + (size_t)row0 * a.ldr * rsz);
    a.M = rows; a.m_fastest = gemm_m_fastest(rows, a.N, a.K);
    return a;
}

int gemm_run(const char *who, const GemmArgs &call, const GemmLaunch *plan, int n, int dtype, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    HGR_REQUIRE(!cap_out || n <= cap_max, "%s: %d launches, hgr_gemm_plan_capture armed for %d", who, n, cap_max);
    for (int i = 0; i < n; ++i) {
        const GemmLaunch &L = plan[i];
        GemmArgs a = L.rows == call.M ? call : gemm_rows(call, L.row0, L.rows, L.out32 ? 4 : 2, epi_has_idn16(L.epilogue) ? 2 : 4);
        a.tiles_m = L.tiles_m; a.tiles_n = L.tiles_n; a.total = L.total;
        a.nbig = L.nbig; a.big_panels = L.big_panels; a.tiles_m_half = L.tiles_m_half; a.group = L.group;
        if (cap_out) {
            cap_out[i] = hgr_gemm_launch{L.kernel, L.variant, L.epilogue, L.out32, L.act, (int32_t)L.grid_x, (int32_t)L.grid_y, a.tiles_m, a.tiles_n, a.total,
                                         a.nbig, a.big_panels, a.tiles_m_half, a.group, a.m_fastest, a.vec_ok, L.row0, L.rows};
            continue;
        }
        const dim3 grid(L.grid_x, L.grid_y);
        switch (L.kernel) {
            case HGR_KERNEL_128: launch_128(a, dtype, L.epilogue, L.out32, L.variant, grid, s); break;
            case HGR_KERNEL_256: launch_256(a, dtype, L.epilogue, L.out32, L.variant != 0, grid, s); break;
            case HGR_KERNEL_DUO: launch_duo(a, dtype, L.epilogue, L.out32, L.variant, grid, s); break;
            default: launch_p8(a, dtype, L.act, grid, s); break;
        }
    }
    if (cap_out) return HGR_OK;
    HGR_CHECK_LAUNCH(who);
    return HGR_OK;
}

}  // namespace

extern "C" int hgr_gemm_plan_capture(hgr_gemm_launch *out, int max_launches) {
    if (!out && max_launches == 0) {             // disarm; 1 = no covered call had consumed the capture
        const int armed = cap_out != nullptr;
        CaptureScope disarm;
        return armed;
    }
    HGR_REQUIRE(out && max_launches >= 1, "hgr_gemm_plan_capture: out must not be null and max_launches >= 1 (or NULL, 0 to disarm), got %d", max_launches);
    cap_out = out; cap_max = max_launches;
    return HGR_OK;
}

extern "C" int hgr_gemm_set_tail(int enabled, int full_panels) {
    HGR_REQUIRE((enabled == 0 || enabled == 1) && full_panels >= -1, "hgr_gemm_set_tail: enabled must be 0 or 1, full_panels >= -1 (-1 = choose), got %d, %d", enabled, full_panels);
    k_pb.set(full_panels);
    return k_tail.set(enabled);
}

extern "C" int hgr_gemm_set_tile(int tile) {
    HGR_REQUIRE(tile == 0 || tile == 128 || tile == 256 || tile == 2, "hgr_gemm_set_tile: tile must be 0, 128, 256 or 2 (256 x 128 tiles, two workgroups per CU), got %d", tile);
    return k_tile.set(tile);
}

extern "C" int hgr_gemm_set_p8(int mode) {
    HGR_REQUIRE(mode >= 0 && mode <= 2, "hgr_gemm_set_p8: mode must be 0 (never), 1 (wherever it covers) or 2 (by shape), got %d", mode);
    return k_p8.set(mode);
}

extern "C" int hgr_gemm_set_persist(int enabled) {
    HGR_REQUIRE(enabled == 0 || enabled == 1, "hgr_gemm_set_persist: enabled must be 0 or 1, got %d", enabled);
    return k_persist.set(enabled);
}

// ---- hgr_gemm_nt ---------------------------------------------------------------------------------------------------------
namespace {
// Kernel and tile plan of one hgr_gemm_nt call (validated; `a` = the whole call): one launch, or two for the split plan.  Returns the count.
int plan_gemm_nt(const GemmArgs &a, int epilogue, bool out_f32, GemmLaunch plan[2]) {
    const int M = a.M, N = a.N, K = a.K;
    // rows [m_lo, m_lo + m_cnt) with one tile size
    auto tiled = [&](int m_lo, int m_cnt, bool big) {
        // outputs at most 64 wide (1x1 convolutions into the 64-channel ResNet stages): the 256 x 64 arrangement of the small kernel
        const bool tall = !big && N <= 64 && m_cnt >= 1024 && epilogue == HGR_EPI_BIAS_RELU && !out_f32;
        GemmLaunch L = tall  ? plan_tiles(HGR_KERNEL_128, V128_TALL, HGR_EPI_BIAS_RELU, false, m_cnt, 1, 256, 1)
                       : big ? plan_tiles(HGR_KERNEL_256, 0, epilogue, out_f32, m_cnt, N, 256, 256)
                             : plan_tiles(HGR_KERNEL_128, V128_PLAIN, epilogue, out_f32, m_cnt, N, BM, BN);
        L.row0 = m_lo;
        return L;
    };
    // Tile choice.  The 256^2 deep-pipelined kernel owns a CU (one 512-thread workgroup), so a launch runs in rounds of
    // 256 workgroups; 128^2 tiles run 2 workgroups per CU.  Three plans are priced with measured tile times: all big,
    // all small, or full rounds of big tiles on the first row panels + the remaining panels on the small-tile kernel in a
    // second launch (pays off at long K, where a mostly empty last big round is expensive: c_proj / patch GEMM).
    const int force = k_tile.get();
    const int tn256 = (N + 255) / 256, tm256 = (M + 255) / 256;
    const int64_t t256 = (int64_t)tm256 * tn256;
    const int64_t t128 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
    // measured tile times on MI355X (us): 256^2 tile ~ 1.75 per K-tile + 14 (prologue + epilogue, nothing overlaps them
    // at one workgroup per CU); 128^2 tile at 2 per CU ~ 1.08 per K-tile + 9
    const double Tb = 1.75 * (K / 64) + 14.0, Ts = 1.08 * (K / 64) + 9.0;
    const double cost_small = (double)((t128 + 511) / 512) * Ts;
    const double cost_big = (double)((t256 + 255) / 256) * Tb;
    const int64_t rounds = t256 / 256;
    const int big_panels = (int)((rounds * 256) / tn256);
    const int m1 = big_panels * 256;
    double cost_split = 1e30;
    if (k_split.get() && rounds >= 1 && m1 > 0 && m1 < M) {
        const int64_t ts = (int64_t)((M - m1 + 127) / 128) * ((N + 127) / 128);
        cost_split = (double)rounds * Tb + (double)((ts + 511) / 512) * Ts + 2.0;          // + one kernel boundary
    }
    // 256 x 128 tiles, two workgroups per CU (gemm_nt_duo): fp32 residual / 16-bit epilogues of the transformer towers
    const bool duo_ok = K >= 128 && (out_f32 || (epilogue != HGR_EPI_BIAS_RESIDUAL && epilogue != HGR_EPI_ACCUM)) &&
                        (int64_t)M * a.lda * 2 < (1ll << 32) && (int64_t)N * a.ldw * 2 < (1ll << 32) && a.ldc < (1 << 20) && a.ldr < (1 << 20);
    // Plan choice for the shapes gemm_nt_duo covers: measured (tools/gemm_plan_ab.py, same-process A/B, f16, one MI355X; bit-identical
    // outputs): qkv 97 -> 91 us, out-proj 59 -> 49, c_fc 136 -> 124, c_proj 145 -> 126, patch 124 -> 118, class logits 24.7 -> 20.7,
    // text qkv 168 -> 154, ViT-L/14 out / proj 411 -> 361 / 1029 -> 999, ViT-L/14 qkv / fc a tie; a launch with fewer tiles than
    // half the chip's 512 slots (small text batches, ragged test shapes) stays on the 128^2 / cost-model plans.
    const int64_t tduo = (int64_t)((M + 255) / 256) * ((N + 127) / 128);
    // ... and an output much narrower than its 128-column tiles (the 64-channel ResNet stage: half of every tile would be padding;
    // measured 252 vs 194 us on the 256 x 64 arrangement of the small kernel) stays where it was
    const bool duo_fits = (N + 127) / 128 * 128 - N <= N / 8;
    if (duo_ok && (force == 2 || (force == 0 && tduo >= 256 && duo_fits))) plan[0] = plan_duo(a, 0, epilogue, out_f32);
    else if (force == 128 || K < 128) plan[0] = tiled(0, M, false);
    else if (epi_has_idn16(epilogue) && force != 256) plan[0] = tiled(0, M, false);   // only the 128 kernel loads the identity / stores by full lines
    else if (force == 256) plan[0] = tiled(0, M, true);
    else if (cost_split < cost_big && cost_split < cost_small) { plan[0] = tiled(0, m1, true); plan[1] = tiled(m1, M - m1, false); return 2; }
    else plan[0] = tiled(0, M, cost_big <= cost_small && t256 >= 128);
    return 1;
}
}  // namespace

extern "C" int hgr_gemm_nt(const void *A, int64_t lda, const void *W, int64_t ldw, void *C, int64_t ldc,
                           const float *bias, const void *residual, int64_t ldr,
                           int M, int N, int K, int dtype, int epilogue, int out_f32, void *stream) {
    CaptureScope capture;
    HGR_REQUIRE(A && W && C, "hgr_gemm_nt: null operand");
    HGR_REQUIRE(M >= 1 && N >= 1 && K >= BK, "hgr_gemm_nt: bad shape M=%d N=%d K=%d", M, N, K);
    HGR_REQUIRE(K % BK == 0, "hgr_gemm_nt: K=%d must be a multiple of %d (pad the operands)", K, BK);
    HGR_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0, "hgr_gemm_nt: lda=%lld ldw=%lld must be >= K and multiples of 8", (long long)lda, (long long)ldw);
    HGR_REQUIRE(hgr_aligned(A, 16) && hgr_aligned(W, 16), "hgr_gemm_nt: A and W must be 16-byte aligned");
    HGR_REQUIRE(ldc >= N, "hgr_gemm_nt: ldc=%lld < N=%d", (long long)ldc, N);
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_gemm_nt: bad dtype %d", dtype);
    HGR_REQUIRE(epilogue >= HGR_EPI_NONE && epilogue <= HGR_EPI_QGELU_GRAD16, "hgr_gemm_nt: bad epilogue %d", epilogue);
    HGR_REQUIRE(epilogue != HGR_EPI_ACCUM || out_f32, "hgr_gemm_nt: ACCUM accumulates into an fp32 C");
    HGR_REQUIRE(!epi_has_bias(epilogue) || bias, "hgr_gemm_nt: epilogue %d needs bias", epilogue);
    HGR_REQUIRE((epilogue != HGR_EPI_BIAS_RESIDUAL && !epi_has_idn16(epilogue)) || (residual && ldr >= N), "hgr_gemm_nt: epilogue %d needs its second operand (residual / identity / pre-activation) with ldr >= N", epilogue);
    HGR_REQUIRE(!epi_has_idn16(epilogue) || !out_f32, "hgr_gemm_nt: ADD16_RELU / QGELU_GRAD16 write 16-bit output");
    HGR_REQUIRE(hgr_aligned(C, out_f32 ? 4 : 2), "hgr_gemm_nt: C misaligned");

    bool vec = (ldc % 4 == 0) && hgr_aligned(C, out_f32 ? 16 : 8);
    if (epi_has_bias(epilogue)) vec = vec && hgr_aligned(bias, 16);
    if (epilogue == HGR_EPI_BIAS_RESIDUAL) vec = vec && (ldr % 4 == 0) && hgr_aligned(residual, 16);
    if (epi_has_idn16(epilogue)) vec = vec && (ldr % 4 == 0) && hgr_aligned(residual, 8);
    GemmArgs a = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, vec, duo_dbg());
    a.bias = bias; a.res = (const float *)residual; a.ldr = ldr;
    GemmLaunch plan[2];
    const int n = plan_gemm_nt(a, epilogue, out_f32 != 0, plan);
    return gemm_run("hgr_gemm_nt", a, plan, n, dtype, stream);
}

// ---- 3 x 3 convolutions ----------------------------------------------------------------------------------------------------
namespace {
// Input channels of the direct kernel (hgr_conv_direct.hip) that takes a convolution, 0 = the implicit GEMM; HGR_CONV_DIRECT=0 keeps the latter
int conv_direct_channels(int C, int Cout, int stride, int Kp, int64_t in_pixels, bool out16_aligned) {
    if (!k_conv_direct.get() || stride != 1 || !out16_aligned) return 0;
    // 32 input channels (the stem at 112 x 112)
    if (C == 32 && (Cout == 32 || Cout == 64) && Kp >= 288) return 32;
    // 64 -> 64 channels (layer1 of the ModifiedResNets): the implicit GEMM pulls every input byte nine times through LDS-DMA at
    // ~28 GB/s per CU (258 us at 56 x 56, batch 512); the halo-tile kernel reads it 1.27 times
    if (C == 64 && Cout == 64 && Kp >= 576 && in_pixels >= 4096) return 64;
    return 0;
}

// the ladder of the implicit-GEMM convolution (`a` carries the geometry)
GemmLaunch plan_conv3x3(const GemmArgs &a, int64_t in_pixels, bool relu, bool out16_aligned) {
    const int C = a.cC, Cout = a.N, Kp = a.K, stride = a.cStride, force = k_tile.get(), epi = relu ? HGR_EPI_BIAS_RELU : HGR_EPI_NONE;
    // big tiles when the output is at least 256 wide-ish and the launch has >= 160 of them (measured at batch 512: 14x14x256
    // 160 -> 142 us with 392 tiles, 7x7x512 160 -> 135 us with 196 tiles; K is 2304 / 4608 there, so one round is long)
    const int64_t t256 = (int64_t)((a.M + 255) / 256) * ((Cout + 255) / 256);
    // ... and 256-wide tiles do not waste more columns than 128-wide ones would (Cout = 128: half of every 256^2 tile would be
    // padding - measured 1066 vs 646 us at 56x56x128 and 285 vs 160 us at 28x28x128, batch 512)
    const int waste256 = (Cout + 255) / 256 * 256 - Cout, waste128 = (Cout + 127) / 128 * 128 - Cout;
    const bool big = relu && force != 128 && Kp >= 128 && Cout >= 128 && (t256 >= 160 || force == 256) && waste256 <= waste128;
    // 256 x 128 tiles, two workgroups per CU (gemm_nt_duo with the implicit-im2col loader): C % 64 == 0, stride 1, outputs that fill
    // 128-column tiles, operands addressable with 32-bit offsets; HGR_CONV_DUO=0 keeps the kernels above
    const int64_t tduo = (int64_t)((a.M + 255) / 256) * ((Cout + 127) / 128);
    if (k_conv_duo.get() && relu && a.cUni && stride == 1 && Cout % 128 == 0 && Kp == 9 * C && tduo >= 256 && out16_aligned &&
        in_pixels * C * 2 < (1ll << 31) && (int64_t)Cout * Kp * 2 < (1ll << 32) && force == 0)
        return plan_duo(a, 5, HGR_EPI_BIAS_RELU, false);
    if (big) return plan_tiles(HGR_KERNEL_256, 1, HGR_EPI_BIAS_RELU, false, a.M, Cout, 256, 256);
    // tall 256 x 64 tiles: no MFMAs spent on columns that do not exist
    if (Cout <= 64 && a.M >= 1024) return plan_tiles(HGR_KERNEL_128, V128_CONV_TALL, epi, false, a.M, 1, 256, 1);
    return plan_tiles(HGR_KERNEL_128, V128_CONV, epi, false, a.M, Cout, BM, BN);
}

int conv3x3_launch(const void *x, const void *w, const float *bias, void *out,
                   int B, int H, int W, int C, int Cout, int stride, int Kp, int dtype, bool relu, void *stream) {
    CaptureScope capture;
    HGR_REQUIRE(x && w && out && (bias || !relu), "hgr_conv3x3_nhwc: null operand");
    HGR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cout >= 1 && (stride == 1 || stride == 2), "hgr_conv3x3_nhwc: bad geometry B=%d H=%d W=%d Cout=%d stride=%d", B, H, W, Cout, stride);
    HGR_REQUIRE(C >= 8 && C % 8 == 0 && C <= 16384, "hgr_conv3x3_nhwc: C=%d must be a multiple of 8 in [8, 16384]", C);
    HGR_REQUIRE(Kp >= 9 * C && Kp % BK == 0, "hgr_conv3x3_nhwc: Kp=%d must be >= 9*C and a multiple of %d", Kp, BK);
    HGR_REQUIRE(hgr_aligned(x, 16) && hgr_aligned(w, 16) && hgr_aligned(out, 8) && (!bias || hgr_aligned(bias, 16)) && Cout % 4 == 0, "hgr_conv3x3_nhwc: misaligned operand / Cout %% 4 != 0");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_conv3x3_nhwc: bad dtype %d", dtype);
    if (const int direct = conv_direct_channels(C, Cout, stride, Kp, (int64_t)B * H * W, hgr_aligned(out, 16))) {
        if (cap_out) { *cap_out = hgr_gemm_launch{HGR_KERNEL_CONV_DIRECT, direct, relu ? HGR_EPI_BIAS_RELU : HGR_EPI_NONE, 0, relu}; return HGR_OK; }
        return hgr_conv3x3_c32_launch(x, w, bias, out, B, H, W, Cout, Kp, dtype, relu ? 1 : 0, stream, 0, direct);
    }
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const int64_t M64 = (int64_t)B * Ho * Wo;
    HGR_REQUIRE(M64 < (1ll << 31), "hgr_conv3x3_nhwc: too many output pixels");
    GemmArgs a = gemm_args(x, 0, w, Kp, out, Cout, (int)M64, Cout, Kp, true, 0);
    a.bias = bias; a.m_fastest = 0;
    a.cH = H; a.cW = W; a.cC = C; a.cStride = stride; a.cHo = Ho; a.cWo = Wo;
    a.cMagic = (unsigned)(((1ull << 32) + (unsigned)C - 1) / (unsigned)C);
    a.cUni = (C % 64 == 0) ? 1 : 0;
    const GemmLaunch L = plan_conv3x3(a, (int64_t)B * H * W, relu, hgr_aligned(out, 16));
    return gemm_run("hgr_conv3x3_nhwc", a, &L, 1, dtype, stream);
}
}  // namespace

extern "C" int hgr_conv3x3_nhwc(const void *x, const void *w, const float *bias, void *out,
                                int B, int H, int W, int C, int Cout, int stride, int Kp, int dtype, void *stream) {
    return conv3x3_launch(x, w, bias, out, B, H, W, C, Cout, stride, Kp, dtype, true, stream);
}

extern "C" int hgr_conv3x3_nhwc_plain(const void *x, const void *w, void *out, int B, int H, int W, int C, int Cout, int Kp,
                                      int dtype, void *stream) {
    return conv3x3_launch(x, w, nullptr, out, B, H, W, C, Cout, 1, Kp, dtype, false, stream);
}

extern "C" int hgr_gemm_nt_splitk(const void *A, int64_t lda, const void *W, int64_t ldw, float *partial, int64_t ldc,
                                  int M, int N, int K, int kc, int dtype, void *stream) {
    CaptureScope capture;
    HGR_REQUIRE(A && W && partial, "hgr_gemm_nt_splitk: null operand");
    HGR_REQUIRE(M >= 1 && N >= 1 && K >= BK && K % BK == 0 && kc >= BK && kc % BK == 0, "hgr_gemm_nt_splitk: bad shape M=%d N=%d K=%d kc=%d", M, N, K, kc);
    HGR_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0 && hgr_aligned(A, 16) && hgr_aligned(W, 16), "hgr_gemm_nt_splitk: operands must be 16-byte aligned with leading dimensions %% 8 == 0");
    HGR_REQUIRE(ldc >= N && ldc % 4 == 0 && hgr_aligned(partial, 16), "hgr_gemm_nt_splitk: partial must be 16-byte aligned, ldc %% 4 == 0");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_gemm_nt_splitk: bad dtype %d", dtype);
    const int S = (K + kc - 1) / kc;
    HGR_REQUIRE(S <= 65535, "hgr_gemm_nt_splitk: %d splits exceed the grid limit", S);
    GemmArgs a = gemm_args(A, lda, W, ldw, partial, ldc, M, N, K, true, 0);
    a.m_fastest = 0; a.kc = kc; a.csplit = (int64_t)M * ldc;
    // every slice at least 2 K-tiles deep and an output of at least one 256^2 tile: the deep-pipelined kernel
    const bool big = k_tile.get() != 128 && M >= 256 && N >= 256 && kc >= 128 && (K - (S - 1) * kc) >= 128;
    const GemmLaunch L = big ? plan_tiles(HGR_KERNEL_256, 0, HGR_EPI_NONE, true, M, N, 256, 256, (unsigned)S)
                             : plan_tiles(HGR_KERNEL_128, V128_PLAIN, HGR_EPI_NONE, true, M, N, BM, BN, (unsigned)S);
    return gemm_run("hgr_gemm_nt_splitk", a, &L, 1, dtype, stream);
}

// ---- LayerNorm folded into the GEMMs around it --------------------------------------------------------------------------
namespace {
int ln_common_checks(const char *who, const void *A, int64_t lda, const void *W, int64_t ldw, int M, int N, int K, int dtype) {
    HGR_REQUIRE(A && W, "%s: null operand", who);
    HGR_REQUIRE(M >= 1 && N >= 128 && N % 128 == 0 && K >= 128 && K % 64 == 0, "%s: bad shape M=%d N=%d K=%d (N %% 128 == 0, K %% 64 == 0, K >= 128)", who, M, N, K);
    HGR_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0 && hgr_aligned(A, 16) && hgr_aligned(W, 16), "%s: operands must be 16-byte aligned with leading dimensions %% 8 == 0", who);
    HGR_REQUIRE((int64_t)M * lda * 2 < (1ll << 32) && (int64_t)N * ldw * 2 < (1ll << 32) && N < (1 << 20), "%s: operands beyond 4 GB / N >= 2^20", who);
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "%s: bad dtype %d", who, dtype);
    return HGR_OK;
}
}  // namespace

extern "C" int hgr_gemm_nt_res_stats(const void *A, int64_t lda, const void *W, int64_t ldw, void *xh, void *xl, int64_t ldx,
                                     const float *bias, float *stats, int M, int N, int K, int dtype, void *stream) {
    return hgr_gemm_nt_res_stats_guard(A, lda, W, ldw, xh, xl, ldx, bias, stats, 0.f, nullptr, M, N, K, dtype, stream);
}

extern "C" int hgr_gemm_nt_res_stats_guard(const void *A, int64_t lda, const void *W, int64_t ldw, void *xh, void *xl, int64_t ldx,
                                           const float *bias, float *stats, float guard_sumsq, uint32_t *flag,
                                           int M, int N, int K, int dtype, void *stream) {
    CaptureScope capture;
    if (int rc = ln_common_checks("hgr_gemm_nt_res_stats", A, lda, W, ldw, M, N, K, dtype)) return rc;
    HGR_REQUIRE(!flag || (guard_sumsq > 0.f && hgr_aligned(flag, 4)), "hgr_gemm_nt_res_stats_guard: flag needs guard_sumsq > 0 and 4-byte alignment");
    HGR_REQUIRE(xh && xl && bias && stats, "hgr_gemm_nt_res_stats: null xh / xl / bias / stats");
    // the interior epilogue reads and writes the pair with 16-byte accesses (8 columns per lane) at 32-bit offsets of up to 127 rows
    HGR_REQUIRE(ldx >= N && ldx % 8 == 0 && ldx < (1 << 23) && hgr_aligned(xh, 16) && hgr_aligned(xl, 16), "hgr_gemm_nt_res_stats: xh / xl must be 16-byte aligned, ldx %% 8 == 0, ldx < 2^23");
    HGR_REQUIRE(hgr_aligned(bias, 16) && hgr_aligned(stats, 8), "hgr_gemm_nt_res_stats: bias must be 16-byte, stats 8-byte aligned");
    GemmArgs a = gemm_args(A, lda, W, ldw, nullptr, 0, M, N, K, true, duo_dbg());
    a.bias = bias;
    a.ln_stats = stats; a.ln_slots = N / 64; a.ln_xh = xh; a.ln_xl = xl; a.ln_ldx = ldx;
    a.ln_flag = flag; a.ln_guard = guard_sumsq;
    const GemmLaunch L = plan_duo(a, 1, HGR_EPI_BIAS_RESIDUAL, true);
    return gemm_run("hgr_gemm_nt_res_stats", a, &L, 1, dtype, stream);
}

extern "C" int hgr_gemm_nt_ln(const void *X16, int64_t ldx, const void *Wfold, int64_t ldw, void *C, int64_t ldc,
                              const float *ln_s, const float *ln_c, const float *stats, float eps,
                              int M, int N, int K, int dtype, int act, void *stream) {
    CaptureScope capture;
    if (int rc = ln_common_checks("hgr_gemm_nt_ln", X16, ldx, Wfold, ldw, M, N, K, dtype)) return rc;
    HGR_REQUIRE(C && ln_s && ln_c && stats, "hgr_gemm_nt_ln: null C / ln_s / ln_c / stats");
    HGR_REQUIRE(K % 128 == 0, "hgr_gemm_nt_ln: the row width K=%d must be a multiple of 128 (two 64-column statistic slots per 16-byte load)", K);
    // 16-bit C rows are addressed as a 64-bit tile base + a 32-bit per-lane byte offset of up to 127 rows: 127 * ldc * 2 < 2^32
    HGR_REQUIRE(ldc >= N && ldc % 8 == 0 && ldc < (1 << 23) && hgr_aligned(C, 16), "hgr_gemm_nt_ln: C must be 16-byte aligned with ldc %% 8 == 0, ldc < 2^23");
    HGR_REQUIRE(hgr_aligned(ln_s, 16) && hgr_aligned(ln_c, 16) && hgr_aligned(stats, 16), "hgr_gemm_nt_ln: ln_s / ln_c / stats must be 16-byte aligned");
    HGR_REQUIRE(act == 0 || act == 1, "hgr_gemm_nt_ln: act must be 0 (none) or 1 (QuickGELU), got %d", act);
    GemmArgs a = gemm_args(X16, ldx, Wfold, ldw, C, ldc, M, N, K, true, duo_dbg());
    a.ln_stats = const_cast<float *>(stats); a.ln_slots = K / 64; a.ln_eps = eps; a.ln_s = ln_s; a.ln_c = ln_c;
    const int epi = act ? HGR_EPI_BIAS_QUICKGELU : HGR_EPI_BIAS;
    const GemmLaunch L = k_tile.get() == 0 && p8_wanted(M, N, K) ? plan_p8(M, N, act) : plan_duo(a, 2, epi, false);
    return gemm_run("hgr_gemm_nt_ln", a, &L, 1, dtype, stream);
}

extern "C" int hgr_gemm_nt_bias_gelu_dual(const void *A, int64_t lda, const void *W, int64_t ldw, void *pre, int64_t ldpre, void *post, int64_t ldpost,
                                          const float *bias, int M, int N, int K, int dtype, void *stream) {
    CaptureScope capture;
    if (int rc = ln_common_checks("hgr_gemm_nt_bias_gelu_dual", A, lda, W, ldw, M, N, K, dtype)) return rc;
    HGR_REQUIRE(pre && post && bias, "hgr_gemm_nt_bias_gelu_dual: null pre / post / bias");
    HGR_REQUIRE(ldpre >= N && ldpost >= N && ldpre % 8 == 0 && ldpost % 8 == 0 && ldpre < (1 << 23) && ldpost < (1 << 23) && hgr_aligned(pre, 16) && hgr_aligned(post, 16) && hgr_aligned(bias, 16),
                "hgr_gemm_nt_bias_gelu_dual: pre / post / bias must be 16-byte aligned, leading dimensions >= N, %% 8 == 0, < 2^23");
    GemmArgs a = gemm_args(A, lda, W, ldw, pre, ldpre, M, N, K, true, duo_dbg());
    a.bias = bias; a.ln_xh = post; a.ln_ldx = ldpost;
    const GemmLaunch L = plan_duo(a, 4, HGR_EPI_BIAS, false);
    return gemm_run("hgr_gemm_nt_bias_gelu_dual", a, &L, 1, dtype, stream);
}

extern "C" int hgr_gemm_nt_qgelu_grad_colsum(const void *A, int64_t lda, const void *W, int64_t ldw, void *C, int64_t ldc, const void *pre, int64_t ldpre,
                                             float *colsum_part, int M, int N, int K, int dtype, void *stream) {
    CaptureScope capture;
    if (int rc = ln_common_checks("hgr_gemm_nt_qgelu_grad_colsum", A, lda, W, ldw, M, N, K, dtype)) return rc;
    HGR_REQUIRE(C && pre && colsum_part, "hgr_gemm_nt_qgelu_grad_colsum: null C / pre / colsum_part");
    HGR_REQUIRE(ldc >= N && ldpre >= N && ldc % 8 == 0 && ldpre % 8 == 0 && ldc < (1 << 20) && ldpre < (1 << 20) && hgr_aligned(C, 16) && hgr_aligned(pre, 16) && hgr_aligned(colsum_part, 16),
                "hgr_gemm_nt_qgelu_grad_colsum: C / pre / colsum_part must be 16-byte aligned, leading dimensions >= N, %% 8 == 0, < 2^20");
    GemmArgs a = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, true, duo_dbg());
    a.res = (const float *)pre; a.ldr = ldpre;
    a.colsum = colsum_part; a.colsum_units = (M + 63) / 64;
    const GemmLaunch L = plan_duo(a, 0, HGR_EPI_QGELU_GRAD16, false);
    return gemm_run("hgr_gemm_nt_qgelu_grad_colsum", a, &L, 1, dtype, stream);
}

// ---- logits GEMM with the evaluation consumers in its epilogue ------------------------------------------------------------
#define HGR_LE_PARAMS const void *feat16, const void *zsl_perm16, int rows, int D, int n_perm, const int32_t *tpos_perm, const int32_t *epos_perm, \
    const int32_t *level_first, int n_levels, const int32_t *filler_pos, const int32_t *train_cols, int n_train, const int32_t *test_cols, int n_test, int k, \
    int32_t *out_level, int32_t *out_top1, int32_t *out_topk, void *workspace, int dtype, void *stream
#define HGR_LE_ARGS feat16, zsl_perm16, rows, D, n_perm, tpos_perm, epos_perm, level_first, n_levels, filler_pos, train_cols, n_train, test_cols, n_test, k, \
    out_level, out_top1, out_topk, workspace, dtype, stream
static int logits_eval_stages(int stages, HGR_LE_PARAMS);
extern "C" int hgr_logits_eval(HGR_LE_PARAMS) { return logits_eval_stages(3, HGR_LE_ARGS); }
// the two stages on their own (same arguments; the row stage reads the workspace the tile stage of the same call sequence wrote):
// bench.py times them separately, hgr_logits_eval is the pair
extern "C" int hgr_logits_eval_tile_stage(HGR_LE_PARAMS) { return logits_eval_stages(1, HGR_LE_ARGS); }
extern "C" int hgr_logits_eval_row_stage(HGR_LE_PARAMS) { return logits_eval_stages(2, HGR_LE_ARGS); }

int hgr_logits_eval_rows_launch(const void *feat, const void *zslp, int D, int S, const unsigned long long *keys, const float *tmax,
                                const int *gp1, const float *gm2, const int32_t *level_first, int n_levels, const int32_t *filler_pos, const int32_t *train_cols, int n_train,
                                const int32_t *epos, const int32_t *test_cols, int n_test, int k, int32_t *out_level, int32_t *out_top1,
                                int32_t *out_topk, int rows, int dtype, void *stream);      // hgr_select.hip

extern "C" int64_t hgr_logits_eval_workspace_bytes(int rows, int n_perm) {
    if (rows < 1 || n_perm < 96 || n_perm % 96) return -1;
    return (int64_t)rows * (n_perm / 32) * 32;           // per (row, 32-column slice): 8-byte train key + per 16-column group (max, position, second) = 2 x 12 bytes
}

static int logits_eval_stages(int stages, const void *feat16, const void *zsl_perm16, int rows, int D, int n_perm,
                               const int32_t *tpos_perm, const int32_t *epos_perm, const int32_t *level_first,
                               int n_levels, const int32_t *filler_pos, const int32_t *train_cols, int n_train,
                               const int32_t *test_cols, int n_test, int k,
                               int32_t *out_level, int32_t *out_top1, int32_t *out_topk, void *workspace, int dtype, void *stream) {
    HGR_REQUIRE(feat16 && zsl_perm16 && tpos_perm && epos_perm && level_first && filler_pos && train_cols && out_level && workspace, "hgr_logits_eval: null operand");
    HGR_REQUIRE(rows >= 1 && D >= 128 && D % 128 == 0 && D <= 1024, "hgr_logits_eval: rows=%d D=%d unsupported (D %% 128 == 0, D <= 1024)", rows, D);
    HGR_REQUIRE(n_perm >= 96 && n_perm % 96 == 0 && n_perm / 32 <= 1024, "hgr_logits_eval: n_perm=%d must be a multiple of 96 and <= 32768 (32-column level-aligned slices, 96-column slabs)", n_perm);
    HGR_REQUIRE(n_levels >= 1 && n_levels <= 32 && n_train >= 1, "hgr_logits_eval: bad sizes (n_levels <= 32)");
    HGR_REQUIRE(k == 0 || (out_topk && test_cols && k >= 1 && k <= 32 && n_test >= k), "hgr_logits_eval: bad top-k arguments");
    HGR_REQUIRE(hgr_aligned(feat16, 16) && hgr_aligned(zsl_perm16, 16) && hgr_aligned(tpos_perm, 16) && hgr_aligned(epos_perm, 16) && hgr_aligned(workspace, 16), "hgr_logits_eval: operands must be 16-byte aligned");
    HGR_REQUIRE(dtype == HGR_BF16 || dtype == HGR_F16, "hgr_logits_eval: bad dtype %d", dtype);
    HGR_REQUIRE((int64_t)rows * D * 2 < (1ll << 32) && (int64_t)n_perm * D * 2 < (1ll << 32), "hgr_logits_eval: operands beyond 4 GB");
    const int S = n_perm / 32;
    SlabArgs a;
    a.A = (const char *)feat16; a.lda = D; a.W = (const char *)zsl_perm16; a.ldw = D; a.M = rows; a.K = D; a.Np = n_perm;
    a.tpos = tpos_perm; a.epos = epos_perm; a.S = S;
    { static const int d = hgr_lab_env("HGR_LS_DBG"); a.dbg = d; }
    a.ev_key = (unsigned long long *)workspace;
    a.ev_tmax = (float *)((char *)workspace + (size_t)rows * S * 8);
    a.ev_p1 = (int *)((char *)workspace + (size_t)rows * S * 16);
    a.ev_m2 = (float *)((char *)workspace + (size_t)rows * S * 24);
    if (stages & 1) launch_logits_slab(a, dtype, (hipStream_t)stream);
    HGR_CHECK_LAUNCH("hgr_logits_eval (tile stage)");
    if (!(stages & 2)) return HGR_OK;
    return hgr_logits_eval_rows_launch(feat16, zsl_perm16, D, S, a.ev_key, a.ev_tmax, a.ev_p1, a.ev_m2, level_first, n_levels, filler_pos, train_cols, n_train,
                                       epos_perm, test_cols, n_test, k, out_level, out_top1, out_topk, rows, dtype, stream);
}

