// The hierarchy report of an evaluation batch (include/hgr.h, HGR_REPORT_*): the quantities hgr_eval_counters_rows sums over every
// class and depth (main.py:139-191), kept apart by the depth of the target and the level of the path, plus how far in the tree the
// predictions lie from the target.  Integer counts only, added into an int64 table: the table depends neither on the order of the
// rows, nor on how they fall onto waves and blocks, nor on how they were cut into launches.
#include "hgr_common.h"

namespace {

constexpr int ERR_NT = 512;          // 8 waves, ONE ROW PER WAVE: a row reads up to 22 paths of up to 32 nodes, a lane holds one path position
constexpr int ERR_WAVES = ERR_NT / HGR_WAVE;
constexpr int ERR_MAXL = HGR_REPORT_MAXL;
constexpr int ERR_MAXGRID = 8;       // fixed small grid: batch 512 = 8 rows per wave
constexpr int ERR_PREDS = 20;        // predictions whose height is summed (K = 20 is the largest)
constexpr int ERR_TOP1 = 32;         // the lane that holds top1[r]; lanes 0..k-1 hold pred[r, :k]

// length of the run of set bits that starts at bit 0
__device__ __forceinline__ int prefix_len(unsigned m) { return m == 0xFFFFFFFFu ? 32 : __builtin_ctz(~m); }

__global__ __launch_bounds__(ERR_NT) void eval_report_rows(const int32_t *__restrict__ pred, int k, const int64_t *__restrict__ targets,
                                                           const int32_t *__restrict__ top1, const int32_t *__restrict__ lv, int n_levels,
                                                           const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes,
                                                           const int32_t *__restrict__ anc_levels, int n_nodes,
                                                           unsigned long long *__restrict__ table, int B) {
    __shared__ unsigned long long s_tab[HGR_REPORT_LEN];                      // this block's counts of this launch, table layout
    for (int i = threadIdx.x; i < HGR_REPORT_LEN; i += ERR_NT) s_tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // both 32-lane halves hold the target's path (lane & 31 = position): one ballot compares it against TWO predictions' paths
    const int pos = lane & 31, half = lane >> 5;
    unsigned lvl_rows = 0, lvl_match = 0;                                     // lane i < 32: LEVEL[i] of this wave's rows
    unsigned long long hk1 = 0, hk2 = 0, hk5 = 0, hk10 = 0, hk20 = 0;         // wave-uniform: HEIGHT_AT_K of this wave's rows
    for (int64_t r = (int64_t)blockIdx.x * ERR_WAVES + wave; r < B; r += (int64_t)gridDim.x * ERR_WAVES) {
        const int64_t t64 = targets[r];
        if (t64 < 0 || t64 >= (int64_t)n_nodes) continue;                     // padding row (wave-uniform): nothing counted, no table read
        const int tgt = (int)t64;
        const int o = anc_ptr[tgt];
        const int L = anc_ptr[tgt + 1] - o;
        if (L < 1 || L > ERR_MAXL) continue;                                  // the same rule as hgr_eval_counters_rows
        // round trip 1: the row's predictions (one per lane) and the target's path; 2: the predictions' path ranges and the level
        // arg-maxes; 3: the predictions' paths and the picks' path ranges; 4: the picks' parents
        int x = -1;
        if (lane < k) x = pred[r * k + lane];
        else if (lane == ERR_TOP1) x = top1[r];
        const bool live = pos < L;
        const int pa = live ? anc_nodes[o + pos] : -1;
        const int le = live ? anc_levels[o + pos] : -1;
        int ox = 0, Lx = 0;                                                   // Lx == 0: "unknown" (outside the tree, or no path of 1..32 nodes)
        if ((unsigned)x < (unsigned)n_nodes && (lane < ERR_PREDS || lane == ERR_TOP1)) {
            ox = anc_ptr[x];
            Lx = anc_ptr[x + 1] - ox;
            if (Lx < 1 || Lx > ERR_MAXL) Lx = 0;
        }
        const int q = level_pick(lv + r * n_levels, n_levels, le);            // -2: never a node id, never pa
        const bool qin = (unsigned)q < (unsigned)n_nodes;
        int par = -2;                                                         // parent of the pick; -1 = "root", -2 = no valid pick
        if (half == 0 && live && qin) {
            const int oq = anc_ptr[q];
            const int Lq = anc_ptr[q + 1] - oq;
            par = Lq >= 2 ? anc_nodes[oq + Lq - 2] : -1;
        }
        // top-k hits: first match of the target (ids are distinct: at most one)
        const unsigned long long hb = __ballot(lane < k && x == tgt);
        const int j = hb ? __builtin_ctzll(hb) : ERR_MAXL;
        const int t1 = __shfl(x, ERR_TOP1);
        const unsigned hh = (unsigned)__ballot(live && pa == t1);             // low half: path positions that are the row's top-1
        const unsigned mm = (unsigned)__ballot(live && q == pa);              // path positions matched by their level's arg-max
        const unsigned point = __popc(mm);
        const unsigned edge = path_edges(mm, L);                              // consecutive matched pairs; L == 1: main.py:179-180
        // chain: every pick is a node, the first one hangs under the root, every next one under the pick before it
        const int qprev = __shfl_up(q, 1);
        const bool link = qin && par == (pos == 0 ? -1 : qprev);
        const unsigned chain = (unsigned)__ballot(live && !link) == 0u;
        // common prefixes: step jj compares pred[r, 2 jj] (low half) and pred[r, 2 jj + 1] (high half), the last step top1[r]
        int c_test = 0, c_all = 0;
        unsigned hs1 = 0, hs2 = 0, hs5 = 0, hs10 = 0, hs20 = 0;
#pragma unroll
        for (int jj = 0; jj <= ERR_PREDS / 2; ++jj) {
            const int src = jj < ERR_PREDS / 2 ? 2 * jj + half : ERR_TOP1;
            const int sox = __shfl(ox, src), sLx = __shfl(Lx, src);
            const bool in = live && pos < sLx;
            const int px = in ? anc_nodes[sox + pos] : -1;
            const unsigned long long eq = __ballot(in && px == pa);
            const int c0 = prefix_len((unsigned)eq), c1 = prefix_len((unsigned)(eq >> 32));
            if (jj == ERR_PREDS / 2) { c_all = c0; break; }
            if (jj == 0) c_test = c0;
            const unsigned h0 = 2 * jj < k ? (unsigned)(L - c0) : 0u, h1 = 2 * jj + 1 < k ? (unsigned)(L - c1) : 0u;
            if (2 * jj < 1) hs1 += h0;
            if (2 * jj < 2) hs2 += h0;
            if (2 * jj < 5) hs5 += h0;
            if (2 * jj < 10) hs10 += h0;
            hs20 += h0;
            if (2 * jj + 1 < 2) hs2 += h1;
            if (2 * jj + 1 < 5) hs5 += h1;
            if (2 * jj + 1 < 10) hs10 += h1;
            hs20 += h1;
        }
        hk1 += hs1; hk2 += hs2; hk5 += hs5; hk10 += hs10; hk20 += hs20;
        const int lx_test = __shfl(Lx, 0), lx_all = __shfl(Lx, ERR_TOP1);
        const int d_test = lx_test ? lx_test + L - 2 * c_test : HGR_REPORT_DIST_UNKNOWN;
        const int d_all = lx_all ? lx_all + L - 2 * c_all : HGR_REPORT_DIST_UNKNOWN;
        // the row's counts: lanes 0..9 add DEPTH[L][lane], lanes 10 / 11 the two distance bins, the low half keeps LEVEL in registers
        const unsigned v = lane == 0 ? 1u : lane == 1 ? (unsigned)(j < 1) : lane == 2 ? (unsigned)(j < 2) : lane == 3 ? (unsigned)(j < 5)
                         : lane == 4 ? (unsigned)(j < 10) : lane == 5 ? (unsigned)(j < 20) : lane == 6 ? (unsigned)__popc(hh)
                         : lane == 7 ? point : lane == 8 ? edge : lane == 9 ? chain : 0u;
        if (lane < HGR_REPORT_DEPTH_COLS && v) atomicAdd(&s_tab[HGR_REPORT_DEPTH + L * HGR_REPORT_DEPTH_COLS + lane], (unsigned long long)v);
        if (lane == 10) atomicAdd(&s_tab[HGR_REPORT_DIST_TEST + d_test], 1ull);
        if (lane == 11) atomicAdd(&s_tab[HGR_REPORT_DIST_ALL + d_all], 1ull);
        if (half == 0 && live) {
            lvl_rows += 1;
            lvl_match += (mm >> pos) & 1u;
        }
    }
    if (half == 0) {
        if (lvl_rows) atomicAdd(&s_tab[HGR_REPORT_LEVEL + 2 * pos], (unsigned long long)lvl_rows);
        if (lvl_match) atomicAdd(&s_tab[HGR_REPORT_LEVEL + 2 * pos + 1], (unsigned long long)lvl_match);
    }
    if (lane == 0) {
        if (hk1) atomicAdd(&s_tab[HGR_REPORT_HEIGHT + 0], hk1);
        if (hk2) atomicAdd(&s_tab[HGR_REPORT_HEIGHT + 1], hk2);
        if (hk5) atomicAdd(&s_tab[HGR_REPORT_HEIGHT + 2], hk5);
        if (hk10) atomicAdd(&s_tab[HGR_REPORT_HEIGHT + 3], hk10);
        if (hk20) atomicAdd(&s_tab[HGR_REPORT_HEIGHT + 4], hk20);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HGR_REPORT_LEN; i += ERR_NT) {              // one flush per block: integer adds, any order
        const unsigned long long s = s_tab[i];
        if (s) atomicAdd(&table[i], s);
    }
}

}  // namespace

extern "C" int hgr_eval_report_rows(const int32_t *pred, int k, const int64_t *targets, const int32_t *top1, const int32_t *lv, int n_levels,
                                    const int32_t *anc_ptr, const int32_t *anc_nodes, const int32_t *anc_levels, int n_nodes,
                                    int64_t *table, int rows, void *stream) {
    HGR_REQUIRE(pred && targets && top1 && lv && anc_ptr && anc_nodes && anc_levels && table, "hgr_eval_report_rows: null operand (targets and table are required)");
    HGR_REQUIRE(rows >= 1 && k >= 1 && k <= ERR_MAXL && n_levels >= 1 && n_levels <= ERR_MAXL && n_nodes >= 1,
                "hgr_eval_report_rows: bad sizes rows=%d k=%d n_levels=%d n_nodes=%d (k, n_levels <= 32)", rows, k, n_levels, n_nodes);
    const int need = (rows - 1) / ERR_WAVES + 1;
    const int grid = need < ERR_MAXGRID ? need : ERR_MAXGRID;
    hipLaunchKernelGGL(eval_report_rows, dim3(grid), dim3(ERR_NT), 0, (hipStream_t)stream, pred, k, targets, top1, lv, n_levels, anc_ptr, anc_nodes,
                       anc_levels, n_nodes, reinterpret_cast<unsigned long long *>(table), rows);
    HGR_CHECK_LAUNCH("hgr_eval_report_rows");
    return HGR_OK;
}
