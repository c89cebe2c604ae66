// The evaluation counters of a MIXED-class batch (main.py:139-191): every row brings its own target and is scored against that
// target's own ancestor path, read from a device CSR of all paths.  Integer counts only until one thread finalises: the result
// does not depend on the order of the rows or on how they fall onto threads.
#include "hgr_common.h"

namespace {

constexpr int ECR_NT = 512;          // batch 512 = one pass; 8 waves on 4 SIMDs leave 256 VGPRs per lane for the unrolled row
constexpr int ECR_MAXL = 32;         // longest path (and most levels, and largest k) the unrolled loops cover

__global__ __launch_bounds__(ECR_NT) void eval_counters_rows(const int32_t *__restrict__ pred, int k, const int64_t *__restrict__ targets,
                                                             const int32_t *__restrict__ top1, const int32_t *__restrict__ lv, int n_levels,
                                                             const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes,
                                                             const int32_t *__restrict__ anc_levels, int n_nodes,
                                                             double *__restrict__ acc, int B) {
    // s_cnt: hits@1,2,5,10,20, hits_all, valid rows.  s_edge / s_point: matched consecutive level pairs (first-level matches in
    // bin 1, main.py:179-180) and matched levels, binned by the row's path length L: the ratios edge / (L - 1) and point / L are
    // formed once per bin from exact integers, so no double is ever added per row.
    __shared__ unsigned s_cnt[8];
    __shared__ unsigned s_edge[ECR_MAXL + 1], s_point[ECR_MAXL + 1];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x <= ECR_MAXL) { s_edge[threadIdx.x] = 0; s_point[threadIdx.x] = 0; }
    __syncthreads();
    unsigned cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int r = threadIdx.x; r < B; r += ECR_NT) {
        const int64_t t64 = targets[r];
        if (t64 < 0 || t64 >= (int64_t)n_nodes) continue;                     // padding row: nothing counted, no table read
        const int tgt = (int)t64;
        const int o = anc_ptr[tgt];
        const int L = anc_ptr[tgt + 1] - o;
        if (L < 1 || L > ECR_MAXL) continue;                                  // a node without a path counts as padding too
        // every load of the row is requested before the first compare (see eval_counters): the top-k ids and top-1 need only r,
        // the path needs o, the level arg-maxes need the path's levels - three dependent round trips per row, not one per level.
        // All arrays below are indexed by unrolled constants only: registers, no scratch.
        int pr[ECR_MAXL], pa[ECR_MAXL], le[ECR_MAXL], lvv[ECR_MAXL];
#pragma unroll
        for (int i = 0; i < ECR_MAXL; ++i) pr[i] = i < k ? pred[(int64_t)r * k + i] : -1;
        const int t1 = top1[r];
#pragma unroll
        for (int i = 0; i < ECR_MAXL; ++i) {
            pa[i] = i < L ? anc_nodes[o + i] : -1;
            le[i] = i < L ? anc_levels[o + i] : -1;
        }
#pragma unroll
        for (int i = 0; i < ECR_MAXL; ++i) lvv[i] = (unsigned)le[i] < (unsigned)n_levels ? lv[(int64_t)r * n_levels + le[i]] : -2;   // -2: never a node id, never pa
        int j = ECR_MAXL;                                                     // no match: inside no top-k, whatever k is
#pragma unroll
        for (int i = ECR_MAXL - 1; i >= 0; --i)
            if (i < k && pr[i] == tgt) j = i;                                 // first match (ids are distinct: at most one)
        cnt[0] += j < 1; cnt[1] += j < 2; cnt[2] += j < 5; cnt[3] += j < 10; cnt[4] += j < 20;
        unsigned mm = 0, hh = 0;                                              // bit i: level i of the path matched / is the row's top-1
#pragma unroll
        for (int i = 0; i < ECR_MAXL; ++i) {
            const bool live = i < L;
            hh |= (unsigned)(live && t1 == pa[i]) << i;
            mm |= (unsigned)(live && lvv[i] == pa[i]) << i;
        }
        cnt[5] += __popc(hh);
        const unsigned point = __popc(mm);
        const unsigned edge = L == 1 ? (mm & 1u) : __popc(mm & (mm >> 1));    // consecutive matched pairs; L == 1: main.py:179-180
        cnt[6] += 1;
        if (edge) atomicAdd(&s_edge[L], edge);
        if (point) atomicAdd(&s_point[L], point);
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        unsigned v = cnt[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[c], v);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[6] != 0) {                                  // an all-padding batch leaves acc untouched
        for (int c = 0; c < 6; ++c) acc[c] += (double)s_cnt[c];
        double path = (double)s_edge[1], point = (double)s_point[1];
        for (int L = 2; L <= ECR_MAXL; ++L) {                                 // fixed order, one division per bin
            path += (double)s_edge[L] / (double)(L - 1);
            point += (double)s_point[L] / (double)L;
        }
        acc[6] += path;
        acc[7] += point;
        acc[8] += (double)s_cnt[6];
    }
}

}  // namespace

extern "C" int hgr_eval_counters_rows(const int32_t *pred, int k, const int64_t *targets, const int32_t *top1, const int32_t *lv, int n_levels,
                                      const int32_t *anc_ptr, const int32_t *anc_nodes, const int32_t *anc_levels, int n_nodes,
                                      double *acc, int rows, void *stream) {
    HGR_REQUIRE(pred && targets && top1 && lv && anc_ptr && anc_nodes && anc_levels && acc, "hgr_eval_counters_rows: null operand (targets is required)");
    HGR_REQUIRE(rows >= 1 && k >= 1 && k <= ECR_MAXL && n_levels >= 1 && n_levels <= ECR_MAXL && n_nodes >= 1,
                "hgr_eval_counters_rows: bad sizes rows=%d k=%d n_levels=%d n_nodes=%d (k, n_levels <= 32)", rows, k, n_levels, n_nodes);
    hipLaunchKernelGGL(eval_counters_rows, dim3(1), dim3(ECR_NT), 0, (hipStream_t)stream, pred, k, targets, top1, lv, n_levels, anc_ptr, anc_nodes,
                       anc_levels, n_nodes, acc, rows);
    HGR_CHECK_LAUNCH("hgr_eval_counters_rows");
    return HGR_OK;
}
