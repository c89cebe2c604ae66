// Path scores (include/hgr.h, hgr_path_scores): S[r, n] = the weighted sum of the logits of row r along the root-to-node path of n,
// an ancestor gather-reduce over all N columns of every row.  Every term is one explicit fused multiply-add, added in path order from
// the top down: S does not depend on how rows and columns fall onto lanes, workgroups and launches.
#include "hgr_common.h"

namespace {

constexpr int PS_NT = 256;           // 4 waves, ONE NODE COLUMN PER LANE: the stores and the pass-through loads of a wave are one 256-B run
constexpr int PS_G = 4;              // rows per group: one load of a path id and one read of its weight serve PS_G gathers and PS_G FMAs
                                     // (8, 16 and 32 rows measured: no faster - the gathers' cache lines bound the kernel, profiles/NOTES.md)
constexpr int PS_ROWS = 32;          // rows per block: the path ids come from memory for the first group and from L1 for the other seven
constexpr int PS_MAXL = HGR_PATH_MAXL;
constexpr int PS_WLD = PS_MAXL + 1;  // LDS row stride of the weight table: lanes with different L read the same j - 33 L + j spreads them over
                                     // the banks (32 L + j puts them on two), lanes with the same L read one address (a broadcast)
constexpr int PS_MAXGRID_Y = 65535;

__global__ __launch_bounds__(PS_NT) void path_scores(const float *__restrict__ x, int64_t ld, float *__restrict__ s, int64_t ld_out, int n_nodes,
                                                     const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes,
                                                     const float *__restrict__ wtab, int rows) {
    __shared__ float s_w[(PS_MAXL + 1) * PS_WLD];
    for (int i = threadIdx.x; i < (PS_MAXL + 1) * PS_MAXL; i += PS_NT) s_w[(i / PS_MAXL) * PS_WLD + (i % PS_MAXL)] = wtab[i];
    __syncthreads();
    const int64_t n64 = (int64_t)blockIdx.x * PS_NT + threadIdx.x;
    if (n64 >= n_nodes) return;                                              // no barrier below
    const int n = (int)n64;
    const int o = anc_ptr[n];
    int L = anc_ptr[n + 1] - o;
    if (L < 1 || L > PS_MAXL) L = 0;                                          // pass-through (the sibling kernels' padding rule)
    const float *w = s_w + L * PS_WLD;
    for (int64_t rb = (int64_t)blockIdx.y * PS_ROWS; rb < rows; rb += (int64_t)gridDim.y * PS_ROWS) {
        const int64_t rend = rb + PS_ROWS < rows ? rb + PS_ROWS : rows;
        for (int64_t r0 = rb; r0 < rend; r0 += PS_G) {
            const float *xr[PS_G];
#pragma unroll
            for (int g = 0; g < PS_G; ++g) xr[g] = x + (r0 + g < rend ? r0 + g : rend - 1) * ld;      // a row past the end reads the last one, stores nothing
            float acc[PS_G];
            if (L == 0) {
#pragma unroll
                for (int g = 0; g < PS_G; ++g) acc[g] = xr[g][n];
            } else {
#pragma unroll
                for (int g = 0; g < PS_G; ++g) acc[g] = 0.0f;
                int next = anc_nodes[o];
                for (int j = 0; j < L; ++j) {
                    const int a = next;
                    if (j + 1 < L) next = anc_nodes[o + j + 1];               // the next id is on its way while this one's gathers are
                    if ((unsigned)a < (unsigned)n_nodes) {
                        const float wj = w[j];
#pragma unroll
                        for (int g = 0; g < PS_G; ++g) acc[g] = __builtin_fmaf(wj, xr[g][a], acc[g]);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < PS_G; ++g)
                if (r0 + g < rend) s[(r0 + g) * ld_out + n] = acc[g];
        }
    }
}

}  // namespace

extern "C" int hgr_path_scores(const float *logits, int64_t ld, float *scores, int64_t ld_out, int n_nodes, const int32_t *anc_ptr,
                               const int32_t *anc_nodes, const float *wtab, int rows, void *stream) {
    HGR_REQUIRE(logits && scores && anc_ptr && anc_nodes && wtab, "hgr_path_scores: null operand");
    HGR_REQUIRE(rows >= 1 && n_nodes >= 1 && ld >= n_nodes && ld_out >= n_nodes, "hgr_path_scores: bad sizes rows=%d n_nodes=%d ld=%lld ld_out=%lld",
                rows, n_nodes, (long long)ld, (long long)ld_out);
    // the gathers read other columns of the row: in place is wrong, and so is any overlap of the two [rows, ld] ranges
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(logits), x1 = x0 + (uintptr_t)rows * (uintptr_t)ld * sizeof(float);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(scores), s1 = s0 + (uintptr_t)rows * (uintptr_t)ld_out * sizeof(float);
    HGR_REQUIRE(x1 <= s0 || s1 <= x0, "hgr_path_scores: scores overlaps logits (the gathers read other columns of the row)");
    const int64_t gy = ((int64_t)rows - 1) / PS_ROWS + 1;
    const dim3 grid((unsigned)(((int64_t)n_nodes - 1) / PS_NT + 1), (unsigned)(gy < PS_MAXGRID_Y ? gy : PS_MAXGRID_Y));
    hipLaunchKernelGGL(path_scores, grid, dim3(PS_NT), 0, (hipStream_t)stream, logits, ld, scores, ld_out, n_nodes, anc_ptr, anc_nodes, wtab, rows);
    HGR_CHECK_LAUNCH("hgr_path_scores");
    return HGR_OK;
}
