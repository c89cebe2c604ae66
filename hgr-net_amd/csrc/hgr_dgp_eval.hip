// Scoring of DGP's predicted classifiers (include/hgr.h, hgr_dgp_score_rows; the reference's baseline/DGP/evaluate_imagenet.py
// and evaluate_21kp.py, test_on_subset): one pass over a row of the classifier product gives the target's rank by COUNTING
// (#columns >= the target's score, ties against the target), the row's top-1 and the arg-max of every depth level with the reference's
// -1 filler, all on the table as the reference scores it - the leading seen columns read as one constant.  Integer outputs only: they
// depend on no lane, wave or launch order.  The order "larger value, then lower column" is the 64-bit key of hgr_common.h (key_of),
// reduced with wave_max_u64; the filler competes as the key of (-1, first column outside the level).
#include "hgr_common.h"

namespace {

// Threads per row: 8 waves up to 16 levels, 4 waves up to 32 - 64 KB of per-thread level keys either way (two rows per CU; a batch of
// 512 rows is one round of the chip, and the kernel waits on its loads: more waves per row hide them)
template <int NLV> constexpr int ds_nt() { return NLV <= 16 ? 512 : 256; }
constexpr int DS_MAXGRID = 1024;        // rows beyond it are taken in further rounds by the same workgroups
constexpr int DS_MAXL = 32;

template <typename T> struct DsVec;
template <> struct DsVec<_Float16> { typedef f16x8 vec; static constexpr int N = 8; };
template <> struct DsVec<float> { typedef f32x4 vec; static constexpr int N = 4; };

// dynamic LDS: acc[NLV][threads] (per thread and level the best key seen, 0 = none; the thread's own column, so no two lanes share a
// word and a 64-bit access is conflict-free) | s_key[32] | s_top[DS_NW] | s_cnt[DS_NW] | s_fd[DS_NW]
template <int NLV> constexpr size_t ds_lds_bytes() { return (size_t)NLV * ds_nt<NLV>() * 8 + DS_MAXL * 8 + (ds_nt<NLV>() / HGR_WAVE) * 16; }

template <typename T, int NLV>
__global__ __launch_bounds__(ds_nt<NLV>()) void dgp_score_rows(const T *__restrict__ table, int64_t ld, int n_cols, int n_masked, float mask_value,
                                                        const int32_t *__restrict__ depth, int n_levels, const int64_t *__restrict__ targets,
                                                        int target, int32_t *__restrict__ rank, int32_t *__restrict__ top1,
                                                        int32_t *__restrict__ lv, int32_t *__restrict__ pred, int k_pred, int rows) {
    constexpr int DS_NT = ds_nt<NLV>(), DS_NW = DS_NT / HGR_WAVE;
    extern __shared__ __attribute__((aligned(16))) char ds_dyn[];
    unsigned long long *acc = (unsigned long long *)ds_dyn;
    unsigned long long *s_key = acc + NLV * DS_NT;
    unsigned long long *s_top = s_key + DS_MAXL;
    unsigned *s_cnt = (unsigned *)(s_top + DS_NW);
    int *s_fd = (int *)(s_cnt + DS_NW);
    typedef typename DsVec<T>::vec vec;
    constexpr int VN = DsVec<T>::N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float mv = mask_value + 0.0f;
    const int lvl0 = depth[0];
    const bool dvec = (reinterpret_cast<uintptr_t>(depth) & 15) == 0;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const T *xr = table + r * ld;
        const int64_t t64 = targets ? targets[r] : (int64_t)target;
        const bool tok = t64 >= 0 && t64 < (int64_t)n_cols;
        const int t = tok ? (int)t64 : 0;
        const float tv = (t < n_masked ? mv : (float)xr[t]) + 0.0f;         // masking applies to the target too
#pragma unroll
        for (int l = 0; l < NLV; ++l) acc[l * DS_NT + tid] = 0ull;
        unsigned cnt = 0u;
        unsigned long long top = 0ull;
        int fd = 0x7fffffff;                                                  // first column whose level differs from column 0's
        auto visit = [&](int c, float x, int d) {
            const float v = (c < n_masked ? mv : x) + 0.0f;                   // -0 -> +0: the key's bit order must agree with the compare
            cnt += v >= tv ? 1u : 0u;
            const unsigned long long key = key_of(v, c);
            top = key > top ? key : top;
            if (d != lvl0 && c < fd) fd = c;
            if ((unsigned)d < (unsigned)n_levels) {                          // n_levels <= NLV: the slot exists
                unsigned long long *slot = &acc[d * DS_NT + tid];
                if (key > *slot) *slot = key;
            }
        };
        if (dvec && (reinterpret_cast<uintptr_t>(xr) & 15) == 0) {            // 16-byte loads: VN columns per lane and step
            const int nv = n_cols / VN;
            const vec *xv = reinterpret_cast<const vec *>(xr);
            const u32x4 *dv = reinterpret_cast<const u32x4 *>(depth);
            for (int i = tid; i < nv; i += DS_NT) {
                const vec x = xv[i];
                u32x4 d[VN / 4];
#pragma unroll
                for (int q = 0; q < VN / 4; ++q) d[q] = dv[i * (VN / 4) + q];
#pragma unroll
                for (int e = 0; e < VN; ++e) visit(VN * i + e, (float)x[e], (int)d[e >> 2][e & 3]);
            }
            const int c = VN * nv + tid;                                      // the last n_cols % VN columns
            if (c < n_cols) visit(c, (float)xr[c], depth[c]);
        } else {
            for (int c = tid; c < n_cols; c += DS_NT) visit(c, (float)xr[c], depth[c]);
        }
        // the wave's count, best key and first other-level column (shuffles), then the waves' through LDS
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); fd = min(fd, __shfl_xor(fd, o)); }
        top = wave_max_u64(top);
        if (lane == 0) { s_cnt[wave] = cnt; s_top[wave] = top; s_fd[wave] = fd; }
        __syncthreads();
        for (int l = wave; l < n_levels; l += DS_NW) {                        // wave w reduces levels w, w + DS_NW, ...: DS_NT keys each
            unsigned long long m = 0ull;
#pragma unroll
            for (int i = 0; i < DS_NT / 64; ++i) { const unsigned long long x = acc[l * DS_NT + lane + 64 * i]; m = x > m ? x : m; }
            m = wave_max_u64(m);
            if (lane == 0) s_key[l] = m;
        }
        __syncthreads();
        if (tid < n_levels) {
            // the reference fills every column outside level l with -1 before its arg-max, so the filler competes: its first column is
            // column 0, or - when column 0 is on level l - the first column of another level (none: the level holds every column)
            const int l = tid;
            int fo = 0;
            if (l == lvl0) { fo = s_fd[0]; for (int w = 1; w < DS_NW; ++w) fo = min(fo, s_fd[w]); }
            unsigned long long key = s_key[l];
            if (fo < n_cols) { const unsigned long long fk = key_of(-1.0f, fo); key = fk > key ? fk : key; }
            float v; int p;
            key_decode(key, v, p);
            lv[r * n_levels + l] = p;
        }
        if (wave == DS_NW - 1) {
            unsigned c = 0u;
            unsigned long long b = 0ull;
            for (int w = 0; w < DS_NW; ++w) { c += s_cnt[w]; b = s_top[w] > b ? s_top[w] : b; }
            const int rk = tok ? (int)c : 0x7fffffff;                         // a target outside the table never hits
            if (lane == 0) {
                float v; int p;
                key_decode(b, v, p);
                top1[r] = p;
                rank[r] = rk;
            }
            // the rank in the shape hgr_eval_counters reads hits from: the target at position rank - 1 of a top-k row, -1 elsewhere
            if (pred && lane < k_pred) pred[r * k_pred + lane] = (tok && lane == rk - 1) ? t : -1;
        }
        __syncthreads();                                                      // the next row rewrites the scratch
    }
}

template <typename T, int NLV>
int launch_dgp_score_rows(const void *table, int64_t ld, int n_cols, int n_masked, float mask_value, const int32_t *depth, int n_levels,
                          const int64_t *targets, int target, int32_t *rank, int32_t *top1, int32_t *lv, int32_t *pred, int k_pred, int rows,
                          hipStream_t stream) {
    constexpr size_t bytes = ds_lds_bytes<NLV>();
    static bool granted = false;
    if (bytes > 65536 && !granted) {
        hipError_t e = hipFuncSetAttribute((const void *)dgp_score_rows<T, NLV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return hgr_set_error(HGR_ELAUNCH, "hgr_dgp_score_rows: cannot reserve %zu B of LDS: %s", bytes, hipGetErrorString(e));
        granted = true;
    }
    hipLaunchKernelGGL((dgp_score_rows<T, NLV>), dim3(rows < DS_MAXGRID ? rows : DS_MAXGRID), dim3(ds_nt<NLV>()), bytes, stream, (const T *)table, ld,
                       n_cols, n_masked, mask_value, depth, n_levels, targets, target, rank, top1, lv, pred, k_pred, rows);
    HGR_CHECK_LAUNCH("hgr_dgp_score_rows");
    return HGR_OK;
}

}  // namespace

extern "C" int hgr_dgp_score_rows(const void *table, int64_t ld, int table_f32, int n_cols, int n_masked, float mask_value, const int32_t *depth,
                                  int n_levels, const int64_t *targets, int target, int32_t *rank, int32_t *top1, int32_t *lv, int32_t *pred,
                                  int k_pred, int rows, void *stream) {
    HGR_REQUIRE(table && depth && rank && top1 && lv, "hgr_dgp_score_rows: null operand");
    HGR_REQUIRE(table_f32 == 0 || table_f32 == 1, "hgr_dgp_score_rows: table_f32 must be 0 (fp16) or 1 (fp32), got %d", table_f32);
    HGR_REQUIRE(rows >= 1 && n_cols >= 1 && ld >= n_cols, "hgr_dgp_score_rows: bad sizes rows=%d n_cols=%d ld=%lld (ld >= n_cols >= 1)", rows, n_cols, (long long)ld);
    HGR_REQUIRE(n_levels >= 1 && n_levels <= DS_MAXL, "hgr_dgp_score_rows: n_levels=%d unsupported (1..32)", n_levels);
    HGR_REQUIRE(n_masked >= 0 && n_masked <= n_cols, "hgr_dgp_score_rows: n_masked=%d outside 0..n_cols=%d", n_masked, n_cols);
    HGR_REQUIRE(mask_value == mask_value, "hgr_dgp_score_rows: the mask value is NaN");
    HGR_REQUIRE(targets || (target >= 0 && target < n_cols), "hgr_dgp_score_rows: target=%d outside the %d columns", target, n_cols);
    HGR_REQUIRE(k_pred >= 0 && k_pred <= 32 && (k_pred == 0) == (pred == nullptr), "hgr_dgp_score_rows: pred needs 1 <= k_pred <= 32 (and k_pred = 0 no pred), got %d", k_pred);
    HGR_REQUIRE(hgr_aligned(table, table_f32 ? 4 : 2) && hgr_aligned(depth, 4), "hgr_dgp_score_rows: table / depth misaligned");
    hipStream_t s = (hipStream_t)stream;
    if (table_f32) {
        if (n_levels <= 16) return launch_dgp_score_rows<float, 16>(table, ld, n_cols, n_masked, mask_value, depth, n_levels, targets, target, rank, top1, lv, pred, k_pred, rows, s);
        return launch_dgp_score_rows<float, 32>(table, ld, n_cols, n_masked, mask_value, depth, n_levels, targets, target, rank, top1, lv, pred, k_pred, rows, s);
    }
    if (n_levels <= 16) return launch_dgp_score_rows<_Float16, 16>(table, ld, n_cols, n_masked, mask_value, depth, n_levels, targets, target, rank, top1, lv, pred, k_pred, rows, s);
    return launch_dgp_score_rows<_Float16, 32>(table, ld, n_cols, n_masked, mask_value, depth, n_levels, targets, target, rank, top1, lv, pred, k_pred, rows, s);
}
