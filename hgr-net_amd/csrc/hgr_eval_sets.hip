// Candidate sets (include/hgr.h, hgr_set_ranks and hgr_set_counters_rows): one more pass over the scores row hgr_eval_rows got answers
// up to 16 candidate sets at once - per set the rank of the row's own class among the set's columns and the set's best column - and a
// second small kernel adds the counters of every set to an int64 table kept apart by the target's path length.  Integer outputs only:
// counts and column ids depend on no lane, workgroup, row order or cut into launches.
#include "hgr_common.h"

namespace {

// Threads per row.  Up to 4 sets: 8 waves (at N = 21 841, batch 512 on an MI355X: 65 us against 110 us with 4 waves - the kernel waits
// on its loads, more waves hide them); 8 and 16 sets: 4 waves (16 sets: 134 us against 142 us with 8 waves - the reduction of 16 counters
// and keys per wave outweighs them; 16 waves would hold the 16-set registers only with scratch).  profiles/NOTES.md, "Candidate sets".
template <int S> constexpr int sr_nt() { return S <= 4 ? 512 : 256; }
constexpr int SR_MAXGRID = 1024;     // rows beyond it are taken in further rounds by the same workgroups
constexpr int SR_MAXS = HGR_SETS_MAXS;

// signed order of the tie key, reversed, as an unsigned: the smaller key wins the unsigned max
__device__ __forceinline__ unsigned tie_low(int tk) { return ~((unsigned)tk ^ 0x80000000u); }

// One row.  S = the number of sets the registers are laid out for (n_sets <= S, the bits behind n_sets are masked away).  Per lane and
// set: cnt = members seen that are before the target, key = the best member seen as (orderable(x + 0.0f) << 32) | tie_low(tie_key), col
// its column.  0 is "no member yet": every finite score has orderable bits > 0.
template <int S> struct SetRow {
    unsigned cnt[S];
    unsigned long long key[S];
    int col[S];
    float tx;                        // the target's score
    int t, tkt;                      // the target's column (-1: no rank is taken) and its tie key
    const int32_t *__restrict__ tie_key;

    __device__ __forceinline__ void visit(int c, float x, unsigned m) {
        if (m == 0u) return;                                                  // a column of no set
        const unsigned ov = orderable(x + 0.0f);                              // -0 -> +0: the bit order must agree with the compare
        unsigned need = 0u;                                                   // sets whose best this column may replace
#pragma unroll
        for (int s = 0; s < S; ++s) need |= (unsigned)(((m >> s) & 1u) & (unsigned)(ov >= (unsigned)(key[s] >> 32))) << s;
        const bool tie = t >= 0 && x == tx && c != t;
        unsigned beat = (t >= 0 && x > tx) ? m : 0u;
        if (need | (unsigned)tie) {                                           // rare: a lane's best changes O(log n) times on unordered data
            const int tk = tie_key[c];
            if (tie && tk < tkt) beat = m;
            const unsigned long long k = ((unsigned long long)ov << 32) | tie_low(tk);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (((need >> s) & 1u) && k > key[s]) { key[s] = k; col[s] = c; }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) cnt[s] += (beat >> s) & 1u;
    }
};

template <int S>
__global__ __launch_bounds__(sr_nt<S>()) void set_ranks(const float *__restrict__ x, int64_t ld, int n_nodes, const uint32_t *__restrict__ member,
                                                   const int32_t *__restrict__ tie_key, int n_sets, const int64_t *__restrict__ targets,
                                                   int32_t *__restrict__ rank, int32_t *__restrict__ top1, int rows) {
    constexpr int SR_NT = sr_nt<S>(), SR_WAVES = SR_NT / HGR_WAVE;
    __shared__ unsigned s_cnt[SR_WAVES][S];
    __shared__ unsigned long long s_key[SR_WAVES][S];
    __shared__ int s_col[SR_WAVES][S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned mask = n_sets >= 32 ? 0xFFFFFFFFu : (1u << n_sets) - 1u;
    const bool mvec = (reinterpret_cast<uintptr_t>(member) & 15) == 0;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float *xr = x + r * ld;
        SetRow<S> st;
        st.tie_key = tie_key;
#pragma unroll
        for (int s = 0; s < S; ++s) { st.cnt[s] = 0u; st.key[s] = 0ull; st.col[s] = -1; }
        // the target's score, tie key and member word, once per row; no rank is taken when it lies in none of the sets
        unsigned tm = 0u;
        st.t = -1; st.tx = 0.0f; st.tkt = 0;
        if (targets) {
            const int64_t t64 = targets[r];
            if (t64 >= 0 && t64 < (int64_t)n_nodes) {
                tm = member[t64] & mask;
                if (tm) { st.t = (int)t64; st.tx = xr[t64]; st.tkt = tie_key[t64]; }
            }
        }
        if (mvec && (reinterpret_cast<uintptr_t>(xr) & 15) == 0) {                                // 16-byte loads: four columns per lane and step
            const int n4 = n_nodes >> 2;
            const f32x4 *x4 = reinterpret_cast<const f32x4 *>(xr);
            const u32x4 *m4 = reinterpret_cast<const u32x4 *>(member);
            for (int i = tid; i < n4; i += SR_NT) {
                const f32x4 xv = x4[i];
                const u32x4 mv = m4[i];
                st.visit(4 * i + 0, xv[0], mv[0] & mask);
                st.visit(4 * i + 1, xv[1], mv[1] & mask);
                st.visit(4 * i + 2, xv[2], mv[2] & mask);
                st.visit(4 * i + 3, xv[3], mv[3] & mask);
            }
            const int c = 4 * n4 + tid;                                       // the last n_nodes % 4 columns
            if (c < n_nodes) st.visit(c, xr[c], member[c] & mask);
        } else {
            for (int c = tid; c < n_nodes; c += SR_NT) st.visit(c, xr[c], member[c] & mask);
        }
        // the wave's counts and best keys (shuffles), then the waves' through LDS
#pragma unroll
        for (int s = 0; s < S; ++s) {
            unsigned v = st.cnt[s];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            const unsigned long long b = wave_max_u64(st.key[s]);
            if (lane == 0) { s_cnt[wave][s] = v; s_key[wave][s] = b; }
            if (b == 0ull ? lane == 0 : st.key[s] == b) s_col[wave][s] = b == 0ull ? -1 : st.col[s];      // keys of a set are distinct: one lane
        }
        __syncthreads();
        if (tid < n_sets && tid < S) {
            unsigned v = 0u;
            unsigned long long b = 0ull;
            int c = -1;
#pragma unroll
            for (int w = 0; w < SR_WAVES; ++w) {
                v += s_cnt[w][tid];
                if (s_key[w][tid] > b) { b = s_key[w][tid]; c = s_col[w][tid]; }
            }
            top1[r * n_sets + tid] = c;
            if (targets) rank[r * n_sets + tid] = ((tm >> tid) & 1u) ? (int)v : -1;
        }
        __syncthreads();                                                      // the next row rewrites the scratch
    }
}

template <int S>
void launch_set_ranks(const float *scores, int64_t ld, int n_nodes, const uint32_t *member, const int32_t *tie_key, int n_sets,
                      const int64_t *targets, int32_t *rank, int32_t *top1, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(set_ranks<S>, dim3(rows < SR_MAXGRID ? rows : SR_MAXGRID), dim3(sr_nt<S>()), 0, stream, scores, ld, n_nodes, member, tie_key,
                       n_sets, targets, rank, top1, rows);
}

// ---- the counters of every set ----------------------------------------------------------------------------------------------------------
constexpr int SC_NT = 512;           // 8 waves, ONE ROW PER WAVE: lane i < 32 holds position i of the target's path
constexpr int SC_WAVES = SC_NT / HGR_WAVE;
constexpr int SC_MAXGRID = 8;
constexpr int SC_MAXL = HGR_REPORT_MAXL;
constexpr int SC_SET = (SC_MAXL + 1) * HGR_SETS_COLS;                         // one set's table
constexpr int SC_LEN = SR_MAXS * SC_SET;

__global__ __launch_bounds__(SC_NT) void set_counters_rows(const int32_t *__restrict__ rank, const int32_t *__restrict__ top1, int n_sets,
                                                           const int64_t *__restrict__ targets, const int32_t *__restrict__ lv, int n_levels,
                                                           const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes,
                                                           const int32_t *__restrict__ anc_levels, int n_nodes,
                                                           unsigned long long *__restrict__ table, int rows) {
    __shared__ unsigned long long s_tab[SC_LEN];                              // this block's counts of this launch, table layout
    const int len = n_sets * SC_SET;
    for (int i = threadIdx.x; i < len; i += SC_NT) s_tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * SC_WAVES + wave; r < rows; r += (int64_t)gridDim.x * SC_WAVES) {
        const int64_t t64 = targets[r];
        if (t64 < 0 || t64 >= (int64_t)n_nodes) continue;                     // padding row (wave-uniform)
        const int tgt = (int)t64;
        const int o = anc_ptr[tgt];
        const int L = anc_ptr[tgt + 1] - o;
        if (L < 1 || L > SC_MAXL) continue;                                   // the same rule as hgr_eval_counters_rows
        const bool live = lane < L;
        const int pa = live ? anc_nodes[o + lane] : -1;
        const int le = live ? anc_levels[o + lane] : -1;
        const int q = level_pick(lv + r * n_levels, n_levels, le);
        const unsigned mm = (unsigned)__ballot(live && q == pa);              // path positions matched by their level's arg-max
        const unsigned point = __popc(mm), edge = path_edges(mm, L);
        for (int s = 0; s < n_sets; ++s) {
            const int rk = rank[r * n_sets + s];                              // wave-uniform
            if (rk < 0) continue;                                             // the target is no member of this set
            const int t1 = top1[r * n_sets + s];
            const unsigned hh = (unsigned)__ballot(live && pa == t1);
            const unsigned v = lane == 0 ? 1u : lane == 1 ? (unsigned)(rk < 1) : lane == 2 ? (unsigned)(rk < 2) : lane == 3 ? (unsigned)(rk < 5)
                             : lane == 4 ? (unsigned)(rk < 10) : lane == 5 ? (unsigned)(rk < 20) : lane == 6 ? (unsigned)__popc(hh)
                             : lane == 7 ? point : lane == 8 ? edge : 0u;
            if (lane < HGR_SETS_COLS && v) atomicAdd(&s_tab[s * SC_SET + L * HGR_SETS_COLS + lane], (unsigned long long)v);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += SC_NT) {                          // one flush per block: integer adds, any order
        const unsigned long long s = s_tab[i];
        if (s) atomicAdd(&table[i], s);
    }
}

}  // namespace

extern "C" int hgr_set_ranks(const float *scores, int64_t ld, int n_nodes, const uint32_t *member, const int32_t *tie_key, int n_sets,
                             const int64_t *targets, int32_t *rank, int32_t *top1, int rows, void *stream) {
    HGR_REQUIRE(scores && member && tie_key && top1, "hgr_set_ranks: null operand (targets is optional, rank only without targets)");
    HGR_REQUIRE(!targets || rank, "hgr_set_ranks: targets without a rank buffer");
    HGR_REQUIRE(rows >= 1 && n_nodes >= 1 && ld >= n_nodes, "hgr_set_ranks: bad sizes rows=%d n_nodes=%d ld=%lld", rows, n_nodes, (long long)ld);
    HGR_REQUIRE(n_sets >= 1 && n_sets <= SR_MAXS, "hgr_set_ranks: %d sets (1..%d)", n_sets, SR_MAXS);
    hipStream_t st = (hipStream_t)stream;
    if (n_sets == 1) launch_set_ranks<1>(scores, ld, n_nodes, member, tie_key, n_sets, targets, rank, top1, rows, st);
    else if (n_sets == 2) launch_set_ranks<2>(scores, ld, n_nodes, member, tie_key, n_sets, targets, rank, top1, rows, st);
    else if (n_sets <= 4) launch_set_ranks<4>(scores, ld, n_nodes, member, tie_key, n_sets, targets, rank, top1, rows, st);
    else if (n_sets <= 8) launch_set_ranks<8>(scores, ld, n_nodes, member, tie_key, n_sets, targets, rank, top1, rows, st);
    else launch_set_ranks<16>(scores, ld, n_nodes, member, tie_key, n_sets, targets, rank, top1, rows, st);
    HGR_CHECK_LAUNCH("hgr_set_ranks");
    return HGR_OK;
}

extern "C" int hgr_set_counters_rows(const int32_t *rank, const int32_t *top1, int n_sets, const int64_t *targets, const int32_t *lv, int n_levels,
                                     const int32_t *anc_ptr, const int32_t *anc_nodes, const int32_t *anc_levels, int n_nodes,
                                     int64_t *table, int rows, void *stream) {
    HGR_REQUIRE(rank && top1 && targets && lv && anc_ptr && anc_nodes && anc_levels && table, "hgr_set_counters_rows: null operand");
    HGR_REQUIRE(rows >= 1 && n_nodes >= 1 && n_levels >= 1 && n_levels <= SC_MAXL, "hgr_set_counters_rows: bad sizes rows=%d n_nodes=%d n_levels=%d (<= 32)",
                rows, n_nodes, n_levels);
    HGR_REQUIRE(n_sets >= 1 && n_sets <= SR_MAXS, "hgr_set_counters_rows: %d sets (1..%d)", n_sets, SR_MAXS);
    const int need = (rows - 1) / SC_WAVES + 1;
    hipLaunchKernelGGL(set_counters_rows, dim3(need < SC_MAXGRID ? need : SC_MAXGRID), dim3(SC_NT), 0, (hipStream_t)stream, rank, top1, n_sets, targets,
                       lv, n_levels, anc_ptr, anc_nodes, anc_levels, n_nodes, reinterpret_cast<unsigned long long *>(table), rows);
    HGR_CHECK_LAUNCH("hgr_set_counters_rows");
    return HGR_OK;
}
