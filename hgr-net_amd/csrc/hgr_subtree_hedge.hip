// Hedged predictions (include/hgr.h, hgr_subtree_hedge and hgr_hedge_counters_rows): the softmax of a class row in 2^-30 fixed point,
// every node's subtree mass as a uint32 sum scattered up the ancestor CSR, and per threshold the deepest node whose mass reaches it.
// The mass row of one logits row lives in LDS for the whole row: one workgroup per row, the logits are read three times (maximum,
// normaliser, scatter), the masses never leave the CU unless the caller asks for them.  Given q the masses are integer sums: they
// depend on no order, lane or launch; the normaliser is added in an order fixed by n_nodes alone, the same for every row.
#include <math.h>

#include "hgr_common.h"

namespace {

constexpr int SH_NT = 1024;          // 16 waves: at N = 21 841 the mass row (87 KB) leaves room for ONE workgroup per CU - its waves hide the latency
constexpr int SH_WAVES = SH_NT / HGR_WAVE;
constexpr int SH_MAXGRID = 1024;     // rows beyond it are taken in further rounds by the same workgroups
constexpr int SH_MAXT = HGR_HEDGE_MAXT;
constexpr int SH_MAXL = HGR_REPORT_MAXL;
constexpr float SH_ONE = 1073741824.0f;        // 2^30
constexpr float SH_INV = 9.313225746154785e-10f;   // 2^-30

// e[n] of the definition: a difference, a product and expf, one rounding each - the normaliser pass and the scatter pass call this one
// function, so both see the same bits
__device__ __forceinline__ float hedge_exp(float x, float m, float tau) { return expf(tau * (x - m)); }

__global__ __launch_bounds__(SH_NT) void subtree_hedge(const float *__restrict__ x, int64_t ld, int n_nodes, const int32_t *__restrict__ cand_pos,
                                                       const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes, float tau,
                                                       const uint32_t *__restrict__ thr, int T, int32_t *__restrict__ pick,
                                                       float *__restrict__ pick_mass, uint32_t *__restrict__ mass_out, int64_t ld_mass, int rows) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mass[];         // [n_nodes]: the row's masses
    __shared__ float s_f[SH_WAVES];
    __shared__ uint32_t s_u[SH_WAVES];
    __shared__ unsigned long long s_key[SH_WAVES][SH_MAXT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the thresholds, one register each (a threshold behind T is never reached: a row's total stays below 2^31)
    uint32_t th[SH_MAXT];
#pragma unroll
    for (int i = 0; i < SH_MAXT; ++i) th[i] = i < T ? thr[i] : 0xFFFFFFFFu;

    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float *xr = x + r * ld;
        // pass 1: the maximum over the candidates; the mass row is cleared on the way
        float m = -INFINITY;
        for (int n = tid; n < n_nodes; n += SH_NT) {
            s_mass[n] = 0u;
            if (!cand_pos || cand_pos[n] >= 0) m = fmaxf(m, xr[n]);
        }
        m = wave_max(m);
        if (lane == 0) s_f[wave] = m;
        __syncthreads();
        m = s_f[0];
#pragma unroll
        for (int w = 1; w < SH_WAVES; ++w) m = fmaxf(m, s_f[w]);
        __syncthreads();                                                      // s_f is written again below
        // pass 2: the normaliser; lane partial sums over n = tid, tid + 1024, ..., then the wave's tree, then the 16 waves in order
        float z = 0.0f;
        for (int n = tid; n < n_nodes; n += SH_NT)
            if (!cand_pos || cand_pos[n] >= 0) z += hedge_exp(xr[n], m, tau);
        z = wave_sum(z);
        if (lane == 0) s_f[wave] = z;
        __syncthreads();                                                      // also: the cleared mass row is visible to every wave
        z = s_f[0];
#pragma unroll
        for (int w = 1; w < SH_WAVES; ++w) z += s_f[w];
        // pass 3: the scatter, one candidate per lane up its path
        uint32_t total = 0u;
        for (int n = tid; n < n_nodes; n += SH_NT) {
            if (cand_pos && cand_pos[n] < 0) continue;
            const uint32_t q = (uint32_t)rintf(hedge_exp(xr[n], m, tau) / z * SH_ONE);
            if (q == 0u) continue;
            total += q;
            const int o = anc_ptr[n];
            const int L = anc_ptr[n + 1] - o;
            if (L < 1 || L > SH_MAXL) {
                atomicAdd(&s_mass[n], q);
                continue;
            }
            for (int j = 0; j < L; ++j) {
                const int a = anc_nodes[o + j];
                if ((unsigned)a < (unsigned)n_nodes) atomicAdd(&s_mass[a], q);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        if (lane == 0) s_u[wave] = total;
        __syncthreads();                                                      // the masses are complete
        // pass 4: per threshold the largest key L << 47 | mass << 16 | (0xFFFF - id) among the nodes that reach it
        unsigned long long best[SH_MAXT];
#pragma unroll
        for (int i = 0; i < SH_MAXT; ++i) best[i] = 0ull;
        for (int n = tid; n < n_nodes; n += SH_NT) {
            const uint32_t ms = s_mass[n];
            if (mass_out) mass_out[r * ld_mass + n] = ms;
            const int L = anc_ptr[n + 1] - anc_ptr[n];
            if (L < 1 || L > SH_MAXL) continue;
            const unsigned long long key = ((unsigned long long)L << 47) | ((unsigned long long)ms << 16) | (unsigned long long)(0xFFFF - n);
#pragma unroll
            for (int i = 0; i < SH_MAXT; ++i)
                if (ms >= th[i] && key > best[i]) best[i] = key;
        }
#pragma unroll
        for (int i = 0; i < SH_MAXT; ++i) {
            const unsigned long long b = wave_max_u64(best[i]);
            if (lane == 0) s_key[wave][i] = b;
        }
        __syncthreads();
        if (tid < T) {
            unsigned long long b = s_key[0][tid];
            for (int w = 1; w < SH_WAVES; ++w) b = s_key[w][tid] > b ? s_key[w][tid] : b;
            uint32_t all = 0u;
            for (int w = 0; w < SH_WAVES; ++w) all += s_u[w];
            // a valid key is never 0 (L >= 1)
            pick[r * T + tid] = b ? 0xFFFF - (int)(b & 0xFFFFull) : -1;
            pick_mass[r * T + tid] = (float)(b ? (uint32_t)((b >> 16) & 0x7FFFFFFFull) : all) * SH_INV;
        }
        __syncthreads();                                                      // the next row clears s_mass and rewrites the scratch
    }
}

// ---- the outcome counters of the picks ------------------------------------------------------------------------------------------------
constexpr int HC_NT = 512;           // 8 waves, ONE ROW PER WAVE: lane i < 32 holds position i of the target's path
constexpr int HC_WAVES = HC_NT / HGR_WAVE;
constexpr int HC_MAXGRID = 8;
constexpr int HC_LEN = SH_MAXT * HGR_HEDGE_COLS;

__device__ __forceinline__ int hc_prefix_len(unsigned m) { return m == 0xFFFFFFFFu ? 32 : __builtin_ctz(~m); }

__global__ __launch_bounds__(HC_NT) void hedge_counters_rows(const int32_t *__restrict__ pick, int T, const int64_t *__restrict__ targets,
                                                             const int32_t *__restrict__ anc_ptr, const int32_t *__restrict__ anc_nodes,
                                                             int n_nodes, unsigned long long *__restrict__ table, int rows) {
    __shared__ unsigned long long s_tab[HC_LEN];                              // this block's counts of this launch, table layout
    const int len = T * HGR_HEDGE_COLS;
    for (int i = threadIdx.x; i < len; i += HC_NT) s_tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * HC_WAVES + wave; r < rows; r += (int64_t)gridDim.x * HC_WAVES) {
        const int64_t t64 = targets[r];
        if (t64 < 0 || t64 >= (int64_t)n_nodes) continue;                     // padding row (wave-uniform)
        const int tgt = (int)t64;
        const int ot = anc_ptr[tgt];
        const int Lt = anc_ptr[tgt + 1] - ot;
        if (Lt < 1 || Lt > SH_MAXL) continue;                                 // the same rule as hgr_eval_counters_rows
        const int pa = lane < Lt ? anc_nodes[ot + lane] : -1;
        for (int i = 0; i < T; ++i) {
            const int x = pick[r * T + i];                                    // wave-uniform
            int ox = 0, Lx = 0;
            if ((unsigned)x < (unsigned)n_nodes) {
                ox = anc_ptr[x];
                Lx = anc_ptr[x + 1] - ox;
                if (Lx < 1 || Lx > SH_MAXL) Lx = 0;
            }
            const bool in = lane < Lx && lane < Lt;
            const int px = in ? anc_nodes[ox + lane] : -1;
            const int c = hc_prefix_len((unsigned)__ballot(in && px == pa));
            if (lane == 0) {
                const int col = x == -1 ? HGR_HEDGE_COL_ABSTAIN : Lx == 0 ? HGR_HEDGE_COL_WRONG : x == tgt ? HGR_HEDGE_COL_EXACT
                              : (c == Lx && Lx < Lt) ? HGR_HEDGE_COL_ANCESTOR : (c == Lt && Lt < Lx) ? HGR_HEDGE_COL_BELOW : HGR_HEDGE_COL_WRONG;
                unsigned long long *row = s_tab + i * HGR_HEDGE_COLS;
                atomicAdd(&row[HGR_HEDGE_COL_ROWS], 1ull);
                atomicAdd(&row[col], 1ull);
                if (Lx) atomicAdd(&row[HGR_HEDGE_COL_SUM_LPICK], (unsigned long long)Lx);
                if (c) atomicAdd(&row[HGR_HEDGE_COL_SUM_COMMON], (unsigned long long)c);
                atomicAdd(&row[HGR_HEDGE_COL_SUM_LT], (unsigned long long)Lt);
                atomicAdd(&row[HGR_HEDGE_COL_HIST + Lx], 1ull);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += HC_NT) {                          // one flush per block: integer adds, any order
        const unsigned long long s = s_tab[i];
        if (s) atomicAdd(&table[i], s);
    }
}

}  // namespace

extern "C" int hgr_subtree_hedge(const float *scores, int64_t ld, int n_nodes, const int32_t *cand_pos, const int32_t *anc_ptr,
                                 const int32_t *anc_nodes, float temperature, const uint32_t *thr, int n_thr, int32_t *pick, float *pick_mass,
                                 uint32_t *mass_out, int64_t ld_mass, int rows, void *stream) {
    HGR_REQUIRE(scores && anc_ptr && anc_nodes && thr && pick && pick_mass, "hgr_subtree_hedge: null operand (cand_pos and mass_out are optional)");
    HGR_REQUIRE(rows >= 1 && n_nodes >= 1 && n_nodes <= HGR_HEDGE_MAXN && ld >= n_nodes && (!mass_out || ld_mass >= n_nodes),
                "hgr_subtree_hedge: bad sizes rows=%d n_nodes=%d (<= %d) ld=%lld ld_mass=%lld", rows, n_nodes, HGR_HEDGE_MAXN, (long long)ld,
                (long long)ld_mass);
    HGR_REQUIRE(n_thr >= 1 && n_thr <= HGR_HEDGE_MAXT, "hgr_subtree_hedge: %d thresholds (1..%d)", n_thr, HGR_HEDGE_MAXT);
    HGR_REQUIRE(isfinite(temperature) && temperature > 0.0f, "hgr_subtree_hedge: temperature %g (finite, > 0)", (double)temperature);
    static bool granted = false;                 // once: the largest mass row, beyond the 64 KB a kernel gets without asking
    if (!granted) {
        hipError_t e = hipFuncSetAttribute((const void *)subtree_hedge, hipFuncAttributeMaxDynamicSharedMemorySize, HGR_HEDGE_MAXN * 4);
        if (e != hipSuccess) return hgr_set_error(HGR_ELAUNCH, "hgr_subtree_hedge: cannot reserve %d B of LDS: %s", HGR_HEDGE_MAXN * 4, hipGetErrorString(e));
        granted = true;
    }
    const size_t bytes = ((size_t)n_nodes * 4 + 15) & ~(size_t)15;
    hipLaunchKernelGGL(subtree_hedge, dim3(rows < SH_MAXGRID ? rows : SH_MAXGRID), dim3(SH_NT), bytes, (hipStream_t)stream, scores, ld, n_nodes,
                       cand_pos, anc_ptr, anc_nodes, temperature, thr, n_thr, pick, pick_mass, mass_out, ld_mass, rows);
    HGR_CHECK_LAUNCH("hgr_subtree_hedge");
    return HGR_OK;
}

extern "C" int hgr_hedge_counters_rows(const int32_t *pick, int n_thr, const int64_t *targets, const int32_t *anc_ptr, const int32_t *anc_nodes,
                                       int n_nodes, int64_t *table, int rows, void *stream) {
    HGR_REQUIRE(pick && targets && anc_ptr && anc_nodes && table, "hgr_hedge_counters_rows: null operand");
    HGR_REQUIRE(rows >= 1 && n_nodes >= 1 && n_thr >= 1 && n_thr <= HGR_HEDGE_MAXT, "hgr_hedge_counters_rows: bad sizes rows=%d n_nodes=%d n_thr=%d (1..%d)",
                rows, n_nodes, n_thr, HGR_HEDGE_MAXT);
    const int need = (rows - 1) / HC_WAVES + 1;
    hipLaunchKernelGGL(hedge_counters_rows, dim3(need < HC_MAXGRID ? need : HC_MAXGRID), dim3(HC_NT), 0, (hipStream_t)stream, pick, n_thr, targets,
                       anc_ptr, anc_nodes, n_nodes, reinterpret_cast<unsigned long long *>(table), rows);
    HGR_CHECK_LAUNCH("hgr_hedge_counters_rows");
    return HGR_OK;
}
