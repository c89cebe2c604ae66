// How the host half of an entry point picks a template instantiation from its runtime integers, and sizes a 1-D grid.  Host only.
// A selector hands a compile-time tag to a generic lambda, so the launch line is written once:
//     hgr_by_dtype(dtype, [&](auto dt) { typedef typename decltype(dt)::elem E;
//         hipLaunchKernelGGL((relu_bwd16<dt.value>), grid, dim3(256), 0, s, (const E *)dy, (const E *)y, (E *)out, n / 8); });
// Selectors nest; only the combinations a call site spells out are instantiated.  HGR_REQUIRE / HGR_CHECK_LAUNCH return from the
// function they stand in: they stay outside the lambdas.
#pragma once
#include "hgr_common.h"

template <int V> using hgr_int = std::integral_constant<int, V>;
// the dtype tag also names the 16-bit element type: value = HGR_BF16 / HGR_F16, elem = __bf16 / _Float16
template <int DT> struct hgr_dtype_tag : hgr_int<DT> { typedef typename T16<DT>::elem elem; };

// dtype was validated by the caller's HGR_REQUIRE; anything that is not HGR_BF16 takes the f16 arm
template <typename F> inline void hgr_by_dtype(int dtype, F &&f) { if (dtype == HGR_BF16) f(hgr_dtype_tag<HGR_BF16>{}); else f(hgr_dtype_tag<HGR_F16>{}); }
template <typename F> inline void hgr_by_flag(bool on, F &&f) { if (on) f(std::true_type{}); else f(std::false_type{}); }
// slices per lane of a row kernel, rounded up to a power of two: 1, 2, 4, 8, 16 (hgr_norm.hip, hgr_train.hip)
template <typename F> inline void hgr_by_nv_pow2(int nv, F &&f) {
    if (nv <= 1) f(hgr_int<1>{}); else if (nv <= 2) f(hgr_int<2>{}); else if (nv <= 4) f(hgr_int<4>{}); else if (nv <= 8) f(hgr_int<8>{}); else f(hgr_int<16>{});
}
// float4 slices per thread of a 256-thread row kernel, exactly: 1, 2, 3, 4 (the baselines' rows of C <= 4096 columns, hgr_rows.h)
template <typename F> inline void hgr_by_nv4(int nv, F &&f) {
    if (nv == 1) f(hgr_int<1>{}); else if (nv == 2) f(hgr_int<2>{}); else if (nv == 3) f(hgr_int<3>{}); else f(hgr_int<4>{});
}
// `out_type` of hgr_free.hip: HGR_BF16, HGR_F16 or HGR_OUT_F32 (validated by the caller; anything else takes the fp32 arm)
template <typename F> inline void hgr_by_out_type(int out_type, F &&f) {
    if (out_type == HGR_BF16) f(hgr_int<HGR_BF16>{}); else if (out_type == HGR_F16) f(hgr_int<HGR_F16>{}); else f(hgr_int<HGR_OUT_F32>{});
}

// Workgroups of a grid-stride kernel: one per `per` items, at least 1, at most `cap`
static inline unsigned hgr_grid1(int64_t total, int64_t cap, int per = 256) {
    const int64_t g = (total + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}
