"""CPU: the case tables, float64 references and error bounds that tests/test_gpu_stream_kernels.py holds the streaming kernels of the
OM training step to - hgr_transpose16, hgr_transpose16_colsum, hgr_colsum, hgr_cast16, hgr_cast16_transpose, hgr_quickgelu16, hgr_sumsq,
hgr_adamw (csrc/hgr_train.hip) and hgr_bn_fold, hgr_bn_unfold_grad (csrc/hgr_train_rn.hip) - tested here without a device.

Case tables.  One table per kernel; every case names the route it is expected to take, and a pure-Python restatement of the entry point's
dispatch condition (`*_route`) must give that route.  `test_tables_reach_every_route` asserts that every route, finish and loop of every
kernel is in its table, and that every case marked grid-stride exceeds its grid cap (grid1: 256 threads x cap blocks).  Alignment is
expressed as `lead` = 0 (16-byte aligned base) or 1 (one element further: the GPU file puts the operand at lead = _G + 1).

References.  Transposition and casts are compared as bits (casts: x.to(dt) on the CPU, round to nearest even); everything else against a
float64 restatement made from the same input bits.  AdamW: torch.optim.AdamW + clip_grad_norm_ on float64 copies, from the state the
kernel was given, with the fp32-rounded scalars the kernel receives (`adamw_closed_form` restates the kernel's comment and agrees with
that optimiser to 1e-12).

Bounds.  u = 2^-24 is one fp32 rounding, relative.  Each bound below is a formula with its derivation beside it; none is taken from a
device result.  An fp32 emulation of each kernel formula (torch fp32 ops in the kernel's order) must stay inside its bound, and a
deliberately broken emulation must leave it.

Where a rounding count of the arithmetic exceeds a coefficient the bounds started from, the derived term is added and named: the relative
error r of a clipped gradient on m' and v' (adamw_bounds), the error e_f of 1 - lr wd on p', 2^-25 |mean s| on the folded bias, and the
error of s = gamma / sigma on the unfolded gradients.  The bound on p' counts on b1 m and (1 - b1) g having one sign (adamw_inputs
builds them so and the tests assert it), and every step is held against the float64 optimiser started from the state bits the kernel
was given: the bounds are those of one launch.  The f16 kernels round a product once through an FMA with a +0 addend, which gives +0 for a
-0 product: the one planted gradient that is -0 is compared by value in f16, every other x = +-0 gradient as bits.

Worst error / bound (CPU: the emulations below; MI355X: tests/test_gpu_stream_kernels.py, the worst RATIO line per kernel of one run):

    kernel                   CPU bf16  CPU f16   MI355X bf16  MI355X f16
    quickgelu forward        0.998     0.982     0.998        0.982
    quickgelu backward       0.985     0.887     0.985        0.887
    bn_fold                  0.999     0.999     0.999        0.999
                             CPU fp32            MI355X
    adamw p'                 0.862               0.520
    adamw m'                 0.461               0.350
    adamw v'                 0.486               0.519
    bn_unfold_grad           0.374               0.275
    sumsq                    0.026               0.038
    colsum rows_f32                              0.045
    colsum scalar            0.001               0.005 (fp32), 0.001 (bf16, f16)
    colsum vec                                   0.008 (fp32), 0.003 (bf16, f16)
    transpose16_colsum                           0.007 (bf16, f16)
No ratio exceeds 1.  The 16-bit rows are tight by construction (a result on a rounding tie of the type is at ratio ~ 1).  The sums sit far
below their bound because the bound is the worst case over `depth` roundings of one sign while random data errs like a random walk; the
integer cases, which are exact, are the sharp check of every band, chunk and loop, and the bound still sees one dropped row.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from hgr_net_amd import synth

from test_attention_host import BF16, F16, DTS, half_ulp16, ratio, within

F32 = torch.float32
U32 = 2.0 ** -24                       # one fp32 round-to-nearest, relative
ESIZE = {BF16: 2, F16: 2, F32: 4}


def tag(dt):
    return {BF16: "bf16", F16: "f16", F32: "f32"}[dt]


# ==== dispatch restatements ========================================================================================================
def grid1(total, per=256, cap=16384):
    """csrc/hgr_launch.h hgr_grid1(total, cap, per): blocks of `per` threads, at most `cap` of them."""
    g = (total + per - 1) // per
    return min(max(g, 1), cap)


def grid_strides(total, per=256, cap=16384):
    """Some thread of the launch makes a second trip of its grid-stride loop."""
    return total > per * cap


def base_aligned(lead, coff, dt, align=16):
    """The operand starts `lead` + `coff` elements behind a 16-byte aligned address."""
    return ((lead + coff) * ESIZE[dt]) % align == 0


def finish_route(nrb):
    """colsum_finish: the second stage over `nrb` bands of partial sums."""
    return "final" if nrb < 32 else ("deep" if nrb < 2048 else "two_level")


def deep_loops(nb):
    """Which loops of colsum_reduce_deep run for a chunk of `nb` bands: wave q starts at band q, the unrolled loop takes 16 bands per trip
    while rb + 12 < nb, the remainder loop 4 per trip."""
    seen = set()
    for q in range(4):
        rb = q
        while rb + 12 < nb:
            seen.add("unrolled")
            rb += 16
        if rb < nb:
            seen.add("remainder")
    return seen


def finish_loops(nrb):
    """Every (pass, loop) of the finish: `final`, or the loops of each colsum_reduce_deep launch; `one_band_chunk` when the last 256-band
    chunk of the two-level finish holds a single band."""
    r = finish_route(nrb)
    if r == "final":
        return {"final"}
    if r == "deep":
        return {"deep." + s for s in deep_loops(nrb)}
    n2 = (nrb + 255) // 256
    out = {"mid." + s for s in deep_loops(256)} | {"top." + s for s in deep_loops(n2)}
    last = nrb - (n2 - 1) * 256
    out |= {"mid." + s for s in deep_loops(last)}
    if last == 1:
        out.add("one_band_chunk")
    return out


def finish_depth(nrb):
    """Additions on the longest path of colsum_finish.  final: nrb in sequence.  deep: accumulator a0 of a wave takes at most
    ceil(nb / 16) + 3 bands (its share of the unrolled trips, then up to 3 remainder trips), (a0 + a1) + (a2 + a3) is 2 more, the LDS
    combine of the 4 waves 2 more."""
    deep = lambda nb: (nb + 15) // 16 + 3 + 2 + 2
    r = finish_route(nrb)
    if r == "final":
        return nrb
    if r == "deep":
        return deep(nrb)
    return deep(256) + deep((nrb + 255) // 256)


def transpose16_route(c):
    ok = c.ldx % 8 == 0 and c.ldy % 8 == 0 and base_aligned(c.lead_x, c.coff, BF16) and base_aligned(c.lead_y, 0, BF16)
    return "vec" if ok else "scalar"


def transpose16_edges(c):
    """Which arms of transpose16<CS> a vector-route case runs: whole / ragged 8-element loads (columns), whole / ragged stores (rows)."""
    e = set()
    for c0 in range(0, c.cols, 64):
        for cc in range(0, 64, 8):
            if c0 + cc < c.cols:
                e.add("load8" if c0 + cc + 7 < c.cols else "load_ragged")
    for r0 in range(0, c.rows, 64):
        for rr in range(0, 64, 8):
            if r0 + rr < c.rows:
                e.add("store8" if r0 + rr + 7 < c.rows else "store_ragged")
    if c.rows > 64 or c.cols > 64:
        e.add("blocks")
    return e


def transpose16_colsum_route(c):
    ok = c.ldx % 8 == 0 and c.ldy % 8 == 0 and base_aligned(c.lead_x, c.coff, BF16) and base_aligned(c.lead_y, 0, BF16)
    return finish_route((c.rows + 63) // 64) if ok else "refused"


def colsum_route(c):
    """hgr_colsum: (partial kernel, finish).  rows_f32 is one pass and has no finish."""
    f32 = c.dt == F32
    x_al, o_al = base_aligned(c.lead_x, c.coff, c.dt), base_aligned(c.lead_o, 0, F32)
    if f32 and c.rows <= 32 and c.cols % 4 == 0 and c.ldx % 4 == 0 and x_al and o_al:
        return "rows_f32", None
    vec = c.cols % 64 == 0 and x_al and c.ldx % (4 if f32 else 8) == 0 and c.rows >= 32
    return ("vec" if vec else "scalar"), finish_route((c.rows + 511) // 512)


def cast16_transpose_route(c):
    ok = (c.ldx % 4 == 0 and c.ldy % 8 == 0 and c.ldyt % 8 == 0 and base_aligned(c.lead_x, 0, F32) and base_aligned(c.lead_y, 0, BF16)
          and base_aligned(c.lead_t, 0, BF16))
    return "vec" if ok else "element"


def up(x, m):
    return (x + m - 1) // m * m


# ==== case tables ==================================================================================================================
# ---- hgr_transpose16: (rows, cols), ldx, coff, ldy, lead of x and y -> vec (transpose16<0>) or scalar (transpose16_scalar) --------------
def _tc(name, rows, cols, route, ldx=None, coff=0, ldy=None, lead_x=0, lead_y=0):
    return NS(name=name, rows=rows, cols=cols, ldx=cols if ldx is None else ldx, coff=coff, ldy=up(rows, 8) if ldy is None else ldy,
              lead_x=lead_x, lead_y=lead_y, route=route)


TRANSPOSE_CASES = [
    _tc("one_tile", 64, 64, "vec"),                                   # whole loads, whole stores, one block
    _tc("one_row", 1, 8, "vec"),                                      # ragged store of one row
    _tc("ragged_rows_2x2", 65, 72, "vec"),                            # a second block in both directions, one ragged row
    _tc("ragged_cols_ld72", 130, 70, "vec", ldx=72, ldy=136),         # cols % 8 = 6: the element-wise load arm
    _tc("wide_short", 7, 200, "vec"),                                 # four column blocks, ragged stores only
    _tc("column_slice", 65, 72, "vec", ldx=88, coff=8),               # x is a column slice: ldx = cols + 16, coff = 8
    _tc("ldy_up_to_64", 65, 72, "vec", ldy=128),                      # ldy = rows rounded up to 64: 63 padding columns
    _tc("odd_ldx_tiny", 3, 5, "scalar", ldx=5),                       # ldx % 8 != 0
    _tc("odd_ldx_2x2", 65, 67, "scalar", ldx=67),
    _tc("odd_ldy", 130, 72, "scalar", ldy=131),                       # ldy % 8 != 0
    _tc("x_2byte_aligned", 64, 64, "scalar", lead_x=1),               # aligned shape, x one element off
    _tc("y_2byte_aligned", 64, 64, "scalar", lead_y=1),
]

# ---- hgr_transpose16_colsum: rows -> nrb = ceil(rows / 64) -> the finish ----------------------------------------------------------------
#   rows 1, 63, 64, 65, 1984 (nrb 1, 1, 1, 2, 31): colsum_final          1985 (32): deep, unrolled loop only
#   2050 (33), 3000 (47): deep, unrolled + remainder                      131 009 (2048): two-level, top pass remainder loop only
#   131 073 (2049): two-level with a last chunk of one band
TCS_ROWS = [1, 63, 64, 65, 1984, 1985, 2050, 3000]
TCS_BIG = [131009, 131073]
TCS_RANDOM_ROWS = [65, 3000, 131073]


def _tcs(rows, cols, dt):
    return NS(name="r%d_c%d_%s" % (rows, cols, tag(dt)), rows=rows, cols=cols, dt=dt, ldx=up(cols, 8), coff=0, ldy=up(rows, 8), lead_x=0,
              lead_y=0, route=finish_route((rows + 63) // 64))


def _tcs_t(c, dt):
    """A vector-route case of TRANSPOSE_CASES through transpose16<1> (bf16) / transpose16<2> (f16): the same view of x and of y."""
    return NS(name="t_%s_%s" % (c.name, tag(dt)), rows=c.rows, cols=c.cols, dt=dt, ldx=c.ldx, coff=c.coff, ldy=c.ldy, lead_x=c.lead_x,
              lead_y=c.lead_y, route=finish_route((c.rows + 63) // 64))


def tcs_edges(c):
    """The arms of transpose16<CS != 0> a case runs: those of the transposition, and for the column sum the `c0 + threadIdx.x < cols`
    guard cutting a block's 64 lanes (`sum_guard`), a partial row stride `cols` that is no multiple of 8 (`ragged_partial`: only after an
    element-wise load), x as a column slice and padding columns in y beyond the next multiple of 8."""
    e = transpose16_edges(c)
    if c.cols % 64:
        e.add("sum_guard")
    if c.cols % 8:
        e.add("ragged_partial")
    if c.coff or c.ldx > up(c.cols, 8):
        e.add("x_slice")
    if c.ldy > up(c.rows, 8):
        e.add("ldy_padding")
    return e


# the transposition cases: every vector-route case of TRANSPOSE_CASES, both types - (64, 64); (1, 8); (65, 72); (130, 70) with ldx = 72 (the
# element-wise load arm, the sum guard at cols % 8 != 0 and a partial stride of 70); (7, 200); the coff = 8 slice; ldy up to 8 and to 64
TCS_T_CASES = [_tcs_t(c, dt) for c in TRANSPOSE_CASES if c.route == "vec" for dt in DTS]
TCS_CASES = (TCS_T_CASES + [_tcs(r, c, dt) for r in TCS_ROWS for c in (8, 72) for dt in DTS]
             + [_tcs(r, c, dt) for r in TCS_BIG for c, dt in ((8, BF16), (72, F16))])
TCS_REFUSED = [NS(name="odd_ldx", rows=65, cols=70, dt=BF16, ldx=70, coff=0, ldy=72, lead_x=0, lead_y=0, route="refused"),
               NS(name="odd_ldy", rows=65, cols=72, dt=BF16, ldx=72, coff=0, ldy=65, lead_x=0, lead_y=0, route="refused"),
               NS(name="x_misaligned", rows=64, cols=64, dt=F16, ldx=64, coff=0, ldy=64, lead_x=1, lead_y=0, route="refused"),
               NS(name="y_misaligned", rows=64, cols=64, dt=F16, ldx=64, coff=0, ldy=64, lead_x=0, lead_y=1, route="refused")]


# ---- hgr_colsum: partial route and finish ------------------------------------------------------------------------------------------------
def _cc(name, dt, rows, cols, route, finish="final", ldx=None, coff=0, lead_x=0, lead_o=0, strides=False, random=False):
    return NS(name="%s_%s_r%d_c%d" % (name, tag(dt), rows, cols), dt=dt, rows=rows, cols=cols, ldx=cols if ldx is None else ldx, coff=coff,
              lead_x=lead_x, lead_o=lead_o, route=route, finish=finish, strides=strides, random=random)


COLSUM_GRID_STRIDE_COLS = 4 * (16384 * 256) + 8
COLSUM_CASES = (
    # few fp32 rows, one pass (colsum_rows_f32): contiguous and as a column slice
    [_cc("rows", F32, r, c, "rows_f32", None, random=(r, c) == (32, 260)) for r in (1, 2, 32) for c in (4, 260, 4096)]
    + [_cc("rows_slice", F32, r, c, "rows_f32", None, ldx=c + 8) for r in (1, 2, 32) for c in (4, 260, 4096)]
    + [_cc("rows_grid_stride", F32, 1, COLSUM_GRID_STRIDE_COLS, "rows_f32", None, strides=True)]
    # every fall-through out of it
    + [_cc("fall_cols", F32, 2, 262, "scalar"),                                 # cols % 4 != 0
       _cc("fall_ldx", F32, 2, 260, "scalar", ldx=262),                         # ldx % 4 != 0
       _cc("fall_x", F32, 2, 260, "scalar", lead_x=1),                          # x 4-byte aligned only
       _cc("fall_out", F32, 2, 260, "scalar", lead_o=1),                        # out 4-byte aligned only
       _cc("fall_out_vec", F32, 32, 64, "vec", lead_o=1)]                       # ... which the vec route does not mind
    # 16-byte loads (colsum_partial_vec): a whole band is 512 rows, 16 (fp32) or 32 (16-bit) row groups
    + [_cc("vec", dt, r, c, "vec", random=(r, c) == (513, 192)) for dt in DTS for r in (32, 33, 511, 512, 513) for c in (64, 192)]
    + [_cc("vec", F32, r, c, "vec", random=(r, c) == (513, 192)) for r in (33, 511, 512, 513) for c in (64, 192)]
    + [_cc("vec_slice", dt, 33, 64, "vec", ldx=80, coff=8) for dt in (BF16, F16, F32)]
    # element loads (colsum_partial)
    + [_cc("scalar", dt, r, c, "scalar", random=(r, c) == (513, 65)) for dt in (BF16, F16, F32) for r in (1, 3, 513) for c in (1, 63, 65)]
    + [_cc("scalar_few_rows", dt, 31, 64, "scalar") for dt in DTS]               # too few rows for vec (fp32 would take rows_f32)
    + [_cc("scalar_odd_coff", dt, 33, 64, "scalar", ldx=72, coff=1) for dt in (BF16, F16, F32)]
    # the finishes through this entry: nrb = 31 (final), 32 (deep), 2048 and 2049 (two-level)
    + [_cc("finish", dt, r, 5, "scalar", f) for dt in (BF16, F16, F32) for r, f in ((15872, "final"), (15873, "deep"))]
    + [_cc("finish", dt, r, 5, "scalar", "two_level") for dt in (BF16, F16, F32) for r in (1048065, 1048577)]
    + [_cc("finish", BF16, 1048577, 64, "vec", "two_level")]
)

# ---- hgr_cast16 (grid1 of n / 4, cap 16384) and hgr_cast16_transpose ----------------------------------------------------------------------
CAST_PATTERN = 4096
CAST_NS = [(4, False), (1028, False), (16777216 + 4, True)]                     # (n, grid-stride)


def _ct(name, rows, cols, route, ldx=None, ldy=None, ldyt=None, lead_x=0, lead_y=0, lead_t=0):
    return NS(name=name, rows=rows, cols=cols, ldx=cols if ldx is None else ldx, ldy=cols if ldy is None else ldy,
              ldyt=up(rows, 8) if ldyt is None else ldyt, lead_x=lead_x, lead_y=lead_y, lead_t=lead_t, route=route)


CAST_T_CASES = [
    _ct("one_tile", 64, 64, "vec"),
    _ct("tiny", 8, 8, "vec"),
    _ct("ragged_rows_2x2", 65, 72, "vec"),
    _ct("ragged_cols_ld72", 130, 70, "vec", ldx=72, ldy=72),                    # cols % 8 = 6 inside the vector route: its element arm
    _ct("one_row", 1, 8, "vec"),
    _ct("odd_everything", 3, 5, "element", ldyt=3),
    _ct("odd_ldx", 130, 70, "element", ldx=70, ldy=72),
    _ct("x_misaligned", 64, 64, "element", lead_x=1),
    _ct("y_misaligned", 64, 64, "element", lead_y=1),
    _ct("yt_misaligned", 64, 64, "element", lead_t=1),
]

# ---- hgr_quickgelu16 (grid1 of n / 8), hgr_sumsq (cap 1024), hgr_adamw (cap 4096) ---------------------------------------------------------
GELU_PATTERN = 4096
GELU_NS = [(8, False), (2056, False), (8 * (16384 * 256) + 8, True)]
SUMSQ_NS = [(1, False), (255, False), (257, False), (262144, False), (262145, True), (786449, True)]
ADAMW_PATTERN = 1024
ADAMW_NS = [(1, False), (255, False), (1000, False), (4096 * 256 + 3, True)]
# branch sets of hgr_adamw: name, sumsq_total given, norm of the first step's gradient (the second and third have 1.5 and 0.7 times it),
# grad_scale, wd, first step, state starts at zero; max_norm is ADAMW_HP's for all of them
ADAMW_BRANCHES = [
    NS(name="no_total", total=False, norm=3.0, gscale=1.0, wd=0.1, step0=1, zero=True),
    NS(name="clip_active", total=True, norm=30.0, gscale=1.0, wd=0.1, step0=1, zero=True),
    NS(name="clip_inactive", total=True, norm=0.1, gscale=1.0, wd=0.1, step0=1, zero=True),
    NS(name="scaled_no_total", total=False, norm=3.0, gscale=0.25, wd=0.1, step0=1, zero=True),
    NS(name="scaled_clip", total=True, norm=30.0, gscale=0.25, wd=0.0, step0=1, zero=True),          # scaled norm 7.5 > 1: active
    NS(name="scaled_norm_decides", total=True, norm=3.0, gscale=0.25, wd=0.0, step0=1, zero=True),   # norm 3 > 1 but scaled 0.75: inactive (second step: 1.125, active)
    NS(name="no_decay", total=True, norm=30.0, gscale=1.0, wd=0.0, step0=1, zero=True),
    NS(name="late_step", total=True, norm=30.0, gscale=1.0, wd=0.1, step0=1000, zero=False),
    NS(name="late_step_no_total", total=False, norm=3.0, gscale=1.0, wd=0.0, step0=1000, zero=False),
]
ADAMW_HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0)

# ---- hgr_bn_fold / hgr_bn_unfold_grad: K = Cin * khw; K > 256 takes the second trip of the 256-thread loops ----------------------------------
BN_SHAPES = [(3, 9), (40, 9), (64, 1), (300, 1)]
BN_COUT = [1, 5]


def test_tables_reach_every_route():
    # transpose16
    for c in TRANSPOSE_CASES:
        assert transpose16_route(c) == c.route, c.name
        assert c.ldx >= c.coff + c.cols and c.ldy >= c.rows, c.name
    assert {c.route for c in TRANSPOSE_CASES} == {"vec", "scalar"}
    edges = set().union(*[transpose16_edges(c) for c in TRANSPOSE_CASES if c.route == "vec"])
    assert edges == {"load8", "load_ragged", "store8", "store_ragged", "blocks"}, edges
    assert any(c.route == "scalar" and (c.rows > 64 and c.cols > 64) for c in TRANSPOSE_CASES)
    # transpose16_colsum
    for c in TCS_CASES + TCS_REFUSED:
        assert transpose16_colsum_route(c) == c.route, c.name
        assert c.ldx >= c.coff + c.cols and c.ldy >= c.rows, c.name
    geometry = lambda c: (c.rows, c.cols, c.ldx, c.coff, c.ldy, c.lead_x, c.lead_y)
    vec = [c for c in TRANSPOSE_CASES if c.route == "vec"]
    assert len(vec) == 7 and any((c.rows, c.cols, c.ldx) == (130, 70, 72) for c in vec)
    for dt in DTS:                                           # transpose16<1> and <2> are kernels of their own: each runs every arm
        mine = [c for c in TCS_T_CASES if c.dt == dt]
        assert [geometry(c) for c in mine] == [geometry(c) for c in vec], tag(dt)
        edges = set().union(*[tcs_edges(c) for c in mine])
        assert edges == {"load8", "load_ragged", "store8", "store_ragged", "blocks", "sum_guard", "ragged_partial", "x_slice",
                         "ldy_padding"}, (tag(dt), edges)
        assert {c.ldy - c.rows for c in mine} >= {0, 7, 63} and any(c.coff == 8 and c.ldx == c.cols + 16 for c in mine)
    assert len({c.name for c in TCS_CASES}) == len(TCS_CASES)
    loops = set().union(*[finish_loops((c.rows + 63) // 64) for c in TCS_CASES])
    assert loops == {"final", "deep.unrolled", "deep.remainder", "mid.unrolled", "mid.remainder", "top.remainder", "one_band_chunk"}, loops
    assert finish_loops(32) == {"deep.unrolled"} and finish_loops(33) == {"deep.unrolled", "deep.remainder"}
    assert [(r + 63) // 64 for r in TCS_ROWS + TCS_BIG] == [1, 1, 1, 2, 31, 32, 33, 47, 2048, 2049]
    assert {c.dt for c in TCS_CASES if c.rows == 131073} == set(DTS) and {c.cols for c in TCS_CASES if c.rows == 131073} == {8, 72}
    # colsum
    for c in COLSUM_CASES:
        assert colsum_route(c) == (c.route, c.finish), (c.name, colsum_route(c))
        assert c.strides == (c.route == "rows_f32" and grid_strides(c.cols // 4)), c.name
    assert {(c.route, c.finish) for c in COLSUM_CASES} >= {("rows_f32", None), ("vec", "final"), ("scalar", "final"), ("scalar", "deep"),
                                                           ("scalar", "two_level"), ("vec", "two_level")}
    assert any(c.strides for c in COLSUM_CASES)
    assert {(c.rows + 511) // 512 for c in COLSUM_CASES if c.name.startswith("finish")} == {31, 32, 2048, 2049}
    assert "one_band_chunk" in finish_loops(2049)
    for dt in (BF16, F16, F32):
        assert {c.route for c in COLSUM_CASES if c.dt == dt} >= {"vec", "scalar"}, tag(dt)
    assert {c.route for c in COLSUM_CASES if c.random} == {"rows_f32", "vec", "scalar"}
    # casts
    for n, strides in CAST_NS:
        assert n % 4 == 0 and grid_strides(n // 4) == strides, n
    assert any(s for _, s in CAST_NS) and any(n % CAST_PATTERN for n, _ in CAST_NS)
    for c in CAST_T_CASES:
        assert cast16_transpose_route(c) == c.route, c.name
    assert {c.route for c in CAST_T_CASES} == {"vec", "element"}
    # quickgelu, sumsq, adamw
    for n, strides in GELU_NS:
        assert n % 8 == 0 and grid_strides(n // 8) == strides, n
    for n, strides in SUMSQ_NS:
        assert grid_strides(n, 256, 1024) == strides, n
    assert grid1(262144, 256, 1024) == 1024 and grid1(262143, 256, 1024) == 1024 and grid1(257, 256, 1024) == 2
    for n, strides in ADAMW_NS:
        assert grid_strides(n, 256, 4096) == strides, n
    assert all(any(s for _, s in t) for t in (GELU_NS, SUMSQ_NS, ADAMW_NS))
    br = ADAMW_BRANCHES
    assert {b.total for b in br} == {True, False} and {b.gscale for b in br} == {1.0, 0.25} and {b.wd for b in br} == {0.0, 0.1}
    assert {b.step0 for b in br} == {1, 1000} and all(b.zero == (b.step0 == 1) for b in br)
    active = {(b.gscale, b.norm * b.gscale > ADAMW_HP["max_norm"]) for b in br if b.total}
    assert active == {(1.0, True), (1.0, False), (0.25, True), (0.25, False)}
    # batch norm: the 256-thread loops make one trip and two
    assert {(cin * khw > 256) for cin, khw in BN_SHAPES} == {True, False} and {khw for _, khw in BN_SHAPES} == {1, 9}


# ==== inputs =======================================================================================================================
def normal(shape, seed, scale=1.0, name="stream"):
    n = int(np.prod(shape))
    return torch.from_numpy((scale * synth.normal(seed, name, n)).astype(np.float32).reshape(shape))


def ints(shape, seed, lo=-3, hi=4, name="stream.int"):
    n = int(np.prod(shape))
    return torch.from_numpy(synth.randint(seed, name, n, lo, hi).astype(np.float32).reshape(shape))


def bit_patterns(shape, seed, avoid):
    """Random 16-bit patterns (NaNs, infinities, subnormals included) as int16, none of them one of `avoid` (the poison patterns)."""
    n = int(np.prod(shape))
    v = synth.randint(seed, "stream.bits", n, 0, 65536)
    for a in avoid:
        v[v == a] = 0x1234
    return torch.from_numpy(v.astype(np.uint16).view(np.int16).reshape(shape))


def cast_specials(dt):
    """fp32 values at which a cast goes wrong: exact ties (round to even, both directions), +-0, the largest finite value and the first
    value that rounds to inf, values that round into the subnormal range and to zero, inf and NaN."""
    if dt == F16:
        v = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0, 65504.0, 65519.996, 65520.0, -65520.0,
             2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -15 + 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * 1.0000001, 2.0 ** -26,
             3 * 2.0 ** -25]
    else:
        big = float(np.float32(3.3895313892515355e38))            # bf16 max = (2 - 2^-7) 2^127
        tie = float(np.float32((2 - 2.0 ** -8) * 2.0 ** 127))       # half way to 2^128: rounds to inf
        v = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 256.0 + 1.0, 256.0 + 3.0, big, float(np.nextafter(np.float32(tie), np.float32(0))),
             tie, -tie, 2.0 ** -126, 2.0 ** -126 - 2.0 ** -134, 2.0 ** -127 + 2.0 ** -134, 2.0 ** -133, 2.0 ** -134, -(2.0 ** -134),
             float(np.nextafter(np.float32(2.0 ** -134), np.float32(1))), 2.0 ** -135, 3 * 2.0 ** -134]
    v += [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1e-45]
    return torch.tensor(v, dtype=F32)


def cast_pattern(dt, seed=11):
    """CAST_PATTERN floats: N(0, 1) with the special values planted over the first entries, and 4 tail values."""
    x = normal((CAST_PATTERN,), seed)
    s = cast_specials(dt)
    x[:s.numel()] = s
    return x, torch.tensor([1.0 + 2.0 ** -11, -0.0, float("inf"), 0.3], dtype=F32)


def same_bits16(got, want):
    """NaNs compare as NaN-ness, everything else as bits."""
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]))


def test_cast_specials_do_what_they_are_planted_for():
    for dt in DTS:
        s = cast_specials(dt)
        y = s.to(dt)
        mx = torch.finfo(dt).max
        assert float(y[0]) == 1.0 and float(y[1]) == 1.0 + (2.0 ** -9 if dt == F16 else 2.0 ** -6) and float(y[2]) == -1.0       # ties to even
        assert float(y[5]) == mx and float(y[6]) == mx and math.isinf(float(y[7])) and float(y[8]) == -math.inf
        tiny = torch.finfo(dt).smallest_normal
        assert float(y[9]) == tiny and float(y[10]) == tiny and 0 < float(y[11]) < tiny and 0 < float(y[12]) < tiny
        assert float(y[13]) == 0.0 and float(y[14]) == 0.0 and math.copysign(1.0, float(y[14])) == -1.0                        # tie to even: -0
        assert float(y[15]) > 0.0 and float(y[16]) == 0.0 and float(y[17]) == 2 * float(y[12] if dt == F16 else y[15])
        x, tail = cast_pattern(dt)
        assert bool(torch.isnan(x.to(dt)).any()) and bool(torch.isinf(x.to(dt)).any()) and x.numel() == CAST_PATTERN and tail.numel() == 4


# ==== sums =========================================================================================================================
def sum_bound(abs_sum64, result64, depth, alpha=1.0):
    """|got - ref| for a sum of fp32 terms added in any order, scaled and accumulated: every term passes through at most `depth` additions,
    each a factor (1 + d), |d| <= u, so the sum errs by ((1 + u)^depth - 1) sum |x_i| <= (depth + 1) u sum |x_i| for depth <= 4096 (the
    second-order part is below depth^2 u^2 / 2 < u at that depth).  alpha * acc is one more rounding of at most u |alpha| sum |x_i| (1 + ...)
    and the add onto `out` one of at most u |result|; 2^-23 |result| as the issue states it covers that add with room."""
    assert depth <= 4096
    return (depth + 2) * U32 * abs(alpha) * abs_sum64 + 2.0 ** -23 * result64.abs()


def colsum_depth(c):
    """Additions on the longest path of hgr_colsum for a case of COLSUM_CASES (read from the kernels).
    rows_f32: rows - 1 in sequence.  scalar: 4 row groups of a 512-row band, ceil(512 / 4) adds each, then 3 for s0 + s1 + s2 + s3.
    vec: 16 (fp32) or 32 (16-bit) row groups, ceil(512 / groups) adds each, then `groups` adds in sequence.  Then the finish."""
    if c.route == "rows_f32":
        return max(c.rows - 1, 0)
    band = min(c.rows, 512)
    if c.route == "scalar":
        part = (band + 3) // 4 + 3
    else:
        groups = 16 if c.dt == F32 else 32
        part = (band + groups - 1) // groups + groups
    return part + finish_depth((c.rows + 511) // 512)


def tcs_depth(rows):
    """transpose16<CS>: two accumulators of 32 adds over a 64-row tile and one add of the two, then the finish."""
    return 33 + finish_depth((rows + 63) // 64)


def sumsq_blocks(n):
    return grid1(n, 256, 1024)


def sumsq_depth(n):
    """hgr_sumsq: a thread adds ceil(n / (blocks * 256)) squares (the square is one more rounding unless it is contracted into an FMA: +1),
    wave_sum is 6 levels, (s0 + s1) + (s2 + s3) 2; the last block: ceil(blocks / 256) partials per thread, 6, 2; the add onto *out is the
    2^-23 |result| term of sum_bound."""
    b = sumsq_blocks(n)
    return (n + b * 256 - 1) // (b * 256) + 1 + 6 + 2 + (b + 255) // 256 + 6 + 2


def emu_colsum(x, band, alpha, start, drop_last_row=False):
    """fp32: per-band sums, then the sum of the bands, alpha, start - torch's own fp32 order (the bound holds for any order)."""
    rows, cols = x.shape
    parts = []
    for r0 in range(0, rows, band):
        blk = x[r0:min(rows, r0 + band)].float()
        if drop_last_row and blk.shape[0] == band:
            blk = blk[:-1]
        acc = torch.zeros(cols, dtype=F32)
        for r in range(blk.shape[0]):
            acc = acc + blk[r]
        parts.append(acc)
    tot = torch.zeros(cols, dtype=F32)
    for p in parts:
        tot = tot + p
    return start + np.float32(alpha) * tot


def test_sum_bound_holds_for_the_emulation_and_sees_a_dropped_row():
    for dt, band, rows in ((F32, 512, 1100), (BF16, 64, 200), (F16, 512, 513)):
        x = normal((rows, 24), 3 + rows).to(dt)
        start = normal((24,), 5)
        ref = start.double() + 0.5 * x.double().sum(0)
        bound = sum_bound(x.double().abs().sum(0), ref, band + (rows + band - 1) // band, 0.5)       # the emulation's own depth: sequential
        worst = within(emu_colsum(x, band, 0.5, start), ref, bound, "colsum emulation " + tag(dt))
        assert ratio(emu_colsum(x, band, 0.5, start, drop_last_row=True), ref, bound) > 1.0, (tag(dt), worst)
        print("RATIO-CPU colsum", tag(dt), round(worst, 3))
    # hgr_sumsq: 256 threads x blocks strided partial sums of fp32 squares, then the partials in thread order - inside the bound of its depth
    for n in (257, 262145, 786449):
        x = normal((n,), 7 + n)
        blocks = sumsq_blocks(n)
        pad = torch.zeros(up(n, blocks * 256))
        pad[:n] = x * x
        lanes = torch.zeros(blocks * 256)
        for row in pad.view(-1, blocks * 256):
            lanes = lanes + row
        got = lanes.view(blocks, 256).sum(1).sum(0, keepdim=True)
        ref = (x.double() ** 2).sum().reshape(1)
        print("RATIO-CPU sumsq", n, round(within(got, ref, sum_bound(ref, ref, sumsq_depth(n)), "sumsq emulation"), 3))
        lost = (lanes.view(blocks, 256)[:-1]).sum(1).sum(0, keepdim=True)                   # the last block's partial not added
        assert ratio(lost, ref, sum_bound(ref, ref, sumsq_depth(n))) > 1.0
    # depths read from the kernels never exceed the number of terms of a column
    for c in COLSUM_CASES:
        assert colsum_depth(c) <= max(c.rows, 1) + 12, c.name
    assert sumsq_depth(1) == 1 + 1 + 8 + 1 + 8 and sumsq_depth(262145) == 2 + 1 + 8 + 4 + 8


def test_integer_sums_are_exact_in_fp32():
    """The exact cases: values in [-3, 3], at most 2^20 + 2^10 rows - every partial sum is an integer below 2^24, alpha = 0.5 and an integer
    start keep it a multiple of 0.5 below 2^23."""
    rows = max(c.rows for c in COLSUM_CASES)
    assert 3 * rows + 8 < 2 ** 23 and 9 * max(n for n, _ in SUMSQ_NS) + 8 < 2 ** 24


# ==== QuickGELU ====================================================================================================================
LOG2E32 = np.float32(1.4426950408889634)
C1702 = np.float32(1.702)


def gelu_inputs(n, dt, seed=21):
    """Pre-activations N(0, 4) clipped to +-8 and incoming gradients N(0, 1), rounded to the type."""
    x = normal((n,), seed, 2.0).clamp_(-8.0, 8.0).to(dt)
    du = normal((n,), seed + 1).to(dt)
    return x, du


def gelu_planted(dt):
    """(x, du): saturated, vanished and zero pre-activations.  x >= 16: sigmoid is exactly 1 in fp32 (exp2 of -39 and below is under
    2^-24); x <= -64: exp2 of 157 and above overflows, 1 / inf = 0 (-65504 is the largest magnitude tried: 1.702 x stays finite); x = +-0:
    sigmoid = rcp(2) = 0.5."""
    big = [16.0, 17.5, 100.0, 1000.0, 65504.0 if dt == F16 else 65536.0, 16.0, 32.0, 64.0]
    neg = [-64.0, -100.0, -1000.0, -65504.0 if dt == F16 else -65536.0, -64.0, -128.0, -256.0, -512.0]
    x = torch.tensor(big + neg + [0.0, -0.0] * 4, dtype=F32).to(dt)
    du = torch.tensor([1.0, -0.337, 3.0, 2.0 ** -14, -7.0, 0.0, 1.5, -2.0] * 2 + [1.0, 1.0, -0.337, -0.337, 2.0 ** -24 * 3, 6e-8, 5.0, -0.0], dtype=F32).to(dt)
    assert x.numel() == du.numel() == 24
    return x, du


def gelu_ref64(x16, du16):
    """x * sigmoid(1.702 x) and autograd of it, float64, from the 16-bit inputs' values."""
    x = x16.double().requires_grad_(True)
    y = x * torch.sigmoid(1.702 * x)
    y.backward(du16.double())
    return y.detach(), x.grad.detach()


def gelu_fwd_bound(ref64, dt):
    """One rounding to the type plus the fp32 arithmetic in front of it: z = 1.702 x (u), t = -log2(e) z (u, and log2(e) itself is rounded:
    u) - |t| <= 20 for |x| <= 8, so 3 u * 20 * ln 2 < 42 u on exp2(t) - v_exp_f32 and v_rcp_f32 one ulp (2 u) each, 1 + e (u), x * s (u
    for bf16): relative to s at most 42 u e / (1 + e) + 6 u < 48 u < 2^-18.4; 2^-17 as the issue states it."""
    return half_ulp16(ref64, dt) + 2.0 ** -17 * ref64.abs()


def gelu_bwd_bound(ref64, du64, dt):
    """g' = s (1 + 1.702 x (1 - s)).  The relative error of s is below 2^-18.4 (above); 1 - s is formed in fp32 and inherits the absolute
    error of s: about 2^-18 (|g'| + 1.702 |x| s^2) on the derivative, which is below 2^-18 (1.1 + 1.702 * 8 * 1) < 2^-14.1 for |x| <= 8."""
    return half_ulp16(ref64, dt) + 2.0 ** -14 * du64.abs()


def _ulp_step(x, k):
    """x moved by k fp32 ulps (k in {-1, 0, 1}) wherever it is positive and finite."""
    if not k:
        return x
    return torch.where(torch.isfinite(x) & (x > 0), (x.contiguous().view(torch.int32) + k).view(F32), x)


def emu_gelu(x16, du16, dt, k_exp=0, k_rcp=0, coef=C1702, drop_1ms=False):
    """fp32, the kernel's order: s = rcp(1 + exp2(-log2e * (1.702 x))); forward (16)(x s); backward (16)((du s)(1 + 1.702 x (1 - s))).
    exp2 and the reciprocal can be moved by one ulp (v_exp_f32, v_rcp_f32)."""
    x = x16.float()
    z = np.float32(coef) * x
    e = _ulp_step(torch.exp2(-LOG2E32 * z), k_exp)
    s = _ulp_step(1.0 / (1.0 + e), k_rcp)
    fwd = (x * s).to(dt)
    inner = torch.ones_like(x) if drop_1ms else (1.0 - s)
    bwd = ((du16.float() * s) * (1.0 + (np.float32(coef) * x) * inner)).to(dt)
    return fwd, bwd


def test_quickgelu_emulation_within_bounds_and_broken_ones_caught():
    worst = {}
    for dt in DTS:
        x, du = gelu_inputs(GELU_PATTERN, dt)
        assert float(x.float().abs().max()) <= 8.0 and float(x.float().min()) < -6.0 and float(x.float().max()) > 6.0
        rf, rb = gelu_ref64(x, du)
        assert bool(torch.isfinite(rf).all()) and bool(torch.isfinite(rb).all())             # the cap: no element is left out
        bf, bb = gelu_fwd_bound(rf, dt), gelu_bwd_bound(rb, du.double(), dt)
        wf = wb = 0.0
        for k_exp in (-1, 0, 1):
            for k_rcp in (-1, 0, 1):
                f, b = emu_gelu(x, du, dt, k_exp, k_rcp)
                wf, wb = max(wf, within(f, rf, bf, "fwd")), max(wb, within(b, rb, bb, "bwd"))
        worst[tag(dt)] = (round(wf, 3), round(wb, 3))
        f, b = emu_gelu(x, du, dt, coef=1.7)                                             # 1.7 for 1.702
        assert ratio(f, rf, bf) > 1.0 and ratio(b, rb, bb) > 1.0, tag(dt)
        _, b = emu_gelu(x, du, dt, drop_1ms=True)                                        # the derivative without (1 - s)
        assert ratio(b, rb, bb) > 1.0, tag(dt)
    print("RATIO-CPU quickgelu (fwd, bwd)", worst)


def test_quickgelu_planted_values_hold_in_the_emulation():
    for dt in DTS:
        x, du = gelu_planted(dt)
        f, b = emu_gelu(x, du, dt)
        assert same_bits16(f[:8], x[:8]) and same_bits16(b[:8], du[:8])
        assert bool((f[8:16].float() == 0).all()) and bool((b[8:16].float() == 0).all())
        assert bool((f[16:].float() == 0).all()) and same_bits16(b[16:], (du[16:].double() * 0.5).to(dt))


# ==== AdamW ========================================================================================================================
def f32(v):
    return float(np.float32(v))


def adamw_scalars():
    """The scalars as the kernel receives them: rounded to fp32, then handed to the float64 reference as they are."""
    hp = ADAMW_HP
    return NS(lr=f32(hp["lr"]), b1=f32(hp["beta1"]), b2=f32(hp["beta2"]), eps=f32(hp["eps"]), max_norm=f32(hp["max_norm"]))


def adamw_inputs(n, br, seed=31):
    """p, m0, v0 and three gradients whose global norm is br.norm.  Every gradient of an element has one sign, and m0 has it too: b1 m and
    (1 - b1) g never cancel, |m'| is the sum of their magnitudes, and the relative error of m' that the bound on p' counts on is the
    one stated (with cancellation it is unbounded, and no fixed multiple of |step| would do)."""
    p = normal((n,), seed)
    g0 = normal((n,), seed + 1)
    g0 = torch.where(g0 == 0, torch.ones_like(g0), g0)
    gs = []
    for k, f in enumerate((1.0, 1.5, 0.7)):
        g = (g0 * (0.5 + torch.from_numpy(synth.uniform(seed + 2 + k, "stream.adamw", n)).float())).double()
        gs.append((g * (br.norm * f / float(g.norm()))).float())
    if br.zero:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:
        m0 = (gs[0] * 0.3 * br.gscale).float()
        v0 = (gs[0].double() ** 2 * 0.5 * br.gscale ** 2).float()
    return p, m0, v0, gs


def sumsq_total_of(g):
    """The squared norm the kernel is given: the float64 sum of squares, rounded to fp32."""
    return torch.tensor([float((g.double() ** 2).sum())], dtype=F32)


def adamw_ref64(p, g, m, v, step, br, sc):
    """One step of torch.optim.AdamW after clip_grad_norm_, float64, from the given state bits.  The gradient the optimiser sees is
    grad_scale * g; without sumsq_total nothing is clipped.  Returns p', m', v' and what the bounds need."""
    pr = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.AdamW([pr], lr=sc.lr, betas=(sc.b1, sc.b2), eps=sc.eps, weight_decay=f32(br.wd))
    pr.grad = g.double() * br.gscale
    if br.total:
        torch.nn.utils.clip_grad_norm_([pr], sc.max_norm)
    st = opt.state[pr]
    st["step"] = torch.tensor(float(step - 1), dtype=F32)
    st["exp_avg"], st["exp_avg_sq"] = m.double().clone(), v.double().clone()
    gc = pr.grad.clone()
    opt.step()
    return pr.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), gc


def adamw_closed_form(p, g, m, v, step, br, sc):
    """The kernel's comment in float64: p *= 1 - lr wd; m, v EMA; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps), the gradient scaled by
    grad_scale * min(1, max_norm / (grad_scale * norm + 1e-6))."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    clip = br.gscale
    if br.total:
        clip = br.gscale * min(1.0, sc.max_norm / (float(g.norm()) * br.gscale + 1e-6))
    gi = g * clip
    m1 = sc.b1 * m + (1 - sc.b1) * gi
    v1 = sc.b2 * v + (1 - sc.b2) * gi * gi
    bc1, bc2 = 1 - sc.b1 ** step, 1 - sc.b2 ** step
    p1 = p * (1 - sc.lr * f32(br.wd)) - (sc.lr / bc1) * m1 / (v1.sqrt() / math.sqrt(bc2) + sc.eps)
    return p1, m1, v1


def adamw_clip_active(g, br, sc):
    """Whether this step's gradient is clipped: the factor max_norm / (grad_scale * norm + 1e-6) of the kernel's comment is below 1.  The
    cases keep it further from 1 than its own rounding (3.5 u) by far, so the fp32 kernel decides alike."""
    if not br.total:
        return False
    factor = sc.max_norm / (float(g.double().norm()) * br.gscale + 1e-6)
    assert abs(factor - 1.0) > 1e-5, (br.name, factor)
    return factor < 1.0


def adamw_bounds(p, g, m, v, step, br, sc, ref):
    """Bounds on m', v', p' of one step from the same state bits.  r is the relative error of gi = fl(g * clip), decided for this step
    from the norm of this step's own gradient.  No total, or grad_scale * norm <= max_norm (an inactive clip: max_norm / (norm + 1e-6)
    stays above 1 through its 3.5 u, the tables keep the norms away from max_norm, and min(1, .) is exactly 1): clip = grad_scale, a power
    of two in every branch here, and r = 0.  An active clip - clip_active, scaled_clip, no_decay, late_step at every step, and
    scaled_norm_decides at its second step, where the gradient is 1.5 times the first - needs r: the given total is the float64 sum
    rounded to fp32 (u, u / 2 after the root), sqrtf u and the division u (both correctly rounded: the build has no fast-math flag),
    + 1e-6 u, the two products with grad_scale exact for a power of two and u each otherwise, the product g * clip u:
    r = 4.5 u, or 6.5 u for a grad_scale that is no power of two.
      m' = b1 m + (1 - b1) gi: 1 - b1 is exact in fp32 (Sterbenz); two products and the sum, 3 u, and r on the second term:
           2^-22 (|t1| + |t2|) + r |t2|.
      v' = b2 v + ((1 - b2) gi) gi: 2^-22 (|t1| + |t2|) + 2 r |t2|.
      p' = p f - step, f = 1 - lr wd: f errs by e_f (computed here from the scalars, at most 2^-25 (1 + lr wd)), the product and the
           difference by u each: (2^-23 + e_f) |p'| + (2 u + e_f) |step| since |p f| <= |p'| + |step|.  step = (lr / bc1) m' / (sqrt(v')
           rsqrt(bc2) + eps) inherits (4 u + r) from m' (no cancellation in m': see adamw_inputs) and half of (4 u + 2 r) from v', lr / bc1,
           sqrtf, rsqrtf (2 u), the product, + eps, the division and the product with m': 8 u - 14 u + 2 r <= 28 u, inside the 2^-19 = 32 u
           the issue states together with the 2 u + e_f above.  bc = 1 - powf(beta, step) carries powf's error (2 u on a value near 1)
           divided by bc: 2^-23 / bc1 on the step, and half of that, 2^-24 / bc2, under the root."""
    p1, m1, v1, gc = ref
    r = 0.0
    if adamw_clip_active(g, br, sc):
        r = (4.5 if math.frexp(br.gscale)[0] == 0.5 else 6.5) * U32
    tm = (sc.b1 * m.double()).abs(), ((1 - sc.b1) * gc).abs()
    tv = (sc.b2 * v.double()).abs(), (1 - sc.b2) * gc * gc
    bm = 2.0 ** -22 * (tm[0] + tm[1]) + r * tm[1]
    bv = 2.0 ** -22 * (tv[0] + tv[1]) + 2 * r * tv[1]
    wd = f32(br.wd)
    f_exact = 1.0 - sc.lr * wd
    e_f = abs(float(np.float32(1.0) - np.float32(sc.lr) * np.float32(wd)) - f_exact) / f_exact
    assert e_f <= 2.0 ** -25 * 1.01
    bc1, bc2 = 1 - sc.b1 ** step, 1 - sc.b2 ** step
    stp = (p.double() * f_exact - p1).abs()
    bp = (2.0 ** -23 + e_f) * p1.abs() + (2.0 ** -19 + 2.0 ** -23 / bc1 + 2.0 ** -24 / bc2) * stp
    return bp, bm, bv


def emu_adamw(p, g, m, v, step, br, sc, total=None, bc_step=None, decay_after=False, no_1e6=False):
    """fp32, the kernel's order (no FMA contraction: one rounding more per product-sum than the device may make)."""
    one = np.float32(1.0)
    lr, b1, b2, eps, wd, gs = (np.float32(x) for x in (sc.lr, sc.b1, sc.b2, sc.eps, br.wd, br.gscale))
    clip = gs
    if total is not None:
        norm = np.sqrt(np.float32(total)) * gs
        clip = gs * min(one, np.float32(sc.max_norm) / (norm if no_1e6 else norm + np.float32(1e-6)))
    st = np.float32(step if bc_step is None else bc_step)
    bc1, bc2 = one - np.power(b1, st), one - np.power(b2, st)
    rs2 = one / np.sqrt(bc2)
    gi = g * clip
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    upd = (lr / bc1) * mi / (vi.sqrt() * rs2 + eps)
    pn = (p - upd) * (one - lr * wd) if decay_after else p * (one - lr * wd) - upd
    return pn, mi, vi


def test_adamw_closed_form_is_the_optimiser():
    sc = adamw_scalars()
    for br in ADAMW_BRANCHES:
        p, m, v, gs = adamw_inputs(257, br)
        pc, mc, vc = p.double(), m.double(), v.double()
        pr = torch.nn.Parameter(p.double().clone())
        opt = torch.optim.AdamW([pr], lr=sc.lr, betas=(sc.b1, sc.b2), eps=sc.eps, weight_decay=f32(br.wd))
        for k in range(3):
            step = br.step0 + k
            pr.grad = gs[k].double() * br.gscale
            if br.total:
                torch.nn.utils.clip_grad_norm_([pr], sc.max_norm)
            if k == 0:                                   # the state a late step starts from
                opt.state[pr]["step"] = torch.tensor(float(step - 1), dtype=F32)
                opt.state[pr]["exp_avg"], opt.state[pr]["exp_avg_sq"] = m.double().clone(), v.double().clone()
            opt.step()
            pc, mc, vc = adamw_closed_form(pc, gs[k], mc, vc, step, br, sc)
            scale = 1.0 + float(pc.abs().max())
            assert float((pc - pr.detach()).abs().max()) <= 1e-12 * scale, (br.name, step)
            st = opt.state[pr]
            assert float((mc - st["exp_avg"]).abs().max()) <= 1e-12 and float((vc - st["exp_avg_sq"]).abs().max()) <= 1e-12, (br.name, step)


def _adamw_emulated_steps(br, n=1000, **broken):
    """Three steps of one fp32 state; every step is checked against the float64 optimiser started from the same state bits.  Returns the
    worst ratio per output over the three steps."""
    sc = adamw_scalars()
    p, m, v, gs = adamw_inputs(n, br)
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        step = br.step0 + k
        g = gs[k]
        assert bool(((sc.b1 * m.double()) * g.double() >= 0).all())                 # no cancellation in m'
        ref = adamw_ref64(p, g, m, v, step, br, sc)
        bp, bm, bv = adamw_bounds(p, g, m, v, step, br, sc, ref)
        total = float(sumsq_total_of(g)) if br.total else None
        pn, mn, vn = emu_adamw(p, g, m, v, step, br, sc, total, **broken)
        for i, (got, want, bound) in enumerate(((pn, ref[0], bp), (mn, ref[1], bm), (vn, ref[2], bv))):
            assert bool(torch.isfinite(want).all())
            worst[i] = max(worst[i], ratio(got, want, bound))
        p, m, v = pn, mn, vn
    return worst


def test_adamw_emulation_within_bounds_and_broken_ones_caught():
    sc = adamw_scalars()
    table = {}
    for br in ADAMW_BRANCHES:
        w = _adamw_emulated_steps(br)
        assert max(w) <= 1.0, (br.name, w)
        table[br.name] = [round(x, 3) for x in w]
        if br.total and br.norm * br.gscale <= sc.max_norm:                          # an inactive clip multiplies by exactly grad_scale
            p, m, v, gs = adamw_inputs(64, br)
            _, mn, _ = emu_adamw(p, gs[0], m, v, br.step0, br, sc, float(sumsq_total_of(gs[0])))
            assert torch.equal(mn, np.float32(sc.b1) * m + (np.float32(1) - np.float32(sc.b1)) * (gs[0] * np.float32(br.gscale)))
    print("RATIO-CPU adamw (p, m, v)", table)
    late = [b for b in ADAMW_BRANCHES if b.name == "late_step"][0]
    first = [b for b in ADAMW_BRANCHES if b.name == "clip_active"][0]
    for br in (first, late):
        w = _adamw_emulated_steps_bc(br)
        assert w[0] > 1.0, (br.name, "bias correction of step - 1", w)
    assert _adamw_emulated_steps(first, decay_after=True)[0] > 1.0                   # weight decay applied after the update
    # clip without the 1e-6 at a norm of about 1e-5 and max_norm 1e-5: the factor is 1 instead of 1 / 1.1
    tiny = NS(name="tiny_norm", total=True, norm=1e-5 * 1.0001, gscale=1.0, wd=0.1, step0=1, zero=True)
    sc2 = adamw_scalars()
    sc2.max_norm = f32(1e-5)
    p, m, v, gs = adamw_inputs(1000, tiny)
    ref = adamw_ref64(p, gs[0], m, v, 1, tiny, sc2)
    assert adamw_clip_active(gs[0], tiny, sc2)                                       # 1e-5 / (1.0001e-5 + 1e-6): the bounds carry r
    bp, bm, bv = adamw_bounds(p, gs[0], m, v, 1, tiny, sc2, ref)
    good = emu_adamw(p, gs[0], m, v, 1, tiny, sc2, float(sumsq_total_of(gs[0])))
    bad = emu_adamw(p, gs[0], m, v, 1, tiny, sc2, float(sumsq_total_of(gs[0])), no_1e6=True)
    assert ratio(good[1], ref[1], bm) <= 1.0 and ratio(good[2], ref[2], bv) <= 1.0
    assert ratio(bad[1], ref[1], bm) > 1.0 and ratio(bad[2], ref[2], bv) > 1.0


def _adamw_emulated_steps_bc(br, n=1000):
    """The emulation with bias corrections of step - 1 (step 1 would divide by zero: there it uses step + 1)."""
    sc = adamw_scalars()
    p, m, v, gs = adamw_inputs(n, br)
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        step = br.step0 + k
        ref = adamw_ref64(p, gs[k], m, v, step, br, sc)
        bounds = adamw_bounds(p, gs[k], m, v, step, br, sc, ref)
        total = float(sumsq_total_of(gs[k])) if br.total else None
        out = emu_adamw(p, gs[k], m, v, step, br, sc, total, bc_step=step - 1 if step > 1 else step + 1)
        for i in range(3):
            worst[i] = max(worst[i], ratio(out[i], ref[i], bounds[i]))
        p, m, v = emu_adamw(p, gs[k], m, v, step, br, sc, total)
    return worst


# ==== batch-norm fold / unfold =========================================================================================================
BN_EPS = 1e-5


def bn_inputs(cout, cin, khw, seed=41):
    k = int(round(math.sqrt(khw)))
    w = normal((cout, cin, k, k), seed, 0.1)
    gamma = (0.5 + torch.from_numpy(synth.uniform(seed + 1, "stream.bn", cout))).float()
    beta = normal((cout,), seed + 2, 0.1)
    mean = normal((cout,), seed + 3, 0.2)
    var = (0.5 + torch.from_numpy(synth.uniform(seed + 4, "stream.bn", cout))).float()
    return w, gamma, beta, mean, var


def bn_layout(w):
    """[Cout, Cin, kh, kw] -> [Cout, (ky, kx, ci)]: the layout of the kernels' comment."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def bn_fold_ref64(w, gamma, beta, mean, var):
    s = gamma.double() / torch.sqrt(var.double() + f32(BN_EPS))
    return bn_layout(w.double() * s.view(-1, 1, 1, 1)), beta.double() - mean.double() * s, s


def bn_fold_bounds(w, gamma, beta, mean, var, dt):
    """s = gamma / sqrtf(var + eps): the sum u, halved by the root, the root u, the division u - 2.5 u.  w16 = (16)(w s): one product more,
    3.5 u <= 2^-22 before the rounding to the type.  bias = beta - mean s: 3.5 u on the product and u on the difference, which is at most
    |beta| + |mean s|: u |beta| + 4.5 u |mean s| = 2^-22 (|beta| + |mean s|) + 2^-25 |mean s| at most."""
    wf, b, s = bn_fold_ref64(w, gamma, beta, mean, var)
    ms = (mean.double() * s).abs()
    return half_ulp16(wf, dt) + 2.0 ** -22 * wf.abs(), 2.0 ** -22 * (beta.double().abs() + ms) + 2.0 ** -25 * ms


def emu_bn_fold(w, gamma, beta, mean, var, dt):
    s = gamma / torch.sqrt(var + np.float32(BN_EPS))
    return bn_layout(w * s.view(-1, 1, 1, 1)).to(dt), beta - mean * s


def bn_unfold_ref64(gwf, gbf, w, gamma, beta, mean, var, start):
    """start + autograd through w' = w gamma / sigma, b' = beta - mean gamma / sigma of sum(w' gwf) + sum(b' gbf), float64."""
    wr, ga, be = (t.double().clone().requires_grad_(True) for t in (w, gamma, beta))
    s = ga / torch.sqrt(var.double() + f32(BN_EPS))
    wf = bn_layout(wr * s.view(-1, 1, 1, 1))
    bf = be - mean.double() * s
    ((wf * gwf.double()).sum() + (bf * gbf.double()).sum()).backward()
    return start[0].double() + wr.grad, start[1].double() + ga.grad, start[2].double() + be.grad


def bn_unfold_bounds(gwf, gbf, w, gamma, mean, var, start):
    """inv_sigma = 1 / sqrtf(var + eps): 2.5 u; s = gamma inv_sigma: 3.5 u.
      g_w += gwf s: 4.5 u on the product, u on the sum (at most |g_w| + |gwf s|): 2^-22 (|g_w| + |gwf s|) + 2^-23 |gwf s| at most.
      g_gamma += (tot - gbf mean) inv_sigma, tot = sum_k gwf w over K terms: every term passes through d = ceil(K / 256) + 1 (the product,
        unless contracted) + 6 (wave_sum) + 3 (red[0] + .. + red[3]) roundings: d u sum |gwf w| inv_sigma; gbf mean u, the difference u,
        inv_sigma 2.5 u, the product u, the sum u: with T1 = |g_gamma|, T2 = |tot| inv_sigma, T3 = |gbf mean| inv_sigma at most
        u T1 + 6.5 u (T2 + T3) <= 2^-22 (T1 + T2 + T3) + 3 u (T2 + T3).
      g_beta += gbf: u |result| <= 2^-22 (|g_beta| + |gbf|)."""
    cout = w.shape[0]
    K = w[0].numel()
    isg = 1.0 / torch.sqrt(var.double() + f32(BN_EPS))
    s = gamma.double() * isg
    gs_ = (gwf.double() * s.view(-1, 1)).abs()
    gs_w = gs_.view(cout, -1, w.shape[1]).permute(0, 2, 1).reshape(w.shape)               # back to [Cout, Cin, kh, kw]
    b_w = 2.0 ** -22 * (start[0].double().abs() + gs_w) + 2.0 ** -23 * gs_w
    wl = bn_layout(w.double())
    d = (K + 255) // 256 + 1 + 6 + 3
    t1, t2, t3 = start[1].double().abs(), (gwf.double() * wl).sum(1).abs() * isg, (gbf.double() * mean.double()).abs() * isg
    b_g = 2.0 ** -22 * (t1 + t2 + t3) + 3 * U32 * (t2 + t3) + d * U32 * (gwf.double() * wl).abs().sum(1) * isg
    b_b = 2.0 ** -22 * (start[2].double().abs() + gbf.double().abs())
    return b_w, b_g, b_b


def emu_bn_unfold(gwf, gbf, w, gamma, mean, var, start, overwrite=False):
    isg = 1.0 / torch.sqrt(var + np.float32(BN_EPS))
    s = gamma * isg
    cout = w.shape[0]
    gw = (gwf * s.view(-1, 1)).view(cout, -1, w.shape[1]).permute(0, 2, 1).reshape(w.shape)
    tot = (gwf * bn_layout(w)).sum(1)
    gg = (tot - gbf * mean) * isg
    if overwrite:
        return gw, gg, gbf.clone()
    return start[0] + gw, start[1] + gg, start[2] + gbf


def test_bn_emulations_within_bounds_and_an_overwrite_is_caught():
    worst = {}
    for cin, khw in BN_SHAPES:
        for cout in BN_COUT:
            w, gamma, beta, mean, var = bn_inputs(cout, cin, khw, 41 + cin)
            for dt in DTS:
                rw, rb, _ = bn_fold_ref64(w, gamma, beta, mean, var)
                bw, bb = bn_fold_bounds(w, gamma, beta, mean, var, dt)
                ew, eb = emu_bn_fold(w, gamma, beta, mean, var, dt)
                worst["fold " + tag(dt)] = max(worst.get("fold " + tag(dt), 0.0), within(ew, rw, bw, "fold w"), within(eb, rb, bb, "fold b"))
            K = cin * khw
            gwf, gbf = normal((cout, K), 51 + cin), normal((cout,), 52 + cin)
            start = (normal(tuple(w.shape), 53 + cin), normal((cout,), 54 + cin), normal((cout,), 55 + cin))
            ref = bn_unfold_ref64(gwf, gbf, w, gamma, beta, mean, var, start)
            bounds = bn_unfold_bounds(gwf, gbf, w, gamma, mean, var, start)
            got = emu_bn_unfold(gwf, gbf, w, gamma, mean, var, start)
            bad = emu_bn_unfold(gwf, gbf, w, gamma, mean, var, start, overwrite=True)
            for i in range(3):
                assert bool(torch.isfinite(ref[i]).all())
                worst["unfold"] = max(worst.get("unfold", 0.0), within(got[i], ref[i], bounds[i], "unfold %d" % i))
                assert ratio(bad[i], ref[i], bounds[i]) > 1.0, (cin, khw, cout, i)
    print("RATIO-CPU bn", {k: round(v, 3) for k, v in worst.items()})
