"""CPU: the inputs, references, bounds and case tables that tests/test_gpu_conv.py holds the ModifiedResNet convolution and pool kernels
to (hgr_conv3x3_nhwc, hgr_conv3x3_nhwc_plain, hgr_conv3x3_pool2_nhwc, hgr_stem_conv1 and the streaming kernels around them), tested
here against a plain torch emulation of the kernels' arithmetic - an unsound planted input or a wrong bound is found without a device,
deliberately broken emulations show that the checks bite, and every case's dispatch route is pinned with hgr_gemm_plan_capture.

A case is ONE call: (B, H, W, C, Cout, stride) are the call's own input / output channels.  A `plain` case is the data gradient of the
forward convolution Cout -> C (training_rn._conv3x3_bwd): its x is dY, its weight the flipped forward weight, and its expectation is
autograd's dX of F.conv2d on the same integers.

Planted sparse.  x integers in {-2..2}, one seed per image (no two images equal: a halo chunk left over from another tile or image
changes bits); weights ternary, 24 nonzeros per output channel in a run that starts at column (co * 24) % 9C, random signs; bias integers
in [-4, 4].  Asserted per case: every (tap, channel) column has a nonzero weight in some output channel, every |pre-activation| <= 256:
all values are exact integers in bf16 and f16, any single wrong operand moves an output by at least 1.
Planted dense.  x in {-2..2}, dense ternary weights, integer bias, |sum| < 2^24 (asserted): the fp32 accumulation is exact in any
order, every MAC is live, the expectation is the exact sum rounded once - sensitivity goes down to one unit in the last place.
Planted tie (the dense x and w once more, ReLU cases only).  bias = integer + h + 2^-19, h = half a unit in the last place of the
16-bit type in [16, 32) (2^-4 / 2^-7).  h + 2^-19 is not a 16-bit value (it rounds to h), T + h + 2^-19 is an exact fp32 value for every
integer |T| < 32, and for T in [16, 32) it lies 2^-19 ABOVE a rounding tie of the type: a kernel that rounds the bias to 16 bits, or
rounds the result twice, lands ON the tie and goes down to T instead of up.  The integer biases above are exact in 16 bits and
cannot see that.  The fused pool's inputs are then values the first rounding really changes.

Random with a bound.  N(0, 1) activations (and a run at scale 3), He-scaled weights, against float64 from the same 16-bit operands:
    |got - ref| <= half_ulp16(ref) + n 2^-23 (sum |w| |x| + |bias|),     n = 9C + 1
- the textbook (n - 1) u forward error of an fp32 sum in any order, doubled because the rounding inside an MFMA chain is not documented as
one rounding per add; ReLU is 1-Lipschitz, so the bound carries through it.

The old flat tolerance (tests/test_gpu_kernels.py: max |got - ref| < 3e-2 max(1, max |ref|) for bf16) is evaluated on the same broken
emulations in test_broken_conv_emulation_is_caught: what it lets through is the gap these files close.

Worst error / bound over the cases marked rnd, scales 1 and 3 (CPU: the emulation below; MI355X: tests/test_gpu_conv.py, which also
runs hgr_stem_conv1 and the attention-pool token kernels against their bounds):

    route / kernel        CPU bf16  CPU f16   MI355X bf16  MI355X f16
    v128                  0.988     0.935     0.988        0.935
    tall                  0.921     0.610     0.921        0.610
    k256                  0.910     0.593     0.910        0.593
    duo (row sample)      0.925     0.632     0.925        0.656
    direct32              0.963     0.790     0.963        0.790
    direct64              0.932     0.660     0.932        0.660
    stem_conv1                                0.998        0.986
    attnpool_tokens                           0.974        0.935
    attnpool_tokens_bwd                       0.980        0.979
No ratio exceeds 1.  The half_ulp16 term is tight by construction (a result next to a rounding tie of the type sits at ratio ~ 1), so
values near 1 are expected; the fp32 allowance is never what a correct kernel needs - at C = 64 it is as large as half a unit of f16,
which is why the f16 ratios are lower.
"""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hgr_net_amd import _lib, ops, synth

from test_attention_host import BF16, F16, DTS, half_ulp16, ratio, within

HGR_BF16, HGR_F16 = 0, 1
SPARSE_NNZ = 24
TIE_H = {BF16: 2.0 ** -4, F16: 2.0 ** -7}            # half a unit in the last place in [16, 32)
TIE_EPS = 2.0 ** -19

# (kernel, variant) of hgr_gemm_launch per route name (include/hgr.h: HGR_KERNEL_*; V128_CONV = 2, V128_CONV_TALL = 3; gemm_nt_256 conv = 1;
# gemm_nt_duo conv = 5; the direct kernel's variant = its input channels); the epilogue is BIAS_RELU = 4 or NONE = 0
ROUTES = {"v128": (1, 2), "tall": (1, 3), "k256": (2, 1), "duo": (3, 5), "direct32": (6, 32), "direct64": (6, 64)}

Case = collections.namedtuple("Case", "B H W C Cout stride relu route rnd tile")


def _c(b, h, w, c, cout, stride, relu, route, rnd=False, tile=0):
    return Case(b, h, w, c, cout, stride, relu, route, rnd, tile)


def case_id(cs):
    return "%s-%s-%dx%dx%dx%d-%d-s%d%s" % (cs.route, "relu" if cs.relu else "plain", cs.B, cs.H, cs.W, cs.C, cs.Cout, cs.stride, "-t256" if cs.tile else "")


CONV_CASES = [
    # ---- implicit GEMM, 128 x 128 tiles
    _c(2, 7, 9, 8, 16, 1, True, "v128", rnd=True),       # fewer rows than a tile; K = 72 padded to 128: K-tile chunks with tap >= 9
    _c(2, 7, 9, 16, 8, 1, False, "v128", rnd=True),      # ... and its data gradient
    _c(3, 5, 6, 40, 40, 1, True, "v128"),                # multiply-high division at a non-power-of-two C
    _c(3, 5, 6, 40, 40, 1, False, "v128"),
    _c(2, 6, 5, 192, 132, 1, True, "v128"),              # ragged N (its data gradient would have C = 132)
    _c(3, 10, 11, 64, 64, 1, True, "v128", rnd=True),    # three row tiles, < 4096 input pixels: not the direct kernel
    _c(3, 10, 11, 64, 64, 1, False, "v128", rnd=True),
    _c(2, 7, 9, 64, 128, 2, True, "v128"),               # stride 2 at odd H and W
    _c(2, 8, 8, 24, 48, 2, True, "v128"),
    _c(1, 1, 1, 8, 8, 1, True, "v128"),                  # only the centre tap is live
    _c(1, 1, 1, 8, 8, 1, False, "v128"),
    # ---- tall 256 x 64 tiles
    _c(5, 15, 14, 64, 32, 1, True, "tall", rnd=True),    # 1050 rows, ragged last tile
    _c(5, 15, 14, 64, 32, 1, False, "tall", rnd=True),   # dX of the stem's conv3 (32 -> 64 forward): EPI_NONE on tall tiles
    _c(3, 19, 18, 8, 64, 1, True, "tall"),
    _c(5, 29, 30, 16, 64, 2, True, "tall"),              # stride 2, 15 x 15 out
    _c(15, 16, 17, 64, 64, 1, True, "tall"),             # 4080 pixels: one step below the direct threshold
    _c(15, 16, 17, 64, 64, 1, False, "tall"),
    # ---- 256 x 256 tiles: pinned with hgr_gemm_set_tile(256), and by natural dispatch (163 tiles)
    _c(2, 9, 9, 64, 256, 1, True, "k256", rnd=True, tile=256),
    _c(2, 9, 9, 40, 256, 1, True, "k256", tile=256),     # non-uniform taps
    _c(10, 64, 65, 40, 256, 1, True, "k256"),
    # ---- gemm_nt_duo with the implicit loader
    _c(8, 64, 64, 64, 256, 1, True, "duo", rnd=True),    # exactly 256 tiles, full tiles only
    _c(17, 62, 62, 64, 128, 1, True, "duo", rnd=True),   # 256 tiles, ragged last panel
    _c(25, 41, 64, 64, 256, 1, True, "duo"),             # 65600 rows: 256 full panels + one half panel (the smallest M with tiles_m_half > 0)
    # ---- direct halo-tile kernel, C = 32
    _c(1, 16, 16, 32, 32, 1, True, "direct32", rnd=True), _c(1, 16, 16, 32, 64, 1, True, "direct32", rnd=True),
    _c(1, 16, 16, 32, 32, 1, False, "direct32", rnd=True),
    _c(1, 1, 1, 32, 32, 1, True, "direct32"), _c(1, 1, 1, 32, 64, 1, True, "direct32"), _c(1, 1, 1, 32, 32, 1, False, "direct32"),
    _c(2, 17, 33, 32, 32, 1, True, "direct32"), _c(2, 17, 33, 32, 64, 1, True, "direct32"), _c(2, 17, 33, 32, 32, 1, False, "direct32"),
    _c(2, 5, 70, 32, 32, 1, True, "direct32"), _c(2, 5, 70, 32, 64, 1, True, "direct32"), _c(2, 5, 70, 32, 32, 1, False, "direct32"),
    # 17 x 17 = four ragged tiles: 520 tiles on 512 workgroups; 1040 tiles, up to three per workgroup, both halo buffers reused
    _c(130, 17, 17, 32, 32, 1, True, "direct32"), _c(130, 17, 17, 32, 64, 1, True, "direct32"), _c(130, 17, 17, 32, 32, 1, False, "direct32"),
    _c(260, 17, 17, 32, 64, 1, True, "direct32"),
    # ---- direct 8-wave kernel, C = Cout = 64
    _c(16, 16, 16, 64, 64, 1, True, "direct64", rnd=True), _c(16, 16, 16, 64, 64, 1, False, "direct64", rnd=True),   # exactly 4096 pixels
    _c(5, 29, 31, 64, 64, 1, True, "direct64"), _c(5, 29, 31, 64, 64, 1, False, "direct64"),
    _c(65, 17, 17, 64, 64, 1, True, "direct64"), _c(65, 17, 17, 64, 64, 1, False, "direct64"),                       # 260 tiles on 256 workgroups
    _c(130, 17, 17, 64, 64, 1, True, "direct64"), _c(130, 17, 17, 64, 64, 1, False, "direct64"),
]
# an output view that is 8-byte but not 16-byte aligned leaves the direct kernel for the implicit GEMM (and stays exact)
MISALIGNED_OUT_CASES = [(_c(1, 16, 16, 32, 32, 1, True, "v128"), 8), (_c(2, 17, 33, 32, 64, 1, True, "tall"), 8),
                        (_c(1, 16, 16, 32, 32, 1, False, "v128"), 8)]
SAMPLED = {cs for cs in CONV_CASES if cs.route == "duo" and cs.rnd}            # random bound on a row sample only

POOL_SHAPES = [(1, 2, 2), (1, 16, 16), (2, 18, 34), (130, 18, 18)]             # (B, H, W) of hgr_conv3x3_pool2_nhwc, Cout 32 and 64
POOL_CASES = [_c(b, h, w, 32, cout, 1, True, "direct32") for (b, h, w) in POOL_SHAPES for cout in (32, 64)]
STEM_CASES = [(1, 4, 8), (2, 8, 24), (3, 36, 40), (1, 68, 48), (1, 1024, 48)]    # (b, R, Cout); (1, 1024, 48): 61872 bytes of LDS
STEM_RANDOM = (3, 36, 40)
STEM_IM2COL_R = [2, 5, 7, 20]
AVGPOOL_SHAPES = [(1, 2, 2, 8), (2, 6, 10, 24), (3, 4, 18, 64)]
ATTNPOOL_SHAPES = [(1, 1, 8), (3, 7, 64), (2, 3, 2048)]                          # (b, S, C): S the side, S * S cells
IM2COL_T_SHAPES = [(1, 1, 1), (3, 1, 9), (2, 5, 1), (2, 3, 3), (3, 7, 9)]        # (b, H, W), C = 8, ld padded to 64
ELEMWISE_N = [8, 4616]
ELEMWISE_BIG = 32768 * 256 * 8 + 4616                                            # the grid-stride loop's second pass


def kp_of(c):
    return (9 * c + 63) // 64 * 64


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def seed_of(cs):
    return 7919 * (CONV_CASES + POOL_CASES + [m[0] for m in MISALIGNED_OUT_CASES]).index(cs) + 11


# ---- planted operands --------------------------------------------------------------------------------------------------------------------
def plant_x(b, h, w, c, seed, lo=-2, hi=2):
    """[b, h, w, c] float32 integers in {lo..hi}, one seed per image."""
    return torch.stack([torch.from_numpy(synth.randint(100003 * seed + i, "conv.x", h * w * c, lo, hi + 1).astype(np.float32)).view(h, w, c)
                        for i in range(b)])


def plant_w_sparse(c, cout, seed):
    """[cout, 9c] ternary: SPARSE_NNZ nonzeros per row in a run from column (co * SPARSE_NNZ) % 9c, random signs."""
    k = 9 * c
    sign = np.where(synth.uniform(seed, "conv.ws", cout * SPARSE_NNZ) < 0.5, -1.0, 1.0).astype(np.float32).reshape(cout, SPARSE_NNZ)
    cols = (np.arange(cout)[:, None] * SPARSE_NNZ + np.arange(SPARSE_NNZ)[None, :]) % k
    w = torch.zeros(cout, k)
    w.scatter_(1, torch.from_numpy(cols), torch.from_numpy(sign))
    return w


def plant_w_dense(c, cout, seed):
    return torch.from_numpy(synth.randint(seed, "conv.wd", cout * 9 * c, -1, 2).astype(np.float32)).view(cout, 9 * c)


def plant_bias(cout, seed):
    return torch.from_numpy(synth.randint(seed, "conv.b", cout, -4, 5).astype(np.float32))


def tie_bias(cout, dt, seed):
    """integer + h + 2^-19 (fp32): 2^-19 above a rounding tie of `dt` once an integer sum in [16, 32) is added; rounds to integer + h in dt."""
    b = (plant_bias(cout, seed + 1).double() + TIE_H[dt] + TIE_EPS).float()
    assert torch.equal(b.double(), plant_bias(cout, seed + 1).double() + TIE_H[dt] + TIE_EPS)       # exact in fp32
    return b


def flip_weight(w, c, cout):
    """w [cout, 9c] (ky, kx, c) of a convolution c -> cout  ->  [c, 9 cout] of its data gradient cout -> c (an involution)."""
    return w.view(cout, 3, 3, c).flip(1, 2).permute(3, 1, 2, 0).reshape(c, 9 * cout).contiguous()


def pack_w(w, dt, kp=None):
    """[cout, Kp] of type dt: the live 9c columns, zeros beyond (the folded layout)."""
    kp = kp_of(w.shape[1] // 9) if kp is None else kp
    out = torch.zeros(w.shape[0], kp, dtype=dt)
    out[:, :w.shape[1]] = w.to(dt)
    return out


def conv_sum(x, w, stride=1):
    """sum_{ky, kx, c} w x, pad 1: x [b, h, w, c] NHWC, w [cout, 9c] in (ky, kx, c) order -> [b * ho * wo, cout]; in x's precision."""
    cout, c = w.shape[0], x.shape[3]
    y = F.conv2d(x.permute(0, 3, 1, 2), w.to(x.dtype).view(cout, 3, 3, c).permute(0, 3, 1, 2), stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, cout)


def autograd_dx(dy, w_call):
    """dX of F.conv2d (pad 1, stride 1) for the forward weight whose flip is w_call [c_out_of_call, 9 c_in_of_call]; dy [b, h, w, c_in_of_call]."""
    b, h, wd, cin = dy.shape
    cout = w_call.shape[0]
    wf = flip_weight(w_call, cin, cout)                                # forward weight [cin (forward outputs), 9 cout (forward inputs)]
    x0 = torch.zeros(b, cout, h, wd, dtype=dy.dtype, requires_grad=True)
    F.conv2d(x0, wf.to(dy.dtype).view(cin, 3, 3, cout).permute(0, 3, 1, 2), padding=1).backward(dy.permute(0, 3, 1, 2))
    return x0.grad.permute(0, 2, 3, 1).reshape(-1, cout)


@functools.lru_cache(maxsize=6)
def planted(cs, kind):
    """(x [B, H, W, C], w [Cout, 9C], S [M, Cout]) float32, all integers: S the exact sums without the bias.  kind: sparse | dense."""
    seed = seed_of(cs)
    x = plant_x(cs.B, cs.H, cs.W, cs.C, seed)
    w = plant_w_sparse(cs.C, cs.Cout, seed) if kind == "sparse" else plant_w_dense(cs.C, cs.Cout, seed)
    s = conv_sum(x, w, cs.stride) if cs.relu else autograd_dx(x, w)
    return x, w, s


def planted_bias(cs, kind, dt):
    """None for a plain case; integers in [-4, 4]; kind == "tie": tie_bias."""
    if not cs.relu:
        return None
    return tie_bias(cs.Cout, dt, seed_of(cs)) if kind == "tie" else plant_bias(cs.Cout, seed_of(cs))


def kinds_of(cs):
    return ("sparse", "dense", "tie") if cs.relu else ("sparse", "dense")


def expect(s, bias, relu, dt):
    """The exact pre-activation (float64; S + bias is an exact fp32 value wherever a tie is near, see the head of the file), ReLU, ONE rounding."""
    v = s.double() if bias is None else s.double() + bias.double()
    return (torch.relu(v) if relu else v).float().to(dt)


def planted_expect(cs, kind, dt):
    """x, w [Cout, Kp] and the expected output [M, Cout] of type dt, the fp32 bias or None."""
    x, w, s = planted(cs, "dense" if kind == "tie" else kind)
    bias = planted_bias(cs, kind, dt)
    return x.to(dt), pack_w(w, dt), bias, expect(s, bias, cs.relu, dt)


def pool_expect(y16, b, h, w, cout):
    """avgpool2 of the 16-bit conv output [b * h * w, cout]: the fp32 average of four, rounded once."""
    y = y16.float().view(b, h, w, cout)
    return ((y[:, 0::2, 0::2] + y[:, 0::2, 1::2] + y[:, 1::2, 0::2] + y[:, 1::2, 1::2]) * 0.25).to(y16.dtype).reshape(-1, cout)


# ---- random operands and the float64 reference ------------------------------------------------------------------------------------------------
def rand_inputs(cs, scale, dt):
    seed = seed_of(cs) + int(scale)
    n = cs.B * cs.H * cs.W * cs.C
    x = torch.from_numpy((scale * synth.normal(seed, "conv.rx", n)).astype(np.float32)).view(cs.B, cs.H, cs.W, cs.C).to(dt)
    w = torch.from_numpy(((2.0 / (9 * cs.C)) ** 0.5 * synth.normal(seed, "conv.rw", cs.Cout * 9 * cs.C)).astype(np.float32)).view(cs.Cout, 9 * cs.C).to(dt)
    bias = torch.from_numpy((0.1 * synth.normal(seed, "conv.rb", cs.Cout)).astype(np.float32)) if cs.relu else None
    return x, w, bias


def im2col(x, stride=1, rows=None, no_hpad=False, drop=None, stale=None, bump=None):
    """The implicit im2col as the kernels index it: [n, 9c] in (ky, kx, c) order for the output rows `rows` (default all), zeros outside
    the image.  The three mistakes the planted inputs must catch: no_hpad - no horizontal pad, a tap left of x = 0 wraps to the previous
    row; drop = (row, tap) - that tap of that output pixel reads zeros; stale = (row, tap, ch0) - channels ch0 .. ch0 + 7 of that tap
    come from the same place of the PREVIOUS image; bump = (row, tap, ch) - that one operand is off by 1."""
    b, h, w, c = x.shape
    ho, wo = out_hw(h, w, stride)
    r = torch.arange(b * ho * wo) if rows is None else rows
    bi, oy, ox = r // (ho * wo), (r // wo) % ho, r % wo
    flat = x.reshape(b * h * w, c)
    cols = []
    for t in range(9):
        hi, wi = oy * stride - 1 + t // 3, ox * stride - 1 + t % 3
        ok = (hi >= 0) & (hi < h)
        if not no_hpad:
            ok = ok & (wi >= 0) & (wi < w)
        idx = (bi * h + hi) * w + wi
        ok = ok & (idx >= 0) & (idx < b * h * w)
        cols.append(flat[idx.clamp(0, b * h * w - 1)] * ok[:, None].to(x.dtype))
    col = torch.stack(cols, 1)
    if drop is not None:
        col[drop[0], drop[1]] = 0
    if bump is not None:
        col[bump] += 1
    if stale is not None:
        row, tap, ch0 = stale
        col[row, tap, ch0:ch0 + 8] = col[row - ho * wo, tap, ch0:ch0 + 8]
    return col.reshape(-1, 9 * c)


def sample_rows(cs, seed=5):
    """The rows the large cases are checked on: the first and the last image, both rows at every 256-row tile edge, 4096 random rows."""
    ho, wo = out_hw(cs.H, cs.W, cs.stride)
    m, per = cs.B * ho * wo, ho * wo
    edges = torch.arange(256, m, 256)
    rnd = torch.from_numpy(synth.randint(seed, "conv.rows", 4096, 0, m))
    return torch.unique(torch.cat([torch.arange(per), torch.arange(m - per, m), edges - 1, edges, torch.tensor([m - 1]), rnd]))


def ref_random(cs, x16, w16, bias, dt, rows=None):
    """float64 from the 16-bit operands and the element-wise bound, for all output rows or `rows`."""
    if rows is None:
        s, mag = conv_sum(x16.double(), w16.double(), cs.stride), conv_sum(x16.double().abs(), w16.double().abs(), cs.stride)
    else:
        col = im2col(x16.double(), cs.stride, rows)
        s, mag = col @ w16.double().t(), col.abs() @ w16.double().abs().t()
    if bias is not None:
        s, mag = s + bias.double(), mag + bias.double().abs()
    ref = torch.relu(s) if cs.relu else s
    return ref, half_ulp16(ref, dt) + (9 * cs.C + 1) * 2.0 ** -23 * mag


# ---- emulation of the kernels' arithmetic ----------------------------------------------------------------------------------------------------
def emu_conv(x16, w16, bias, stride, relu, dt, bias16=False, keep32=False, **broken):
    """Implicit im2col, fp32 products and sums, the fp32 bias, ReLU, ONE rounding.  bias16: the bias rounded to 16 bits first (a mistake);
    keep32: the unrounded fp32 result (for emu_pool's mistake)."""
    acc = im2col(x16.float(), stride, **broken) @ w16.float().t()
    if bias is not None:
        acc = acc + (bias.to(dt).float() if bias16 else bias)
    acc = torch.relu(acc) if relu else acc
    return acc if keep32 else acc.to(dt)


def emu_pool(x16, w16, bias, b, h, w, dt, average_first=False):
    """conv, rounded to 16 bits, then the fp32 average of four, rounded.  average_first: the pool reads the UNROUNDED values (a mistake)."""
    cout = w16.shape[0]
    y = emu_conv(x16, w16, bias, 1, True, dt, keep32=average_first)
    if not average_first:
        return pool_expect(y, b, h, w, cout)
    y = y.view(b, h, w, cout)
    return ((y[:, 0::2, 0::2] + y[:, 0::2, 1::2] + y[:, 1::2, 0::2] + y[:, 1::2, 1::2]) * 0.25).to(dt).reshape(-1, cout)


def emu_avgpool2_bwd(dy, b, h, w, dt, swapped=False):
    """dx[b, y, x] = dy[b, y / 2, x / 2] / 4 by the kernel's flat index arithmetic; swapped: H and W exchanged in it (a mistake)."""
    if swapped:
        h, w = w, h
    pix = torch.arange(b * h * w)
    src = ((pix // (w * h)) * (h // 2) + ((pix // w) % h) // 2) * (w // 2) + (pix % w) // 2
    return (dy.float()[src] * 0.25).to(dt)


# ---- the streaming kernels' inputs and references ------------------------------------------------------------------------------------------------
def avgpool_inputs(b, h, w, c, dt):
    """x [b, h, w, c] integers in [-128, 128] (the average of four has two more bits than bf16 holds: a real rounding); dy = 4 * integers
    in [-31, 31] (dy / 4 exact); the references: the fp32 average rounded once, autograd's gradient of avg_pool2d."""
    x = plant_x(b, h, w, c, 900 + h * w, -128, 128)
    fwd = pool_expect(x.to(dt).reshape(-1, c), b, h, w, c)
    dy = 4.0 * plant_x(b, h // 2, w // 2, c, 901 + h * w, -31, 31)
    x0 = torch.zeros(b, c, h, w, requires_grad=True)
    F.avg_pool2d(x0, 2).backward(dy.permute(0, 3, 1, 2))
    return x.to(dt).reshape(-1, c), fwd, dy.to(dt).reshape(-1, c), x0.grad.permute(0, 2, 3, 1).reshape(-1, c).to(dt)


def attnpool_tokens_ref(x16, pos, b, s, c, dt):
    """tokens = cat(mean over the s * s cells, cells) + pos in float64 [b * (s * s + 1), c] and the bound."""
    g = s * s
    cells = x16.double().view(b, g, c)
    ref = (torch.cat([cells.mean(1, keepdim=True), cells], 1) + pos.double()).reshape(-1, c)
    return ref, half_ulp16(ref, dt) + 2.0 ** -23 * g * float(cells.abs().max())


def attnpool_tokens_bwd_ref(dtok16, b, cells, c, dt):
    """dx[b, p] = dtok[b, 1 + p] + dtok[b, 0] / cells in float64 [b * cells, c] and the bound: 1 / cells, the product and the sum round."""
    d = dtok16.double().view(b, cells + 1, c)
    t, m = d[:, 1:], d[:, :1] / cells
    ref = (t + m).reshape(-1, c)
    return ref, half_ulp16(ref, dt) + 2.0 ** -23 * (t.abs() + m.abs()).reshape(-1, c)


def stem_inputs(b, r, cout, seed):
    """image fp32 [b, 3, r, r] integers in {-2..2}, w [cout, 27] ternary (dense: all 27 columns live), integer bias, the exact sums
    [b * ho * ho, cout] of the stride-2 convolution."""
    img = plant_x(b, r, r, 3, seed)                                  # NHWC integers
    w = plant_w_dense(3, cout, seed)
    return img.permute(0, 3, 1, 2).contiguous(), w, plant_bias(cout, seed), conv_sum(img, w, 2)


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def _fake(i, off=0):
    """Operand i of a planned call: distinct, 4 KiB-aligned, never dereferenced (tests/workers/gemm_plan_replay.py)."""
    return 0x100000000000 * (i + 1) + off


def plan_of(cs, out_off=0):
    """The launches hgr_gemm_plan_capture records for the case's call; nothing is launched."""
    kp = kp_of(cs.C)
    if cs.relu:
        fn = lambda: _lib.call("hgr_conv3x3_nhwc", _fake(0), _fake(1), _fake(2), _fake(3, out_off), cs.B, cs.H, cs.W, cs.C, cs.Cout, cs.stride, kp, HGR_F16, 0)
    else:
        fn = lambda: _lib.call("hgr_conv3x3_nhwc_plain", _fake(0), _fake(1), _fake(3, out_off), cs.B, cs.H, cs.W, cs.C, cs.Cout, kp, HGR_F16, 0)
    prev = ops.gemm_set_tile(cs.tile) if cs.tile else None
    try:
        return ops.gemm_plan(fn)
    finally:
        if prev is not None:
            ops.gemm_set_tile(prev)


def check_route(cs, out_off=0):
    plan = plan_of(cs, out_off)
    assert len(plan) == 1, plan
    got = (plan[0]["kernel"], plan[0]["variant"], plan[0]["epilogue"])
    assert got == ROUTES[cs.route] + (4 if cs.relu else 0,), (case_id(cs), plan)
    return plan[0]


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
def _old_flat_tolerance_passes(got, ref, dt):
    """tests/test_gpu_kernels.py::test_conv3x3_implicit_gemm_vs_conv2d's criterion."""
    tol = 3e-2 if dt == BF16 else 4e-3
    return float((got.double() - ref).abs().max()) < tol * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("cs", CONV_CASES + POOL_CASES + [m[0] for m in MISALIGNED_OUT_CASES], ids=case_id)
def test_planted_inputs_meet_their_conditions(cs):
    for kind in ("sparse", "dense"):
        x, w, s = planted(cs, kind)
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 2 and bool((w.abs() <= 1).all()) and bool((w == w.round()).all())
        if cs.B > 1 and cs.H * cs.W * cs.C >= 64:                                          # images pairwise different
            assert len(torch.unique(x.reshape(cs.B, -1), dim=0)) == cs.B
        assert bool((w != 0).any(0).all()), "a (tap, channel) column without a weight"
        assert bool((s == s.round()).all())
        top = float(s.abs().max()) + 4 + 1                                                     # |S + bias|, the tie bias included
        if kind == "sparse":
            assert int((w != 0).sum(1).max()) <= SPARSE_NNZ and top <= 256, top
        else:
            assert top < 2 ** 24 and top < 65504
        for dt in DTS:                                                                         # exact in both types
            assert torch.equal(x.to(dt).float(), x) and torch.equal(w.to(dt).float(), w)
            if kind == "sparse":
                assert torch.equal(expect(s, planted_bias(cs, kind, dt), cs.relu, dt).double(),
                                   torch.relu(s.double() + planted_bias(cs, kind, dt).double()) if cs.relu else s.double())
    if cs.relu and cs.B * cs.H * cs.W >= 64 and cs.C >= 16:                                  # the tie bias has outputs to bite on
        s = planted(cs, "dense")[2]
        for dt in DTS:
            t = s.double() + plant_bias(cs.Cout, seed_of(cs) + 1).double()
            assert int(((t >= 16) & (t < 32)).sum()) > 0
            assert torch.equal(tie_bias(cs.Cout, dt, seed_of(cs)).to(dt).double(), plant_bias(cs.Cout, seed_of(cs) + 1).double() + TIE_H[dt])


def test_data_gradient_is_the_plain_convolution_with_the_flipped_weight():
    """autograd's dX of F.conv2d equals conv_sum(dY, flip_weight(w)): the convention of training_rn._conv3x3_bwd, on integers, exact."""
    for cs in (c for c in CONV_CASES if not c.relu and c.B * c.H * c.W < 5000):
        for kind in ("sparse", "dense"):
            x, w, s = planted(cs, kind)
            assert torch.equal(s, conv_sum(x, w, 1)), case_id(cs)
            assert torch.equal(flip_weight(flip_weight(w, cs.C, cs.Cout), cs.Cout, cs.C), w)


@pytest.mark.parametrize("cs", CONV_CASES, ids=case_id)
def test_routes(cs):
    """Every case reaches the kernel, variant and epilogue it was written for (256 CUs: an MI355X, and what the library assumes without
    a device)."""
    L = check_route(cs)
    if cs.route == "duo":
        m = cs.B * cs.H * cs.W
        assert L["tiles_m"] == -(-m // 256) and L["tiles_n"] == cs.Cout // 128
        if (cs.B, cs.H, cs.W) == (8, 64, 64):
            assert L["grid_x"] == 256 and L["tiles_m_half"] == 0 and m % 256 == 0
        if (cs.B, cs.H, cs.W) == (17, 62, 62):
            assert L["grid_x"] == 256 and L["tiles_m_half"] == 0 and m % 256 != 0
        if (cs.B, cs.H, cs.W) == (25, 41, 64):
            assert L["tiles_m_half"] == 1 and L["big_panels"] == 256, L
    if cs.route == "k256" and not cs.tile:
        assert L["grid_x"] == 163
    if cs.route in ("v128", "tall", "k256"):
        ho, wo = out_hw(cs.H, cs.W, cs.stride)
        assert L["rows"] == cs.B * ho * wo
    if cs.route == "tall":
        assert L["rows"] >= 1024 and L["grid_x"] == -(-L["rows"] // 256)


def test_routes_of_misaligned_outputs_and_thresholds():
    for cs, off in MISALIGNED_OUT_CASES:
        check_route(cs, off)
        assert check_route(cs._replace(route="direct32"), 0)["kernel"] == 6                   # the aligned call is the direct kernel's
    # one pixel fewer than 4096 leaves the 8-wave kernel; the forced tile is back at 0 after plan_of
    assert check_route(_c(16, 16, 16, 64, 64, 1, True, "direct64"))["variant"] == 64
    check_route(_c(15, 16, 17, 64, 64, 1, True, "tall"))
    assert ops.gemm_set_tile(0) == 0


EMU_CASES = [cs for cs in CONV_CASES if cs.B * cs.H * cs.W <= 5000]


@pytest.mark.parametrize("cs", EMU_CASES, ids=case_id)
def test_emulation_reproduces_planted_expectations(cs):
    for dt in DTS:
        for kind in kinds_of(cs):
            x, w, bias, want = planted_expect(cs, kind, dt)
            got = emu_conv(x, w[:, :9 * cs.C], bias, cs.stride, cs.relu, dt)
            assert torch.equal(got.double(), want.double()), (case_id(cs), kind, dt)


@pytest.mark.parametrize("cs", POOL_CASES[:6], ids=case_id)
def test_pool_emulation_reproduces_planted_expectations(cs):
    for dt in DTS:
        for kind in kinds_of(cs):
            x, w, bias, want = planted_expect(cs, kind, dt)
            got = emu_pool(x, w[:, :288], bias, cs.B, cs.H, cs.W, dt)
            assert torch.equal(got.double(), pool_expect(want, cs.B, cs.H, cs.W, cs.Cout).double())


_worst = {}


@pytest.mark.parametrize("cs", [c for c in CONV_CASES if c.rnd], ids=case_id)
def test_emulation_stays_within_the_random_bound(cs):
    for dt in DTS:
        for scale in (1.0, 3.0):
            x, w, bias = rand_inputs(cs, scale, dt)
            rows = sample_rows(cs)[::8] if cs in SAMPLED else None
            ref, bound = ref_random(cs, x, w, bias, dt, rows)
            got = (im2col(x.float(), cs.stride, rows) @ w.float().t())
            got = got + bias if bias is not None else got
            got = (torch.relu(got) if cs.relu else got).to(dt)
            key = (cs.route, "bf16" if dt == BF16 else "f16")
            _worst[key] = max(_worst.get(key, 0.0), within(got, ref, bound, (case_id(cs), scale)))
    print("worst error / bound so far:", {k: round(v, 3) for k, v in sorted(_worst.items())})


MUTANT_CASE = _c(3, 10, 11, 64, 64, 1, True, "v128", rnd=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("broken", ["no_hpad", "tap_dropped", "stale_chunk", "one_operand", "bias16"])
def test_broken_conv_emulation_is_caught(dt, broken):
    """Each mistake changes bits of a planted expectation: the four that touch operands those of BOTH the sparse and the dense input, the
    bias rounded to 16 bits those of the tie input (integer biases are exact in 16 bits).  On N(0, 1) data the random bound refuses the
    four operand mistakes; the 16-bit bias stays inside it at C = 64 (error / bound 0.98 bf16, 0.59 f16: the fp32 allowance n 2^-23 sum
    |w| |x| is then as large as the bias's rounding error) - the tie input is what catches it.
    The old flat tolerance (3e-2 / 4e-3 of max(1, max |ref|), 0.157 / 0.021 here) refuses the missing pad (error 3.1), the dropped tap (0.99)
    and the stale chunk (0.38) but passes the 16-bit bias (0.015 / 0.002) in both types and one operand off by 1 (error max |w| = 0.1) in
    bf16 - the gap these tests close."""
    cs = MUTANT_CASE
    ho, wo = out_hw(cs.H, cs.W, cs.stride)
    corner = 2 * ho * wo - 1                                                   # the last pixel of image 1: tap 0 is inside the image
    kw = dict(no_hpad=dict(no_hpad=True), tap_dropped=dict(drop=(corner, 0)), stale_chunk=dict(stale=(corner - 5, 4, 8)),
              one_operand=dict(bump=(corner - 7, 4, 13)), bias16=dict(bias16=True))[broken]
    for kind in kinds_of(cs):
        x, w, bias, want = planted_expect(cs, kind, dt)
        got = emu_conv(x, w[:, :9 * cs.C], bias, cs.stride, cs.relu, dt, **kw)
        assert torch.equal(got, want) == (broken == "bias16" and kind != "tie"), kind
    x, w, bias = rand_inputs(cs, 1.0, dt)
    ref, bound = ref_random(cs, x, w, bias, dt)
    bad = emu_conv(x, w, bias, cs.stride, cs.relu, dt, **kw)
    assert (ratio(bad, ref, bound) > 1.0) == (broken != "bias16")
    assert _old_flat_tolerance_passes(bad, ref, dt) == (broken == "bias16" or (broken == "one_operand" and dt == BF16))


@pytest.mark.parametrize("dt", DTS)
def test_pool_that_averages_before_rounding_is_caught(dt):
    """The fused pool must average the 16-bit conv outputs.  Integer conv outputs are exact in 16 bits, so only the tie input sees a
    pool that averages the fp32 values; on N(0, 1) data the difference is a fraction of a unit in the last place and the old flat tolerance
    passes it."""
    cs = POOL_CASES[2]                                                          # (1, 16, 16), Cout 32
    x, w, bias, want = planted_expect(cs, "tie", dt)
    good = emu_pool(x, w[:, :288], bias, cs.B, cs.H, cs.W, dt)
    assert torch.equal(good, pool_expect(want, cs.B, cs.H, cs.W, cs.Cout))
    assert not torch.equal(emu_pool(x, w[:, :288], bias, cs.B, cs.H, cs.W, dt, average_first=True), good)
    x, w, bias = rand_inputs(cs, 1.0, dt)
    y = emu_conv(x, w, bias, 1, True, dt)
    ref = pool_expect(y, cs.B, cs.H, cs.W, cs.Cout)
    bad = emu_pool(x, w, bias, cs.B, cs.H, cs.W, dt, average_first=True)
    assert not torch.equal(bad, ref) and _old_flat_tolerance_passes(bad, ref.double(), dt)


@pytest.mark.parametrize("dt", DTS)
def test_avgpool2_bwd_with_h_and_w_swapped_is_caught(dt):
    """At H = W = 6 - the only shape the kernel was tested at - a swap of H and W changes nothing; at 6 x 10 and 4 x 18 it does."""
    for b, h, w, c in AVGPOOL_SHAPES + [(2, 6, 6, 64)]:
        _, _, dy, want = avgpool_inputs(b, h, w, c, dt)
        assert torch.equal(emu_avgpool2_bwd(dy, b, h, w, dt), want)
        assert torch.equal(emu_avgpool2_bwd(dy, b, h, w, dt, swapped=True), want) == (h == w), (h, w)


def test_stem_inputs_are_exact_and_live():
    for b, r, cout in STEM_CASES:
        img, w, bias, s = stem_inputs(b, r, cout, 40 + r)
        assert bool((w != 0).any(0).all()) and float(s.abs().max()) + 4 <= 256 and bool((s == s.round()).all())
        assert tuple(s.shape) == (b * (r // 2) ** 2, cout)
        nhwc = img.permute(0, 2, 3, 1)
        if r <= 68:                                                            # the two restatements agree: conv2d and the index arithmetic
            assert torch.equal(im2col(nhwc, 2) @ w.t(), s)
        lds = ((27 * (r + 8) * 2 + 15) & ~15) + 4 * 16 * ((cout + 15) // 16) * 32
        assert lds <= 64 * 1024 and (r != 1024 or lds == 61872)


def test_conv_entry_points_refuse_before_any_launch():
    """The argument checks of the conv entry points return before anything is planned or launched, with a message that names the entry
    point; tests/test_gpu_conv.py repeats them on device buffers that must stay unwritten."""
    lib = _lib.load()
    p = _fake

    def refused(fn, name):
        with pytest.raises(_lib.HgrError) as err:
            fn()
        assert name in str(err.value), str(err.value)

    conv = lambda c, cout, kp, xoff=0: (lambda: _lib.call("hgr_conv3x3_nhwc", p(0, xoff), p(1), p(2), p(3), 2, 6, 6, c, cout, 1, kp, HGR_F16, 0))
    for fn in (conv(12, 16, 128), conv(8, 18, 128), conv(16, 16, 128), conv(8, 16, 128, xoff=2)):
        refused(fn, "hgr_conv3x3_nhwc")
    refused(lambda: _lib.call("hgr_conv3x3_pool2_nhwc", p(0), p(1), p(2), p(3), 1, 5, 6, 32, 32, 320, HGR_F16, 0), "hgr_conv3x3_pool2_nhwc")
    refused(lambda: _lib.call("hgr_stem_conv1", p(0), p(1), p(2), p(3), 1, 6, 32, 64, HGR_F16, 0), "hgr_stem_conv1")
    refused(lambda: _lib.call("hgr_stem_conv1", p(0), p(1), p(2), p(3), 1, 8, 56, 64, HGR_F16, 0), "hgr_stem_conv1")
    for name in ("hgr_relu_bwd16", "hgr_add16"):
        refused(lambda: _lib.call(name, p(0), p(1), p(2), 12, HGR_F16, 0), name)
    assert lib.hgr_gemm_plan_capture(None, 0) == 0
