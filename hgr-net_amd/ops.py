"""Tensor-level wrappers over the C ABI: take torch CUDA(HIP) tensors, pass raw device pointers,
sizes and the current HIP stream to libhgr.so.  torch is plumbing here (device memory, streams);
all arithmetic happens in the hand-written kernels."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_ACCUM, EPI_BIAS, EPI_BIAS_ADD16_RELU, EPI_BIAS_QUICKGELU, EPI_BIAS_RELU, EPI_BIAS_RESIDUAL, EPI_NONE, EPI_QGELU_GRAD16,
                   HGR_BF16, HGR_F16)

# when a list, every gemm_nt call appends (name, start_event, end_event, algorithmic flops, algorithmic bytes, tag);
# events are recorded on the launch stream (torch's current stream).  Used by bench.py's roofline pass only.
PROFILE = None

# bumped by every raw kernel that writes parameter storage behind torch's back (hgr_adamw): tensors written through a
# ctypes pointer keep their data_ptr and _version, so caches keyed on those (CLIP._prepared, the HIP graphs of
# tree_model.forward) also key on this counter.
WEIGHTS_GEN = [0]

# set by tree_model while it captures the head / tail graphs of a pipelined evaluation step (model/clip_tree.py): called at the point
# of the step behind which only the class-token rows are worked on (clip/model.py:_run_blocks)
SPLIT_HOOK = None


def split_point(name: str) -> None:
    h = SPLIT_HOOK
    if h is not None:
        h(name)


TORCH16 = {HGR_BF16: torch.bfloat16, HGR_F16: torch.float16}
# the residual stream between the folded-LayerNorm GEMMs is a PAIR (csrc/hgr_common.h: pair_split / pair_dec): hi = x rounded to the
# MFMA type and one byte q = the next 8 mantissa bits of x (19 significant bits with f16, 3 bytes).  PAIR_LO is the byte plane's dtype.
PAIR_LO = torch.uint8


def pair_value(xh: torch.Tensor, xl: torch.Tensor) -> torch.Tensor:
    """fp32 value of every row of the pair (decoded by hgr_pair_rows_f32 - the kernels' own decoder)."""
    out = torch.empty(xh.shape, dtype=torch.float32, device=xh.device)
    return pair_rows_f32(xh.contiguous(), xl.contiguous(), out)
DT_OF = {torch.bfloat16: HGR_BF16, torch.float16: HGR_F16}


def dtype_code(name) -> int:
    if name in (HGR_BF16, HGR_F16):
        return name
    return {"bf16": HGR_BF16, "bfloat16": HGR_BF16, "f16": HGR_F16, "fp16": HGR_F16, "float16": HGR_F16,
            torch.bfloat16: HGR_BF16, torch.float16: HGR_F16}[name]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Optional[torch.Tensor]) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise _lib.HgrError("libhgr ops need device tensors (no CPU path)")
    return t.data_ptr()


def gemm_nt(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
            residual: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE, n: Optional[int] = None, tag: str = "") -> torch.Tensor:
    """out[M, :N] = epilogue(a[M,K] @ w[N,K]^T); `out` fp32 or the operands' 16-bit type (may be wider than N).
    `tag` only labels the PROFILE record (bench.py's roofline pass)."""
    assert a.dim() == 2 and w.dim() == 2 and out.dim() == 2 and a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1
    m, k = a.shape
    nn = w.shape[0] if n is None else n
    assert w.shape[1] == k and out.shape[0] == m and out.shape[1] >= nn and out.stride(1) == 1
    out32 = out.dtype == torch.float32
    assert out32 or out.dtype == a.dtype
    if residual is not None:
        assert residual.stride(1) == 1 and residual.dtype == (a.dtype if epilogue in (EPI_BIAS_ADD16_RELU, EPI_QGELU_GRAD16) else torch.float32)
    prof = PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    _lib.call("hgr_gemm_nt", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(out), out.stride(0),
              _dev(bias), _dev(residual), residual.stride(0) if residual is not None else 0,
              m, nn, k, DT_OF[a.dtype], epilogue, 1 if out32 else 0, _stream())
    if prof is not None:
        ev1.record()
        byts = 2 * m * k + 2 * nn * k + (4 if out32 else 2) * m * nn + (4 * m * nn if residual is not None else 0)
        prof.append(("gemm_nt", ev0, ev1, 2.0 * m * nn * k, float(byts), tag))
    return out


def _prof_begin():
    if PROFILE is None:
        return None
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    return ev0, ev1


def _prof_end(ev, flops, byts, tag):
    if ev is not None:
        ev[1].record()
        PROFILE.append(("gemm_nt", ev[0], ev[1], float(flops), float(byts), tag))


# Range guard of the LayerNorm-folded residual stream (hgr_gemm_nt_res_stats_guard): a 64-column slot whose sum of squares exceeds
# LN_GUARD_SUMSQ = 16384^2 could hold an element beyond a quarter of the f16 range (65504); below it every |x| <= 16384.
LN_GUARD_SUMSQ = 16384.0 ** 2


def gemm_nt_res_stats(a: torch.Tensor, w: torch.Tensor, xh: torch.Tensor, xl: torch.Tensor, bias: torch.Tensor, stats: torch.Tensor,
                      tag: str = "", flag: Optional[torch.Tensor] = None) -> None:
    """(xh, xl) += a @ w^T + bias on the residual stream kept as a pair (xh = x in the MFMA type = the next GEMM's A operand, xl one
    byte per element: the rounding error of xh on an 8-bit grid, see PAIR_LO) and, for the LayerNorm that follows, stats[m, slot] = (sum, sum of squares) of every 64-column slot of the
    new row (hgr_gemm_nt_res_stats).  `flag` (uint32 / int32 [1], zeroed by the caller): range guard, non-zero afterwards when a
    slot's sum of squares exceeded LN_GUARD_SUMSQ or was inf / NaN (hgr_gemm_nt_res_stats_guard)."""
    m, k = a.shape
    n = w.shape[0]
    assert a.dtype == w.dtype == xh.dtype and xl.dtype == PAIR_LO and xh.shape == xl.shape == (m, n) and xh.stride() == xl.stride()
    assert stats.dtype == torch.float32 and stats.numel() >= m * (n // 64) * 2 and a.stride(1) == w.stride(1) == xh.stride(1) == 1
    ev = _prof_begin()
    if flag is None:
        _lib.call("hgr_gemm_nt_res_stats", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(xh), _dev(xl), xh.stride(0), _dev(bias),
                  _dev(stats), m, n, k, DT_OF[a.dtype], _stream())
    else:
        assert flag.numel() == 1 and flag.element_size() == 4
        _lib.call("hgr_gemm_nt_res_stats_guard", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(xh), _dev(xl), xh.stride(0), _dev(bias),
                  _dev(stats), LN_GUARD_SUMSQ, _dev(flag), m, n, k, DT_OF[a.dtype], _stream())
    _prof_end(ev, 2.0 * m * n * k, 2 * m * k + 2 * n * k + 6 * m * n + 8 * m * (n // 64), tag)     # pair: 3 bytes read + 3 written per element; slot statistics


def gemm_nt_res_stats_wide_ok(m: int, n: int, k: int, lda: int, ldw: int, ldx: int, dtype) -> bool:
    """Shape contract of hgr_gemm_nt_res_stats_wide, asked of the library itself (hgr_gemm_nt_res_stats_wide_ok: whole 320 x 256
    tiles, at most one per compute unit, K % 128 == 0 and >= 256)."""
    code = dtype if isinstance(dtype, int) else DT_OF.get(dtype, -1)
    return bool(_lib.load().hgr_gemm_nt_res_stats_wide_ok(int(m), int(n), int(k), int(lda), int(ldw), int(ldx), int(code)))


# launches of hgr_gemm_nt_res_stats_wide made through ops.gemm_nt_res_stats_wide (tests tell the two producer routes apart by it)
WIDE_CALLS = [0]


def gemm_nt_res_stats_wide(a: torch.Tensor, w: torch.Tensor, xh: torch.Tensor, xl: torch.Tensor, bias: torch.Tensor, stats: torch.Tensor,
                           tag: str = "", flag: Optional[torch.Tensor] = None) -> None:
    """gemm_nt_res_stats on 320 x 256 tiles, one workgroup per compute unit in one round (hgr_gemm_nt_res_stats_wide): the same bits
    in xh, xl, stats and flag; shapes outside gemm_nt_res_stats_wide_ok are an error."""
    m, k = a.shape
    n = w.shape[0]
    assert a.dtype == w.dtype == xh.dtype and xl.dtype == PAIR_LO and xh.shape == xl.shape == (m, n) and xh.stride() == xl.stride()
    assert stats.dtype == torch.float32 and stats.numel() >= m * (n // 64) * 2 and a.stride(1) == w.stride(1) == xh.stride(1) == 1
    assert flag is None or (flag.numel() == 1 and flag.element_size() == 4)
    ev = _prof_begin()
    _lib.call("hgr_gemm_nt_res_stats_wide", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(xh), _dev(xl), xh.stride(0), _dev(bias),
              _dev(stats), LN_GUARD_SUMSQ if flag is not None else 0.0, _dev(flag), m, n, k, DT_OF[a.dtype], _stream())
    if not _lib.muted():
        WIDE_CALLS[0] += 1
    _prof_end(ev, 2.0 * m * n * k, 2 * m * k + 2 * n * k + 6 * m * n + 8 * m * (n // 64), tag)     # as gemm_nt_res_stats


def gemm_nt_bias_gelu_dual(a: torch.Tensor, w: torch.Tensor, pre: torch.Tensor, post: torch.Tensor, bias: torch.Tensor) -> None:
    """pre = a @ w^T + bias, post = QuickGELU(pre as rounded), both 16-bit, one launch (training forward of the MLP)."""
    assert a.dim() == 2 and w.dim() == 2 and a.dtype == w.dtype == pre.dtype == post.dtype and a.stride(1) == w.stride(1) == pre.stride(1) == post.stride(1) == 1
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and pre.shape == (m, n) and post.shape == (m, n) and bias.dtype == torch.float32 and bias.numel() == n
    _lib.call("hgr_gemm_nt_bias_gelu_dual", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(pre), pre.stride(0), _dev(post), post.stride(0),
              _dev(bias), m, n, k, DT_OF[a.dtype], _stream())


def gemm_nt_qgelu_grad_colsum(dy: torch.Tensor, wt: torch.Tensor, dx: torch.Tensor, pre: torch.Tensor, part: torch.Tensor) -> None:
    """dx (16-bit) = (dy @ wt^T) * g'(pre) - gemm_nt(..., epilogue=EPI_QGELU_GRAD16) bit for bit - and part[u, :] = column sums of dx
    as rounded over rows [64 u, 64 u + 64): the bias gradient of the layer below is colsum(part) (hgr_gemm_nt_qgelu_grad_colsum)."""
    assert dy.dim() == 2 and wt.dim() == 2 and dy.dtype == wt.dtype == dx.dtype == pre.dtype and dy.stride(1) == wt.stride(1) == dx.stride(1) == pre.stride(1) == 1
    m, k = dy.shape
    n = wt.shape[0]
    assert wt.shape[1] == k and dx.shape == (m, n) and pre.shape == (m, n)
    assert part.dtype == torch.float32 and part.is_contiguous() and part.shape == ((m + 63) // 64, n)
    _lib.call("hgr_gemm_nt_qgelu_grad_colsum", _dev(dy), dy.stride(0), _dev(wt), wt.stride(0), _dev(dx), dx.stride(0), _dev(pre), pre.stride(0),
              _dev(part), m, n, k, DT_OF[dy.dtype], _stream())


def gelu_dual_ok(m: int, n: int, k: int, lda: int, ldw: int) -> bool:
    """Shape contract of hgr_gemm_nt_bias_gelu_dual (the 256 x 128 tile kernel: whole column tiles, 32-bit operand offsets)."""
    return n % 128 == 0 and k % 64 == 0 and k >= 128 and m * lda * 2 < (1 << 32) and n * ldw * 2 < (1 << 32)


def gemm_nt_ln(x16: torch.Tensor, wfold: torch.Tensor, out: torch.Tensor, ln_s: torch.Tensor, ln_c: torch.Tensor, stats: torch.Tensor,
               eps: float = 1e-5, quickgelu: bool = False, tag: str = "") -> torch.Tensor:
    """out (16-bit) = act(LayerNorm(x) @ W^T + b) from the un-normalised 16-bit rows x16, the gamma-folded weight and the
    row statistics of the producer (hgr_gemm_nt_ln; see include/hgr.h)."""
    m, k = x16.shape
    n = wfold.shape[0]
    assert x16.dtype == wfold.dtype == out.dtype and out.shape[0] == m and out.shape[1] >= n and ln_s.numel() == n and ln_c.numel() == n
    assert x16.stride(1) == wfold.stride(1) == out.stride(1) == 1 and stats.dtype == torch.float32 and stats.numel() >= m * (k // 64) * 2
    ev = _prof_begin()
    _lib.call("hgr_gemm_nt_ln", _dev(x16), x16.stride(0), _dev(wfold), wfold.stride(0), _dev(out), out.stride(0), _dev(ln_s), _dev(ln_c),
              _dev(stats), float(eps), m, n, k, DT_OF[x16.dtype], 1 if quickgelu else 0, _stream())
    _prof_end(ev, 2.0 * m * n * k, 2 * m * k + 2 * n * k + 2 * m * n, tag)
    return out


def gemm_nt_ln_mha(x16: torch.Tensor, wfold: torch.Tensor, att: torch.Tensor, ln_s: torch.Tensor, ln_c: torch.Tensor, stats: torch.Tensor,
                   b: int, l: int, heads: int, causal: bool, eps: float = 1e-5, tag: str = "qkv_mha") -> torch.Tensor:
    """att [b*l, heads*64] = softmax(q k^T / 8 [+ causal]) v with [q | k | v] = LayerNorm(x) @ W_in^T + b_in, one launch, no qkv tensor
    (hgr_gemm_nt_ln_mha; see include/hgr.h).  Same bits as gemm_nt_ln into a qkv buffer + mha."""
    m, k = x16.shape
    w = heads * 64
    assert m == b * l and k == w and wfold.shape == (3 * w, k) and x16.dtype == wfold.dtype == att.dtype and att.shape == (m, w)
    assert x16.stride(1) == wfold.stride(1) == att.stride(1) == 1 and ln_s.numel() == ln_c.numel() == 3 * w
    assert stats.dtype == torch.float32 and stats.numel() >= m * (k // 64) * 2
    ev = _prof_begin()
    _lib.call("hgr_gemm_nt_ln_mha", _dev(x16), x16.stride(0), _dev(wfold), wfold.stride(0), _dev(ln_s), _dev(ln_c), _dev(stats), float(eps),
              _dev(att), att.stride(0), b, l, heads, 1 if causal else 0, DT_OF[x16.dtype], _stream())
    _prof_end(ev, 2.0 * m * 3 * w * k + 4.0 * b * heads * l * l * 64, 2 * m * k + 2 * 3 * w * k + 2 * m * w, tag)
    return att


def ln_mha_ok(w: int, l: int, rows: Optional[int] = None, ldx: Optional[int] = None) -> bool:
    """Shape contract of hgr_gemm_nt_ln_mha: whole sequences inside a 256-row tile, head width 64, row width a multiple of 128, and
    (the kernel's LDS-DMA addresses its operands with 32-bit byte offsets) operands below 4 GB.  Larger inputs are REJECTED further
    down as well: hgr_gemm_nt_ln has the same 32-bit offsets (ln_common_checks raises HgrError) - slice the batch (the towers' callers
    never get there: 4 GB of 16-bit rows is 2.8 M tokens of width 768)."""
    if not (1 <= l <= 64 and w % 128 == 0):
        return False
    if rows is not None and rows * (ldx if ldx is not None else w) * 2 >= (1 << 32):
        return False
    return 3 * w * w * 2 < (1 << 32)


def vit_embed_ln_stats(patches, cls, pos, gamma, beta, xh, xl, stats, b, g, eps=1e-5):
    _lib.call("hgr_vit_embed_ln_stats", _dev(patches), _dev(cls), _dev(pos), _dev(gamma), _dev(beta), _dev(xh), _dev(xl), _dev(stats),
              b, g, xh.shape[1], eps, DT_OF[xh.dtype], _stream())


def vit_patch_embed_ln_ok(b: int, r: int, patch: int, w: int, dtype) -> bool:
    """Shape contract of hgr_vit_patch_embed_ln, asked of the library itself (hgr_vit_patch_embed_ln_ok: patch 32, at most 56 patches
    per image, width 768, f16 / bf16).  Everything else keeps im2col_patches -> gemm_nt -> vit_embed_ln_stats."""
    code = DT_OF.get(dtype, dtype if isinstance(dtype, int) else -1)
    return bool(_lib.load().hgr_vit_patch_embed_ln_ok(int(b), int(r), int(patch), int(w), int(code)))


def vit_patch_embed_ln(image: torch.Tensor, conv_w: torch.Tensor, cls, pos, gamma, beta, xh, xl, stats, patch: int, eps=1e-5) -> None:
    """fp32 NCHW pixels -> the pair (xh, xl) + slot statistics of ln_pre(tokens), one launch (hgr_vit_patch_embed_ln): the bits of
    im2col_patches -> gemm_nt (fp32 out) -> vit_embed_ln_stats.  Recorded for PROFILE as the patch GEMM with the bytes it really moves."""
    assert image.dtype == torch.float32 and image.dim() == 4 and image.shape[1] == 3 and image.shape[2] == image.shape[3] and image.is_contiguous()
    b, r = image.shape[0], image.shape[2]
    w, k = conv_w.shape
    gg = (r // patch) ** 2
    assert conv_w.is_contiguous() and k == 3 * patch * patch and conv_w.dtype == xh.dtype and xl.dtype == PAIR_LO
    assert xh.is_contiguous() and xl.is_contiguous() and xh.shape == xl.shape == (b * (gg + 1), w)
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= b * (gg + 1) * (w // 64) * 2
    ev = _prof_begin()
    _lib.call("hgr_vit_patch_embed_ln", _dev(image), _dev(conv_w), _dev(cls), _dev(pos), _dev(gamma), _dev(beta), _dev(xh), _dev(xl), _dev(stats),
              b, r, patch, w, eps, DT_OF[xh.dtype], _stream())
    rows = b * (gg + 1)
    _prof_end(ev, 2.0 * b * gg * w * k, 4 * b * 3 * r * r + 2 * w * k + 3 * rows * w + 8 * rows * (w // 64), "patch")


def row_stats16(x: torch.Tensor, xh: torch.Tensor, xl: torch.Tensor, stats: torch.Tensor) -> None:
    assert x.dtype == torch.float32 and x.is_contiguous() and xh.is_contiguous() and xl.is_contiguous() and xh.shape == xl.shape == x.shape
    assert xl.dtype == PAIR_LO and stats.numel() >= x.shape[0] * (x.shape[1] // 64) * 2
    _lib.call("hgr_row_stats16", _dev(x), _dev(xh), _dev(xl), _dev(stats), x.shape[0], x.shape[1], DT_OF[xh.dtype], _stream())


def pair_rows_f32(xh: torch.Tensor, xl: torch.Tensor, out: torch.Tensor, row_mul: int = 1, row_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = xh[src] + xl[src] (fp32), src = i * row_mul + row_idx[i]: selected rows of the 16-bit pair back in fp32."""
    assert xh.is_contiguous() and xl.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.shape[1] == xh.shape[1] and xl.dtype == PAIR_LO
    _lib.call("hgr_pair_rows_f32", _dev(xh), _dev(xl), _dev(out), out.shape[0], out.shape[1], row_mul, _dev(row_idx), DT_OF[xh.dtype], _stream())
    return out


def vit_head(xh: torch.Tensor, xl: torch.Tensor, row_mul: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, proj_t: torch.Tensor,
             out: torch.Tensor) -> torch.Tensor:
    """out[b] = LayerNorm(xh[b * row_mul] + xl[b * row_mul]) (16-bit) @ proj_t^T, fp32 [B, D] (hgr_vit_head: ln_post + visual.proj)."""
    assert xh.dtype == proj_t.dtype and xl.dtype == PAIR_LO and xh.stride() == xl.stride() and xh.stride(1) == 1
    assert out.dtype == torch.float32 and out.is_contiguous() and proj_t.is_contiguous() and proj_t.shape[1] == xh.shape[1] and out.shape[1] == proj_t.shape[0]
    ev = _prof_begin()
    _lib.call("hgr_vit_head", _dev(xh), _dev(xl), xh.stride(0), int(row_mul), _dev(gamma), _dev(beta), float(eps), _dev(proj_t), _dev(out),
              out.shape[0], xh.shape[1], out.shape[1], DT_OF[xh.dtype], _stream())
    _prof_end(ev, 2.0 * out.shape[0] * out.shape[1] * xh.shape[1], 0, "head")
    return out


def gemm_set_tile(tile: int) -> int:
    """Pin hgr_gemm_nt's tile plan (0 = cost model, 128, 256); returns the previous setting."""
    lib = _lib.load()
    prev = lib.hgr_gemm_set_tile(int(tile))
    if prev < 0:
        raise _lib.HgrError(f"hgr_gemm_set_tile failed ({prev}): {lib.hgr_last_error().decode()}")
    return prev


def gemm_set_tail(enabled: bool, full_panels: int = -1) -> int:
    """Tail plan of the 256 x 128 tile kernel on / off (hgr_gemm_set_tail); returns the previous setting."""
    lib = _lib.load()
    prev = lib.hgr_gemm_set_tail(1 if enabled else 0, int(full_panels))
    if prev < 0:
        raise _lib.HgrError(f"hgr_gemm_set_tail failed ({prev}): {lib.hgr_last_error().decode()}")
    return prev


def gemm_set_persist(enabled: bool) -> int:
    """Persistent form of the residual-producer GEMMs on / off (hgr_gemm_set_persist); returns the previous setting."""
    lib = _lib.load()
    prev = lib.hgr_gemm_set_persist(1 if enabled else 0)
    if prev < 0:
        raise _lib.HgrError(f"hgr_gemm_set_persist failed ({prev}): {lib.hgr_last_error().decode()}")
    return prev


def gemm_plan(fn) -> list:
    """The launches ONE call of an NT-family entry point inside fn() would make (hgr_gemm_plan_capture): the call validates and plans,
    launches nothing; one dict per launch, keyed like hgr_gemm_launch of include/hgr.h."""
    lib = _lib.load()
    out = (_lib.GemmLaunch * 4)()
    rc = lib.hgr_gemm_plan_capture(out, len(out))
    if rc:
        raise _lib.HgrError(f"hgr_gemm_plan_capture failed ({rc}): {lib.hgr_last_error().decode()}")
    try:
        fn()
    finally:                                     # a covered call has disarmed the thread; anything else must not leave it armed
        unused = lib.hgr_gemm_plan_capture(None, 0)
    if unused:
        raise _lib.HgrError("gemm_plan: fn() made no call that hgr_gemm_plan_capture covers")
    return [{name: getattr(rec, name) for name, _ in rec._fields_} for rec in out if rec.kernel]


def im2col_patches(image: torch.Tensor, out: torch.Tensor, patch: int) -> torch.Tensor:
    b, c, r, r2 = image.shape
    assert c == 3 and r == r2 and image.dtype == torch.float32 and image.is_contiguous() and out.is_contiguous()
    _lib.call("hgr_im2col_patches", _dev(image), _dev(out), b, r, patch, out.shape[1], DT_OF[out.dtype], _stream())
    return out


def im2col_patches_tokens(image: torch.Tensor, out: torch.Tensor, patch: int, l: int) -> torch.Tensor:
    """Patches written straight into the [B, L] token layout (row b*L + 1 + p); class rows stay as they are."""
    b, c, r, _ = image.shape
    assert image.dtype == torch.float32 and image.is_contiguous() and out.is_contiguous() and out.shape[0] == b * l
    _lib.call("hgr_im2col_patches_ex", _dev(image), _dev(out), b, r, patch, out.shape[1], l, 1, DT_OF[out.dtype], _stream())
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # clip/clip.py:77
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def im2col_patches_u8(image: torch.Tensor, out: torch.Tensor, patch: int, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """uint8 NHWC [B, R, R, 3] -> normalised 16-bit patch rows in (py, px, c) order."""
    import ctypes
    b, r, r2, c = image.shape
    assert image.dtype == torch.uint8 and c == 3 and r == r2 and image.is_contiguous() and out.is_contiguous()
    g = r // patch
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _lib.call("hgr_im2col_patches_u8", _dev(image), _dev(out), b, r, patch, out.shape[1], g * g, 0, m3, s3, DT_OF[out.dtype], _stream())
    return out


def preprocess_bicubic(src: torch.Tensor, off: torch.Tensor, hw: torch.Tensor, tab: Optional[torch.Tensor], xb: torch.Tensor, xk: torch.Tensor, kx: int,
                       yb: torch.Tensor, yk: torch.Tensor, ky: int, out_u8: Optional[torch.Tensor], out_f32: Optional[torch.Tensor],
                       mean=CLIP_MEAN, std=CLIP_STD, b: int = 0, r: int = 0) -> None:
    """Resize + center crop (+ normalise) of packed uint8 RGB images; tables from hgr_net_amd.preprocess."""
    import ctypes
    assert src.dtype == torch.uint8 and off.dtype == torch.int64 and all(t.dtype == torch.int32 for t in (hw, xb, xk, yb, yk))
    t = xb.numel() // (2 * r)                                  # number of table sets
    assert off.numel() == b and hw.numel() == 2 * b and xb.numel() == 2 * t * r and xk.numel() == t * r * kx and yk.numel() == t * r * ky
    assert (tab is None and t == b) or (tab is not None and tab.dtype == torch.int32 and tab.numel() == b)
    assert out_u8 is None or (out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and out_u8.numel() == b * r * r * 3)
    assert out_f32 is None or (out_f32.dtype == torch.float32 and out_f32.is_contiguous() and out_f32.numel() == b * r * r * 3)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    _lib.call("hgr_preprocess_bicubic", _dev(src), _dev(off), _dev(hw), _dev(tab), _dev(xb), _dev(xk), kx, _dev(yb), _dev(yk), ky,
              _dev(out_u8), _dev(out_f32), m3, s3, b, r, _stream())


def vit_assemble(t: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, b: int, l: int) -> torch.Tensor:
    _lib.call("hgr_vit_assemble", _dev(t), _dev(cls), _dev(pos), b, l, t.shape[1], _stream())
    return t


def vit_embed_ln(patches, cls, pos, gamma, beta, x, b, g, eps=1e-5):
    _lib.call("hgr_vit_embed_ln", _dev(patches), _dev(cls), _dev(pos), _dev(gamma), _dev(beta), _dev(x), b, g, x.shape[1], eps, _stream())
    return x


def layernorm(x: torch.Tensor, gamma, beta, out: torch.Tensor, rows: Optional[int] = None, row_mul: int = 1,
              row_idx: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    w = x.shape[-1]
    rows = out.shape[0] if rows is None else rows
    out32 = out.dtype == torch.float32
    _lib.call("hgr_layernorm", _dev(x), _dev(gamma), _dev(beta), _dev(out), rows, w, row_mul, _dev(row_idx), eps,
              HGR_BF16 if out32 else DT_OF[out.dtype], 1 if out32 else 0, _stream())
    return out


def mha(qkv: torch.Tensor, out: torch.Tensor, b: int, l: int, heads: int, causal: bool, stats: Optional[torch.Tensor] = None,
        q_rows: int = 0) -> torch.Tensor:
    """``stats`` fp32 [b, heads, l, 2]: also keep every row's softmax statistics (max, 1 / sum) for mha_bwd (training forward).
    ``q_rows`` > 0: only the first q_rows query rows of every sequence are computed and written (hgr_mha_rows)."""
    assert qkv.is_contiguous() and out.is_contiguous() and qkv.shape[1] == 3 * heads * 64 and out.shape[1] == heads * 64
    if q_rows:
        assert stats is None
        _lib.call("hgr_mha_rows", _dev(qkv), _dev(out), b, l, heads, 1 if causal else 0, int(q_rows), DT_OF[qkv.dtype], _stream())
        return out
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == b * heads * l * 2
        _lib.call("hgr_mha_stats", _dev(qkv), _dev(out), _dev(stats), b, l, heads, 1 if causal else 0, DT_OF[qkv.dtype], _stream())
        return out
    _lib.call("hgr_mha", _dev(qkv), _dev(out), b, l, heads, 1 if causal else 0, DT_OF[qkv.dtype], _stream())
    return out


def text_embed(tokens: torch.Tensor, emb: torch.Tensor, pos: torch.Tensor, x: torch.Tensor, l: int) -> torch.Tensor:
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1
    n = tokens.shape[0]
    _lib.call("hgr_text_embed", _dev(tokens), tokens.stride(0), _dev(emb), _dev(pos), _dev(x), n, l, emb.shape[1], emb.shape[0], _stream())
    return x


def eot_index(tokens: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    assert tokens.dtype == torch.int64 and out.dtype == torch.int32
    _lib.call("hgr_eot_index", _dev(tokens), tokens.stride(0), _dev(out), tokens.shape[0], tokens.shape[1], _stream())
    return out


def l2norm_rows(x: torch.Tensor, y16: Optional[torch.Tensor] = None, y32: Optional[torch.Tensor] = None) -> None:
    assert x.dtype == torch.float32 and x.is_contiguous()
    dt = DT_OF[y16.dtype] if y16 is not None else HGR_BF16
    _lib.call("hgr_l2norm_rows", _dev(x), _dev(y16), _dev(y32), x.shape[0], x.shape[1], dt, _stream())


def topk_rows(logits: torch.Tensor, k: int, cols: Optional[torch.Tensor] = None, n_cols: Optional[int] = None,
              want_values: bool = False):
    """int32 [rows, k] node ids of the k largest logits over `cols` (int32) or the first n_cols columns."""
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    rows = logits.shape[0]
    nc = cols.numel() if cols is not None else (logits.shape[1] if n_cols is None else n_cols)
    idx = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    val = torch.empty((rows, k), dtype=torch.float32, device=logits.device) if want_values else None
    _lib.call("hgr_topk_rows", _dev(logits), logits.stride(0), _dev(cols), nc, k, _dev(idx), _dev(val), rows, _stream())
    return (idx, val) if want_values else idx


def level_argmax(logits: torch.Tensor, depth: torch.Tensor, n_levels: int, cols: Optional[torch.Tensor] = None,
                 n_cols: Optional[int] = None, want_top1: bool = False):
    """int32 [rows, n_levels]: per depth level the arg-max node id over `cols` (main.py:162-176);
    with want_top1 also int32 [rows, 1]: the unmasked top-1 over `cols` (main.py:157)."""
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and depth.dtype == torch.int32
    rows = logits.shape[0]
    nc = cols.numel() if cols is not None else (logits.shape[1] if n_cols is None else n_cols)
    out = torch.empty((rows, n_levels), dtype=torch.int32, device=logits.device)
    top1 = torch.empty((rows, 1), dtype=torch.int32, device=logits.device) if want_top1 else None
    _lib.call("hgr_level_argmax", _dev(logits), logits.stride(0), _dev(cols), nc, _dev(depth), n_levels, _dev(out), _dev(top1), rows, _stream())
    return (out, top1) if want_top1 else out


class EvalIndex:
    """Dense per-column maps for the fused evaluation kernel (built once per model on the host): depth of every node,
    column -> position in the train / test subsets (-1 = absent), position -> node id, and the reference's -1-filler
    position per level."""

    def __init__(self, depth: torch.Tensor, train_cols: torch.Tensor, test_cols: Optional[torch.Tensor], n_levels: int):
        import numpy as np
        d = depth.cpu().numpy()
        n = len(d)
        tr = train_cols.cpu().numpy().astype(np.int64)
        assert d.min() >= 0 and n_levels <= 32 and d[tr].max() < n_levels, "a subset node lies deeper than n_levels"
        assert len(set(tr.tolist())) == len(tr), "train columns must be distinct"
        lv = d[tr]
        filler = np.full(n_levels, -1, dtype=np.int32)
        for l in range(n_levels):
            other = np.nonzero(lv != l)[0]
            if other.size:
                filler[l] = int(other[0])
        tpos = np.full(n, -1, dtype=np.int32)
        tpos[tr] = np.arange(len(tr), dtype=np.int32)
        dev = depth.device
        self.n_nodes, self.n_levels, self.n_train = n, n_levels, len(tr)
        self.lvl8 = torch.from_numpy(np.minimum(d, 255).astype(np.uint8)).to(dev)
        self.train_pos = torch.from_numpy(tpos).to(dev)
        self.train_cols = train_cols.to(torch.int32).contiguous()
        self.filler = torch.from_numpy(filler).to(dev)
        self.test_pos = self.test_cols = None
        self.n_test = 0
        if test_cols is not None:
            te = test_cols.cpu().numpy().astype(np.int64)
            assert len(set(te.tolist())) == len(te), "test columns must be distinct"
            epos = np.full(n, -1, dtype=np.int32)
            epos[te] = np.arange(len(te), dtype=np.int32)
            self.test_pos = torch.from_numpy(epos).to(dev)
            self.test_cols = test_cols.to(torch.int32).contiguous()
            self.n_test = len(te)


def eval_rows(logits: torch.Tensor, index: EvalIndex, k: int):
    """(level arg-max [rows, n_levels], top-1 [rows, 1], top-k [rows, k]) int32 node ids from one fused kernel."""
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[1] >= index.n_nodes
    rows = logits.shape[0]
    dev = logits.device
    lvl = torch.empty((rows, index.n_levels), dtype=torch.int32, device=dev)
    top1 = torch.empty((rows, 1), dtype=torch.int32, device=dev)
    topk = torch.empty((rows, max(k, 1)), dtype=torch.int32, device=dev)
    _lib.call("hgr_eval_rows", _dev(logits), logits.stride(0), index.n_nodes, _dev(index.lvl8), _dev(index.train_pos), _dev(index.train_cols),
              index.n_train, index.n_levels, _dev(index.filler), _dev(index.test_pos), _dev(index.test_cols), index.n_test, k,
              _dev(lvl), _dev(top1), _dev(topk), rows, _stream())
    return lvl, top1, topk


class LogitsEvalPlan:
    """Level-sorted view of the class matrix for hgr_logits_eval (include/hgr.h): the column permutation (levels contiguous, each
    padded to a multiple of 32 columns, total to a multiple of 96 = one CU's slab), the per-column train / test positions in permuted
    order and the first 32-column slice of every level.  Built once per model from an EvalIndex; `bind(zsl16)` gathers the permuted
    16-bit class matrix (once per tensor object handed in, i.e. once per update_classifier)."""
    SLICE, SLAB = 32, 96

    def __init__(self, index: EvalIndex):
        import numpy as np
        lvl = index.lvl8.cpu().numpy().astype(np.int64)
        tpos = index.train_pos.cpu().numpy()
        epos = index.test_pos.cpu().numpy() if index.test_pos is not None else np.full(len(lvl), -1, dtype=np.int32)
        cols, level_first = [], [0]
        for l in range(index.n_levels):
            c = np.nonzero(lvl == l)[0]
            pad = (-c.size) % self.SLICE
            cols.append(np.concatenate([c, np.full(pad, -1, dtype=np.int64)]))
            level_first.append(level_first[-1] + (c.size + pad) // self.SLICE)
        assert int((lvl >= index.n_levels).sum()) == 0, "a node lies deeper than n_levels"
        perm = np.concatenate(cols)
        tail = (-perm.size) % self.SLAB                              # whole 96-column slabs; the slices behind the last level belong to no level
        if tail or perm.size == 0:
            perm = np.concatenate([perm, np.full(tail or self.SLAB, -1, dtype=np.int64)])
        dev = index.lvl8.device
        valid = perm >= 0
        safe = np.where(valid, perm, 0)
        self.index = index
        self.n_perm = int(perm.size)
        self.perm = torch.from_numpy(safe).to(dev)
        self.valid = torch.from_numpy(valid).to(dev)
        self.tpos = torch.from_numpy(np.where(valid, tpos[safe], -1).astype(np.int32)).to(dev)
        self.epos = torch.from_numpy(np.where(valid, epos[safe], -1).astype(np.int32)).to(dev)
        self.level_first = torch.from_numpy(np.asarray(level_first, dtype=np.int32)).to(dev)
        self.zsl = None
        self._src = None
        self._ws = None

    MAX_SLICES = 1024            # hgr_logits_eval: 32-column slices per row (csrc/hgr_gemm.hip) = 32 768 permuted columns

    @property
    def supported(self) -> bool:
        """Whether hgr_logits_eval covers this hierarchy (padding every level to 32 columns brings hierarchies somewhat below
        32 768 nodes over its capacity): callers fall back to forward() + hgr_eval_rows otherwise."""
        return self.n_perm // self.SLICE <= self.MAX_SLICES and self.index.n_levels <= 32

    def bind(self, zsl16: torch.Tensor, algo_d: Optional[int] = None) -> "LogitsEvalPlan":
        """``algo_d``: the embedding width the product stands for when zsl16 is a K-concatenated operand (clip_tree.LOGITS_SPLIT) -
        profiling reports the ALGORITHMIC flops 2 B N D, not the doubled K."""
        self.algo_d = int(algo_d or zsl16.shape[1])
        if self._src is not zsl16:                   # the tensor OBJECT it was given (held): a new classifier is a new tensor
            z = zsl16[self.perm]
            z[~self.valid] = 0
            self.zsl, self._src = z.contiguous(), zsl16
        return self

    def workspace(self, rows: int, dev) -> torch.Tensor:
        need = int(_lib.load().hgr_logits_eval_workspace_bytes(rows, self.n_perm))
        if self._ws is None or self._ws.numel() < need or self._ws.device != torch.device(dev):
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws


def logits_eval(feat16: torch.Tensor, plan: LogitsEvalPlan, k: int, stage: str = ""):
    """(level arg-max [rows, n_levels], top-1 [rows, 1], top-k [rows, k]) int32 node ids straight from the L2-normalised 16-bit
    image features: the logits GEMM with the evaluation in its epilogue (hgr_logits_eval) - no [rows, N] logits in memory.
    ``stage`` = "tile" / "row": that stage alone (measurement; the row stage reads the workspace the last tile stage wrote)."""
    ix = plan.index
    assert plan.zsl is not None, "LogitsEvalPlan.bind(zsl16) first"
    assert feat16.is_contiguous() and feat16.dtype == plan.zsl.dtype and feat16.shape[1] == plan.zsl.shape[1]
    rows, d = feat16.shape
    dev = feat16.device
    lvl = torch.empty((rows, ix.n_levels), dtype=torch.int32, device=dev)
    top1 = torch.empty((rows, 1), dtype=torch.int32, device=dev)
    topk = torch.empty((rows, max(k, 1)), dtype=torch.int32, device=dev)
    prof = PROFILE
    ev = _prof_begin()
    _lib.call({"": "hgr_logits_eval", "tile": "hgr_logits_eval_tile_stage", "row": "hgr_logits_eval_row_stage"}[stage],
              _dev(feat16), _dev(plan.zsl), rows, d, plan.n_perm, _dev(plan.tpos), _dev(plan.epos), _dev(plan.level_first),
              ix.n_levels, _dev(ix.filler), _dev(ix.train_cols), ix.n_train, _dev(ix.test_cols), ix.n_test, k,
              _dev(lvl), _dev(top1), _dev(topk), _dev(plan.workspace(rows, dev)), DT_OF[feat16.dtype], _stream())
    da = getattr(plan, "algo_d", d)
    _prof_end(ev, 2.0 * rows * ix.n_nodes * da, 2 * rows * da + 2 * ix.n_nodes * da, "logits_eval" + ("_" + stage if stage else ""))
    return lvl, top1, topk


def eval_counters(pred: torch.Tensor, targets: Optional[torch.Tensor], target: int, top1: torch.Tensor, lv: torch.Tensor,
                  parents: torch.Tensor, levels: torch.Tensor, acc: torch.Tensor) -> None:
    """Advance the nine float64 evaluation counters with one batch (main.py:139-191) from eval_rows' outputs."""
    assert pred.dtype == top1.dtype == lv.dtype == parents.dtype == levels.dtype == torch.int32 and acc.dtype == torch.float64
    assert pred.is_contiguous() and lv.is_contiguous() and top1.is_contiguous() and acc.numel() == 9
    assert targets is None or (targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == pred.shape[0])
    _lib.call("hgr_eval_counters", _dev(pred), pred.shape[1], _dev(targets), int(target), _dev(top1), _dev(lv), lv.shape[1], _dev(parents),
              _dev(levels), parents.numel(), _dev(acc), pred.shape[0], _stream())


def eval_counters_rows(pred: torch.Tensor, targets: torch.Tensor, top1: torch.Tensor, lv: torch.Tensor, anc_ptr: torch.Tensor,
                       anc_nodes: torch.Tensor, anc_levels: torch.Tensor, acc: torch.Tensor) -> None:
    """Advance the nine float64 evaluation counters with one batch of MIXED classes (main.py:139-191): every row is scored against
    the path of its own target (CSR anc_ptr [n_nodes + 1] / anc_nodes / anc_levels); rows with a target outside [0, n_nodes) are
    padding and count nothing.  The result does not depend on the order of the rows."""
    assert pred.dtype == top1.dtype == lv.dtype == anc_ptr.dtype == anc_nodes.dtype == anc_levels.dtype == torch.int32 and acc.dtype == torch.float64
    assert pred.is_contiguous() and lv.is_contiguous() and top1.is_contiguous() and acc.numel() == 9
    assert anc_ptr.is_contiguous() and anc_nodes.is_contiguous() and anc_levels.is_contiguous() and anc_ptr.numel() >= 2
    assert targets is not None and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == pred.shape[0]
    assert top1.numel() == pred.shape[0] and lv.shape[0] == pred.shape[0]
    _lib.call("hgr_eval_counters_rows", _dev(pred), pred.shape[1], _dev(targets), _dev(top1), _dev(lv), lv.shape[1], _dev(anc_ptr),
              _dev(anc_nodes), _dev(anc_levels), anc_ptr.numel() - 1, _dev(acc), pred.shape[0], _stream())


# layout of the hierarchy report's table: mirrors HGR_REPORT_* of include/hgr.h (offsets in int64 entries)
REPORT_MAXL = 32
REPORT_DEPTH_COLS = ("rows", "hit@1", "hit@2", "hit@5", "hit@10", "hit@20", "anc_hit", "point", "edge", "chain")
REPORT_DEPTH = 0                                                   # [33][10] by the target's path length L
REPORT_LEVEL = REPORT_DEPTH + (REPORT_MAXL + 1) * len(REPORT_DEPTH_COLS)      # [32][2] by path position: rows, matches
REPORT_DIST_BINS = 2 * REPORT_MAXL + 2                             # distances 0..64 and "unknown"
REPORT_DIST_UNKNOWN = 2 * REPORT_MAXL + 1
REPORT_DIST_TEST = REPORT_LEVEL + 2 * REPORT_MAXL                  # [66] dist(pred[r, 0], target)
REPORT_DIST_ALL = REPORT_DIST_TEST + REPORT_DIST_BINS              # [66] dist(top1[r], target)
REPORT_HEIGHT = REPORT_DIST_ALL + REPORT_DIST_BINS                 # [5] summed heights of the first K predictions, K in REPORT_HEIGHT_K
REPORT_HEIGHT_K = (1, 2, 5, 10, 20)
REPORT_LEN = REPORT_HEIGHT + len(REPORT_HEIGHT_K)                  # 531


def eval_report_rows(pred: torch.Tensor, targets: torch.Tensor, top1: torch.Tensor, lv: torch.Tensor, anc_ptr: torch.Tensor,
                     anc_nodes: torch.Tensor, anc_levels: torch.Tensor, table: torch.Tensor) -> None:
    """Add one batch to the hierarchy report's int64 table (layout above; definitions in include/hgr.h): the operands of
    eval_counters_rows, the same padding rule, exact integer counts only - the table does not depend on the order of the rows or on
    how they were cut into calls."""
    assert pred.dtype == top1.dtype == lv.dtype == anc_ptr.dtype == anc_nodes.dtype == anc_levels.dtype == torch.int32
    assert table.dtype == torch.int64 and table.numel() == REPORT_LEN and table.is_contiguous()
    assert pred.is_contiguous() and lv.is_contiguous() and top1.is_contiguous()
    assert anc_ptr.is_contiguous() and anc_nodes.is_contiguous() and anc_levels.is_contiguous() and anc_ptr.numel() >= 2
    assert targets is not None and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == pred.shape[0]
    assert top1.numel() == pred.shape[0] and lv.shape[0] == pred.shape[0]
    _lib.call("hgr_eval_report_rows", _dev(pred), pred.shape[1], _dev(targets), _dev(top1), _dev(lv), lv.shape[1], _dev(anc_ptr),
              _dev(anc_nodes), _dev(anc_levels), anc_ptr.numel() - 1, _dev(table), pred.shape[0], _stream())


PATH_MAXL = 32                      # HGR_PATH_MAXL of include/hgr.h (= REPORT_MAXL): the longest path a weight table has a row for


def path_scores(logits: torch.Tensor, anc_ptr: torch.Tensor, anc_nodes: torch.Tensor, wtab: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Path scores [rows, n_nodes] fp32 (hgr_path_scores, definition in include/hgr.h): every node scored by the weighted logits along
    its root-to-node path, P(n) = anc_nodes[anc_ptr[n]:anc_ptr[n + 1]], with row L of ``wtab`` [33, 32] as the weights of a path of L
    nodes; a node without a path of 1..32 nodes keeps its logit.  ``logits`` and ``out`` may be views of wider buffers (unit column
    stride, at least n_nodes columns; further columns of ``out`` are left alone) and must not overlap.  Returns out[:, :n_nodes]."""
    n_nodes = anc_ptr.numel() - 1
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[1] >= n_nodes >= 1
    assert anc_ptr.dtype == anc_nodes.dtype == torch.int32 and anc_ptr.is_contiguous() and anc_nodes.is_contiguous()
    assert wtab.dtype == torch.float32 and wtab.shape == (PATH_MAXL + 1, PATH_MAXL) and wtab.is_contiguous()
    rows = logits.shape[0]
    if out is None:
        out = torch.empty((rows, n_nodes), dtype=torch.float32, device=logits.device)
    assert out.dim() == 2 and out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] == rows and out.shape[1] >= n_nodes
    # the strides go to the library as they are: it rejects rows = 0, a leading dimension below n_nodes and overlapping operands
    _lib.call("hgr_path_scores", _dev(logits), logits.stride(0), _dev(out), out.stride(0), n_nodes, _dev(anc_ptr), _dev(anc_nodes),
              _dev(wtab), rows, _stream())
    return out[:, :n_nodes]


# hedged predictions: mirrors HGR_HEDGE_* of include/hgr.h (columns of one row of the outcome table, in int64 entries)
HEDGE_MAXT = 8
HEDGE_MAXN = 36864
HEDGE_SCALE = 1 << 30                                              # masses and thresholds are multiples of 2^-30
HEDGE_COL_NAMES = ("rows", "abstain", "exact", "ancestor", "below", "wrong", "sum_lpick", "sum_common", "sum_lt")
HEDGE_COL_HIST = len(HEDGE_COL_NAMES)                              # [33] picks by path length, 0 = abstained or without a path
HEDGE_COLS = HEDGE_COL_HIST + REPORT_MAXL + 1                      # 42


def hedge_thresholds(thetas) -> list:
    """thr[i] = ceil(theta_i * 2^30), in double on the host: the fixed-point thresholds of hgr_subtree_hedge.  1 .. HEDGE_MAXT values
    in (0, 1], strictly increasing; anything else is a ValueError."""
    try:
        th = [float(t) for t in thetas]
    except TypeError:
        raise ValueError(f"hedge thresholds {thetas!r}: a sequence of numbers") from None
    if not 1 <= len(th) <= HEDGE_MAXT:
        raise ValueError(f"hedge: {len(th)} thresholds (1..{HEDGE_MAXT})")
    if not all(0.0 < t <= 1.0 for t in th):                        # a NaN fails both comparisons
        raise ValueError(f"hedge thresholds {th}: each in (0, 1]")
    if any(b <= a for a, b in zip(th, th[1:])):
        raise ValueError(f"hedge thresholds {th}: strictly increasing")
    return [int(math.ceil(t * HEDGE_SCALE)) for t in th]


def subtree_hedge(scores: torch.Tensor, cand_pos: Optional[torch.Tensor], anc_ptr: torch.Tensor, anc_nodes: torch.Tensor,
                  temperature: float, thr: torch.Tensor, pick: Optional[torch.Tensor] = None, pick_mass: Optional[torch.Tensor] = None,
                  mass_out: Optional[torch.Tensor] = None):
    """(pick int32 [rows, T], pick_mass fp32 [rows, T]) of hgr_subtree_hedge (definition in include/hgr.h): per threshold the deepest
    node whose subtree holds at least that much of the row's softmax(temperature * scores) over the candidates (cand_pos[n] >= 0; None:
    every node), -1 where no node does.  ``thr``: int32 [T] on the device, hedge_thresholds' values.  ``mass_out``: int32 [rows, >=
    n_nodes] (unit column stride) that receives every node's mass in units of 2^-30 (below 2^31: int32 holds the uint32 as it is);
    further columns are left alone.  ``scores`` may be a view of a wider buffer."""
    n_nodes = anc_ptr.numel() - 1
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.stride(1) == 1
    assert anc_ptr.dtype == anc_nodes.dtype == torch.int32 and anc_ptr.is_contiguous() and anc_nodes.is_contiguous()
    assert cand_pos is None or (cand_pos.dtype == torch.int32 and cand_pos.is_contiguous() and cand_pos.numel() == n_nodes)
    assert thr.dtype == torch.int32 and thr.dim() == 1 and thr.is_contiguous()
    rows, t = scores.shape[0], thr.numel()
    if pick is None:
        pick = torch.empty((rows, t), dtype=torch.int32, device=scores.device)
    if pick_mass is None:
        pick_mass = torch.empty((rows, t), dtype=torch.float32, device=scores.device)
    assert pick.dtype == torch.int32 and pick.shape == (rows, t) and pick.is_contiguous()
    assert pick_mass.dtype == torch.float32 and pick_mass.shape == (rows, t) and pick_mass.is_contiguous()
    assert mass_out is None or (mass_out.dim() == 2 and mass_out.dtype == torch.int32 and mass_out.stride(1) == 1 and mass_out.shape[0] == rows)
    # sizes and the temperature go to the library as they are: it rejects what hgr.h lists, before anything is launched
    _lib.call("hgr_subtree_hedge", _dev(scores), scores.stride(0), n_nodes, _dev(cand_pos), _dev(anc_ptr), _dev(anc_nodes), float(temperature),
              _dev(thr), t, _dev(pick), _dev(pick_mass), _dev(mass_out), mass_out.stride(0) if mass_out is not None else 0, rows, _stream())
    return pick, pick_mass


def hedge_counters_rows(pick: torch.Tensor, targets: torch.Tensor, anc_ptr: torch.Tensor, anc_nodes: torch.Tensor, table: torch.Tensor) -> None:
    """Add one batch of picks to the hedge outcome table, int64 [T, HEDGE_COLS] (hgr_hedge_counters_rows, include/hgr.h): the padding
    rule of eval_counters_rows, exact integer counts only."""
    assert pick.dtype == anc_ptr.dtype == anc_nodes.dtype == torch.int32 and pick.dim() == 2 and pick.is_contiguous()
    assert anc_ptr.is_contiguous() and anc_nodes.is_contiguous() and anc_ptr.numel() >= 2
    assert table.dtype == torch.int64 and table.shape == (pick.shape[1], HEDGE_COLS) and table.is_contiguous()
    assert targets is not None and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == pick.shape[0]
    _lib.call("hgr_hedge_counters_rows", _dev(pick), pick.shape[1], _dev(targets), _dev(anc_ptr), _dev(anc_nodes), anc_ptr.numel() - 1,
              _dev(table), pick.shape[0], _stream())


# candidate sets: mirrors HGR_SETS_* of include/hgr.h (one set's table is [REPORT_MAXL + 1][SETS_COLS], by the target's path length)
SETS_MAXS = 16
SETS_COL_NAMES = ("rows", "hit@1", "hit@2", "hit@5", "hit@10", "hit@20", "anc_hit", "point", "edge")
SETS_COLS = len(SETS_COL_NAMES)                                    # 9


def check_sets(sets, n_nodes: int) -> dict:
    """``sets`` as an ordered dict name -> list of node ids, or ValueError: no mapping, no set or more than SETS_MAXS, an id twice in
    one set, an id outside [0, n_nodes).  Host only."""
    try:
        items = [(str(k), [int(c) for c in (v.tolist() if hasattr(v, "tolist") else v)]) for k, v in dict(sets).items()]
    except (TypeError, ValueError):
        raise ValueError(f"sets {sets!r}: a mapping from a name to node ids") from None
    if not 1 <= len(items) <= SETS_MAXS:
        raise ValueError(f"sets: {len(items)} candidate sets (1..{SETS_MAXS})")
    for name, ids in items:
        if len(set(ids)) != len(ids):
            raise ValueError(f"sets[{name!r}]: a node id appears twice")
        bad = [c for c in ids if not 0 <= c < n_nodes]
        if bad:
            raise ValueError(f"sets[{name!r}]: node id {bad[0]} outside the hierarchy (0..{n_nodes - 1})")
    return dict(items)


class SetIndex:
    """The per-column maps of hgr_set_ranks for up to SETS_MAXS candidate sets, built once on the host: ``member`` int32 [n_nodes]
    (bit s = column c belongs to set s, in the order of ``sets``), ``tie_key`` int32 [n_nodes] (the model's test classes keep their
    position in the test subset, every other node follows in node order from n_test upward: a set listed in the model's test order
    breaks ties the way hgr_eval_rows does), ``names`` and ``sizes``.  ``sets``: an ordered mapping name -> node ids.  ValueError,
    before anything is allocated on the device: no set or more than SETS_MAXS, an id twice in one set, an id outside the hierarchy."""

    def __init__(self, eval_index: EvalIndex, sets):
        import numpy as np
        n = eval_index.n_nodes
        items = list(check_sets(sets, n).items())
        member = np.zeros(n, dtype=np.int32)
        for s, (name, ids) in enumerate(items):
            member[np.asarray(ids, dtype=np.int64)] |= np.int32(1 << s)
        key = np.full(n, -1, dtype=np.int64)
        if eval_index.test_pos is not None:
            key = eval_index.test_pos.cpu().numpy().astype(np.int64)
        rest = key < 0
        key[rest] = eval_index.n_test + np.arange(int(rest.sum()), dtype=np.int64)
        dev = eval_index.lvl8.device
        self.n_nodes, self.n_sets = n, len(items)
        self.names = tuple(name for name, _ in items)
        self.sizes = tuple(len(ids) for _, ids in items)
        self.member = torch.from_numpy(member).to(dev)
        self.tie_key = torch.from_numpy(key.astype(np.int32)).to(dev)


def set_ranks(scores: torch.Tensor, index: SetIndex, targets: Optional[torch.Tensor] = None, rank: Optional[torch.Tensor] = None,
              top1: Optional[torch.Tensor] = None):
    """(rank int32 [rows, S] or None, top1 int32 [rows, S]) of hgr_set_ranks (definition in include/hgr.h): per candidate set of
    ``index`` the number of its members that come before the row's target (-1: the target is no member, or no node) and its best
    member (-1: an empty set).  ``scores``: what hgr_eval_rows gets, fp32 [rows, >= n_nodes], unit column stride - a view of a wider
    buffer is fine; ``targets`` int64 [rows] or None (then only top1 is made)."""
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.stride(1) == 1
    rows, s = scores.shape[0], index.n_sets
    assert targets is None or (targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == rows)
    if top1 is None:
        top1 = torch.empty((rows, s), dtype=torch.int32, device=scores.device)
    if rank is None and targets is not None:
        rank = torch.empty((rows, s), dtype=torch.int32, device=scores.device)
    assert top1.dtype == torch.int32 and top1.shape == (rows, s) and top1.is_contiguous()
    assert rank is None or (rank.dtype == torch.int32 and rank.shape == (rows, s) and rank.is_contiguous())
    # the sizes go to the library as they are: it rejects what hgr.h lists, before anything is launched
    _lib.call("hgr_set_ranks", _dev(scores), scores.stride(0), index.n_nodes, _dev(index.member), _dev(index.tie_key), s, _dev(targets),
              _dev(rank if targets is not None else None), _dev(top1), rows, _stream())
    return (rank if targets is not None else None), top1


def set_counters_rows(rank: torch.Tensor, top1: torch.Tensor, targets: torch.Tensor, lv: torch.Tensor, anc_ptr: torch.Tensor,
                      anc_nodes: torch.Tensor, anc_levels: torch.Tensor, table: torch.Tensor) -> None:
    """Add one batch to the candidate sets' int64 table [S, REPORT_MAXL + 1, SETS_COLS] (hgr_set_counters_rows, include/hgr.h): a row
    counts in set s when rank[r, s] >= 0 and it is no padding row of eval_counters_rows; exact integer counts only."""
    assert rank.dtype == top1.dtype == lv.dtype == anc_ptr.dtype == anc_nodes.dtype == anc_levels.dtype == torch.int32
    assert rank.dim() == 2 and rank.is_contiguous() and top1.shape == rank.shape and top1.is_contiguous() and lv.is_contiguous()
    assert anc_ptr.is_contiguous() and anc_nodes.is_contiguous() and anc_levels.is_contiguous() and anc_ptr.numel() >= 2
    assert table.dtype == torch.int64 and table.shape == (rank.shape[1], REPORT_MAXL + 1, SETS_COLS) and table.is_contiguous()
    assert targets is not None and targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == rank.shape[0]
    assert lv.shape[0] == rank.shape[0]
    _lib.call("hgr_set_counters_rows", _dev(rank), _dev(top1), rank.shape[1], _dev(targets), _dev(lv), lv.shape[1], _dev(anc_ptr), _dev(anc_nodes),
              _dev(anc_levels), anc_ptr.numel() - 1, _dev(table), rank.shape[0], _stream())


def dgp_mask_value(value: float, dtype: torch.dtype) -> float:
    """`value` as a table of `dtype` stores it: the reference's `table[:, :n] = 1e-7` on an fp16 table writes 2^-23."""
    return float(torch.tensor(value, dtype=torch.float64).to(dtype))


def dgp_score_rows(table: torch.Tensor, depth: torch.Tensor, n_levels: int, n_masked: int = 0, mask_value: float = 1e-7,
                   targets: Optional[torch.Tensor] = None, target: int = 0, n_cols: Optional[int] = None, k_pred: int = 0, out=None):
    """(rank [rows], top1 [rows, 1], lv [rows, n_levels], pred [rows, k_pred] or None), all int32, of hgr_dgp_score_rows (definition
    in include/hgr.h): the DGP scoring of one classifier-product table, fp16 or fp32 [rows, >= n_cols] with unit column stride (a view
    of a wider buffer is fine).  The first `n_masked` columns read as `mask_value` rounded to the table's type; ``targets`` int64
    [rows], or one ``target`` for every row; ``out`` = the four tensors of an earlier call, to be written again."""
    assert table.dim() == 2 and table.dtype in (torch.float16, torch.float32) and table.stride(1) == 1
    assert depth.dtype == torch.int32 and depth.is_contiguous()
    rows = table.shape[0]
    nc = table.shape[1] if n_cols is None else n_cols
    assert 1 <= nc <= table.shape[1] and depth.numel() >= nc
    assert targets is None or (targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == rows)
    dev = table.device
    if out is None:
        out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty((rows, 1), dtype=torch.int32, device=dev),
               torch.empty((rows, n_levels), dtype=torch.int32, device=dev),
               torch.empty((rows, k_pred), dtype=torch.int32, device=dev) if k_pred else None)
    rank, top1, lv, pred = out
    assert rank.dtype == top1.dtype == lv.dtype == torch.int32 and rank.numel() == rows and top1.numel() == rows
    assert lv.shape == (rows, n_levels) and rank.is_contiguous() and top1.is_contiguous() and lv.is_contiguous()
    assert (pred is None) == (k_pred == 0) and (pred is None or (pred.dtype == torch.int32 and pred.shape == (rows, k_pred) and pred.is_contiguous()))
    # the sizes go to the library as they are: it rejects what hgr.h lists, before anything is launched
    _lib.call("hgr_dgp_score_rows", _dev(table), table.stride(0), 1 if table.dtype == torch.float32 else 0, nc, n_masked,
              dgp_mask_value(mask_value, table.dtype), _dev(depth), n_levels, _dev(targets), int(target), _dev(rank), _dev(top1), _dev(lv),
              _dev(pred), k_pred, rows, _stream())
    return rank, top1, lv, pred


# ---- ModifiedResNet (RN) tower -------------------------------------------------------------------
def conv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, b: int, h: int, wd: int, c: int,
                 stride: int = 1) -> torch.Tensor:
    """out NHWC = relu(conv3x3(x NHWC, pad 1) + bias); w [Cout, Kp] in (ky, kx, c) order (BN folded)."""
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and x.dtype == w.dtype == out.dtype
    prof = PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    _lib.call("hgr_conv3x3_nhwc", _dev(x), _dev(w), _dev(bias), _dev(out), b, h, wd, c, w.shape[0], stride, w.shape[1],
              DT_OF[x.dtype], _stream())
    if prof is not None:
        ev1.record()
        mo = out.shape[0]
        prof.append(("gemm_nt", ev0, ev1, 2.0 * mo * 9 * c * w.shape[0], float(2 * x.numel() + 2 * w.numel() + 2 * out.numel()), "conv3x3"))
    return out


def conv3x3_pool2_nhwc(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, b: int, h: int, wd: int, c: int) -> torch.Tensor:
    """out NHWC [b, h/2, wd/2, Cout] = avgpool2(relu(conv3x3(x NHWC, pad 1) + bias)); C = 32 only (the stem)."""
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and x.dtype == w.dtype == out.dtype
    _lib.call("hgr_conv3x3_pool2_nhwc", _dev(x), _dev(w), _dev(bias), _dev(out), b, h, wd, c, w.shape[0], w.shape[1], DT_OF[x.dtype], _stream())
    return out


def stem_conv1(image: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out NHWC [B*Ho*Ho, Cout] = relu(conv3x3 stride 2 pad 1 (image fp32 NCHW) + bias); w [Cout, Kp] folded, (ky, kx, c) order."""
    assert image.dtype == torch.float32 and image.is_contiguous() and image.shape[1] == 3 and image.shape[2] == image.shape[3]
    assert w.is_contiguous() and out.is_contiguous() and w.dtype == out.dtype and out.shape[1] == w.shape[0]
    _lib.call("hgr_stem_conv1", _dev(image), _dev(w), _dev(bias), _dev(out), image.shape[0], image.shape[2], w.shape[0], w.shape[1],
              DT_OF[out.dtype], _stream())
    return out


def stem_im2col(image: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    assert image.dtype == torch.float32 and image.is_contiguous() and out.is_contiguous() and out.shape[1] == 64
    _lib.call("hgr_stem_im2col", _dev(image), _dev(out), image.shape[0], image.shape[2], DT_OF[out.dtype], _stream())
    return out


def avgpool2_nhwc(x: torch.Tensor, out: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    _lib.call("hgr_avgpool2_nhwc", _dev(x), _dev(out), b, h, w, c, DT_OF[x.dtype], _stream())
    return out


def attnpool_tokens(x: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, b: int, s: int, c: int) -> torch.Tensor:
    _lib.call("hgr_attnpool_tokens", _dev(x), _dev(pos), _dev(out), b, s, c, DT_OF[x.dtype], _stream())
    return out


def attnpool_attend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, b: int, l: int, heads: int) -> torch.Tensor:
    assert q.dtype == torch.float32 and q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    _lib.call("hgr_attnpool_attend", _dev(q), _dev(k), _dev(v), _dev(out), b, l, heads, DT_OF[k.dtype], _stream())
    return out


# ---- torchvision-style ResNet (baseline/resnet.py) ------------------------------------------------------
def stem7_geometry(r: int):
    """(Hc, Hp): conv 7x7 / stride 2 / pad 3 outputs per edge, then max-pool 3x3 / stride 2 / pad 1."""
    hc = (r - 1) // 2 + 1
    return hc, (hc - 1) // 2 + 1


def _stem7_check(image: torch.Tensor, out: torch.Tensor) -> None:
    assert image.dtype == torch.float32 and image.is_contiguous() and image.dim() == 4 and image.shape[1] == 3 and image.shape[2] == image.shape[3]
    assert out.is_contiguous() and out.dtype in DT_OF


def stem7_pool(image: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out NHWC [B*Hp*Hp, 64] = maxpool3s2(relu(conv7x7 stride 2 pad 3 (image fp32 NCHW) + bias)) in one launch; w [64, Kp] folded,
    (ky, kx, c) order."""
    _stem7_check(image, out)
    b, r = image.shape[0], image.shape[2]
    hp = stem7_geometry(r)[1]
    assert w.is_contiguous() and w.dtype == out.dtype and w.shape[0] == 64 and bias.dtype == torch.float32 and bias.numel() == 64
    assert out.numel() == b * hp * hp * 64
    _lib.call("hgr_stem7_pool", _dev(image), _dev(w), _dev(bias), _dev(out), b, r, w.shape[1], DT_OF[out.dtype], _stream())
    return out


def stem7_im2col(image: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out [B*Hc*Hc, Kp] 16-bit: the 147 taps of every conv output in (ky, kx, c) order, zero beyond."""
    _stem7_check(image, out)
    b, r = image.shape[0], image.shape[2]
    hc = stem7_geometry(r)[0]
    assert out.dim() == 2 and out.shape[0] == b * hc * hc
    _lib.call("hgr_stem7_im2col", _dev(image), _dev(out), b, r, out.shape[1], DT_OF[out.dtype], _stream())
    return out


def maxpool3s2_nhwc(x: torch.Tensor, out: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype and x.numel() == b * h * w * c
    assert out.numel() == b * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * c
    _lib.call("hgr_maxpool3s2_nhwc", _dev(x), _dev(out), b, h, w, c, DT_OF[x.dtype], _stream())
    return out


def subsample2_nhwc(x: torch.Tensor, out: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    """out[b, yo, xo, :] = x[b, 2 yo, 2 xo, :]: the input rows of a 1 x 1 / stride 2 convolution."""
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype and x.numel() == b * h * w * c
    assert out.numel() == b * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * c
    _lib.call("hgr_subsample2_nhwc", _dev(x), _dev(out), b, h, w, c, DT_OF[x.dtype], _stream())
    return out


def meanpool_nhwc(x: torch.Tensor, out: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    """out [b, c] = mean over the h*w cells of x NHWC; out is x's 16-bit type or fp32."""
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == b * h * w * c and out.numel() == b * c
    assert out.dtype in (x.dtype, torch.float32)
    _lib.call("hgr_meanpool_nhwc", _dev(x), _dev(out), b, h, w, c, DT_OF[x.dtype], 1 if out.dtype == torch.float32 else 0, _stream())
    return out


# ---- training: backward / optimizer ------------------------------------------------------------------
def transpose16(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[c, r] = x[r, c]; out is [cols, ld >= rows] (its padding columns must already be zero)."""
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1 and x.element_size() == 2 and out.dtype == x.dtype
    _lib.call("hgr_transpose16", _dev(x), x.stride(0), _dev(out), out.stride(0), x.shape[0], x.shape[1], _stream())
    return out


def transpose16_colsum(x: torch.Tensor, out_t: torch.Tensor, colsum_out: torch.Tensor, scratch: torch.Tensor, accumulate: bool = True,
                       alpha: float = 1.0) -> torch.Tensor:
    """out_t[c][r] = x[r][c] and colsum_out[c] (+)= alpha * sum_r x[r][c] in one pass over x (16-bit)."""
    assert x.dim() == 2 and x.stride(1) == 1 and out_t.stride(1) == 1 and x.dtype == out_t.dtype and x.dtype in DT_OF
    assert colsum_out.dtype == torch.float32 and scratch.dtype == torch.float32 and colsum_out.numel() >= x.shape[1]
    rows, cols = x.shape
    assert out_t.shape[0] >= cols and out_t.stride(0) >= rows and scratch.numel() >= (rows + 63) // 64 * cols
    _lib.call("hgr_transpose16_colsum", _dev(x), x.stride(0), _dev(out_t), out_t.stride(0), rows, cols, DT_OF[x.dtype], _dev(colsum_out),
              1 if accumulate else 0, alpha, _dev(scratch), _stream())
    return out_t


def colsum(x: torch.Tensor, out: torch.Tensor, scratch: torch.Tensor, accumulate: bool = True, alpha: float = 1.0) -> torch.Tensor:
    assert x.dim() == 2 and x.stride(1) == 1 and out.dtype == torch.float32 and scratch.dtype == torch.float32
    rows, cols = x.shape
    assert scratch.numel() >= (rows + 511) // 512 * cols
    f32 = x.dtype == torch.float32
    _lib.call("hgr_colsum", _dev(x), x.stride(0), rows, cols, 1 if f32 else 0, HGR_BF16 if f32 else DT_OF[x.dtype], _dev(out),
              1 if accumulate else 0, alpha, _dev(scratch), _stream())
    return out


def cast16(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel()
    _lib.call("hgr_cast16", _dev(x), _dev(out), x.numel(), DT_OF[out.dtype], _stream())
    return out


def cast16_transpose(x: torch.Tensor, y: torch.Tensor, yt: torch.Tensor) -> None:
    """y[r, c] = (16-bit) x[r, c] and yt[c, r] = the same value, one launch (yt's columns beyond x.shape[0] are left as they are)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and y.stride(1) == 1 and yt.stride(1) == 1 and y.dtype == yt.dtype and y.dtype in DT_OF
    rows, cols = x.shape
    assert y.shape[0] == rows and y.shape[1] >= cols and yt.shape[0] >= cols and yt.stride(0) >= rows
    _lib.call("hgr_cast16_transpose", _dev(x), x.stride(0), _dev(y), y.stride(0), _dev(yt), yt.stride(0), rows, cols, DT_OF[y.dtype], _stream())


def quickgelu16(a: torch.Tensor, out: torch.Tensor, du: Optional[torch.Tensor] = None) -> torch.Tensor:
    """forward: out = a*sigmoid(1.702a); with du: out = du * g'(a)."""
    assert a.is_contiguous() and out.is_contiguous() and (du is None or du.is_contiguous())
    _lib.call("hgr_quickgelu16", _dev(a), _dev(du), _dev(out), a.numel(), 0 if du is None else 1, DT_OF[a.dtype], _stream())
    return out


def layernorm_bwd_scratch(rows: int, w: int) -> int:
    return int(_lib.load().hgr_layernorm_bwd_scratch_floats(rows, w))


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, dx: torch.Tensor, dgamma: torch.Tensor, dbeta: torch.Tensor,
                  scratch: torch.Tensor, rows: Optional[int] = None, row_mul: int = 1, row_idx: Optional[torch.Tensor] = None, eps: float = 1e-5,
                  dx16: Optional[torch.Tensor] = None, dx16_colsum: Optional[torch.Tensor] = None) -> None:
    """dx[src rows] += dLN; dgamma += ...; dbeta += ...  (all fp32, accumulate).  ``dx16``: also the updated dx rows as a 16-bit copy;
    ``dx16_colsum`` (fp32 [w], with dx16): += the column sums of those 16-bit rows (the bias gradient of the Linear they are dY of)."""
    w = x.shape[-1]
    rows = dy.shape[0] if rows is None else rows
    f32 = dy.dtype == torch.float32
    assert scratch.numel() >= layernorm_bwd_scratch(rows, w) and dy.is_contiguous()
    if dx16 is not None and dx16_colsum is not None:
        assert dx16.is_contiguous() and dx16.shape == dx.shape and (f32 or dx16.dtype == dy.dtype)
        assert dx16_colsum.dtype == torch.float32 and dx16_colsum.is_contiguous() and dx16_colsum.numel() == w
        _lib.call("hgr_layernorm_bwd_cast_colsum", _dev(dy), 1 if f32 else 0, _dev(x), _dev(gamma), _dev(dx), _dev(dx16), _dev(dgamma), _dev(dbeta),
                  _dev(dx16_colsum), _dev(scratch), rows, w, row_mul, _dev(row_idx), eps, DT_OF[dx16.dtype], _stream())
        return
    assert dx16_colsum is None
    if dx16 is not None:
        assert dx16.is_contiguous() and dx16.shape == dx.shape and (f32 or dx16.dtype == dy.dtype)
        _lib.call("hgr_layernorm_bwd_cast", _dev(dy), 1 if f32 else 0, _dev(x), _dev(gamma), _dev(dx), _dev(dx16), _dev(dgamma), _dev(dbeta), _dev(scratch),
                  rows, w, row_mul, _dev(row_idx), eps, DT_OF[dx16.dtype], _stream())
        return
    _lib.call("hgr_layernorm_bwd", _dev(dy), 1 if f32 else 0, _dev(x), _dev(gamma), _dev(dx), _dev(dgamma), _dev(dbeta), _dev(scratch),
              rows, w, row_mul, _dev(row_idx), eps, HGR_BF16 if f32 else DT_OF[dy.dtype], _stream())


def mha_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, dqkv: torch.Tensor, b: int, l: int, heads: int, causal: bool,
            stats: Optional[torch.Tensor] = None, colsum_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``colsum_part`` (fp32 [b, 3 * heads * 64], every entry written): per-sequence column sums of dqkv as rounded - summed over b
    they are the in_proj bias gradient (hgr_mha_bwd_colsum)."""
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == b * heads * l * 2
    if colsum_part is not None:
        assert colsum_part.dtype == torch.float32 and colsum_part.is_contiguous() and colsum_part.shape == (b, 3 * heads * 64)
        _lib.call("hgr_mha_bwd_colsum", _dev(qkv), _dev(out), _dev(dout), _dev(dqkv), _dev(stats), _dev(colsum_part), b, l, heads, 1 if causal else 0,
                  DT_OF[qkv.dtype], _stream())
        return dqkv
    if stats is not None:
        _lib.call("hgr_mha_bwd_stats", _dev(qkv), _dev(out), _dev(dout), _dev(dqkv), _dev(stats), b, l, heads, 1 if causal else 0,
                  DT_OF[qkv.dtype], _stream())
        return dqkv
    _lib.call("hgr_mha_bwd", _dev(qkv), _dev(out), _dev(dout), _dev(dqkv), b, l, heads, 1 if causal else 0, DT_OF[qkv.dtype], _stream())
    return dqkv


def ce_rows(logits: torch.Tensor, labels: torch.Tensor, loss_rows: torch.Tensor, dlogits: Optional[torch.Tensor] = None, gscale: float = 1.0) -> None:
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and labels.dtype == torch.int32
    _lib.call("hgr_ce_rows", _dev(logits), logits.stride(0), _dev(labels), logits.shape[0], logits.shape[1], gscale, _dev(loss_rows),
              _dev(dlogits), dlogits.stride(0) if dlogits is not None else 0, _stream())


def l2norm_bwd(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous() and x.dtype == dy.dtype == dx.dtype == torch.float32
    _lib.call("hgr_l2norm_bwd", _dev(x), _dev(dy), _dev(dx), x.shape[0], x.shape[1], 1 if accumulate else 0, _stream())
    return dx


def matmul_f32(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """out[M,N] (+)= alpha * a[M,K] @ b[K,N] for fp32 2-D tensors with ARBITRARY strides (pass .t() views freely)."""
    assert a.dtype == b.dtype == out.dtype == torch.float32 and out.stride(1) == 1 and a.shape[1] == b.shape[0]
    m, k = a.shape
    n = b.shape[1]
    _lib.call("hgr_matmul_f32", _dev(a), a.stride(0), a.stride(1), _dev(b), b.stride(0), b.stride(1), _dev(out), out.stride(0), m, n, k,
              alpha, 1 if accumulate else 0, _stream())
    return out


# ---- ModifiedResNet tower in training ---------------------------------------------------------------------------
def conv3x3_plain(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, b: int, h: int, wd: int, c: int) -> torch.Tensor:
    """out NHWC = conv3x3(x NHWC, pad 1, stride 1) with w [Cout, Kp] in (ky, kx, c) order; no bias, no activation."""
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and x.dtype == w.dtype == out.dtype
    _lib.call("hgr_conv3x3_nhwc_plain", _dev(x), _dev(w), _dev(out), b, h, wd, c, w.shape[0], w.shape[1], DT_OF[x.dtype], _stream())
    return out


def gemm_nt_splitk(a: torch.Tensor, w: torch.Tensor, partial: torch.Tensor, kc: int) -> torch.Tensor:
    """partial[s] [M, N] fp32 = a[:, s*kc:(s+1)*kc] @ w[:, same]^T for every K slice."""
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and a.dtype == w.dtype and a.shape[1] == w.shape[1]
    m, k = a.shape
    n = w.shape[0]
    s = (k + kc - 1) // kc
    assert partial.dtype == torch.float32 and partial.is_contiguous() and partial.numel() >= s * m * n
    _lib.call("hgr_gemm_nt_splitk", _dev(a), a.stride(0), _dev(w), w.stride(0), _dev(partial), n, m, n, k, kc, DT_OF[a.dtype], _stream())
    return partial


def splitk_slices(tiles: int, m: int, slots: int = 512) -> int:
    """Number of reduction slices for a split-K weight gradient with `tiles` output tiles over `m` rows, each slice at least 512
    rows deep: from the smallest count s0 that fills >= 85 % of whole rounds of `slots` workgroups up to 1.25 s0, the one that fills
    them best (16 tiles on 256 slots: 16 slices = 100 % instead of 14 = 87.5 %; measured on the 1024 x 1024 out_proj gradient of
    ViT-L/14 at batch 256: the idle CUs cost more than the two extra partial tiles)."""
    smax = max(1, min(m // 512, 4096))
    best = (0.0, 1)
    first = None
    for s in range(1, smax + 1):
        wgs = tiles * s
        eff = wgs / (-(-wgs // slots) * slots)
        if first is None and eff >= 0.85:
            first, best = s, (eff, s)
        elif first is not None:
            if s > max(first + 1, int(first * 1.25)):
                break
            if eff > best[0] + 1e-9:
                best = (eff, s)
        elif eff > best[0]:
            best = (eff, s)
    return best[1]


def tn_slices(na: int, nb: int, m: int) -> int:
    """Reduction slices of hgr_gemm_tn_splitk for a [na, nb] product over m rows, for the tile plan the library will run
    (hgr_gemm_tn_tile: 256 x 256 tiles, one workgroup per CU, or 128 x 128, two per CU)."""
    t = int(_lib.load().hgr_gemm_tn_tile(na, nb))
    return splitk_slices(-(-na // t) * -(-nb // t), m, slots=256 if t == 256 else 512)


def gemm_tn_splitk(p: torch.Tensor, q: torch.Tensor, partial: torch.Tensor, kc: int) -> torch.Tensor:
    """partial[s] [Na, Nb] = p[rows of slice s]^T . q[rows of slice s]; p [M, Na], q [M, Nb] 16-bit row-major."""
    assert p.dim() == 2 and q.dim() == 2 and p.stride(1) == 1 and q.stride(1) == 1 and p.dtype == q.dtype and p.shape[0] == q.shape[0]
    m, na = p.shape
    nb = q.shape[1]
    s = (m + kc - 1) // kc
    assert partial.dtype == torch.float32 and partial.is_contiguous() and partial.numel() >= s * na * nb
    _lib.call("hgr_gemm_tn_splitk", _dev(p), p.stride(0), _dev(q), q.stride(0), _dev(partial), nb, m, na, nb, kc, DT_OF[p.dtype], _stream())
    return partial


def conv3x3_wgrad_splitk(dy: torch.Tensor, x: torch.Tensor, partial: torch.Tensor, b: int, h: int, w: int, c: int, kc: int) -> torch.Tensor:
    """partial[s] [Cout, 9 C] in (ky, kx, c) order = dy[slice]^T . im2col(x)[slice] for a 3x3 / pad 1 / stride 1 convolution."""
    assert dy.dim() == 2 and dy.stride(1) == 1 and x.is_contiguous() and dy.dtype == x.dtype and dy.shape[0] == b * h * w
    cout = dy.shape[1]
    s = (b * h * w + kc - 1) // kc
    assert partial.dtype == torch.float32 and partial.is_contiguous() and partial.numel() >= s * cout * 9 * c
    _lib.call("hgr_conv3x3_wgrad_splitk", _dev(dy), dy.stride(0), _dev(x), _dev(partial), 9 * c, b, h, w, c, cout, kc, DT_OF[dy.dtype], _stream())
    return partial


def relu_bwd16(dy: torch.Tensor, y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = dy if out is None else out
    assert dy.is_contiguous() and y.is_contiguous() and out.is_contiguous() and dy.numel() == y.numel() == out.numel()
    _lib.call("hgr_relu_bwd16", _dev(dy), _dev(y), _dev(out), dy.numel(), DT_OF[dy.dtype], _stream())
    return out


def add16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = a if out is None else out
    assert a.is_contiguous() and b.is_contiguous() and out.is_contiguous() and a.numel() == b.numel() == out.numel()
    _lib.call("hgr_add16", _dev(a), _dev(b), _dev(out), a.numel(), DT_OF[a.dtype], _stream())
    return out


def avgpool2_bwd_nhwc(dy: torch.Tensor, dx: torch.Tensor, b: int, h: int, w: int, c: int) -> torch.Tensor:
    assert dy.is_contiguous() and dx.is_contiguous() and dx.numel() == 4 * dy.numel() == b * h * w * c
    _lib.call("hgr_avgpool2_bwd_nhwc", _dev(dy), _dev(dx), b, h, w, c, DT_OF[dy.dtype], _stream())
    return dx


def attnpool_tokens_bwd(dtok: torch.Tensor, dx: torch.Tensor, b: int, s: int, c: int) -> torch.Tensor:
    assert dtok.is_contiguous() and dx.is_contiguous() and dtok.numel() == b * (s + 1) * c and dx.numel() == b * s * c
    _lib.call("hgr_attnpool_tokens_bwd", _dev(dtok), _dev(dx), b, s, c, DT_OF[dtok.dtype], _stream())
    return dx


def im2col3x3_t(xt: torch.Tensor, out: torch.Tensor, b: int, h: int, w: int) -> torch.Tensor:
    """xt [C, ld] (transposed NHWC activation) -> out [9C, ld]: the transposed im2col of a 3x3 / pad 1 convolution."""
    c, ld = xt.shape
    assert xt.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (9 * c, ld) and ld >= b * h * w
    _lib.call("hgr_im2col3x3_t", _dev(xt), _dev(out), b, h, w, c, ld, DT_OF[xt.dtype], _stream())
    return out


def bn_fold(w: torch.Tensor, bn, w16: torch.Tensor, bias: torch.Tensor) -> None:
    """conv weight fp32 [Cout, Cin, kh, kw] + BatchNorm2d (running stats) -> folded w16 [Cout, Kp] ((ky, kx, ci) order), bias."""
    cout, cin, kh, kw = w.shape
    assert w.is_contiguous() and w.dtype == torch.float32 and w16.is_contiguous() and bias.dtype == torch.float32
    _lib.call("hgr_bn_fold", _dev(w), _dev(bn.weight.data), _dev(bn.bias.data), _dev(bn.running_mean), _dev(bn.running_var), float(bn.eps),
              _dev(w16), _dev(bias), cout, cin, kh * kw, w16.shape[1], DT_OF[w16.dtype], _stream())


def bn_unfold_grad(gwf: torch.Tensor, gbf: torch.Tensor, w: torch.Tensor, bn, g_w: torch.Tensor, g_gamma: torch.Tensor, g_beta: torch.Tensor) -> None:
    cout, cin, kh, kw = w.shape
    assert gwf.dtype == gbf.dtype == g_w.dtype == torch.float32 and gwf.stride(1) == 1 and g_w.is_contiguous() and w.is_contiguous()
    _lib.call("hgr_bn_unfold_grad", _dev(gwf), gwf.stride(0), _dev(gbf), _dev(w), _dev(bn.weight.data), _dev(bn.running_mean),
              _dev(bn.running_var), float(bn.eps), _dev(g_w), _dev(g_gamma), _dev(g_beta), cout, cin, kh * kw, _stream())


def csr_group_aggregate(support: torch.Tensor, op, att: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
                        slope: float = 1.0, normalize: bool = False) -> torch.Tensor:
    """DGP graph propagation step: out[i] = act(sum_e att[grp_e] / deg_e * (support[col_e] + bias)); `op` carries the
    merged CSR and the work-item tables (hgr_net_amd.baseline.dgp.GraphOperator)."""
    assert support.dtype == out.dtype == att.dtype == torch.float32 and support.stride(1) == 1 and out.stride(1) == 1
    assert support.shape[0] == out.shape[0] == op.n and support.shape[1] == out.shape[1] and att.numel() == op.D
    c = support.shape[1]
    _lib.call("hgr_csr_group_aggregate", _dev(support), support.stride(0), _dev(op.item_row), _dev(op.item_e0), _dev(op.item_e1),
              _dev(op.item_slot), op.item_row.numel(), _dev(op.col), _dev(op.inv_deg), _dev(op.grp), _dev(att), op.D, _dev(bias),
              _dev(op.split_row), _dev(op.split_slot0), _dev(op.split_n), op.split_row.numel(), _dev(op.partial(c)), _dev(out),
              out.stride(0), c, slope, 1 if normalize else 0, _stream())
    return out


def csr_group_att_grad(support: torch.Tensor, op, bias: Optional[torch.Tensor], g: torch.Tensor, y: Optional[torch.Tensor],
                       dout: Optional[torch.Tensor], p: torch.Tensor, slope: float = 0.2) -> torch.Tensor:
    """DGP backward gather: dout[i] = g[i] * (y[i] > 0 ? 1 : slope) (y None: g is dO already) and the attention gradient's rows
    p[i, d] = dout[i] . sum_{e in (i, d)} inv_e (support[col_e] + bias); da = colsum(p).  dout may alias g."""
    assert support.dtype == g.dtype == p.dtype == torch.float32 and support.stride(1) == 1 and g.stride(1) == 1
    assert support.shape[0] == g.shape[0] == op.n and support.shape == g.shape and p.shape == (op.n, op.D) and p.is_contiguous()
    for t in (y, dout):
        assert t is None or (t.dtype == torch.float32 and t.stride(1) == 1 and t.shape == g.shape)
    assert y is None or dout is not None
    c = support.shape[1]
    _lib.call("hgr_csr_group_att_grad", _dev(support), support.stride(0), _dev(bias), _dev(g), g.stride(0), _dev(y),
              y.stride(0) if y is not None else 0, _dev(dout), dout.stride(0) if dout is not None else 0, _dev(op.item_row), _dev(op.item_e0),
              _dev(op.item_e1), _dev(op.item_slot), op.item_row.numel(), _dev(op.col), _dev(op.inv_deg), _dev(op.grp), op.D,
              _dev(op.split_row), _dev(op.split_slot0), _dev(op.split_n), op.split_row.numel(), _dev(op.partial_groups()), _dev(p), c, slope, _stream())
    return p


def dgp_loss_head(o: torch.Tensor, rows: torch.Tensor, f: torch.Tensor, loss_rows: torch.Tensor, loss: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    """Masked L2 loss of the DGP trainer on F.normalize(o) and its gradient with respect to o (hgr_dgp_loss_head); `rows` int32, distinct
    (the caller checks: a duplicate would make two workgroups write one row of dout).  The loss stays on the device."""
    assert o.dtype == f.dtype == dout.dtype == loss_rows.dtype == loss.dtype == torch.float32 and rows.dtype == torch.int32
    assert o.stride(1) == 1 and f.stride(1) == 1 and dout.stride(1) == 1 and rows.is_contiguous() and o.shape == dout.shape
    n_t = rows.numel()
    assert f.shape == (n_t, o.shape[1]) and loss_rows.numel() >= n_t and loss.numel() >= 1
    _lib.call("hgr_dgp_loss_head", _dev(o), o.stride(0), _dev(rows), _dev(f), f.stride(0), n_t, o.shape[0], _dev(loss_rows), _dev(loss),
              _dev(dout), dout.stride(0), o.shape[1], _stream())
    return loss


def dropout_counter(x: torch.Tensor, y: torch.Tensor, seed: int, step: int, layer: int) -> torch.Tensor:
    """y = x * keep * 2 with keep = baseline.dgp.dropout_keep(seed, step, layer, rows, cols): counter-based, nothing stored; y may be x."""
    assert x.dtype == y.dtype == torch.float32 and x.dim() == 2 and x.shape == y.shape and x.stride(1) == 1 and y.stride(1) == 1
    seed &= 0xFFFFFFFF
    _lib.call("hgr_dropout_counter", _dev(x), x.stride(0), _dev(y), y.stride(0), x.shape[0], x.shape[1],
              seed - (1 << 32) if seed >> 31 else seed, step, layer, _stream())
    return y


def adam_l2(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
            wd: float = 0.0) -> None:
    """torch.optim.Adam step with coupled weight decay (hgr_adam_l2) on one fp32 tensor."""
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32 and p.numel() == g.numel() == m.numel() == v.numel()
    WEIGHTS_GEN[0] += 1
    _lib.call("hgr_adam_l2", _dev(p), _dev(g), _dev(m), _dev(v), p.numel(), lr, betas[0], betas[1], eps, wd, step, _stream())


# ---- CNZSL baseline (baseline/cnzsl.py) ------------------------------------------------------------------------------------------------
CN_EPS = 1e-5                # ClassStandardization's epsilon, added to the VARIANCE (cnzsl.py:162)
CN_MOMENTUM = 0.1            # running <- 0.9 running + 0.1 batch (cnzsl.py:165-166)
CN_RESIDENT_ROWS = 2048      # hgr_cnzsl_std_chain_*: up to this many rows a 16-column strip stays in LDS
RELU_BWD_CHUNK = 256         # hgr_relu_bwd_colsum_f32: rows per partial column sum


def _f32_rows(*ts) -> bool:
    return all(t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 for t in ts)


def cnzsl_std_chain_fwd(z: torch.Tensor, bias: torch.Tensor, running, c: torch.Tensor, a: Optional[torch.Tensor] = None,
                        stats: Optional[torch.Tensor] = None, train: bool = True, eps: float = CN_EPS, momentum: float = CN_MOMENTUM) -> torch.Tensor:
    """Modules 2 (bias) .. 5 of CNZSLModel in one launch: c = cs(relu(cs(z + bias))).  `running` = (mean1, var1, mean2, var2), fp32
    [H] each: updated in place with `train`, used as the statistics without.  Training also writes a = relu(cs(z + bias)) and
    stats [4, H] = (m1, v1, m2, v2) for the backward; S >= 2 there (HgrError before any launch otherwise)."""
    assert _f32_rows(z, c) and z.shape == c.shape and (a is None or (_f32_rows(a) and a.shape == z.shape))
    s, h = z.shape
    vecs = (bias,) + tuple(running)
    assert len(vecs) == 5 and all(v.dtype == torch.float32 and v.is_contiguous() and v.numel() == h for v in vecs)
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 4 * h)
    _lib.call("hgr_cnzsl_std_chain_fwd", _dev(z), z.stride(0), *[_dev(v) for v in vecs], _dev(c), c.stride(0), _dev(a),
              a.stride(0) if a is not None else 0, _dev(stats), s, h, 1 if train else 0, eps, momentum, _stream())
    return c


def cnzsl_std_chain_bwd(dc: torch.Tensor, a: torch.Tensor, z: torch.Tensor, bias: torch.Tensor, stats: torch.Tensor, dz: torch.Tensor,
                        dbias: torch.Tensor, eps: float = CN_EPS) -> torch.Tensor:
    """dz = d loss / d z and dbias = colsum(dz) of the training-mode chain, from dc and what the forward saved."""
    assert _f32_rows(dc, a, z, dz) and dc.shape == a.shape == z.shape == dz.shape
    s, h = z.shape
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in (bias, stats, dbias)) and bias.numel() == dbias.numel() == h and stats.numel() == 4 * h
    _lib.call("hgr_cnzsl_std_chain_bwd", _dev(dc), dc.stride(0), _dev(a), a.stride(0), _dev(z), z.stride(0), _dev(bias), _dev(stats),
              _dev(dz), dz.stride(0), _dev(dbias), s, h, eps, _stream())
    return dz


def bias_relu_f32(x: torch.Tensor, bias: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = relu(x + bias) on fp32 rows; in place without `y`."""
    y = x if y is None else y
    assert _f32_rows(x, y) and x.shape == y.shape and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == x.shape[1]
    _lib.call("hgr_bias_relu_f32", _dev(x), x.stride(0), _dev(bias), _dev(y), y.stride(0), x.shape[0], x.shape[1], _stream())
    return y


def relu_bwd_colsum_f32(dy: torch.Tensor, y: torch.Tensor, dx: torch.Tensor, db: torch.Tensor, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = dy [y > 0] (dx may be dy) and db = colsum(dx), deterministic; `scratch` fp32 [ceil(rows / 256) * C] beyond 256 rows."""
    assert _f32_rows(dy, y, dx) and dy.shape == y.shape == dx.shape and db.dtype == torch.float32 and db.is_contiguous() and db.numel() == dy.shape[1]
    rows, c = dy.shape
    chunks = -(-rows // RELU_BWD_CHUNK)
    assert chunks == 1 or (scratch is not None and scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= chunks * c)
    _lib.call("hgr_relu_bwd_colsum_f32", _dev(dy), dy.stride(0), _dev(y), y.stride(0), _dev(dx), dx.stride(0), _dev(db), _dev(scratch),
              rows, c, _stream())
    return dx


def dot_f32(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """out[0] (+)= alpha * sum(a * b) for contiguous fp32 tensors of equal size."""
    assert a.dtype == b.dtype == out.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    _lib.call("hgr_dot_f32", _dev(a), _dev(b), a.numel(), _dev(out), alpha, 1 if accumulate else 0, _stream())
    return out


def embed_scatter_add(tokens: torch.Tensor, dx: torch.Tensor, dtable: torch.Tensor, l: int) -> None:
    assert tokens.dtype == torch.int64 and tokens.stride(1) == 1 and dx.is_contiguous() and dtable.is_contiguous()
    _lib.call("hgr_embed_scatter_add", _dev(tokens), tokens.stride(0), _dev(dx), _dev(dtable), tokens.shape[0], l, dtable.shape[1], dtable.shape[0], _stream())


def rows_axpy(dst: torch.Tensor, src: torch.Tensor, dst_mul: int = 1, dst_idx: Optional[torch.Tensor] = None, alpha: float = 1.0) -> None:
    assert dst.dtype == src.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous()
    _lib.call("hgr_rows_axpy", _dev(dst), dst_mul, _dev(dst_idx), _dev(src), src.shape[0], src.shape[1], alpha, _stream())


def ctx_splice(x: torch.Tensor, ctx: torch.Tensor, pos: torch.Tensor, n: int, l: int) -> torch.Tensor:
    assert x.dtype == ctx.dtype == torch.float32 and x.is_contiguous() and ctx.is_contiguous()
    _lib.call("hgr_ctx_splice", _dev(x), _dev(ctx), _dev(pos), n, l, x.shape[1], ctx.shape[0], _stream())
    return x


def ctx_splice_bwd(dx: torch.Tensor, dctx: torch.Tensor, n: int, l: int) -> None:
    assert dx.dtype == dctx.dtype == torch.float32 and dx.is_contiguous() and dctx.is_contiguous()
    _lib.call("hgr_ctx_splice_bwd", _dev(dx), _dev(dctx), n, l, dx.shape[1], dctx.shape[0], _stream())


def rows_gather(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    assert src.dtype == out.dtype == torch.float32 and src.is_contiguous() and out.is_contiguous() and idx.dtype == torch.int32
    _lib.call("hgr_rows_gather", _dev(out), _dev(src), _dev(idx), out.shape[0], out.shape[1], _stream())
    return out


def sumsq(x: torch.Tensor, out: torch.Tensor) -> None:
    assert x.dtype == torch.float32 and x.is_contiguous()
    _lib.call("hgr_sumsq", _dev(x), x.numel(), _dev(out), _stream())


def adamw(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
          wd: float = 0.0, sumsq_total: Optional[torch.Tensor] = None, max_norm: float = 1.0, grad_scale: float = 1.0) -> None:
    assert p.is_contiguous() and g.is_contiguous() and p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
    WEIGHTS_GEN[0] += 1
    _lib.call("hgr_adamw", _dev(p), _dev(g), _dev(m), _dev(v), p.numel(), lr, betas[0], betas[1], eps, wd, step, _dev(sumsq_total), max_norm, grad_scale, _stream())


# ---- FREE baseline (baseline/free.py) ------------------------------------------------------------------------------------------------------
OUT_F32 = 2                         # HGR_OUT_F32: the fp32 value of an `out_type`
ACT_LRELU02, ACT_SIGMOID = 0, 1     # HGR_ACT_*
NLL_RESIDENT_COLS = 18432           # HGR_NLL_RESIDENT_COLS: up to this many columns hgr_nll_rows16 keeps a row in LDS


def _out_type(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return OUT_F32
    if t.dtype not in DT_OF:
        raise _lib.HgrError(f"destination must be bf16, f16 or fp32, got {t.dtype}")
    return DT_OF[t.dtype]


def _seed32(seed: int) -> int:
    seed &= 0xFFFFFFFF
    return seed - (1 << 32) if seed >> 31 else seed


def normal_counter(out: torch.Tensor, seed: int, stream: int, row0: int = 0, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r, c] = baseline.free.normal_host(seed, stream, row0 + r, c): counter-based N(0, 1), fp32.  `bits` (int32 [rows, C, 2],
    optional) receives the two 32-bit draws of every element."""
    assert _f32_rows(out) and (bits is None or (bits.dtype == torch.int32 and bits.is_contiguous() and bits.numel() == 2 * out.numel()))
    _lib.call("hgr_normal_counter", _dev(out), out.stride(0), _dev(bits), out.shape[0], out.shape[1], _seed32(seed), stream, row0, _stream())
    return out


def free_gen_input(out: torch.Tensor, attribute: torch.Tensor, classes: torch.Tensor, num: int, nz: int, seed: int = 0, stream: int = 0,
                   row0: int = 0, z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [rows, nz + A] = cat(noise, attribute[classes[(row0 + r) // num]]) for the synthetic rows [row0, row0 + rows): the noise
    is the counter normal of (seed, stream, row0 + r, c), or `z` [rows, nz] fp32."""
    assert out.dim() == 2 and out.stride(1) == 1 and _f32_rows(attribute) and classes.dtype == torch.int32 and classes.is_contiguous()
    assert z is None or (_f32_rows(z) and z.shape == (out.shape[0], nz))
    a = attribute.shape[1]
    assert out.shape[1] == nz + a
    _lib.call("hgr_free_gen_input", _dev(out), out.stride(0), _out_type(out), _dev(z), z.stride(0) if z is not None else 0, _dev(attribute),
              attribute.stride(0), attribute.shape[0], _dev(classes), classes.numel(), num, out.shape[0], nz, a, _seed32(seed), stream, row0, _stream())
    return out


def bias_act_rows(x: torch.Tensor, bias: torch.Tensor, y: torch.Tensor, act: int, col0: int = 0) -> torch.Tensor:
    """y[:, col0:col0 + C] = act(x + bias): act = ACT_LRELU02 or ACT_SIGMOID; y bf16 / f16 / fp32, the rest of y untouched."""
    assert _f32_rows(x) and y.dim() == 2 and y.stride(1) == 1 and y.shape[0] == x.shape[0] and y.shape[1] >= col0 + x.shape[1]
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == x.shape[1]
    _lib.call("hgr_bias_act_rows", _dev(x), x.stride(0), _dev(bias), _dev(y), y.stride(0), col0, _out_type(y), act, x.shape[0], x.shape[1], _stream())
    return y


def free_fr_tail(lantent: torch.Tensor, y: torch.Tensor, col0: int = 0, bias: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                 seed: int = 0, stream: int = 0, row0: int = 0, mus: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[:, col0:col0 + A] = sigmoid(mu + eps * sigmoid(sd)), (mu, sd) = the halves of lantent [rows, 2A] (+ bias); `eps` [rows, A]
    fp32 or the counter normals of (seed, stream, row0 + r, c); `mus` [rows, A] fp32 receives mu."""
    assert _f32_rows(lantent) and lantent.shape[1] % 2 == 0 and y.dim() == 2 and y.stride(1) == 1 and y.shape[0] == lantent.shape[0]
    rows, a = lantent.shape[0], lantent.shape[1] // 2
    assert y.shape[1] >= col0 + a and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == 2 * a))
    assert (eps is None or (_f32_rows(eps) and eps.shape == (rows, a))) and (mus is None or (_f32_rows(mus) and mus.shape == (rows, a)))
    _lib.call("hgr_free_fr_tail", _dev(lantent), lantent.stride(0), _dev(bias), _dev(eps), eps.stride(0) if eps is not None else 0, _dev(y),
              y.stride(0), col0, _out_type(y), _dev(mus), mus.stride(0) if mus is not None else 0, rows, a, _seed32(seed), stream, row0, _stream())
    return y


def nll_rows16(logits: torch.Tensor, labels: Optional[torch.Tensor], n: Optional[int] = None, loss_rows: Optional[torch.Tensor] = None,
               dlogits: Optional[torch.Tensor] = None, logsm: Optional[torch.Tensor] = None, dtype=None) -> None:
    """NLLLoss(LogSoftmax) over the first `n` columns of fp32 logits [rows, ld]: loss_rows [rows]; dlogits 16-bit [rows, >= ld] =
    softmax - onehot (unscaled, columns [n, ld) zero); logsm fp32 (may be `logits`) = the log-softmax of columns [0, n)."""
    assert _f32_rows(logits) and (labels is None or (labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == logits.shape[0]))
    rows, ld = logits.shape[0], logits.stride(0)
    n = logits.shape[1] if n is None else n
    assert 1 <= n <= logits.shape[1]
    assert loss_rows is None or (loss_rows.dtype == torch.float32 and loss_rows.is_contiguous() and loss_rows.numel() == rows)
    assert dlogits is None or (dlogits.dtype in DT_OF and dlogits.dim() == 2 and dlogits.stride(1) == 1 and dlogits.shape[0] == rows and dlogits.shape[1] >= ld)
    assert logsm is None or (_f32_rows(logsm) and logsm.shape[0] == rows and logsm.shape[1] >= n)
    dt = DT_OF[dlogits.dtype] if dlogits is not None else (HGR_BF16 if dtype is None else dtype_code(dtype))
    _lib.call("hgr_nll_rows16", _dev(logits), ld, _dev(labels), rows, n, _dev(loss_rows), _dev(dlogits), dlogits.stride(0) if dlogits is not None else 0,
              _dev(logsm), logsm.stride(0) if logsm is not None else 0, dt, _stream())


def adam_l2_cast16(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, w16: torch.Tensor, lr: float, step: int, slices: int = 1,
                   alpha: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8, wd: float = 0.0) -> None:
    """`adam_l2` on g' = alpha * (g[0] + ... + g[slices - 1]) (g: `slices` contiguous slices of p.numel() floats, added in order),
    and w16 = (16-bit) p, in one pass over the weight."""
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous() and w16.is_contiguous()
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32 and w16.dtype in DT_OF
    n = p.numel()
    assert m.numel() == v.numel() == w16.numel() == n and g.numel() >= slices * n and slices >= 1
    WEIGHTS_GEN[0] += 1
    _lib.call("hgr_adam_l2_cast16", _dev(p), _dev(g), n, slices, alpha, _dev(m), _dev(v), _dev(w16), n, lr, betas[0], betas[1], eps, wd, step,
              DT_OF[w16.dtype], _stream())
