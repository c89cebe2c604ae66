"""Weight gradient of a Linear, 1x1 or 3x3 layer: dW += dY^T . X (3x3: dY^T . im2col(X)) and db += column sums of dY.

The product has a small output and a reduction over every row of the batch, so the reduction is cut into slices that fill the
chip, every slice leaves an fp32 partial and `hgr_colsum` adds the partials in a fixed order.  `plan` decides route, slice count
and slice depth from the shape alone (host only, no launch); `WeightGrad.add` owns the buffers and makes the launches.  The
training step (training.py, training_rn.py), the FREE classifier's step and the tools/wgrad*_bench.py scripts all go through here.

Routes:
  * "tn" / "tn_conv": the operands as they lie in memory (`hgr_gemm_tn_splitk`, `hgr_conv3x3_wgrad_splitk`).
  * "nt": both operands transposed first (`hgr_transpose16[_colsum]`), then `hgr_gemm_nt_splitk`, or `hgr_gemm_nt` with the
    accumulate epilogue for one slice.  Taken by a Linear / 1x1 whose operands the TN kernels cannot read (`tn_blocker`): in the
    training step that is the patch-14 ViT conv1, K = 3 * 14 * 14 = 588.  There is no transposing 3x3 route.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import torch

from . import ops
from ._lib import EPI_ACCUM, HgrError


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def grad(p: torch.nn.Parameter) -> torch.Tensor:
    """The fp32 accumulator behind ``p.grad``, made on first use."""
    if p.grad is None:
        p.grad = torch.zeros_like(p.data, dtype=torch.float32)
    return p.grad


class WgradPlan(NamedTuple):
    route: str              # "tn" | "tn_conv" | "nt"
    slices: int
    kc: Optional[int]       # rows of the reduction per slice; None: one `hgr_gemm_nt` launch with EPI_ACCUM, no partial
    mp: int                 # length of the reduction as the kernel sees it: m, on "nt" m padded to a multiple of 64


def plan(cout: int, k: int, m: int, *, conv: bool = False, tn_ok: bool = True) -> WgradPlan:
    """Slice plan of a [cout, k] weight gradient over m rows (conv: k = 9 C).  ``tn_ok``: the operands pass `tn_blocker`."""
    if tn_ok:
        # the conv loader always runs on 128-tiles; the linear product asks the library for its tile (hgr_gemm_tn_tile)
        s0 = ops.splitk_slices(-(-cout // 128) * -(-k // 128), m) if conv else ops.tn_slices(cout, k, m)
        kc = pad64(-(-m // s0))
        return WgradPlan("tn_conv" if conv else "tn", -(-m // kc), kc, m)
    if conv:
        raise HgrError("3x3 weight gradient: there is no transposing route")
    mp = pad64(m)
    if cout >= 256 and k >= 256:                              # 256^2 tiles, one workgroup per CU
        s = min(mp // 128, -(-256 // (-(-cout // 256) * -(-k // 256))))
    else:
        s = min(mp // 64, -(-512 // (-(-cout // 128) * -(-k // 128))))
    if s <= 1:
        return WgradPlan("nt", 1, None, mp)
    # few output tiles, long reduction: slice K over the chip, add the fp32 partials in a fixed order
    kc = pad64(-(-mp // s))
    return WgradPlan("nt", -(-mp // kc), kc, mp)


def tn_blocker(cout: int, k: int, dy_stride, x_stride, dy_ptr: int, x_ptr: int, *, conv: bool = False, x_contiguous: bool = True) -> Optional[str]:
    """None when the TN kernels can read dY [m, cout] and X [m, k] (conv: [m, k / 9]) where they lie, else the condition that
    fails.  Plain integers: strides in elements as (row, column), pointers in bytes."""
    if cout % 8 or k % 8:
        return f"cout = {cout} and k = {k} must be multiples of 8"
    if dy_stride[1] != 1 or x_stride[1] != 1:
        return f"column strides {dy_stride[1]}, {x_stride[1]} must be 1"
    if dy_stride[0] % 8 or x_stride[0] % 8:
        return f"row strides {dy_stride[0]}, {x_stride[0]} must be multiples of 8 elements"
    if dy_ptr % 16 or x_ptr % 16:
        return "both operands must be 16-byte aligned"
    if conv and not x_contiguous:
        return "the input of a 3x3 layer must be contiguous"
    return None


class WeightGrad:
    """`add` for one dtype and device.  Owns the fp32 partials, the reduce buffer and the transposed operands of the "nt" route,
    each grown on demand and reused by every layer and step; ``scratch(n)`` hands out >= n fp32 of column-sum scratch."""

    def __init__(self, dt: torch.dtype, dev, scratch: Callable[[int], torch.Tensor]):
        self.dt, self.dev, self.scratch = dt, dev, scratch
        self._bufs: Dict[str, torch.Tensor] = {}

    def _buf(self, name: str, rows: int, cols: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or t.numel() < rows * cols:
            t = self._bufs[name] = torch.empty(rows * cols, dtype=dtype, device=self.dev)
        return t[: rows * cols].view(rows, cols)

    def add(self, gw: torch.Tensor, dy16: torch.Tensor, x16: torch.Tensor, *, gb: Optional[torch.Tensor] = None,
            dy_colsum: Optional[torch.Tensor] = None, conv: Optional[tuple] = None) -> None:
        """gw[:, :k] += dy16^T . x16, or dy16^T . im2col(x16) with ``conv`` = (b, h, c) (3x3, pad 1, stride 1, k = 9 c in
        (ky, kx, c) order).  dy16 [m, cout], x16 [m, k] (conv: [m, c]); gw fp32 [cout, >= k], contiguous - columns >= k are
        never written.  ``gb`` [cout] += column sums of dy16; None: the producer of dy16 has added them already.  ``dy_colsum``:
        partial column sums of dy16 its producer made (fp32 [rows, cout], e.g. one row per 64 rows of dy16) - the bias gradient is
        their column sum, dy16 is not read again.  On the "nt" route the sums ride on the transposition of an aligned dy16 instead."""
        m, cout = dy16.shape
        k = 9 * conv[2] if conv else x16.shape[1]
        why = tn_blocker(cout, k, dy16.stride(), x16.stride(), dy16.data_ptr(), x16.data_ptr(), conv=bool(conv), x_contiguous=x16.is_contiguous())
        if why and conv:
            raise HgrError(f"3x3 weight gradient: {why} (there is no transposing route)")
        p = plan(cout, k, m, conv=bool(conv), tn_ok=why is None)
        part = self._buf("part", p.slices, cout * k) if p.kc else None
        if p.route == "nt":
            dyt, xt = self._buf("dyt", cout, p.mp, self.dt), self._buf("xt", k, p.mp, self.dt)
            if p.mp != m:                                     # the pad columns must be zero, the rest is overwritten
                dyt.zero_()
                xt.zero_()
            if gb is not None and dy16.stride(0) % 8 == 0 and dy16.data_ptr() % 16 == 0:      # db rides on the transposition of dY
                ops.transpose16_colsum(dy16, dyt, gb, self.scratch((m + 63) // 64 * cout), accumulate=True)
                gb = None
            else:
                ops.transpose16(dy16, dyt)
            ops.transpose16(x16, xt)
            if part is None:
                ops.gemm_nt(dyt, xt, gw, epilogue=EPI_ACCUM)
            else:
                ops.gemm_nt_splitk(dyt, xt, part, p.kc)
        elif conv:
            ops.conv3x3_wgrad_splitk(dy16, x16, part, conv[0], conv[1], conv[1], conv[2], p.kc)
        else:
            ops.gemm_tn_splitk(dy16, x16, part, p.kc)
        if part is not None:
            self._add_slices(part, gw, cout, k)
        if gb is not None:
            src = dy_colsum if dy_colsum is not None else dy16
            ops.colsum(src, gb, self.scratch((src.shape[0] + 511) // 512 * cout), accumulate=True)

    def _add_slices(self, part: torch.Tensor, gw: torch.Tensor, cout: int, k: int) -> None:
        """gw [cout, >= k] += sum of the fp32 slices part [s, cout * k]."""
        scratch = self.scratch((part.shape[0] + 511) // 512 * cout * k) if part.shape[0] > 1 else None
        if part.shape[0] > 1 and gw.shape[1] == k:
            ops.colsum(part, gw.view(-1), scratch, accumulate=True)
            return
        if part.shape[0] > 1:                                 # accumulator is K-padded: reduce, then add the live columns
            red = self._buf("red", cout, k)
            ops.colsum(part, red.view(-1), scratch, accumulate=False)
        else:
            red = part.view(cout, k)
        gw[:, :k].add_(red)
