"""OM / hierarchical training step on libhgr.so: what the reference's ``tree_model.train_batch``
(model/clip_tree.py:222-316) and the optimiser glue of ``main.train`` (main.py:86-94) compute.

The reference leans on torch autograd; here forward-with-saves and the backward chains are written
out explicitly and every product / reduction runs in a hand-written kernel:

* towers run with 16-bit MFMA inputs (default bf16, BASELINE configs[4]) on fp32 master weights, an
  fp32 residual stream and fp32 gradients that ACCUMULATE into ``param.grad`` (autograd semantics - the
  K x M inner ``loss_j.backward()`` calls of one step all add into the text tower's gradients);
* per linear layer: dX = dY . W is ``hgr_gemm_nt`` against a weight transposed once per step,
  dW += dY^T . X is ``hgr_gemm_nt`` on transposed activations with the accumulate epilogue, db is a
  column sum; LayerNorm / QuickGELU / attention / L2-norm backward are their own kernels;
* the loss head ([B, <= 257] logits, the two projections) is tiny and stays in fp32 (``hgr_matmul_f32``);
* like the reference, the image tower is run forward once, the image-side gradient of all inner steps
  is accumulated on the detached normalised features, and ONE image-tower backward follows
  (clip_tree.py:224-226,280).

Only the host-side orchestration is Python; ``random`` drives negative sampling exactly as in the
reference (seed it for reproducibility).  ModifiedResNet image towers: training_rn.py.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import torch

from . import ops
from ._lib import EPI_BIAS, EPI_BIAS_RESIDUAL, EPI_QGELU_GRAD16, HgrError
from .clip.model import VisionTransformer
from .wgrad import WeightGrad, grad as _grad, pad64 as _pad64


import os

# QuickGELU backward in the epilogue of the c_proj data-gradient GEMM; HGR_GELU_BWD_FUSED=0 keeps the separate pass for A/B runs
GELU_BWD_FUSED = os.environ.get("HGR_GELU_BWD_FUSED", "1") != "0"
GELU_FWD_FUSED = os.environ.get("HGR_GELU_FWD_FUSED", "1") != "0"     # c_fc forward writes pre-activation and activation in one launch
COLSUM_FUSED = os.environ.get("HGR_COLSUM_FUSED", "1") != "0"         # bias gradients as by-products of the kernels that produce dY (no hgr_colsum pass over dY)


def check_distinct_ids(id_lists) -> None:
    """Every inner step's node ids must be distinct: its text-feature gradient goes back with hgr_rows_axpy, a plain ``+=`` per
    destination row (include/hgr.h), so a node listed twice in one step would receive one of its two gradients, or a torn sum.
    Host lists only: no device work, no sync."""
    for j, ids in enumerate(id_lists):
        seen = set()
        for i in ids:
            if i in seen:
                raise ValueError(f"OMTrainer: inner step {j} lists node {i} twice (ids must be distinct: a duplicate row would receive two gradients)")
            seen.add(i)


class _Lin:
    """One nn.Linear-shaped weight in training form: 16-bit copy, its transpose, fp32 bias, grad targets."""

    def __init__(self, weight: torch.nn.Parameter, bias: Optional[torch.nn.Parameter], dt: torch.dtype, kpad: int = 0):
        self.weight, self.bias = weight, bias
        self.n, self.k = weight.shape[0], weight.numel() // weight.shape[0]
        dev = weight.device
        # buffers live as long as the engine: refresh() re-derives their contents from the fp32 master every step in ONE launch
        # (hgr_cast16_transpose); the zero padding (K of the patch-14 forward operand 588 -> 640, N of the transposed operand to a
        # multiple of 64) is written once, here
        kp = max(kpad, self.k)
        self.w16_fwd = (torch.zeros if kp > self.k else torch.empty)(self.n, kp, dtype=dt, device=dev)
        self.w16 = self.w16_fwd[:, : self.k] if kp > self.k else self.w16_fwd
        self.wt16 = torch.zeros(self.k, _pad64(self.n), dtype=dt, device=dev)             # [K, N] for dX = dY . W
        self.refresh()

    def refresh(self) -> None:
        """This step's 16-bit operands from the (updated) fp32 weight."""
        w32 = self.weight.data.reshape(self.n, self.k)
        if not w32.is_contiguous():
            w32 = w32.contiguous()
        ops.cast16_transpose(w32, self.w16_fwd, self.wt16)
        self.b32 = self.bias.data if self.bias is not None else None


class _Blk:
    def __init__(self, blk, dt):
        self.ln1, self.ln2 = blk.ln_1, blk.ln_2
        self.w_in = _Lin(blk.attn.in_proj_weight, blk.attn.in_proj_bias, dt)
        self.w_out = _Lin(blk.attn.out_proj.weight, blk.attn.out_proj.bias, dt)
        self.w_fc = _Lin(blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, dt)
        self.w_proj = _Lin(blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, dt)

    def refresh(self) -> None:
        for lin in (self.w_in, self.w_out, self.w_fc, self.w_proj):
            lin.refresh()


class Engine:
    """Forward-with-saves / backward for the transformer stacks of one CLIP model."""

    def __init__(self, clip_model, dtype: str = "bf16"):
        self.m = clip_model
        self.dt = ops.TORCH16[ops.dtype_code(dtype)]
        self.dev = next(clip_model.parameters()).device
        self._scratch = None
        self.wgrad = WeightGrad(self.dt, self.dev, self.scratch)      # one set of weight-gradient buffers for every layer of both towers

    # -- helpers -------------------------------------------------------------------------------
    def scratch(self, n: int) -> torch.Tensor:
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = torch.empty(max(n, 1 << 22), dtype=torch.float32, device=self.dev)
        return self._scratch

    def prepare(self):
        """16-bit weight copies + transposes for this step (weights change every step)."""
        m, dt = self.m, self.dt
        vit = isinstance(m.visual, VisionTransformer)
        # the operand buffers are built once per set of parameter OBJECTS (a reloaded / re-wrapped model builds them again) and
        # refreshed in place afterwards: one launch per weight instead of allocations + cast + zero fill + transpose
        key = tuple(id(p) for p in m.transformer.parameters()) + (tuple(id(p) for p in m.visual.parameters()) if vit else ())
        if getattr(self, "_prep_key", None) == key:
            for blk in self.tblocks:
                blk.refresh()
            if vit:
                for blk in self.vblocks:
                    blk.refresh()
                self.conv.refresh()
        else:
            self.tblocks = [_Blk(b, dt) for b in m.transformer.resblocks]
            if vit:
                self.vblocks = [_Blk(b, dt) for b in m.visual.transformer.resblocks]
                ps = m.visual.patch_size
                self.conv = _Lin(m.visual.conv1.weight, None, dt, kpad=_pad64(3 * ps * ps))
            self._prep_key = key
        self.rn = None
        if not vit:
            from .training_rn import RNTower                # ModifiedResNet (the reference's README trains --arch RN50)
            self.rn = RNTower(m.visual, dt, self.scratch, self.wgrad)

    def _linear_bwd(self, lin: _Lin, dy16: torch.Tensor, x16: torch.Tensor, m: int, need_dx: bool = True,
                    gelu_pre: Optional[torch.Tensor] = None, dy_colsum: Optional[torch.Tensor] = None,
                    dx_colsum: Optional[list] = None, bias_done: bool = False) -> Optional[torch.Tensor]:
        """dW += dY^T X, db += colsum(dY) (wgrad.py); returns dX = dY W (16-bit) if wanted.  dy16 [m, n], x16 [m, >= k].
        ``dy_colsum``: partial column sums of dy16 its producer already made (fp32 [rows, n]): db comes from them, dy16 is not
        read a third time.  ``dx_colsum`` (a list, with ``gelu_pre``): receives such sums of the returned dX.
        ``bias_done``: the producer of dy16 already added its column sums to the bias gradient (hgr_layernorm_bwd_cast_colsum)."""
        self.wgrad.add(_grad(lin.weight).view(lin.n, lin.k), dy16, x16[:, : lin.k],
                       gb=_grad(lin.bias) if lin.bias is not None and not bias_done else None, dy_colsum=dy_colsum)
        return self._linear_dx(lin, dy16, m, gelu_pre, dx_colsum) if need_dx else None

    def _linear_dx(self, lin: _Lin, dy16: torch.Tensor, m: int, gelu_pre: Optional[torch.Tensor] = None, dx_colsum: Optional[list] = None) -> torch.Tensor:
        """dX = dY W (16-bit).  With ``gelu_pre`` (the QuickGELU pre-activation that produced this layer's input) the GEMM's
        epilogue multiplies by g'(pre): the result is the gradient w.r.t. the pre-activation, no separate activation pass."""
        dx = torch.empty(m, lin.k, dtype=self.dt, device=self.dev)
        if lin.n % 64:
            raise HgrError("backward GEMM needs the output width to be a multiple of 64")
        wt = lin.wt16[:, : lin.n] if lin.wt16.shape[1] == lin.n else lin.wt16
        if gelu_pre is not None:
            if dx_colsum is not None and COLSUM_FUSED and ops.gelu_dual_ok(m, lin.k, wt.shape[1], dy16.stride(0), wt.stride(0)) \
                    and wt.shape[0] == lin.k and gelu_pre.stride(0) % 8 == 0 and m >= 256:
                # the column sums of dX (= the bias gradient of the layer below) leave the same epilogue (hgr_gemm_nt_qgelu_grad_colsum)
                part = torch.empty((m + 63) // 64, lin.k, dtype=torch.float32, device=self.dev)
                ops.gemm_nt_qgelu_grad_colsum(dy16, wt, dx, gelu_pre, part)
                dx_colsum.append(part)
            else:
                ops.gemm_nt(dy16, wt, dx, residual=gelu_pre, epilogue=EPI_QGELU_GRAD16, n=lin.k)
        else:
            ops.gemm_nt(dy16, wt, dx, n=lin.k)
        return dx

    # -- transformer stack ---------------------------------------------------------------------
    def blocks_fwd(self, x: torch.Tensor, blocks: List[_Blk], heads: int, b: int, l: int, causal: bool):
        """Returns (x_out, saves).  Same arithmetic as clip.model._run_blocks, out of place, keeping what backward needs."""
        m, w = x.shape
        dt, dev = self.dt, self.dev
        saves = []
        for k in blocks:
            h1 = torch.empty(m, w, dtype=dt, device=dev)
            ops.layernorm(x, k.ln1.weight.data, k.ln1.bias.data, h1)
            qkv = torch.empty(m, 3 * w, dtype=dt, device=dev)
            ops.gemm_nt(h1, k.w_in.w16, qkv, bias=k.w_in.b32, epilogue=EPI_BIAS)
            att = torch.empty(m, w, dtype=dt, device=dev)
            st = torch.empty(b, heads, l, 2, dtype=torch.float32, device=dev) if l > 32 else None     # softmax row statistics for mha_bwd
            ops.mha(qkv, att, b, l, heads, causal, stats=st)
            x1 = torch.empty_like(x)
            ops.gemm_nt(att, k.w_out.w16, x1, bias=k.w_out.b32, residual=x, epilogue=EPI_BIAS_RESIDUAL)
            h2 = torch.empty(m, w, dtype=dt, device=dev)
            ops.layernorm(x1, k.ln2.weight.data, k.ln2.bias.data, h2)
            a = torch.empty(m, 4 * w, dtype=dt, device=dev)
            u = torch.empty_like(a)
            if GELU_FWD_FUSED and ops.gelu_dual_ok(m, 4 * w, k.w_fc.w16.shape[1], h2.stride(0), k.w_fc.w16.stride(0)) and m >= 256:
                ops.gemm_nt_bias_gelu_dual(h2, k.w_fc.w16, a, u, k.w_fc.b32)          # pre-activation and activation from one GEMM
            else:
                ops.gemm_nt(h2, k.w_fc.w16, a, bias=k.w_fc.b32, epilogue=EPI_BIAS)
                ops.quickgelu16(a, u)
            x2 = torch.empty_like(x)
            ops.gemm_nt(u, k.w_proj.w16, x2, bias=k.w_proj.b32, residual=x1, epilogue=EPI_BIAS_RESIDUAL)
            saves.append((x, h1, qkv, att, x1, h2, a, u, st))
            x = x2
        return x, saves

    def blocks_bwd(self, dx: torch.Tensor, blocks: List[_Blk], saves, heads: int, b: int, l: int, causal: bool) -> torch.Tensor:
        """dx: fp32 gradient w.r.t. the stack output (consumed in place); returns the gradient w.r.t. its input."""
        m, w = dx.shape
        dt, dev = self.dt, self.dev
        scr = self.scratch(ops.layernorm_bwd_scratch(m, w))
        dy = torch.empty(m, w, dtype=dt, device=dev)
        ops.cast16(dx, dy)               # later 16-bit copies of dx come out of the LayerNorm backward that updates it
        # bias gradients of out_proj / c_proj = column sums of the residual-stream gradient `dy`: the LayerNorm backward that writes dy
        # adds them on its way (COLSUM_FUSED); only the stack's first dy (the cast above) goes through hgr_colsum
        order = list(reversed(blocks))
        proj_bias_done = False
        for pos, (k, (x0, h1, qkv, att, x1, h2, a, u, st)) in enumerate(zip(order, reversed(saves))):
            # x2 = x1 + c_proj(gelu(c_fc(ln_2(x1))))
            da_sums: list = []
            if GELU_BWD_FUSED:      # d(pre-activation) straight from the c_proj data-gradient GEMM (HGR_EPI_QGELU_GRAD16)
                da = self._linear_bwd(k.w_proj, dy, u, m, gelu_pre=a, dx_colsum=da_sums, bias_done=proj_bias_done)
            else:
                du = self._linear_bwd(k.w_proj, dy, u, m, bias_done=proj_bias_done)
                da = torch.empty_like(a)
                ops.quickgelu16(a, da, du=du)
            dh2 = self._linear_bwd(k.w_fc, da, h2, m, dy_colsum=da_sums[0] if da_sums else None)
            out_b = _grad(k.w_out.bias) if COLSUM_FUSED and k.w_out.bias is not None else None
            ops.layernorm_bwd(dh2, x1, k.ln2.weight.data, dx, _grad(k.ln2.weight), _grad(k.ln2.bias), scr, dx16=dy, dx16_colsum=out_b)
            # x1 = x0 + out_proj(attn(in_proj(ln_1(x0))))
            datt = self._linear_bwd(k.w_out, dy, att, m, bias_done=out_b is not None)
            dqkv = torch.empty_like(qkv)
            qkv_sums = torch.empty(b, 3 * w, dtype=torch.float32, device=dev) if COLSUM_FUSED and k.w_in.bias is not None and l <= 320 else None
            ops.mha_bwd(qkv, att, datt, dqkv, b, l, heads, causal, stats=st, colsum_part=qkv_sums)
            dh1 = self._linear_bwd(k.w_in, dqkv, h1, m, dy_colsum=qkv_sums)
            nxt = order[pos + 1] if pos + 1 < len(order) else None
            proj_b = _grad(nxt.w_proj.bias) if COLSUM_FUSED and nxt is not None and nxt.w_proj.bias is not None else None
            ops.layernorm_bwd(dh1, x0, k.ln1.weight.data, dx, _grad(k.ln1.weight), _grad(k.ln1.bias), scr, dx16=dy, dx16_colsum=proj_b)
            proj_bias_done = proj_b is not None
        return dx

    # -- image tower (ViT) ----------------------------------------------------------------------
    def image_fwd(self, image: torch.Tensor):
        if self.rn is not None:
            return self.rn.fwd(image)
        v, dt, dev = self.m.visual, self.dt, self.dev
        image = image.float().contiguous()
        b, _, r, _ = image.shape
        ps = v.patch_size
        g = r // ps
        l, w = g * g + 1, v.conv1.weight.shape[0]
        kp = _pad64(3 * ps * ps)
        patches = torch.zeros(b * l, kp, dtype=dt, device=dev)           # class rows (and the K padding) stay zero
        ops.im2col_patches_tokens(image, patches, ps, l)
        t = torch.empty(b * l, w, dtype=torch.float32, device=dev)
        ops.gemm_nt(patches, self.conv.w16_fwd, t)
        ops.vit_assemble(t, v.class_embedding.data, v.positional_embedding.data, b, l)
        x = torch.empty_like(t)
        ops.layernorm(t, v.ln_pre.weight.data, v.ln_pre.bias.data, x)    # fp32 out
        xl, saves = self.blocks_fwd(x, self.vblocks, w // 64, b, l, False)
        c32 = torch.empty(b, w, dtype=torch.float32, device=dev)
        ops.layernorm(xl, v.ln_post.weight.data, v.ln_post.bias.data, c32, rows=b, row_mul=l)
        feat = torch.empty(b, v.output_dim, dtype=torch.float32, device=dev)
        ops.matmul_f32(c32, v.proj.data, feat)                            # [B, W] @ [W, D], fp32 head
        return feat, dict(patches=patches, t=t, xl=xl, saves=saves, c32=c32, b=b, l=l, w=w)

    def image_bwd(self, dfeat: torch.Tensor, s: dict):
        if self.rn is not None:
            return self.rn.bwd(dfeat, s)
        v, dt, dev = self.m.visual, self.dt, self.dev
        b, l, w = s["b"], s["l"], s["w"]
        ops.matmul_f32(s["c32"].t(), dfeat, _grad(v.proj), accumulate=True)                 # dproj += c^T dfeat
        dc = torch.empty(b, w, dtype=torch.float32, device=dev)
        ops.matmul_f32(dfeat, v.proj.data.t(), dc)                                          # dc = dfeat proj^T
        dx = torch.zeros(b * l, w, dtype=torch.float32, device=dev)
        scr = self.scratch(ops.layernorm_bwd_scratch(b * l, w))
        ops.layernorm_bwd(dc, s["xl"], v.ln_post.weight.data, dx, _grad(v.ln_post.weight), _grad(v.ln_post.bias), scr, rows=b, row_mul=l)
        dx = self.blocks_bwd(dx, self.vblocks, s["saves"], w // 64, b, l, False)
        dt_ = torch.zeros(b * l, w, dtype=torch.float32, device=dev)
        ops.layernorm_bwd(dx, s["t"], v.ln_pre.weight.data, dt_, _grad(v.ln_pre.weight), _grad(v.ln_pre.bias), scr)
        # t[b,l] = patch_out[b,l] + pos[l] + (l == 0) cls
        ops.colsum(dt_.view(b, l * w), _grad(v.positional_embedding).view(-1), self.scratch(((b + 511) // 512) * l * w), accumulate=True)
        ops.colsum(dt_.view(b, l * w)[:, :w], _grad(v.class_embedding), self.scratch(((b + 511) // 512) * w), accumulate=True)
        d16 = torch.empty(b * l, w, dtype=dt, device=dev)
        ops.cast16(dt_, d16)
        self._linear_bwd(self.conv, d16, s["patches"], b * l, need_dx=False)                # zero class rows add nothing

    # -- text tower -------------------------------------------------------------------------------
    def text_fwd(self, tokens: torch.Tensor, ctx: Optional[torch.nn.Parameter] = None, l: Optional[int] = None):
        """``l``: the trimmed sequence length (last EOT position + 1 over these prompts) when the caller knows it on the host;
        None reads it back from the device (one synchronisation)."""
        m, dt, dev = self.m, self.dt, self.dev
        tokens = tokens.long()
        n = tokens.shape[0]
        w = m.transformer.width
        eot = torch.empty(n, dtype=torch.int32, device=dev)
        ops.eot_index(tokens, eot)
        if l is None:
            l = int(eot.max().item()) + 1
        x = torch.empty(n * l, w, dtype=torch.float32, device=dev)
        ops.text_embed(tokens, m.token_embedding.weight.data, m.positional_embedding.data, x, l)
        if ctx is not None:
            ops.ctx_splice(x, ctx.data, m.positional_embedding.data, n, l)
        xl, saves = self.blocks_fwd(x, self.tblocks, w // 64, n, l, True)
        f32 = torch.empty(n, w, dtype=torch.float32, device=dev)
        ops.layernorm(xl, m.ln_final.weight.data, m.ln_final.bias.data, f32, rows=n, row_mul=l, row_idx=eot)
        feat = torch.empty(n, m.text_projection.shape[1], dtype=torch.float32, device=dev)
        ops.matmul_f32(f32, m.text_projection.data, feat)
        return feat, dict(tokens=tokens, eot=eot, l=l, n=n, w=w, xl=xl, saves=saves, f32=f32, ctx=ctx)

    def text_bwd(self, dfeat: torch.Tensor, s: dict):
        m, dev = self.m, self.dev
        n, l, w = s["n"], s["l"], s["w"]
        ops.matmul_f32(s["f32"].t(), dfeat, _grad(m.text_projection), accumulate=True)
        df = torch.empty(n, w, dtype=torch.float32, device=dev)
        ops.matmul_f32(dfeat, m.text_projection.data.t(), df)
        dx = torch.zeros(n * l, w, dtype=torch.float32, device=dev)
        scr = self.scratch(ops.layernorm_bwd_scratch(n * l, w))
        ops.layernorm_bwd(df, s["xl"], m.ln_final.weight.data, dx, _grad(m.ln_final.weight), _grad(m.ln_final.bias), scr,
                          rows=n, row_mul=l, row_idx=s["eot"])
        dx = self.blocks_bwd(dx, self.tblocks, s["saves"], w // 64, n, l, True)
        # x[i*l + t] = token_embedding[tok] + positional[t]
        gp = _grad(m.positional_embedding)
        ops.colsum(dx.view(n, l * w), gp.view(-1)[: l * w], self.scratch(((n + 511) // 512) * l * w), accumulate=True)
        if s["ctx"] is not None:                                # CoOp: context gradient; placeholder tokens get none
            ops.ctx_splice_bwd(dx, _grad(s["ctx"]), n, l)
        ops.embed_scatter_add(s["tokens"], dx, _grad(m.token_embedding.weight), l)


class OMTrainer:
    """``train_batch`` of the reference's tree_model on the Engine above."""

    def __init__(self, tree, dtype: str = "bf16"):
        self.tree = tree
        self.engine = Engine(tree.clip_model, dtype)
        # test hook: force the negative-class lists of the inner steps (list of (ids, label_pos)), else sample
        self.contra_override: Optional[Callable[[int], tuple]] = None
        self.last_contra: list = []
        # data-parallel hook: called with "early" once every gradient except the image tower's is final (right before the
        # image tower's backward, model/clip_tree.py:280) and with "late" at the end of the step
        self.grad_ready_hook: Optional[Callable[[str], None]] = None
        # data-parallel process group (None = single process): with a group the step's distinct prompts are SHARDED over the ranks -
        # every rank text-encodes and back-propagates 1 / world of them (see _text_features_dp) instead of all of them
        self.dp_group = None
        self.last_text_rows = 0          # prompts this rank encoded in the last step (tests / accounting)
        # Data-parallel loss head.  False (default): every rank runs the [b_local, <= 257] head of its own image rows and the feature
        # gradient dL/d(text features) is all-reduced - scalable, but its fp32 sum is associated differently from a one-rank run, and a
        # 16-bit backward chain amplifies ANY input difference to its own rounding noise (measured 3 - 4e-3 relative L2 on the text
        # tower's gradients against the one-rank step; round 3's partial-gradient scheme: 1.8e-2).  True (HGR_DP_EXACT_HEAD=1): the
        # normalised image features are all-gathered and every rank runs the head over the WHOLE batch - the same kernels on the same
        # operands in the same order as one rank, so the text tower's backward starts from the same bits (x world, exact) and its
        # gradients equal the one-rank step's up to the fp32 order of the cross-rank sums (<= 1e-4).  The head's FLOPs are then
        # replicated on every rank (B_total x <= 257 x D per inner step, fp32): reproducibility across world sizes, not speed.
        self.dp_exact_head = os.environ.get("HGR_DP_EXACT_HEAD", "0") == "1"
        self._warned_picks = False
        self._pin = {}                   # pinned host staging for the step's index lists, one buffer per use (see _stage_ints)
        self._eot_host = None            # EOT position of every node's prompt (host copy, made once): the trimmed length without a mid-step sync

    def _stage_ints(self, lists, dtype=torch.int32, slot: str = "loc"):
        """The step's host-made index lists on the device through ONE asynchronous copy out of a persistent pinned buffer: a
        `torch.tensor(list, device=...)` per inner step is a synchronous pageable copy, i.e. a drain of the launch queue each time
        (measured on the ViT-L/14 step: ~20 copies, 0.1 - 0.7 ms of idle GPU each, 4.5 ms of a 234 ms step).  Returns one device
        view per list (segments start at multiples of 4 elements).  A `slot` is written once per step, and the step ends in a host
        synchronisation (the loss float), so the previous step's copy out of it has completed before it is overwritten."""
        dev = self.engine.dev
        offs, total = [], 0
        for l in lists:
            offs.append(total)
            total += (len(l) + 3) // 4 * 4
        total = max(total, 4)
        item = torch.empty((), dtype=dtype).element_size()
        pin = self._pin.get(slot)
        if pin is None or pin.numel() < total * item:
            pin = self._pin[slot] = torch.empty(max(total * item, 1 << 16), dtype=torch.uint8, pin_memory=True)
        host = pin[: total * item].view(dtype)
        hn = host.numpy()
        for l, o in zip(lists, offs):
            hn[o: o + len(l)] = l
        devbuf = torch.empty(total, dtype=dtype, device=dev)
        devbuf.copy_(host, non_blocking=True)
        return [devbuf[o: o + len(l)] for l, o in zip(lists, offs)]

    def _head(self, img_n, dimg_n, tfeat, label_pos: int, weight, loss_acc, ce_out=None, replicas: int = 1):
        """logits = img_n tn^T * exp(logit_scale); CE (all rows share the label); gradients of the three inputs.  ``replicas`` > 1
        (exact data-parallel head): img_n holds the rows of ALL ranks and every rank runs this same call, so the per-row weight stays
        that of a rank's own shard (rows / replicas) and the terms every rank would add to a summed gradient carry 1 / replicas."""
        e, m, dev = self.engine, self.engine.m, self.engine.dev
        b, d = img_n.shape
        b = b // replicas                                      # the shard size the 1/b of the mean refers to (gradients are summed over ranks, then x 1/world)
        n = tfeat.shape[0]
        tn = torch.empty_like(tfeat)
        ops.l2norm_rows(tfeat, y32=tn)
        scale = self._scale
        rows = img_n.shape[0]
        logits = torch.empty(rows, n, dtype=torch.float32, device=dev)
        ops.matmul_f32(img_n, tn.t(), logits, alpha=scale)
        labels = torch.full((rows,), label_pos, dtype=torch.int32, device=dev)
        loss_rows = torch.empty(rows, dtype=torch.float32, device=dev)
        dlog = torch.empty_like(logits)
        wv = float(weight)
        ops.ce_rows(logits, labels, loss_rows, dlog, gscale=wv / b)
        ops.matmul_f32(loss_rows.view(1, rows), torch.ones(rows, 1, device=dev), loss_acc, alpha=wv / rows, accumulate=True)   # loss_j = mean * w
        if ce_out is not None:
            ops.matmul_f32(loss_rows.view(1, rows), torch.ones(rows, 1, device=dev), ce_out, alpha=1.0 / rows)
        ops.matmul_f32(dlog, tn, dimg_n, alpha=scale, accumulate=True)                     # d img_n += s * dlog @ tn
        dtn = torch.empty_like(tn)
        ops.matmul_f32(dlog.t(), img_n, dtn, alpha=scale)                                  # d tn = s * dlog^T @ img_n
        # d logit_scale += sum(dlog * logits)   (logits = cos * exp(ls) => d logits / d ls = logits)
        ops.dot_f32(dlog, logits, _grad(m.logit_scale).view(1), alpha=1.0 / replicas, accumulate=True)
        dtfeat = torch.empty_like(tfeat)
        ops.l2norm_bwd(tfeat, dtn, dtfeat)
        return dtfeat

    # -- prompt-parallel text tower (data-parallel training) ---------------------------------------------------------------
    def _trimmed_len(self, ids) -> int:
        """Token count up to and including the last EOT among the prompts `ids` (clip/model.py:350: the EOT token is the row's
        arg-max) from a host copy of the per-node EOT positions, made once - Engine.text_fwd would otherwise read it back from the
        device in the middle of the step, with the image tower's forward still in the queue."""
        nt = self.tree.node_tokens
        if self._eot_host is None or self._eot_host[0] != (nt.data_ptr(), tuple(nt.shape)):
            self._eot_host = ((nt.data_ptr(), tuple(nt.shape)), nt.argmax(dim=-1).cpu().numpy())
        return int(self._eot_host[1][ids].max()) + 1

    def _text_shard(self, n_u: int):
        """Contiguous shard [lo, hi) of the step's n_u distinct prompts for this rank, shard size ns = ceil(n_u / world) (the last
        shards may be short or empty); every rank encodes exactly ns rows so that the all-gather is regular - missing rows are
        filled with the step's first prompt and never receive a gradient."""
        import torch.distributed as dist
        world, rank = dist.get_world_size(self.dp_group), dist.get_rank(self.dp_group)
        ns = -(-n_u // world)
        lo = min(n_u, rank * ns)
        return world, rank, ns, lo, min(n_u, lo + ns)

    def _agree_on_picks(self, picks: list, dp):
        """Data-parallel step: every rank must work on the SAME negatives (one prompt list, sharded over the ranks).  Ranks seeded alike
        (main.run does that) draw the same lists and only pay a 16-byte max-reduce of a hash here; when they differ - a caller that
        did not seed `random`, a loader that advanced it unevenly - the ranks adopt the group's first rank's draw instead of failing
        (round-4 advisor finding: `main` raised at the first step).  The loss weights are functions of the step plan, not of the draw."""
        import hashlib
        import torch.distributed as dist
        mine = [(list(ids), int(pos)) for ids, pos, _, _ in picks]
        hsh = int.from_bytes(hashlib.sha256(repr(mine).encode()).digest()[:7], "little")
        # (max hash, -min hash, max length, -min length) in ONE reduce: every rank - the source rank included - learns whether the
        # draws differ AND whether the plans differ in length, so a length mismatch raises on all ranks together (round-5 advisor
        # finding: only the non-source ranks raised, the source went on into the next collective and hung until the timeout)
        chk = torch.tensor([hsh, -hsh, len(mine), -len(mine)], dtype=torch.int64, device=self.engine.dev)
        dist.all_reduce(chk, op=dist.ReduceOp.MAX, group=dp)
        chk = chk.tolist()
        if chk[2] != -chk[3]:
            raise HgrError("data-parallel OM step: the ranks planned different numbers of inner steps (different target classes?): "
                           "hand every rank its rows of the SAME single-class batch")
        if chk[0] == -chk[1]:
            return picks
        if not self._warned_picks:
            self._warned_picks = True
            import warnings
            warnings.warn("data-parallel OM step: the ranks drew different negative classes (Python `random` is not seeded alike on "
                          "every rank); every rank now takes the first rank's draw each step - seed `random` identically to avoid "
                          "the extra broadcast")
        box = [mine]
        dist.broadcast_object_list(box, src=dist.get_global_rank(dp, 0) if hasattr(dist, "get_global_rank") else 0, group=dp)
        return [(list(ids), int(pos), w, wt) for (ids, pos), (_, _, w, wt) in zip(box[0], picks)]

    def _text_features_dp(self, uniq: list, ctx):
        """The reference text-encodes the <= 257 prompts of every inner step on the device that owns the batch
        (model/clip_tree.py:256-262).  Data-parallel, every rank used to encode - and back-propagate - ALL distinct prompts of the
        step: at ViT-L/14 + CoOp that is ~25 % of a rank's FLOPs, replicated world times.  Here rank r encodes the prompts
        uniq[lo:hi) only and the [n_u, D] features are all-gathered (fp32, a few MB); see _text_backward_dp for the way back."""
        import torch.distributed as dist
        tree, e = self.tree, self.engine
        world, rank, ns, lo, hi = self._text_shard(len(uniq))
        # the sharding is only meaningful when every rank works on the SAME prompt list (same single-class batch, same sampling seed:
        # SURVEY H7, dataset/imagenet_group.py shard="within"); a rank that drew other negatives would gather garbage or hang in a
        # mis-sized collective, so the list's hash is compared first (one 16-byte max-reduce; the step synchronises with the host
        # for logit_scale and the EOT length anyway)
        import hashlib
        hsh = int.from_bytes(hashlib.sha256(repr(uniq).encode()).digest()[:7], "little")
        chk = torch.tensor([hsh, -hsh], dtype=torch.int64, device=e.dev)
        dist.all_reduce(chk, op=dist.ReduceOp.MAX, group=self.dp_group)
        chk = chk.tolist()
        if chk[0] != -chk[1]:
            raise HgrError("data-parallel OM step: the ranks drew different negative classes (seed `random` identically on every rank and "
                           "hand every rank its rows of the SAME single-class batch); prompt-parallel text encoding needs one prompt list")
        mine = uniq[lo:hi] + [uniq[0]] * (ns - (hi - lo))
        feat_l, tsave = e.text_fwd(tree.node_tokens[self._stage_ints([mine], torch.int64, "uniq")[0]], ctx, l=self._trimmed_len(mine))
        self.last_text_rows = ns
        full = torch.empty(world, ns, feat_l.shape[1], dtype=torch.float32, device=e.dev)
        dist.all_gather(list(full.unbind(0)), feat_l.contiguous(), group=self.dp_group)
        # rank r's block starts at row r * ns = the index of its first prompt, and padding rows exist at the tail only: the first
        # n_u rows of the gathered buffer ARE the features in `uniq` order
        return full.view(world * ns, -1)[: len(uniq)], tsave

    def _text_backward_dp(self, dtfeat_u: torch.Tensor, tsave: dict, n_u: int, reduce: bool = True):
        """dL/d(text features) is a sum over the images of the WHOLE batch: all-reduce it (sum; [n_u, D] fp32) BEFORE the text
        tower's backward, then every rank back-propagates its own prompts' rows only.  The parameter gradients a rank gets are the
        full-batch gradients of its prompts; the bucketed gradient all-reduce that follows sums them over the prompt shards, exactly
        as it sums the image tower's over the image shards.  Compared with back-propagating each rank's PARTIAL feature gradient
        through the 16-bit backward chain (round 3: 1.8e-2 relative L2 against the one-rank step) the text-tower gradients now
        differ from the one-rank step's by fp32 summation order only."""
        import torch.distributed as dist
        e = self.engine
        world, rank, ns, lo, hi = self._text_shard(n_u)
        if reduce:                     # (exact head: every rank already holds the whole batch's feature gradient)
            dist.all_reduce(dtfeat_u, op=dist.ReduceOp.SUM, group=self.dp_group)
        mine = torch.zeros(ns, dtfeat_u.shape[1], dtype=torch.float32, device=e.dev)
        if hi > lo:
            mine[: hi - lo] = dtfeat_u[lo:hi]
        e.text_bwd(mine, tsave)

    @torch.no_grad()
    def train_batch(self, inputs, targets, training_method: str = "OM", sample_strategy: Optional[str] = None) -> float:
        tree, e = self.tree, self.engine
        if not inputs.is_cuda:
            raise HgrError("train_batch needs device tensors: there is no CPU path")
        strategy = sample_strategy or tree.opts.sample_strategy
        # every host read-back of the step happens HERE, before the image tower is queued: behind it the host would wait for the tower's
        # forward and the device would then idle through the host-side sampling below
        target = int(targets[0].item()) if torch.is_tensor(targets) else int(targets[0])
        self._scale = float(e.m.logit_scale.data.exp())      # one scalar D2H per step
        lw_host = tree.layer_weight.detach().float().cpu() if tree.opts.weights == "adaptive" else None
        e.prepare()
        feat, isave = e.image_fwd(inputs)
        img_n = torch.empty_like(feat)
        ops.l2norm_rows(feat, y32=img_n)
        dimg_n = torch.zeros_like(img_n)                      # img_feats_.grad of the reference
        loss_acc = torch.zeros(1, 1, dtype=torch.float32, device=e.dev)
        if training_method == "OM":
            steps = tree.outer_inner_plan(target)
        elif training_method == "hierarchical":               # clip_tree.py:283-316
            parents = list(tree.c2p[target]) + [target]
            steps = [dict(p_out=target, depth=j, parents_in=parents, k_loop=j, m_loop=0, K=len(parents), M=1, hier=True) for j in range(len(parents))]
        else:
            raise NotImplementedError(f"training_method {training_method!r} (the reference implements 'OM' and 'hierarchical' only)")
        # negative sampling first (host), then ONE text-tower pass over the de-duplicated prompts of all inner steps:
        # the weights are constant within a step, so encoding each distinct prompt once and back-propagating the summed
        # feature gradient once is the same arithmetic as the reference's K x M separate encode_text + backward calls
        # the scalar loss weights as HOST values: the closed forms are made on the CPU, `adaptive` from one read-back of layer_weight
        # (its gradient path below stays on the device) - a device tensor + float() per inner step drained the launch queue 3 x 17 times
        def host_weights(mode, n):
            if mode == "adaptive":
                return torch.softmax(100 ** lw_host[:n], dim=0)
            return tree.get_weights(mode, n, device="cpu")

        picks = []
        for i, st in enumerate(steps):
            if self.contra_override is not None:
                ids, pos = self.contra_override(i)
            else:
                ids, pos = tree.get_contra_ids(strategy, st["p_out"], st["depth"], st["parents_in"])
            if st.get("hier"):
                wgt = host_weights(tree.opts.weights, st["K"])[st["k_loop"]]
            else:
                wmode = tree.opts.weighting
                w_in = host_weights("equal" if wmode == "out" else tree.opts.weights, st["M"])
                w_out = host_weights("equal" if wmode == "in" else tree.opts.weights, st["K"])
                wgt = w_in[st["m_loop"]] * w_out[st["k_loop"]]
            picks.append((list(ids), pos, float(wgt), wgt))
        dp = self.dp_group if self.dp_group is not None else getattr(tree, "_dp_group", None)
        self.dp_group = dp
        if dp is not None:
            picks = self._agree_on_picks(picks, dp)
        check_distinct_ids([ids for ids, _, _, _ in picks])    # before the text tower and the gather / scatter loop below
        self.last_contra = [(ids, pos) for ids, pos, _, _ in picks]
        uniq = sorted({i for ids, _, _, _ in picks for i in ids})
        where = {nid: j for j, nid in enumerate(uniq)}
        if dp is not None:
            tfeat_u, tsave = self._text_features_dp(uniq, getattr(tree, "ctx", None))
        else:
            tfeat_u, tsave = e.text_fwd(tree.node_tokens[self._stage_ints([uniq], torch.int64, "uniq")[0]], getattr(tree, "ctx", None),
                                        l=self._trimmed_len(uniq))
            self.last_text_rows = len(uniq)
        dtfeat_u = torch.zeros_like(tfeat_u)
        exact = dp is not None and self.dp_exact_head
        img_h, dimg_h, replicas = img_n, dimg_n, 1
        if exact:
            # every rank runs the head over the rows of ALL ranks (rank-major: the one-rank run's row order)
            import torch.distributed as dist
            replicas, rnk = dist.get_world_size(dp), dist.get_rank(dp)
            img_h = torch.empty(replicas, img_n.shape[0], img_n.shape[1], dtype=torch.float32, device=e.dev)
            dist.all_gather(list(img_h.unbind(0)), img_n.contiguous(), group=dp)
            img_h = img_h.view(replicas * img_n.shape[0], -1)
            dimg_h = torch.zeros_like(img_h)
        adaptive = tree.opts.weights == "adaptive"
        ces = torch.zeros(len(picks), 1, dtype=torch.float32, device=e.dev) if adaptive else None
        locs = self._stage_ints([[where[i] for i in ids] for ids, _, _, _ in picks])
        for j, (ids, pos, wgt, _) in enumerate(picks):
            loc = locs[j]
            tfeat = torch.empty(len(ids), tfeat_u.shape[1], dtype=torch.float32, device=e.dev)
            ops.rows_gather(tfeat_u, loc, tfeat)
            dtfeat = self._head(img_h, dimg_h, tfeat, pos, wgt, loss_acc, ces[j: j + 1] if adaptive else None, replicas)
            ops.rows_axpy(dtfeat_u, dtfeat, dst_mul=0, dst_idx=loc)
        if exact:
            dimg_n.copy_(dimg_h.view(replicas, -1, dimg_h.shape[1])[rnk])          # this rank's rows of the whole-batch image-side gradient
        if dp is not None:
            self._text_backward_dp(dtfeat_u, tsave, len(uniq), reduce=not exact)
        else:
            e.text_bwd(dtfeat_u, tsave)
        if adaptive:
            # loss = sum_j CE_j * w_j(layer_weight): the <= 13-element softmax(100 ** layer_weight) of get_weights is host-level
            # glue in the reference too (clip_tree.py:209); its gradient comes from autograd over those tiny tensors
            with torch.enable_grad():
                ws = []
                for st in steps:
                    if st.get("hier"):
                        ws.append(tree.get_weights("adaptive", st["K"])[st["k_loop"]])
                    else:
                        wmode = tree.opts.weighting
                        w_in = tree.get_weights("equal" if wmode == "out" else "adaptive", st["M"])
                        w_out = tree.get_weights("equal" if wmode == "in" else "adaptive", st["K"])
                        ws.append(w_in[st["m_loop"]] * w_out[st["k_loop"]])
                (torch.stack(ws) * ces.view(-1)).sum().backward()
        if self.grad_ready_hook is not None:
            self.grad_ready_hook("early")
        dfeat = torch.empty_like(feat)
        ops.l2norm_bwd(feat, dimg_n, dfeat)
        e.image_bwd(dfeat, isave)
        if self.grad_ready_hook is not None:
            self.grad_ready_hook("late")
        return float(loss_acc.item())


class FusedAdamW:
    """clip_grad_norm_(params, max_norm) + AdamW.step() of main.py:87-91 as fused kernels on fp32 masters.

    The parameters and their gradients are re-laid out as views into TWO flat fp32 buffers (256-byte aligned
    slots), so that one step is ONE `hgr_sumsq` + ONE `hgr_adamw` launch over everything (the clip factor is
    read from device memory: no host synchronisation), `zero_grad` is one memset and the data-parallel
    gradient all-reduce runs directly on bucket-sized views of the flat gradient buffer, without packing."""

    def __init__(self, params, lr: float = 3e-7, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_norm: Optional[float] = 1.0):
        self.params = [p for p in params]
        self.param_groups = [dict(lr=lr, params=self.params)]       # so the reference's cosine_lr scheduler can drive it (utils.py:82-95)
        self.betas, self.eps, self.wd, self.max_norm = betas, eps, weight_decay, max_norm
        self.step_count = 0
        dev = self.params[0].device
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.gflat = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, offs):
            n = p.numel()
            self.flat[off: off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off: off + n].view(p.data.shape)
            g = self.gflat[off: off + n].view(p.data.shape)
            if p.grad is not None:
                g.copy_(p.grad)
            p.grad = g
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self._tot = torch.zeros(1, dtype=torch.float32, device=dev)
        self.grad_scale = 1.0

    def _relink(self):
        """A caller may have dropped gradients (`p.grad = None`): point them back at the flat buffer."""
        off = 0
        for p in self.params:
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.gflat[off: off + n].data_ptr():
                g = self.gflat[off: off + n].view(p.data.shape)
                if p.grad is not None:
                    g.copy_(p.grad)
                else:
                    g.zero_()
                p.grad = g
            off += (n + 63) // 64 * 64

    def set_late_params(self, late_params) -> None:
        """Mark the parameters whose gradients become final LAST in a step (the image tower: the reference's single
        image-tower backward is the last thing train_batch does, model/clip_tree.py:280).  Everything else - text tower,
        projections, logit_scale, CoOp context - is final before that backward starts, so its buckets can be all-reduced
        while the image tower is still back-propagating (`allreduce_part`)."""
        late = {id(p) for p in late_params}
        early, lateb = [], []
        off = 0
        for p in self.params:
            n = (p.numel() + 63) // 64 * 64
            dst = lateb if id(p) in late else early
            if dst and dst[-1][1] == off:
                dst[-1][1] = off + n
            else:
                dst.append([off, off + n])
            off += n
        self._ranges = {"early": [tuple(r) for r in early], "late": [tuple(r) for r in lateb]}
        self._works = []

    def allreduce_part(self, part: str, group=None, bucket_bytes: int = 64 << 20) -> None:
        """Overlapped gradient all-reduce: `part` = "early" right after the text tower's backward (asynchronous: the
        collectives run on the communicator's stream beside the image tower's backward kernels), then "late" after the
        image tower's backward, which also waits for everything.  Same result as `allreduce` (sum, 1/world folded into the
        next step's grad_scale); bucketed views of the flat buffer, no packing."""
        import torch.distributed as dist
        if not hasattr(self, "_ranges"):
            raise HgrError("FusedAdamW.allreduce_part: call set_late_params(image-tower parameters) first")
        if part == "early":
            self._relink()
        step = max(1, bucket_bytes // 4)
        for lo, hi in self._ranges[part]:
            for b in range(lo, hi, step):
                self._works.append(dist.all_reduce(self.gflat[b: min(hi, b + step)], op=dist.ReduceOp.SUM, group=group, async_op=True))
        if part == "late":
            for w in self._works:
                w.wait()
            self._works = []
            self.grad_scale = 1.0 / dist.get_world_size(group)

    def allreduce(self, group=None, bucket_bytes: int = 64 << 20):
        """Sum the flat gradient buffer over the ranks, bucket by bucket (RCCL all-reduce on views, no packing);
        the 1/world average is folded into the next step's `grad_scale`."""
        import torch.distributed as dist
        self._relink()
        step = max(1, bucket_bytes // 4)
        from .parallel import native_comm
        nc = native_comm()
        for lo in range(0, self.gflat.numel(), step):
            if nc is not None:
                nc.allreduce(self.gflat[lo: lo + step])                      # hgr_allreduce: RCCL through the C ABI, current stream
            else:
                dist.all_reduce(self.gflat[lo: lo + step], op=dist.ReduceOp.SUM, group=group)
        self.grad_scale = 1.0 / dist.get_world_size(group)

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        self._relink()
        lr = self.param_groups[0]["lr"]
        tot = None
        if self.max_norm is not None:
            tot = self._tot
            tot.zero_()
            ops.sumsq(self.gflat, tot)
        ops.adamw(self.flat, self.gflat, self.m, self.v, lr, self.step_count, self.betas, self.eps, self.wd, tot, self.max_norm or 0.0, self.grad_scale)
        self.grad_scale = 1.0

    def zero_grad(self):
        self._relink()
        self.gflat.zero_()
