"""CNZSL baseline on MI355X: the class-normalised prototype network of baseline/CNZSL/cnzsl.py - `CNZSLModel` with the reference's
parameter names and `state_dict` schema ('model.0.weight', ..., 'model.3.running_mean', ..., 'model.6.bias'), its training step and
its evaluation loop, on cached image features.

The model is attribute -> prototype: Linear, ReLU, Linear, ClassStandardization, ReLU, ClassStandardization, Linear, ReLU, and
logits = (5 x / |x|) (5 protos / |protos|)^T = 25 cos(feature, prototype).  Reference quirks, kept:

  * ClassStandardization divides by the VARIANCE plus 1e-5, not by a standard deviation; the variance is the unbiased one over the
    class dimension; training updates running <- 0.9 running + 0.1 batch; evaluation uses the running vectors.
  * `test()` takes the top-1 of `hit_ratio` and the per-level picks over the TEST classes (main.test takes them over the train
    classes); the -1 fill of the off-level columns competes there as well.
  * The running vectors are non-trainable parameters, so they travel in the state_dict and Adam never sees them.

On the device a forward is three fp32 products (`hgr_matmul_f32`), `hgr_bias_relu_f32` behind the outer two, and ONE launch of
`hgr_cnzsl_std_chain_fwd` for everything between the second product and the third.  `CNZSLModel.forward` is inference only;
training goes through `CNZSLTrainer` (closed-form backward, `hgr_adam_l2`), scoring through `CNZSLEvaluator` (`hgr_eval_rows` with
both of its subsets set to the test classes, then the counters of the main evaluation).  No atomics anywhere: a step repeated from
the same state gives bit-equal parameters.  `prototypes_host`, `train_step_host` and `score_host` are the plain torch / numpy twins
the device route is tested against.  `python -m hgr_net_amd.baseline.train_cnzsl` is the reference script's command line.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from .. import ops
from ._shared import K_SLICE, AdamL2State, BufferPool, TreeScorer, mean_rows, metric_string, need_device, sliced_matmul_f32  # noqa: F401
from .dgp_eval import ListTree, build_list_tree

EPS, MOMENTUM, SCALE = ops.CN_EPS, ops.CN_MOMENTUM, 5.0
TOP = (1, 2, 5, 10, 20)                        # dgp_eval.TOP: what _shared.TreeScorer and metric_string count
TRAINABLE = ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.6.weight", "model.6.bias")
RUNNING = ("model.3.running_mean", "model.3.running_var", "model.5.running_mean", "model.5.running_var")


def cosine_logits(xn: torch.Tensor, pn: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = 25 xn pn^T for row-normalised operands, accumulated over slices of K_SLICE columns (_shared.sliced_matmul_f32)."""
    return sliced_matmul_f32(xn, pn, out, alpha=SCALE * SCALE)


class ClassStandardization(nn.Module):
    """The holder of one layer's running statistics (cnzsl.py:139-173): non-trainable parameters, as in the reference.  The
    arithmetic lives in `hgr_cnzsl_std_chain_fwd`, which runs both layers and the ReLU between them."""

    def __init__(self, feat_dim: int):
        super().__init__()
        self.running_mean = nn.Parameter(torch.zeros(feat_dim), requires_grad=False)
        self.running_var = nn.Parameter(torch.ones(feat_dim), requires_grad=False)

    def forward(self, class_feats):
        raise NotImplementedError("ClassStandardization runs inside hgr_cnzsl_std_chain_fwd: call CNZSLModel.prototypes / CNZSLTrainer")


class CNZSLModel(nn.Module):
    """cnzsl.py:191-219.  `cn=False` / `init=False` are the reference's `--cn False` / `--init False`."""

    def __init__(self, attr_dim: int, hid_dim: int, proto_dim: int, cn: bool = True, init: bool = True, device="cuda"):
        super().__init__()
        if hid_dim % 4 or proto_dim % 4:
            raise ValueError(f"hid_dim={hid_dim} and proto_dim={proto_dim} must be multiples of 4")
        self.attr_dim, self.hid_dim, self.proto_dim, self.cn = attr_dim, hid_dim, proto_dim, bool(cn)
        self.model = nn.Sequential(
            nn.Linear(attr_dim, hid_dim), nn.ReLU(),
            nn.Linear(hid_dim, hid_dim), ClassStandardization(hid_dim) if cn else nn.Identity(), nn.ReLU(),
            ClassStandardization(hid_dim) if cn else nn.Identity(), nn.Linear(hid_dim, proto_dim), nn.ReLU())
        if init:
            b = math.sqrt(3.0 / (hid_dim * proto_dim))
            self.model[-2].weight.data.uniform_(-b, b)
        self.to(device)
        self._pool = BufferPool(self.model[0].weight)

    def running(self):
        m = self.model
        return (m[3].running_mean.data, m[3].running_var.data, m[5].running_mean.data, m[5].running_var.data)

    def _check(self, t: torch.Tensor, width: int, what: str) -> torch.Tensor:
        need_device(t, "CNZSLModel", what)
        if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
            raise ValueError(f"{what} must be [rows, {width}], got {tuple(t.shape)}")
        return t.float().contiguous()

    def _run(self, attrs: torch.Tensor, train: bool, buf) -> Dict[str, torch.Tensor]:
        """The prototype network on `attrs` [S, A]; every intermediate the backward needs, in buffers of `buf`."""
        m, s, h, p = self.model, attrs.shape[0], self.hid_dim, self.proto_dim
        h1 = ops.matmul_f32(attrs, m[0].weight.data.t(), buf("h1", (s, h)))
        ops.bias_relu_f32(h1, m[0].bias.data)
        z = ops.matmul_f32(h1, m[2].weight.data.t(), buf("z", (s, h)))
        out = {"h1": h1, "z": z}
        if self.cn:
            out["c"], out["a"], out["stats"] = buf("c", (s, h)), buf("a", (s, h)), buf("stats", (4, h))
            ops.cnzsl_std_chain_fwd(z, m[2].bias.data, self.running(), out["c"], out["a"] if train else None,
                                    out["stats"] if train else None, train=train)
        else:
            out["c"] = ops.bias_relu_f32(z, m[2].bias.data, buf("c", (s, h)))
        out["p"] = ops.matmul_f32(out["c"], m[6].weight.data.t(), buf("p", (s, p)))
        ops.bias_relu_f32(out["p"], m[6].bias.data)
        return out

    @torch.no_grad()
    def prototypes(self, attrs: torch.Tensor) -> torch.Tensor:
        """`self.model(attrs)` in eval mode: [N, proto_dim], a buffer the next call of this size overwrites."""
        return self._run(self._check(attrs, self.attr_dim, "attrs"), False, self._pool.pool)["p"]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, attrs: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise NotImplementedError("training mode: CNZSLModel.forward is inference only (model.eval()); train with CNZSLTrainer")
        x = self._check(x, self.proto_dim, "x")
        p = self.prototypes(attrs)
        pn, xn = self._pool.pool("pn", p.shape), self._pool.pool("xn", x.shape)
        ops.l2norm_rows(p, y32=pn)
        ops.l2norm_rows(x, y32=xn)
        logits = torch.empty((x.shape[0], p.shape[0]), dtype=torch.float32, device=x.device)
        return cosine_logits(xn, pn, logits)


class CNZSLTrainer:
    """cnzsl.py:323-337 and :358-359 on cached features: cross-entropy (mean over the batch) of 25 cos(feature, prototype) against
    the seen classes, `Adam(lr, weight_decay)` with coupled decay on the six trainable tensors, `StepLR(step_size, gamma)` ticked
    by `epoch_end()`.  One step: three products, the chain kernel, `l2norm_rows` on both sides, the logits product, `ce_rows`,
    the mirrored backward and `adam_l2` per tensor; nothing in it synchronises with the host, every buffer is kept."""

    def __init__(self, model: CNZSLModel, lr: float = 1e-4, weight_decay: float = 1e-4, step_size: int = 25, gamma: float = 0.1,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        self.model, self.lr0, self.wd, self.step_size, self.gamma, self.betas, self.eps = model, lr, weight_decay, int(step_size), gamma, betas, eps
        self.epoch = 0
        sd = dict(model.named_parameters())
        self.opt = AdamL2State({k: sd[k] for k in TRAINABLE}, betas, eps, weight_decay, "CNZSLTrainer")
        self.params, self.m, self.v, self.g = self.opt.params, self.opt.m, self.opt.v, self.opt.g
        self._pool = BufferPool(self.params[TRAINABLE[0]])
        self._buf = self._pool.pool

    @property
    def t(self) -> int:
        return self.opt.t

    @property
    def lr(self) -> float:
        return self.lr0 * self.gamma ** (self.epoch // self.step_size)

    def epoch_end(self) -> None:
        self.epoch += 1

    def _scratch(self, rows: int, cols: int) -> torch.Tensor:
        return self._buf("scratch", (max(1, -(-rows // ops.RELU_BWD_CHUNK)) * cols,))

    @torch.no_grad()
    def _forward_backward(self, feats, labels, attrs_seen) -> torch.Tensor:
        md, m = self.model, self.model.model
        x = md._check(feats, md.proto_dim, "feats")
        attrs = md._check(attrs_seen, md.attr_dim, "attrs_seen")
        if not (torch.is_tensor(labels) and labels.is_cuda and labels.numel() == x.shape[0]):
            raise RuntimeError("CNZSLTrainer needs the labels as a device tensor, one per feature row")
        lab = labels.reshape(-1).to(torch.int32)
        bsz, s, h, p = x.shape[0], attrs.shape[0], md.hid_dim, md.proto_dim
        f = md._run(attrs, True, self._buf)
        pn, xn = self._buf("pn", (s, p)), self._buf("xn", (bsz, p))
        ops.l2norm_rows(f["p"], y32=pn)
        ops.l2norm_rows(x, y32=xn)
        logits = cosine_logits(xn, pn, self._buf("logits", (bsz, s)))
        loss_rows, dlogits = self._buf("loss_rows", (bsz,)), self._buf("dlogits", (bsz, s))
        ops.ce_rows(logits, lab, loss_rows, dlogits, gscale=1.0 / bsz)
        loss = mean_rows(self._pool, loss_rows, self._buf("loss", (1,)))
        # backward: logits = 25 xn pn^T -> dpn; the row normalisation; ReLU + bias of module 6/7; the chain; ReLU + bias of module 0/1
        g = self.g
        dpn = ops.matmul_f32(dlogits.t(), xn, self._buf("dpn", (s, p)), alpha=SCALE * SCALE)
        dp = ops.l2norm_bwd(f["p"], dpn, self._buf("dp", (s, p)))
        ops.relu_bwd_colsum_f32(dp, f["p"], dp, g["model.6.bias"], self._scratch(s, max(p, h)))
        ops.matmul_f32(dp.t(), f["c"], g["model.6.weight"])
        dc = ops.matmul_f32(dp, m[6].weight.data, self._buf("dc", (s, h)))
        dz = self._buf("dz", (s, h))
        if md.cn:
            ops.cnzsl_std_chain_bwd(dc, f["a"], f["z"], m[2].bias.data, f["stats"], dz, g["model.2.bias"])
        else:
            ops.relu_bwd_colsum_f32(dc, f["c"], dz, g["model.2.bias"], self._scratch(s, max(p, h)))
        ops.matmul_f32(dz.t(), f["h1"], g["model.2.weight"])
        dh1 = ops.matmul_f32(dz, m[2].weight.data, self._buf("dh1", (s, h)))
        ops.relu_bwd_colsum_f32(dh1, f["h1"], dh1, g["model.0.bias"], self._scratch(s, max(p, h)))
        ops.matmul_f32(dh1.t(), attrs, g["model.0.weight"])
        self.logits = logits
        return loss

    def _running_snapshot(self):
        return [r.clone() for r in self.model.running()] if self.model.cn else None

    def grads(self, feats, labels, attrs_seen) -> dict:
        """Gradients of the training loss by state-dict name; no optimiser step, and the running vectors are put back."""
        keep = self._running_snapshot()
        self._forward_backward(feats, labels, attrs_seen)
        if keep is not None:
            for r, k in zip(self.model.running(), keep):
                r.copy_(k)
        return {k: v.clone() for k, v in self.g.items()}

    def step(self, feats, labels, attrs_seen) -> torch.Tensor:
        """One iteration of the reference's `train()`; returns the loss as a 0-dim device tensor."""
        loss = self._forward_backward(feats, labels, attrs_seen).clone().reshape(())
        self.opt.step(self.lr)
        return loss


# ---- scoring (cnzsl.py:221-321) ----------------------------------------------------------------------------------------------------------
def score_host(logits, targets, tree: ListTree, test_index) -> dict:
    """One batch of `test()` in numpy from its logits [b, >= N]: {'pred' [b, 20] the top-20 test classes, 'top1' [b] the best test
    class, 'lv' [b, n_levels] per depth level the best test class with every off-level column reading -1, 'acc' float64 [9] the
    batch's counters}.  `targets`: one node index, or one per row.  The lowest position of `test_index` wins a tie."""
    v = np.asarray(logits, dtype=np.float32)
    te = np.asarray(test_index, dtype=np.int64).reshape(-1)
    n = len(tree.nodes)
    if v.ndim != 2 or v.shape[1] < n or np.isnan(v[:, :n]).any():
        raise ValueError("logits must be [rows, >= nodes] without NaN")
    b = v.shape[0]
    tg = np.full(b, int(targets), dtype=np.int64) if np.ndim(targets) == 0 else np.asarray(targets, dtype=np.int64).reshape(-1)
    sub = v[:, te]
    pred = te[np.argsort(-sub, axis=1, kind="stable")[:, :max(TOP)]]
    top1 = te[sub.argmax(1)]
    lv = np.empty((b, tree.n_levels), dtype=np.int64)
    lev = tree.depth[te]
    for l in range(tree.n_levels):
        lv[:, l] = te[np.where(lev[None, :] == l, sub, np.float32(-1.0)).argmax(1)]
    acc = np.zeros(9, dtype=np.float64)
    for r in range(b):
        path = tree.path(int(tg[r]))
        L = len(path)
        for i, k in enumerate(TOP):
            acc[i] += int((pred[r, :k] == tg[r]).sum())
        mt = [int(lv[r, tree.depth[q]]) == q for q in path]
        acc[5] += sum(int(top1[r]) == q for q in path)
        acc[6] += float(mt[0]) if L == 1 else sum(x and y for x, y in zip(mt[:-1], mt[1:])) / (L - 1)
        acc[7] += sum(mt) / L
        acc[8] += 1
    return {"pred": pred.astype(np.int32), "top1": top1.astype(np.int32), "lv": lv.astype(np.int32), "acc": acc}


class CNZSLEvaluator(TreeScorer):
    """`test()` on cached features: `nodes` the ordered node list (seen classes first), `test_index` the candidate classes,
    `attrs` [N, A] on the device.  The prototypes of all nodes are computed and normalised once; a batch is one product, one
    `hgr_eval_rows` launch and the counters (_shared.TreeScorer: `add`, `add_rows`, `counters`, `result`)."""

    def __init__(self, graph_edges, nodes: Sequence[str], test_index, model: CNZSLModel, attrs: torch.Tensor, tree: Optional[ListTree] = None):
        super().__init__(tree if tree is not None else build_list_tree(graph_edges, nodes), test_index, attrs.device)
        if attrs.shape[0] != self.n:
            raise ValueError(f"attrs has {attrs.shape[0]} rows for {self.n} nodes")
        was_training = model.training
        p = model.eval().prototypes(attrs)
        model.train(was_training)
        self.device, self.k = p.device, p.shape[1]
        self.pn = torch.empty_like(p)
        ops.l2norm_rows(p, y32=self.pn)
        self._cap, self._buf = 0, None

    def logits(self, feats: torch.Tensor) -> torch.Tensor:
        """25 cos(feature, prototype) of one batch, [B, N]: a view of a buffer the next batch overwrites."""
        if not (torch.is_tensor(feats) and feats.is_cuda and feats.dim() == 2 and feats.shape[1] == self.k and feats.shape[0] >= 1):
            raise ops._lib.HgrError(f"features must be a device tensor [B, {self.k}] (no CPU path)")
        x = feats.float().contiguous()
        b = x.shape[0]
        if self._cap < b:
            self._buf = (torch.empty((b, self.k), dtype=torch.float32, device=self.device), torch.empty((b, self.n), dtype=torch.float32, device=self.device))
            self._cap = b
        xn, out = self._buf[0][:b], self._buf[1][:b]
        ops.l2norm_rows(x, y32=xn)
        return cosine_logits(xn, self.pn, out)

    scores = logits


# ---- host twins: plain torch, any floating type --------------------------------------------------------------------------------------------
def std_chain_host(z: torch.Tensor, bias: torch.Tensor, running=None, train: bool = True, eps: float = EPS, momentum: float = MOMENTUM):
    """What `hgr_cnzsl_std_chain_fwd` computes, in torch (differentiable): (c, a, stats [4, H], the updated running vectors or
    None).  Training uses the batch statistics, evaluation `running` = (mean1, var1, mean2, var2)."""
    u = z + bias
    m1, v1 = (u.mean(0), u.var(0)) if train else (running[0], running[1])
    a = torch.relu((u - m1) / (v1 + eps))
    m2, v2 = (a.mean(0), a.var(0)) if train else (running[2], running[3])
    c = (a - m2) / (v2 + eps)
    stats = torch.stack([m1, v1, m2, v2])
    new = None
    if train and running is not None:
        new = tuple((1.0 - momentum) * r + momentum * s.detach() for r, s in zip(running, (m1, v1, m2, v2)))
    return c, a, stats, new


def _running_of(sd, dtype):
    return tuple(torch.as_tensor(sd[k]).to(dtype) for k in RUNNING)


def prototypes_host(sd: dict, attrs, cn: bool = True, train: bool = False, dtype=torch.float32, tap: Optional[dict] = None):
    """`CNZSLModel.model(attrs)` from a state dict (tensors or arrays), on the CPU in `dtype`.  Evaluation returns the prototypes;
    training returns (prototypes, updated running vectors) and keeps the graph of tensors that require gradients.  `tap`, if
    given, receives z = h1 W2^T (the chain kernel's input)."""
    w = {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(attrs).to(dtype)
    h1 = torch.relu(x @ w["model.0.weight"].t() + w["model.0.bias"])
    z = h1 @ w["model.2.weight"].t()
    if tap is not None:
        tap["z"] = z
    new = None
    if cn:
        c, _, _, new = std_chain_host(z, w["model.2.bias"], _running_of(w, dtype), train)
    else:
        c = torch.relu(z + w["model.2.bias"])
    p = torch.relu(c @ w["model.6.weight"].t() + w["model.6.bias"])
    return (p, new) if train else p


def logits_host(protos: torch.Tensor, x) -> torch.Tensor:
    x = torch.as_tensor(x).to(protos.dtype)
    return (SCALE * x / x.norm(dim=1, keepdim=True)) @ (SCALE * protos / protos.norm(dim=1, keepdim=True)).t()


def train_state_host(sd: dict, dtype=torch.float32) -> dict:
    """The state `train_step_host` advances: parameters, Adam moments and the step count."""
    sd = {k: torch.as_tensor(np.asarray(v.detach().cpu()) if torch.is_tensor(v) else np.asarray(v)).to(dtype).clone() for k, v in sd.items()}
    tr = [k for k in TRAINABLE if k in sd]
    return {"sd": sd, "m": {k: torch.zeros_like(sd[k]) for k in tr}, "v": {k: torch.zeros_like(sd[k]) for k in tr}, "t": 0}


def train_step_host(state: dict, feats, labels, attrs_seen, cn: bool = True, lr: float = 1e-4, weight_decay: float = 1e-4,
                    betas=(0.9, 0.999), eps: float = 1e-8, update: bool = True):
    """One iteration of `train()` on the CPU in the state's dtype: forward in training mode, mean cross-entropy, autograd,
    torch.optim.Adam's arithmetic with coupled decay.  Returns (loss, gradients by name, logits); with `update` the state moves on
    (parameters, moments, running vectors)."""
    sd = state["sd"]
    dtype = sd["model.0.weight"].dtype
    leaf = {k: sd[k].clone().requires_grad_(True) for k in TRAINABLE}
    full = dict(sd)
    full.update(leaf)
    tap = {}
    protos, new = prototypes_host(full, attrs_seen, cn, True, dtype, tap)
    logits = logits_host(protos, feats)
    loss = torch.nn.functional.cross_entropy(logits, torch.as_tensor(labels).long().reshape(-1))
    *gl, dz = torch.autograd.grad(loss, [leaf[k] for k in TRAINABLE] + [tap["z"]])
    grads = dict(zip(TRAINABLE, gl))
    state["absdz"] = float(dz.abs().sum(0).max())        # what the bias gradient of module 2 is a cancelling sum of
    if update:
        state["t"] += 1
        t = state["t"]
        with torch.no_grad():
            for k in TRAINABLE:
                g = grads[k] + weight_decay * sd[k]
                state["m"][k] = betas[0] * state["m"][k] + (1 - betas[0]) * g
                state["v"][k] = betas[1] * state["v"][k] + (1 - betas[1]) * g * g
                denom = state["v"][k].sqrt() / math.sqrt(1 - betas[1] ** t) + eps
                sd[k] = sd[k] - (lr / (1 - betas[0] ** t)) * state["m"][k] / denom
            if cn:
                for k, r in zip(RUNNING, new):
                    sd[k] = r.detach()
    return loss.detach(), {k: g.detach() for k, g in grads.items()}, logits.detach()


# ---- synthetic material (hgr_net_amd.synth: a pure function of the seed) -----------------------------------------------------------------
def synth_state(seed: int, attr_dim: int, hid_dim: int, proto_dim: int, cn: bool = True, running: bool = False) -> Dict[str, np.ndarray]:
    """A state dict of fp32 arrays: fan-in scaled normal weights, the reference's `--init True` range for the last layer, POSITIVE
    last-layer biases (few dead prototype columns), and with `running` non-trivial running vectors instead of (0, 1)."""
    from .. import synth
    f32 = lambda a, *shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape).astype(np.float32))
    b = math.sqrt(3.0 / (hid_dim * proto_dim))
    sd = {"model.0.weight": f32(synth.normal(seed, "cnzsl.w0", hid_dim * attr_dim) / math.sqrt(attr_dim), hid_dim, attr_dim),
          "model.0.bias": f32(0.1 * synth.normal(seed, "cnzsl.b0", hid_dim), hid_dim),
          "model.2.weight": f32(synth.normal(seed, "cnzsl.w2", hid_dim * hid_dim) / math.sqrt(hid_dim), hid_dim, hid_dim),
          "model.2.bias": f32(0.1 * synth.normal(seed, "cnzsl.b2", hid_dim), hid_dim)}
    if cn:
        for i in (3, 5):
            sd[f"model.{i}.running_mean"] = f32(0.1 * synth.normal(seed, f"cnzsl.rm{i}", hid_dim) if running else np.zeros(hid_dim), hid_dim)
            sd[f"model.{i}.running_var"] = f32(0.5 + synth.uniform(seed, f"cnzsl.rv{i}", hid_dim) if running else np.ones(hid_dim), hid_dim)
    sd["model.6.weight"] = f32((2.0 * synth.uniform(seed, "cnzsl.w6", proto_dim * hid_dim) - 1.0) * b, proto_dim, hid_dim)
    sd["model.6.bias"] = f32(0.05 + 0.05 * synth.uniform(seed, "cnzsl.b6", proto_dim), proto_dim)
    return sd


def synth_rows(seed: int, name: str, rows: int, cols: int) -> np.ndarray:
    """fp32 [rows, cols] ~ N(0, 1): attributes, or feature rows with negative entries."""
    from .. import synth
    return np.ascontiguousarray(synth.normal(seed, name, rows * cols).reshape(rows, cols).astype(np.float32))
