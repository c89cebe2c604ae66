"""DGP baseline graph propagation on MI355X: the repository's ancestor / descendant aggregation,
`GCN_Dense_Att` of baseline/DGP/models/gcn_dense_att.py, with the same constructor, parameter names and `state_dict`
schema ('a_att', 'r_att', 'conv1.w', 'conv1.b', ..., 'conv-last.w', 'conv-last.b').

The reference keeps one torch sparse COO matrix per distance group and side and runs D `torch.mm(adj, support)` per
layer.  Here each side is ONE CSR over all groups (edge -> group id, 1 / degree); a layer is one fp32 MFMA product
(`hgr_matmul_f32`) and one gather-reduce launch (`hgr_csr_group_aggregate`) that also applies the attention weights,
the bias, LeakyReLU and the final row normalisation.  `GCN_Dense_Att.forward` is inference only (`torch.no_grad`).

Training (train_gcn_dense_att.py:80-102) goes through `DGPTrainer`, not through `model.train()(x)`: the same forward with
counter-based dropout (`hgr_dropout_counter`, host twin `dropout_keep`), the masked L2 loss and its gradient
(`hgr_dgp_loss_head`), a closed-form backward - `hgr_csr_group_att_grad` for dO and the attention gradient, the forward
gather on `GraphOperator.adjoint()` for the transposed propagation, three fp32 products per layer - and coupled-decay Adam
(`hgr_adam_l2`).  No atomics anywhere: a step repeated from the same state and seed gives bit-equal parameters.
`python -m hgr_net_amd.baseline.train_dgp` is the reference script's command line on top of it.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from .. import ops
from ._shared import AdamL2State, BufferPool, fmix32, need_device

CHUNK = 256          # edges per work item: bounds the longest gather a single workgroup performs


def group_edges(n: int, edges: Sequence[Sequence[int]]) -> List[List[Tuple[int, int]]]:
    """materials/make_dense_grouped_graph.py:14-38: edges_set[d] = every (u, x) with x at BFS distance d from u along
    the directed edges (d = 0 holds the self pairs).  Same pair order as the reference script."""
    adjs: List[List[int]] = [[] for _ in range(n)]
    for u, v in edges:
        adjs[u].append(v)
    groups: List[List[Tuple[int, int]]] = []
    for u in range(n):
        dist = {u: 0}
        q, head = [u], 0
        while head < len(q):
            x = q[head]
            head += 1
            for y in adjs[x]:
                if y not in dist:
                    dist[y] = dist[x] + 1
                    q.append(y)
        for x, d in dist.items():
            while len(groups) <= d:
                groups.append([])
            groups[d].append((u, x))
    return groups


def fold_groups(edges_set: Sequence[Sequence[Sequence[int]]], lim: int = 4) -> List[List[Tuple[int, int]]]:
    """train_gcn_dense_att.py:52-56: distances beyond `lim` share group `lim`."""
    out = [[tuple(e) for e in g] for g in edges_set[:lim + 1]]
    for g in edges_set[lim + 1:]:
        out[lim].extend(tuple(e) for e in g)
    return out


class GraphOperator:
    """One side of the propagation: the D in-degree-normalised operators `normt_spm(adj_d or adj_d^T, 'in')`
    (baseline/DGP/utils.py:56-65) merged into a CSR with per-edge group ids, plus the work-item tables of the kernel."""

    def __init__(self, n: int, edges_set: Sequence[Sequence[Sequence[int]]], transpose: bool, device):
        assert len(edges_set) <= 32
        rows, cols, grps = [], [], []
        for d, edges in enumerate(edges_set):
            e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
            # a_adj = (adj^T row-normalised): row = edge target, column = edge source; r_adj: the other way round
            r, c = (e[:, 0], e[:, 1]) if transpose else (e[:, 1], e[:, 0])
            rows.append(r); cols.append(c); grps.append(np.full(len(e), d, np.int64))
        row, col, grp = np.concatenate(rows), np.concatenate(cols), np.concatenate(grps)
        # 1 / (row sum of the group's matrix) = 1 / number of edges of (row, group), duplicates counted like coo -> csr does
        key = row * len(edges_set) + grp
        cnt = np.bincount(key, minlength=n * len(edges_set))
        inv = (1.0 / cnt[key]).astype(np.float32)
        self._build(n, len(edges_set), row, col, grp, inv, device)

    def _build(self, n: int, D: int, row, col, grp, inv, device) -> None:
        """CSR and work-item tables of the edges (row, col, grp, inv), sorted here by (row, group, column)."""
        order = np.lexsort((col, grp, row))                     # by row, then group, then column: fixed summation order
        row, col, grp, inv = row[order], col[order], grp[order], inv[order]
        self._coo = (row, col, grp, inv)                        # host copy: adjoint() transposes it
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(row, minlength=n), out=ptr[1:])
        item_row, item_e0, item_e1, item_slot = [], [], [], []
        split_row, split_slot0, split_n = [], [], []
        slots = 0
        for i in range(n):
            e0, e1 = int(ptr[i]), int(ptr[i + 1])
            k = max(1, -(-(e1 - e0) // CHUNK))
            if k == 1:
                item_row.append(i); item_e0.append(e0); item_e1.append(e1); item_slot.append(-1)
            else:
                split_row.append(i); split_slot0.append(slots); split_n.append(k)
                for j in range(k):
                    item_row.append(i); item_e0.append(e0 + j * CHUNK); item_e1.append(min(e1, e0 + (j + 1) * CHUNK)); item_slot.append(slots)
                    slots += 1
        # heavy items first: the tail of the launch is made of short rows
        order = np.argsort(-(np.asarray(item_e1) - np.asarray(item_e0)), kind="stable")
        i32 = lambda a: torch.tensor(np.asarray(a, dtype=np.int32), device=device)
        self.n, self.D, self.nnz, self.n_slots = n, D, len(col), slots
        self.item_row, self.item_e0 = i32(np.asarray(item_row)[order]), i32(np.asarray(item_e0)[order])
        self.item_e1, self.item_slot = i32(np.asarray(item_e1)[order]), i32(np.asarray(item_slot)[order])
        self.split_row, self.split_slot0, self.split_n = i32(split_row), i32(split_slot0), i32(split_n)
        self.col = i32(col)
        self.inv_deg = torch.tensor(inv, device=device)
        self.grp = torch.tensor(grp.astype(np.uint8), device=device)
        self._partial = None
        self._partial_groups = None

    def partial(self, c: int) -> torch.Tensor:
        if self.n_slots == 0:
            return None
        if self._partial is None or self._partial.shape[1] != c:
            self._partial = torch.empty((self.n_slots, c), dtype=torch.float32, device=self.col.device)
        return self._partial

    def aggregate(self, support: torch.Tensor, att: torch.Tensor, bias, out: torch.Tensor, slope: float, normalize: bool) -> torch.Tensor:
        ops.csr_group_aggregate(support, self, att, bias, out, slope, normalize)
        return out

    def partial_groups(self) -> torch.Tensor:
        """[n_slots, D] partials of hgr_csr_group_att_grad for the rows cut into several items."""
        if self.n_slots == 0:
            return None
        if self._partial_groups is None:
            self._partial_groups = torch.empty((self.n_slots, self.D), dtype=torch.float32, device=self.col.device)
        return self._partial_groups

    def adjoint(self) -> "GraphOperator":
        """The transposed operator for the backward pass: edge (i, j) becomes (j, i) and keeps ITS OWN 1 / degree and group, so
        that `aggregate(dO, att, None, T, 1.0, False)` on it is T[j] = sum_{e: col_e = j} att[grp_e] inv_e dO[row_e].  Sorted by
        (column, group, row) of the original, with its own work-item tables: the adjoint of the ancestor side has the descendant
        side's skew (the root's row is cut into many items)."""
        row, col, grp, inv = self._coo
        t = GraphOperator.__new__(GraphOperator)
        t._build(self.n, self.D, col, row, grp, inv, self.col.device)
        return t


class GraphConv(nn.Module):
    """gcn_dense_att.py:12-46: parameters `w [in, out]` (Xavier) and `b [out]`; LeakyReLU(0.2) unless `relu=False`."""

    def __init__(self, in_channels: int, out_channels: int, dropout: bool = False, relu: bool = True):
        super().__init__()
        self.dropout = nn.Dropout(p=0.5) if dropout else None
        self.w = nn.Parameter(torch.empty(in_channels, out_channels))
        self.b = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.w)
        self.relu = nn.LeakyReLU(negative_slope=0.2) if relu else None

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor, op: GraphOperator, att: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        if self.training and self.dropout is not None:
            raise NotImplementedError("training-mode dropout: this build runs the DGP propagation for inference (model.eval())")
        n, c = inputs.shape[0], self.w.shape[1]
        if c % 4:
            raise ValueError(f"out_channels={c} must be a multiple of 4")
        support = torch.empty((n, c), dtype=torch.float32, device=inputs.device)
        ops.matmul_f32(inputs, self.w, support)                                    # bias is folded into the aggregation
        out = torch.empty((n, c), dtype=torch.float32, device=inputs.device)
        return op.aggregate(support, att, self.b, out, 0.2 if self.relu is not None else 1.0, normalize)


class GCN_Dense_Att(nn.Module):
    """gcn_dense_att.py:49-115.  `hidden_layers` like the reference: 'd2048,d' = dropout + 2048 hidden, dropout last."""

    def __init__(self, n: int, edges_set, in_channels: int, out_channels: int, hidden_layers: str, device="cuda"):
        super().__init__()
        self.n, self.d = n, len(edges_set)
        self.a_op = GraphOperator(n, edges_set, transpose=False, device=device)
        self.r_op = GraphOperator(n, edges_set, transpose=True, device=device)
        hl = hidden_layers.split(",")
        dropout_last = hl[-1] == "d"
        if dropout_last:
            hl = hl[:-1]
        self.a_att = nn.Parameter(torch.ones(self.d))
        self.r_att = nn.Parameter(torch.ones(self.d))
        layers, last_c, i = [], in_channels, 0
        for c in hl:
            dropout = c[0] == "d"
            c = int(c[1:] if dropout else c)
            i += 1
            conv = GraphConv(last_c, c, dropout=dropout)
            self.add_module("conv{}".format(i), conv)
            layers.append(conv)
            last_c = c
        conv = GraphConv(last_c, out_channels, relu=False, dropout=dropout_last)
        self.add_module("conv-last", conv)
        layers.append(conv)
        self.layers = layers
        self.to(device)

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("GCN_Dense_Att needs device tensors: the product path has no CPU fallback")
        x = x.float().contiguous()
        graph_side = True
        for k, conv in enumerate(self.layers):
            op, att = (self.a_op, self.a_att) if graph_side else (self.r_op, self.r_att)
            att = torch.softmax(att.float(), dim=0).contiguous()                  # D <= 32 scalars
            x = conv(x, op, att, normalize=(k == len(self.layers) - 1))          # F.normalize fused into the last layer
            graph_side = not graph_side
        return x


# ---- training (baseline/DGP/train_gcn_dense_att.py:80-102) -----------------------------------------------------------------
def dropout_keep(seed: int, step: int, layer: int, n_rows: int, n_cols: int) -> np.ndarray:
    """Host twin of `hgr_dropout_counter`: the keep mask [n_rows, n_cols] (bool) of training step `step` (1-based) in front of
    layer `layer` (index into `GCN_Dense_Att.layers`).  With 32-bit wrap-around arithmetic and fmix32 = murmur3's finaliser:

        key  = fmix32(seed + 0x9E3779B9 * (step + 1));  key = fmix32(key ^ (layer * 0x85EBCA6B + 0xC2B2AE35))
        keep = fmix32((row * n_cols + column) ^ key) >> 31

    A pure function of its arguments: forward and backward recompute it, nothing is stored, and an oracle reproduces a
    training step exactly.  It is NOT torch's generator: parity with `nn.Dropout` under `torch.manual_seed` is not a goal,
    only its distribution (each element kept with probability 1/2, kept elements scaled by 2)."""
    if n_rows * n_cols > 0xFFFFFFFF:
        raise ValueError("dropout_keep: n_rows * n_cols must fit the 32-bit element index")
    m = 0xFFFFFFFF
    key = fmix32(np.array([((seed & m) + 0x9E3779B9 * ((step + 1) & m)) & m], np.uint64))
    key = fmix32(key ^ np.uint64(((layer & m) * 0x85EBCA6B + 0xC2B2AE35) & m))
    idx = np.arange(n_rows * n_cols, dtype=np.uint64)
    return ((fmix32(idx ^ key) >> np.uint64(31)) != 0).reshape(n_rows, n_cols)


class DGPTrainer:
    """Full-graph training of a `GCN_Dense_Att` on the device: the reference's epoch (train_gcn_dense_att.py:96-102) - forward
    with dropout, `utils.l2_loss` on the selected rows, backward through both sparse sides and the attention logits,
    `torch.optim.Adam(lr, weight_decay)` - as fp32 products (`hgr_matmul_f32`), the forward gather, the backward gather
    (`hgr_csr_group_att_grad`), the forward gather on the adjoint operators, `hgr_dgp_loss_head`, `hgr_dropout_counter`
    and `hgr_adam_l2`.  The model's own forward stays inference only; nothing in a step synchronises with the host.

    `rows` [n_t] are DISTINCT output rows and `targets` [n_t, out_channels] their target vectors, row k of `targets`
    belonging to output row `rows[k]`.  (The reference script indexes both the outputs and the fc vectors with the same
    shuffled list; train_dgp.py maps that convention onto this one.)"""

    def __init__(self, model: GCN_Dense_Att, lr: float = 1e-3, weight_decay: float = 5e-4, seed: int = 0,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        self.model, self.lr, self.wd, self.seed, self.betas, self.eps = model, lr, weight_decay, int(seed), betas, eps
        sides = {k % 2 for k in range(len(model.layers))}
        self.adj = {s: (model.a_op if s == 0 else model.r_op).adjoint() for s in sides}
        self.opt = AdamL2State(dict(model.named_parameters()), betas, eps, weight_decay, "DGPTrainer")
        self.params, self.m, self.v, self.g = self.opt.params, self.opt.m, self.opt.v, self.opt.g
        self._names = {id(p): k for k, p in self.params.items()}
        self._buf = BufferPool(model.a_att).pool
        self._rows = None

    @property
    def t(self) -> int:
        """Optimiser steps taken; the dropout of step t + 1 uses t + 1."""
        return self.opt.t

    def _side(self, k: int):
        m = self.model
        return (m.a_op, m.a_att, 0) if k % 2 == 0 else (m.r_op, m.r_att, 1)

    def _prepare(self, x, rows, targets):
        m = self.model
        dev = m.a_att.device
        need_device(x, "DGPTrainer")
        x = x.float().contiguous()
        # distinct rows: checked on the host once per rows object (a device tensor costs one copy back, the first time only)
        if self._rows is None or self._rows[0] is not rows:
            r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
            r = r.astype(np.int64).reshape(-1)
            if r.size == 0 or r.min() < 0 or r.max() >= m.n:
                raise ValueError("DGPTrainer: rows must be indices into the graph's nodes")
            if np.unique(r).size != r.size:
                raise ValueError("DGPTrainer: rows must be distinct (a duplicate row would receive two gradients)")
            self._rows = (rows, torch.tensor(r.astype(np.int32), device=dev))
        rows_dev = self._rows[1]
        targets = torch.as_tensor(targets).to(dev).float().contiguous()
        if targets.shape != (rows_dev.numel(), m.layers[-1].w.shape[1]):
            raise ValueError(f"DGPTrainer: targets must be [{rows_dev.numel()}, {m.layers[-1].w.shape[1]}], got {tuple(targets.shape)}")
        return x, rows_dev, targets

    @torch.no_grad()
    def _forward_backward(self, x: torch.Tensor, rows: torch.Tensor, targets: torch.Tensor, step: int) -> torch.Tensor:
        m, n = self.model, self.model.n
        layers = m.layers
        saved, h = [], x
        for k, conv in enumerate(layers):
            op, att, _ = self._side(k)
            a = torch.softmax(att.data.float(), dim=0).contiguous()              # D <= 32 scalars
            xd = h
            if conv.dropout is not None:
                xd = ops.dropout_counter(h, self._buf(("xd", k), h.shape), self.seed, step, k)
            c = conv.w.shape[1]
            if c % 4:
                raise ValueError(f"out_channels={c} must be a multiple of 4")
            s = ops.matmul_f32(xd, conv.w.data, self._buf(("s", k), (n, c)))
            # the last layer stays un-normalised: F.normalize and its backward live in the loss head
            y = op.aggregate(s, a, conv.b.data, self._buf(("y", k), (n, c)), 0.2 if conv.relu is not None else 1.0, False)
            saved.append((xd, s, y, a))
            h = y
        n_t = rows.numel()
        loss = self._buf("loss", (1,))
        g = self._buf(("g", len(layers) - 1), h.shape)
        ops.dgp_loss_head(h, rows, targets, self._buf("loss_rows", (n_t,)), loss, g)
        for name in ("a_att", "r_att"):
            self.g[name].zero_()
        for k in range(len(layers) - 1, -1, -1):
            conv = layers[k]
            op, att, side = self._side(k)
            xd, s, y, a = saved[k]
            c = conv.w.shape[1]
            p = self._buf(("p", side), (n, op.D))
            if conv.relu is not None:
                ops.csr_group_att_grad(s, op, conv.b.data, g, y, g, p, 0.2)          # dO replaces G in place
            else:
                ops.csr_group_att_grad(s, op, conv.b.data, g, None, None, p)
            scratch = self._buf("colsum", (((n + 511) // 512) * max(4096, op.D),))
            da = ops.colsum(p, self._buf(("da", side), (op.D,)), scratch, accumulate=False)
            self.g["a_att" if side == 0 else "r_att"].add_(a * (da - (a * da).sum()))   # softmax backward, D <= 32 scalars
            t = self.adj[side].aggregate(g, a, None, self._buf(("t", k), (n, c)), 1.0, False)
            ops.colsum(t, self.g[self._names[id(conv.b)]], scratch, accumulate=False)
            ops.matmul_f32(xd.t(), t, self.g[self._names[id(conv.w)]])
            if k > 0:
                g = ops.matmul_f32(t, conv.w.data.t(), self._buf(("g", k - 1), xd.shape))
                if conv.dropout is not None:
                    ops.dropout_counter(g, g, self.seed, step, k)
        return loss

    def grads(self, x, rows, targets) -> dict:
        """Gradients of the training loss of the NEXT step (its dropout masks), by state-dict name; no optimiser step."""
        x, rows, targets = self._prepare(x, rows, targets)
        self._forward_backward(x, rows, targets, self.t + 1)
        return {k: v.clone() for k, v in self.g.items()}

    def step(self, x, rows, targets) -> torch.Tensor:
        """One epoch of the reference: forward (dropout where `hidden_layers` has a 'd'), loss, backward, Adam.  Returns the
        training-mode loss as a 0-dim device tensor."""
        x, rows, targets = self._prepare(x, rows, targets)
        loss = self._forward_backward(x, rows, targets, self.t + 1).clone().reshape(())
        self.opt.step(self.lr)
        return loss

    @torch.no_grad()
    def losses(self, x, rows, targets, val_rows=None, val_targets=None) -> Tuple[float, float]:
        """The reference's `train_loss` / `val_loss` (train_gcn_dense_att.py:104-112): eval mode through the inference
        forward, `utils.l2_loss` on the selected rows; val_loss = 0 without validation rows."""
        m = self.model
        was_training = m.training
        out = m.eval()(x)
        m.train(was_training)

        def l2(r, t):
            r = torch.as_tensor(np.asarray(r.detach().cpu() if torch.is_tensor(r) else r), dtype=torch.long, device=out.device).reshape(-1)
            t = torch.as_tensor(t).to(out.device).float()
            return float(((out[r] - t) ** 2).sum() / (len(r) * 2))
        return l2(rows, targets), (l2(val_rows, val_targets) if val_rows is not None and len(val_rows) else 0.0)
