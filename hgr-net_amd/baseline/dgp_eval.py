"""Scoring of DGP's predicted classifiers on the device: what the reference's baseline/DGP/evaluate_imagenet.py and
evaluate_21kp.py (`test_on_subset`) compute from an `epoch_K.pred` file and image features - Hit@1/2/5/10/20, `To`, `Path`, `Point`.

Per batch, in half precision, the reference forms `table = [feat | 1] @ pred_vectors.T`, overwrites the `n` leading (seen) columns
with 1e-7 unless `--consider-trains`, counts `rks = (table >= table[:, target]).sum(1)` and `hits[k] += (rks <= k).sum()`, takes the
top-1 over all columns (`To`) and, per node of the target's path, the top-1 with every column off that node's level filled with -1
(`Path`, `Point`).  evaluate_21kp.py is the same loop with the test set as the node list and n = 0.

Reference quirk, reproduced: `logits = copy.copy(table)` shares storage with `table`, so the 1e-7 fill also lands in the values the
top-1 and the level picks are taken from - everything is scored on the MASKED table.  In fp16 the fill is 2^-23: positive, it beats
every negative score of its level.  Ties are pinned here ("the lowest column holding the maximum"); `torch.topk` promises no order.

Here the product is `ops.gemm_nt` with a bias epilogue (the bias column of the predictions; acc + bias rounded to fp16 once, as the
product with the ones column is), one `hgr_dgp_score_rows` launch scores the table and `hgr_eval_counters` /
`hgr_eval_counters_rows` advance float64 counters that stay on the device until `result()`.  `score_rows_host` / `counters_host` are
the numpy twins of the two kernels."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from ..hierarchy import build_hierarchy

TOP = (1, 2, 5, 10, 20)
FILL = 1e-7                      # evaluate_imagenet.py:93; an fp16 table stores it as 2^-23
MAXL = 32                        # longest path / most levels the kernels take
K_PRED = 20                      # width of the rank's top-k shaped encoding: max(TOP)


# ---- the files --------------------------------------------------------------------------------------------------------------------------
def load_pred(path) -> dict:
    """{'wnids': [str], 'pred': fp32 tensor [len(wnids), K + 1]} as train_dgp / the reference's trainers save `epoch_K.pred`."""
    obj = torch.load(path, map_location="cpu")
    if not isinstance(obj, dict) or "wnids" not in obj or "pred" not in obj:
        raise ValueError(f"{path}: not a prediction file ({{'wnids', 'pred'}})")
    pred = torch.as_tensor(obj["pred"]).detach().to(torch.float32)
    wnids = list(obj["wnids"])
    if pred.dim() != 2 or pred.shape[0] != len(wnids):
        raise ValueError(f"{path}: {len(wnids)} wnids for predictions of shape {tuple(pred.shape)}")
    return {"wnids": wnids, "pred": pred}


def pick_vectors(pred: dict, wnids: Sequence[str]) -> torch.Tensor:
    """utils.py:34-49 on `dict(zip(pred['wnids'], pred['pred']))`: row i = the vector of wnids[i], a ZERO vector when the file has
    none (the last one when the file lists a wnid twice, like the dict)."""
    vec = torch.as_tensor(pred["pred"]).detach().to(torch.float32).cpu()
    pos = {w: i for i, w in enumerate(pred["wnids"])}
    out = torch.zeros((len(wnids), vec.shape[1]), dtype=torch.float32)
    have = [(i, pos[w]) for i, w in enumerate(wnids) if w in pos]
    if have:
        dst, src = zip(*have)
        out[list(dst)] = vec[list(src)]
    return out


def load_features(path) -> Dict[str, np.ndarray]:
    """A feature file: one [n_i, K] array per wnid (`np.savez(path, **{wnid: rows})`)."""
    out = {}
    with np.load(path) as z:
        for w in z.files:
            a = np.asarray(z[w])
            if a.ndim != 2 or a.dtype.kind != "f":
                raise ValueError(f"{path}: '{w}' is {a.dtype} {a.shape}, expected a float [n, K] array")
            out[w] = a
    widths = {a.shape[1] for a in out.values()}
    if len(widths) > 1:
        raise ValueError(f"{path}: feature widths differ: {sorted(widths)}")
    return out


def keep_rows(n: int, ratio: float) -> int:
    """--keep-ratio: the first ceil(ratio * n) rows of a class (the reference's `datasets` package is not part of it; this rule is ours)."""
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"keep ratio {ratio} outside (0, 1]")
    return min(n, int(math.ceil(ratio * n - 1e-12)))


# ---- the tree over an ordered name list (evaluate_imagenet.py:26-59) -------------------------------------------------------------------
@dataclass
class ListTree:
    nodes: List[str]
    c2p: List[List[int]]             # positions in `nodes` of the ancestors strictly between the root and the node
    depth: np.ndarray                # int32 [N] = len(c2p[i])
    d2n: Dict[int, List[int]]
    n_levels: int

    def path(self, i: int) -> List[int]:
        return self.c2p[i] + [i]


def build_list_tree(graph_edges, nodes_name: Sequence[str]) -> ListTree:
    """The reference's `gen_tree(nodes_name)`: paths are shortest root paths of the FULL graph (hierarchy.build_hierarchy's search),
    indexed into `nodes_name` (first occurrence, like list.index)."""
    h = build_hierarchy(graph_edges)
    full = {w: i for i, w in enumerate(h.nodes)}
    pos: Dict[str, int] = {}
    for i, w in enumerate(nodes_name):
        pos.setdefault(w, i)
    c2p = []
    for w in nodes_name:
        if w not in full:
            raise ValueError(f"node '{w}' is not in the graph")
        chain = []
        for a in h.c2p[full[w]]:
            name = h.nodes[a]
            if name not in pos:
                raise ValueError(f"ancestor '{name}' of '{w}' is not in the node list: the list must hold every node's whole path")
            chain.append(pos[name])
        c2p.append(chain)
    depth = np.array([len(c) for c in c2p], dtype=np.int32)
    d2n: Dict[int, List[int]] = {}
    for i, d in enumerate(depth.tolist()):
        d2n.setdefault(d, []).append(i)
    n_levels = int(depth.max()) + 1 if len(depth) else 0
    return ListTree(list(nodes_name), c2p, depth, d2n, n_levels)


# ---- numpy twins of the kernels ---------------------------------------------------------------------------------------------------------
def score_rows_host(table, depth, n_levels: int, n_masked: int = 0, mask_value: float = FILL, targets=None, target: int = 0,
                    n_cols: Optional[int] = None):
    """(rank [rows], top1 [rows], lv [rows, n_levels]) int32: hgr_dgp_score_rows (include/hgr.h) in numpy.  `table` fp16 or fp32
    [rows, >= n_cols]; the first `n_masked` columns read as `mask_value` rounded to the table's type; the lowest column wins a tie."""
    t = np.asarray(table)
    if t.ndim != 2 or t.dtype not in (np.float16, np.float32):
        raise ValueError("table must be a 2-d fp16 or fp32 array")
    nc = t.shape[1] if n_cols is None else int(n_cols)
    depth = np.asarray(depth)[:nc]
    if not (1 <= nc <= t.shape[1] and len(depth) == nc and 0 <= n_masked <= nc and 1 <= n_levels <= MAXL):
        raise ValueError("bad sizes")
    v = t[:, :nc].astype(np.float32)                                   # exact for both types
    if np.isnan(v).any():
        raise ValueError("NaN scores are not defined")
    v[:, :n_masked] = np.float32(np.asarray(mask_value, dtype=np.float64).astype(t.dtype))
    tg = np.full(t.shape[0], int(target), dtype=np.int64) if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1)
    if len(tg) != t.shape[0] or tg.min() < 0 or tg.max() >= nc:
        raise ValueError("a target lies outside the scored columns")
    rank = (v >= v[np.arange(len(tg)), tg][:, None]).sum(1).astype(np.int32)
    top1 = v.argmax(1).astype(np.int32)                                # numpy's argmax: the first maximum
    lv = np.empty((t.shape[0], n_levels), dtype=np.int32)
    for l in range(n_levels):
        lv[:, l] = np.where(depth[None, :] == l, v, np.float32(-1.0)).argmax(1)
    return rank, top1, lv


def counters_host(tree: ListTree, rank, top1, lv, targets) -> np.ndarray:
    """float64 [9] of one batch, as hgr_eval_counters(_rows) advance them: hits@1,2,5,10,20 (rank <= k), top-1 hits on any node of
    the target's path, edges / (L - 1) (the single match when L == 1), points / L, rows."""
    acc = np.zeros(9, dtype=np.float64)
    for r, t in enumerate(np.asarray(targets).reshape(-1).tolist()):
        path = tree.path(int(t))
        L = len(path)
        for i, k in enumerate(TOP):
            acc[i] += int(rank[r]) <= k
        m = [int(lv[r, tree.depth[p]]) == p for p in path]
        acc[5] += sum(int(top1[r]) == p for p in path)
        acc[6] += float(m[0]) if L == 1 else sum(a and b for a, b in zip(m[:-1], m[1:])) / (L - 1)
        acc[7] += sum(m) / L
        acc[8] += 1
    return acc


# ---- results and the reference's printed lines -------------------------------------------------------------------------------------------
def result_from_acc(acc: np.ndarray, nodes: Sequence[str]) -> dict:
    """`acc` float64 [N + 1, 9]: one row per class of the class route, the last row for the packed route."""
    acc = np.asarray(acc, dtype=np.float64)
    tot = acc.sum(0)
    per_class = {}
    for i in np.nonzero(acc[:-1, 8] > 0)[0].tolist():
        a = acc[i]
        per_class[nodes[i]] = {"hits": a[:5].tolist(), "tot": int(a[8]), "to": float(a[5]), "path": float(a[6]), "point": float(a[7])}
    return {"hits": tot[:5].tolist(), "tot": int(tot[8]), "to": float(tot[5]), "path": float(tot[6]), "point": float(tot[7]),
            "per_class": per_class,
            "results": {w: [h / c["tot"] for h in c["hits"]] for w, c in per_class.items()}}


def class_line(i: int, n_classes: int, wnid: str, hits, tot: int, s_hits, s_tot: int, s_to: float, s_path: float, s_point: float) -> str:
    """evaluate_imagenet.py:246-253."""
    s = "{}/{}, {}: ".format(i, n_classes, wnid)
    for h, sh in zip(hits, s_hits):
        s += "{:.0f}%({:.2f}%) ".format(h / tot * 100, sh / s_tot * 100)
    s += "To:{:.2f}% ".format(s_to / s_tot * 100)
    s += "Path:{:.2f}% ".format(s_path / s_tot * 100)
    s += "Point:{:.2f}% ".format(s_point / s_tot * 100)
    return s + "x{}({})".format(tot, s_tot)


def summary_line(s_hits, s_tot: int) -> str:
    """evaluate_imagenet.py:255-258."""
    return "summary: " + "".join("{:.2f}% ".format(h / s_tot * 100) for h in s_hits) + "total {}".format(s_tot)


def report_lines(res: dict, order: Sequence[str]) -> List[str]:
    """The per-class lines in the order the classes were evaluated (running sums as the reference prints them), then `summary:`."""
    lines, s_hits, s_tot, s_to, s_path, s_point = [], [0.0] * 5, 0, 0.0, 0.0, 0.0
    for i, w in enumerate(order, 1):
        c = res["per_class"].get(w)
        if c is None:
            continue
        s_hits = [a + b for a, b in zip(s_hits, c["hits"])]
        s_tot += c["tot"]; s_to += c["to"]; s_path += c["path"]; s_point += c["point"]
        lines.append(class_line(i, len(order), w, c["hits"], c["tot"], s_hits, s_tot, s_to, s_path, s_point))
    if res["tot"]:
        lines.append(summary_line(res["hits"], res["tot"]))
    return lines


class HostEvaluator:
    """The evaluator's bookkeeping on tables that already exist, in numpy: the twin the device route is tested against."""

    def __init__(self, tree: ListTree, n_seen: int, consider_trains: bool = False):
        self.tree, self.n_masked = tree, 0 if consider_trains else int(n_seen)
        self.acc = np.zeros((len(tree.nodes) + 1, 9), dtype=np.float64)

    def add(self, table, target: int):
        rank, top1, lv = score_rows_host(table, self.tree.depth, self.tree.n_levels, self.n_masked, FILL, None, target, len(self.tree.nodes))
        self.acc[target] += counters_host(self.tree, rank, top1, lv, np.full(len(rank), target))
        return rank, top1, lv

    def add_rows(self, table, targets):
        rank, top1, lv = score_rows_host(table, self.tree.depth, self.tree.n_levels, self.n_masked, FILL, targets, 0, len(self.tree.nodes))
        self.acc[-1] += counters_host(self.tree, rank, top1, lv, targets)
        return rank, top1, lv

    def result(self) -> dict:
        return result_from_acc(self.acc, self.tree.nodes)


# ---- the device route -------------------------------------------------------------------------------------------------------------------
def _table_dtype(name) -> torch.dtype:
    try:
        return {"f16": torch.float16, "fp16": torch.float16, "float16": torch.float16, torch.float16: torch.float16,
                "f32": torch.float32, "fp32": torch.float32, "float32": torch.float32, torch.float32: torch.float32}[name]
    except KeyError:
        raise ValueError(f"dtype {name!r}: the table is 'f16' (the reference's arithmetic) or 'fp32'") from None


class DGPEvaluator:
    """`nodes`: the ordered class list the predictions are scored over, its first `n_seen` entries the seen classes (0: the 21K-P
    protocol); `pred`: a prediction file's dict or the picked [N, K + 1] matrix itself.  `add(features, target)` takes one class per
    batch, `add_rows(features, targets)` rows of mixed classes; `features` are [B, K] fp16 or fp32 device tensors (`cnn`, if given, is
    applied first).  Nothing is read back before `result()`.  dtype 'f16' reproduces the reference's half-precision table and its
    ties; 'fp32' keeps acc + bias in fp32 (the operands are fp16 either way)."""

    def __init__(self, graph_edges, nodes: Sequence[str], n_seen: int, pred, consider_trains: bool = False, dtype="f16",
                 device="cuda:0", cnn: Optional[Callable] = None, tree: Optional[ListTree] = None):
        from .. import ops
        from ._shared import ancestor_tables                           # imports this module
        self.ops = ops
        self.tree = tree if tree is not None else build_list_tree(graph_edges, nodes)
        n = len(self.tree.nodes)
        if not 0 <= n_seen <= n:
            raise ValueError(f"n_seen={n_seen} outside 0..{n}")
        if n < 1 or self.tree.n_levels > MAXL:
            raise ValueError(f"{n} nodes on {self.tree.n_levels} levels: at least one node, at most {MAXL} levels")
        vec = pick_vectors(pred, self.tree.nodes) if isinstance(pred, dict) else torch.as_tensor(pred).detach().to(torch.float32).cpu()
        if vec.dim() != 2 or vec.shape[0] != n or vec.shape[1] < 2:
            raise ValueError(f"predictions of shape {tuple(vec.shape)} for {n} nodes (one row per node, a bias column last)")
        self.device = torch.device(device)
        self.cnn, self.n, self.n_seen = cnn, n, int(n_seen)
        self.n_masked = 0 if consider_trains else int(n_seen)
        self.table_dtype = _table_dtype(dtype)
        self.k = vec.shape[1] - 1
        self.kp = -(-self.k // 64) * 64                                # hgr_gemm_nt: K % 64 == 0, zero padded
        v16 = vec.to(torch.float16)                                    # evaluate_imagenet.py:193
        w16 = torch.zeros((n, self.kp), dtype=torch.float16)
        w16[:, :self.k] = v16[:, :self.k]
        self.w16 = w16.to(self.device)
        self.bias = v16[:, self.k].to(torch.float32).to(self.device)
        self.ld = -(-n // 8) * 8                                       # table rows start 16-byte aligned
        self.depth = torch.from_numpy(self.tree.depth.copy()).to(self.device)
        self._ptr_host, self.anc_ptr, self.anc_nodes, self.anc_levels = ancestor_tables(self.tree, self.device)
        self.acc = torch.zeros((n + 1, 9), dtype=torch.float64, device=self.device)     # one row per class, the last for add_rows
        self._buf, self._cap = None, 0

    def index(self, target) -> int:
        return self.tree.nodes.index(target) if isinstance(target, str) else int(target)

    def _buffers(self, rows: int):
        """Staging rows, table and outputs of a batch of `rows` rows: views of one set of buffers sized for the largest batch so far."""
        if self._cap < rows:
            dev = self.device
            self._buf = {"feat": torch.zeros((rows, self.kp), dtype=torch.float16, device=dev),
                         "table": torch.zeros((rows, self.ld), dtype=self.table_dtype, device=dev),
                         "out": (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty((rows, 1), dtype=torch.int32, device=dev),
                                 torch.empty((rows, self.tree.n_levels), dtype=torch.int32, device=dev),
                                 torch.empty((rows, K_PRED), dtype=torch.int32, device=dev))}
            self._cap = rows
        b = self._buf
        return {"feat": b["feat"][:rows], "table": b["table"][:rows], "out": tuple(t[:rows] for t in b["out"])}

    def table(self, features: torch.Tensor) -> torch.Tensor:
        """The classifier product [B, N] of one batch (a view of a buffer the next batch of this size overwrites)."""
        if self.cnn is not None:
            features = self.cnn(features)
        if not (isinstance(features, torch.Tensor) and features.is_cuda and features.dim() == 2 and features.shape[1] == self.k
                and features.dtype in (torch.float16, torch.float32) and features.shape[0] >= 1):
            raise self.ops._lib.HgrError(f"features must be a device tensor [B, {self.k}] in fp16 or fp32 (no CPU path)")
        b = self._buffers(features.shape[0])
        if self.kp == self.k and features.dtype == torch.float16 and features.is_contiguous() and features.data_ptr() % 16 == 0:
            f16 = features
        else:
            f16 = b["feat"]
            f16[:, :self.k].copy_(features)                            # the reference's `.half()`; the padding columns stay zero
        self.ops.gemm_nt(f16, self.w16, b["table"], bias=self.bias, epilogue=self.ops.EPI_BIAS, n=self.n, tag="dgp_eval")
        return b["table"][:, :self.n]

    def _score(self, features, targets, target):
        tab = self.table(features)
        out = self._buffers(tab.shape[0])["out"]
        return self.ops.dgp_score_rows(tab, self.depth, self.tree.n_levels, self.n_masked, FILL, targets=targets, target=target,
                                       n_cols=self.n, k_pred=K_PRED, out=out)

    def add(self, features: torch.Tensor, target):
        """One batch of ONE class (a node index or its wnid); returns the device outputs (rank, top1, lv) of the batch - views of
        buffers the next batch overwrites."""
        t = self.index(target)
        if not 0 <= t < self.n:
            raise ValueError(f"target {target} outside the {self.n} nodes")
        rank, top1, lv, pred = self._score(features, None, t)
        o, e = self._ptr_host[t], self._ptr_host[t + 1]
        self.ops.eval_counters(pred, None, t, top1.view(-1), lv, self.anc_nodes[o:e], self.anc_levels[o:e], self.acc[t])
        return rank, top1, lv

    def add_rows(self, features: torch.Tensor, targets: torch.Tensor):
        """One batch of MIXED classes: `targets` int64 [B] on the device, node indices; a row whose target lies outside the nodes
        counts nothing."""
        if not (isinstance(targets, torch.Tensor) and targets.is_cuda and targets.numel() == features.shape[0]):
            raise self.ops._lib.HgrError("targets must be a device tensor with one node index per row")
        tg = (targets if targets.dtype == torch.int64 else targets.to(torch.int64)).contiguous().view(-1)
        rank, top1, lv, pred = self._score(features, tg, 0)
        self.ops.eval_counters_rows(pred, tg, top1.view(-1), lv, self.anc_ptr, self.anc_nodes, self.anc_levels, self.acc[self.n])
        return rank, top1, lv

    def result(self) -> dict:
        """The one host read: {'hits' [5], 'tot', 'to', 'path', 'point', 'per_class' {wnid: the same}, 'results' {wnid: hits / tot}}."""
        return result_from_acc(self.acc.cpu().numpy(), self.tree.nodes)
