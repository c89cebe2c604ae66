"""What the three baselines (DGP, CNZSL, FREE) share on the host: the ancestor tables and the counters of `test()`, the pool of kept
device buffers, the coupled-decay Adam state, the fp32 product in slices of K, the mean of a loss vector, the device check and the
host twin of the kernels' counter mix.  Kernel-side counterpart: csrc/hgr_rows.h."""
from __future__ import annotations

from typing import Dict, Tuple, Union

import numpy as np
import torch

from .. import ops
from .dgp_eval import MAXL, TOP, ListTree

K_SLICE = 512


def need_device(t, who: str, what: str = "") -> None:
    """`who` needs `t` on the device: the products have no CPU path."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{who} needs device tensors{f' ({what})' if what else ''}: the product path has no CPU fallback")


def fmix32(h) -> np.ndarray:
    """murmur3's 32-bit finaliser on uint64 values holding 32-bit numbers: the host twin of csrc/hgr_rows.h `fmix32`."""
    h = np.asarray(h).astype(np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def sliced_matmul_f32(x: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, accumulate_first: bool = False,
                      k_slice: int = K_SLICE) -> torch.Tensor:
    """out (+)= alpha x wt^T for x [M, K] and wt [N, K], accumulated over slices of `k_slice` columns; the first slice overwrites
    `out` unless `accumulate_first` (a bias written there beforehand).  `hgr_matmul_f32` keeps ONE fp32 accumulator per output over
    the whole inner dimension; at 2048 columns that chain lands 2.3e-6 of max|out| away from the blocked sum of a CPU BLAS (the
    reference's fp32 run is 3.9e-7 from fp64), in slices of 512 columns 7.8e-7."""
    k = x.shape[1]
    for j in range(0, k, k_slice):
        e = min(k, j + k_slice)
        ops.matmul_f32(x[:, j:e], wt[:, j:e].t(), out, alpha=alpha, accumulate=accumulate_first or j > 0)
    return out


class BufferPool:
    """Device buffers kept between calls by key.  `device`: a tensor's device, or a parameter whose device is read at every call (a
    model may move after the pool was made).  ONE re-allocation rule: the shape, the dtype or the device changed."""

    def __init__(self, device: Union[torch.device, torch.Tensor]):
        self._device = device
        self.bufs: Dict[object, torch.Tensor] = {}

    def pool(self, key, shape, dtype: torch.dtype = torch.float32, zero: bool = False) -> torch.Tensor:
        """The buffer of `key`; uninitialised when new, zero-filled with `zero` (padding that no kernel writes stays zero)."""
        b, dev = self.bufs.get(key), getattr(self._device, "device", self._device)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype or b.device != dev:
            b = self.bufs[key] = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=dev)
        return b


def mean_rows(pool: BufferPool, rows_vec: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[0] = mean(rows_vec) as one `hgr_dot_f32` against a kept vector of ones."""
    b = rows_vec.numel()
    ones = pool.bufs.get("ones")
    if ones is None or ones.numel() != b:
        ones = pool.bufs["ones"] = torch.ones(b, dtype=torch.float32, device=rows_vec.device)
    return ops.dot_f32(rows_vec, ones, out, alpha=1.0 / b)


class AdamL2State:
    """`torch.optim.Adam(lr, weight_decay)` with coupled decay over named parameters: the moments `m`, `v`, the gradients `g` the
    backward writes into, the step count `t`; one `hgr_adam_l2` launch per tensor."""

    def __init__(self, named_params: Dict[str, torch.Tensor], betas: Tuple[float, float], eps: float, wd: float, who: str = "AdamL2State"):
        self.params, self.betas, self.eps, self.wd, self.t = dict(named_params), betas, eps, wd, 0
        for k, p in self.params.items():
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError(f"{who}: parameter {k} must be a contiguous fp32 device tensor")
        self.m = {k: torch.zeros_like(p.data) for k, p in self.params.items()}
        self.v = {k: torch.zeros_like(p.data) for k, p in self.params.items()}
        self.g = {k: torch.zeros_like(p.data) for k, p in self.params.items()}

    def step(self, lr: float) -> None:
        self.t += 1
        for k, p in self.params.items():
            ops.adam_l2(p.data, self.g[k], self.m[k], self.v[k], lr, self.t, self.betas, self.eps, self.wd)


# ---- test(): the counters of cnzsl.py:221-321, which FREE's classifier.py shares ---------------------------------------------------------
def ancestor_tables(tree: ListTree, device):
    """(ptr_host, anc_ptr, anc_nodes, anc_levels): every node's path (its ancestors, then itself) and the depth of each path node as
    one CSR - `ptr_host` a list for slicing on the host, the other three int32 on the device (`hgr_eval_counters(_rows)`)."""
    ptr, anc, lev = [0], [], []
    for i in range(len(tree.nodes)):
        path = tree.path(i)
        anc.extend(path)
        lev.extend(int(tree.depth[q]) for q in path)
        ptr.append(len(anc))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32).to(device)
    return ptr, i32(ptr), i32(anc), i32(lev)


def metric_string(acc) -> str:
    """The string `test()` prints, from the nine counters (hits@1,2,5,10,20, hits_all, path_all, point_all, rows).  The reference
    keeps the hits and hits_all as fp32 tensors and the other two as Python floats; the divisions are done in those types."""
    acc = np.asarray(acc, dtype=np.float64)
    n = int(acc[8])
    out = "\n"
    for i, k in enumerate(TOP):
        out += "Top@{}(%):{:.2f}".format(k, float(np.float32(acc[i]) / np.float32(n) * np.float32(100.0)))
        out += ", " if k != TOP[-1] else "."
    out += " hit_ratio(%):{:.2f}".format(float(np.float32(acc[5]) / np.float32(n) * np.float32(100.0)))
    out += " path_ratio(%):{:.2f}".format(acc[6] / n * 100.0)
    out += " point_ratio(%):{:.2f}".format(acc[7] / n * 100.0)
    return out


class TreeScorer:
    """`test()` over the candidate classes `test_index` of `tree`: one `hgr_eval_rows` launch per batch with both of its subsets set
    to the candidates, then the nine float64 counters of the main evaluation, which stay on the device until `result()`.  A subclass
    says how a batch of features becomes [B, >= N] scores (`scores`); whatever follows the targets in `add` / `add_rows` goes there."""

    def __init__(self, tree: ListTree, test_index, device):
        self.tree, self.n = tree, len(tree.nodes)
        if tree.n_levels > MAXL:
            raise ValueError(f"{tree.n_levels} levels: at most {MAXL}")
        te = np.asarray(test_index.detach().cpu() if torch.is_tensor(test_index) else test_index, dtype=np.int64).reshape(-1)
        if te.size < max(TOP) or te.min() < 0 or te.max() >= self.n or np.unique(te).size != te.size:
            raise ValueError(f"test_index: at least {max(TOP)} distinct node indices below {self.n}")
        self.test_index = te
        te32 = torch.tensor(te.astype(np.int32), device=device)
        self.index = ops.EvalIndex(torch.from_numpy(tree.depth.astype(np.int32)).to(device), te32, te32, tree.n_levels)
        self._ptr_host, self.anc_ptr, self.anc_nodes, self.anc_levels = ancestor_tables(tree, device)
        self.acc = torch.zeros(9, dtype=torch.float64, device=device)

    def scores(self, feats: torch.Tensor, *how) -> torch.Tensor:
        raise NotImplementedError

    @torch.no_grad()
    def add(self, feats: torch.Tensor, target: int, *how):
        """One batch of ONE class (the reference's test loader); returns the device outputs (pred [B, 20], top1 [B, 1], lv [B, n_levels])."""
        t = int(target)
        if not 0 <= t < self.n:
            raise ValueError(f"target {target} outside the {self.n} nodes")
        lv, top1, pred = ops.eval_rows(self.scores(feats, *how), self.index, max(TOP))
        o, e = self._ptr_host[t], self._ptr_host[t + 1]
        ops.eval_counters(pred, None, t, top1.view(-1), lv, self.anc_nodes[o:e], self.anc_levels[o:e], self.acc)
        return pred, top1, lv

    @torch.no_grad()
    def add_rows(self, feats: torch.Tensor, targets: torch.Tensor, *how):
        """One batch of MIXED classes: `targets` [B] on the device, node indices."""
        if not (torch.is_tensor(targets) and targets.is_cuda and targets.numel() == feats.shape[0]):
            raise ops._lib.HgrError("targets must be a device tensor with one node index per row")
        tg = targets.to(torch.int64).contiguous().view(-1)
        lv, top1, pred = ops.eval_rows(self.scores(feats, *how), self.index, max(TOP))
        ops.eval_counters_rows(pred, tg, top1.view(-1), lv, self.anc_ptr, self.anc_nodes, self.anc_levels, self.acc)
        return pred, top1, lv

    def counters(self) -> np.ndarray:
        return self.acc.cpu().numpy()

    def result(self) -> str:
        """The one host read: the metric string of `test()`."""
        return metric_string(self.counters())
