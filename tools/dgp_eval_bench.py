#!/usr/bin/env python3
"""Dev tool: one batch of the DGP scoring at ImageNet-21K scale on SYNTHETIC material (a generated 12-level DAG of 20 842 nodes of
which 1 000 are seen, K = 2048, batch 512; the ImageNet-21K material files are not part of the repository).  Times, in one process
and interleaved, per batch: the classifier product (ops.gemm_nt with the bias epilogue), hgr_dgp_score_rows alone beside its byte
floor (rows x n_cols x 2 B), the whole `DGPEvaluator.add()`, and - as the baseline - a torch-on-device restatement of the
reference's loop (evaluate_imagenet.py:79-150: half matmul with the ones column, the 1e-7 fill, one clone + index_fill + top-1 per
path node, the `>=` count), generous to it: no host read per batch, the `rest` index lists already on the device.
usage: dgp_eval_bench.py [n_nodes] [rounds] [batch]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from hgr_net_amd import ops, synth
from hgr_net_amd.baseline import dgp_eval

n_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 20842
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B = int(sys.argv[3]) if len(sys.argv) > 3 else 512
K, N_SEEN = 2048, min(1000, n_nodes // 2)
DEV = "cuda"

edges = synth.make_dag(n_nodes, 12, seed=7, multi_parent=0.03)
names = sorted({w for e in edges for w in e} - {"fall11"})
order = np.argsort(synth.uniform(0, "dgp.eval.bench.split", len(names)), kind="stable")
nodes = [names[i] for i in order]                                      # the seen classes lead, in no depth order
n = len(nodes)
rng = np.random.default_rng(0)
pred = torch.from_numpy((rng.standard_normal((n, K + 1)) * 0.02).astype(np.float32))
ev = dgp_eval.DGPEvaluator(edges, nodes, N_SEEN, pred, device=DEV)
tree = ev.tree
feat = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).half().to(DEV)
target = int(np.argmax(tree.depth))                                    # the longest path: the baseline's worst case, ours does not care
targets = torch.from_numpy(rng.integers(N_SEEN, n, B)).to(DEV)


def timeit(fn, it=20):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e3                                 # us


# ---- the reference's loop on torch ------------------------------------------------------------------------------------------------------
pv16 = pred.half().to(DEV)
ones = torch.ones((B, 1), dtype=torch.float16, device=DEV)
rest = {d: torch.from_numpy(np.nonzero(tree.depth != d)[0]).to(DEV) for d in range(tree.n_levels)}
top = torch.tensor(dgp_eval.TOP, device=DEV)
t_hits, t_acc = torch.zeros(5, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)


def torch_batch(t=target):
    table = torch.matmul(torch.cat([feat, ones], 1), pv16.t())
    table[:, :N_SEEN] = 1e-7
    path = tree.path(t)
    parent = torch.tensor(path, device=DEV)
    _, p1 = table.topk(1, 1)
    t_acc[0] += (p1 == parent[None, :]).sum()
    dict_path = torch.stack([table.clone().index_fill(1, rest[int(tree.depth[p])], -1).topk(1, 1)[1].squeeze(1) for p in path], 1)
    m = dict_path == parent[None, :]
    t_acc[1] += ((m[:, :-1] & m[:, 1:]).sum() / (len(path) - 1)) if len(path) > 1 else m.sum()
    t_acc[2] += m.sum() / len(path)
    rks = (table >= table[:, t:t + 1]).sum(1)
    t_hits.add_((rks[:, None] <= top[None, :]).sum(0))


# ---- ours, part by part ------------------------------------------------------------------------------------------------------------------
buf = ev._buffers(B)
tab = ev.table(feat)
res = {"n_nodes": n, "n_seen": N_SEEN, "k": K, "batch": B, "levels": tree.n_levels, "path_len_of_target": len(tree.path(target)),
       "material": "synthetic"}
parts = {"product_us": lambda: ev.table(feat),
         "score_rows_us": lambda: ops.dgp_score_rows(tab, ev.depth, tree.n_levels, N_SEEN, dgp_eval.FILL, target=target, n_cols=n,
                                                     k_pred=dgp_eval.K_PRED, out=buf["out"]),
         "score_rows_per_row_targets_us": lambda: ops.dgp_score_rows(tab, ev.depth, tree.n_levels, N_SEEN, dgp_eval.FILL, targets=targets,
                                                                     n_cols=n, k_pred=dgp_eval.K_PRED, out=buf["out"]),
         "add_us": lambda: ev.add(feat, target),
         "add_rows_us": lambda: ev.add_rows(feat, targets),
         "torch_reference_loop_us": torch_batch}
times = {k: [] for k in parts}
for _ in range(rounds):                                                 # interleaved: every route sees the same clocks and neighbours
    for k, fn in parts.items():
        times[k].append(timeit(fn))
for k, v in times.items():
    res[k] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
floor_bytes = B * n * 2
us = res["score_rows_us"]["median"]
res["score_rows_floor_MB"] = round(floor_bytes / 1e6, 2)
res["score_rows_GBps"] = round(floor_bytes / us / 1e3)
res["score_rows_frac_hbm_8TBps"] = round(floor_bytes / us / 1e3 / 8000, 3)
res["add_vs_torch"] = round(res["torch_reference_loop_us"]["median"] / res["add_us"]["median"], 2)
print(json.dumps(res))
