#!/usr/bin/env python3
"""Dev tool: one DGP training epoch at ImageNet-21K scale (synthetic 12-level DAG, 300 -> 2048 -> 2048 channels, 'd2048,d',
1 000 target rows): times `DGPTrainer.step`, every new launch on its own, prices the gathers against their byte floor, and
times - in the same process, interleaved - the reference's formulation on the same GPU (D torch.sparse.mm per layer under
autograd, nn.Dropout, torch.optim.Adam).  The inference forward is reported for scale.
usage: dgp_train_bench.py [n_nodes] [rounds]"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from hgr_net_amd import ops, synth
from hgr_net_amd.baseline import DGPTrainer, GCN_Dense_Att, dgp

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
C_IN, C, N_T = 300, 2048, 1000
dag = synth.make_dag(n, 12, seed=7, multi_parent=0.03)
names = ["fall11"] + sorted({w for e in dag for w in e} - {"fall11"})
idx = {w: i for i, w in enumerate(names)}
n = len(names)
es = dgp.fold_groups(dgp.group_edges(n, [(idx[p], idx[c]) for p, c in dag]), 4)
torch.manual_seed(0)
m = GCN_Dense_Att(n, es, C_IN, C, "d2048,d")
t0 = time.perf_counter(); tr = DGPTrainer(m); t_adj = time.perf_counter() - t0
x = torch.nn.functional.normalize(torch.randn(n, C_IN, device="cuda"))
rows = torch.randperm(n)[:N_T].to(torch.int32)
targets = torch.nn.functional.normalize(torch.randn(N_T, C, device="cuda"))


def timeit(fn, it=5):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it                                       # ms


# ---- the reference's formulation: gcn_dense_att.py on torch.sparse, autograd, torch.optim.Adam ---------------------------
def coo(edges, transpose):
    e = np.asarray(edges, np.int64)
    r, c = (e[:, 0], e[:, 1]) if transpose else (e[:, 1], e[:, 0])
    v = (1.0 / np.bincount(r, minlength=n)[r]).astype(np.float32)
    return torch.sparse_coo_tensor(torch.from_numpy(np.vstack([r, c])), torch.from_numpy(v), (n, n)).coalesce().cuda()


sets = [[coo(e, False) for e in es], [coo(e, True) for e in es]]
params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in m.state_dict().items()}
opt = torch.optim.Adam(params.values(), lr=1e-3, weight_decay=5e-4)
rows_l = rows.long().cuda()


def torch_epoch():
    h = x
    for k, name in enumerate(("conv1", "conv-last")):
        att = torch.softmax(params["a_att" if k == 0 else "r_att"], 0)
        support = torch.mm(torch.nn.functional.dropout(h, 0.5, True), params[name + ".w"]) + params[name + ".b"]
        out = None
        for i, adj in enumerate(sets[k]):
            y = torch.mm(adj, support) * att[i]
            out = y if out is None else out + y
        h = torch.nn.functional.leaky_relu(out, 0.2) if k == 0 else out
    out = torch.nn.functional.normalize(h)
    loss = ((out[rows_l] - targets) ** 2).sum() / (N_T * 2)
    opt.zero_grad()
    loss.backward()
    opt.step()


res = {"n": n, "pairs": [len(g) for g in es], "adjoint_build_s": round(t_adj, 2), "target_rows": N_T}
ours, theirs = [], []
for _ in range(rounds):                                                 # interleaved: both see the same clocks and neighbours
    ours.append(timeit(lambda: tr.step(x, rows, targets), 3))
    theirs.append(timeit(torch_epoch, 3))
res["epoch_ms"] = [round(v, 2) for v in ours]
res["torch_sparse_epoch_ms"] = [round(v, 2) for v in theirs]
res["epoch_vs_torch"] = round(float(np.median(theirs) / np.median(ours)), 2)
res["inference_forward_ms"] = round(timeit(lambda: m.eval()(x)), 3)

# ---- every new launch on its own ------------------------------------------------------------------------------------------
s, g, y = (torch.randn(n, C, device="cuda") for _ in range(3))
d_o, t = torch.empty_like(g), torch.empty_like(g)
bias = m.layers[1].b.data
for name, op, att, adj in (("a_side", m.a_op, torch.softmax(m.a_att.data, 0), tr.adj[0]), ("r_side", m.r_op, torch.softmax(m.r_att.data, 0), tr.adj[1])):
    p = torch.empty(n, op.D, device="cuda")
    ms = timeit(lambda: ops.csr_group_att_grad(s, op, bias, g, y, d_o, p, 0.2))
    floor = (op.nnz + 3 * n) * C * 4 + op.nnz * 9                       # gathered rows + G, Y read, dO written + edge data
    res[name + "_att_grad"] = {"us": round(ms * 1e3, 1), "nnz": op.nnz, "items": op.item_row.numel(), "split_rows": op.split_row.numel(),
                               "floor_GB": round(floor / 1e9, 3), "GBps": round(floor / ms / 1e6), "frac_hbm_8TBps": round(floor / ms / 1e6 / 8000, 3)}
    ms = timeit(lambda: adj.aggregate(g, att, None, t, 1.0, False))
    floor = (adj.nnz + n) * C * 4 + adj.nnz * 9 + 2 * adj.n_slots * C * 4
    res[name + "_adjoint_gather"] = {"us": round(ms * 1e3, 1), "items": adj.item_row.numel(), "split_rows": adj.split_row.numel(),
                                     "floor_GB": round(floor / 1e9, 3), "GBps": round(floor / ms / 1e6), "frac_hbm_8TBps": round(floor / ms / 1e6 / 8000, 3)}
loss_rows, loss = torch.empty(N_T, device="cuda"), torch.empty(1, device="cuda")
rows_d = rows.cuda()
res["loss_head_us"] = round(timeit(lambda: ops.dgp_loss_head(s, rows_d, targets, loss_rows, loss, d_o)) * 1e3, 1)
res["dropout_2048_us"] = round(timeit(lambda: ops.dropout_counter(s, d_o, 0, 1, 1)) * 1e3, 1)
res["dropout_300_us"] = round(timeit(lambda: ops.dropout_counter(x, torch.empty_like(x), 0, 1, 0)) * 1e3, 1)
w = m.layers[1].w.data
mm, vv, gw = torch.zeros_like(w), torch.zeros_like(w), torch.randn_like(w)
res["adam_l2_2048x2048_us"] = round(timeit(lambda: ops.adam_l2(w, gw, mm, vv, 1e-3, 1, wd=5e-4)) * 1e3, 1)
res["product_S_us"] = round(timeit(lambda: ops.matmul_f32(s, w, t)) * 1e3, 1)
res["product_dW_us"] = round(timeit(lambda: ops.matmul_f32(s.t(), g, gw)) * 1e3, 1)
res["product_dX_us"] = round(timeit(lambda: ops.matmul_f32(g, w.t(), t)) * 1e3, 1)
print(json.dumps(res))
