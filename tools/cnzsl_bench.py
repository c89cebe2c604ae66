#!/usr/bin/env python3
"""Dev tool: the CNZSL baseline at the reference's sizes - one training step (S = 1 000 seen classes, A = 1 024, H = 1 024,
P = 2 048, B = 256) and one evaluation batch (N = 20 842 nodes, B = 256) - timed beside the same arithmetic written in torch ops
(autograd + torch.optim.Adam; topk + one index_fill / arg-max per path level, the reference's loop) on the same GPU, in one
process, the two routes alternating call by call; and the chain kernels on their own beside their byte floor.  Every figure is the
median of `rounds` device-event timings after `warmup` calls.  Prints one JSON line.
usage: cnzsl_bench.py [rounds] [warmup]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from hgr_net_amd import ops, synth
from hgr_net_amd.baseline import cnzsl, dgp_eval

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 60
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 10
assert rounds >= 50 and warmup >= 10 and torch.cuda.is_available()
S, A, H, P, B, N = 1000, 1024, 1024, 2048, 256, 20842
dev = "cuda:0"


def interleaved(fns: dict) -> dict:
    """Median ms of every route, the routes alternating call by call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e))
    return {k: float(np.median(v)) for k, v in times.items()}


# ---- one training step ---------------------------------------------------------------------------------------------------------------------
sd = cnzsl.synth_state(1, A, H, P)
model = cnzsl.CNZSLModel(A, H, P, device=dev)
model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
trainer = cnzsl.CNZSLTrainer(model)
attrs = torch.from_numpy(cnzsl.synth_rows(1, "bench.attrs", S, A)).to(dev)
feats = torch.from_numpy(cnzsl.synth_rows(1, "bench.feats", B, P)).to(dev)
labels = torch.from_numpy(synth.randint(1, "bench.labels", B, 0, S)).to(dev)

tp = {k: torch.nn.Parameter(torch.from_numpy(sd[k]).to(dev)) for k in cnzsl.TRAINABLE}
run = [torch.from_numpy(sd[k]).to(dev) for k in cnzsl.RUNNING]
opt = torch.optim.Adam(tp.values(), lr=1e-4, weight_decay=1e-4)


def torch_step():
    global run
    h1 = torch.relu(attrs @ tp["model.0.weight"].t() + tp["model.0.bias"])
    c, _, _, run = cnzsl.std_chain_host(h1 @ tp["model.2.weight"].t(), tp["model.2.bias"], run, True)
    protos = torch.relu(c @ tp["model.6.weight"].t() + tp["model.6.bias"])
    loss = torch.nn.functional.cross_entropy(cnzsl.logits_host(protos, feats), labels)
    opt.zero_grad()
    loss.backward()
    opt.step()


res = {"rounds": rounds, "warmup": warmup, "train_shape": {"S": S, "A": A, "H": H, "P": P, "B": B}}
t = interleaved({"ours": lambda: trainer.step(feats, labels, attrs), "torch": torch_step})
res["train_step_ms"] = {k: round(v, 4) for k, v in t.items()}
res["train_step_torch_over_ours"] = round(t["torch"] / t["ours"], 3)

# ---- the chain kernels beside their byte floor -------------------------------------------------------------------------------------------------
z, dc = torch.randn(S, H, device=dev), torch.randn(S, H, device=dev)
c, a, dz = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
stats, dbias, bias = torch.empty(4, H, device=dev), torch.empty(H, device=dev), torch.zeros(H, device=dev)
rn = [torch.zeros(H, device=dev), torch.ones(H, device=dev), torch.zeros(H, device=dev), torch.ones(H, device=dev)]
zt = z.clone().requires_grad_(True)


def torch_chain():
    cc, _, _, _ = cnzsl.std_chain_host(zt, bias, None, True)
    cc.backward(dc)
    zt.grad = None


t = interleaved({"fwd": lambda: ops.cnzsl_std_chain_fwd(z, bias, rn, c, a, stats),
                 "bwd": lambda: ops.cnzsl_std_chain_bwd(dc, a, z, bias, stats, dz, dbias),
                 "torch_fwd_bwd": torch_chain})
for k, floor in (("fwd", 3 * S * H * 4), ("bwd", 4 * S * H * 4)):           # z read, a and c written; dc, a, z read, dz written
    res["chain_" + k] = {"us": round(t[k] * 1e3, 2), "floor_bytes": floor, "GBps_at_floor": round(floor / t[k] / 1e6, 1)}
res["chain_torch_fwd_bwd_us"] = round(t["torch_fwd_bwd"] * 1e3, 2)

# ---- one evaluation batch ------------------------------------------------------------------------------------------------------------------------
edges = synth.make_dag(N, 12, seed=7, multi_parent=0.03)
h_nodes = sorted({w for e in edges for w in e} - {synth.ROOT})
tree = dgp_eval.build_list_tree(edges, h_nodes)
n_seen = 1000
test_index = np.arange(n_seen, len(h_nodes))
all_attrs = torch.from_numpy(cnzsl.synth_rows(2, "bench.all_attrs", len(h_nodes), A)).to(dev)
ev = cnzsl.CNZSLEvaluator(edges, h_nodes, test_index, model.eval(), all_attrs, tree=tree)
target = int(test_index[np.argmax(tree.depth[test_index])])                 # a deepest class: the longest path
path = tree.path(target)
te = torch.from_numpy(test_index).to(dev)
rest = [torch.from_numpy(np.nonzero(tree.depth != tree.depth[q])[0]).to(dev) for q in path]
pn = ev.pn


def torch_eval():
    xn = feats / feats.norm(dim=1, keepdim=True)
    logits = 25.0 * xn @ pn.t()
    sub = logits[:, te]
    picks = [te[sub.topk(20, 1)[1]], te[sub.topk(1, 1)[1]]]
    for r in rest:                                                          # cnzsl.py:264-277, one level of the target's path each
        picks.append(te[logits.index_fill(1, r, -1)[:, te].topk(1, 1)[1]])
    return picks


t = interleaved({"ours": lambda: ev.add(feats, target), "torch": torch_eval})
res["eval_shape"] = {"N": len(h_nodes), "B": B, "path_levels": len(path)}
res["eval_batch_ms"] = {k: round(v, 4) for k, v in t.items()}
res["eval_batch_torch_over_ours"] = round(t["torch"] / t["ours"], 3)
print(json.dumps(res))
