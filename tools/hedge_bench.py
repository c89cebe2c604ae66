#!/usr/bin/env python3
"""Dev tool: what hedged predictions (Evaluator(model, hedge=(...)): one hgr_subtree_hedge launch per step behind hgr_eval_rows and one
hgr_hedge_counters_rows behind the counters) cost the evaluation loop.  ViT-B/32, N = 21 841, synthetic DAG of depth 12, batch 512,
synthetic images, one-class batches as evaluate.test's loop feeds them; two routes in ONE process, interleaved round by round, a
pass ends in the counters' read-back:

    B  flat_logits   flat decoding on the logits route (add_batch(model(imgs))): route B of path_decode_bench.py - the baseline,
                     because a hedge leaves the fused route
    H  hedge         the same with 5 thresholds

Compare the routes of one run only: boxes differ by several per cent.

    hedge_bench.py [--steps 60] [--rounds 5] [--batch 512] [--kernel-iters 200] [--hedge 0.1,0.25,0.5,0.75,0.9]

Also times hgr_subtree_hedge alone on the logits of one step (back to back on one stream between two events) beside its byte floor:
one read of the logits plus the CSR over the achievable HBM rate.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from hgr_net_amd import evaluate, ops, synth
from hgr_net_amd.clip.model import build_model
from hgr_net_amd.hierarchy import build_hierarchy
from hgr_net_amd.model import tree_model

HBM_ACHIEVABLE = 6.3e12          # B/s: what a streaming copy reaches on an MI355X (8 TB/s peak)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--arch", default="ViT-B/32")
ap.add_argument("--nodes", type=int, default=21841)
ap.add_argument("--hedge", type=evaluate.parse_hedge, default=(0.1, 0.25, 0.5, 0.75, 0.9))
args = ap.parse_args()

cfg = synth.CLIP_CONFIGS[args.arch]
edges = synth.make_dag(args.nodes, depth=12, seed=7, multi_parent=0.03)
h = build_hierarchy(edges)
n_test = int(round(args.nodes * 13442 / 20842))
splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], args.nodes - n_test, n_test, 13)
tokens = synth.make_tokens(args.nodes, 11, cfg["vocab_size"], n_ctx=0)
tmp = tempfile.mkdtemp(prefix="hgr_hedge_")
gp = os.path.join(tmp, "graph.json")
json.dump(edges, open(gp, "w"))
opts = types.SimpleNamespace(device="cuda", folder=tmp, exp_name="HGR", weights="adaptive", out_ratio=0.25, in_ratio=0.5, from_epoch=-1,
                             graph_path=gp, arch=args.arch, fetch=False, load=False, load_path="none", scale=1.0, num_compare=256, k=1,
                             sample_strategy="topk", weighting="both", train_dtype="bf16", n_ctx=0)
model = tree_model(opts, splits["all"], splits["rest"], node_tokens=tokens, clip_model=build_model(synth.clip_state_dict(cfg, 0)).to("cuda"))
model.update_classifier()
base = synth.images(args.batch, cfg["image_resolution"], 1234).to("cuda")
bufs = [base, base.flip(0).contiguous()]
classes = [int(c) for c in model.test_index.cpu().tolist()[:2]]
labels = [torch.full((args.batch,), c, dtype=torch.int64, device="cuda") for c in classes]

# one Evaluator per route, built ahead of the clock (its index and the ancestor CSR are host work of a whole run, not of a step)
evs = {"flat_logits": evaluate.Evaluator(model), "hedge": evaluate.Evaluator(model, hedge=args.hedge)}
assert not evs["hedge"].fused_ok()


def run(route):
    ev = evs[route]
    ev.acc.zero_()
    if ev.hedge_tab is not None:
        ev.hedge_tab.zero_()
    for s in range(args.steps):
        imgs, target, targets = bufs[s & 1], classes[s & 1], labels[s & 1]
        ev.add_batch(model(imgs, targets, static_output=True), target, targets, want_outputs=False)
    return ev.counters()


routes = tuple(evs)
secs, last = {k: [] for k in routes}, {}
for r in range(args.rounds + 1):                     # round 0 warms every route up (graph captures) and is dropped
    for k in routes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[k] = run(k)
        if r:
            secs[k].append(time.perf_counter() - t0)
total = args.steps * args.batch
ev = evs["hedge"]
result = {"arch": args.arch, "nodes": args.nodes, "batch": args.batch, "steps": args.steps, "rounds": args.rounds, "hedge": list(args.hedge),
          "temperature": ev.hedge_temperature, "max_path": max(len(p) for p in model.c2p) + 1}
for k in routes:
    best, med = min(secs[k]), sorted(secs[k])[len(secs[k]) // 2]
    result[k] = {"images_per_s_best_med": [round(total / best, 1), round(total / med, 1)],
                 "ms_per_step_best_med": [round(best / args.steps * 1e3, 4), round(med / args.steps * 1e3, 4)]}
result["counters_equal"] = last["flat_logits"] == last["hedge"]
rep = ev.hedge_dict()
result["hedge_rows"] = rep["by_threshold"][0]["rows"]
result["abstain_pct"] = [round(e["abstain_pct"], 2) for e in rep["by_threshold"]]
result["mean_pick_depth"] = [round(e["mean_pick_depth"], 3) for e in rep["by_threshold"]]

# hgr_subtree_hedge alone, on the logits of one step
model.join_tail()
logits = model(bufs[0], None)
ptr, nodes, _ = ev._ancestor_csr()
rows, t = logits.shape[0], len(args.hedge)
pick = torch.empty((rows, t), dtype=torch.int32, device="cuda")
pmass = torch.empty((rows, t), dtype=torch.float32, device="cuda")
# eight logits buffers in rotation: 8 x 45 MB at the default shape, more than the 256 MB Infinity Cache holds, so that a launch does
# not find its logits in a cache from the launch before
copies = [logits.clone() for _ in range(8)]


def launch(i):
    ops.subtree_hedge(copies[i & 7], ev.index.test_pos, ptr, nodes, ev.hedge_temperature, ev._hedge_thr, pick, pmass)


for i in range(16):
    launch(i)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
a.record()
for i in range(args.kernel_iters):
    launch(i)
b.record()
torch.cuda.synchronize()
us = a.elapsed_time(b) / args.kernel_iters * 1e3
byts = rows * args.nodes * 4 + (ptr.numel() + nodes.numel() + args.nodes) * 4
result["hgr_subtree_hedge_us_back_to_back"] = round(us, 2)
result["byte_floor_us"] = round(byts / HBM_ACHIEVABLE * 1e6, 2)
result["floor_bytes_per_s"] = round(byts / (us * 1e-6), 0)
result["path_ids_per_row"] = int(nodes.numel())
print(json.dumps(result), flush=True)
