#!/usr/bin/env python3
"""Dev tool: what candidate sets (Evaluator(model, sets={...}): one hgr_set_ranks launch per step behind hgr_eval_rows and one
hgr_set_counters_rows behind the counters) cost the evaluation loop.  ViT-B/32, N = 21 841, synthetic DAG of depth 12, batch 512,
synthetic images, one-class batches as evaluate.test's loop feeds them; four routes in ONE process, interleaved round by round, a
pass ends in the counters' read-back:

    F   fused         the default route (add_images: the logits GEMM with the evaluation in its epilogue) - what a run without
                      candidate sets takes, and what a run with them gives up
    B   flat_logits   the logits route without sets (add_batch(model(imgs))) - the baseline, because the sets leave the fused route
    S4  sets4         the logits route with 4 candidate sets
    S16 sets16        the logits route with 16 candidate sets

Compare the routes of one run only: boxes differ by several per cent.  The feature replaces one whole evaluation run per set, so its
condition is S4 < 2 B; the tool prints both numbers and the verdict.

    eval_sets_bench.py [--steps 60] [--rounds 5] [--batch 512] [--kernel-iters 200]

Also times hgr_set_ranks alone (4 and 16 sets) on the logits of one step, back to back on one stream between two events, beside its
byte floor: rows x n_nodes x 8 B (one read of the scores and of the member words) over the achievable HBM rate.  Prints one JSON line.
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
args = ap.parse_args()

cfg = synth.CLIP_CONFIGS[args.arch]
edges = synth.make_dag(args.nodes, depth=12, seed=7, multi_parent=0.03)
h = build_hierarchy(edges)
n_test = int(round(args.nodes * 13442 / 20842))
splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], args.nodes - n_test, n_test, 13)
tokens = synth.make_tokens(args.nodes, 11, cfg["vocab_size"], n_ctx=0)
tmp = tempfile.mkdtemp(prefix="hgr_sets_")
gp = os.path.join(tmp, "graph.json")
json.dump(edges, open(gp, "w"))
opts = types.SimpleNamespace(device="cuda", folder=tmp, exp_name="HGR", weights="adaptive", out_ratio=0.25, in_ratio=0.5, from_epoch=-1,
                             graph_path=gp, arch=args.arch, fetch=False, load=False, load_path="none", scale=1.0, num_compare=256, k=1,
                             sample_strategy="topk", weighting="both", train_dtype="bf16", n_ctx=0)
model = tree_model(opts, splits["all"], splits["rest"], node_tokens=tokens, clip_model=build_model(synth.clip_state_dict(cfg, 0)).to("cuda"))
model.update_classifier()
base = synth.images(args.batch, cfg["image_resolution"], 1234).to("cuda")
bufs = [base, base.flip(0).contiguous()]
test = [int(c) for c in model.test_index.cpu().tolist()]
seen = set(test)
train = [int(c) for c in model.train_index.cpu().tolist() if int(c) not in seen]
classes = test[:2]
labels = [torch.full((args.batch,), c, dtype=torch.int64, device="cuda") for c in classes]


def make_sets(count):
    """The shape of the paper's table: the test set, nested subsets of it (2-hops inside 3-hops), and each with the seen classes added."""
    out = {"rest": test, "rest+train": test + train}
    i = 2
    while len(out) < count:
        sub = test[:max(len(test) // i, 2)]
        out[f"hop{i}"] = sub
        if len(out) < count:
            out[f"hop{i}+train"] = sub + train
        i += 1
    return out


# one Evaluator per route, built ahead of the clock (its index and the ancestor CSR are host work of a whole run, not of a step)
evs = {"fused": evaluate.Evaluator(model), "flat_logits": evaluate.Evaluator(model), "sets4": evaluate.Evaluator(model, sets=make_sets(4)),
       "sets16": evaluate.Evaluator(model, sets=make_sets(16))}
assert evs["fused"].fused_ok() and not evs["sets4"].fused_ok()


def run(route):
    ev = evs[route]
    ev.acc.zero_()
    if ev.sets_tab is not None:
        ev.sets_tab.zero_()
    for s in range(args.steps):
        imgs, target, targets = bufs[s & 1], classes[s & 1], labels[s & 1]
        if route == "fused":
            ev.add_images(imgs, target, targets)
        else:
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
result = {"arch": args.arch, "nodes": args.nodes, "batch": args.batch, "steps": args.steps, "rounds": args.rounds}
for k in routes:
    best, med = min(secs[k]), sorted(secs[k])[len(secs[k]) // 2]
    result[k] = {"images_per_s_best_med": [round(total / best, 1), round(total / med, 1)],
                 "ms_per_step_best_med": [round(best / args.steps * 1e3, 4), round(med / args.steps * 1e3, 4)]}
result["counters_equal"] = all(last[k] == last["flat_logits"] for k in routes)
b, s4 = result["flat_logits"]["ms_per_step_best_med"][1], result["sets4"]["ms_per_step_best_med"][1]
result["sets4_over_flat_logits"] = round(s4 / b, 4)
result["condition_sets4_below_twice_flat_logits"] = bool(s4 < 2.0 * b)
rep = evs["sets16"].sets_dict()["sets"]
result["sets16_rows"] = [e["num_sample"] for e in rep]
result["sets16_classes"] = [e["classes"] for e in rep]

# hgr_set_ranks alone, on the logits of one step
model.join_tail()
logits = model(bufs[0], None)
rows = logits.shape[0]
# eight logits buffers in rotation: 8 x 45 MB at the default shape, more than the 256 MB Infinity Cache holds, so that a launch does
# not find its logits in a cache from the launch before
copies = [logits.clone() for _ in range(8)]
result["byte_floor_us"] = round(rows * args.nodes * 8 / HBM_ACHIEVABLE * 1e6, 2)
for name in ("sets4", "sets16"):
    ix = evs[name].sets
    rank = torch.empty((rows, ix.n_sets), dtype=torch.int32, device="cuda")
    top1 = torch.empty((rows, ix.n_sets), dtype=torch.int32, device="cuda")
    for i in range(16):
        ops.set_ranks(copies[i & 7], ix, labels[0], rank, top1)
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(args.kernel_iters):
        ops.set_ranks(copies[i & 7], ix, labels[0], rank, top1)
    e.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(e) / args.kernel_iters * 1e3
    result[f"hgr_set_ranks_{ix.n_sets}_us_back_to_back"] = round(us, 2)
    result[f"hgr_set_ranks_{ix.n_sets}_floor_bytes_per_s"] = round(rows * args.nodes * 8 / (us * 1e-6), 0)
print(json.dumps(result), flush=True)
