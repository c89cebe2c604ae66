#!/usr/bin/env python3
"""Dev tool: what the hierarchy report (Evaluator(model, report=True): one hgr_eval_report_rows launch per step, on the tail's stream
behind hgr_eval_counters_rows) costs the evaluation loop.  ViT-B/32, N = 21 841, batch 512, synthetic images, full batches of mixed
classes (Evaluator.add_images_rows: the two-graph pipelined step); report off and report on in ONE process, interleaved round by
round, a pass ends in the counters' (and the table's) read-back.  Compare the two routes of one run only: boxes differ by several
per cent.

    hier_report_bench.py [--steps 60] [--rounds 5] [--batch 512] [--kernel-iters 200]

Also times the two row kernels alone (hgr_eval_counters_rows, hgr_eval_report_rows) on the outputs of one step, back to back on one
stream between two events.  Prints one JSON line.
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
tmp = tempfile.mkdtemp(prefix="hgr_hier_")
gp = os.path.join(tmp, "graph.json")
json.dump(edges, open(gp, "w"))
opts = types.SimpleNamespace(device="cuda", folder=tmp, exp_name="HGR", weights="equal", out_ratio=0.25, in_ratio=0.5, from_epoch=-1,
                             graph_path=gp, arch=args.arch, fetch=False, load=False, load_path="none", scale=1.0, num_compare=256, k=1,
                             sample_strategy="topk", weighting="both", train_dtype="bf16", n_ctx=0)
model = tree_model(opts, splits["all"], splits["rest"], node_tokens=tokens, clip_model=build_model(synth.clip_state_dict(cfg, 0)).to("cuda"))
model.update_classifier()
base = synth.images(args.batch, cfg["image_resolution"], 1234).to("cuda")
bufs = [base, base.flip(0).contiguous()]
te = torch.tensor(model.test_index.cpu().tolist(), dtype=torch.int64)
g = torch.Generator().manual_seed(0)
labels = [te[torch.randint(0, len(te), (args.batch,), generator=g)].to("cuda") for _ in range(2)]      # mixed classes, every row its own


def run(report):
    ev = evaluate.Evaluator(model, report=True) if report else evaluate.Evaluator(model)
    for s in range(args.steps):
        ev.add_images_rows(bufs[s & 1], labels[s & 1])
    c = ev.counters()
    return c, (ev.report_table() if report else None)


routes = {"report_off": False, "report_on": True}
secs, last = {k: [] for k in routes}, {}
for r in range(args.rounds + 1):                     # round 0 warms both routes up (graph captures) and is dropped
    for k, rep in routes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[k] = run(rep)
        if r:
            secs[k].append(time.perf_counter() - t0)
total = args.steps * args.batch
result = {"arch": args.arch, "nodes": args.nodes, "batch": args.batch, "steps": args.steps, "rounds": args.rounds}
for k in routes:
    best, med = min(secs[k]), sorted(secs[k])[len(secs[k]) // 2]
    result[k] = {"images_per_s_best_med": [round(total / best, 1), round(total / med, 1)],
                 "ms_per_step_best_med": [round(best / args.steps * 1e3, 4), round(med / args.steps * 1e3, 4)]}
table = last["report_on"][1]
result["counters_equal"] = last["report_on"][0] == last["report_off"][0]
result["table_rows"] = int(evaluate.report_from_table(table)["num_sample"])

# the two row kernels alone, on the outputs of one step
ev = evaluate.Evaluator(model, report=True)
model.join_tail()
lv, p1, pred = ops.eval_rows(model(bufs[0], None), ev.index, max(evaluate.TOPK))
p1 = p1.view(-1)
csr = ev._ancestor_csr()
kern = {"hgr_eval_counters_rows": lambda: ops.eval_counters_rows(pred, labels[0], p1, lv, *csr, ev.acc),
        "hgr_eval_report_rows": lambda: ops.eval_report_rows(pred, labels[0], p1, lv, *csr, ev.report)}
for name, fn in kern.items():
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.kernel_iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    result[name + "_us_back_to_back"] = round(a.elapsed_time(b) / args.kernel_iters * 1e3, 2)
print(json.dumps(result), flush=True)
