#!/usr/bin/env python3
"""Dev tool: the evaluation loop over classes of UNEQUAL size, one class per batch (the group loaders' contract, what evaluate.test does
by default) against full batches packed from several classes (opts.pack_batches: dataset.packing.PackedBatches + Evaluator.add_images_rows).
ViT-B/32, N = 21 841, batch 512, synthetic images; both routes in ONE process, interleaved round by round, over the same list of source
batches (a class of s images = s // 512 full batches and one remainder).

    pack_eval_bench.py [--sizes-json FILE] [--classes 32] [--seed 0] [--rounds 3] [--batch 512]

Two lists are run: the ragged one and a uniform one (every class exactly one full batch), which shows what the packer's row copy costs
when nothing needs packing.  Both routes read their images from the same two recycled device buffers (views of them for partial
batches), i.e. the group route at its best: its graphs are keyed by the input address inside one shape.

THE DEFAULT RAGGED LIST IS AN ASSUMPTION.  The class sizes of the real unseen split (11 171 023 images over ~20 K classes, a few hundred
per class) are not available offline; the default draws --classes sizes from a log-normal with median 400 and sigma 0.8, clipped to
1 .. 1500, seeded.  Quote numbers from it with that caveat, or pass the real sizes with --sizes-json (a JSON list of integers).

Prints one JSON line: per list and route images/s and ms per image (best and median round) and the HIP-graph captures of one pass.
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
import numpy as np
import torch

from hgr_net_amd import evaluate, synth
from hgr_net_amd.clip.model import build_model
from hgr_net_amd.dataset.packing import PackedBatches
from hgr_net_amd.hierarchy import build_hierarchy
from hgr_net_amd.model import tree_model

ap = argparse.ArgumentParser()
ap.add_argument("--sizes-json", default=None)
ap.add_argument("--classes", type=int, default=32)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--arch", default="ViT-B/32")
ap.add_argument("--nodes", type=int, default=21841)
args = ap.parse_args()

if args.sizes_json:
    ragged = [int(s) for s in json.load(open(args.sizes_json))]
else:
    rng = np.random.default_rng(args.seed)
    ragged = np.clip(np.round(rng.lognormal(np.log(400.0), 0.8, args.classes)), 1, 1500).astype(int).tolist()
lists = {"ragged": ragged, "uniform": [args.batch] * len(ragged)}

cfg = synth.CLIP_CONFIGS[args.arch]
edges = synth.make_dag(args.nodes, depth=12, seed=7, multi_parent=0.03)
h = build_hierarchy(edges)
n_test = int(round(args.nodes * 13442 / 20842))
splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], args.nodes - n_test, n_test, 13)
tokens = synth.make_tokens(args.nodes, 11, cfg["vocab_size"], n_ctx=0)
tmp = tempfile.mkdtemp(prefix="hgr_pack_")
gp = os.path.join(tmp, "graph.json")
json.dump(edges, open(gp, "w"))
opts = types.SimpleNamespace(device="cuda", folder=tmp, exp_name="HGR", weights="equal", out_ratio=0.25, in_ratio=0.5, from_epoch=-1,
                             graph_path=gp, arch=args.arch, fetch=False, load=False, load_path="none", scale=1.0, num_compare=256, k=1,
                             sample_strategy="topk", weighting="both", train_dtype="bf16", n_ctx=0)
model = tree_model(opts, splits["all"], splits["rest"], node_tokens=tokens, clip_model=build_model(synth.clip_state_dict(cfg, 0)).to("cuda"))
model.update_classifier()
base = synth.images(args.batch, cfg["image_resolution"], 1234).to("cuda")
bufs = [base, base.flip(0).contiguous()]
te = model.test_index.cpu().tolist()

captures = [0]


class _CountingCapture(torch.cuda.graph):
    def __enter__(self):
        captures[0] += 1
        return super().__enter__()


torch.cuda.graph = _CountingCapture          # tree_model looks torch.cuda.graph up at every capture


def source(sizes):
    """The batch dicts a group loader hands out for these class sizes: device images, host labels, one class per batch."""
    out = []
    for c, s in enumerate(sizes):
        label = te[(7 * c + 3) % len(te)]
        for o in range(0, s, args.batch):
            n = min(args.batch, s - o)
            out.append({"img": bufs[len(out) & 1][:n][None], "label": torch.full((1, n), label, dtype=torch.long)})
    return out


def run_groups(src):                         # the loop of evaluate.test, flag off
    ev = evaluate.Evaluator(model)
    for d in src:
        imgs, targets = d["img"].to("cuda", non_blocking=True)[0], d["label"].to("cuda", non_blocking=True)[0]
        ev.add_images(imgs, int(d["label"][0][0]), targets)
    return ev.counters()


def run_packed(src):                         # the loop of evaluate.test with opts.pack_batches
    ev = evaluate.Evaluator(model)
    for d in PackedBatches(src, args.batch, "cuda"):
        ev.add_images_rows(d["img"][0], d["label"][0])
    return ev.counters()


routes = {"groups": run_groups, "packed": run_packed}
result = {"arch": args.arch, "nodes": args.nodes, "batch": args.batch, "rounds": args.rounds,
          "sizes_source": args.sizes_json or f"ASSUMED: lognormal(median 400, sigma 0.8) clipped to 1..1500, seed {args.seed}", "ragged_sizes": ragged}
for name, sizes in lists.items():
    src, total = source(sizes), sum(sizes)
    secs, caps, counters = {k: [] for k in routes}, {}, {}
    for r in range(args.rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            captures[0] = 0
            t0 = time.perf_counter()
            counters[k] = fn(src)            # counters() reads the device: the pass has finished
            secs[k].append(time.perf_counter() - t0)
            caps[k] = captures[0]
    result[name] = {"images": total, "source_batches": len(src), "packed_batches": -(-total // args.batch),
                    "num_sample_equal": counters["groups"]["num_sample"] == counters["packed"]["num_sample"] == total}
    for k in routes:
        best, med = min(secs[k]), sorted(secs[k])[len(secs[k]) // 2]
        result[name][k] = {"images_per_s_best_med": [round(total / best, 1), round(total / med, 1)],
                           "ms_per_image_best_med": [round(best / total * 1e3, 5), round(med / total * 1e3, 5)],
                           "graph_captures_per_pass": caps[k]}
print(json.dumps(result), flush=True)
