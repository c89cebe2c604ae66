"""`python -m hgr_net_amd.baseline.train_cnzsl`: the command line of the reference's baseline/CNZSL/cnzsl.py on the device trainer
and evaluator (`cnzsl.CNZSLTrainer`, `cnzsl.CNZSLEvaluator`), on CACHED image features.

The reference recomputes ResNet-50 features in every step and reads its attributes from `text_feats.json`; here both are files:
`--features FILE.npz` (the DGP evaluator's format: one [n_i, P] array per wnid) and `--attributes FILE` (.npz / .json, [N, A] in
node order - seen classes first, then the graph's nodes in order of appearance - or a list of chunks as `text_feats.json` is
read).  `--synthetic N` needs no file.  Training batches are single-class groups, as the reference's loaders yield them;
checkpoints `FILE_PATH_{epoch}` are written for epoch > 5 in the reference's state_dict schema; the loss lines and the metric line
are the reference's.  Where the reference needs a second run with `--train False` to score, this script scores after training too.
The candidate classes of `--data_train` / `--data_test` are looked up in `--split_path` (the reference reads them from a second,
hard-coded split file)."""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Sequence

import numpy as np
import torch

HID_DIM = 1024                                   # cnzsl.py:343
SYN_ATTR, SYN_HID, SYN_PROTO, SYN_TRAIN_ROWS, SYN_TEST_ROWS = 64, 128, 256, 8, 4


def _bool(s):
    if s in ("True", "False"):
        return s == "True"
    raise argparse.ArgumentTypeError("True or False")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m hgr_net_amd.baseline.train_cnzsl", description="CNZSL baseline on cached features")
    p.add_argument("--print_freq", default=1, type=int)
    p.add_argument("--data_train", default="train", type=str)
    p.add_argument("--data_test", default="rest", type=str, help="rest,all")
    p.add_argument("--graph_path", default="data/process_results/graph_edges_cls.json", type=str)
    p.add_argument("--split_path", default="data/process_results/splits_for_tree.json", type=str)
    p.add_argument("--batch_size", default=256, type=int)
    p.add_argument("--test_batch_size", default=256, type=int)
    p.add_argument("--epoch", default=9, type=int)
    p.add_argument("--attr", default="transformer", type=str, help="w2v, transformer")
    p.add_argument("--load", default=False, action="store_true")
    p.add_argument("--file_path", default="cnzsl/cnzsl_", type=str)
    p.add_argument("--train", default=True, type=_bool)
    p.add_argument("--cn", default=True, type=_bool)
    p.add_argument("--init", default=True, type=_bool)
    p.add_argument("--attributes", default=None, metavar="FILE", help=".npz / .json: [N, A] in node order, or a list of chunks")
    p.add_argument("--features", default=None, metavar="FILE.npz", help="one [n_i, P] array per wnid")
    p.add_argument("--seed", default=1, type=int)
    p.add_argument("--synthetic", default=None, type=int, metavar="N", help="generated graph, attributes and features; needs no file")
    args = p.parse_args(argv)
    if args.batch_size < 1 or args.test_batch_size < 1 or args.epoch < 0 or args.print_freq < 1:
        p.error("batch sizes and --print_freq must be positive, --epoch non-negative")
    if args.synthetic is not None and args.synthetic < 100:
        p.error("--synthetic N: at least 100 nodes")
    if args.synthetic is None and (args.attributes is None or args.features is None):
        p.error("--attributes and --features are needed without --synthetic")
    return args


def ordered_nodes(graph_edges, train_classes: Sequence[str]) -> List[str]:
    """gen_tree's node order (cnzsl.py:77-89): the seen classes, then the graph's other nodes in order of appearance."""
    from ..hierarchy import build_hierarchy
    seen = set(train_classes)
    return list(train_classes) + [w for w in build_hierarchy(graph_edges).nodes if w not in seen]


def load_attributes(path: str) -> np.ndarray:
    """fp32 [N, A]: an .npz (its 'attrs' array, or its only one), or a .json holding the matrix or a list of [n_i, A] chunks."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            a = np.asarray(z["attrs"] if "attrs" in z.files else z[z.files[0]])
    else:
        obj = json.load(open(path, "r"))
        a = np.concatenate([np.asarray(c, dtype=np.float32) for c in obj], 0) if isinstance(obj[0][0], list) else np.asarray(obj)
    if a.ndim != 2 or a.dtype.kind != "f":
        raise ValueError(f"{path}: attributes are {a.dtype} {a.shape}, expected a float [N, A] matrix")
    return np.ascontiguousarray(a.astype(np.float32))


def synthetic_material(n_nodes: int, seed: int):
    """(graph_edges, splits, attrs [N, A] in node order, features {wnid: rows}) from hgr_net_amd.synth: every class is a random
    direction plus noise, so a few steps already lower the loss."""
    from .. import synth
    from ..hierarchy import build_hierarchy
    from . import cnzsl
    edges = synth.make_dag(n_nodes, 10, seed=7 + seed, multi_parent=0.03)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], n_nodes // 4, n_nodes // 4, 13 + seed)
    nodes = ordered_nodes(edges, splits["train"])
    attrs = cnzsl.synth_rows(seed, "cnzsl.synthetic.attrs", len(nodes), SYN_ATTR)
    feats: Dict[str, np.ndarray] = {}
    for key, rows in (("train", SYN_TRAIN_ROWS), ("rest", SYN_TEST_ROWS)):
        for w in splits[key]:
            base = cnzsl.synth_rows(seed, "cnzsl.synthetic.base." + w, 1, SYN_PROTO)
            feats[w] = base + 0.5 * cnzsl.synth_rows(seed, "cnzsl.synthetic.noise." + w, rows, SYN_PROTO)
    return edges, splits, attrs, feats


def class_batches(features: Dict[str, np.ndarray], classes: Sequence[str], index: Dict[str, int], batch_size: int, device):
    """Single-class groups in class order: (device rows [b, P], the class's index)."""
    for w in classes:
        rows = features.get(w)
        if rows is None or len(rows) == 0:
            continue
        x = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(device)
        for o in range(0, len(x), batch_size):
            yield x[o:o + batch_size], index[w]


def main(argv=None) -> str:
    args = parse_args(argv)
    from . import cnzsl, dgp_eval
    if not torch.cuda.is_available():
        raise RuntimeError("train_cnzsl needs the GPU: the product path has no CPU fallback")
    dev = torch.device("cuda:0")
    if args.synthetic is not None:
        graph_edges, splits, attrs, features = synthetic_material(args.synthetic, args.seed)
        hid = SYN_HID
    else:
        graph_edges = json.load(open(args.graph_path, "r"))
        splits = json.load(open(args.split_path, "r"))
        attrs, features, hid = load_attributes(args.attributes), dgp_eval.load_features(args.features), HID_DIM
    for key in ("train", args.data_train, args.data_test):
        if key not in splits:
            raise SystemExit(f"split '{key}' is not in the split file (has {sorted(splits)})")
    train_classes = list(splits["train"])
    nodes = ordered_nodes(graph_edges, train_classes)
    if attrs.shape[0] != len(nodes):
        raise SystemExit(f"{attrs.shape[0]} attribute rows for {len(nodes)} nodes")
    index = {w: i for i, w in enumerate(nodes)}
    proto = next(iter(features.values())).shape[1]
    attribute = torch.from_numpy(attrs).to(dev)
    n_seen = len(train_classes)

    print("\n<=============== Starting training ===============>", flush=True)
    torch.manual_seed(args.seed)
    model = cnzsl.CNZSLModel(attrs.shape[1], hid, proto, cn=args.cn, init=args.init, device=dev)
    if args.load:
        model.load_state_dict(torch.load(args.file_path, map_location=dev))
    if args.train:
        trainer = cnzsl.CNZSLTrainer(model, lr=1e-4, weight_decay=1e-4, step_size=25, gamma=0.1)      # cnzsl.py:358-359
        seen_attrs = attribute[:n_seen].contiguous()                                                 # attribute[train_mask]
        for w in splits[args.data_train]:
            if index[w] >= n_seen:
                raise SystemExit(f"--data_train class {w} is not a seen class: its label has no logit")
        out_dir = os.path.dirname(args.file_path)
        for epoch in range(args.epoch):
            print("epoch:{}".format(epoch))
            for i, (x, t) in enumerate(class_batches(features, splits[args.data_train], index, args.batch_size, dev)):
                loss = trainer.step(x, torch.full((x.shape[0],), t, dtype=torch.int32, device=dev), seen_attrs)
                if i % args.print_freq == 0:
                    print("loss: {:.2f}".format(float(loss)), flush=True)
            trainer.epoch_end()
            if epoch > 5:
                if out_dir:
                    os.makedirs(out_dir, exist_ok=True)
                torch.save(model.state_dict(), args.file_path + "_{}".format(epoch))
    print("attr:{},cn:{},init:{}".format(args.attr, args.cn, args.init), flush=True)
    test_index = [index[w] for w in splits[args.data_test]]
    ev = cnzsl.CNZSLEvaluator(graph_edges, nodes, test_index, model.eval(), attribute)
    for x, t in class_batches(features, splits[args.data_test], index, args.test_batch_size, dev):
        ev.add(x, t)
    print("End of testing.")
    out = ev.result()
    print(out, flush=True)
    return out


if __name__ == "__main__":
    main()
