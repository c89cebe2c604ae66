"""`python -m hgr_net_amd.baseline.evaluate_dgp`: the command line of the reference's baseline/DGP/evaluate_imagenet.py and
evaluate_21kp.py on the device evaluator (`dgp_eval.DGPEvaluator`).  It reads an `epoch_K.pred` file, scores its classifiers against
image FEATURES - cached ones (`--features FILE.npz`, one [n_i, K] array per wnid: tower-free evaluation) or those of images pushed
through the baseline's ResNet on the device (`--cnn FILE.pth --image-dir DIR`, resnet.ResNetFeatures as the evaluator's `cnn`) -,
prints the reference's per-class lines and its `summary:` line in the reference's formats and writes `{wnid: hits / tot}` to `--output`.

Reference options: --pred --test-set --output --keep-ratio --consider-trains --graph_path.  Ours: --split_path, --train-set (its
classes lead the node list and are the seen columns; empty = the 21K-P protocol of evaluate_21kp.py: the test set is the node list,
n = 0), --features, --batch-size, --dtype, --synthetic N (a generated graph, predictions and features: runs with no material files).
--cnn FILE.pth is the reference's option (a `make_resnet50_base()` state_dict); it needs --image-dir DIR (one sub-folder per wnid;
--image-size, --version: extract_features.add_cnn_options, where the unknown transform of the reference is spoken of), or, with
--synthetic N, `--cnn synthetic` scores generated images through a seeded net end to end.
--gpu and --test-train are not offered (the reference's --test-train cannot run: wrong call arity, undefined names).
--keep-ratio keeps the first ceil(ratio * n_i) rows of a class.  The per-class lines are printed after the last batch, from the
counters read once: no batch waits for the host."""
from __future__ import annotations

import argparse
import json
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import dgp_eval, extract_features


def add_eval_options(parser: argparse.ArgumentParser, standalone: bool = True) -> None:
    """The scoring options, shared with `train_dgp --eval-after`."""
    if standalone:
        parser.add_argument("--pred", default="gcn_dense_att/zsl/epoch_3000.pred")
        parser.add_argument("--split_path", default="data/process_results/splits_for_tree.json")
        parser.add_argument("--synthetic", type=int, default=None, metavar="N",
                            help="score generated predictions and features on a generated N-node graph instead of the material files")
        parser.add_argument("--seed", type=int, default=0, help="seed of the --synthetic material")
        extract_features.add_cnn_options(parser)
    parser.add_argument("--test-set", default="rest")
    parser.add_argument("--train-set", default="train", help="split whose classes lead the node list as the seen columns; '' = the 21K-P protocol")
    parser.add_argument("--output", default=None)
    parser.add_argument("--keep-ratio", type=float, default=1.0)
    parser.add_argument("--consider-trains", action="store_true")
    parser.add_argument("--graph_path", default="data/process_results/graph_edges_cls.json")
    parser.add_argument("--features", default=None, metavar="FILE.npz", help="one [n_i, K] float array per wnid")
    parser.add_argument("--batch-size", type=int, default=256)
    parser.add_argument("--dtype", default="f16", choices=["f16", "fp32"], help="the table's type: f16 = the reference's arithmetic and ties")


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m hgr_net_amd.baseline.evaluate_dgp", description=__doc__.split("\n\n")[0])
    add_eval_options(parser)
    args = parser.parse_args(argv)
    check_args(args)
    extract_features.check_cnn_args(args, args.synthetic is not None)
    if args.cnn is not None and args.features is not None:
        raise SystemExit("--features and --cnn exclude each other: cached features or images")
    return args


def check_args(args: argparse.Namespace) -> None:
    if args.batch_size < 1:
        raise SystemExit("--batch-size must be at least 1")
    if not 0.0 < args.keep_ratio <= 1.0:
        raise SystemExit("--keep-ratio must lie in (0, 1]")


def synthetic_features(vectors: torch.Tensor, wnids: Sequence[str], seed: int, max_rows: int = 9) -> Dict[str, np.ndarray]:
    """1..max_rows feature rows per class: the class's own classifier direction plus unit noise."""
    from .. import synth
    k = vectors.shape[1] - 1
    counts = synth.randint(seed, "dgp.eval.rows", len(wnids), 1, max_rows + 1)
    out = {}
    for i, w in enumerate(wnids):
        v = vectors[i, :k].numpy().astype(np.float64)
        noise = synth.normal(seed, "dgp.eval.feat." + w, int(counts[i]) * k).reshape(int(counts[i]), k)
        out[w] = (noise + 3.0 * v / max(float(np.linalg.norm(v)), 1e-6)).astype(np.float32)
    return out


def synthetic_material(n_nodes: int, seed: int, dim: int = 192):
    """(graph_edges, splits, pred, features) of a generated graph: half of the nodes are seen, `rest` are the others."""
    from .. import synth
    edges = synth.make_dag(n_nodes, 10, seed=7 + seed, multi_parent=0.03)
    wnids = sorted({w for e in edges for w in e} - {"fall11"})
    order = np.argsort(synth.uniform(seed, "dgp.eval.split", len(wnids)), kind="stable")
    n_train = max(1, len(wnids) // 2)
    splits = {"train": [wnids[i] for i in order[:n_train]], "rest": [wnids[i] for i in order[n_train:]]}
    vec = torch.from_numpy(synth.normal(seed, "dgp.eval.pred", len(wnids) * (dim + 1)).reshape(len(wnids), dim + 1).astype(np.float32) * 0.25)
    pred = {"wnids": wnids, "pred": vec}
    rest = splits["rest"]
    features = synthetic_features(dgp_eval.pick_vectors(pred, rest), rest, seed)
    return edges, splits, pred, features


def evaluate(graph_edges, train_wnids: Sequence[str], test_wnids: Sequence[str], pred, features: Dict[str, np.ndarray],
             consider_trains: bool = False, keep_ratio: float = 1.0, batch_size: int = 256, dtype: str = "f16", device="cuda:0",
             log=print, cnn=None) -> dict:
    """evaluate_imagenet.py:175-261 on features: every test class with rows is scored in batches of `batch_size`, the class at
    position i of the test set against column len(train) + i.  Returns `DGPEvaluator.result()` + 'lines' (what was printed).
    With `cnn` (images -> features on the device, resnet.ResNetFeatures) `features` holds `extract_features.ImageRows` per wnid."""
    nodes = list(train_wnids) + list(test_wnids)
    log("test set: {} classes, ratio={}".format(len(test_wnids), keep_ratio))
    log("consider train classifiers: {}".format(consider_trains))
    ev = dgp_eval.DGPEvaluator(graph_edges, nodes, len(train_wnids), pred, consider_trains=consider_trains, dtype=dtype, device=device,
                               cnn=cnn)
    for i, wnid in enumerate(test_wnids):
        rows = features.get(wnid)
        if rows is None or len(rows) == 0:                             # evaluate_imagenet.py:235
            continue
        if cnn is not None:
            for o in range(0, dgp_eval.keep_rows(len(rows), keep_ratio), batch_size):
                n = min(batch_size, dgp_eval.keep_rows(len(rows), keep_ratio) - o)
                ev.add(rows.batch(o, n, ev.device), len(train_wnids) + i)
            continue
        if rows.shape[1] != ev.k:
            raise ValueError(f"features of '{wnid}' are {rows.shape[1]} wide, the predictions want {ev.k}")
        rows = rows[:dgp_eval.keep_rows(len(rows), keep_ratio)]
        for o in range(0, len(rows), batch_size):
            chunk = np.ascontiguousarray(rows[o:o + batch_size])
            ev.add(torch.from_numpy(chunk).to(ev.device, non_blocking=True), len(train_wnids) + i)
    res = ev.result()
    # per-class lines carry the position of the class in the test set, like the reference's enumerate(test_wnids, 1)
    lines = dgp_eval.report_lines(res, test_wnids) if res["tot"] else ["summary: no test class has features"]
    for line in lines:
        log(line)
    res["lines"] = lines
    return res


def run(args: argparse.Namespace, graph_edges, splits: dict, pred, features: Dict[str, np.ndarray], device="cuda:0", log=print,
        cnn=None) -> dict:
    train = list(splits[args.train_set]) if args.train_set else []
    test = list(splits[args.test_set])
    res = evaluate(graph_edges, train, test, pred, features, consider_trains=args.consider_trains, keep_ratio=args.keep_ratio,
                   batch_size=args.batch_size, dtype=args.dtype, device=device, log=log, cnn=cnn)
    if args.output is not None:
        with open(args.output, "w") as f:
            json.dump(res["results"], f)
    return res


def main(argv=None) -> Optional[dict]:
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_dgp needs the GPU: the product path has no CPU fallback")
    cnn = None
    if args.cnn is not None:
        cnn = extract_features.load_cnn(args.cnn, args.version, args.seed)
    if args.synthetic is not None:
        graph_edges, splits, pred, features = synthetic_material(args.synthetic, args.seed, **({} if cnn is None else {"dim": cnn.out_channels}))
        if cnn is not None:                                            # generated images instead of generated features
            features = extract_features.synthetic_rows(splits["rest"], args.seed, args.image_size or extract_features.SYNTHETIC_SIZE)
    else:
        if args.features is None and cnn is None:
            raise SystemExit("--features FILE.npz or --cnn FILE.pth --image-dir DIR is required (or --synthetic N)")
        graph_edges = json.load(open(args.graph_path, "r"))
        splits = json.load(open(args.split_path, "r"))
        pred = dgp_eval.load_pred(args.pred)
        if cnn is not None:
            features = extract_features.image_dir_rows(args.image_dir, args.image_size or 224, "cuda:0", splits[args.test_set])
        else:
            features = dgp_eval.load_features(args.features)
    return run(args, graph_edges, splits, pred, features, cnn=cnn)


if __name__ == "__main__":
    main()
