"""`python -m hgr_net_amd.baseline.train_dgp`: the command line of the reference's baseline/DGP/train_gcn_dense_att.py on the
device trainer (`dgp.DGPTrainer`).  Same options, same printed line, same files (`epoch_K.pth` = the state dict in the
reference's schema, `epoch_K.pred` = {'wnids', 'pred'}, `trlog`); the three material files are options here, and
`--synthetic N` trains on a generated graph with random vectors and targets where the material files are absent.
`--eval-after` scores the final predictions in memory with evaluate_dgp's options (`--features`, `--test-set`, ...).

Row convention.  The reference builds `fc_vectors[k] = fc_vector[wnids.index(train_wnids[k])]`, shuffles `tlist = range(len(
fc_vectors))` and compares `output_vectors[tlist[:n_train]]` with `fc_vectors[tlist[:n_train]]`: target k is matched to OUTPUT
ROW k (train_gcn_dense_att.py:60-69, 86-87, 99).  This script does the same.  `DGPTrainer.step(x, rows, targets)` itself is
stricter and more general: `rows` are distinct output rows in any order and `targets[k]` belongs to `rows[k]`; the reference's
convention is `rows = tlist[:n_train]`, `targets = fc_vectors[rows]`."""
from __future__ import annotations

import argparse
import json
import os
import os.path as osp
import random
from typing import List, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(prog="python -m hgr_net_amd.baseline.train_dgp", description=__doc__.split("\n\n")[0])
    parser.add_argument("--max-epoch", type=int, default=3000)
    parser.add_argument("--trainval", default="10,0")
    parser.add_argument("--lr", type=float, default=0.001)
    parser.add_argument("--weight-decay", type=float, default=0.0005)
    parser.add_argument("--save_epoch", type=int, default=1000)
    parser.add_argument("--save_path", default="result/att")
    parser.add_argument("--gpu", default="0")
    parser.add_argument("--no-pred", action="store_true")
    parser.add_argument("--graph", default="materials/imagenet-dense-grouped-graph_1.json")
    parser.add_argument("--fc-weights", default="materials/fc-weights.json")
    parser.add_argument("--splits", default="data/process_results/splits_for_tree.json")
    parser.add_argument("--hidden-layers", default="d2048,d")
    parser.add_argument("--seed", type=int, default=0, help="dropout counter seed, parameter initialisation and the train / val shuffle")
    parser.add_argument("--synthetic", type=int, default=None, metavar="N",
                        help="train on a generated N-node graph (synth.make_dag) with random vectors and targets instead of the material files")
    parser.add_argument("--eval-after", action="store_true",
                        help="score the final predictions in memory like evaluate_dgp (its options below; with --synthetic on generated features)")
    from .evaluate_dgp import add_eval_options, check_args
    add_eval_options(parser.add_argument_group("scoring (--eval-after)"), standalone=False)
    args = parser.parse_args(argv)
    check_args(args)
    return args


def split_trainval(n_trainval: int, trainval: str, seed: int) -> Tuple[List[int], List[int]]:
    """train_gcn_dense_att.py:82-87: a shuffled range(n_trainval) cut at n_train = round(n * v_train / (v_train + v_val))."""
    v_train, v_val = map(float, trainval.split(","))
    n_train = round(n_trainval * (v_train / (v_train + v_val)))
    tlist = list(range(n_trainval))
    random.Random(seed).shuffle(tlist)
    return tlist[:n_train], tlist[n_train:]


def fc_targets(wnids: Sequence[str], fcfile, train_wnids: Sequence[str]) -> torch.Tensor:
    """train_gcn_dense_att.py:63-69: row k = fc_vector[wnids.index(train_wnids[k])] (not yet normalised)."""
    fc_vector = [x[1] for x in fcfile]
    pos = {w: i for i, w in reversed(list(enumerate(wnids)))}          # first occurrence, like list.index
    return torch.tensor([fc_vector[pos[w]] for w in train_wnids], dtype=torch.float32)


def synthetic_dag(n_nodes: int, seed: int):
    """The edge list [[parent, child], ...] the synthetic material is generated from."""
    from .. import synth
    return synth.make_dag(n_nodes, 10, seed=7 + seed, multi_parent=0.03)


def synthetic_material(n_nodes: int, seed: int, dim_in: int = 300, dim_out: int = 512):
    """(graph, fcfile, splits) in the formats of the three material files, from synth.make_dag."""
    from .. import synth
    from . import dgp
    dag = synthetic_dag(n_nodes, seed)
    wnids = ["fall11"] + sorted({w for e in dag for w in e} - {"fall11"})
    idx = {w: i for i, w in enumerate(wnids)}
    n = len(wnids)
    edges_set = dgp.group_edges(n, [(idx[p], idx[c]) for p, c in dag])
    vec = synth.normal(seed, "dgp.synthetic.vectors", n * dim_in).reshape(n, dim_in).astype(np.float32)
    fc = synth.normal(seed, "dgp.synthetic.fc", n * dim_out).reshape(n, dim_out).astype(np.float32)
    order = np.argsort(synth.uniform(seed, "dgp.synthetic.split", n), kind="stable")
    n_train = max(1, n // 2)
    graph = {"wnids": wnids, "vectors": vec, "edges_set": edges_set}
    return graph, [[w, fc[i]] for i, w in enumerate(wnids)], {"train": [wnids[i] for i in order[:n_train]], "rest": [wnids[i] for i in order[n_train:]]}


def main(argv=None) -> None:
    args = parse_args(argv)
    os.environ.setdefault("CUDA_VISIBLE_DEVICES", args.gpu)           # utils.set_gpu
    print("using gpu {}".format(args.gpu))
    from . import dgp
    if not torch.cuda.is_available():
        raise RuntimeError("train_dgp needs the GPU: the product path has no CPU fallback")
    if args.synthetic is not None:
        graph, fcfile, splits = synthetic_material(args.synthetic, args.seed)
    else:
        graph = json.load(open(args.graph, "r"))
        fcfile = json.load(open(args.fc_weights, "r"))
        splits = json.load(open(args.splits, "r"))
    wnids = graph["wnids"]
    n = len(wnids)
    print("edges_set", [len(l) for l in graph["edges_set"]])
    edges_set = dgp.fold_groups(graph["edges_set"], 4)
    print("edges_set", [len(l) for l in edges_set])
    word_vectors = F.normalize(torch.as_tensor(np.asarray(graph["vectors"], dtype=np.float32))).cuda()
    fc_vectors = F.normalize(fc_targets(wnids, fcfile, splits["train"])).cuda()

    torch.manual_seed(args.seed)
    gcn = dgp.GCN_Dense_Att(n, edges_set, word_vectors.shape[1], fc_vectors.shape[1], args.hidden_layers)
    print("word vectors:", word_vectors.shape)
    print("fc vectors:", fc_vectors.shape)
    print("hidden layers:", args.hidden_layers)
    trainer = dgp.DGPTrainer(gcn, lr=args.lr, weight_decay=args.weight_decay, seed=args.seed)

    train, val = split_trainval(len(fc_vectors), args.trainval, args.seed)
    print("num train: {}, num val: {}".format(len(train), len(val)))
    rows, targets = torch.tensor(train, dtype=torch.int32), fc_vectors[torch.tensor(train, dtype=torch.long)]
    val_rows = torch.tensor(val, dtype=torch.int32) if val else None
    val_targets = fc_vectors[torch.tensor(val, dtype=torch.long)] if val else None
    os.makedirs(args.save_path, exist_ok=True)
    trlog = {"train_loss": [], "val_loss": [], "min_loss": 0}
    min_loss = 1e18
    for epoch in range(1, args.max_epoch + 1):
        trainer.step(word_vectors, rows, targets)
        train_loss, val_loss = trainer.losses(word_vectors, rows, targets, val_rows, val_targets)
        print("epoch {}, train_loss={:.4f}, val_loss={:.4f}".format(epoch, train_loss, val_loss), flush=True)
        trlog["train_loss"].append(train_loss)
        trlog["val_loss"].append(val_loss)
        trlog["min_loss"] = min_loss
        torch.save(trlog, osp.join(args.save_path, "trlog"))
        if epoch % args.save_epoch == 0:
            pred_obj = None if args.no_pred else {"wnids": wnids, "pred": gcn.eval()(word_vectors)}
            torch.save(gcn.state_dict(), osp.join(args.save_path, "epoch_{}.pth".format(epoch)))
            torch.save(pred_obj, osp.join(args.save_path, "epoch_{}.pred".format(epoch)))
    if args.eval_after:
        eval_after(args, wnids, gcn.eval()(word_vectors), splits)


def eval_after(args: argparse.Namespace, wnids: Sequence[str], vectors: torch.Tensor, splits: dict) -> dict:
    """Score the predictions in memory: evaluate_dgp's run on {'wnids', 'pred'} without the file in between."""
    from . import dgp_eval, evaluate_dgp
    pred = {"wnids": list(wnids), "pred": vectors.detach().to(torch.float32).cpu()}
    if args.synthetic is not None:
        graph_edges = synthetic_dag(args.synthetic, args.seed)
        splits = {k: [w for w in v if w != "fall11"] for k, v in splits.items()}       # the synthetic splits draw from the root too
        test = list(splits[args.test_set])
        features = evaluate_dgp.synthetic_features(dgp_eval.pick_vectors(pred, test), test, args.seed)
    else:
        if args.features is None:
            raise SystemExit("--eval-after needs --features FILE.npz")
        graph_edges = json.load(open(args.graph_path, "r"))
        features = dgp_eval.load_features(args.features)
    return evaluate_dgp.run(args, graph_edges, splits, pred, features)


if __name__ == "__main__":
    main()
