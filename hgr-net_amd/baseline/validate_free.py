"""`python -m hgr_net_amd.baseline.validate_free`: the command line of the reference's baseline/FREE/validate.py on the device route
(`free.FREEClassifier`), on CACHED image features: load the generator and the FR module, synthesise `--syn_num` features per test
class, fit the softmax classifier for `--epochs` epochs (512 real + 1000 synthetic rows per step, a new order of the real rows
every epoch, the last batch of an epoch skipped) and print `test()`'s metric string.

The reference recomputes ResNet-50 features in every step and reads `text_feats.json`; here both are files: `--features FILE.npz`
(one [n_i, 2048] array per wnid, as extract_features writes) and `--attributes FILE` ([N, A] in node order; the rows are
L2-normalised as validate.py:254 does).  `--synthetic N` needs no file: a generated graph, attributes, features and networks."""
from __future__ import annotations

import argparse
import json
from typing import Dict, List, Sequence

import numpy as np
import torch

SYN = dict(attSize=64, ngh=128, latensize=64, batch_size=48, syn_batch=80, syn_num=8, train_rows=40, test_rows=4)


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(prog="python -m hgr_net_amd.baseline.validate_free", description="FREE baseline, validation route, on cached features")
    p.add_argument("--load_G", type=str, default=None, help="checkpoint with the generator under 'netG'")
    p.add_argument("--load_F", type=str, default=None, help="checkpoint with the FR module under 'netFR'")
    p.add_argument("--attSize", type=int, default=1024)
    p.add_argument("--resSize", type=int, default=2048)
    p.add_argument("--ngh", type=int, default=4096)
    p.add_argument("--latensize", type=int, default=2048)
    p.add_argument("--nclass_seen", type=int, default=983)
    p.add_argument("--classifier_lr", type=float, default=0.001)
    p.add_argument("--syn_num", type=int, default=100)
    p.add_argument("--manualSeed", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=512, help="real rows per step; 1000 synthetic rows join them")
    p.add_argument("--graph", default="data/process_results/graph_edges_cls.json")
    p.add_argument("--splits", default="data/process_results/splits_for_tree.json")
    p.add_argument("--attributes", default=None, metavar="FILE", help=".npz / .json: [N, A] in node order, or a list of chunks")
    p.add_argument("--features", default=None, metavar="FILE.npz", help="one [n_i, 2048] array per wnid")
    p.add_argument("--epochs", type=int, default=20)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f16"], help="the MFMA input type of the fit and of test()")
    p.add_argument("--seed", type=int, default=0, help="counter seed of the synthesis / FR noise and of the --synthetic material")
    p.add_argument("--save-cls", default=None, metavar="PATH", help="where the classifier's state_dict goes (validate.py: cls_{attSize})")
    p.add_argument("--synthetic", type=int, default=None, metavar="N", help="generated graph, attributes, features and networks; needs no file")
    args = p.parse_args(argv)
    if args.batch_size < 1 or args.epochs < 0 or args.syn_num < 1:
        p.error("--batch_size and --syn_num must be positive, --epochs non-negative")
    if args.synthetic is not None and args.synthetic < 100:
        p.error("--synthetic N: at least 100 nodes")
    if args.synthetic is None and None in (args.attributes, args.features, args.load_G, args.load_F):
        p.error("--attributes, --features, --load_G and --load_F are needed without --synthetic")
    return args


class RealLoader:
    """The train loader on cached rows: `DataLoader(batch_size, shuffle=True)` - every pass over it draws a new order (a host
    generator seeded once), so the short or last batch that fit_zsl skips holds other rows in every epoch.  Yields (rows, labels)
    on the device."""

    def __init__(self, features: Dict[str, np.ndarray], classes: Sequence[str], index: Dict[str, int], batch_size: int, seed: int, device):
        have = [w for w in classes if w in features and len(features[w])]
        if not have:
            raise ValueError("no feature rows for the train classes")
        self.x = torch.from_numpy(np.concatenate([np.asarray(features[w], dtype=np.float32) for w in have], 0)).to(device)
        self.y = torch.from_numpy(np.concatenate([np.full(len(features[w]), index[w], dtype=np.int64) for w in have])).to(device)
        self.batch_size, self.gen = int(batch_size), torch.Generator().manual_seed(seed)

    def __len__(self) -> int:
        return -(-len(self.x) // self.batch_size)

    def __iter__(self):
        order = torch.randperm(len(self.x), generator=self.gen).to(self.x.device)
        for o in range(0, len(order), self.batch_size):
            idx = order[o:o + self.batch_size]
            yield self.x.index_select(0, idx), self.y.index_select(0, idx)


def synthetic_material(n_nodes: int, seed: int):
    from .. import synth
    from ..hierarchy import build_hierarchy
    from . import free
    from .train_cnzsl import ordered_nodes
    edges = synth.make_dag(n_nodes, 10, seed=7 + seed, multi_parent=0.03)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], n_nodes // 4, n_nodes // 4, 13 + seed)
    nodes = ordered_nodes(edges, splits["train"])
    attrs = free.synth_rows(seed, "free.synthetic.attrs", len(nodes), SYN["attSize"])
    feats: Dict[str, np.ndarray] = {}
    for key, rows in (("train", SYN["train_rows"]), ("rest", SYN["test_rows"])):
        for w in splits[key]:
            base = free.synth_rows(seed, "free.synthetic.base." + w, 1, free.RES)
            noise = free.synth_rows(seed, "free.synthetic.noise." + w, rows, free.RES)
            feats[w] = (1.0 / (1.0 + np.exp(-(base + 0.5 * noise)))).astype(np.float32)
    return edges, splits, attrs, feats


def main(argv=None) -> str:
    args = parse_args(argv)
    from . import dgp_eval, free
    from .train_cnzsl import load_attributes, ordered_nodes
    if not torch.cuda.is_available():
        raise RuntimeError("validate_free needs the GPU: the product path has no CPU fallback")
    dev = torch.device("cuda:0")
    seed = args.seed if args.manualSeed is None else args.manualSeed
    print("Random Seed: ", seed)
    torch.manual_seed(seed)
    syn_batch = 1000
    if args.synthetic is not None:
        graph_edges, splits, attrs, features = synthetic_material(args.synthetic, args.seed)
        args.attSize, args.ngh, args.latensize, args.batch_size, args.syn_num = (SYN[k] for k in ("attSize", "ngh", "latensize", "batch_size", "syn_num"))
        syn_batch = SYN["syn_batch"]
    else:
        graph_edges, splits = json.load(open(args.graph, "r")), json.load(open(args.splits, "r"))
        attrs, features = load_attributes(args.attributes), dgp_eval.load_features(args.features)
    if args.latensize * 2 != args.ngh:
        raise SystemExit(f"--latensize * 2 = {args.latensize * 2} must equal --ngh = {args.ngh}: validate.py passes it as the width of `hidden`")
    train_classes = list(splits["train"])
    nodes = ordered_nodes(graph_edges, train_classes)
    if attrs.shape != (len(nodes), args.attSize):
        raise SystemExit(f"attributes are {attrs.shape} for {len(nodes)} nodes and --attSize {args.attSize}")
    attrs = attrs / np.sqrt((attrs.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)      # validate.py:254
    index = {w: i for i, w in enumerate(nodes)}
    opt = free.make_opt(attSize=args.attSize, resSize=args.resSize, ngh=args.ngh, latensize=args.latensize, nclass_seen=args.nclass_seen,
                        decoder_hidden=4096 if args.synthetic is None else SYN["ngh"])
    netG, netFR = free.Generator(opt, args.dtype), free.FR(opt, opt.attSize, args.dtype)
    if args.synthetic is not None:
        netG.load_state_dict({k: torch.from_numpy(v) for k, v in free.synth_state(args.seed, opt, "netG").items()})
        netFR.load_state_dict({k: torch.from_numpy(v) for k, v in free.synth_state(args.seed, opt, "netFR").items()})
    else:
        netG.load_state_dict(torch.load(args.load_G, map_location="cpu")["netG"])
        netFR.load_state_dict(torch.load(args.load_F, map_location="cpu")["netFR"])
    tree = dgp_eval.build_list_tree(graph_edges, nodes)
    test_index = [index[w] for w in splits["rest"]]
    nclass = 18278 if args.synthetic is None else len(nodes)
    cls = free.FREEClassifier(netG, netFR, tree, test_index, torch.from_numpy(np.ascontiguousarray(attrs)).to(dev), max(nclass, len(nodes)),
                              lr=args.classifier_lr, beta1=0.5, nepoch=args.epochs, batch_size=args.batch_size + syn_batch, syn_num=args.syn_num,
                              syn_batch_size=syn_batch, dtype=args.dtype, seed=seed)
    loader = RealLoader(features, train_classes, index, args.batch_size, seed, dev)
    # a short last batch is the one fit_zsl skips; every trained batch has --batch_size rows
    cls.fit_zsl(loader)
    if args.save_cls:
        torch.save({k: v.detach().cpu().clone() for k, v in cls.model.state_dict().items()}, args.save_cls)
    for w in splits["rest"]:
        rows = features.get(w)
        if rows is not None and len(rows):
            cls.add(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev), index[w])
    print("End of testing.")
    out = cls.result()
    print(out, flush=True)
    return out


if __name__ == "__main__":
    main()
