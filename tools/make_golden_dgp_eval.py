#!/usr/bin/env python3
"""Generates tests/golden/dgp_eval_small.npz by RUNNING the reference's `test_on_subset` (baseline/DGP/evaluate_imagenet.py) on the
CPU: `.cuda()` patched to identity, a stub for the missing `datasets.imagenet` (and for `models.resnet`, which wants torchvision),
the module's DataLoader replaced by one without workers, `cnn` = identity on feature rows, the edge JSON under a temporary working
directory.  64 nodes in permuted order (16 seen first), K = 64, every unseen class with 1 - 9 feature rows, both settings of
`consider_trains`.  Weights and features come from {-1, -1/2, 0, 1/2, 1}, biases from multiples of 1/4 in [-2, 2]: every partial
sum is a multiple of 1/4 below 2^11 / 4, so the fp16 table is exact in any accumulation order.  The fixture holds inputs and the
recorded outputs only.  Seeds are tried until the fixture exercises what it is for (the assertions below)."""
import json
import os
import sys
import tempfile
import types
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("HGR_REFERENCE", "/root/reference")) / "baseline" / "DGP"
sys.path.insert(0, str(REPO))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402

from hgr_net_amd import synth                                          # noqa: E402
from hgr_net_amd.baseline import dgp_eval                              # noqa: E402

GOLD = REPO / "tests" / "golden"
N_NODES, N_SEEN, K = 64, 16, 64


def load_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    ds = types.ModuleType("datasets")
    dsi = types.ModuleType("datasets.imagenet")
    dsi.ImageNet = object
    ds.imagenet = dsi
    rn = types.ModuleType("models.resnet")
    rn.make_resnet50_base = lambda: None
    sys.modules.update({"datasets": ds, "datasets.imagenet": dsi, "models.resnet": rn})
    sys.path.insert(0, str(REF))
    import evaluate_imagenet as ev
    real_loader = torch.utils.data.DataLoader
    ev.DataLoader = lambda dataset, batch_size, shuffle, num_workers: real_loader(dataset=dataset, batch_size=batch_size, shuffle=shuffle, num_workers=0)
    return ev


def material(seed: int):
    edges = synth.make_dag(N_NODES, 12, seed=100 + seed, multi_parent=0.05)
    names = sorted({w for e in edges for w in e} - {"fall11"})
    assert len(names) == N_NODES
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N_NODES)
    nodes = [names[i] for i in perm]                                   # 16 seen classes lead, in no depth order
    vals = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32)
    w = vals[rng.integers(0, 5, (N_NODES, K))]
    b = (rng.integers(-8, 9, N_NODES) * 0.25).astype(np.float32)
    pred = np.concatenate([w, b[:, None]], 1)
    counts = rng.integers(1, 10, N_NODES - N_SEEN)
    counts[rng.integers(0, len(counts))] = 1                           # a 1-row batch
    feats = [vals[rng.integers(0, 5, (int(c), K))] for c in counts]
    return edges, nodes, pred, feats


def run_reference(ev, edges, nodes, pred, feats):
    ev.test_index = torch.arange(N_NODES)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data", "process_results"))
        json.dump(edges, open(os.path.join(tmp, "data", "process_results", "graph_edges_cls.json"), "w"))
        os.chdir(tmp)
        try:
            tree = ev.tree(list(nodes))
        finally:
            os.chdir(cwd)
    pv = torch.from_numpy(pred).half()
    out = np.zeros((2, N_NODES - N_SEEN, 9), np.float64)
    for ct in (0, 1):
        for i, f in enumerate(feats):
            wnid = nodes[N_SEEN + i]
            subset = [(torch.from_numpy(row), wnid) for row in f]
            with torch.no_grad():
                hits, tot, hits_all, _, path_all, point_all = ev.test_on_subset(subset, lambda x: x, N_SEEN, pv, N_SEEN + i, tree, bool(ct))
            out[ct, i] = [*hits.tolist(), float(hits_all), float(path_all), float(point_all), float(tot)]
    return tree, out


def check(edges, nodes, pred, feats, tree_ref, ref):
    """The conditions that make the fixture worth having; returns None when one fails, the arrays to store otherwise."""
    tree = dgp_eval.build_list_tree(edges, nodes)
    assert tree.c2p == [list(c) for c in tree_ref.c2p], "the ordered-list tree disagrees with the reference's gen_tree"
    if tree.n_levels < 10:                                             # depth at least 9
        return None
    p16 = pred.astype(np.float16)
    ties = rows = fill_wins = 0
    tables = []
    mine = np.zeros_like(ref)
    for i, f in enumerate(feats):
        t = N_SEEN + i
        exact = np.concatenate([f.astype(np.float64), np.ones((len(f), 1))], 1) @ p16.astype(np.float64).T
        tab = exact.astype(np.float16)
        assert np.array_equal(tab.astype(np.float64), exact), "the fp16 table must be exact"
        tables.append(tab)
        for ct in (0, 1):
            h = dgp_eval.HostEvaluator(tree, N_SEEN, consider_trains=bool(ct))
            h.add(tab, t)
            mine[ct, i] = h.acc[t]
        v = tab.astype(np.float32).copy()
        v[:, :N_SEEN] = np.float32(np.float16(dgp_eval.FILL))
        others = np.delete(v[:, N_SEEN:], i, axis=1)
        ties += int((others == v[:, [t]]).any(1).sum())
        rows += len(f)
        for p in tree.path(t):
            on = np.nonzero(tree.depth == tree.depth[p])[0]
            if len(on) < N_NODES:
                fill_wins += int((v[:, on].max(1) < -1.0).sum())
    assert np.array_equal(mine[..., [0, 1, 2, 3, 4, 5, 8]], ref[..., [0, 1, 2, 3, 4, 5, 8]]), "score_rows_host disagrees with the reference (integers)"
    assert np.abs(mine[..., 6:8] - ref[..., 6:8]).max() < 1e-12, "score_rows_host disagrees with the reference (path / point)"
    differ = int((ref[0, :, :5] != ref[1, :, :5]).any(1).sum())
    print(f"  rows with a tie at the target {100 * ties / rows:.0f} %, fill wins {fill_wins}, classes whose hits differ {differ}, depth {tree.n_levels - 1}")
    if ties < 0.3 * rows or fill_wins < 10 or differ < 10:
        return None
    return tree, np.concatenate(tables, 0)


def main():
    ev = load_reference()
    for seed in range(32):
        print("seed", seed)
        edges, nodes, pred, feats = material(seed)
        tree_ref, ref = run_reference(ev, edges, nodes, pred, feats)
        ok = check(edges, nodes, pred, feats, tree_ref, ref)
        if ok is not None:
            break
    else:
        raise SystemExit("no seed met the fixture's conditions")
    tree, table = ok
    ptr = np.cumsum([0] + [len(c) for c in tree.c2p]).astype(np.int32)
    dst = GOLD / "dgp_eval_small.npz"
    np.savez_compressed(dst, seed=np.int32(seed), edges=np.array(edges), nodes=np.array(nodes), n_seen=np.int32(N_SEEN), pred=pred,
                        feat=np.concatenate(feats, 0), feat_count=np.array([len(f) for f in feats], np.int32),
                        c2p_ptr=ptr, c2p_flat=np.array([p for c in tree.c2p for p in c], np.int32), table=table,
                        # [consider_trains][unseen class][hits@1,2,5,10,20, hits_all, path_all, point_all, tot] as test_on_subset returned them
                        ref=ref)
    print("wrote", dst, dst.stat().st_size)


if __name__ == "__main__":
    main()
