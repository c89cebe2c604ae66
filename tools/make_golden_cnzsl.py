#!/usr/bin/env python3
"""Generates tests/golden/cnzsl_train_small.npz and tests/golden/cnzsl_eval_small.npz by RUNNING the reference's CNZSL code
(baseline/CNZSL/cnzsl.py) on the CPU.  That file executes at import (argument parsing, data loading, a ResNet-50), so nothing is
imported: at run time the file is parsed with `ast`, the definitions `ClassStandardization`, `CNZSLModel`, `gen_tree`, `count_acc`
and `test` are kept and compiled into a prepared namespace (torch, nn, np, F, the two switches, and what `test` reads as module
globals).  `.cuda()` is patched to identity.  Nothing of the file is copied; the fixtures hold seeds and recorded outputs only -
inputs come from hgr_net_amd.baseline.cnzsl.synth_state / synth_rows by seed.

Training fixture: S = 37 seen classes, A = 40, H = 48, P = 96, B = 24; three steps of Adam(lr 1e-4, weight_decay 1e-4): a batch of
mixed labels, a single-class batch, the first batch again.  Run twice with the same reference classes, in fp32 and in fp64.
`err32` = the largest over the gradient tensors of max|g32 - g64| / norm: the measured distance between two correct
implementations.  norm = max|g64|, except for 'model.2.bias': behind a standardisation that subtracts the column mean this
gradient is a sum that cancels to zero in exact arithmetic (fp64 gives ~1e-17, fp32 ~1e-8), so its error is measured against what
it is a cancelling sum of, `absdz` = max over columns of sum_rows |d loss / d z|.

Evaluation fixture: the reference's `test()` with a fake loader, `feature_encoder` = identity (P = 2048 is hard-coded there), 64
nodes in permuted order with 16 seen classes first, A = 40, H = 64, non-trivial running vectors, every test class with 1 - 9 feature
rows.  Seeds are tried until a recorded level pick is a filler win and a batch has one row."""
import ast
import contextlib
import copy
import io
import json
import os
import sys
import tempfile
import types
from collections import defaultdict
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("HGR_REFERENCE", "/root/reference")) / "baseline" / "CNZSL" / "cnzsl.py"
sys.path.insert(0, str(REPO))

import networkx as nx                                                  # noqa: E402
import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
import torch.nn as nn                                                  # noqa: E402
import torch.nn.functional as F                                        # noqa: E402
from torch.autograd import Variable                                    # noqa: E402

from hgr_net_amd import synth                                          # noqa: E402
from hgr_net_amd.baseline import cnzsl, dgp_eval                       # noqa: E402

GOLD = REPO / "tests" / "golden"
KEEP = {"ClassStandardization", "CNZSLModel", "gen_tree", "count_acc", "test"}
S, A, H, P, B, STEPS, LR, WD = 37, 40, 48, 96, 24, 3, 1e-4, 1e-4
TRAIN_SEED = 11
N_NODES, N_SEEN, EA, EH, EP = 64, 16, 40, 64, 2048


def load_reference(cn=True, init=True) -> dict:
    """The kept definitions of the reference file, compiled into a namespace of their own."""
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    tree = ast.parse(REF.read_text(), filename=str(REF))
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in KEEP]
    assert {n.name for n in body} == KEEP
    ns = {"torch": torch, "nn": nn, "np": np, "F": F, "USE_CLASS_STANDARTIZATION": cn, "USE_PROPER_INIT": init, "json": json, "nx": nx,
          "copy": copy, "defaultdict": defaultdict, "Variable": Variable, "DEVICE": "cpu",
          "map_label": lambda names, all_names, batch=False: [all_names.index(n) for n in names] if batch else all_names.index(names)}
    exec(compile(ast.Module(body=body, type_ignores=[]), str(REF), "exec"), ns)
    return ns


def rel(a, b, norm=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if norm is None else norm))


# ---- training -------------------------------------------------------------------------------------------------------------------------------
def train_material():
    attrs = cnzsl.synth_rows(TRAIN_SEED, "cnzsl.train.attrs", S, A)
    x_mixed = cnzsl.synth_rows(TRAIN_SEED, "cnzsl.train.x0", B, P)
    x_single = cnzsl.synth_rows(TRAIN_SEED, "cnzsl.train.x1", B, P)
    mixed = synth.randint(TRAIN_SEED, "cnzsl.train.labels", B, 0, S)
    single = np.full(B, int(mixed[0]), np.int64)
    return attrs, [x_mixed, x_single, x_mixed], [mixed, single, mixed]


def run_training(ns, sd0, attrs, feats, labels, dtype):
    model = ns["CNZSLModel"](A, H, P).to(dtype)
    model.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd0.items()})
    taps = []

    def tap(mod, inp, out):                                            # z = h1 W2^T + b: its gradient is what the bias gradient sums
        out.retain_grad()
        taps.append(out)
    model.model[2].register_forward_hook(tap)
    optim = torch.optim.Adam(model.model.parameters(), lr=LR, weight_decay=WD)
    at = torch.from_numpy(attrs).to(dtype)
    out = {"losses": [], "grads": [], "gmin": {}, "logits": [], "absdz": []}
    model.train()
    for x, lab in zip(feats, labels):
        logits = model(torch.from_numpy(x).to(dtype), at)
        loss = F.cross_entropy(logits, torch.from_numpy(lab).long())
        optim.zero_grad()
        loss.backward()
        g = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        out["grads"].append(g)
        out["absdz"].append(float(taps[-1].grad.abs().sum(0).max()))
        for k, p in model.named_parameters():
            if p.grad is None:
                continue
            c = (p.grad + WD * p.detach()).abs().numpy()
            r = c / c.max()
            out["gmin"][k] = r if k not in out["gmin"] else np.minimum(out["gmin"][k], r)
        optim.step()
        out["losses"].append(float(loss.detach()))
        out["logits"].append(logits.detach().numpy().copy())
        assert bool(torch.isfinite(logits).all()), "a zero-norm prototype row"
    out["sd"] = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    return out


def make_train(ns):
    sd0 = cnzsl.synth_state(TRAIN_SEED, A, H, P)
    attrs, feats, labels = train_material()
    r32 = run_training(ns, sd0, attrs, feats, labels, torch.float32)
    r64 = run_training(ns, sd0, attrs, feats, labels, torch.float64)
    names = list(r32["grads"][0])
    assert names == list(cnzsl.TRAINABLE)
    errs = {}
    for k in names:
        norm = r64["absdz"][0] if k == "model.2.bias" else None
        errs[k] = rel(r32["grads"][0][k], r64["grads"][0][k], norm)
        print(f"{k:16s} |g32 - g64| / norm = {errs[k]:.3e}   max|g64| = {np.abs(r64['grads'][0][k]).max():.3e}")
    err32 = max(errs.values())
    theta = 100 * 4 * err32
    print(f"err32 = {err32:.3e}; parameter threshold {theta:.3e}; absdz64 = {r64['absdz'][0]:.4f}")
    for k in names:
        dead = np.ones_like(r32["gmin"][k], dtype=bool)
        for step in range(STEPS):
            dead &= (r32["grads"][step][k] == 0) & (r64["grads"][step][k] == 0)
        small = float(((r32["gmin"][k] < theta) & ~dead).mean())
        print(f"{k:16s} below the threshold in some step: {100 * small:.2f} %  (dead: {100 * dead.mean():.2f} %)")
        if k.endswith("weight"):
            assert small <= 0.01, (k, small)
    print("losses", r32["losses"], r64["losses"])
    assert r32["losses"][2] < r32["losses"][0]
    twin = cnzsl.train_state_host(sd0, torch.float64)
    for x, lab in zip(feats, labels):
        cnzsl.train_step_host(twin, x, lab, attrs, lr=LR, weight_decay=WD)
    print("fp64 twin vs fp64 reference, state after step 3:", max(rel(twin["sd"][k].numpy(), r64["sd"][k]) for k in r64["sd"]))
    dst = GOLD / "cnzsl_train_small.npz"
    np.savez_compressed(
        dst, seed=np.int32(TRAIN_SEED), dims=np.array([S, A, H, P, B], np.int32), lr=np.float64(LR), weight_decay=np.float64(WD),
        labels=np.stack(labels).astype(np.int32), err32=np.float64(err32), absdz64=np.float64(r64["absdz"][0]),
        losses32=np.array(r32["losses"], np.float64), losses64=np.array(r64["losses"], np.float64),
        logits32=np.stack(r32["logits"]).astype(np.float32), logits64=np.stack(r64["logits"]),
        **{"sd0_" + k: v for k, v in sd0.items()}, **{"sd3_" + k: v for k, v in r32["sd"].items()},
        **{"grad1_" + k: v for k, v in r32["grads"][0].items()}, **{"grad1_64_" + k: v for k, v in r64["grads"][0].items()},
        **{"gmin_" + k: v.astype(np.float32) for k, v in r32["gmin"].items()})
    print("wrote", dst, dst.stat().st_size)


# ---- evaluation -----------------------------------------------------------------------------------------------------------------------------
def eval_material(seed: int):
    edges = synth.make_dag(N_NODES, 12, seed=200 + seed, multi_parent=0.05)
    names = sorted({w for e in edges for w in e} - {"fall11"})
    assert len(names) == N_NODES
    rng = np.random.default_rng(seed)
    train_classes = [names[i] for i in rng.permutation(N_NODES)[:N_SEEN]]
    counts = rng.integers(1, 10, N_NODES - N_SEEN)
    counts[rng.integers(0, len(counts))] = 1                           # a 1-row batch
    return edges, train_classes, counts.astype(np.int64)


def run_eval(ns, seed: int):
    edges, train_classes, counts = eval_material(seed)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        gp = os.path.join(tmp, "g.json")
        json.dump(edges, open(gp, "w"))
        opts = types.SimpleNamespace(graph_path=gp, data_split_test="zsl_test", data_test="rest", print_freq=1, attr="transformer", cn=True, init=True)
        p2c, c2p, d2n, nodes, start_up = ns["gen_tree"](opts, train_classes)
        assert nodes[:N_SEEN] == train_classes
        tree = dgp_eval.build_list_tree(edges, nodes)
        assert tree.c2p == [list(c) for c in c2p], "the ordered-list tree disagrees with the reference's gen_tree"
        test_names = nodes[N_SEEN:]
        test_index = torch.tensor([nodes.index(w) for w in test_names])
        sd = cnzsl.synth_state(seed, EA, EH, EP, running=True)
        attrs = cnzsl.synth_rows(seed, "cnzsl.eval.attrs", N_NODES, EA)
        feats = cnzsl.synth_rows(seed, "cnzsl.eval.feats", int(counts.sum()), EP)
        model = ns["CNZSLModel"](EA, EH, EP)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        batches, o = [], 0
        for i, c in enumerate(counts.tolist()):
            t = int(test_index[i])
            batches.append({"img": torch.from_numpy(feats[o:o + c])[None], "label": torch.full((1, c), t, dtype=torch.int64)})
            o += c
        logits = []
        fwd = model.forward
        model.forward = lambda x, a: (logits.append(fwd(x, a).detach().numpy().copy()), torch.from_numpy(logits[-1]))[1]
        manager = type("DataManager_test", (), {"__init__": lambda self, **k: None, "get_data_loader": lambda self: batches})
        ns.update(opts=opts, DataManager_test=manager, ordered_nodes=nodes, splits={"rest": test_names}, model=model,
                  feature_encoder=lambda x: x, attribute=torch.from_numpy(attrs), test_index=test_index, c2p=c2p, d2n=d2n)
        os.makedirs(os.path.join(tmp, "result_cnzsl"))
        os.chdir(tmp)
        try:
            text = io.StringIO()
            with contextlib.redirect_stdout(text), torch.no_grad():
                ns["test"]()
        finally:
            os.chdir(cwd)
    lines = [l for l in text.getvalue().split("\n") if l.startswith("Top@")]
    assert len(lines) == len(batches) + 1 and len(logits) == len(batches)
    with torch.no_grad():
        p64 = cnzsl.prototypes_host(sd, attrs, dtype=torch.float64)
        l64 = cnzsl.logits_host(p64, feats).numpy()
    l32 = np.concatenate(logits, 0)
    err32 = rel(l32, l64)
    # the twin on the recorded logits: every cumulative line and the final one
    acc, filler, o = np.zeros(9), 0, 0
    for i, c in enumerate(counts.tolist()):
        t = int(test_index[i])
        r = cnzsl.score_host(logits[i], t, tree, test_index.numpy())
        acc += r["acc"]
        assert cnzsl.metric_string(acc) == "\n" + lines[i], (i, cnzsl.metric_string(acc), lines[i])
        for q in tree.path(t):
            on = test_index.numpy()[tree.depth[test_index.numpy()] == tree.depth[q]]
            filler += int((logits[i][:, on].max(1) < -1.0).sum())
    assert cnzsl.metric_string(acc) == "\n" + lines[-1]
    print(f"  seed {seed}: filler wins among the recorded level picks {filler}, depth {tree.n_levels - 1}, err32 {err32:.3e}, {lines[-1]}")
    if filler < 1 or tree.n_levels < 8:
        return None
    return dict(seed=np.int32(seed), edges=np.array(edges), nodes=np.array(nodes), n_seen=np.int32(N_SEEN), dims=np.array([EA, EH, EP], np.int32),
                counts=counts.astype(np.int32), test_index=test_index.numpy().astype(np.int32), logits=l32, err32=np.float64(err32),
                lines=np.array(lines))


def make_eval(ns):
    for seed in range(32):
        got = run_eval(ns, seed)
        if got is not None:
            break
    else:
        raise SystemExit("no seed met the evaluation fixture's conditions")
    dst = GOLD / "cnzsl_eval_small.npz"
    np.savez_compressed(dst, **got)
    print("wrote", dst, dst.stat().st_size)


if __name__ == "__main__":
    namespace = load_reference()
    make_train(namespace)
    make_eval(namespace)
