"""GPU: evaluation of batches packed from several classes - hgr_eval_counters_rows against a per-row restatement of main.py:139-191
and against the single-class kernel, its independence of the row order, and evaluate.test with opts.pack_batches end to end."""
import json
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import evaluate, ops, synth
from hgr_net_amd.clip.model import build_model
from hgr_net_amd.dataset.packing import PackedBatches
from hgr_net_amd.model import tree_model

DEV = "cuda"
INT = evaluate.COUNTERS[:6] + ["num_sample"]
RATIO = ["path_all", "point_all"]
# path_all / point_all are double-precision sums of at most ~1e3 terms of magnitude <= 1: any reordering stays below 1e-12
RATIO_TOL = 1e-9


def _cfg(z):
    cfg = json.loads(str(z["config"])) if not isinstance(z, dict) else z
    if isinstance(cfg["vision_layers"], list):
        cfg["vision_layers"] = tuple(cfg["vision_layers"])
    return cfg


def _tree_case(case, golden_dir, dt="bf16", tdt="f16"):
    meta = json.load(open(golden_dir / f"tree_{case}.json"))
    z = np.load(golden_dir / f"tree_{case}.npz")
    cfg = _cfg(meta["config"])
    d = meta["dag"]
    edges = synth.make_dag(meta["n_nodes"], d["depth"], d["seed"], d["multi_parent"])
    return meta, z, cfg, edges


def _opts(tmp_path, edges, **kw):
    g = tmp_path / "graph.json"
    g.write_text(json.dumps(edges))
    o = types.SimpleNamespace(device=DEV, folder=str(tmp_path / "out"), exp_name="HGR", weights="equal", out_ratio=0.25,
                              in_ratio=0.5, from_epoch=-1, graph_path=str(g), arch="synthetic", fetch=False, load=False,
                              load_path="none", scale=1.0, num_compare=256, k=1, sample_strategy="topk", weighting="both")
    o.__dict__.update(kw)
    return o


def _model(case, golden_dir, tmp_path):
    from hgr_net_amd.hierarchy import build_hierarchy
    meta, z, cfg, edges = _tree_case(case, golden_dir)
    sd = synth.clip_state_dict(cfg, 0)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], meta["n_train"], meta["n_test"], meta["split_seed"])
    model = tree_model(_opts(tmp_path, edges), splits["all"], splits["rest"],
                       node_tokens=torch.from_numpy(z["node_tokens"].astype(np.int64)), clip_model=build_model(sd).to(DEV))
    return model, meta, cfg


@pytest.fixture(scope="module", params=["tinyvit_n90", "smallvit_n300"])
def tree(request, golden_dir, tmp_path_factory):
    model, meta, cfg = _model(request.param, golden_dir, tmp_path_factory.mktemp(request.param))
    return model, evaluate.Evaluator(model)


# ---- 1. / 2. the kernel --------------------------------------------------------------------------------------------------------------
def _recount(pred, top1, lv, targets, c2p, n_nodes):
    """main.py:139-191 for one batch, row by row, every row against the path of its own target."""
    want = dict.fromkeys(evaluate.COUNTERS, 0.0)
    for r, t in enumerate(targets):
        if t < 0 or t >= n_nodes:
            continue
        parents = list(c2p[t]) + [t]                                              # main.py:151-152
        hit = np.nonzero(pred[r] == t)[0]                                          # :139-148: correct[:k] of this row
        for k in evaluate.TOPK:
            want[f"hits@{k}"] += int(hit.size > 0 and hit[0] < k)
        want["hits_all"] += sum(int(top1[r] == p) for p in parents)                # :157-160
        dict_path = [lv[r, len(c2p[p])] for p in parents]                          # :162-176: arg-max of the level of every path node
        edge = point = 0
        if len(parents) - 1 == 0 and parents[0] == dict_path[0]:                   # :179-180
            want["path_all"] += 1
        for j in range(len(parents) - 1):                                          # :181-185
            if parents[j] == dict_path[j]:
                point += 1
            if parents[j] == dict_path[j] and parents[j + 1] == dict_path[j + 1]:
                edge += 1
        if parents[-1] == dict_path[-1]:                                           # :186-187
            point += 1
        if len(parents) - 1 != 0:                                                  # :188-190
            want["path_all"] += edge / (len(parents) - 1)
        want["point_all"] += point / len(parents)
        want["num_sample"] += 1
    return want


def _kernel_case(model, ev, rows, seed):
    """Random fp32 logits made on the CPU (the path nodes and the target of a row lifted now and then, so that every counter moves),
    per-row targets from test_index with the forced cases, and eval_rows' outputs for them.  One row: two one-row batches."""
    rng = np.random.default_rng(seed)
    n = len(model.nodes)
    te = model.test_index.cpu().numpy()
    depth = np.array([len(p) for p in model.c2p])
    in_test0 = [int(t) for t in te if depth[t] == 0]
    d0 = in_test0[0] if in_test0 else int(np.nonzero(depth == 0)[0][0])       # outside the split it can never be in the top-20: hits@k stay 0 on
    deep = int(te[np.argmax(depth[te])])                                         # both sides, path / point / hits_all are what it checks
    if rows == 1:
        batches = [np.array([d0]), np.array([deep])]
    else:
        t = te[rng.integers(0, len(te), rows)].astype(np.int64)
        t[1], t[2] = d0, deep
        if rows >= 8:
            t[0] = t[rows // 2] = t[rows - 1] = -1                               # padding at the start, in the middle and at the end
            t[3] = n + 5                                                         # out of range: padding too
        batches = [t]
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, n, generator=g)
    for r, t in enumerate(batches[0]):
        if 0 <= t < n:
            for p in list(model.c2p[t]) + [int(t)]:
                if rng.random() < 0.5:
                    logits[r, p] += 4.0
            if rng.random() < 0.4:
                logits[r, t] += float(rng.random() * 3.0)
    lv, p1, pred = ops.eval_rows(logits.to(DEV), ev.index, max(evaluate.TOPK))
    return batches, lv, p1.view(-1).contiguous(), pred


@pytest.mark.parametrize("rows", [1, 63, 65, 1100])
def test_counters_rows_vs_recount_and_single_class_kernel(tree, rows):
    model, ev = tree
    n = len(model.nodes)
    batches, lv, p1, pred = _kernel_case(model, ev, rows, 7 + rows)
    csr = ev._ancestor_csr()
    assert csr[0].dtype == torch.int32 and csr[0].numel() == n + 1
    acc = torch.zeros(9, dtype=torch.float64, device=DEV)
    acc_b = torch.zeros(9, dtype=torch.float64, device=DEV)
    want = dict.fromkeys(evaluate.COUNTERS, 0.0)
    for t in batches:
        tg = torch.from_numpy(np.asarray(t, dtype=np.int64)).to(DEV)
        ops.eval_counters_rows(pred, tg, p1, lv, *csr, acc)
        for k, v in _recount(pred.cpu().numpy(), p1.cpu().numpy(), lv.cpu().numpy(), t, model.c2p, n).items():
            want[k] += v
        for c in sorted({int(x) for x in t if 0 <= x < n}):                       # (b) the single-class kernel, one call per class
            idx = torch.from_numpy(np.nonzero(t == c)[0]).to(DEV)
            parents, _, levels32, _ = ev._parents(c)
            ops.eval_counters(pred[idx].contiguous(), None, c, p1[idx].contiguous(), lv[idx].contiguous(), parents, levels32, acc_b)
    got = dict(zip(evaluate.COUNTERS, acc.cpu().tolist()))
    got_b = dict(zip(evaluate.COUNTERS, acc_b.cpu().tolist()))
    print(f"[measured] rows={rows} kernel {got}")
    print(f"[measured] rows={rows} path_all - recount {got['path_all'] - want['path_all']:.3e}, - single-class kernel "
          f"{got['path_all'] - got_b['path_all']:.3e}; point_all {got['point_all'] - want['point_all']:.3e}, "
          f"{got['point_all'] - got_b['point_all']:.3e}")
    assert got["num_sample"] == sum(int(((t >= 0) & (t < n)).sum()) for t in batches) > 0
    for k in INT:
        assert got[k] == want[k] == got_b[k], k
    for k in RATIO:
        assert abs(got[k] - want[k]) <= RATIO_TOL and abs(got[k] - got_b[k]) <= RATIO_TOL, k
    if rows >= 63:
        assert got["point_all"] > 0 and got["path_all"] > 0 and got["hits_all"] > 0 and got["hits@20"] > 0      # the case exercises them
    # an all-padding batch (negative and too-large ids) leaves the counters bit-identical
    before = acc.clone()
    pad = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    pad[::2] = n
    ops.eval_counters_rows(pred, pad, p1, lv, *csr, acc)
    assert torch.equal(acc.view(torch.int64), before.view(torch.int64))


def test_counters_rows_do_not_depend_on_the_row_order(tree):
    model, ev = tree
    rows = 1100
    batches, lv, p1, pred = _kernel_case(model, ev, rows, 99)
    tg = torch.from_numpy(batches[0]).to(DEV)
    csr = ev._ancestor_csr()
    acc = torch.zeros(9, dtype=torch.float64, device=DEV)
    ops.eval_counters_rows(pred, tg, p1, lv, *csr, acc)
    assert float(acc[6]) > 0 and float(acc[7]) > 0
    for seed in (1, 2):
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(seed)).to(DEV)
        acc2 = torch.zeros(9, dtype=torch.float64, device=DEV)
        ops.eval_counters_rows(pred[perm].contiguous(), tg[perm].contiguous(), p1[perm].contiguous(), lv[perm].contiguous(), *csr, acc2)
        assert torch.equal(acc, acc2)


# ---- 3. - 5. evaluate.test with opts.pack_batches ------------------------------------------------------------------------------------------
SIZES = [5, 37, 64, 1, 130, 3, 20]
B = 64


class _Recorder(evaluate.Evaluator):
    """The Evaluator evaluate.test makes, kept, with the input shape and the graph generations after every packed batch."""
    made = []

    def __init__(self, model):
        super().__init__(model)
        self.shapes, self.gens = [], []
        _Recorder.made.append(self)

    def _note(self, imgs):
        m = self.model
        self.shapes.append(tuple(imgs.shape))
        self.gens.append((m._pipe.cache.gen if m._pipe is not None else None, m._graph_cache.gen))

    def add_images_rows(self, imgs, targets, want_outputs=False):
        out = super().add_images_rows(imgs, targets, want_outputs)
        self._note(imgs)
        return out

    def add_batch_rows(self, logits, targets, want_outputs=False):
        out = super().add_batch_rows(logits, targets, want_outputs)
        self._note(logits)
        return out


@pytest.fixture(scope="module")
def e2e(golden_dir, tmp_path_factory):
    """One model, one class list, every route once: packed (fused + pipelined), packed with HGR_EVAL_FUSED=0, the single-class
    evaluator on the row subsets of the same packed batches, and the existing one-class-per-batch loop."""
    model, meta, cfg = _model("smallvit_n300", golden_dir, tmp_path_factory.mktemp("e2e"))
    model.update_classifier()
    te = model.test_index.cpu().tolist()
    classes = [te[i] for i in np.random.default_rng(5).choice(len(te), len(SIZES), replace=False)]
    imgs = [synth.images(n, cfg["image_resolution"], 500 + i) for i, n in enumerate(SIZES)]

    def loader():
        return [{"img": x[None], "label": torch.full((1, x.shape[0]), c, dtype=torch.long)} for x, c in zip(imgs, classes)]

    def run(pack, env=None):
        o = types.SimpleNamespace(**vars(model.opts))
        o.test_batch_size = B
        if pack:
            o.pack_batches = True
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(evaluate, "Evaluator", _Recorder)
            for k, v in (env or {}).items():
                mp.setenv(k, v)
            out = evaluate.test(o, model, DEV, None, loader=loader(), log=False)
        ev = _Recorder.made.pop()
        return out, ev.counters(), ev

    res = {"packed": run(True), "packed_unfused": run(True, {"HGR_EVAL_FUSED": "0"})}
    ref = evaluate.Evaluator(model)                        # the single-class evaluator on the row subsets of the SAME packed batches
    for d in PackedBatches(loader(), B, DEV):
        logits = model(d["img"][0], None)
        lab = d["label"][0].cpu()
        for c in sorted(set(lab[lab >= 0].tolist())):
            ref.add_batch(logits[(lab == c).to(DEV)].contiguous(), c, want_outputs=False)
    res["per_class"] = (ref.summary(), ref.counters(), ref)
    res["groups"] = run(False)
    return res


def test_packed_evaluation_equals_single_class_counters_on_the_same_batches(e2e):
    want_s, want, _ = e2e["per_class"]
    assert want["num_sample"] == sum(SIZES)
    for route in ("packed", "packed_unfused"):
        got_s, got, _ = e2e[route]
        print(f"[measured] {route}: {got}")
        for k in INT:
            assert got[k] == want[k], (route, k)
        for k in RATIO:
            assert abs(got[k] - want[k]) <= RATIO_TOL, (route, k)
        assert got_s == want_s


def test_packed_run_is_one_shape_and_one_graph_generation(e2e):
    for route in ("packed", "packed_unfused"):
        ev = e2e[route][2]
        assert len(ev.shapes) == math.ceil(sum(SIZES) / B) == 5 and len({s[0] for s in ev.shapes}) == 1 and ev.shapes[0][0] == B
        assert any(g is not None for g in ev.gens[0])
        assert all(g == ev.gens[0] for g in ev.gens[1:]), route                  # no new generation after the first batch
    assert len(set(e2e["packed"][2].shapes)) == 1                                # the fused route records the image batches themselves
    assert e2e["groups"][2].shapes == []                                         # flag off: the packed entry points are never reached


def test_packed_run_against_the_one_class_per_batch_run(e2e):
    """Different batch sizes take different GEMM plans: logits may round differently and near-ties may flip, so only num_sample
    is asserted; everything else is printed."""
    _, packed, _ = e2e["packed"]
    _, groups, _ = e2e["groups"]
    for k in evaluate.COUNTERS:
        print(f"[measured] {k}: packed {packed[k]:.6f} - one class per batch {groups[k]:.6f} = {packed[k] - groups[k]:+.3e}")
    assert packed["num_sample"] == groups["num_sample"] == sum(SIZES)


# ---- 6. flag off ---------------------------------------------------------------------------------------------------------------------
def test_flag_off_is_the_existing_loop(golden_dir, tmp_path):
    model, meta, cfg = _model("smallvit_n300", golden_dir, tmp_path)
    model.update_classifier()
    assert not hasattr(model.opts, "pack_batches")
    ev = evaluate.Evaluator(model)
    for i in range(meta["batches"]):
        img = synth.images(meta["bsz"], cfg["image_resolution"], meta["image_seed0"] + i).to(DEV)
        ev.add_batch(model(img, None), meta["targets"][i])

    def loader():
        for i in range(meta["batches"]):
            yield {"img": synth.images(meta["bsz"], cfg["image_resolution"], meta["image_seed0"] + i)[None],
                   "label": torch.full((1, meta["bsz"]), meta["targets"][i], dtype=torch.long)}
    out = evaluate.test(model.opts, model, DEV, None, loader=loader(), log=False)
    assert out == ev.summary()
