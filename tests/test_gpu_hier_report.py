"""GPU: the hierarchy report - hgr_eval_report_rows against a per-row restatement of its definitions (include/hgr.h) on model
hierarchies and on a hand-built CSR, its independence of the row order and of the cut into launches, its sums against the existing
counters, and evaluate.test with opts.hier_report end to end on every route."""
import json
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
COLS = ops.REPORT_DEPTH_COLS
K = max(evaluate.TOPK)


# ---- helpers in the style of test_gpu_packed_eval.py (copied: test modules do not import each other) -----------------------------------
def _cfg(z):
    cfg = json.loads(str(z["config"])) if not isinstance(z, dict) else z
    if isinstance(cfg["vision_layers"], list):
        cfg["vision_layers"] = tuple(cfg["vision_layers"])
    return cfg


def _tree_case(case, golden_dir):
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


def _kernel_case(model, ev, rows, seed):
    """Random fp32 logits made on the CPU (the path nodes and the target of a row lifted now and then, so that every count moves),
    per-row targets from test_index with the forced cases (padding at the start, in the middle and at the end, one target out of
    range, a depth-0 target, the deepest test target), and eval_rows' outputs for them.  One row: two one-row batches."""
    rng = np.random.default_rng(seed)
    n = len(model.nodes)
    te = model.test_index.cpu().numpy()
    depth = np.array([len(p) for p in model.c2p])
    in_test0 = [int(t) for t in te if depth[t] == 0]
    d0 = in_test0[0] if in_test0 else int(np.nonzero(depth == 0)[0][0])
    deep = int(te[np.argmax(depth[te])])
    if rows == 1:
        batches = [np.array([d0]), np.array([deep])]
    else:
        t = te[rng.integers(0, len(te), rows)].astype(np.int64)
        t[1], t[2] = d0, deep
        if rows >= 8:
            t[0] = t[rows // 2] = t[rows - 1] = -1
            t[3] = n + 5
        batches = [t]
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, n, generator=g)
    for r, t in enumerate(batches[0]):
        if 0 <= t < n:
            for p in list(model.c2p[t]) + [int(t)]:
                if rng.random() < 0.6:
                    logits[r, p] += 4.0
            if rng.random() < 0.4:
                logits[r, t] += float(rng.random() * 3.0)
    lv, p1, pred = ops.eval_rows(logits.to(DEV), ev.index, K)
    return batches, lv, p1.view(-1).contiguous(), pred


# ---- the restatement: include/hgr.h's definitions, one row at a time ---------------------------------------------------------------------
def _restate(pred, top1, lv, targets, ptr, nodes, levels, n_nodes, table=None):
    """The table hgr_eval_report_rows must produce for these rows, from numpy arrays, as a list of Python ints."""
    T = [0] * ops.REPORT_LEN if table is None else table
    k, n_levels = pred.shape[1], lv.shape[1]

    def path(x):                                         # P(x); None outside the tree
        return [int(v) for v in nodes[ptr[x]:ptr[x + 1]]] if 0 <= x < n_nodes else None

    def parent(x):
        p = path(x)
        return p[len(p) - 2] if len(p) >= 2 else "root"

    for r, t in enumerate(targets):
        t = int(t)
        pt = path(t)
        if pt is None or not 1 <= len(pt) <= 32:        # padding
            continue
        L = len(pt)
        plev = [int(v) for v in levels[ptr[t]:ptr[t] + L]]

        def prefix(x):                                   # c(x, t), or None for an "unknown" prediction
            px = path(int(x))
            if px is None or not 1 <= len(px) <= 32:
                return None, None
            c = 0
            while c < min(len(px), L) and px[c] == pt[c]:
                c += 1
            return c, len(px)

        def height(x):
            c, _ = prefix(x)
            return L if c is None else L - c

        def dist(x):
            c, lx = prefix(x)
            return ops.REPORT_DIST_UNKNOWN if c is None else lx + L - 2 * c

        row = dict.fromkeys(COLS, 0)
        row["rows"] = 1
        hit = [i for i in range(k) if int(pred[r, i]) == t]
        for kk in evaluate.TOPK:
            row[f"hit@{kk}"] = int(bool(hit) and hit[0] < kk)
        row["anc_hit"] = sum(int(p == int(top1[r])) for p in pt)
        q = [int(lv[r, l]) if 0 <= l < n_levels else None for l in plev]
        match = [q[i] == pt[i] for i in range(L)]
        row["point"] = sum(match)
        row["edge"] = int(match[0]) if L == 1 else sum(int(match[i] and match[i + 1]) for i in range(L - 1))
        valid = all(v is not None and 0 <= v < n_nodes for v in q)
        row["chain"] = int(valid and parent(q[0]) == "root" and all(parent(q[i + 1]) == q[i] for i in range(L - 1)))
        for c, name in enumerate(COLS):
            T[ops.REPORT_DEPTH + L * len(COLS) + c] += row[name]
        for i in range(L):
            T[ops.REPORT_LEVEL + 2 * i] += 1
            T[ops.REPORT_LEVEL + 2 * i + 1] += int(match[i])
        T[ops.REPORT_DIST_TEST + dist(pred[r, 0])] += 1
        T[ops.REPORT_DIST_ALL + dist(top1[r])] += 1
        for i, kk in enumerate(ops.REPORT_HEIGHT_K):
            T[ops.REPORT_HEIGHT + i] += sum(height(pred[r, s]) for s in range(min(kk, k)))
    return T


def _csr_np(csr):
    return [x.cpu().numpy() for x in csr]


def _launch(pred, tg, p1, lv, csr, table=None):
    table = torch.zeros(ops.REPORT_LEN, dtype=torch.int64, device=DEV) if table is None else table
    ops.eval_report_rows(pred, tg, p1, lv, *csr, table)
    return table


def _depth_col(T, name):
    """Column ``name`` of DEPTH as a list over L = 0..32."""
    c = COLS.index(name)
    return [int(T[ops.REPORT_DEPTH + L * len(COLS) + c]) for L in range(ops.REPORT_MAXL + 1)]


# ---- 1. the kernel against the restatement, 4. against the existing counters -------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 65, 1100])
def test_report_rows_vs_restatement_and_counters(tree, rows):
    """1100 rows = more than two passes of a 512-lane stride loop (and 18 passes of the 64 waves the kernel's grid holds)."""
    model, ev = tree
    n = len(model.nodes)
    batches, lv, p1, pred = _kernel_case(model, ev, rows, 11 + rows)
    csr = ev._ancestor_csr()
    ptr, nodes, levels = _csr_np(csr)
    table = torch.zeros(ops.REPORT_LEN, dtype=torch.int64, device=DEV)
    acc = torch.zeros(9, dtype=torch.float64, device=DEV)
    want = [0] * ops.REPORT_LEN
    for t in batches:
        tg = torch.from_numpy(np.asarray(t, dtype=np.int64)).to(DEV)
        ops.eval_counters_rows(pred, tg, p1, lv, *csr, acc)
        _launch(pred, tg, p1, lv, csr, table)
        _restate(pred.cpu().numpy(), p1.cpu().numpy(), lv.cpu().numpy(), t, ptr, nodes, levels, n, want)
    got = table.cpu().tolist()
    bad = [i for i in range(ops.REPORT_LEN) if got[i] != want[i]]
    print(f"[measured] rows={rows}: {sum(1 for v in got if v)} non-zero entries, {len(bad)} differ {[(i, got[i], want[i]) for i in bad[:8]]}")
    assert got == want
    # 4. tied to hgr_eval_counters_rows on the same outputs
    c = dict(zip(evaluate.COUNTERS, acc.cpu().tolist()))
    assert sum(_depth_col(got, "rows")) == c["num_sample"] == sum(int(((t >= 0) & (t < n)).sum()) for t in batches) > 0
    for kk in evaluate.TOPK:
        assert sum(_depth_col(got, f"hit@{kk}")) == c[f"hits@{kk}"], kk
    assert sum(_depth_col(got, "anc_hit")) == c["hits_all"]
    edge, point = _depth_col(got, "edge"), _depth_col(got, "point")
    path_all = edge[1] + sum(edge[L] / (L - 1) for L in range(2, ops.REPORT_MAXL + 1))
    point_all = sum(point[L] / L for L in range(1, ops.REPORT_MAXL + 1))
    print(f"[measured] rows={rows}: path_all {path_all!r} vs {c['path_all']!r}, point_all {point_all!r} vs {c['point_all']!r}")
    # double sums of fewer than 1e4 terms of magnitude at most 1: 1e-9 relative
    assert abs(path_all - c["path_all"]) <= 1e-9 * max(abs(c["path_all"]), 1e-300)
    assert abs(point_all - c["point_all"]) <= 1e-9 * max(abs(c["point_all"]), 1e-300)
    assert sum(got[ops.REPORT_LEVEL + 2 * i + 1] for i in range(ops.REPORT_MAXL)) == sum(point)
    assert got[ops.REPORT_DIST_TEST] == sum(_depth_col(got, "hit@1"))
    assert sum(got[ops.REPORT_DIST_TEST:ops.REPORT_DIST_TEST + ops.REPORT_DIST_BINS]) == c["num_sample"]
    assert sum(got[ops.REPORT_DIST_ALL:ops.REPORT_DIST_ALL + ops.REPORT_DIST_BINS]) == c["num_sample"]
    if rows >= 63:
        assert sum(point) > 0 and sum(edge) > 0 and sum(_depth_col(got, "chain")) > 0 and got[ops.REPORT_HEIGHT + 4] > 0     # the case exercises them
    # an all-padding batch adds nothing
    pad = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    pad[::2] = n
    before = table.clone()
    _launch(pred, pad, p1, lv, csr, table)
    assert torch.equal(table, before)


# ---- 2. a hand-built CSR, no model -----------------------------------------------------------------------------------------------------
def _hand_csr():
    """40 nodes.  0..31: one chain, node i has the path [0..i] (node 31: 32 nodes, the maximum).  32: a 33-node path.  33: an empty
    range.  34: [0, 1, 34] (a sibling of 2).  37: a second root.  36: [37, 1, 36] - equal to [0, 1, 2] at position 1, different at
    position 0.  38: [37, 38].  35: [37, 38, 35].  39: [0, 39].  The level of a path node is its position (node 32's own: 31)."""
    paths = {i: list(range(i + 1)) for i in range(32)}
    paths.update({32: list(range(33)), 33: [], 34: [0, 1, 34], 35: [37, 38, 35], 36: [37, 1, 36], 37: [37], 38: [37, 38], 39: [0, 39]})
    ptr, nodes, levels = [0], [], []
    for x in range(40):
        nodes += paths[x]
        levels += [min(i, 31) for i in range(len(paths[x]))]
        ptr.append(len(nodes))
    return paths, tuple(torch.tensor(a, dtype=torch.int32, device=DEV) for a in (ptr, nodes, levels))


def _one_row(target, pred0, top1, csr, lv_row=None, k=K):
    pred = torch.full((1, k), -1, dtype=torch.int32, device=DEV)
    pred[0, 0] = pred0
    lv = torch.full((1, 32), 33, dtype=torch.int32, device=DEV) if lv_row is None else torch.tensor([lv_row], dtype=torch.int32, device=DEV)
    return _launch(pred, torch.tensor([target], dtype=torch.int64, device=DEV), torch.tensor([top1], dtype=torch.int32, device=DEV), lv, csr).cpu().tolist()


def test_hand_built_csr_rows_by_hand():
    """Values worked out by hand from the definitions, independent of the restatement."""
    paths, csr = _hand_csr()
    # target 2 = [0, 1, 2] against 36 = [37, 1, 36]: the match at position 1 is no common prefix - c = 0, dist 6, height 3; top-1 = the
    # 33-node node: unknown.  The other 19 predictions are -1: unknown, height 3 each.
    T = _one_row(2, 36, 32, csr)
    assert T[ops.REPORT_DIST_TEST + 6] == 1 and T[ops.REPORT_DIST_ALL + ops.REPORT_DIST_UNKNOWN] == 1
    assert T[ops.REPORT_HEIGHT:ops.REPORT_HEIGHT + 5] == [3, 6, 15, 30, 60]
    assert T[ops.REPORT_DEPTH + 3 * len(COLS):ops.REPORT_DEPTH + 4 * len(COLS)] == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert T[ops.REPORT_LEVEL:ops.REPORT_LEVEL + 8] == [1, 0, 1, 0, 1, 0, 0, 0] and sum(T) == 1 + 3 + 2 + 114
    # the 33-node path as a target counts nothing, and so does the empty range
    assert not any(_one_row(32, 0, 0, csr)) and not any(_one_row(33, 0, 0, csr))
    # the 33-node path as a prediction: the unknown bin, height Lt = 32; top-1 = the target itself: distance 0, 1 path node hit
    lv_row = list(range(32))
    T = _one_row(31, 32, 31, csr, lv_row)
    assert T[ops.REPORT_DIST_TEST + ops.REPORT_DIST_UNKNOWN] == 1 and T[ops.REPORT_DIST_ALL + 0] == 1
    assert T[ops.REPORT_HEIGHT:ops.REPORT_HEIGHT + 5] == [32, 64, 160, 320, 640]
    assert T[ops.REPORT_DEPTH + 32 * len(COLS):ops.REPORT_DEPTH + 33 * len(COLS)] == [1, 0, 0, 0, 0, 0, 1, 32, 31, 1]    # every level matched: a chain
    assert T[ops.REPORT_LEVEL:ops.REPORT_LEVEL + 64] == [1, 1] * 32
    # a -1 at a path level: that level unmatched, no chain; 30 is the target's parent: distance 1, height 1, k = 1 leaves the other K alone
    lv_row[7] = -1
    T = _one_row(31, 30, 30, csr, lv_row, k=1)
    assert T[ops.REPORT_DEPTH + 32 * len(COLS):ops.REPORT_DEPTH + 33 * len(COLS)] == [1, 0, 0, 0, 0, 0, 1, 31, 29, 0]
    assert T[ops.REPORT_DIST_TEST + 1] == 1 and T[ops.REPORT_DIST_ALL + 1] == 1 and T[ops.REPORT_HEIGHT:ops.REPORT_HEIGHT + 5] == [1] * 5
    # every level of [37, 1, 36] matched, but 1 does not hang under 37: no chain; the hit is at position 0
    T = _one_row(36, 36, 1, csr, [37, 1, 36] + [0] * 29)
    assert T[ops.REPORT_DEPTH + 3 * len(COLS):ops.REPORT_DEPTH + 4 * len(COLS)] == [1, 1, 1, 1, 1, 1, 1, 3, 2, 0]
    assert T[ops.REPORT_DIST_TEST + 0] == 1 and T[ops.REPORT_DIST_ALL + 5] == 1          # [0, 1] against [37, 1, 36]: 2 + 3 - 0


@pytest.mark.parametrize("k", [K, 3])
def test_hand_built_csr_vs_restatement(k):
    paths, csr = _hand_csr()
    ptr, nodes, levels = _csr_np(csr)
    rng = np.random.default_rng(40 + k)
    targets = np.array([31, 32, 33, 36, 2, 0, 38, -1, 45, 35, 34, 39, 37, 31, 2, 36, 30, 17] * 3, dtype=np.int64)
    rows = len(targets)
    pred = rng.integers(-1, 42, (rows, k)).astype(np.int32)          # ids outside [0, 40) included
    pred[0, 0], pred[3, 0], pred[4, 0], pred[5, 1], pred[13, 0] = 32, 2, 36, 0, 31
    top1 = rng.integers(-1, 42, rows).astype(np.int32)
    top1[0], top1[4] = 32, 33
    lv = rng.integers(-1, 41, (rows, 32)).astype(np.int32)
    for r, t in enumerate(targets):
        if 0 <= t < 40 and r % 3 != 2:                                # two rows in three: the path itself, sometimes damaged
            for i, p in enumerate(paths[int(t)][:32]):
                lv[r, i] = p
            if r % 3 == 1 and paths[int(t)]:
                lv[r, int(rng.integers(0, min(len(paths[int(t)]), 32)))] = -1
    want = _restate(pred, top1, lv, targets, ptr, nodes, levels, 40)
    got = _launch(*(torch.from_numpy(a).to(DEV) for a in (pred, targets, top1, lv)), csr).cpu().tolist()
    bad = [i for i in range(ops.REPORT_LEN) if got[i] != want[i]]
    print(f"[measured] k={k}: {sum(1 for v in got if v)} non-zero entries, {len(bad)} differ {[(i, got[i], want[i]) for i in bad[:8]]}")
    assert got == want
    n_valid = sum(1 for t in targets if 0 <= t < 40 and 1 <= len(paths[int(t)]) <= 32)
    assert sum(_depth_col(got, "rows")) == n_valid == rows - 4 * 3
    assert _depth_col(got, "chain")[32] > 0 and got[ops.REPORT_DIST_TEST + ops.REPORT_DIST_UNKNOWN] > 0


# ---- 3. order and split independence ---------------------------------------------------------------------------------------------------
def test_report_does_not_depend_on_row_order_or_on_the_cut_into_launches(tree):
    model, ev = tree
    rows = 1100
    batches, lv, p1, pred = _kernel_case(model, ev, rows, 99)
    tg = torch.from_numpy(batches[0]).to(DEV)
    csr = ev._ancestor_csr()
    whole = _launch(pred, tg, p1, lv, csr)
    assert int(whole[ops.REPORT_HEIGHT + 4]) > 0
    for seed in (1, 2):
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(seed)).to(DEV)
        assert torch.equal(whole, _launch(pred[perm].contiguous(), tg[perm].contiguous(), p1[perm].contiguous(), lv[perm].contiguous(), csr))
    parts = torch.zeros_like(whole)
    for lo, hi in ((0, 1), (1, 8), (8, rows)):
        _launch(pred[lo:hi].contiguous(), tg[lo:hi].contiguous(), p1[lo:hi].contiguous(), lv[lo:hi].contiguous(), csr, parts)
    assert torch.equal(whole, parts)


# ---- 5. / 6. evaluate.test with opts.hier_report ----------------------------------------------------------------------------------------
SIZES = [5, 37, 64, 1, 130, 3, 20]
B = 64


@pytest.fixture(scope="module")
def e2e(golden_dir, tmp_path_factory):
    """The small ViT tree model (the smallest fixture the fused evaluation route takes), ragged one-class batches, every route once:
    fused + pipelined, HGR_EVAL_FUSED=0, packed, and the flag off - with every call of the report wrapper counted."""
    tmp = tmp_path_factory.mktemp("hier")
    model, meta, cfg = _model("smallvit_n300", golden_dir, tmp)
    model.update_classifier()
    te = model.test_index.cpu().tolist()
    classes = [te[i] for i in np.random.default_rng(5).choice(len(te), len(SIZES), replace=False)]
    imgs = [synth.images(n, cfg["image_resolution"], 500 + i) for i, n in enumerate(SIZES)]
    made, calls = [], []

    class Keep(evaluate.Evaluator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    def loader():
        return [{"img": x[None], "label": torch.full((1, x.shape[0]), c, dtype=torch.long)} for x, c in zip(imgs, classes)]

    def run(name, report=True, pack=False, fused="1"):
        o = types.SimpleNamespace(**vars(model.opts))
        o.test_batch_size = B
        path = tmp / f"{name}.json"
        o.hier_report = str(path) if report else None
        if pack:
            o.pack_batches = True
        real = ops.eval_report_rows
        n0 = len(calls)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(evaluate, "Evaluator", Keep)
            mp.setattr(ops, "eval_report_rows", lambda *a, **kw: (calls.append(name), real(*a, **kw))[1])
            mp.setenv("HGR_EVAL_FUSED", fused)
            out = evaluate.test(o, model, DEV, None, loader=loader(), log=False)
        return {"out": out, "path": path, "ev": made.pop(), "calls": len(calls) - n0}

    res = {"fused": run("fused"), "unfused": run("unfused", fused="0"), "packed": run("packed", pack=True), "off": run("off", report=False)}
    # the restatement on forward() + eval_rows of the same one-class batches
    ev = evaluate.Evaluator(model)
    ptr, nodes, levels = _csr_np(ev._ancestor_csr())
    want = [0] * ops.REPORT_LEN
    for x, c in zip(imgs, classes):
        lv, p1, pred = ops.eval_rows(model(x.to(DEV), None), ev.index, K)
        _restate(pred.cpu().numpy(), p1.view(-1).cpu().numpy(), lv.cpu().numpy(), [c] * x.shape[0], ptr, nodes, levels, len(model.nodes), want)
    res["want"] = want
    return res


def test_report_files_of_the_three_routes_are_identical_and_equal_the_restatement(e2e):
    texts = {r: e2e[r]["path"].read_text() for r in ("fused", "unfused", "packed")}
    rep = json.loads(texts["fused"])
    print(f"[measured] {evaluate.format_report(rep)}")
    print(f"[measured] launches: { {r: e2e[r]['calls'] for r in ('fused', 'unfused', 'packed', 'off')} }")
    assert rep["num_sample"] == sum(SIZES)
    want = evaluate.report_from_table(torch.tensor(e2e["want"], dtype=torch.int64))
    assert rep == json.loads(json.dumps(want))
    assert texts["unfused"] == texts["fused"] and texts["packed"] == texts["fused"]
    assert e2e["fused"]["calls"] == e2e["unfused"]["calls"] == len(SIZES) and e2e["packed"]["calls"] == -(-sum(SIZES) // B)
    for r in ("fused", "unfused", "packed"):
        assert e2e[r]["ev"].report_table().tolist() == e2e["want"], r


def test_metric_string_is_the_one_of_a_run_without_the_flag(e2e):
    assert e2e["fused"]["out"] == e2e["unfused"]["out"] == e2e["off"]["out"]


def test_flag_off_launches_nothing_and_writes_nothing(e2e):
    off = e2e["off"]
    assert off["ev"].report is None and off["calls"] == 0 and not off["path"].exists()
    with pytest.raises(AssertionError):
        off["ev"].report_table()
