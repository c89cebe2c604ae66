"""GPU: hierarchy-path decoding - hgr_path_scores against an fp64 restatement of its definition (include/hgr.h) on model hierarchies
and on a hand-built CSR, its independence of the cut into launches, the arguments it rejects, and the decoding mode built on it:
Evaluator(decode="path"), evaluate.predict and evaluate.test with --decode path on every route."""
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import _lib, evaluate, ops, synth
from hgr_net_amd.clip.model import build_model
from hgr_net_amd.model import tree_model
from oracle import tree_ref

DEV = "cuda"
K = max(evaluate.TOPK)
U = 2.0 ** -24                       # unit roundoff of fp32
METHODS = ("equal", "increasing", "decreasing", "nl_increasing", "nl_decreasing", "adaptive")


# ---- helpers in the style of test_gpu_hier_report.py (copied: test modules do not import each other) ------------------------------------
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
    o = types.SimpleNamespace(device=DEV, folder=str(tmp_path / "out"), exp_name="HGR", weights="adaptive", out_ratio=0.25,
                              in_ratio=0.5, from_epoch=-1, graph_path=str(g), arch="synthetic", fetch=False, load=False,
                              load_path="none", scale=1.0, num_compare=256, k=1, sample_strategy="topk", weighting="both")
    o.__dict__.update(kw)
    return o


def _model(case, golden_dir, tmp_path):
    """opts.weights = "adaptive": the model has a layer_weight.  Its initial value (1 / nodes of the level, 1.0 for a single root)
    makes softmax(100 ** w) a one-hot row; here it is set to values in [0, 0.3), which give every path position a real weight."""
    from hgr_net_amd.hierarchy import build_hierarchy
    meta, z, cfg, edges = _tree_case(case, golden_dir)
    sd = synth.clip_state_dict(cfg, 0)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], meta["n_train"], meta["n_test"], meta["split_seed"])
    model = tree_model(_opts(tmp_path, edges), splits["all"], splits["rest"],
                       node_tokens=torch.from_numpy(z["node_tokens"].astype(np.int64)), clip_model=build_model(sd).to(DEV))
    with torch.no_grad():
        model.layer_weight.copy_((0.3 * torch.rand(model.layer_weight.shape, generator=torch.Generator().manual_seed(3))).to(DEV))
    return model, meta, cfg


# ---- the restatement: include/hgr.h's definition in float64, one node column at a time -------------------------------------------------
def _restate(x, ptr, nodes, wtab, n_nodes):
    """(S64, A, L) on the CPU: S64[r, n] = sum_j W[L][j] x[r, P(n)[j]] in float64 (the products of two fp32 values are exact in
    float64), A[r, n] = sum_j |W[L][j] x[r, P(n)[j]]|, L[n] = the path length, 0 for a pass-through column (S64 = x, A = 0)."""
    x, w = x.detach().cpu().double(), wtab.detach().cpu().double()
    ptr, nodes = ptr.cpu().tolist(), nodes.cpu().tolist()
    rows = x.shape[0]
    s, a, ls = torch.empty(rows, n_nodes, dtype=torch.float64), torch.zeros(rows, n_nodes, dtype=torch.float64), [0] * n_nodes
    for n in range(n_nodes):
        o, L = ptr[n], ptr[n + 1] - ptr[n]
        if L < 1 or L > 32:
            s[:, n] = x[:, n]
            continue
        ls[n] = L
        acc = torch.zeros(rows, dtype=torch.float64)
        for j in range(L):
            c = nodes[o + j]
            if 0 <= c < n_nodes:
                t = w[L, j] * x[:, c]
                acc += t
                a[:, n] += t.abs()
        s[:, n] = acc
    return s, a, torch.tensor(ls, dtype=torch.float64)


def _bound(a, ls):
    """|S - S64| <= (L + 1) 2^-24 sum_j |W[L][j] x[a_j]|: L sequential fused multiply-adds, one rounding each (gamma_L <= (L + 1) u)."""
    return (ls + 1.0)[None, :] * U * a


@pytest.fixture(scope="module", params=["tinyvit_n90", "smallvit_n300"])
def tree(request, golden_dir, tmp_path_factory):
    """(model, ancestor CSR on the device, 64 rows of 0.05 * randn logits, seed 5, on the CPU): shared, never written."""
    model, meta, cfg = _model(request.param, golden_dir, tmp_path_factory.mktemp(request.param))
    ptr, nodes, _ = evaluate.Evaluator(model)._ancestor_csr()
    n = len(model.nodes)
    assert ptr.numel() == n + 1 and max(len(p) for p in model.c2p) + 1 == 8            # paths of up to 8 nodes
    x = 0.05 * torch.randn(64, n, generator=torch.Generator().manual_seed(5))
    return model, ptr, nodes, x


def _dyadic_table():
    w = torch.zeros(33, 32)
    for L in range(1, 33):
        w[L, :L - 1] = 1.0 / 64
        w[L, L - 1] = 1.0 - (L - 1) / 64
    return w


def _random_convex_table(seed):
    w = torch.zeros(33, 32)
    g = torch.Generator().manual_seed(seed)
    for L in range(1, 33):
        v = torch.rand(L, generator=g) + 0.05
        w[L, :L] = v / v.sum()
    return w


# ---- 1. exact arithmetic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_dyadic_inputs_give_the_exact_sums_in_views_of_wider_buffers(tree, rows):
    """Logits k / 256 and weights 1 / 64 (the node itself: 1 - (L - 1) / 64): every product is a multiple of 2^-14 and every partial
    sum is exact in fp32, so the kernel must return the float64 sum itself.  ld = n + 8, ld_out = n + 24; the extra output columns
    keep their sentinel."""
    model, ptr, nodes, _ = tree
    n = len(model.nodes)
    xb = torch.randint(-256, 257, (rows, n + 8), generator=torch.Generator().manual_seed(100 + rows)).float() / 256
    w = _dyadic_table()
    xd = xb.to(DEV)
    ob = torch.full((rows, n + 24), 7.5, device=DEV)
    s = ops.path_scores(xd[:, :n], ptr, nodes, w.to(DEV), out=ob[:, :n])
    assert s.shape == (rows, n) and s.data_ptr() == ob.data_ptr() and xd[:, :n].stride(0) == n + 8 and s.stride(0) == n + 24
    s64, _, ls = _restate(xb[:, :n], ptr, nodes, w, n)
    assert int((ls > 1).sum()) > n // 2 and int(ls.max()) == 8
    got = s.cpu()
    print(f"[measured] rows={rows} n={n}: max |S - S64| = {float((got.double() - s64).abs().max()):.3e}")
    assert torch.equal(got, s64.float()) and torch.equal(got.double(), s64)
    assert bool((ob[:, n:] == 7.5).all()) and torch.equal(xd.cpu(), xb)


# ---- 2. real weights ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(tree):
    """Per method: (weight table on the device, S of the 64 shared rows from one launch, S64, elementwise bound)."""
    model, ptr, nodes, x = tree
    n = len(model.nodes)
    xd = x.to(DEV)
    out = {}
    for method in METHODS:
        w = evaluate.path_weight_table(model, method)
        s = ops.path_scores(xd, ptr, nodes, w)
        s64, a, ls = _restate(x, ptr, nodes, w, n)
        out[method] = (w, s, s64, _bound(a, ls))
    return out


@pytest.mark.parametrize("method", METHODS)
def test_real_weights_within_the_bound_of_sequential_fmas(tree, real, method):
    model, ptr, nodes, x = tree
    w, s, s64, bound = real[method]
    for L in range(1, model.max_depth + 2):
        assert torch.equal(w[L, :L], model.get_weights(method, L).detach()), (method, L)
    err = (s.cpu().double() - s64).abs()
    print(f"[measured] {method}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
          f"|S| max {float(s64.abs().max()):.3e}")
    assert bool((err <= bound).all())
    assert float(s64.abs().max()) > 1e-3 and not torch.equal(s.cpu(), x)          # the case is no pass-through


# ---- 3. a hand-built CSR, no model -----------------------------------------------------------------------------------------------------
def _hand_paths():
    """70 nodes.  0: [0] (L = 1).  1: [0, 1].  2: 32 nodes, [0, 38..67, 2] (higher-numbered columns).  3: an empty range.  4: 33 nodes,
    [0, 36..67] (both pass-through).  5: [0, 5].  6: [0, 75, 6] - 75 = n_nodes + 5, skipped.  7: [-1, 7] - skipped likewise.  69: [0, 5,
    69] (lower-numbered columns).  Every third of the rest: [0, 5, n]; the others [0, n]: node 0 is on most paths."""
    paths = {0: [0], 1: [0, 1], 2: [0] + list(range(38, 68)) + [2], 3: [], 4: [0] + list(range(36, 68)), 5: [0, 5], 6: [0, 75, 6], 7: [-1, 7]}
    for n in range(8, 70):
        paths[n] = [0, 5, n] if n % 3 == 0 or n == 69 else [0, n]
    assert len(paths[2]) == 32 and len(paths[4]) == 33
    ptr, nodes = [0], []
    for n in range(70):
        nodes += paths[n]
        ptr.append(len(nodes))
    return paths, torch.tensor(ptr, dtype=torch.int32), torch.tensor(nodes, dtype=torch.int32)


def test_hand_built_csr():
    """3 rows (fewer than one row group).  The logits are a view at column 8 of a buffer of n_nodes + 24 columns: the ids 75 and -1 point
    at valid memory whether they are skipped or not - a missing check gives a wrong number (the buffer holds 1000 there), no bad access."""
    paths, ptr, nodes = _hand_paths()
    n = 70
    g = torch.Generator().manual_seed(70)
    buf = torch.full((3, n + 24), 1000.0)
    buf[:, 8:8 + n] = 0.05 * torch.randn(3, n, generator=g)
    x = buf[:, 8:8 + n]
    w = _random_convex_table(71)
    s = ops.path_scores(buf.to(DEV)[:, 8:8 + n], ptr.to(DEV), nodes.to(DEV), w.to(DEV)).cpu()
    s64, a, ls = _restate(x, ptr, nodes, w, n)
    err = (s.double() - s64).abs()
    print(f"[measured] hand-built: max err {float(err.max()):.3e}, max |S| {float(s.abs().max()):.3e}")
    assert bool((err <= _bound(a, ls)).all()) and float(s.abs().max()) < 1.0
    assert torch.equal(s[:, 3], x[:, 3]) and torch.equal(s[:, 4], x[:, 4])       # the empty and the 33-node range: the logit itself
    assert torch.equal(s[:, 0], x[:, 0])                                          # L = 1 with weight 1
    assert ls[2] == 32 and ls[3] == ls[4] == 0
    # by hand, in fp32: node 6 = W[3][0] x[0] + W[3][2] x[6] (75 skipped), node 7 = W[2][1] x[7] (-1 skipped)
    w3, w2 = w[3], w[2]
    assert torch.allclose(s[:, 6], w3[0] * x[:, 0] + w3[2] * x[:, 6], rtol=0, atol=1e-7)
    assert torch.allclose(s[:, 7], w2[1] * x[:, 7], rtol=0, atol=1e-7)


def test_one_node_and_more_row_blocks_than_the_grid_holds():
    """n_nodes = 1, and with it the one size at which the launch takes another path: more 32-row blocks than the grid's second
    dimension holds (65 535), so that blocks take a second round of rows.  One column keeps that at 8 MB."""
    ptr, nodes = torch.tensor([0, 1], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV)
    w = _random_convex_table(1).to(DEV)
    x = torch.randn(3, 1, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(ops.path_scores(x, ptr, nodes, w), x)
    rows = 65535 * 32 + 37
    x = torch.randn(rows, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = torch.full((rows + 1, 1), 7.5, device=DEV)
    s = ops.path_scores(x, ptr, nodes, w, out=out[:rows])
    assert torch.equal(s, x) and float(out[rows, 0]) == 7.5


# ---- 4. independence of the cut --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["increasing", "adaptive"])
def test_scores_do_not_depend_on_the_cut_into_launches(tree, real, method):
    model, ptr, nodes, x = tree
    w, whole, _, _ = real[method]
    xd = x.to(DEV)
    ones = torch.cat([ops.path_scores(xd[r:r + 1], ptr, nodes, w) for r in range(64)])
    split = torch.cat([ops.path_scores(xd[:5], ptr, nodes, w), ops.path_scores(xd[5:], ptr, nodes, w)])
    assert torch.equal(whole, ones) and torch.equal(whole, split)


# ---- 5. / 6. the Evaluator ---------------------------------------------------------------------------------------------------------------
def _targets(model, rows, seed, pad):
    te = model.test_index.cpu().numpy()
    t = te[np.random.default_rng(seed).integers(0, len(te), rows)].astype(np.int64)
    if pad:
        t[0] = t[rows // 2] = t[rows - 1] = -1
        t[3] = len(model.nodes) + 5
    return torch.from_numpy(t).to(DEV)


def _lifted(model, x, targets):
    """The shared logits with the path of every row's target lifted now and then, so that every counter moves."""
    rng = np.random.default_rng(17)
    x = x.clone()
    for r, t in enumerate(targets.cpu().tolist()):
        if 0 <= t < len(model.nodes):
            for p in list(model.c2p[t]) + [t]:
                if rng.random() < 0.7:
                    x[r, p] += 0.2
    return x.to(DEV)


def _state(ev, out):
    return [ev.acc.cpu(), ev.report_table()] + [o.cpu().clone() for o in out]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def _run_class(ev, logits, target):
    return _state(ev, ev.add_batch(logits, target, torch.full((logits.shape[0],), target, dtype=torch.int64, device=DEV)))


def _run_rows(ev, logits, targets):
    return _state(ev, ev.add_batch_rows(logits, targets, want_outputs=True))


def test_self_weights_are_flat_decoding(tree):
    model, ptr, nodes, x = tree
    xd = x.to(DEV)
    assert torch.equal(ops.path_scores(xd, ptr, nodes, evaluate.path_weight_table(model, "self")), xd)
    tg = _targets(model, 64, 8, pad=True)
    logits = _lifted(model, x, tg)
    target = int(model.test_index[3])
    flat, path = evaluate.Evaluator(model, report=True), evaluate.Evaluator(model, report=True, decode="path", decode_weights="self")
    a, b = _run_class(flat, logits, target), _run_class(path, logits, target)
    assert _same(a, b) and float(a[0][8]) == 64
    a, b = _run_rows(flat, logits, tg), _run_rows(path, logits, tg)                # accumulated on top of the class batch
    assert _same(a, b) and float(a[0][8]) == 64 + 60 and int(a[1].sum()) > 0
    assert flat._scores is None and flat._wtab is None and path._scores is not None


@pytest.mark.parametrize("method", ["increasing", "equal"])
def test_path_decoding_is_eval_rows_on_the_path_scores(tree, method):
    model, ptr, nodes, x = tree
    tg = _targets(model, 64, 9, pad=True)
    logits = _lifted(model, x, tg)
    target = int(model.test_index[5])
    w = evaluate.path_weight_table(model, method)
    scores = ops.path_scores(logits, ptr, nodes, w)
    assert not torch.equal(scores, logits)
    path, flat = evaluate.Evaluator(model, report=True, decode="path", decode_weights=method), evaluate.Evaluator(model, report=True)
    a, b = _run_class(path, logits, target), _run_class(flat, scores, target)
    assert _same(a, b) and float(a[0][8]) == 64
    a, b = _run_rows(path, logits, tg), _run_rows(flat, scores, tg)
    assert _same(a, b) and float(a[0][8]) == 64 + 60
    # and it is another decoding than the flat one on these logits
    plain = _run_rows(evaluate.Evaluator(model, report=True), logits, tg)
    assert not _same(a[2:], plain[2:])


# ---- 7. against the fp64 restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["equal", "increasing", "decreasing"])
def test_decoded_indices_equal_the_fp64_restatement_where_it_decides(tree, real, method):
    """top-20 over the test columns, top-1 over the train columns and the arg-max per level (oracle.tree_ref.level_argmax: it carries
    the filler rule) from S64.  A row is decidable when every gap that orders its outputs exceeds twice the sum of the two elements'
    bounds of test 2 (against "all the rest" the largest bound of the rest is taken: no smaller than the pair's own)."""
    model, ptr, nodes, x = tree
    w, s, s64, bound = real[method]
    n = len(model.nodes)
    ev = evaluate.Evaluator(model)
    lv, p1, pred = (t.cpu().numpy() for t in ops.eval_rows(s, ev.index, K))
    te, tr = model.test_index.cpu().numpy(), model.train_index.cpu().numpy()
    depth = model.hierarchy.depth
    s64n, bn = s64.numpy(), bound.numpy()

    def head_decided(v, b, k):
        """the order of the first k of v (descending) and their lead over the rest"""
        o = np.argsort(-v, kind="stable")
        ok = all(v[o[i]] - v[o[i + 1]] > 2 * (b[o[i]] + b[o[i + 1]]) for i in range(min(k, len(o)) - 1))
        if len(o) > k:
            ok = ok and v[o[k - 1]] - v[o[k]] > 2 * (b[o[k - 1]] + b[o[k:]].max())
        return ok

    level_cols = [np.nonzero(depth == l)[0] for l in range(ev.n_levels)]
    want_lv = np.stack([tree_ref.level_argmax(s64n, tr, c.tolist(), n) for c in level_cols], axis=1)
    decided = 0
    for r in range(64):
        ok = head_decided(s64n[r, te], bn[r, te], K) and head_decided(s64n[r, tr], bn[r, tr], 1)
        for c in level_cols:
            cols = np.array([t for t in tr if depth[t] == depth[c[0]]] if len(c) else [], dtype=np.int64)
            if len(cols):                                   # the level's train columns and the exact -1 of the filler
                v, b = np.append(s64n[r, cols], -1.0), np.append(bn[r, cols], 0.0)
                ok = ok and head_decided(v, b, 1)
        if not ok:
            continue
        decided += 1
        assert np.array_equal(pred[r], te[tree_ref.topk_desc(s64n[r, te], K)]), r
        assert int(p1[r, 0]) == int(tr[tree_ref.topk_desc(s64n[r, tr], 1)[0]]), r
        assert np.array_equal(lv[r], want_lv[r]), r
    print(f"[measured] {method}: {decided} of 64 rows decidable")
    assert decided >= 58                                    # a condition of the case, not a measurement: at least 90 % of the rows


# ---- 9. rejected arguments ---------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    """Real, amply sized device tensors: a missing check would give a wrong number, never a bad access."""
    _, ptr, nodes = _hand_paths()
    ptr, nodes, w = ptr.to(DEV), nodes.to(DEV), _random_convex_table(3).to(DEV)
    n = 70
    big = torch.zeros(16 * 100, device=DEV)
    out = torch.full((8, 100), 7.5, device=DEV)
    x = big[:800].view(8, 100)
    st = torch.cuda.current_stream().cuda_stream

    def call(xp, ld, sp, ld_out, rows):
        _lib.call("hgr_path_scores", xp, ld, sp, ld_out, n, ptr.data_ptr(), nodes.data_ptr(), w.data_ptr(), rows, st)

    cases = {"rows = 0": (x.data_ptr(), 100, out.data_ptr(), 100, 0), "ld < n_nodes": (x.data_ptr(), 69, out.data_ptr(), 100, 8),
             "ld_out < n_nodes": (x.data_ptr(), 100, out.data_ptr(), 69, 8), "scores is logits": (x.data_ptr(), 100, x.data_ptr(), 100, 8),
             "scores overlaps logits by one row": (x.data_ptr(), 100, big[700:].data_ptr(), 100, 8),
             "logits overlaps scores by one row": (big[700:].data_ptr(), 100, x.data_ptr(), 100, 8),
             "null logits": (0, 100, out.data_ptr(), 100, 8)}
    for name, args in cases.items():
        with pytest.raises(_lib.HgrError, match="hgr_path_scores"):
            call(*args)
    with pytest.raises(_lib.HgrError, match="hgr_path_scores"):
        ops.path_scores(x, ptr, nodes, w, out=x)
    torch.cuda.synchronize()
    assert bool((out == 7.5).all()) and bool((big == 0).all())                  # nothing was launched
    call(x.data_ptr(), 100, big[800:].data_ptr(), 100, 8)                          # adjacent ranges are fine
    call(x.data_ptr(), 100, out.data_ptr(), 100, 8)
    assert bool((out[:, :n] == 0).all()) and bool((out[:, n:] == 7.5).all())


# ---- 8. routes, 10. predict ---------------------------------------------------------------------------------------------------------------
SIZES = [5, 37, 64, 3]
B = 64


@pytest.fixture(scope="module")
def e2e(golden_dir, tmp_path_factory):
    """The small ViT tree model (the smallest fixture the fused evaluation route takes) with its classifier, and ragged one-class
    batches of images."""
    tmp = tmp_path_factory.mktemp("path_e2e")
    model, meta, cfg = _model("smallvit_n300", golden_dir, tmp)
    model.update_classifier()
    te = model.test_index.cpu().tolist()
    classes = [te[i] for i in np.random.default_rng(5).choice(len(te), len(SIZES), replace=False)]
    imgs = [synth.images(n, cfg["image_resolution"], 700 + i) for i, n in enumerate(SIZES)]
    return model, classes, imgs, tmp


def test_routes_of_the_evaluator_under_path_decoding(e2e):
    model, classes, imgs, _ = e2e
    assert evaluate.Evaluator(model).fused_ok()                                   # the fixture takes the fused route when decoding flat
    a, b = (evaluate.Evaluator(model, report=True, decode="path") for _ in range(2))
    c, d = (evaluate.Evaluator(model, report=True, decode="path") for _ in range(2))
    assert not a.fused_ok()
    for x, cl in zip(imgs, classes):
        xd = x.to(DEV)
        tg = torch.full((x.shape[0],), cl, dtype=torch.int64, device=DEV)
        tg[0] = -1                                                                # a padding row for the row scorers
        oa = a.add_images(xd, cl, want_outputs=True)
        ob = b.add_batch(model(xd), cl)
        assert all(torch.equal(p, q) for p, q in zip(oa, ob))
        c.add_images_rows(xd, tg)
        d.add_batch_rows(model(xd), tg)
    assert _same(_state(a, ()), _state(b, ())) and _same(_state(c, ()), _state(d, ()))
    assert float(a.acc[8]) == sum(SIZES) and float(c.acc[8]) == sum(SIZES) - len(SIZES)


def test_evaluate_test_with_decode_flags(e2e, capsys):
    model, classes, imgs, tmp = e2e

    def loader():
        return [{"img": x[None], "label": torch.full((1, x.shape[0]), c, dtype=torch.long)} for x, c in zip(imgs, classes)]

    def run(name, **kw):
        o = types.SimpleNamespace(**vars(model.opts))
        o.test_batch_size = B
        o.hier_report = None
        o.__dict__.update(kw)
        capsys.readouterr()
        out = evaluate.test(o, model, DEV, None, loader=loader(), log=False)
        return out, capsys.readouterr().out

    flat, flat_log = run("flat", decode="flat")
    assert flat == run("default")[0] and "decode:" not in flat_log
    # the composition of test 6 on the same batches
    ev = evaluate.Evaluator(model, report=True)
    ptr, nodes, _ = ev._ancestor_csr()
    w = evaluate.path_weight_table(model, "increasing")
    moved = False
    for x, c in zip(imgs, classes):
        logits = model(x.to(DEV))
        scores = ops.path_scores(logits, ptr, nodes, w)
        moved = moved or not torch.equal(ops.eval_rows(scores, ev.index, K)[2], ops.eval_rows(logits, ev.index, K)[2])
        ev.add_batch(scores, c)
    want = ev.summary()
    assert moved                                                                  # path decoding predicts something else here
    for pack in (False, True):
        out, log = run("self", decode="path", decode_weights="self", pack_batches=pack)
        assert out == flat and "decode: path (self)\n" in log and log.index("decode: path (self)") < log.index(out)
        path = tmp / f"rep_{int(pack)}.json"
        out, log = run("inc", decode="path", decode_weights="increasing", pack_batches=pack, hier_report=str(path))
        assert out == want and "decode: path (increasing)\n" in log
        rep = json.loads(path.read_text())
        assert rep["num_sample"] == sum(SIZES)
        assert rep == json.loads(json.dumps(evaluate.report_from_table(ev.report_table())))


def test_predict(e2e):
    model, classes, imgs, _ = e2e
    x = imgs[1]
    logits = model(x.to(DEV))
    ev = evaluate.Evaluator(model)
    ptr, nodes, _ = ev._ancestor_csr()
    out = evaluate.predict(model, x, want_scores=True)                            # images on the host are moved
    lv, p1, pred = ops.eval_rows(logits, ev.index, K)
    assert set(out) == {"topk", "top1", "levels", "scores"}
    assert torch.equal(out["topk"], pred) and torch.equal(out["top1"], p1.view(-1)) and torch.equal(out["levels"], lv)
    assert torch.equal(out["scores"], logits) and out["topk"].shape == (x.shape[0], K) and out["levels"].shape == (x.shape[0], ev.n_levels)
    assert out["levels"].dtype == out["topk"].dtype == out["top1"].dtype == torch.int32
    for method in ("increasing", "adaptive"):
        scores = ops.path_scores(logits, ptr, nodes, evaluate.path_weight_table(model, method))
        lv, p1, pred = ops.eval_rows(scores, ev.index, 5)
        out = evaluate.predict(model, x.to(DEV), k=5, decode="path", decode_weights=method, want_scores=True)
        assert torch.equal(out["topk"], pred) and torch.equal(out["top1"], p1.view(-1)) and torch.equal(out["levels"], lv)
        assert torch.equal(out["scores"], scores) and out["topk"].shape == (x.shape[0], 5)
    assert "scores" not in evaluate.predict(model, x, decode="path")
    with pytest.raises(ValueError):
        evaluate.predict(model, x, decode="nonsense")
