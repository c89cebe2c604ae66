"""CPU: the host side of the DGP scoring (hgr_net_amd.baseline.dgp_eval / evaluate_dgp) against the reference's own
`test_on_subset` run recorded in tests/golden/dgp_eval_small.npz (tools/make_golden_dgp_eval.py): the numpy twins of the kernels, the
ordered-list tree, the prediction and feature files, the options and the printed lines."""
import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hgr_net_amd.baseline import dgp_eval, evaluate_dgp

INT_COLS, SUM_COLS = [0, 1, 2, 3, 4, 5, 8], [6, 7]      # hits@1,2,5,10,20, hits_all, tot | path_all, point_all


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN / "dgp_eval_small.npz")
    fx = {k: z[k] for k in z.files}
    fx["edges"] = [list(map(str, e)) for e in fx["edges"]]
    fx["nodes"] = [str(w) for w in fx["nodes"]]
    fx["n_seen"] = int(fx["n_seen"])
    fx["starts"] = np.concatenate([[0], np.cumsum(fx["feat_count"])]).astype(int)
    fx["tree"] = dgp_eval.build_list_tree(fx["edges"], fx["nodes"])
    return fx


def class_rows(fx, i):
    return slice(fx["starts"][i], fx["starts"][i + 1])


def check_against_reference(acc, ref):
    """acc / ref [classes, 9]: integers equal, the path / point sums within 1e-9."""
    assert np.array_equal(acc[:, INT_COLS], ref[:, INT_COLS])
    assert np.abs(acc[:, SUM_COLS] - ref[:, SUM_COLS]).max() <= 1e-9


def test_fixture_is_what_the_maker_promises():
    fx = fixture()
    n, ns = len(fx["nodes"]), fx["n_seen"]
    assert (n, ns, fx["pred"].shape) == (64, 16, (64, 65)) and fx["table"].dtype == np.float16
    assert fx["feat_count"].min() == 1 and fx["feat_count"].max() <= 9 and len(fx["feat_count"]) == n - ns
    assert fx["tree"].n_levels - 1 >= 9
    exact = np.concatenate([fx["feat"].astype(np.float64), np.ones((len(fx["feat"]), 1))], 1) @ fx["pred"].astype(np.float16).astype(np.float64).T
    assert np.array_equal(fx["table"].astype(np.float64), exact)       # no accumulation order can change this table
    assert int((fx["ref"][0, :, :5] != fx["ref"][1, :, :5]).any(1).sum()) >= 10


@pytest.mark.parametrize("consider_trains", [False, True])
def test_host_twins_reproduce_the_reference(consider_trains):
    fx = fixture()
    h = dgp_eval.HostEvaluator(fx["tree"], fx["n_seen"], consider_trains)
    for i in range(len(fx["feat_count"])):
        h.add(fx["table"][class_rows(fx, i)], fx["n_seen"] + i)
    ref = fx["ref"][int(consider_trains)]
    check_against_reference(h.acc[fx["n_seen"]:-1], ref)
    res = h.result()
    assert res["tot"] == int(ref[:, 8].sum()) and res["hits"] == ref[:, :5].sum(0).tolist()
    assert abs(res["path"] - ref[:, 6].sum()) <= 1e-9 and abs(res["point"] - ref[:, 7].sum()) <= 1e-9 and res["to"] == ref[:, 5].sum()
    w = fx["nodes"][fx["n_seen"] + 3]
    assert res["results"][w] == (ref[3, :5] / ref[3, 8]).tolist()
    # the packed route counts the same rows in one go
    p = dgp_eval.HostEvaluator(fx["tree"], fx["n_seen"], consider_trains)
    targets = np.repeat(np.arange(fx["n_seen"], len(fx["nodes"])), fx["feat_count"])
    p.add_rows(fx["table"], targets)
    assert np.array_equal(p.acc[-1, INT_COLS], ref[:, INT_COLS].sum(0)) and np.abs(p.acc[-1, SUM_COLS] - ref[:, SUM_COLS].sum(0)).max() <= 1e-9


def test_ties_count_against_the_target_not_topk_membership():
    """rank counts every column >= the target's score: with j other columns at the target's value the rank is j + 1 + #greater,
    where top-k membership (lowest index first) would put a low-index target at #greater + 1."""
    t = np.zeros((1, 8), np.float16)
    t[0] = [3, 1, 1, 1, 5, 0, 1, -2]
    depth = np.zeros(8, np.int32)
    rank, top1, lv = dgp_eval.score_rows_host(t, depth, 1, target=1)
    assert rank.tolist() == [6] and top1.tolist() == [4] and lv.tolist() == [[4]]
    rank, _, _ = dgp_eval.score_rows_host(t, depth, 1, n_masked=5, mask_value=1.0, target=6)      # masked columns tie with a stored 1
    assert rank.tolist() == [6]
    rank, top1, _ = dgp_eval.score_rows_host(t, depth, 1, n_masked=8, target=7)                  # everything masked: all tie, column 0 leads
    assert rank.tolist() == [8] and top1.tolist() == [0]


def test_score_rows_host_edge_values():
    f = np.float16(dgp_eval.FILL)
    assert float(f) == 2.0 ** -23
    t = np.array([[-5, -3, 0.0, -0.0, float(f), -1, -np.inf, np.inf]], np.float16)
    depth = np.array([0, 1, 1, 2, 2, 3, 3, 5], np.int32)
    rank, top1, lv = dgp_eval.score_rows_host(t, depth, 6, n_masked=1, target=0)
    # v = [2^-23, -3, 0, -0, 2^-23, -1, -inf, inf]: the fill ties with the stored 2^-23, -0 with +0
    assert rank.tolist() == [3] and top1.tolist() == [7]
    # level 0: the masked column; 1: +0 at column 2; 2: 2^-23 at 4 over -0; 3: -1 at column 5 ties with the filler at column 0 -> 0;
    # 4: empty -> 0; 5: inf
    assert lv.tolist() == [[0, 2, 4, 0, 0, 7]]
    rank, _, _ = dgp_eval.score_rows_host(t, depth, 6, n_masked=1, target=3)
    assert rank.tolist() == [5]                                        # +0, -0, both 2^-23, inf
    below = np.array([[-2, -3, -4, 0.5]], np.float32)
    _, _, lv = dgp_eval.score_rows_host(below, np.array([1, 0, 0, 1], np.int32), 2, target=0)
    assert lv.tolist() == [[0, 3]]                                     # level 0 all below -1: the first column outside it
    with pytest.raises(ValueError):
        dgp_eval.score_rows_host(t, depth, 6, target=8)
    with pytest.raises(ValueError):
        dgp_eval.score_rows_host(t.astype(np.float64), depth, 6)


def test_pick_vectors_and_pred_file(tmp_path):
    pred = {"wnids": ["a", "b", "c", "b"], "pred": torch.arange(12, dtype=torch.float32).reshape(4, 3)}
    v = dgp_eval.pick_vectors(pred, ["c", "zz", "b", "a"])
    assert v.tolist() == [[6, 7, 8], [0, 0, 0], [9, 10, 11], [0, 1, 2]]         # missing: zeros; listed twice: the last, like dict(zip())
    torch.save(pred, tmp_path / "epoch_1.pred")
    back = dgp_eval.load_pred(tmp_path / "epoch_1.pred")
    assert back["wnids"] == pred["wnids"] and torch.equal(back["pred"], pred["pred"])
    torch.save({"wnids": ["a"]}, tmp_path / "bad.pred")
    with pytest.raises(ValueError):
        dgp_eval.load_pred(tmp_path / "bad.pred")


def test_list_tree_matches_the_fixture_and_names_a_missing_ancestor():
    fx = fixture()
    tree = fx["tree"]
    ptr, flat = fx["c2p_ptr"], fx["c2p_flat"]
    assert tree.c2p == [flat[ptr[i]:ptr[i + 1]].tolist() for i in range(len(tree.nodes))]
    assert np.array_equal(tree.depth, np.diff(ptr)) and tree.n_levels == int(np.diff(ptr).max()) + 1
    assert all(tree.d2n[d] == np.nonzero(tree.depth == d)[0].tolist() for d in tree.d2n)
    deep = int(np.argmax(tree.depth))
    gone = tree.nodes[tree.c2p[deep][0]]
    with pytest.raises(ValueError, match=f"ancestor '{gone}'"):
        dgp_eval.build_list_tree(fx["edges"], [w for w in tree.nodes if w != gone])
    with pytest.raises(ValueError, match="not in the graph"):
        dgp_eval.build_list_tree(fx["edges"], tree.nodes + ["n99999999"])
    # the 21K-P protocol: a test set closed under ancestors is its own node list
    closed = [tree.nodes[i] for i in sorted(set(tree.path(deep)))]
    sub = dgp_eval.build_list_tree(fx["edges"], closed)
    assert sub.n_levels == len(closed) and sorted(sub.depth.tolist()) == list(range(len(closed)))


def test_feature_file_and_keep_ratio(tmp_path):
    a, b = np.ones((3, 4), np.float32), np.zeros((1, 4), np.float16)
    np.savez(tmp_path / "f.npz", n1=a, n2=b)
    f = dgp_eval.load_features(tmp_path / "f.npz")
    assert sorted(f) == ["n1", "n2"] and f["n1"].shape == (3, 4) and f["n2"].dtype == np.float16
    np.savez(tmp_path / "g.npz", n1=a, n2=np.zeros((1, 5), np.float32))
    with pytest.raises(ValueError, match="widths"):
        dgp_eval.load_features(tmp_path / "g.npz")
    np.savez(tmp_path / "h.npz", n1=np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        dgp_eval.load_features(tmp_path / "h.npz")
    assert [dgp_eval.keep_rows(9, r) for r in (1.0, 0.5, 0.1, 1 / 3)] == [9, 5, 1, 3]
    with pytest.raises(ValueError):
        dgp_eval.keep_rows(9, 0.0)


def test_options():
    a = evaluate_dgp.parse_args([])
    assert (a.pred, a.test_set, a.train_set, a.output, a.keep_ratio, a.consider_trains, a.batch_size, a.dtype, a.synthetic, a.features) == \
        ("gcn_dense_att/zsl/epoch_3000.pred", "rest", "train", None, 1.0, False, 256, "f16", None, None)
    assert a.graph_path == "data/process_results/graph_edges_cls.json" and a.split_path == "data/process_results/splits_for_tree.json"
    a = evaluate_dgp.parse_args("--pred p --test-set hop2 --train-set= --output o.json --keep-ratio 0.25 --consider-trains --graph_path g.json "
                                "--split_path s.json --features f.npz --batch-size 64 --dtype fp32 --synthetic 200".split())
    assert (a.pred, a.test_set, a.train_set, a.output, a.keep_ratio, a.consider_trains, a.graph_path, a.split_path, a.features, a.batch_size,
            a.dtype, a.synthetic) == ("p", "hop2", "", "o.json", 0.25, True, "g.json", "s.json", "f.npz", 64, "fp32", 200)
    for bad in (["--batch-size", "0"], ["--keep-ratio", "0"], ["--dtype", "bf16"], ["--cnn", "x"], ["--test-train"], ["--gpu", "1"]):
        with pytest.raises(SystemExit):
            evaluate_dgp.parse_args(bad)
    from hgr_net_amd.baseline import train_dgp
    t = train_dgp.parse_args([])
    assert t.eval_after is False and t.test_set == "rest" and t.batch_size == 256 and t.max_epoch == 3000
    t = train_dgp.parse_args(["--eval-after", "--consider-trains", "--features", "f.npz", "--synthetic", "300"])
    assert t.eval_after and t.consider_trains and t.features == "f.npz" and t.synthetic == 300


def test_printed_lines_have_the_reference_formats():
    hits, s_hits = [1, 2, 2, 3, 3], [10.0, 12.0, 15.0, 20.0, 25.0]
    line = dgp_eval.class_line(3, 48, "n00000007", hits, 3, s_hits, 40, 8.0, 5.5, 21.25)
    assert line == "3/48, n00000007: 33%(25.00%) 67%(30.00%) 67%(37.50%) 100%(50.00%) 100%(62.50%) To:20.00% Path:13.75% Point:53.12% x3(40)"
    assert dgp_eval.summary_line(s_hits, 40) == "summary: 25.00% 30.00% 37.50% 50.00% 62.50% total 40"
    fx = fixture()
    h = dgp_eval.HostEvaluator(fx["tree"], fx["n_seen"])
    for i in range(len(fx["feat_count"])):
        h.add(fx["table"][class_rows(fx, i)], fx["n_seen"] + i)
    lines = dgp_eval.report_lines(h.result(), fx["nodes"][fx["n_seen"]:])
    ref = fx["ref"][0]
    assert len(lines) == len(ref) + 1 and lines[-1] == dgp_eval.summary_line(ref[:, :5].sum(0), int(ref[:, 8].sum()))
    assert lines[0].startswith("1/48, {}: ".format(fx["nodes"][fx["n_seen"]])) and lines[0].endswith("x{0}({0})".format(int(ref[0, 8])))


def test_synthetic_material_is_closed_and_deterministic():
    edges, splits, pred, feats = evaluate_dgp.synthetic_material(200, 0, dim=32)
    nodes = splits["train"] + splits["rest"]
    tree = dgp_eval.build_list_tree(edges, nodes)                      # every path lies inside the list
    assert len(tree.nodes) == len(pred["wnids"]) and pred["pred"].shape[1] == 33
    assert set(feats) == set(splits["rest"]) and all(1 <= len(v) <= 9 and v.shape[1] == 32 for v in feats.values())
    again = evaluate_dgp.synthetic_material(200, 0, dim=32)
    assert json.dumps(again[1]) == json.dumps(splits) and all(np.array_equal(again[3][w], feats[w]) for w in feats)
