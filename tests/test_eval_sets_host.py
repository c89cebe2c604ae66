"""CPU: the host side of the candidate sets - sets_from_table and format_sets on a hand-written table, the bit layout and tie keys of
ops.SetIndex, the arguments the Python surface rejects before anything touches a device, --eval_sets parsing and resolution, and the
two entry points in include/hgr.h, in the ctypes table and in the built library."""
import json
import re
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    """The device="cpu" model of test_path_decode_host (copied: test modules do not import each other)."""
    from hgr_net_amd import synth
    from hgr_net_amd.clip.model import build_model
    from hgr_net_amd.hierarchy import build_hierarchy
    from hgr_net_amd.model import tree_model
    tmp = tmp_path_factory.mktemp("sets_host")
    edges = synth.make_dag(120, depth=8, seed=3, multi_parent=0.05)
    g = tmp / "g.json"
    g.write_text(json.dumps(edges))
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], 40, 50, 13)
    o = types.SimpleNamespace(device="cpu", folder=str(tmp), exp_name="HGR", weights="adaptive", out_ratio=0.25, in_ratio=0.5,
                              from_epoch=-1, graph_path=str(g), arch="x", fetch=False, load=False, load_path="none", scale=1.0,
                              num_compare=16, k=1, sample_strategy="topk", weighting="both")
    return tree_model(o, splits["all"], splits["rest"], node_tokens=synth.make_tokens(120, 11, 512),
                      clip_model=build_model(synth.clip_state_dict("tiny-vit", 0)))


def test_sets_from_table_on_a_hand_written_table():
    from hgr_net_amd import evaluate, ops
    assert ops.SETS_COL_NAMES == ("rows", "hit@1", "hit@2", "hit@5", "hit@10", "hit@20", "anc_hit", "point", "edge")
    assert ops.SETS_COLS == 9 and ops.SETS_MAXS == 16
    t = torch.zeros(3, ops.REPORT_MAXL + 1, ops.SETS_COLS, dtype=torch.int64)
    # set "a": 4 rows of path length 1 (edge = the single match: 3) and 10 rows of path length 3 (edge over 2 pairs, point over 3 nodes)
    t[0, 1] = torch.tensor([4, 1, 2, 3, 4, 4, 1, 3, 3])
    t[0, 3] = torch.tensor([10, 2, 3, 5, 6, 9, 4, 12, 5])
    # set "b": rows of path length 32 only; set "c": no rows
    t[1, 32] = torch.tensor([2, 0, 0, 1, 1, 2, 0, 32, 31])
    rep = evaluate.sets_from_table(t, ("a", "b", "c"), (7, 40, 0))
    assert list(rep) == ["sets"] and [e["name"] for e in rep["sets"]] == ["a", "b", "c"]
    a, b, c = rep["sets"]
    assert a["classes"] == 7 and a["num_sample"] == 14 and [a[f"hits@{k}"] for k in (1, 2, 5, 10, 20)] == [3, 5, 8, 10, 13]
    assert a["acc@1"] == 3 / 14 * 100.0 and a["acc@20"] == 13 / 14 * 100.0
    assert a["hits_all"] == 5 and a["hit_ratio"] == 5 / 14 * 100.0
    assert a["path_all"] == 3 + 5 / 2 and a["path_ratio"] == 5.5 / 14 * 100.0            # L == 1: the match itself, no division by L - 1
    assert a["point_all"] == 3 + 12 / 3 and a["point_ratio"] == 7.0 / 14 * 100.0
    assert [e["depth"] for e in a["by_depth"]] == [0, 2]
    d0, d2 = a["by_depth"]
    assert d0 == {"depth": 0, "rows": 4, "hits@1": 1, "acc@1": 25.0, "hits@2": 2, "acc@2": 50.0, "hits@5": 3, "acc@5": 75.0, "hits@10": 4,
                  "acc@10": 100.0, "hits@20": 4, "acc@20": 100.0, "hit_ratio": 25.0, "path_ratio": 75.0, "point_ratio": 75.0}
    assert d2["path_ratio"] == 5 / 2 / 10 * 100.0 and d2["point_ratio"] == 12 / 3 / 10 * 100.0 and d2["hit_ratio"] == 40.0
    assert b["num_sample"] == 2 and b["path_all"] == 1.0 and b["point_all"] == 1.0 and b["by_depth"][0]["depth"] == 31
    assert c["num_sample"] == 0 and c["classes"] == 0 and c["by_depth"] == [] and c["hits@1"] == 0
    assert all(c[k] is None for k in ("acc@1", "acc@2", "acc@5", "acc@10", "acc@20", "hit_ratio", "path_ratio", "point_ratio"))
    assert json.loads(json.dumps(rep)) == rep                                            # a JSON round trip
    lines = evaluate.format_sets(rep).split("\n")
    assert len(lines) == 3
    # behind the head: exactly the text Evaluator.summary() makes from the same counters
    assert lines[0] == "set a (7 classes, 14 images): " + evaluate.metric_text({k: a[k] for k in evaluate.COUNTERS})
    assert lines[0].endswith("Top@1(%):21.43, Top@2(%):35.71, Top@5(%):57.14, Top@10(%):71.43, Top@20(%):92.86. hit_ratio(%):35.71 "
                             "path_ratio(%):39.29 point_ratio(%):50.00")
    assert lines[1].startswith("set b (40 classes, 2 images): Top@1(%):0.00") and lines[2] == "set c (0 classes, 0 images): no images"
    with pytest.raises(AssertionError):
        evaluate.sets_from_table(t, ("a", "b"), (7, 40))                                 # the table has three sets
    with pytest.raises(AssertionError):
        evaluate.sets_from_table(t.to(torch.int32), ("a", "b", "c"), (7, 40, 0))


def test_summary_text_is_metric_text(cpu_model):
    """Evaluator.summary() and the set lines share one formatter: the reference's line (main.py:205-214) on known counters."""
    from hgr_net_amd import evaluate
    c = dict(zip(evaluate.COUNTERS, [1.0, 2.0, 6.0, 9.0, 11.0, 2.0, 1.2857142857142856, 5.742857142857143, 24.0]))
    want = ("Top@1(%):4.17, Top@2(%):8.33, Top@5(%):25.00, Top@10(%):37.50, Top@20(%):45.83. hit_ratio(%):8.33 path_ratio(%):5.36 "
            "point_ratio(%):23.93")                                                      # tests/golden/tree_tinyvit_n90.json "metric"
    assert evaluate.metric_text(c) == want
    ev = evaluate.Evaluator(cpu_model)
    ev.acc.copy_(torch.tensor([c[k] for k in evaluate.COUNTERS], dtype=torch.float64))
    assert ev.summary() == "\n" + want


def _index12():
    from hgr_net_amd import ops
    depth = torch.tensor([0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3], dtype=torch.int32)
    train = torch.arange(12, dtype=torch.int32)
    test = torch.tensor([9, 4, 11, 6], dtype=torch.int32)                               # test positions 0..3
    return ops.EvalIndex(depth, train, test, 4)


def test_set_index_bit_layout_and_tie_keys():
    from hgr_net_amd import ops
    ix = _index12()
    sets = {"test": [9, 4, 11, 6], "two": [4, 5], "none": [], "all": list(range(12)), "tensor": torch.tensor([11, 0])}
    si = ops.SetIndex(ix, sets)
    assert si.names == ("test", "two", "none", "all", "tensor") and si.sizes == (4, 2, 0, 12, 2) and si.n_sets == 5 and si.n_nodes == 12
    assert si.member.dtype == torch.int32 and si.tie_key.dtype == torch.int32
    want = [0] * 12
    for s, ids in enumerate(([9, 4, 11, 6], [4, 5], [], range(12), [11, 0])):
        for c in ids:
            want[c] |= 1 << s
    assert si.member.tolist() == want and want[4] == 0b01011 and want[11] == 0b11001 and want[1] == 0b01000
    # the test classes keep their test position; the other nodes follow in node order from n_test = 4 upward
    assert si.tie_key.tolist() == [4, 5, 6, 7, 1, 8, 3, 9, 10, 0, 11, 2]
    assert sorted(si.tie_key.tolist()) == list(range(12))                               # distinct: a total order in every set
    full = ops.SetIndex(ix, {str(i): [i % 12] for i in range(16)})                      # 16 sets: bit 15 is the last
    assert full.n_sets == 16 and full.member[3].item() == (1 << 3) | (1 << 15)
    # without a test subset the keys are the node order
    plain = ops.EvalIndex(torch.zeros(5, dtype=torch.int32), torch.arange(5, dtype=torch.int32), None, 1)
    assert ops.SetIndex(plain, {"a": [3]}).tie_key.tolist() == [0, 1, 2, 3, 4]


BAD_SETS = {"empty mapping": {}, "seventeen sets": {str(i): [i] for i in range(17)}, "duplicate id": {"a": [1, 2], "b": [3, 5, 3]},
            "negative id": {"a": [-1]}, "id = n_nodes": {"a": [0], "b": [10 ** 6]}, "no mapping": [1, 2, 3], "no ids": {"a": 5},
            "no integers": {"a": ["n01"]}}


@pytest.mark.parametrize("name", list(BAD_SETS))
def test_rejected_sets(cpu_model, name):
    from hgr_net_amd import evaluate, ops
    with pytest.raises(ValueError):
        ops.check_sets(BAD_SETS[name], 12)
    with pytest.raises(ValueError):
        ops.SetIndex(_index12(), BAD_SETS[name])
    with pytest.raises(ValueError):
        evaluate.Evaluator(cpu_model, sets=BAD_SETS[name])
    if name == "id = n_nodes":
        with pytest.raises(ValueError):
            evaluate.Evaluator(cpu_model, sets={"a": [len(cpu_model.nodes)]})
        evaluate.Evaluator(cpu_model, sets={"a": [len(cpu_model.nodes) - 1]})


def test_evaluator_sets_state(cpu_model):
    from hgr_net_amd import evaluate, ops
    ev = evaluate.Evaluator(cpu_model)                                      # the default: no set state at all
    assert ev.sets is None and ev.sets_tab is None and ev._sets_buf is None
    te = cpu_model.test_index.tolist()
    ev = evaluate.Evaluator(cpu_model, sets={"rest": te, "half": te[::2]})
    assert not ev.fused_ok() and ev._sets_buf is None and ev.sets.names == ("rest", "half") and ev.sets.sizes == (len(te), len(te[::2]))
    assert ev.sets_tab.dtype == torch.int64 and tuple(ev.sets_tab.shape) == (2, ops.REPORT_MAXL + 1, ops.SETS_COLS)
    assert int(ev.sets_tab.abs().sum()) == 0
    assert ev.sets.tie_key[te].tolist() == list(range(len(te)))             # the model's test order
    rep = ev.sets_dict()                                                    # an empty table reads as no images everywhere
    assert [e["num_sample"] for e in rep["sets"]] == [0, 0] and [e["classes"] for e in rep["sets"]] == [len(te), len(te[::2])]
    with pytest.raises(AssertionError):
        evaluate.Evaluator(cpu_model).sets_table()


def test_eval_sets_parsing_and_resolution():
    from hgr_net_amd import evaluate
    from hgr_net_amd.main import build_parser
    p = build_parser()
    o = p.parse_args([])
    assert o.eval_sets is None and o.eval_sets_file is None and o.eval_sets_report is None
    o = p.parse_args(["--eval_sets", "hop2,hop3,hop3+train", "--eval_sets_file", "h.json", "--eval_sets_report", "r.json"])
    assert o.eval_sets == "hop2,hop3,hop3+train" and o.eval_sets_file == "h.json" and o.eval_sets_report == "r.json"
    spec = evaluate.parse_eval_sets(o.eval_sets)
    assert spec == (("hop2", ("hop2",)), ("hop3", ("hop3",)), ("hop3+train", ("hop3", "train")))
    assert evaluate.parse_eval_sets(None) is None and evaluate.parse_eval_sets(spec) == spec
    for bad in ("", "a,,b", "a+", "+a", "a,a", ",".join(f"s{i}" for i in range(17))):
        with pytest.raises(ValueError):
            evaluate.parse_eval_sets(bad)
    nodes = ["n0", "n1", "n2", "n3", "n4", "n5"]
    splits = {"train": ["n1", "n0"], "rest": ["n5", "n3"]}
    extra = {"hop2": ["n3"], "hop3": ["n5", "n3", "n4"]}
    got = evaluate.resolve_eval_sets(spec, splits, nodes, extra)
    assert list(got.items()) == [("hop2", [3]), ("hop3", [5, 3, 4]), ("hop3+train", [5, 3, 4, 1, 0])]
    # a union lists a shared wnid once, in the order of its keys
    assert evaluate.resolve_eval_sets(evaluate.parse_eval_sets("rest+hop3"), splits, nodes, extra) == {"rest+hop3": [5, 3, 4]}
    with pytest.raises(ValueError, match="'hop9'"):
        evaluate.resolve_eval_sets(evaluate.parse_eval_sets("hop2,hop9"), splits, nodes, extra)
    with pytest.raises(ValueError, match="'hop2'"):
        evaluate.resolve_eval_sets(evaluate.parse_eval_sets("hop2"), splits, nodes)         # without the second file
    with pytest.raises(ValueError, match="'rest'"):
        evaluate.resolve_eval_sets(spec, splits, nodes, dict(extra, rest=["n2"]))           # a key present in both files
    with pytest.raises(ValueError, match="'n77'"):
        evaluate.resolve_eval_sets(spec, splits, nodes, dict(extra, hop3=["n5", "n77"]))    # a wnid absent from the hierarchy


def test_header_ctypes_table_and_constants_agree():
    from hgr_net_amd import _lib, ops
    header = (ROOT / "include" / "hgr.h").read_text()
    for name, n_args in (("hgr_set_ranks", 11), ("hgr_set_counters_rows", 13)):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, f"include/hgr.h declares {name}"
        args = [a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(args) == n_args
        assert hasattr(_lib.load(), name)                                   # the built library exports it (no device needed to load)
    assert int(re.search(r"#define\s+HGR_SETS_MAXS\s+(\d+)", header).group(1)) == ops.SETS_MAXS == 16
    assert int(re.search(r"#define\s+HGR_SETS_COLS\s+(\d+)", header).group(1)) == ops.SETS_COLS == len(ops.SETS_COL_NAMES) == 9
    assert ops.SETS_COL_NAMES == ops.REPORT_DEPTH_COLS[:9]                  # the report's depth columns without "chain"


def test_set_ops_on_cpu_tensors_raise_hgr_error():
    from hgr_net_amd import _lib, ops
    si = ops.SetIndex(_index12(), {"a": [1, 2]})
    with pytest.raises(_lib.HgrError):
        ops.set_ranks(torch.zeros(2, 12), si, torch.zeros(2, dtype=torch.int64))
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(_lib.HgrError):
        ops.set_counters_rows(z(2, 1), z(2, 1), torch.zeros(2, dtype=torch.int64), z(2, 4), torch.tensor([0, 1, 3], dtype=torch.int32),
                              z(3), z(3), torch.zeros(1, ops.REPORT_MAXL + 1, ops.SETS_COLS, dtype=torch.int64))
