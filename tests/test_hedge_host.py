"""CPU: the host side of hedged predictions - hedge_from_table on a hand-written table, the threshold to fixed-point conversion, the
hedge arguments the Python surface rejects before anything touches a device, the command-line flags, and the two entry points in
include/hgr.h, in the ctypes table and in the built library."""
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
    tmp = tmp_path_factory.mktemp("hedge_host")
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


def test_hedge_from_table_on_a_hand_written_table():
    from hgr_net_amd import evaluate, ops
    assert ops.HEDGE_COL_NAMES == ("rows", "abstain", "exact", "ancestor", "below", "wrong", "sum_lpick", "sum_common", "sum_lt")
    t = torch.zeros(3, ops.HEDGE_COLS, dtype=torch.int64)
    # theta 0.25: 10 rows = 2 abstained, 3 exact, 1 ancestor, 1 below, 3 wrong; picks of 2 nodes except the abstentions
    t[0, :9] = torch.tensor([10, 2, 3, 1, 1, 3, 16, 12, 40])
    t[0, ops.HEDGE_COL_HIST + 0], t[0, ops.HEDGE_COL_HIST + 2] = 2, 8
    # theta 0.5: every row abstained - nothing picked, no precision
    t[1, :9] = torch.tensor([10, 10, 0, 0, 0, 0, 0, 0, 40])
    t[1, ops.HEDGE_COL_HIST + 0] = 10
    # theta 1.0: no rows at all
    rep = evaluate.hedge_from_table(t, (0.25, 0.5, 1.0), temperature=100.0)
    assert rep["thresholds"] == [0.25, 0.5, 1.0] and rep["temperature"] == 100.0 and len(rep["by_threshold"]) == 3
    a, b, c = rep["by_threshold"]
    assert a == {"threshold": 0.25, "rows": 10, "abstain": 2, "abstain_pct": 20.0, "exact": 3, "exact_pct": 30.0, "ancestor": 1,
                 "ancestor_pct": 10.0, "below": 1, "below_pct": 10.0, "wrong": 3, "wrong_pct": 30.0, "correct": 6, "correct_pct": 60.0,
                 "mean_pick_depth": 1.6, "h_precision": 0.75, "h_recall": 0.3, "pick_depth_histogram": {"0": 2, "2": 8}}
    assert b["abstain_pct"] == 100.0 and b["correct"] == 10 and b["mean_pick_depth"] == 0.0 and b["h_precision"] is None
    assert b["h_recall"] == 0.0 and b["pick_depth_histogram"] == {"0": 10}
    assert c["rows"] == 0 and c["correct"] == 0 and c["pick_depth_histogram"] == {}
    assert all(c[k] is None for k in ("abstain_pct", "exact_pct", "ancestor_pct", "below_pct", "wrong_pct", "correct_pct", "mean_pick_depth",
                                      "h_precision", "h_recall"))
    assert json.loads(json.dumps(rep)) == rep and "temperature" not in evaluate.hedge_from_table(t, (0.25, 0.5, 1.0))
    lines = evaluate.format_hedge(rep).split("\n")
    assert len(lines) == 4 and all(l.startswith("hedge ") for l in lines)                     # a header and one line per threshold
    assert "0.250" in lines[1] and "60.00" in lines[1] and "0.750" in lines[1] and "0.500" in lines[2] and "1.000" in lines[3]
    with pytest.raises(AssertionError):
        evaluate.hedge_from_table(t, (0.25, 0.5))                                             # the table has three rows
    with pytest.raises(AssertionError):
        evaluate.hedge_from_table(t.to(torch.int32), (0.25, 0.5, 1.0))


def test_threshold_to_fixed_point():
    from hgr_net_amd import ops
    assert ops.HEDGE_SCALE == 2 ** 30
    assert ops.hedge_thresholds([2.0 ** -30, 0.5, 1.0]) == [1, 2 ** 29, 2 ** 30]
    assert ops.hedge_thresholds((2.0 ** -31,)) == [1] and ops.hedge_thresholds((2.0 ** -30 + 2.0 ** -50,)) == [2]      # ceil, in double
    assert ops.hedge_thresholds([0.1]) == [107374183]                                        # 0.1 * 2^30 = 107374182.4
    assert ops.hedge_thresholds([0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 1]) [-1] == 2 ** 30


BAD = {"empty": (), "nine values": tuple(0.1 * i for i in range(1, 10)), "not increasing": (0.5, 0.25), "repeated": (0.5, 0.5),
       "zero": (0.0, 0.5), "negative": (-0.1,), "above one": (0.5, 1.5), "nan": (float("nan"),), "no sequence": 0.5}


@pytest.mark.parametrize("name", list(BAD))
def test_rejected_hedge_arguments(cpu_model, name):
    from hgr_net_amd import evaluate, ops
    with pytest.raises(ValueError):
        ops.hedge_thresholds(BAD[name])
    with pytest.raises(ValueError):
        evaluate.Evaluator(cpu_model, hedge=BAD[name])


def test_evaluator_hedge_state(cpu_model):
    from hgr_net_amd import evaluate, ops
    ev = evaluate.Evaluator(cpu_model)                                      # the default: no hedge state at all
    assert ev.hedge is None and ev.hedge_tab is None and ev._hedge_thr is None and ev._hedge_pick is None and ev.hedge_temperature is None
    ev = evaluate.Evaluator(cpu_model, hedge=[0.25, 0.5, 1.0])
    assert ev.hedge == (0.25, 0.5, 1.0) and not ev.fused_ok() and ev._hedge_pick is None
    assert ev._hedge_thr.dtype == torch.int32 and ev._hedge_thr.tolist() == [2 ** 28, 2 ** 29, 2 ** 30]
    assert ev.hedge_tab.dtype == torch.int64 and tuple(ev.hedge_tab.shape) == (3, ops.HEDGE_COLS) and int(ev.hedge_tab.abs().sum()) == 0
    assert ev.hedge_temperature == float(cpu_model.clip_model.logit_scale.detach().exp())              # the model's, read once
    assert evaluate.Evaluator(cpu_model, hedge=[0.5], hedge_temperature=7).hedge_temperature == 7.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            evaluate.Evaluator(cpu_model, hedge=[0.5], hedge_temperature=bad)
    with pytest.raises(AssertionError):
        evaluate.Evaluator(cpu_model).hedge_table()
    rep = ev.hedge_dict()                                                   # an empty table reads as rows = 0 everywhere
    assert [e["rows"] for e in rep["by_threshold"]] == [0, 0, 0] and rep["thresholds"] == [0.25, 0.5, 1.0]


def test_parser_flags():
    from hgr_net_amd.main import build_parser
    p = build_parser()
    o = p.parse_args([])
    assert o.hedge is None and o.hedge_temperature is None and o.hedge_report is None
    o = p.parse_args(["--hedge", "0.25,0.5,0.9", "--hedge_temperature", "50", "--hedge_report", "h.json"])
    assert o.hedge == (0.25, 0.5, 0.9) and o.hedge_temperature == 50.0 and o.hedge_report == "h.json"
    assert p.parse_args(["--hedge", "1"]).hedge == (1.0,)
    for bad in (["--hedge", ""], ["--hedge", "0.5,0.25"], ["--hedge", "0,0.5"], ["--hedge", "0.5,1.5"], ["--hedge", "a,b"], ["--hedge"],
                ["--hedge", ",".join(str(0.1 * i) for i in range(1, 10))], ["--hedge_temperature", "hot"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_header_ctypes_table_and_constants_agree():
    from hgr_net_amd import _lib, ops
    header = (ROOT / "include" / "hgr.h").read_text()
    for name, n_args in (("hgr_subtree_hedge", 15), ("hgr_hedge_counters_rows", 9)):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, f"include/hgr.h declares {name}"
        args = [a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(args) == n_args
        assert hasattr(_lib.load(), name)                                   # the built library exports it (no device needed to load)
    assert int(re.search(r"#define\s+HGR_HEDGE_MAXT\s+(\d+)", header).group(1)) == ops.HEDGE_MAXT == 8
    assert int(re.search(r"#define\s+HGR_HEDGE_MAXN\s+(\d+)", header).group(1)) == ops.HEDGE_MAXN == 36864
    assert ops.HEDGE_MAXN * 4 == 147456 and ops.HEDGE_MAXN <= 0xFFFF        # the mass row in LDS; the id field of the pick key
    cols = dict((k, int(v)) for k, v in re.findall(r"HGR_HEDGE_COL_([A-Z_]+)\s*=\s*(\d+)", header))
    assert [cols[n.upper()] for n in ops.HEDGE_COL_NAMES] == list(range(9)) and cols["HIST"] == ops.HEDGE_COL_HIST == 9
    assert re.search(r"#define\s+HGR_HEDGE_COLS\s+\(HGR_HEDGE_COL_HIST \+ HGR_REPORT_MAXL \+ 1\)", header)
    assert ops.HEDGE_COLS == 9 + ops.REPORT_MAXL + 1 == 42
    assert _lib.ABI_VERSION == 5


def test_hedge_ops_on_cpu_tensors_raise_hgr_error():
    from hgr_net_amd import _lib, ops
    ptr = torch.tensor([0, 1, 3], dtype=torch.int32)
    nodes = torch.tensor([0, 0, 1], dtype=torch.int32)
    thr = torch.tensor(ops.hedge_thresholds([0.5]), dtype=torch.int32)
    with pytest.raises(_lib.HgrError):
        ops.subtree_hedge(torch.zeros(2, 2), None, ptr, nodes, 1.0, thr)
    with pytest.raises(_lib.HgrError):
        ops.hedge_counters_rows(torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), ptr, nodes,
                                torch.zeros(1, ops.HEDGE_COLS, dtype=torch.int64))
