"""CPU: the host side of hierarchy-path decoding - the weight table of hgr_path_scores against tree_model.get_weights and the
reference-captured weights, the two command-line flags, the entry point in include/hgr.h and in the ctypes table, and the arguments
the Python surface rejects before anything touches a device."""
import json
import re
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
METHODS = ("equal", "increasing", "decreasing", "nl_increasing", "nl_decreasing", "adaptive")


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    """The device="cpu" model of test_tree_model_host_logic (copied: test modules do not import each other), layer_weight set to
    values in [0, 0.3): the adaptive weights are then neither a uniform nor a one-hot row."""
    from hgr_net_amd import synth
    from hgr_net_amd.clip.model import build_model
    from hgr_net_amd.hierarchy import build_hierarchy
    from hgr_net_amd.model import tree_model
    tmp = tmp_path_factory.mktemp("path_host")
    edges = synth.make_dag(120, depth=8, seed=3, multi_parent=0.05)
    g = tmp / "g.json"
    g.write_text(json.dumps(edges))
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], 40, 50, 13)
    o = types.SimpleNamespace(device="cpu", folder=str(tmp), exp_name="HGR", weights="adaptive", out_ratio=0.25, in_ratio=0.5,
                              from_epoch=-1, graph_path=str(g), arch="x", fetch=False, load=False, load_path="none", scale=1.0,
                              num_compare=16, k=1, sample_strategy="topk", weighting="both")
    m = tree_model(o, splits["all"], splits["rest"], node_tokens=synth.make_tokens(120, 11, 512),
                   clip_model=build_model(synth.clip_state_dict("tiny-vit", 0)))
    with torch.no_grad():
        m.layer_weight.copy_(0.3 * torch.rand(m.layer_weight.shape, generator=torch.Generator().manual_seed(3)))
    return m


@pytest.mark.parametrize("method", METHODS)
def test_weight_table_rows_are_get_weights(cpu_model, method):
    from hgr_net_amd import evaluate, ops
    m = cpu_model
    tab = evaluate.path_weight_table(m, method)
    assert tab.shape == (33, 32) == (ops.PATH_MAXL + 1, ops.PATH_MAXL) and tab.dtype == torch.float32 and tab.device == m.train_index.device
    assert not tab.requires_grad
    n_rows = m.max_depth + 1
    assert 2 <= n_rows <= 32
    want = torch.zeros(33, 32)
    for L in range(1, n_rows + 1):
        w = m.get_weights(method, L).detach()
        assert torch.equal(tab[L, :L], w), (method, L)                      # bit for bit
        want[L, :L] = w
        assert abs(float(tab[L].double().sum()) - 1.0) <= 1e-6 and float(tab[L].min()) >= 0.0, (method, L)
    assert torch.equal(tab, want)                                           # every other entry is 0: row 0, rows behind max_depth + 1, columns >= L
    if method == "adaptive":
        row = tab[n_rows, :n_rows]
        assert float(row.max()) < 0.5 and float(row.min()) > 0.01 and float(row.max() - row.min()) > 1e-3      # neither one-hot nor uniform


def test_weight_table_equals_the_reference_captured_weights(cpu_model, golden_dir):
    from hgr_net_amd import evaluate
    table = json.load(open(golden_dir / "tree_tinyvit_n90.json"))["weights_table"]           # captured from the reference
    assert set(table) == set(METHODS) - {"adaptive"}
    for method, by_depth in table.items():
        tab = evaluate.path_weight_table(cpu_model, method)
        seen = 0
        for d, ref in by_depth.items():
            L = int(d)
            if L <= cpu_model.max_depth + 1:
                assert torch.allclose(tab[L, :L], torch.tensor(ref), rtol=0, atol=1e-7), (method, L)
                seen += 1
        assert seen >= 4, method


def test_self_weights_are_one_hot_and_unknown_methods_are_rejected(cpu_model):
    from hgr_net_amd import evaluate
    tab = evaluate.path_weight_table(cpu_model, "self")
    want = torch.zeros(33, 32)
    for L in range(1, cpu_model.max_depth + 2):
        want[L, L - 1] = 1.0
    assert torch.equal(tab, want)
    with pytest.raises(ValueError):
        cpu_model.get_weights("self", 3)                                    # lives in the table only
    for bad in ("nonsense", "", "Equal"):
        with pytest.raises(ValueError):
            evaluate.path_weight_table(cpu_model, bad)
    assert set(evaluate.DECODE_WEIGHTS) == set(METHODS) | {"self"} and evaluate.DECODES == ("flat", "path")


def test_adaptive_table_without_layer_weight_is_a_value_error(cpu_model):
    from hgr_net_amd import evaluate
    fake = types.SimpleNamespace(train_index=cpu_model.train_index, max_depth=cpu_model.max_depth, get_weights=cpu_model.get_weights)
    with pytest.raises(ValueError):
        evaluate.path_weight_table(fake, "adaptive")


def test_parser_flags_defaults_and_choices():
    from hgr_net_amd import evaluate
    from hgr_net_amd.main import build_parser
    p = build_parser()
    o = p.parse_args([])
    assert o.decode == "flat" and o.decode_weights == "increasing"
    o = p.parse_args(["--decode", "path", "--decode_weights", "self"])
    assert o.decode == "path" and o.decode_weights == "self"
    for w in evaluate.DECODE_WEIGHTS:
        assert p.parse_args(["--decode_weights", w]).decode_weights == w
    for bad in (["--decode", "tree"], ["--decode_weights", "nonsense"], ["--decode"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_header_ctypes_table_and_constants_agree():
    from hgr_net_amd import _lib, ops
    header = (ROOT / "include" / "hgr.h").read_text()
    proto = re.search(r"\bint\s+hgr_path_scores\s*\(([^;]*)\)\s*;", header)
    assert proto, "include/hgr.h declares hgr_path_scores"
    args = [a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()]
    assert "hgr_path_scores" in _lib.SIGNATURES and len(_lib.SIGNATURES["hgr_path_scores"]) == len(args) == 10
    maxl = int(re.search(r"#define\s+HGR_PATH_MAXL\s+(\d+)", header).group(1))
    assert maxl == int(re.search(r"#define\s+HGR_REPORT_MAXL\s+(\d+)", header).group(1))
    assert maxl == ops.PATH_MAXL == ops.REPORT_MAXL == 32
    assert hasattr(_lib.load(), "hgr_path_scores")                          # the built library exports it (no device needed to load)
    assert _lib.ABI_VERSION == 5


def test_path_scores_on_cpu_tensors_raises_hgr_error():
    from hgr_net_amd import _lib, ops
    ptr = torch.tensor([0, 1, 3], dtype=torch.int32)
    nodes = torch.tensor([0, 0, 1], dtype=torch.int32)
    wtab = torch.zeros(33, 32)
    with pytest.raises(_lib.HgrError):
        ops.path_scores(torch.zeros(2, 2), ptr, nodes, wtab)
    with pytest.raises(_lib.HgrError):
        ops.path_scores(torch.zeros(2, 2), ptr, nodes, wtab, out=torch.zeros(2, 2))


def test_evaluator_rejects_an_unknown_decode(cpu_model):
    from hgr_net_amd import evaluate
    for kw in ({"decode": "nonsense"}, {"decode": "Path"}, {"decode": "path", "decode_weights": "nonsense"}):
        with pytest.raises(ValueError):
            evaluate.Evaluator(cpu_model, **kw)
    ev = evaluate.Evaluator(cpu_model)                                      # the default: flat, nothing extra is kept
    assert ev.decode == "flat" and ev._wtab is None and ev._scores is None and ev.report is None
    ev = evaluate.Evaluator(cpu_model, decode="path", decode_weights="equal")
    assert ev.decode == "path" and not ev.fused_ok() and ev._scores is None
    assert torch.equal(ev._wtab, evaluate.path_weight_table(cpu_model, "equal"))
