"""CPU: the CNZSL baseline's host side - the plain torch / numpy twins of hgr_net_amd.baseline.cnzsl against what the reference's own
classes and `test()` recorded (tools/make_golden_cnzsl.py -> tests/golden/cnzsl_train_small.npz, cnzsl_eval_small.npz), the
state_dict schema, and the command line.

Bounds.  The training fixture holds `err32`: the reference's classes were run in fp32 and in fp64, and err32 is the largest over the
gradient tensors of max|g32 - g64| / norm - the measured distance between two correct implementations (6.6e-7).  A gradient,
the losses and the logits are accepted within GRAD_TOL = 4 x err32 of the fp64 record.  norm = max|g64|, with one exception written
into the fixture by the tool: the gradient of 'model.2.bias' sits behind a standardisation that subtracts the column mean, so in
exact arithmetic it is zero (fp64: 1e-16, fp32: 4e-8 - rounding noise); its error is measured against what it is a cancelling sum
of, absdz = max over columns of sum_rows |d loss / d z|.
Parameters after three Adam steps: Adam's update m / (sqrt(v) + eps) has degree 0 in the gradient history, so an element whose
coupled gradient g + wd p stayed above THETA = 100 x GRAD_TOL (relative to the tensor's largest) sees a relative gradient error of at
most GRAD_TOL / THETA = 1 % per step, which moves the update by at most 2 x 1 % of its bound 1 (numerator and denominator): after
STEPS steps |p - p_ref| <= STEPS x lr x 0.02 = 6e-6.  Elements below THETA are left out; the tool asserted they are at most 1 % of
any weight tensor."""
import functools
import json
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from hgr_net_amd.baseline import cnzsl, dgp_eval, train_cnzsl
from hgr_net_amd import synth

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
KEYS = ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.3.running_mean", "model.3.running_var",
        "model.5.running_mean", "model.5.running_var", "model.6.weight", "model.6.bias"]
STEPS = 3


@functools.lru_cache(maxsize=None)
def train_fixture() -> types.SimpleNamespace:
    """The training fixture and its inputs, regenerated from the seed exactly as the tool made them."""
    z = dict(np.load(GOLD / "cnzsl_train_small.npz"))
    seed = int(z["seed"])
    s, a, h, p, b = (int(v) for v in z["dims"])
    fx = types.SimpleNamespace(z=z, seed=seed, S=s, A=a, H=h, P=p, B=b, lr=float(z["lr"]), wd=float(z["weight_decay"]), err32=float(z["err32"]))
    fx.sd0 = cnzsl.synth_state(seed, a, h, p)
    fx.attrs = cnzsl.synth_rows(seed, "cnzsl.train.attrs", s, a)
    x0, x1 = cnzsl.synth_rows(seed, "cnzsl.train.x0", b, p), cnzsl.synth_rows(seed, "cnzsl.train.x1", b, p)
    fx.feats, fx.labels = [x0, x1, x0], [z["labels"][i].astype(np.int64) for i in range(STEPS)]
    fx.grad_tol = 4 * fx.err32
    fx.theta = 100 * fx.grad_tol
    fx.state_tol = STEPS * fx.lr * 2 * (fx.grad_tol / fx.theta)
    return fx


@functools.lru_cache(maxsize=None)
def eval_fixture() -> types.SimpleNamespace:
    z = dict(np.load(GOLD / "cnzsl_eval_small.npz"))
    seed = int(z["seed"])
    a, h, p = (int(v) for v in z["dims"])
    fx = types.SimpleNamespace(z=z, seed=seed, A=a, H=h, P=p, err32=float(z["err32"]), edges=z["edges"].tolist(), nodes=z["nodes"].tolist(),
                               counts=z["counts"].astype(np.int64), test_index=z["test_index"].astype(np.int64), lines=z["lines"].tolist())
    fx.sd = cnzsl.synth_state(seed, a, h, p, running=True)
    fx.attrs = cnzsl.synth_rows(seed, "cnzsl.eval.attrs", len(fx.nodes), a)
    fx.feats = cnzsl.synth_rows(seed, "cnzsl.eval.feats", int(fx.counts.sum()), p)
    fx.tree = dgp_eval.build_list_tree(fx.edges, fx.nodes)
    fx.offsets = np.concatenate([[0], np.cumsum(fx.counts)])
    return fx


def grad_err(name: str, got, want64, absdz: float, cn: bool = True) -> float:
    """max|got - want| / norm with the fixture's rule: max|want|, or absdz for the cancelling bias gradient behind a standardisation."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    norm = absdz if (cn and name == "model.2.bias") else np.abs(want64).max()
    return float(np.abs(got - want64).max() / norm)


def rel_err(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def check_state(fx, sd: dict) -> None:
    """The state after step 3 against the fp32 record: elements above THETA within the derived bound, running vectors in full."""
    for k in cnzsl.TRAINABLE:
        if k == "model.2.bias":
            # its gradient is rounding noise around zero (the module docstring), so what Adam divides is wd p + noise and no element
            # is above THETA x absdz: only Adam's own bound holds - each side moved by at most lr per step
            diff = np.abs(np.asarray(sd[k], np.float64) - fx.z["sd3_" + k]).max()
            assert diff <= 2 * STEPS * fx.lr * 1.01, (k, diff)
            continue
        keep = fx.z["gmin_" + k] >= fx.theta
        assert keep.mean() >= (0.99 if k.endswith("weight") else 0.95), k
        diff = np.abs(np.asarray(sd[k], np.float64) - fx.z["sd3_" + k])[keep].max()
        moved = np.abs(fx.z["sd3_" + k] - fx.z["sd0_" + k])[keep].max()
        print(f"{k}: |p - p_ref| {diff:.3e} (bound {fx.state_tol:.1e}; the parameters moved by up to {moved:.3e})")
        assert diff <= fx.state_tol, (k, diff)
        assert moved > 10 * fx.state_tol                                   # the bound is far below the movement it checks
    for k in cnzsl.RUNNING:
        err = rel_err(sd[k], fx.z["sd3_" + k])
        print(f"{k}: {err:.3e}")
        assert err <= fx.grad_tol, (k, err)


def test_fixture_inputs_come_from_the_seed():
    fx = train_fixture()
    assert set(fx.sd0) == set(KEYS)
    for k in KEYS:
        assert np.array_equal(fx.sd0[k], fx.z["sd0_" + k]), k
    assert 1e-8 < fx.err32 < 1e-5
    assert len(set(fx.labels[0].tolist())) > 1 and len(set(fx.labels[1].tolist())) == 1 and np.array_equal(fx.labels[0], fx.labels[2])
    assert fx.z["losses32"][2] < fx.z["losses32"][0]
    assert np.isfinite(fx.z["logits32"]).all()                              # no zero-norm prototype row


def test_training_twin_reproduces_the_reference():
    fx = train_fixture()
    state = cnzsl.train_state_host(fx.sd0, torch.float32)
    for step in range(STEPS):
        loss, grads, logits = cnzsl.train_step_host(state, fx.feats[step], fx.labels[step], fx.attrs, lr=fx.lr, weight_decay=fx.wd)
        if step == 0:
            assert list(grads) == list(cnzsl.TRAINABLE)
            for k, g in grads.items():
                err = grad_err(k, g.numpy(), fx.z["grad1_64_" + k], float(fx.z["absdz64"]))
                print(f"{k}: gradient error {err:.3e} (bound {fx.grad_tol:.3e})")
                assert err <= fx.grad_tol, (k, err)
            assert abs(state["absdz"] / float(fx.z["absdz64"]) - 1) < 1e-4
        assert abs(float(loss) / fx.z["losses64"][step] - 1) <= fx.grad_tol, (step, float(loss))
        assert rel_err(logits.numpy(), fx.z["logits64"][step]) <= fx.grad_tol, step
    assert state["t"] == STEPS
    check_state(fx, {k: v.numpy() for k, v in state["sd"].items()})


def test_training_twin_is_exact_in_fp64():
    """The same twin in fp64 lands on the fp64 record: the reference's arithmetic, not something close to it."""
    fx = train_fixture()
    state = cnzsl.train_state_host(fx.sd0, torch.float64)
    _, grads, _ = cnzsl.train_step_host(state, fx.feats[0], fx.labels[0], fx.attrs, lr=fx.lr, weight_decay=fx.wd, update=False)
    for k, g in grads.items():
        assert grad_err(k, g.numpy(), fx.z["grad1_64_" + k], float(fx.z["absdz64"])) < 1e-12, k
    assert state["t"] == 0 and np.array_equal(state["sd"]["model.3.running_var"].numpy(), np.ones(fx.H))


def test_std_chain_twin_quirks():
    """Division by the variance (not its root), the unbiased variance, the running update, a constant column."""
    z = torch.tensor([[1.0, 0.75], [3.0, 0.75], [8.0, 0.75]], dtype=torch.float64)
    run = tuple(torch.tensor(v, dtype=torch.float64) for v in ([0.5, 0.5], [2.0, 2.0], [0.0, 0.0], [1.0, 1.0]))
    c, a, stats, new = cnzsl.std_chain_host(z, torch.zeros(2, dtype=torch.float64), run, train=True)
    assert stats[0].tolist() == [4.0, 0.75] and stats[1].tolist() == [13.0, 0.0]                  # sum (x - 4)^2 / (3 - 1) = 26 / 2
    assert torch.allclose(a[:, 0], torch.tensor([0.0, 0.0, 4.0 / (13.0 + 1e-5)], dtype=torch.float64), atol=1e-15)
    assert a[:, 1].tolist() == [0.0, 0.0, 0.0] and c[:, 1].tolist() == [0.0, 0.0, 0.0] and bool(torch.isfinite(c).all())
    assert torch.allclose(new[0], torch.tensor([0.9 * 0.5 + 0.1 * 4.0, 0.9 * 0.5 + 0.1 * 0.75], dtype=torch.float64))
    assert torch.allclose(new[1], torch.tensor([0.9 * 2.0 + 0.1 * 13.0, 0.9 * 2.0], dtype=torch.float64))
    ce, ae, _, none = cnzsl.std_chain_host(z, torch.zeros(2, dtype=torch.float64), run, train=False)
    assert none is None and torch.allclose(ae[:, 0], torch.tensor([0.5, 2.5, 7.5], dtype=torch.float64) / (2.0 + 1e-5))
    assert torch.allclose(ce, ae / (1.0 + 1e-5))


def test_prototype_twin_reproduces_the_recorded_logits():
    fx = eval_fixture()
    assert 1e-8 < fx.err32 < 1e-5
    with torch.no_grad():
        protos = cnzsl.prototypes_host(fx.sd, fx.attrs)
        assert protos.dtype == torch.float32 and tuple(protos.shape) == (len(fx.nodes), fx.P) and bool((protos.norm(dim=1) > 0).all())
        logits = cnzsl.logits_host(protos, fx.feats).numpy()
    err = rel_err(logits, fx.z["logits"])
    print(f"logits: {err:.3e} (bound {4 * fx.err32:.3e})")
    assert err <= 4 * fx.err32
    assert (fx.feats < 0).any() and (fx.z["logits"] < -1).any()


def test_scoring_twin_reproduces_every_metric_line():
    """score_host on the reference's own logits: integers, so every cumulative line and the final one are equal as strings."""
    fx = eval_fixture()
    assert fx.tree.nodes == fx.nodes and len(fx.lines) == len(fx.counts) + 1 and (fx.counts == 1).any()
    acc, filler = np.zeros(9), 0
    for i in range(len(fx.counts)):
        rows = fx.z["logits"][fx.offsets[i]:fx.offsets[i + 1]]
        t = int(fx.test_index[i])
        r = cnzsl.score_host(rows, t, fx.tree, fx.test_index)
        for q in fx.tree.path(t):                                           # a filler win: the level's best test class scores below -1
            on = fx.test_index[fx.tree.depth[fx.test_index] == fx.tree.depth[q]]
            lost = rows[:, on].max(1) < -1.0
            filler += int(lost.sum())
            assert not (r["lv"][lost, fx.tree.depth[q]] == q).any()
        acc += r["acc"]
        assert cnzsl.metric_string(acc) == "\n" + fx.lines[i], i
    assert filler >= 1 and cnzsl.metric_string(acc) == "\n" + fx.lines[-1]
    # rows of mixed classes count like the same rows class by class
    tg = np.repeat(fx.test_index[:len(fx.counts)], fx.counts)
    mixed = cnzsl.score_host(fx.z["logits"], tg, fx.tree, fx.test_index)
    assert np.array_equal(mixed["acc"][[0, 1, 2, 3, 4, 5, 8]], acc[[0, 1, 2, 3, 4, 5, 8]]) and np.allclose(mixed["acc"], acc, rtol=0, atol=1e-9)


def test_state_dict_has_the_reference_schema(tmp_path):
    fx = train_fixture()
    model = cnzsl.CNZSLModel(fx.A, fx.H, fx.P, device="cpu")
    assert list(model.state_dict()) == KEYS
    assert [k for k, p in model.named_parameters() if p.requires_grad] == list(cnzsl.TRAINABLE)
    bound = np.sqrt(3.0 / (fx.H * fx.P))
    assert 0.9 * bound < float(model.model[6].weight.data.abs().max()) <= bound
    assert float(cnzsl.CNZSLModel(fx.A, fx.H, fx.P, init=False, device="cpu").model[6].weight.data.abs().max()) > 2 * bound
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fx.sd0.items()})            # strict: a reference checkpoint loads unchanged
    torch.save(model.state_dict(), tmp_path / "cnzsl__6")
    again = cnzsl.CNZSLModel(fx.A, fx.H, fx.P, device="cpu")
    again.load_state_dict(torch.load(tmp_path / "cnzsl__6"))
    for k in KEYS:
        assert np.array_equal(again.state_dict()[k].numpy(), fx.sd0[k]), k
    plain = cnzsl.CNZSLModel(fx.A, fx.H, fx.P, cn=False, device="cpu")
    assert list(plain.state_dict()) == [k for k in KEYS if "running" not in k]
    x, attrs = torch.zeros(2, fx.P), torch.zeros(3, fx.A)
    with pytest.raises(NotImplementedError, match="CNZSLTrainer"):
        model.train()(x, attrs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.eval()(x, attrs)
    with pytest.raises(ValueError):
        cnzsl.CNZSLModel(fx.A, 50, fx.P, device="cpu")


def test_entry_points_are_declared():
    from hgr_net_amd import _lib
    header = (ROOT / "include" / "hgr.h").read_text()
    for name, n_args in (("hgr_cnzsl_std_chain_fwd", 18), ("hgr_cnzsl_std_chain_bwd", 15), ("hgr_bias_relu_f32", 8), ("hgr_relu_bwd_colsum_f32", 11)):
        proto = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, f"include/hgr.h declares {name}"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(proto.group(1).split(",")) == n_args
        assert hasattr(_lib.load(), name)


def test_command_line_and_synthetic_material(tmp_path):
    args = train_cnzsl.parse_args(["--synthetic", "500", "--epoch", "2"])
    assert (args.synthetic, args.epoch, args.batch_size, args.test_batch_size, args.print_freq) == (500, 2, 256, 256, 1)
    assert (args.data_train, args.data_test, args.attr, args.file_path, args.train, args.cn, args.init, args.load) == \
        ("train", "rest", "transformer", "cnzsl/cnzsl_", True, True, True, False)
    args = train_cnzsl.parse_args(["--attributes", "a.npz", "--features", "f.npz", "--cn", "False", "--init", "False", "--train", "False", "--load",
                                   "--file_path", "x/y", "--graph_path", "g.json", "--split_path", "s.json", "--seed", "4"])
    assert (args.cn, args.init, args.train, args.load, args.file_path, args.seed) == (False, False, False, True, "x/y", 4)
    for bad in ([], ["--synthetic", "50"], ["--synthetic", "500", "--cn", "no"], ["--synthetic", "500", "--batch_size", "0"]):
        with pytest.raises(SystemExit):
            train_cnzsl.parse_args(bad)
    edges, splits, attrs, feats = train_cnzsl.synthetic_material(120, 1)
    nodes = train_cnzsl.ordered_nodes(edges, splits["train"])
    assert len(nodes) == 120 and nodes[:30] == splits["train"] and sorted(nodes) == sorted(synth_names(edges))
    assert attrs.shape == (120, train_cnzsl.SYN_ATTR) and attrs.dtype == np.float32
    assert set(feats) == set(splits["train"]) | set(splits["rest"]) and len(splits["rest"]) == 30
    assert all(f.shape == (train_cnzsl.SYN_TRAIN_ROWS, train_cnzsl.SYN_PROTO) for w, f in feats.items() if w in splits["train"])
    again = train_cnzsl.synthetic_material(120, 1)
    assert np.array_equal(again[2], attrs) and all(np.array_equal(again[3][w], feats[w]) for w in feats)
    tree = dgp_eval.build_list_tree(edges, nodes)                          # every node's whole path is in the list
    assert tree.n_levels <= dgp_eval.MAXL
    # attribute files: the matrix, or chunks as text_feats.json is read
    np.savez(tmp_path / "a.npz", attrs=attrs)
    json.dump([attrs[:50].tolist(), attrs[50:].tolist()], open(tmp_path / "chunks.json", "w"))
    json.dump(attrs.tolist(), open(tmp_path / "flat.json", "w"))
    for name in ("a.npz", "chunks.json", "flat.json"):
        assert np.array_equal(train_cnzsl.load_attributes(str(tmp_path / name)), attrs), name
    index = {w: i for i, w in enumerate(nodes)}
    got = list(train_cnzsl.class_batches(feats, splits["train"][:3] + ["absent"], index, 5, "cpu"))
    assert [(tuple(x.shape), t) for x, t in got] == [((5, 256), 0), ((3, 256), 0), ((5, 256), 1), ((3, 256), 1), ((5, 256), 2), ((3, 256), 2)]


def synth_names(edges):
    return {w for e in edges for w in e} - {synth.ROOT}
