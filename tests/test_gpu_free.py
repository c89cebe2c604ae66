"""GPU: the FREE baseline on the device against the fixtures the reference's own code recorded (tools/make_golden_free.py; its
docstring defines err32, err16, the gradient floors and the per-row gaps; tests/test_free_host.py rebuilds the inputs by seed).

  * forward, fed the recorded z / eps: dtype="fp32" within 4 x err32 of the fp64 run (the factor tests/test_gpu_cnzsl.py uses for
    its products; K is sliced as cnzsl.cosine_logits slices it), dtype="bf16" within 3 x err16.
  * two fit_zsl steps from the fixture's state with the recorded permutations and eps: losses, bias gradients and the first weight
    gradient within 3 x err16 of fp64; the weights after two steps on EVERY recorded entry within 3 k16 lr err16 / (|g| / max|g|),
    at most twice the cap two Adam steps obey, and the device's own movement within that cap (the tool derives both); the third
    loader batch is never trained on; a step repeated from the same state is bit-equal.
  * test() with dtype="fp32": pred, top1, lv (where the winner is no filler) on every row (the fixture asserts that all deciding gaps
    exceed 8 x err32_logit), the nine counters and the metric string; with dtype="bf16": the per-row counters on the rows whose
    counter-deciding gaps exceed 2 x err16_logit - at least 90 % of them.
  * both switches at 0 against the fused kernels; the fp32 route refuses to fit (its forward passes and test() are what the issue
    asks of it); the command line's --synthetic run in a child process.

Measured on an MI355X: forward fp32 1.8e-7 .. 6.1e-7 against 1.7e-6, bf16 3.2e-3 .. 4.7e-3 against 1.4e-2; fit losses 1.5e-5 / 5.1e-5,
bias gradients 7.4e-4 / 3.6e-3, first weight gradient 1.4e-3 against 1.4e-2; weights: the worst entry at 0.49 of its bound, 8.5 % of
the entries at the cap, largest movement 2.0539 lr against 2.054 lr; test(): 129 of 129 rows compared in fp32 and in bf16."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_free_host import ROOT, fixture_inputs, load, rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _free():
    from hgr_net_amd import ops
    from hgr_net_amd.baseline import free
    return ops, free


def material(golden_dir):
    """The fixtures, the inputs rebuilt by seed and the tree: computed once, shared, never changed."""
    if not _CACHE:
        from hgr_net_amd.baseline import dgp_eval
        fit = load(golden_dir, "free_fit_small.npz")
        _CACHE.update(fwd=load(golden_dir, "free_forward_small.npz"), fit=fit, cls=load(golden_dir, "free_cls_small.npz"),
                      m=fixture_inputs(fit, fit["counts"]), tree=dgp_eval.build_list_tree(fit["edges"].tolist(), [str(w) for w in fit["nodes"]]))
    return _CACHE


def nets(m, dtype):
    _, free = _free()
    g, f = free.Generator(m["opt"], dtype), free.FR(m["opt"], m["opt"].attSize, dtype)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in m["sd_g"].items()})
    f.load_state_dict({k: torch.from_numpy(v) for k, v in m["sd_fr"].items()})
    return g.to(DEV).eval(), f.to(DEV).eval()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def classifier(c, dtype, perms=None, **kw):
    """A FREEClassifier on the fixture's material whose synthetic table comes from the RECORDED z (one generator call)."""
    _, free = _free()
    m, fit = c["m"], c["fit"]
    _, _, n_nodes, n_seen, num = (int(v) for v in fit["dims"][:5])
    g, f = nets(m, dtype)
    te = np.arange(n_seen, n_nodes)
    syn = g(dev(np.concatenate(m["z"], 0)), dev(m["att"][np.repeat(te, num)])).clone()
    it = iter(perms) if perms is not None else None
    return free.FREEClassifier(g, f, c["tree"], te, dev(m["att"]), n_nodes, dtype=dtype, seed=5, syn=(syn, dev(np.repeat(te, num))),
                               perm=(lambda n: torch.from_numpy(next(it).astype(np.int64))) if it is not None else None, **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_against_the_reference(golden_dir, dtype):
    c = material(golden_dir)
    fx, m = c["fwd"], c["m"]
    tol = 4 * float(fx["err32"]) if dtype == "fp32" else 3 * float(fx["err16"])
    rows, a = fx["x64"].shape[0], int(fx["dims"][0])
    _, free = _free()
    g, f = nets(m, dtype)
    z, eps = free.synth_rows(m["seed"], "free.fwd.z", rows, a), free.synth_rows(m["seed"], "free.fwd.eps", rows, a)
    x = g(dev(z), dev(m["att"][fx["cls"]])).float().cpu().numpy()
    real = m["real"][0][:rows]
    mus, stds, dis, pred, enc, h = f(dev(real), eps=dev(eps))
    errs = {"x": rel(x, fx["x64"]), "hidden": rel(f.getLayersOutDet().float().cpu().numpy(), fx["hidden64"]), "h": rel(h.float().cpu().numpy(), fx["h64"]),
            "mus": rel(mus.cpu().numpy(), fx["mus64"])}
    cl = classifier(c, dtype)
    big = cl.features(dev(real), dev(eps)).float().cpu().numpy()
    errs["input"] = rel(big, np.concatenate((real.astype(np.float64), fx["hidden64"], fx["h64"]), 1))
    print(dtype, errs, "tol", tol)
    assert max(errs.values()) <= tol
    if dtype == "fp32":
        assert max(rel(stds.cpu().numpy(), fx["stds32"]), rel(enc.cpu().numpy(), fx["enc32"]), rel(dis.cpu().numpy(), fx["dis32"]), rel(pred.cpu().numpy(), fx["pred32"])) <= tol


def test_two_fit_steps_against_the_reference(golden_dir):
    c = material(golden_dir)
    fit, m = c["fit"], c["m"]
    a, _, n_nodes, _, _, real_rows, syn_b = (int(v) for v in fit["dims"][:7])
    ops, free = _free()
    tol = 3 * float(fit["err16"])
    cols = torch.from_numpy(fit["cols"].astype(np.int64)).to(DEV)

    def fresh():
        cl = classifier(c, "bf16", perms=fit["perms"])
        cl.load_model({"fc.weight": torch.from_numpy(m["w0"]), "fc.bias": torch.zeros(n_nodes)})
        return cl
    cl = fresh()
    assert cl.batch_size == real_rows + syn_b == 1512
    eps = [dev(free.synth_rows(m["seed"], f"free.eps.fit.{i}", real_rows + syn_b, a)) for i in range(2)]
    errs = {}
    for i in range(2):
        loss = cl.step(dev(m["real"][i]), dev(m["labels"][i]), eps[i])
        assert np.array_equal(cl.last_index.cpu().numpy(), fit["index"][i])
        errs[f"loss{i}"] = abs(float(loss) - fit["losses64"][i]) / fit["losses64"][i]
        errs[f"gb{i}"] = rel(cl._bufs["gb"][:n_nodes].cpu().numpy(), fit["gb64"][i])
        if i == 0:
            part = cl._bufs["part"]
            gw = part.sum(0)[:n_nodes].index_select(1, cols) / cl.batch_size
            errs["gw1"] = rel(gw.cpu().numpy(), fit["gw1_64"])
    # every recorded entry against its own bound (tools/make_golden_free.py derives it): 3 k16 lr err16 / (|g| / max|g|), at most twice
    # the cap that two Adam steps obey - and that cap on the device's own movement
    lr, cap = float(fit["lr"]), float(fit["step_cap"])
    w0c = m["w0"][:, fit["cols"]]
    moved = cl.wp[:n_nodes].index_select(1, cols).cpu().numpy().astype(np.float64) - w0c
    moved64 = fit["w_final64"] - w0c.astype(np.float64)
    unit = lr * np.minimum(2 * cap, 3 * float(fit["k16"]) * float(fit["err16"]) / np.maximum(fit["gmin"].astype(np.float64), 1e-30))
    errs["w"] = float((np.abs(moved - moved64) / unit).max())
    print(errs, "tol", tol, "share of entries at the cap", float((unit >= 2 * cap * lr).mean()), "largest |moved| / lr", np.abs(moved).max() / lr)
    assert max(v for k, v in errs.items() if k != "w") <= tol and errs["w"] <= 1.0
    assert np.abs(moved).max() <= cap * lr * (1 + 1e-4), "two Adam steps move an entry by at most STEP_CAP lr"
    assert torch.equal(cl.w16.float(), cl.wp.to(torch.bfloat16).float()), "the 16-bit operand is the master weight rounded once"
    assert (cl.wp[n_nodes:] == 0).all() and (cl.bp[n_nodes:] == 0).all(), "padding classes stay zero"
    # fit_zsl: three loader batches, the last one skipped (NaN rows would poison the weights); repeated from the same state: the same bits
    loader = [(dev(m["real"][0]), dev(m["labels"][0])), (dev(m["real"][1]), dev(m["labels"][1])), (torch.full((real_rows, free.RES), float("nan"), device=DEV), dev(m["labels"][2]))]
    runs = []
    for _ in range(2):
        r = fresh()
        losses = r.fit_zsl(loader, nepoch=1, log=None)
        assert len(losses) == 2 and r.t == 2 and bool(torch.isfinite(r.wp).all())
        runs.append((r.wp.clone(), r.bp.clone(), r.w16.clone(), torch.stack(losses)))
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "a run repeated from the same state gives bit-equal parameters"


def test_fp32_route_refuses_to_fit(golden_dir):
    cl = classifier(material(golden_dir), "fp32")
    with pytest.raises(NotImplementedError, match="16-bit routes"):
        cl.step(torch.zeros(512, 2048, device=DEV), torch.zeros(512, dtype=torch.int64, device=DEV))


def test_synthesize_is_a_function_of_the_seed_not_of_the_chunks(golden_dir):
    c = material(golden_dir)
    m, fwd = c["m"], c["fwd"]
    ops, free = _free()
    g, _ = nets(m, "bf16")
    att, classes, num = dev(m["att"]), [20, 13, 95, 13, 40, 41, 77], 25
    one, labels = free.synthesize(g, classes, att, num, seed=9, chunk_classes=64)
    for chunk in (1, 3):
        other, l2 = free.synthesize(g, classes, att, num, seed=9, chunk_classes=chunk)
        assert torch.equal(one, other) and torch.equal(labels, l2), f"chunks of {chunk} classes"
    assert one.dtype == torch.bfloat16 and tuple(one.shape) == (len(classes) * num, free.RES)
    assert labels.cpu().tolist() == [q for q in classes for _ in range(num)]
    assert not torch.equal(one, free.synthesize(g, classes, att, num, seed=10)[0])
    a = m["att"].shape[1]
    z = free.normal_host(9, free.STREAM_Z, 0, len(classes) * num, a)
    want = free.generator_host(m["sd_g"], z, m["att"][np.repeat(classes, num)].astype(np.float64), torch.float64).numpy()
    err = rel(one.float().cpu().numpy(), want)
    print("synthesize against the float64 twin on the counter noise:", err, "tol", 3 * float(fwd["err16"]))
    assert err <= 3 * float(fwd["err16"])


def _row_counts(pred, top1, lv, target, tree):
    """Per row what the nine counters add up: hits@1,2,5,10,20, ancestors hit by the top-1, and the level matches along the path."""
    path = tree.path(int(target))
    hits = [(pred[:, :k] == target).sum(1) for k in (1, 2, 5, 10, 20)]
    anc = sum((top1 == q).astype(np.int64) for q in path)
    match = [(lv[:, tree.depth[q]] == q).astype(np.int64) for q in path]
    return np.stack(hits + [anc] + match, 1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_test_against_the_reference(golden_dir, dtype):
    c = material(golden_dir)
    fit, m, tree = c["fit"], c["m"], c["tree"]
    a, n_seen = int(fit["dims"][0]), int(fit["dims"][3])
    ops, free = _free()
    cl = classifier(c, dtype)
    cl.load_model({"fc.weight": torch.from_numpy(c["cls"]["w"]), "fc.bias": torch.from_numpy(c["cls"]["b"])})
    counts = fit["counts"]
    if dtype == "fp32":
        keep_all = fit["gap"] > 8 * float(fit["err32_logit"])
    else:
        keep_all = fit["gap_counters"] > 2 * float(fit["err16_logit"])
    print(dtype, "rows compared", int(keep_all.sum()), "of", len(keep_all))
    assert keep_all.all() if dtype == "fp32" else keep_all.mean() >= 0.9
    o = 0
    for i, n in enumerate(counts.tolist()):
        t = n_seen + i
        eps = dev(free.synth_rows(m["seed"], f"free.eps.test.{i}", n, a))
        pred, top1, lv = (v.cpu().numpy() for v in cl.add(dev(m["test"][o:o + n]), t, eps))
        keep = keep_all[o:o + n]
        rp, rt, rl = fit["pred"][o:o + n], fit["top1"][o:o + n], fit["lv"][o:o + n]
        if dtype == "fp32":
            assert np.array_equal(pred[keep], rp[keep]) and np.array_equal(top1.reshape(-1)[keep], rt[keep]), f"batch {i}"
            real = tree.depth[rl] == np.arange(tree.n_levels)[None, :]          # the winner is on its level: no filler
            assert np.array_equal(lv[keep][real[keep]], rl[keep][real[keep]]), f"batch {i}"
        got, want = _row_counts(pred, top1.reshape(-1), lv, t, tree), _row_counts(rp, rt, rl, t, tree)
        assert np.array_equal(got[keep], want[keep]), f"batch {i}: per-row counters"
        o += n
    assert cl.counters()[8] == counts.sum()
    if dtype == "fp32":
        assert np.array_equal(cl.counters(), fit["acc"]), (cl.counters(), fit["acc"])
        assert cl.result() == "\n" + str(fit["lines"][-1])


def test_switches_select_twins_that_agree(golden_dir, monkeypatch):
    c = material(golden_dir)
    fit, m = c["fit"], c["m"]
    a, _, n_nodes, _, _, real_rows, syn_b = (int(v) for v in fit["dims"][:7])
    ops, free = _free()
    eps = dev(free.synth_rows(m["seed"], "free.eps.fit.0", real_rows + syn_b, a))

    def one_step(**env):
        for k in ("HGR_FREE_NLL_FUSED", "HGR_FREE_ADAM_FUSED"):
            monkeypatch.setenv(k, env.get(k, "1"))
        cl = classifier(c, "bf16", perms=fit["perms"])
        cl.load_model({"fc.weight": torch.from_numpy(m["w0"]), "fc.bias": torch.zeros(n_nodes)})
        loss = cl.step(dev(m["real"][0]), dev(m["labels"][0]), eps)
        return cl, float(loss)
    fused, loss = one_step()
    assert fused.nll_fused and fused.adam_fused
    adam, loss_a = one_step(HGR_FREE_ADAM_FUSED="0")
    assert not adam.adam_fused and loss_a == loss
    for name in ("wp", "mw", "vw", "w16", "bp"):                       # at most two slices: their sum has one order
        assert torch.equal(getattr(fused, name), getattr(adam, name)), name
    nll, loss_n = one_step(HGR_FREE_NLL_FUSED="0")
    assert not nll.nll_fused and abs(loss_n - loss) <= 4 * np.spacing(np.float32(abs(loss)))
    d1, d2 = fused._bufs["d16"].view(torch.int16).to(torch.int32), nll._bufs["d16"].view(torch.int16).to(torch.int32)
    order = lambda b: torch.where(b < 0, -(b & 0x7FFF), b)
    assert (order(d1) - order(d2)).abs().max().item() <= 1, "dlogits within one 16-bit ulp"


def test_cli_synthetic_run_ends_with_a_metric_line():
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    out = subprocess.run([sys.executable, "-m", "hgr_net_amd.baseline.validate_free", "--synthetic", "300", "--epochs", "1"], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    last = [l for l in out.stdout.split("\n") if l.strip()][-1]
    assert re.match(r"Top@1\(%\):\d+\.\d\d, Top@2.* hit_ratio\(%\):\d+\.\d\d path_ratio\(%\):\d+\.\d\d point_ratio\(%\):\d+\.\d\d$", last), last
