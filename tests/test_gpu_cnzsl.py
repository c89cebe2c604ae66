"""GPU: the CNZSL baseline on the device - the class-standardisation chain kernels against their torch twin, `CNZSLTrainer` and
`CNZSLEvaluator` against the fixtures the reference's own code recorded (tests/test_cnzsl_host.py explains the fixtures and derives
GRAD_TOL = 4 x err32 and the parameter bound), and the command line end to end.

Chain kernels.  The bound is the golden tool's rule applied to the twin: per shape the twin runs in fp32 and in fp64 on the CPU,
err32 = the largest over the outputs (c, a, stats, the four running vectors, dz, dbias) of max|t32 - t64| / norm, and the device
must stay within 4 x max(err32, 2^-23) of the fp64 twin - the floor because every output is behind at least four rounded fp32
operations of half an ulp (2^-24) each, which a shape as small as (2, 4) can hit exactly in one implementation and not in the
other.  norm = max|t64|; for dbias, a sum that cancels to zero behind the mean subtraction, norm = max over columns of
sum_rows |dz| (as for 'model.2.bias' in the fixture).  Measured on an MI355X, err32 of the fp32 twin / error of the device:
(2, 4) 1.9e-7 / 5.5e-8; (37, 48) 1.9e-7 / 1.7e-7; (64, 40) 1.9e-7 / 1.7e-7; (1500, 20) 2.2e-7 / 2.5e-7; (2048, 16) 1.8e-7 / 2.7e-7;
(2049, 16) 2.2e-7 / 2.8e-7; (5000, 32) 2.0e-7 / 2.5e-7; evaluation mode 5.8e-8 .. 1.2e-7, the device equal to the twin.  Trainer:
gradients 9e-8 .. 5.9e-7 against 4 x err32 = 2.65e-6; evaluator logits 9.4e-7 against 1.54e-6 (profiles/NOTES.md, "CNZSL")."""
import re

import numpy as np
import pytest
import torch

from test_cnzsl_host import STEPS, check_state, eval_fixture, grad_err, rel_err, train_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 2.0 ** -23
# (S, H, ld): the smallest legal case; the training fixture's; ld > H with a partial strip; a strip resident beyond the 64 KB a launch gets
# unasked; the last resident row count and the first streamed one; well beyond it
CHAIN_SHAPES = [(2, 4, 4), (37, 48, 48), (64, 40, 52), (1500, 20, 20), (2048, 16, 16), (2049, 16, 24), (5000, 32, 32)]


def _ops():
    from hgr_net_amd import ops
    return ops


def _dev_rows(a: np.ndarray, ld: int, fill: float = 7.0) -> torch.Tensor:
    """A device view [rows, cols] of a buffer with leading dimension ld; the padding holds `fill`."""
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return buf[:, :a.shape[1]]


def _chain_inputs(s: int, h: int):
    from hgr_net_amd.baseline import cnzsl
    z = cnzsl.synth_rows(5, f"chain.z.{s}.{h}", s, h)
    dc = cnzsl.synth_rows(5, f"chain.dc.{s}.{h}", s, h)
    bias = 0.3 * cnzsl.synth_rows(5, f"chain.b.{s}.{h}", 1, h)[0]
    run = [0.1 * cnzsl.synth_rows(5, f"chain.r0.{s}.{h}", 1, h)[0], 0.5 + np.abs(cnzsl.synth_rows(5, f"chain.r1.{s}.{h}", 1, h)[0]),
           0.1 * cnzsl.synth_rows(5, f"chain.r2.{s}.{h}", 1, h)[0], 0.5 + np.abs(cnzsl.synth_rows(5, f"chain.r3.{s}.{h}", 1, h)[0])]
    return z, dc, bias, [np.ascontiguousarray(r, dtype=np.float32) for r in run]


def _chain_twin(z, dc, bias, run, dtype, train=True):
    """Every output of the two kernels from the torch twin in `dtype`, as float64 arrays."""
    from hgr_net_amd.baseline import cnzsl
    zt = torch.from_numpy(z).to(dtype).requires_grad_(train)
    bt = torch.from_numpy(bias).to(dtype).requires_grad_(train)
    c, a, stats, new = cnzsl.std_chain_host(zt, bt, tuple(torch.from_numpy(r).to(dtype) for r in run), train)
    out = {"c": c, "a": a}
    if train:
        dz, db = torch.autograd.grad(c, [zt, bt], torch.from_numpy(dc).to(dtype))
        out.update(stats=stats, dz=dz, dbias=db, **{f"run{i}": r for i, r in enumerate(new)})
    return {k: v.detach().double().numpy() for k, v in out.items()}


def _chain_errs(got: dict, want: dict) -> dict:
    absdz = np.abs(want["dz"]).sum(0).max() if "dz" in want else None
    return {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / (absdz if k == "dbias" else np.abs(want[k]).max())) for k in want}


def _chain_device(z, dc, bias, run, ld, train=True):
    ops = _ops()
    s, h = z.shape
    zd, dcd = _dev_rows(z, ld), _dev_rows(dc, ld)
    bd = torch.from_numpy(bias).to(DEV)
    rd = [torch.from_numpy(r).to(DEV) for r in run]
    c, a, dz = (_dev_rows(np.zeros((s, h), np.float32), ld) for _ in range(3))
    stats, dbias = torch.zeros((4, h), device=DEV), torch.zeros(h, device=DEV)
    ops.cnzsl_std_chain_fwd(zd, bd, rd, c, a, stats if train else None, train=train)
    out = {"c": c, "a": a}
    if train:
        ops.cnzsl_std_chain_bwd(dcd, a, zd, bd, stats, dz, dbias)
        out.update(stats=stats, dz=dz, dbias=dbias, **{f"run{i}": r for i, r in enumerate(rd)})
    torch.cuda.synchronize()
    for t in (c, a, dz):                                                    # nothing written beyond column H
        assert bool((t._base[:, h:] == 7.0).all()) if ld > h else True
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("s,h,ld", CHAIN_SHAPES)
def test_chain_kernels_against_the_twin(s, h, ld):
    z, dc, bias, run = _chain_inputs(s, h)
    want = _chain_twin(z, dc, bias, run, torch.float64)
    err32 = max(_chain_errs(_chain_twin(z, dc, bias, run, torch.float32), want).values())
    got = _chain_device(z, dc, bias, run, ld)
    errs = _chain_errs(got, want)
    print(f"chain ({s}, {h}) ld {ld}: twin err32 {err32:.3e}, device {max(errs.values()):.3e} at {max(errs, key=errs.get)}; bound {4 * max(err32, FLOOR):.3e}")
    assert max(errs.values()) <= 4 * max(err32, FLOOR), errs
    again = _chain_device(z, dc, bias, run, ld)                              # a second launch on the same inputs: bit-equal
    for k in got:
        assert np.array_equal(got[k], again[k]), k


@pytest.mark.parametrize("s,h,ld", [(1, 16, 16), (64, 40, 52), (3000, 8, 8)])
def test_chain_forward_in_eval_mode(s, h, ld):
    z, dc, bias, run = _chain_inputs(s, h)
    want = _chain_twin(z, dc, bias, run, torch.float64, train=False)
    err32 = max(_chain_errs(_chain_twin(z, dc, bias, run, torch.float32, train=False), want).values())
    ops = _ops()
    zd, bd, rd = _dev_rows(z, ld), torch.from_numpy(bias).to(DEV), [torch.from_numpy(r).to(DEV) for r in run]
    c, a = _dev_rows(np.zeros((s, h), np.float32), ld), _dev_rows(np.zeros((s, h), np.float32), ld)
    ops.cnzsl_std_chain_fwd(zd, bd, rd, c, a, None, train=False)
    c2 = torch.empty((s, h), device=DEV)
    ops.cnzsl_std_chain_fwd(zd, bd, rd, c2, None, None, train=False)        # a is optional here
    errs = _chain_errs({"c": c.cpu().numpy(), "a": a.cpu().numpy()}, want)
    print(f"chain eval ({s}, {h}): twin err32 {err32:.3e}, device {max(errs.values()):.3e}; bound {4 * max(err32, FLOOR):.3e}")
    assert max(errs.values()) <= 4 * max(err32, FLOOR), errs
    assert torch.equal(c2, c) and all(np.array_equal(r.cpu().numpy(), r0) for r, r0 in zip(rd, run))      # the running vectors are read only


def test_chain_constant_column_and_rejected_sizes():
    """u = 0.5 + 0.25 in every row of column 3 (sums of 0.75 are exact in fp32): variance 0, outputs 0, gradients finite."""
    from hgr_net_amd import _lib
    ops = _ops()
    z, dc, bias, run = _chain_inputs(37, 8)
    z[:, 3], bias[3] = 0.5, 0.25
    got = _chain_device(z, dc, bias, run, 8)
    assert got["stats"][0, 3] == 0.75 and got["stats"][1, 3] == 0.0 and got["stats"][2, 3] == 0.0 and got["stats"][3, 3] == 0.0
    assert not got["a"][:, 3].any() and not got["c"][:, 3].any()
    assert all(np.isfinite(v).all() for v in got.values()) and not got["dz"][:, 3].any()
    want = _chain_twin(z, dc, bias, run, torch.float64)
    err32 = max(_chain_errs(_chain_twin(z, dc, bias, run, torch.float32), want).values())
    assert max(_chain_errs(got, want).values()) <= 4 * max(err32, FLOOR)
    # S = 1 in training mode: rejected before any launch - nothing is written
    zd, bd = torch.ones((1, 8), device=DEV), torch.zeros(8, device=DEV)
    rd = [torch.full((8,), 3.0, device=DEV) for _ in range(4)]
    c, a, stats = torch.full((1, 8), 7.0, device=DEV), torch.full((1, 8), 7.0, device=DEV), torch.full((4, 8), 7.0, device=DEV)
    with pytest.raises(_lib.HgrError, match="S=1"):
        ops.cnzsl_std_chain_fwd(zd, bd, rd, c, a, stats, train=True)
    with pytest.raises(_lib.HgrError, match="S=1"):
        ops.cnzsl_std_chain_bwd(zd, a, zd, bd, stats, torch.empty((1, 8), device=DEV), torch.empty(8, device=DEV))
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and bool((a == 7.0).all()) and bool((stats == 7.0).all()) and all(bool((r == 3.0).all()) for r in rd)
    with pytest.raises(_lib.HgrError, match="multiple of 4"):
        ops.cnzsl_std_chain_fwd(torch.ones((4, 6), device=DEV), torch.zeros(6, device=DEV), [torch.ones(6, device=DEV)] * 4, torch.empty((4, 6), device=DEV),
                                torch.empty((4, 6), device=DEV), torch.empty((4, 6), device=DEV))


@pytest.mark.parametrize("rows,c,ld", [(5, 8, 8), (300, 40, 44), (1000, 96, 96)])
def test_bias_relu_pair(rows, c, ld):
    """y = relu(x + b): one rounded addition, equal to torch's bit for bit; dx = dy [y > 0] exact; db within the summation bound
    (rows - 1) 2^-24 sum|dx| of an fp32 sum in any order, against the fp64 sum."""
    from hgr_net_amd.baseline import cnzsl
    ops = _ops()
    x, dy = cnzsl.synth_rows(8, f"relu.x.{rows}", rows, c), cnzsl.synth_rows(8, f"relu.dy.{rows}", rows, c)
    b = cnzsl.synth_rows(8, f"relu.b.{rows}", 1, c)[0].copy()
    want_y = np.maximum(x + b, np.float32(0))
    xd, bd = _dev_rows(x, ld), torch.from_numpy(b).to(DEV)
    y = ops.bias_relu_f32(xd, bd, _dev_rows(np.zeros_like(x), ld))
    assert np.array_equal(y.cpu().numpy(), want_y) and bool((y._base[:, c:] == 7.0).all())
    ops.bias_relu_f32(xd, bd)                                               # in place
    assert np.array_equal(xd.cpu().numpy(), want_y)
    want_dx = np.where(want_y > 0, dy, np.float32(0))
    dyd, db = _dev_rows(dy, ld), torch.zeros(c, device=DEV)
    scratch = torch.empty(-(-rows // ops.RELU_BWD_CHUNK) * c, device=DEV)
    dx = ops.relu_bwd_colsum_f32(dyd, y, _dev_rows(np.zeros_like(x), ld), db, scratch)
    assert np.array_equal(dx.cpu().numpy(), want_dx) and bool((dx._base[:, c:] == 7.0).all())
    bound = (rows - 1) * 2.0 ** -24 * np.abs(want_dx.astype(np.float64)).sum(0)
    assert (np.abs(db.cpu().numpy().astype(np.float64) - want_dx.astype(np.float64).sum(0)) <= bound).all()
    db2 = torch.zeros(c, device=DEV)
    ops.relu_bwd_colsum_f32(dyd, y, dyd, db2, scratch)                      # in place, and the same sums again
    assert np.array_equal(dyd.cpu().numpy(), want_dx) and torch.equal(db, db2)


# ---- the trainer on the training fixture ------------------------------------------------------------------------------------------------
def _model(fx_sd: dict, a: int, h: int, p: int, **kw):
    from hgr_net_amd.baseline import cnzsl
    model = cnzsl.CNZSLModel(a, h, p, device=DEV, **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fx_sd.items()})
    return model


def _run_trainer(fx, steps=STEPS):
    from hgr_net_amd.baseline import cnzsl
    model = _model(fx.sd0, fx.A, fx.H, fx.P)
    tr = cnzsl.CNZSLTrainer(model, lr=fx.lr, weight_decay=fx.wd)
    attrs = torch.from_numpy(fx.attrs).to(DEV)
    losses = [tr.step(torch.from_numpy(fx.feats[i]).to(DEV), torch.from_numpy(fx.labels[i]).to(DEV), attrs) for i in range(steps)]
    return model, tr, losses


def test_trainer_reproduces_the_reference():
    from hgr_net_amd.baseline import cnzsl
    fx = train_fixture()
    model = _model(fx.sd0, fx.A, fx.H, fx.P)
    tr = cnzsl.CNZSLTrainer(model, lr=fx.lr, weight_decay=fx.wd)
    attrs = torch.from_numpy(fx.attrs).to(DEV)
    grads = tr.grads(torch.from_numpy(fx.feats[0]).to(DEV), torch.from_numpy(fx.labels[0]).to(DEV), attrs)
    assert list(grads) == list(cnzsl.TRAINABLE)
    for k, g in grads.items():
        err = grad_err(k, g.cpu().numpy(), fx.z["grad1_64_" + k], float(fx.z["absdz64"]))
        print(f"{k}: gradient error {err:.3e} (bound {fx.grad_tol:.3e})")
        assert err <= fx.grad_tol, (k, err)
    for k in cnzsl.RUNNING:                                                  # grads() leaves the state where it was
        assert np.array_equal(model.state_dict()[k].cpu().numpy(), fx.sd0[k]), k
    model, tr, losses = _run_trainer(fx)
    assert all(l.is_cuda and l.dim() == 0 for l in losses) and tr.t == STEPS
    for i, l in enumerate(losses):
        err = abs(float(l) / fx.z["losses64"][i] - 1)
        print(f"loss {i}: {float(l):.6f}, error {err:.3e}")
        assert err <= fx.grad_tol, (i, err)
    assert rel_err(tr.logits.cpu().numpy(), fx.z["logits64"][STEPS - 1]) <= fx.grad_tol
    check_state(fx, {k: v.cpu().numpy() for k, v in model.state_dict().items()})
    again, _, losses2 = _run_trainer(fx)                                     # from the same state: bit-equal
    for k, v in model.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))


@pytest.mark.parametrize("cn,init", [(False, True), (True, False)])
def test_trainer_switches_against_the_twin(cn, init):
    """`--cn False` (both standardisations are identities) and `--init False` (nn.Linear's own initialisation of the last layer): one
    step against the fp64 twin from the same state.  The bound is the fixture's rule measured for THIS configuration - the twin in fp32
    against the twin in fp64, 4 x the largest error over the tensors - because the conditioning is the configuration's: without the
    standardisations the prototypes are dominated by the last layer's bias, every row points almost the same way, and the backward of
    the row normalisation subtracts nearly equal vectors (the fp32 twin itself is 4.7e-6 off on 'model.6.bias' there, 2e-7 .. 4e-7 on
    every tensor with the standardisations in)."""
    from hgr_net_amd.baseline import cnzsl
    fx = train_fixture()
    torch.manual_seed(3)
    model = cnzsl.CNZSLModel(fx.A, fx.H, fx.P, cn=cn, init=init, device="cpu")
    with torch.no_grad():
        model.model[6].bias.uniform_(0.05, 0.1)                              # positive, like the fixture's: few dead prototype columns
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    assert ("model.3.running_mean" in sd) == cn
    twin = cnzsl.train_state_host(sd, torch.float64)
    loss64, g64, logits64 = cnzsl.train_step_host(twin, fx.feats[0], fx.labels[0], fx.attrs, cn=cn, lr=fx.lr, weight_decay=fx.wd)
    _, g32, _ = cnzsl.train_step_host(cnzsl.train_state_host(sd, torch.float32), fx.feats[0], fx.labels[0], fx.attrs, cn=cn, update=False)
    tol = 4 * max(grad_err(k, g32[k].numpy(), g64[k].numpy(), twin["absdz"], cn) for k in g64)
    model = model.to(DEV)
    tr = cnzsl.CNZSLTrainer(model, lr=fx.lr, weight_decay=fx.wd)
    args = (torch.from_numpy(fx.feats[0]).to(DEV), torch.from_numpy(fx.labels[0]).to(DEV), torch.from_numpy(fx.attrs).to(DEV))
    grads = tr.grads(*args)
    for k, g in grads.items():
        err = grad_err(k, g.cpu().numpy(), g64[k].numpy(), twin["absdz"], cn)
        print(f"cn={cn} init={init} {k}: gradient error {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (k, err)
    loss = tr.step(*args)
    assert abs(float(loss) / float(loss64) - 1) <= tol and rel_err(tr.logits.cpu().numpy(), logits64.numpy()) <= tol
    for k in cnzsl.TRAINABLE:                                                # the first Adam step moves an element by lr, towards -sign(g + wd p)
        if cn and k == "model.2.bias":                                       # a gradient of rounding noise: no element's sign is certain
            continue
        moved = (model.state_dict()[k].cpu().numpy().astype(np.float64) - sd[k]) / fx.lr
        want = (twin["sd"][k].numpy() - sd[k]) / fx.lr
        sure = np.abs(g64[k].numpy() + fx.wd * sd[k]) >= 100 * tol * np.abs(g64[k].numpy() + fx.wd * sd[k]).max()
        assert np.abs(moved - want)[sure].max() <= 2 * 0.01 + 1e-3, k     # + fp32 rounding of p - lr: 2^-24 |p| / lr
    if cn:
        for k in cnzsl.RUNNING:
            assert rel_err(model.state_dict()[k].cpu().numpy(), twin["sd"][k].numpy()) <= tol, k


# ---- the evaluator on the evaluation fixture ------------------------------------------------------------------------------------------------
def test_evaluator_reproduces_the_reference():
    from hgr_net_amd.baseline import cnzsl
    fx = eval_fixture()
    model = _model(fx.sd, fx.A, fx.H, fx.P).eval()
    attrs, feats = torch.from_numpy(fx.attrs).to(DEV), torch.from_numpy(fx.feats).to(DEV)
    ev = cnzsl.CNZSLEvaluator(fx.edges, fx.nodes, fx.test_index, model, attrs)
    bound = 4 * fx.err32
    acc, worst, filler = np.zeros(9), 0.0, 0
    for i in range(len(fx.counts)):
        o, e, t = int(fx.offsets[i]), int(fx.offsets[i + 1]), int(fx.test_index[i])
        logits = ev.logits(feats[o:e]).cpu().numpy()
        worst = max(worst, float(np.abs(logits.astype(np.float64) - fx.z["logits"][o:e]).max() / np.abs(fx.z["logits"]).max()))
        pred, top1, lv = ev.add(feats[o:e], t)
        want = cnzsl.score_host(logits, t, fx.tree, fx.test_index)           # the device's own logits read back: integers, exact
        assert np.array_equal(pred.cpu().numpy(), want["pred"]) and np.array_equal(top1.cpu().numpy().reshape(-1), want["top1"]), i
        for q in fx.tree.path(t):                                           # every level the reference looks at, filler wins included
            d = fx.tree.depth[q]
            on = fx.test_index[fx.tree.depth[fx.test_index] == d]
            lost = logits[:, on].max(1) < -1.0
            filler += int(lost.sum())
        assert np.array_equal(lv.cpu().numpy(), want["lv"]), i
        acc += want["acc"]
    print(f"device logits vs the recorded ones: {worst:.3e} (bound {bound:.3e}); filler wins {filler}")
    assert worst <= bound and filler >= 1
    got = ev.counters()
    assert np.array_equal(got[[0, 1, 2, 3, 4, 5, 8]], acc[[0, 1, 2, 3, 4, 5, 8]]) and np.abs(got - acc).max() < 1e-9
    assert ev.result() == cnzsl.metric_string(acc)
    print("final line equals the reference's:", ev.result() == "\n" + fx.lines[-1])
    # the model's own forward gives the same logits
    whole = model(feats, attrs).cpu().numpy()
    assert float(np.abs(whole.astype(np.float64) - fx.z["logits"]).max() / np.abs(fx.z["logits"]).max()) <= bound
    # rows of mixed classes count like the same rows class by class
    rows = cnzsl.CNZSLEvaluator(fx.edges, fx.nodes, fx.test_index, model, attrs, tree=fx.tree)
    tg = torch.from_numpy(np.repeat(fx.test_index[:len(fx.counts)], fx.counts)).to(DEV)
    rows.add_rows(feats, tg)
    mixed = rows.counters()
    assert np.array_equal(mixed[[0, 1, 2, 3, 4, 5, 8]], got[[0, 1, 2, 3, 4, 5, 8]]) and np.abs(mixed - got).max() < 1e-9


def test_command_line_end_to_end(capsys):
    from hgr_net_amd.baseline import train_cnzsl
    out = train_cnzsl.main(["--synthetic", "500", "--epoch", "2", "--print_freq", "25"])
    text = capsys.readouterr().out
    losses = [float(m) for m in re.findall(r"^loss: (\d+\.\d\d)$", text, re.M)]
    assert text.count("epoch:") == 2 and len(losses) == 2 * 5 and all(np.isfinite(losses))
    assert "End of testing." in text and out in text
    m = re.fullmatch(r"\nTop@1\(%\):(\d+\.\d\d), Top@2\(%\):\d+\.\d\d, Top@5\(%\):\d+\.\d\d, Top@10\(%\):\d+\.\d\d, Top@20\(%\):(\d+\.\d\d)\. "
                     r"hit_ratio\(%\):\d+\.\d\d path_ratio\(%\):\d+\.\d\d point_ratio\(%\):\d+\.\d\d", out)
    assert m and float(m.group(1)) <= float(m.group(2)) <= 100.0
