"""GPU: DGP training - hgr_csr_group_att_grad and the adjoint gather against the fp64 dense oracle on a skewed graph, the trainer
against the reference's own training run (tests/golden/dgp_train_small.npz), hgr_adam_l2 against torch.optim.Adam, the
counter-based dropout against its host twin and the fp64 oracle under the same masks, and a short end-to-end run.

Tolerances are measured, not chosen: for each compared quantity the yardstick is the error of a plain fp32 torch-CPU restatement
(tests/test_dgp_train_host.py, dtype=torch.float32) against the fp64 oracle on the same inputs, relative to the largest magnitude of
the compared tensor; the device, which adds in another order, gets MARGIN = 4 times that."""
import functools

import numpy as np
import pytest
import torch

from oracle import dgp_ref
from test_dgp_train_host import MARGIN, NAMES, dense_sides, fixture, grad_tol, oracle_train, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- measured yardsticks (fp32 torch CPU against fp64, relative to the tensor's largest magnitude) ----------------------------
# skewed graph of test (a), worst over c in {64, 1028}, both sides, both modes
P_ERR = 1.3e-7       # rows of the attention gradient, P[i, d]
DA_ERR = 3.7e-7      # da = colsum(P): n = 1 500 terms per group
T_ERR = 6.5e-7       # adjoint gather
# the training losses, relative: worst over the three epochs of the fixture run and the dropout step of test (e); about one fp32
# ulp of a loss near 1
LOSS_ERR = 6.7e-8
# hgr_adam_l2 inputs of test (c): parameter change after 3 steps, relative to the largest change
ADAM_ERR = 9.3e-5
# fixture, parameters after 3 epochs on the compared elements, absolute (a parameter moves by about lr = 1e-3 per epoch)
STATE_ERR = 7.8e-8
# "d40,d" on the fixture graph with the masks of seed 5, step 1: gradients (attention logits; weights and biases).  The attention
# gradient a o (da - a . da) cancels (max |datt| = 0.008 of the da it is made of), so its fp32 error depends on the order of the sums:
# over the natural channel order and 9 seeded permutations of the channels of every layer (the same mathematics, other fp32 sums) the
# restatement's error ran from 1.2e-7 to 1.5e-6 for r_att (natural order 1.8e-7, a_att 1.5e-7 ... 3.7e-7).  The yardstick is the worst
# of the ten; one order alone is a lucky or unlucky draw.  Weights and biases: natural order.
DROP_GRAD_ERR_ATT, DROP_GRAD_ERR_W = 1.5e-6, 2.4e-7
# ... and the parameters after that one step on the compared elements, absolute
DROP_STATE_ERR = 1.5e-8


def theta(name):
    """Adam divides by |g|: an element is compared where the fixture's coupled gradient stayed above 100 x the gradient tolerance."""
    return 100 * grad_tol(name)


@functools.lru_cache(maxsize=None)
def skewed():
    """The graph of test_dgp.test_skewed_graph_split_rows_match_oracle: split rows on the descendant side, empty groups."""
    from hgr_net_amd import synth
    from hgr_net_amd.baseline import dgp
    dag = synth.make_dag(1500, 9, seed=4, multi_parent=0.05)
    names = ["fall11"] + sorted({w for e in dag for w in e} - {"fall11"})
    idx = {w: i for i, w in enumerate(names)}
    n = len(names)
    es = dgp.fold_groups(dgp.group_edges(n, [(idx[p], idx[ch]) for p, ch in dag]), 4)
    return n, es, dense_sides(n, es)


def att_grad_case(n, d, c):
    """Inputs of test (a) and its fp64 truth per side and mode; shared by the test and by the yardstick measurement."""
    rng = np.random.default_rng(c)
    s, g = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((n, c)).astype(np.float32)
    y = rng.standard_normal((n, c)).astype(np.float32)
    y[rng.random((n, c)) < 0.01] = 0.0                                  # at 0 the slope applies
    bias = rng.standard_normal(c).astype(np.float32)
    att = dgp_ref.softmax(rng.standard_normal(d).astype(np.float32))
    return tuple(torch.from_numpy(a) for a in (s, g, y, bias, att))


def att_grad_truth(side, s, g, y, bias, att, leaky, dtype=torch.float64):
    s, g, bias, att = s.to(dtype), g.to(dtype), bias.to(dtype), att.to(dtype)
    d_o = g * torch.where(y > 0, 1.0, 0.2).to(dtype) if leaky else g
    p = torch.stack([(d_o * (a.to(dtype) @ (s + bias))).sum(1) for a in side], dim=1)
    t = sum(att[d] * (a.to(dtype).t() @ d_o) for d, a in enumerate(side))
    return d_o, p, p.sum(0), t


@pytest.mark.parametrize("c", [64, 1028])
def test_att_grad_and_adjoint_gather_match_oracle(c):
    from hgr_net_amd import ops
    from hgr_net_amd.baseline import GraphOperator
    n, es, sides = skewed()
    s, g, y, bias, att = att_grad_case(n, len(es), c)
    sd, gd, yd, bd, ad = (t.to(DEV) for t in (s, g, y, bias, att))
    for transpose in (False, True):
        op = GraphOperator(n, es, transpose=transpose, device=DEV)
        adj = op.adjoint()
        assert (op.n_slots > 0) == transpose and (adj.n_slots > 0) == (not transpose)       # each side's skew, and its adjoint's
        for leaky in (True, False):
            want_do, want_p, want_da, want_t = att_grad_truth(sides[int(transpose)], s, g, y, bias, att, leaky)
            runs = []
            for _ in range(2):
                p = torch.full((n, op.D), float("nan"), device=DEV)
                d_o = torch.full((n, c), float("nan"), device=DEV) if leaky else None
                ops.csr_group_att_grad(sd, op, bd, gd, yd if leaky else None, d_o, p, 0.2)
                d_o = d_o if leaky else gd
                da = ops.colsum(p, torch.empty(op.D, device=DEV), torch.empty(((n + 511) // 512) * op.D, device=DEV), accumulate=False)
                t = adj.aggregate(d_o, ad, None, torch.full((n, c), float("nan"), device=DEV), 1.0, False)
                runs.append((d_o, p, da, t))
            for a, b in zip(*runs):
                assert torch.equal(a, b)                                                     # deterministic: no atomics
            d_o, p, da, t = (v.cpu() for v in runs[0])
            assert torch.equal(d_o, want_do.float())                                         # one fp32 product: exact
            errs = {"P": rel_err(p, want_p), "da": rel_err(da, want_da), "T": rel_err(t, want_t)}
            print(c, transpose, leaky, errs)
            assert errs["P"] < MARGIN * P_ERR and errs["da"] < MARGIN * DA_ERR and errs["T"] < MARGIN * T_ERR, (transpose, leaky, errs)


def _model(hidden, t):
    from hgr_net_amd.baseline import GCN_Dense_Att
    z, _, es = fixture()
    m = GCN_Dense_Att(len(z["wnids"]), es, z["x"].shape[1], z["out"].shape[1], hidden, device=DEV)
    m.load_state_dict({k: torch.from_numpy(t["sd0_" + k]) for k in NAMES})
    return m


@functools.lru_cache(maxsize=None)
def fixture_run():
    """Three epochs of the trainer on the fixture: (gradients of epoch 1, the three losses, the state dict after epoch 3)."""
    from hgr_net_amd.baseline import DGPTrainer
    z, t, _ = fixture()
    m = _model(str(int(t["hidden"])), t)
    tr = DGPTrainer(m, lr=float(t["lr"]), weight_decay=float(t["weight_decay"]))
    x, rows, targets = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(t["rows"]), torch.from_numpy(t["targets"]).to(DEV)
    grads = {k: v.cpu() for k, v in tr.grads(x, rows, targets).items()}
    losses = [tr.step(x, rows, targets) for _ in range(3)]
    assert all(l.is_cuda and l.dim() == 0 for l in losses)
    return grads, [float(l) for l in losses], {k: v.detach().cpu() for k, v in m.state_dict().items()}


def test_fixture_gradients_and_losses():
    _, t, _ = fixture()
    grads, losses, _ = fixture_run()
    assert set(grads) == set(NAMES)
    for k in NAMES:
        err = rel_err(grads[k], t["grad1_" + k])
        print(k, err)
        assert err < grad_tol(k), (k, err)
    err = np.abs(np.array(losses) / t["losses"] - 1).max()
    print("losses", losses, err)
    assert err < MARGIN * LOSS_ERR


def _adam_case():
    rng = np.random.default_rng(12)
    n = 4099
    p = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) * 1e-2 for _ in range(3)]
    # gradients near and below eps = 1e-8 (the decay term wd * p must be that small too), exact zeros, a sign change
    p[:600] *= 1e-6
    for i, g in enumerate(gs):
        g[:100] = 0.0
        g[100:300] *= 1e-6
        g[300:500] *= 1e-7
        g[500:600] *= 1e-5 * (-1) ** i
    return p, gs


def test_adam_l2_matches_torch_adam():
    from hgr_net_amd import ops
    p0, gs = _adam_case()
    lr, wd = 1e-3, 5e-4
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=lr, weight_decay=wd)
    p = torch.from_numpy(p0.copy()).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    gen = ops.WEIGHTS_GEN[0]
    for step, g in enumerate(gs, 1):
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        ops.adam_l2(p, torch.from_numpy(g).to(DEV), m, v, lr, step, wd=wd)
    assert ops.WEIGHTS_GEN[0] == gen + 3
    err = rel_err(p.cpu() - torch.from_numpy(p0), ref.detach() - torch.from_numpy(p0))
    print("adam", err)
    assert err < MARGIN * ADAM_ERR


def test_fixture_state_after_three_epochs():
    _, t, _ = fixture()
    _, _, sd = fixture_run()
    for k in NAMES:
        keep = torch.from_numpy(t["gmin_" + k] >= theta(k))
        assert keep.float().mean() >= 0.98, k
        err = float((sd[k] - torch.from_numpy(t["sd3_" + k]))[keep].abs().max())
        print(k, err, float(keep.float().mean()))
        assert err < MARGIN * STATE_ERR, (k, err)


def test_dropout_mask_equals_host_twin():
    from hgr_net_amd import ops
    from hgr_net_amd.baseline import dropout_keep
    rows, c = 157, 40
    keep = torch.from_numpy(dropout_keep(2 ** 31 + 7, 3, 1, rows, c))
    x = torch.randn(rows, c, device=DEV)
    y = ops.dropout_counter(x, torch.empty_like(x), 2 ** 31 + 7, 3, 1)
    assert torch.equal(y.cpu(), x.cpu() * keep * 2)
    # strided operands with an offset: the mask depends on (row, column) alone
    wide_x, wide_y = torch.randn(rows, 3 * c, device=DEV), torch.full((rows, 2 * c + 8), 7.0, device=DEV)
    xs, ys = wide_x[:, c:2 * c], wide_y[:, 8:8 + c]
    ops.dropout_counter(xs, ys, 2 ** 31 + 7, 3, 1)
    assert torch.equal(ys.cpu(), xs.cpu() * keep * 2)
    assert bool((wide_y[:, :8] == 7.0).all()) and bool((wide_y[:, 8 + c:] == 7.0).all())
    ops.dropout_counter(xs, xs, 2 ** 31 + 7, 3, 1)                    # in place, as the backward uses it
    assert torch.equal(xs, ys)


def drop_masks(seed, step, n, dims):
    from hgr_net_amd.baseline import dropout_keep
    return {k: dropout_keep(seed, step, k, n, c) for k, c in enumerate(dims)}


def test_step_with_dropout_matches_oracle_under_the_same_masks():
    from hgr_net_amd.baseline import DGPTrainer
    z, t, es = fixture()
    n, seed = len(z["wnids"]), 5
    m = _model("d40,d", t)
    tr = DGPTrainer(m, seed=seed)
    x, rows, targets = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(t["rows"]), torch.from_numpy(t["targets"]).to(DEV)
    sd0 = {k: t["sd0_" + k] for k in NAMES}
    masks = lambda step: drop_masks(seed, step, n, (z["x"].shape[1], int(t["hidden"])))
    losses, grads, sd = oracle_train(z["x"], dense_sides(n, es), sd0, t["rows"], t["targets"], 1, masks_of_step=masks)
    got = tr.grads(x, rows, targets)
    for k in NAMES:
        err = rel_err(got[k].cpu(), grads[0][k])
        print(k, err)
        assert err < MARGIN * (DROP_GRAD_ERR_ATT if k.endswith("_att") else DROP_GRAD_ERR_W), (k, err)
    loss = float(tr.step(x, rows, targets))
    assert abs(loss / losses[0] - 1) < MARGIN * LOSS_ERR
    for k, p in m.state_dict().items():
        g = (grads[0][k] + 5e-4 * torch.from_numpy(sd0[k]).double()).abs()
        keep = g >= 100 * MARGIN * (DROP_GRAD_ERR_ATT if k.endswith("_att") else DROP_GRAD_ERR_W) * g.max()
        assert keep.float().mean() >= 0.98, k
        err = float((p.cpu().double() - sd[k])[keep].abs().max())
        print(k, err)
        assert err < MARGIN * DROP_STATE_ERR, (k, err)


def test_end_to_end_training_lowers_the_loss_and_is_reproducible():
    from hgr_net_amd.baseline import DGPTrainer
    z, t, _ = fixture()
    x, rows, targets = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(t["rows"]), torch.from_numpy(t["targets"]).to(DEV)
    finals = []
    for _ in range(2):
        m = _model("d40,d", t)
        tr = DGPTrainer(m, seed=3)
        before, _ = tr.losses(x, rows, targets)
        for _ in range(20):
            tr.step(x, rows, targets)
        after, val = tr.losses(x, rows, targets)
        assert after < before and val == 0.0, (before, after)
        finals.append({k: v.clone() for k, v in m.state_dict().items()})
    for k in NAMES:
        assert torch.equal(finals[0][k], finals[1][k]), k                # bit-equal from the same seed
    with pytest.raises(NotImplementedError):
        m.train()(x)
    with pytest.raises(ValueError, match="distinct"):
        tr.step(x, torch.tensor([1, 2, 1]), targets[:3])


# ---- wide rows: three and four float4 slices per thread (2 048 < C <= 4 096) ------------------------------------------------
# fixture graph, c in {3076, 4096}, both sides, LeakyReLU mode; the loss head on the same rows.  Measured like the constants above.
# The head's loss is one more fp32 loss near 1 and shares LOSS_ERR; dL/dO is relative to its largest element.
WIDE_P_ERR, WIDE_DA_ERR, WIDE_T_ERR = 1.6e-7, 3.7e-7, 2.4e-7
WIDE_HEAD_DO_ERR = 4.3e-7


def head_truth(o, rows, f, dtype=torch.float64):
    """Loss and dL/dO of the loss head, restated."""
    o, f = o.to(dtype), f.to(dtype)
    nrm = o.norm(dim=1, keepdim=True).clamp_min(1e-12)
    y = o / nrm
    g = torch.zeros_like(y)
    g[rows] = (y[rows] - f) / len(rows)
    return ((y[rows] - f) ** 2).sum() / (2 * len(rows)), (g - y * (y * g).sum(1, keepdim=True)) / nrm


@pytest.mark.parametrize("c", [3076, 4096])
def test_wide_rows_match_oracle(c):
    from hgr_net_amd import ops
    from hgr_net_amd.baseline import GraphOperator
    z, t, es = fixture()
    n = len(z["wnids"])
    sides = dense_sides(n, es)
    s, g, y, bias, att = att_grad_case(n, len(es), c)
    sd, gd, yd, bd, ad = (v.to(DEV) for v in (s, g, y, bias, att))
    for transpose in (False, True):
        op = GraphOperator(n, es, transpose=transpose, device=DEV)
        want_do, want_p, want_da, want_t = att_grad_truth(sides[int(transpose)], s, g, y, bias, att, True)
        p, d_o = torch.full((n, op.D), float("nan"), device=DEV), torch.full((n, c), float("nan"), device=DEV)
        ops.csr_group_att_grad(sd, op, bd, gd, yd, d_o, p, 0.2)
        da = ops.colsum(p, torch.empty(op.D, device=DEV), torch.empty(op.D, device=DEV), accumulate=False)
        tt = op.adjoint().aggregate(d_o, ad, None, torch.full((n, c), float("nan"), device=DEV), 1.0, False)
        assert torch.equal(d_o.cpu(), want_do.float())
        errs = {"P": rel_err(p.cpu(), want_p), "da": rel_err(da.cpu(), want_da), "T": rel_err(tt.cpu(), want_t)}
        print(c, transpose, errs)
        assert errs["P"] < MARGIN * WIDE_P_ERR and errs["da"] < MARGIN * WIDE_DA_ERR and errs["T"] < MARGIN * WIDE_T_ERR, (transpose, errs)
    rows = torch.from_numpy(t["rows"].astype(np.int64))
    f = torch.nn.functional.normalize(g[:len(rows)])
    want_loss, want_do = head_truth(s, rows, f)
    loss, d_o = torch.empty(1, device=DEV), torch.full((n, c), float("nan"), device=DEV)
    ops.dgp_loss_head(sd, rows.to(torch.int32).to(DEV), f.to(DEV), torch.empty(len(rows), device=DEV), loss, d_o)
    errs = {"loss": abs(float(loss) / float(want_loss) - 1), "dO": rel_err(d_o.cpu(), want_do)}
    print(c, errs)
    assert errs["loss"] < MARGIN * LOSS_ERR and errs["dO"] < MARGIN * WIDE_HEAD_DO_ERR, errs
