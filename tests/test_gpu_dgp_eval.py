"""GPU: the DGP scoring - hgr_dgp_score_rows against its numpy twin (exact integers) on shapes that take every path of the kernel
and on planted ties, the evaluator against the reference's own `test_on_subset` run (tests/golden/dgp_eval_small.npz) through both
routes, the classifier product against fp64, and the two command lines."""
import json

import numpy as np
import pytest
import torch

from test_dgp_eval_host import INT_COLS, SUM_COLS, check_against_reference, class_rows, fixture

from hgr_net_amd.baseline import dgp_eval, evaluate_dgp

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL16 = float(np.float16(dgp_eval.FILL))


def make_case(rows, n_cols, n_levels, n_masked, dtype, seed):
    """A table full of ties (values on a 1/4 grid) with the edge values planted, a depth map with one empty level, per-row targets
    of which some are masked."""
    rng = np.random.default_rng(seed)
    t = (rng.integers(-12, 13, (rows, n_cols)) * 0.25).astype(dtype)
    empty = n_levels // 2 if n_levels > 1 else -1
    levels = [l for l in range(n_levels) if l != empty]
    depth = np.array(levels, np.int32)[rng.integers(0, len(levels), n_cols)]
    targets = rng.integers(0, n_cols, rows).astype(np.int64)
    if n_masked and rows > 1:
        targets[0] = rng.integers(0, n_masked)                         # a masked target ...
        if n_masked < n_cols:
            targets[1] = rng.integers(n_masked, n_cols)                # ... and an unmasked one
    for r in range(rows):
        kind = r % 8
        c = rng.integers(0, n_cols, min(n_cols, 6))
        if kind == 0:                                                  # the target's score in j other columns
            t[r, c] = t[r, targets[r]]
        elif kind == 1:                                                # -0.0 beside +0.0, around the target's own 0
            t[r, c] = np.array([0.0, -0.0] * 3, dtype)[:len(c)]
            t[r, targets[r]] = -0.0
        elif kind == 2:                                                # a stored 2^-23 beside the fill
            t[r, c] = FILL16
        elif kind == 3:                                                # a level whose nodes are all below -1
            t[r, depth == depth[c[0]]] = -1.5 - 0.25 * (r % 3)
        elif kind == 4:                                                # a level maximum of exactly -1
            on = depth == depth[c[0]]
            t[r, on] = np.minimum(t[r, on], -1.0)
            t[r, c[0]] = -1.0
        elif kind == 5:
            t[r, c[:3]] = np.inf
            t[r, c[3:]] = -np.inf
    return t, depth, targets


def run_kernel(t, depth, n_levels, n_masked, targets=None, target=0, ld=None, offset=0):
    """The table as a [rows, n_cols] view of a buffer with leading dimension `ld`, starting `offset` elements into it."""
    from hgr_net_amd import ops
    rows, n_cols = t.shape
    ld = n_cols if ld is None else ld
    buf = torch.full((rows * ld + offset + 8,), 99.0, dtype=torch.from_numpy(t[:0]).dtype, device=DEV)       # 99 would win every compare
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :n_cols]
    view.copy_(torch.from_numpy(t))
    tg = None if targets is None else torch.from_numpy(targets).to(DEV)
    rank, top1, lv, pred = ops.dgp_score_rows(view, torch.from_numpy(depth).to(DEV), n_levels, n_masked, dgp_eval.FILL, targets=tg,
                                              target=target, k_pred=dgp_eval.K_PRED)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), top1.cpu().numpy().reshape(-1), lv.cpu().numpy(), pred.cpu().numpy()


def check_case(t, depth, n_levels, n_masked, targets, **kw):
    rank, top1, lv, pred = run_kernel(t, depth, n_levels, n_masked, targets=targets, **kw)
    h_rank, h_top1, h_lv = dgp_eval.score_rows_host(t, depth, n_levels, n_masked, dgp_eval.FILL, targets)
    assert np.array_equal(rank, h_rank) and np.array_equal(top1, h_top1) and np.array_equal(lv, h_lv)
    want = np.where(np.arange(dgp_eval.K_PRED)[None, :] == h_rank[:, None] - 1, targets[:, None], -1)
    assert np.array_equal(pred, want)
    return rank, top1, lv, pred


# rows, n_cols, ld, offset, n_levels, n_masked ("all" = n_cols), dtype: every n_cols / rows / n_levels / n_masked of the issue; row bases
# that are 16-byte aligned (ld 304, 4104; fp32 ld 40), only 2-byte aligned (ld 37, 4099 in fp16; offset 1), both level layouts (<= 16
# and 17 .. 32 levels), more rows than the grid holds (1030 > 1024)
CASES = [
    (1, 1, 1, 0, 1, 0, np.float16),
    (1, 1, 1, 0, 1, "all", np.float32),
    (5, 37, 37, 0, 13, 3, np.float16),
    (5, 37, 40, 0, 32, 0, np.float32),
    (1030, 37, 37, 1, 17, 3, np.float16),
    (5, 300, 304, 0, 17, "all", np.float16),
    (1030, 300, 304, 0, 13, 3, np.float16),
    (5, 300, 304, 0, 1, 0, np.float32),
    (5, 4099, 4099, 0, 32, 3, np.float16),
    (5, 4099, 4104, 0, 13, 0, np.float16),
    (1, 4099, 4100, 0, 17, 3, np.float32),
    (5, 4099, 4099, 3, 32, "all", np.float32),
]


@pytest.mark.parametrize("rows,n_cols,ld,offset,n_levels,n_masked,dtype", CASES)
def test_score_rows_matches_host_twin(rows, n_cols, ld, offset, n_levels, n_masked, dtype):
    nm = n_cols if n_masked == "all" else min(n_masked, n_cols)
    t, depth, targets = make_case(rows, n_cols, n_levels, nm, dtype, seed=rows * 7 + n_cols + n_levels)
    by_row = check_case(t, depth, n_levels, nm, targets, ld=ld, offset=offset)
    # one target for every row gives the rows that per-row copies of it give
    t0 = int(targets[min(1, rows - 1)])
    same = np.full(rows, t0, np.int64)
    a = check_case(t, depth, n_levels, nm, same, ld=ld, offset=offset)
    b = run_kernel(t, depth, n_levels, nm, targets=None, target=t0, ld=ld, offset=offset)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(by_row[1], a[1]) and np.array_equal(by_row[2], a[2])          # top1 and lv do not depend on the target


def test_planted_ties_rank_is_j_plus_one_plus_greater():
    """The target's score copied into j other columns: rank = j + 1 + #greater, whatever the columns' order - top-k membership
    (lowest index first) would give #greater + 1 for a target in front of its copies."""
    n = 300
    depth = np.zeros(n, np.int32)
    t = np.full((4, n), -2.0, np.float16)
    for r, (j, g) in enumerate([(0, 0), (5, 0), (19, 3), (40, 7)]):
        t[r, 10:10 + g] = 3.0
        t[r, 100:100 + j] = 1.0
        t[r, 50] = 1.0
    targets = np.full(4, 50, np.int64)
    rank, _, _, pred = check_case(t, depth, 1, 0, targets, ld=304)
    assert rank.tolist() == [1, 6, 23, 48]
    assert (pred[0] == 50).nonzero()[0].tolist() == [0] and (pred[1] == 50).nonzero()[0].tolist() == [5] and (pred[2:] == 50).sum() == 0
    # -0.0 ties with +0.0, the fill with a stored 2^-23, and masking applies to the target too
    z = np.array([[0.0, -0.0, -0.0, 0.0, FILL16, 1.0, -1.0, FILL16]], np.float16)
    for tg, nm, want in ((1, 0, 7), (0, 0, 7), (4, 0, 3), (4, 2, 5), (0, 2, 5), (6, 8, 8)):
        rank, top1, lv, _ = check_case(z, np.zeros(8, np.int32), 1, nm, np.array([tg], np.int64))
        assert rank.tolist() == [want]
    assert top1.tolist() == [0]                                        # everything masked: the lowest column


def test_bad_arguments_are_refused_before_any_launch():
    from hgr_net_amd import ops
    from hgr_net_amd._lib import HgrError
    t = torch.zeros((2, 8), dtype=torch.float16, device=DEV)
    d = torch.zeros(8, dtype=torch.int32, device=DEV)
    for kw in (dict(n_levels=33), dict(n_levels=1, n_masked=9), dict(n_levels=1, target=8), dict(n_levels=1, target=-1),
               dict(n_levels=1, mask_value=float("nan"))):
        with pytest.raises(HgrError):
            ops.dgp_score_rows(t, d, **kw)
    with pytest.raises(HgrError):
        ops.dgp_score_rows(t.cpu(), d, 1)
    # a per-row target outside the table never hits and reads nothing
    tg = torch.tensor([3, 8], dtype=torch.int64, device=DEV)
    rank, _, _, pred = ops.dgp_score_rows(t, d, 1, targets=tg, k_pred=20)
    assert rank.tolist() == [8, 2 ** 31 - 1] and (pred[1] == -1).all()


# ---- the evaluator against the reference's recorded run -------------------------------------------------------------------------------------
def evaluator(fx, consider_trains, dtype="f16"):
    pred = {"wnids": fx["nodes"][::-1], "pred": torch.from_numpy(fx["pred"][::-1].copy())}       # picked by name, whatever the file's order
    return dgp_eval.DGPEvaluator(fx["edges"], fx["nodes"], fx["n_seen"], pred, consider_trains=consider_trains, dtype=dtype, device=DEV)


@pytest.mark.parametrize("consider_trains", [False, True])
def test_fixture_through_both_routes(consider_trains):
    fx = fixture()
    ref = fx["ref"][int(consider_trains)]
    n, ns = len(fx["nodes"]), fx["n_seen"]
    feat = torch.from_numpy(fx["feat"]).to(DEV)
    ev = evaluator(fx, consider_trains)
    assert torch.equal(ev.table(feat).cpu(), torch.from_numpy(fx["table"]))                       # bit-equal to the exact product
    for i in range(n - ns):
        f = feat[class_rows(fx, i)]
        ev.add(f if i % 2 else f.half(), ns + i)                       # fp32 and fp16 features
    acc = ev.acc.cpu().numpy()
    check_against_reference(acc[ns:-1], ref)
    assert not acc[:ns].any() and not acc[-1].any()
    res = ev.result()
    assert res["results"][fx["nodes"][ns]] == (ref[0, :5] / ref[0, 8]).tolist() and res["tot"] == int(ref[:, 8].sum())
    # all classes packed into batches of 32 rows
    pk = evaluator(fx, consider_trains)
    targets = torch.from_numpy(np.repeat(np.arange(ns, n), fx["feat_count"])).to(DEV)
    for o in range(0, len(feat), 32):
        pk.add_rows(feat[o:o + 32], targets[o:o + 32])
    packed = pk.acc.cpu().numpy()
    assert not packed[:-1].any()
    assert np.array_equal(packed[-1, INT_COLS], ref[:, INT_COLS].sum(0)) and np.abs(packed[-1, SUM_COLS] - ref[:, SUM_COLS].sum(0)).max() <= 1e-9
    assert np.array_equal(packed[-1, INT_COLS], acc[:, INT_COLS].sum(0)) and np.abs(packed[-1, SUM_COLS] - acc[:, SUM_COLS].sum(0)).max() <= 1e-9


def test_random_features_k2048():
    """Random-normal features, K = 2048, 8 rows, 300 columns: the device outputs equal the twin applied to the device's own table, and
    the table is as close to fp64 as a half-precision product can be asked to be: at most 4 x the error of torch.matmul in half on
    the CPU for the same inputs (the yardstick is computed here; the DGP-training tests' convention)."""
    from hgr_net_amd import synth
    n, k, b, ns = 300, 2048, 8, 40
    edges = synth.make_dag(n, 10, seed=3, multi_parent=0.03)
    nodes = sorted({w for e in edges for w in e} - {"fall11"})
    rng = np.random.default_rng(11)
    pred = (rng.standard_normal((n, k + 1)) * 0.05).astype(np.float32)
    feat = rng.standard_normal((b, k)).astype(np.float32)
    targets = rng.integers(0, n, b).astype(np.int64)
    p16, f16 = torch.from_numpy(pred).half(), torch.from_numpy(feat).half()
    exact = torch.cat([f16.double(), torch.ones(b, 1, dtype=torch.float64)], 1) @ p16.double().T
    cpu_half = torch.cat([f16, torch.ones(b, 1, dtype=torch.float16)], 1) @ p16.T
    yard = float((cpu_half.double() - exact).abs().max())
    for dtype in ("f16", "fp32"):
        ev = dgp_eval.DGPEvaluator(edges, nodes, ns, torch.from_numpy(pred), dtype=dtype, device=DEV)
        rank, top1, lv = ev.add_rows(torch.from_numpy(feat).to(DEV), torch.from_numpy(targets).to(DEV))
        tab = ev._buffers(b)["table"][:, :n].cpu()
        err = float((tab.double() - exact).abs().max())
        print(f"{dtype}: table max |err| against fp64 {err:.3e}, torch.matmul in half on the CPU {yard:.3e}")
        assert err <= 4 * yard
        h_rank, h_top1, h_lv = dgp_eval.score_rows_host(tab.numpy(), ev.tree.depth, ev.tree.n_levels, ns, dgp_eval.FILL, targets)
        assert np.array_equal(rank.cpu().numpy(), h_rank) and np.array_equal(top1.cpu().numpy().reshape(-1), h_top1)
        assert np.array_equal(lv.cpu().numpy(), h_lv)
        host = dgp_eval.HostEvaluator(ev.tree, ns)
        host.add_rows(tab.numpy(), targets)
        acc = ev.acc.cpu().numpy()
        assert np.array_equal(acc[-1, INT_COLS], host.acc[-1, INT_COLS]) and np.abs(acc[-1, SUM_COLS] - host.acc[-1, SUM_COLS]).max() <= 1e-9


def test_cpu_features_are_refused():
    from hgr_net_amd._lib import HgrError
    fx = fixture()
    ev = evaluator(fx, False)
    with pytest.raises(HgrError):
        ev.add(torch.from_numpy(fx["feat"][:2]), fx["n_seen"])


# ---- the command lines ------------------------------------------------------------------------------------------------------------------------
def test_cli_synthetic_output_agrees_with_result(tmp_path, capsys):
    out = tmp_path / "res.json"
    res = evaluate_dgp.main(["--synthetic", "200", "--output", str(out), "--batch-size", "4"])
    printed = capsys.readouterr().out.strip().splitlines()
    assert json.load(open(out)) == res["results"] and len(res["results"]) == len(res["per_class"]) > 50
    assert printed[-1] == dgp_eval.summary_line(res["hits"], res["tot"]) and printed[-1].startswith("summary: ")
    assert printed[2:] == res["lines"] and " To:" in printed[2] and printed[2].startswith("1/")
    # the same material driven by hand, in one batch per class
    edges, splits, pred, feats = evaluate_dgp.synthetic_material(200, 0)
    ev = dgp_eval.DGPEvaluator(edges, splits["train"] + splits["rest"], len(splits["train"]), pred, device=DEV)
    for i, w in enumerate(splits["rest"]):
        ev.add(torch.from_numpy(feats[w]).to(DEV), len(splits["train"]) + i)
    mine = ev.result()
    assert mine["results"] == res["results"] and mine["hits"] == res["hits"] and mine["tot"] == res["tot"] == sum(len(v) for v in feats.values())
    assert 0 < mine["hits"][0] < mine["tot"]                           # neither trivial nor hopeless
    # with the seen classifiers in play other columns compete
    other = evaluate_dgp.main(["--synthetic", "200", "--consider-trains"])
    assert other["tot"] == res["tot"] and other["hits"] != res["hits"]


def test_train_dgp_eval_after_prints_a_summary(tmp_path, capsys):
    from hgr_net_amd.baseline import train_dgp
    train_dgp.main(["--synthetic", "300", "--max-epoch", "2", "--eval-after", "--save_path", str(tmp_path / "run")])
    printed = capsys.readouterr().out.strip().splitlines()
    assert printed[-1].startswith("summary: ") and printed[-1].split()[-2] == "total" and int(printed[-1].split()[-1]) > 0
    assert any(" Path:" in line and " Point:" in line for line in printed)
