"""GPU: candidate sets - hgr_set_ranks against a torch restatement of its definition (a stable descending sort of the set's columns in
tie-key order) over the shapes at which its launch and its load path change, heavy ties against hgr_eval_rows, absent targets,
independence of row order and of the cut into launches, hgr_set_counters_rows against a Python restatement, the rejected arguments,
the reference's own logits (tests/golden/tree_*), and the wiring: Evaluator(sets=), evaluate.predict and evaluate.test with
--eval_sets / --eval_sets_report."""
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import _lib, evaluate, ops, synth
from hgr_net_amd.clip.model import build_model
from hgr_net_amd.hierarchy import build_hierarchy
from hgr_net_amd.model import tree_model

DEV = "cuda"
K = max(evaluate.TOPK)
MAXL = ops.REPORT_MAXL
GRID_CAP = 1024                      # hgr_set_ranks: workgroups at the most, the rows behind them are taken in further rounds


# ---- helpers of test_gpu_hedge.py (copied: test modules do not import each other) --------------------------------------------------------
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


def _model(case, golden_dir, tmp_path, test_wnids=None):
    meta, z, cfg, edges = _tree_case(case, golden_dir)
    sd = synth.clip_state_dict(cfg, 0)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], meta["n_train"], meta["n_test"], meta["split_seed"])
    model = tree_model(_opts(tmp_path, edges), splits["all"], splits["rest"] if test_wnids is None else test_wnids,
                       node_tokens=torch.from_numpy(z["node_tokens"].astype(np.int64)), clip_model=build_model(sd).to(DEV))
    with torch.no_grad():
        model.layer_weight.copy_((0.3 * torch.rand(model.layer_weight.shape, generator=torch.Generator().manual_seed(3))).to(DEV))
    return model, meta, cfg, splits, z


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def _ranks_restated(x, member, tie_key, n_sets, targets):
    """(rank, top1) int64 [rows, n_sets] on the CPU: per set a stable descending sort of x[:, its columns in tie-key order] - the
    position of the target's column in it, and its first column.  x + 0.0 makes -0 a +0: the two compare equal."""
    x = x.detach().cpu().float() + 0.0
    rows, n = x.shape
    member, tie_key = np.asarray(member, dtype=np.int64), np.asarray(tie_key, dtype=np.int64)
    rank = torch.full((rows, n_sets), -1, dtype=torch.int64)
    top1 = torch.full((rows, n_sets), -1, dtype=torch.int64)
    for s in range(n_sets):
        cols = np.nonzero((member >> s) & 1)[0]
        if cols.size == 0:
            continue
        cols = cols[np.argsort(tie_key[cols], kind="stable")]
        assert len(set(tie_key[cols].tolist())) == cols.size                           # distinct over the members of the set
        order = torch.sort(x[:, torch.from_numpy(cols)], dim=1, descending=True, stable=True).indices.numpy()
        top1[:, s] = torch.from_numpy(cols[order[:, 0]])
        if targets is None:
            continue
        for r, t in enumerate(targets):
            if 0 <= t < n and (member[t] >> s) & 1:
                rank[r, s] = int(np.nonzero(cols[order[r]] == t)[0][0])
    return rank, top1


def _stand_in(member, tie_key, n_sets):
    """What ops.set_ranks reads of an ops.SetIndex, from plain arrays."""
    member = np.asarray(member, dtype=np.int64)
    return types.SimpleNamespace(n_nodes=len(member), n_sets=n_sets, member=torch.from_numpy(member.astype(np.int32)).to(DEV),
                                 tie_key=torch.from_numpy(np.asarray(tie_key, dtype=np.int32)).to(DEV))


LDS = ("n", "n + 3", "pad 4", "offset view")


def _device_view(x, ld):
    """x [rows, n] on the device with the leading dimension asked for: contiguous, 3 columns wider (rows of every alignment), padded to
    a multiple of 4 (every row takes the 16-byte loads, with a tail when n % 4 != 0), or a view that starts one column into a wider
    buffer (no row does).  The columns outside the view hold +1000: a kernel that reads them shows."""
    rows, n = x.shape
    if ld == "n":
        return x.to(DEV).contiguous()
    width, off = {"n + 3": (n + 3, 0), "pad 4": ((n + 3) // 4 * 4, 0), "offset view": (n + 7, 1)}[ld]
    buf = torch.full((rows, width), 1000.0)
    buf[:, off:off + n] = x
    return buf.to(DEV)[:, off:off + n]


def _ranks(x, member, tie_key, n_sets, targets, ld="n"):
    """One launch: (rank, top1) int64 on the CPU; both buffers start at -7."""
    rows = x.shape[0]
    xd = _device_view(x, ld)
    tg = None if targets is None else torch.tensor(targets, dtype=torch.int64, device=DEV)
    rank = torch.full((rows, n_sets), -7, dtype=torch.int32, device=DEV)
    top1 = torch.full((rows, n_sets), -7, dtype=torch.int32, device=DEV)
    got = ops.set_ranks(xd, _stand_in(member, tie_key, n_sets), tg, rank if tg is not None else None, top1)
    assert got[1] is top1 and (got[0] is rank if tg is not None else got[0] is None)
    return rank.cpu().long(), top1.cpu().long()


def _family(n, n_sets, rng, full):
    """Member words of n_sets sets.  ``full``: set 0 holds every column, set 1 none, set 2 column n - 1 alone, the others are random
    subsets of every density; otherwise random subsets that all leave column n // 2 out.  Bits behind n_sets are set at random: the
    kernel must ignore them."""
    member = np.zeros(n, dtype=np.int64)
    for s in range(n_sets):
        if full and s == 0:
            bits = np.ones(n, dtype=bool)
        elif full and s == 1:
            bits = np.zeros(n, dtype=bool)
        elif full and s == 2:
            bits = np.arange(n) == n - 1
        else:
            bits = rng.random(n) < (0.03, 0.3, 0.6, 0.95)[s % 4]
        member |= bits.astype(np.int64) << s
    if not full:
        member[n // 2] = 0
    junk = rng.integers(0, 1 << 15, n).astype(np.int64) << n_sets
    return (member | junk) & 0x7FFFFFFF


# ---- 1. the ranks against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 4099])
def test_set_ranks_against_the_sort_restatement(n):
    """Every n_sets in (1, 2, 3, 8, 16) - one launch per register layout, 3 on the layout of 4 - and every leading dimension, for 1 and
    3 rows; targets at column 0, at column n - 1, at the column no set holds, -1 and n.  The tie keys are a random permutation."""
    rng = np.random.default_rng(n)
    tie_key = rng.permutation(n) + 5
    gen = torch.Generator().manual_seed(n)
    case = 0
    for n_sets in (1, 2, 3, 8, 16):
        for ld in LDS:
            for rows in (1, 3):
                full = case % 2 == 0
                member = _family(n, n_sets, rng, full)
                x = torch.randn(rows, n, generator=gen)
                kinds = [0, n - 1, n // 2, -1, n, int(rng.integers(0, n))]
                targets = [kinds[(case + i) % len(kinds)] for i in range(rows)] if rows == 3 else [kinds[case % len(kinds)]]
                rank, top1 = _ranks(x, member, tie_key, n_sets, targets, ld)
                want_rank, want_top1 = _ranks_restated(x, member, tie_key, n_sets, targets)
                assert torch.equal(rank, want_rank) and torch.equal(top1, want_top1), (n_sets, ld, rows, targets)
                if full:                                                                 # the full set, the empty one, the singleton
                    assert torch.equal(top1[:, 0], x.argmax(1)) and (n_sets < 2 or bool((top1[:, 1] == -1).all()))
                    assert n_sets < 3 or bool((top1[:, 2] == n - 1).all())
                    assert all(rank[r, 0] >= 0 for r, t in enumerate(targets) if 0 <= t < n)
                    assert n_sets < 3 or all(rank[r, 2] == (0 if t == n - 1 else -1) for r, t in enumerate(targets))
                else:
                    assert all(bool((rank[r] == -1).all()) for r, t in enumerate(targets) if t in (n // 2, -1, n))
                case += 1


def test_set_ranks_large_row_and_more_rows_than_the_grid():
    n = 36865                                                                           # beyond HGR_HEDGE_MAXN: no row is kept on the chip
    rng = np.random.default_rng(1)
    tie_key = rng.permutation(n)
    member = _family(n, 16, rng, True)
    x = torch.randn(2, n, generator=torch.Generator().manual_seed(1))
    for ld, targets in (("n", [n - 1, 17]), ("offset view", [0, n])):
        rank, top1 = _ranks(x, member, tie_key, 16, targets, ld)
        want = _ranks_restated(x, member, tie_key, 16, targets)
        assert torch.equal(rank, want[0]) and torch.equal(top1, want[1])
    assert int(rank[0, 0]) >= 0 and int(rank.max()) > 100
    rows, n = GRID_CAP + 13, 65
    tie_key = rng.permutation(n)
    member = _family(n, 3, rng, False)
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(2))
    targets = rng.integers(-1, n + 1, rows).tolist()
    rank, top1 = _ranks(x, member, tie_key, 3, targets)
    want = _ranks_restated(x, member, tie_key, 3, targets)
    assert torch.equal(rank, want[0]) and torch.equal(top1, want[1])
    assert len(set(rank[GRID_CAP:].view(-1).tolist())) > 3                               # the second round wrote its rows


# ---- 2. heavy ties --------------------------------------------------------------------------------------------------------------------
def test_heavy_ties_agree_with_eval_rows():
    """Scores on a grid of 1/8, a constant row and rows of +-0 alone: the order is decided by the tie keys.  For the set that is the
    index's test subset (SetIndex gives its columns their test positions as keys) rank < 20 holds exactly where the target is inside
    hgr_eval_rows' top-20, and top1 is its first top-k column; every set equals the restatement."""
    n, rows = 300, 24
    rng = np.random.default_rng(4)
    depth = torch.from_numpy(rng.integers(0, 6, n).astype(np.int32)).to(DEV)
    test = torch.from_numpy(rng.permutation(n)[:150].astype(np.int32)).to(DEV)
    ix = ops.EvalIndex(depth, torch.arange(n, dtype=torch.int32, device=DEV), test, 6)
    te = test.cpu().tolist()
    sets = {"test": te, "odd": te[1::2], "all": list(range(n)), "other": sorted(set(range(n)) - set(te))}
    si = ops.SetIndex(ix, sets)
    x = torch.round(torch.randn(rows, n, generator=torch.Generator().manual_seed(4)) * 8) / 8
    x[3] = 0.125
    x[4] = torch.where(torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    x[5] = -x[4]
    x[6] = torch.where(torch.rand(n, generator=torch.Generator().manual_seed(6)) < 0.1, torch.tensor(0.25), x[4])
    assert bool(torch.signbit(x[4]).any()) and not bool(torch.signbit(x[4]).all())
    targets = [te[int(i)] for i in rng.integers(0, 150, rows)]
    targets[3], targets[4], targets[5] = te[0], te[149], te[25]
    xd, tg = x.to(DEV), torch.tensor(targets, dtype=torch.int64, device=DEV)
    rank, top1 = ops.set_ranks(xd, si, tg)
    want = _ranks_restated(x, si.member.cpu().numpy(), si.tie_key.cpu().numpy(), 4, targets)
    assert torch.equal(rank.cpu().long(), want[0]) and torch.equal(top1.cpu().long(), want[1])
    _, _, topk = ops.eval_rows(xd, ix, K)
    in_top = (topk.long() == tg[:, None]).any(1)
    assert torch.equal(rank[:, 0] < K, in_top) and torch.equal(top1[:, 0], topk[:, 0])
    assert 0 < int(in_top.sum()) < rows                                                 # the case decides something, both ways
    assert rank[3].tolist() == [0, -1, si.tie_key[te[0]].item(), -1] and rank[4, 0].item() == 149 and rank[5, 0].item() == 25
    # where the target is inside the top-20, its rank is its place there
    hit = in_top.nonzero().view(-1)
    assert torch.equal(topk[hit].long().gather(1, rank[hit, :1].long()).view(-1), tg[hit])


# ---- 3. targets absent, and independence of the launch ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared():
    """40 rows x 777 columns, 5 sets, a third of the scores tied; the device's (rank, top1) of ONE launch.  Never written."""
    n, rows = 777, 40
    rng = np.random.default_rng(8)
    tie_key = rng.permutation(n)
    member = _family(n, 5, rng, True)
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(8))
    x = torch.where(x.abs() < 0.43, torch.round(x * 4) / 4, x)
    targets = rng.integers(-1, n + 1, rows).tolist()
    rank, top1 = _ranks(x, member, tie_key, 5, targets)
    want = _ranks_restated(x, member, tie_key, 5, targets)
    assert torch.equal(rank, want[0]) and torch.equal(top1, want[1])
    return x, member, tie_key, targets, rank, top1


def test_without_targets_only_top1_is_written(shared):
    x, member, tie_key, targets, rank, top1 = shared
    r2, t2 = _ranks(x, member, tie_key, 5, None)
    assert torch.equal(t2, top1) and bool((r2 == -7).all())                             # ops.set_ranks hands no rank buffer over
    # and a rank buffer that IS handed over without targets stays as it was
    si = _stand_in(member, tie_key, 5)
    xd = x.to(DEV)
    rb = torch.full((40, 5), -7, dtype=torch.int32, device=DEV)
    tb = torch.full((40, 5), -7, dtype=torch.int32, device=DEV)
    _lib.call("hgr_set_ranks", xd.data_ptr(), xd.stride(0), 777, si.member.data_ptr(), si.tie_key.data_ptr(), 5, 0, rb.data_ptr(), tb.data_ptr(),
              40, torch.cuda.current_stream().cuda_stream)
    assert bool((rb == -7).all()) and torch.equal(tb.cpu().long(), top1)


def test_outputs_do_not_depend_on_row_order_or_cut(shared):
    x, member, tie_key, targets, rank, top1 = shared
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(9))
    r2, t2 = _ranks(x[perm], member, tie_key, 5, [targets[i] for i in perm.tolist()])
    assert torch.equal(r2, rank[perm]) and torch.equal(t2, top1[perm])
    for cuts in ([0, 1, 40], [0, 23, 40]):
        parts = [_ranks(x[lo:hi], member, tie_key, 5, targets[lo:hi], ld) for (lo, hi), ld in zip(zip(cuts, cuts[1:]), ("n + 3", "pad 4"))]
        assert torch.equal(torch.cat([p[0] for p in parts]), rank) and torch.equal(torch.cat([p[1] for p in parts]), top1)


# ---- 4. the counters ---------------------------------------------------------------------------------------------------------------------
def _table_restated(rank, top1, targets, lv, ptr, nodes, levels, n, n_levels):
    """hgr_set_counters_rows in Python: int64 [S, 33, SETS_COLS]."""
    S = rank.shape[1]
    tab = np.zeros((S, MAXL + 1, ops.SETS_COLS), dtype=np.int64)
    rank, top1, lv = (np.asarray(t.cpu()) for t in (rank, top1, lv))
    ptr, nodes, levels = (t.cpu().tolist() for t in (ptr, nodes, levels))
    for r, t in enumerate(torch.as_tensor(targets).cpu().tolist()):
        if not 0 <= t < n:
            continue
        path, lev = nodes[ptr[t]:ptr[t + 1]], levels[ptr[t]:ptr[t + 1]]
        L = len(path)
        if not 1 <= L <= MAXL:
            continue
        match = [0 <= le < n_levels and lv[r, le] == p for p, le in zip(path, lev)]
        point = sum(match)
        edge = int(match[0]) if L == 1 else sum(a and b for a, b in zip(match, match[1:]))
        for s in range(S):
            if rank[r, s] < 0:
                continue
            tab[s, L] += [1] + [int(rank[r, s] < k) for k in evaluate.TOPK] + [sum(p == top1[r, s] for p in path), point, edge]
    return torch.from_numpy(tab)


def test_set_counters_rows_against_the_python_restatement():
    """A synthetic DAG of depth 8 with nodes of two parents; node 7 is given an EMPTY path and node 11 a level outside the table.
    Targets of every path length (L == 1 included), padding rows (-1, n, n + 9, node 7), ranks around every k and -1, top1 on the
    path, off it and outside the tree, level arg-maxes planted along the path so that points and edges occur."""
    h = build_hierarchy(synth.make_dag(400, 8, 5, 0.15))
    n = len(h.nodes)
    ptr, nodes, levels = [0], [], []
    for t in range(n):
        path = [] if t == 7 else list(h.c2p[t]) + [t]
        nodes += path
        levels += [len(h.c2p[q]) if t != 11 else 40 for q in path]
        ptr.append(len(nodes))
    n_levels = max(levels[:ptr[11]] + levels[ptr[12]:]) + 1
    lengths = sorted({ptr[t + 1] - ptr[t] for t in range(n)})
    assert lengths[0] == 0 and lengths[1] == 1 and lengths[-1] >= 7
    rng = np.random.default_rng(12)
    rows, S = 150, 5
    tg = rng.integers(0, n, rows)
    by_len = {}
    for t in range(n):
        by_len.setdefault(ptr[t + 1] - ptr[t], t)
    tg[:len(by_len)] = list(by_len.values())                                            # one target of every path length, 0 included
    tg[20], tg[21], tg[22], tg[23] = -1, n, n + 9, 11
    rank = rng.choice(np.array([-1, 0, 1, 2, 4, 5, 9, 10, 19, 20, 300]), (rows, S))
    rank[:, 4] = -1                                                                     # a set without rows
    lv = rng.integers(0, n, (rows, n_levels))
    top1 = rng.integers(-1, n + 2, (rows, S))
    for r in range(rows):
        t = int(tg[r])
        if not 0 <= t < n:
            continue
        path = nodes[ptr[t]:ptr[t + 1]]
        for p, le in zip(path, levels[ptr[t]:ptr[t + 1]]):
            if le < n_levels and rng.random() < 0.7:
                lv[r, le] = p
        if path:
            top1[r, 0], top1[r, 1] = path[-1], path[0]
            top1[r, 2] = path[len(path) // 2] if r % 2 else top1[r, 2]
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)
    rd, td, ld_, tgd = i32(rank), i32(top1), i32(lv), torch.from_numpy(tg.astype(np.int64)).to(DEV)
    csr = (i32(ptr), i32(nodes), i32(levels))
    want = _table_restated(rd, td, tgd, ld_, *csr, n, n_levels)
    tot = dict(zip(ops.SETS_COL_NAMES, want.sum((0, 1)).tolist()))
    assert all(tot[k] > 0 for k in ops.SETS_COL_NAMES) and int(want[4].sum()) == 0 and int(want[:, 1, 0].sum()) > 0 and int(want[:, 0].sum()) == 0
    assert tot["hit@1"] < tot["hit@2"] < tot["hit@5"] < tot["hit@10"] < tot["hit@20"] < tot["rows"]

    def run(order, cuts):
        tab = torch.zeros((S, MAXL + 1, ops.SETS_COLS), dtype=torch.int64, device=DEV)
        for lo, hi in zip(cuts, cuts[1:]):
            o = order[lo:hi]
            ops.set_counters_rows(rd[o].contiguous(), td[o].contiguous(), tgd[o].contiguous(), ld_[o].contiguous(), *csr, tab)
        return tab.cpu()

    ident = torch.arange(rows, device=DEV)
    assert torch.equal(run(ident, [0, rows]), want)
    assert torch.equal(run(ident, [0, 1, 70, rows]), want)                              # the cut into launches does not matter
    assert torch.equal(run(torch.randperm(rows, generator=torch.Generator().manual_seed(7)).to(DEV), [0, 64, rows]), want)
    # rows is the counters' num_sample where every rank is >= 0: the same padding rule
    acc = torch.zeros(9, dtype=torch.float64, device=DEV)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    ops.eval_counters_rows(zeros(rows, K), tgd, zeros(rows), ld_, *csr, acc)
    tab = torch.zeros((1, MAXL + 1, ops.SETS_COLS), dtype=torch.int64, device=DEV)
    ops.set_counters_rows(zeros(rows, 1), zeros(rows, 1), tgd, ld_, *csr, tab)
    assert float(acc[8]) == int(tab[0, :, 0].sum())
    # point and edge are those of the main counters: path_all and point_all from the per-length integers
    t = tab[0].cpu().double()
    Ls = torch.arange(MAXL + 1, dtype=torch.float64)
    assert float(acc[6]) == pytest.approx(float((t[:, 8] / (Ls - 1).clamp_min(1)).sum()), rel=1e-12)
    assert float(acc[7]) == pytest.approx(float((t[1:, 7] / Ls[1:]).sum()), rel=1e-12)


# ---- 5. rejected arguments ---------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    """Real, amply sized device tensors: a missing check would give a wrong number, never a bad access."""
    n, rows = 20, 8
    x = torch.zeros((rows, n + 4), device=DEV)
    member = torch.full((n,), 3, dtype=torch.int32, device=DEV)
    key = torch.arange(n, dtype=torch.int32, device=DEV)
    tg = torch.zeros(rows, dtype=torch.int64, device=DEV)
    rank = torch.full((rows, 17), -7, dtype=torch.int32, device=DEV)
    top1 = torch.full((rows, 17), -7, dtype=torch.int32, device=DEV)
    lv = torch.zeros((rows, 4), dtype=torch.int32, device=DEV)
    ptr, nodes = torch.arange(n + 1, dtype=torch.int32, device=DEV), torch.arange(n, dtype=torch.int32, device=DEV)
    lev = torch.zeros(n, dtype=torch.int32, device=DEV)
    tab = torch.zeros((17, MAXL + 1, ops.SETS_COLS), dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(x=x.data_ptr(), ld=x.stride(0), n=n, member=member.data_ptr(), key=key.data_ptr(), s=2, tg=tg.data_ptr(), rank=rank.data_ptr(),
              top1=top1.data_ptr(), rows=rows)

    def call(**kw):
        a = dict(ok, **kw)
        _lib.call("hgr_set_ranks", a["x"], a["ld"], a["n"], a["member"], a["key"], a["s"], a["tg"], a["rank"], a["top1"], a["rows"], st)

    cases = {"null scores": dict(x=0), "null member": dict(member=0), "null tie_key": dict(key=0), "null top1": dict(top1=0),
             "targets without rank": dict(rank=0), "null top1 without targets": dict(tg=0, rank=0, top1=0), "rows = 0": dict(rows=0),
             "rows < 0": dict(rows=-1), "n_nodes = 0": dict(n=0), "ld < n_nodes": dict(ld=n - 1), "n_sets = 0": dict(s=0), "n_sets = 17": dict(s=17)}
    for name, kw in cases.items():
        with pytest.raises(_lib.HgrError, match="hgr_set_ranks"):
            call(**kw)
    okc = dict(rank=rank.data_ptr(), top1=top1.data_ptr(), s=2, tg=tg.data_ptr(), lv=lv.data_ptr(), nl=4, ptr=ptr.data_ptr(), nodes=nodes.data_ptr(),
               lev=lev.data_ptr(), n=n, tab=tab.data_ptr(), rows=rows)
    for kw in (dict(rank=0), dict(top1=0), dict(tg=0), dict(lv=0), dict(ptr=0), dict(nodes=0), dict(lev=0), dict(tab=0), dict(rows=0), dict(n=0),
               dict(s=0), dict(s=17), dict(nl=0), dict(nl=33)):
        a = dict(okc, **kw)
        with pytest.raises(_lib.HgrError, match="hgr_set_counters_rows"):
            _lib.call("hgr_set_counters_rows", a["rank"], a["top1"], a["s"], a["tg"], a["lv"], a["nl"], a["ptr"], a["nodes"], a["lev"], a["n"],
                      a["tab"], a["rows"], st)
    torch.cuda.synchronize()
    assert bool((rank == -7).all()) and bool((top1 == -7).all()) and int(tab.abs().sum()) == 0
    call()                                                                            # the same operands, accepted: the sentinels go
    call(tg=0, rank=0)                                                                # no targets: rank is not looked at
    torch.cuda.synchronize()
    assert bool((rank.view(-1)[:rows * 2] == 0).all()) and bool((top1.view(-1)[:rows * 2] == 0).all()) and bool((rank.view(-1)[rows * 2:] == -7).all())


# ---- 6. the reference's own logits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,hits,hits_all,num", [("tinyvit_n90", [1, 2, 6, 9, 11], 2, 24), ("smallvit_n300", None, None, None)])
def test_reference_logits(case, hits, hits_all, num, golden_dir, tmp_path):
    """The logits the reference computed (tests/golden/tree_*.npz) through Evaluator(sets=...): the set `rest` must count what the
    reference's main.test counted (the fixture's counters), the test classes of at most 5 path nodes and rest + train what the in-test
    restatement counts from the same logits."""
    model, meta, cfg, splits, z = _model(case, golden_dir, tmp_path)
    pos = {w: i for i, w in enumerate(model.nodes)}
    rest = [pos[w] for w in splits["rest"]]
    assert rest == model.test_index.cpu().tolist()
    shallow = [t for t in rest if len(model.c2p[t]) + 1 <= 5]
    sets = {"rest": rest, "shallow": shallow, "rest+train": rest + [pos[w] for w in splits["train"]]}
    ev = evaluate.Evaluator(model, sets=sets)
    plain = evaluate.Evaluator(model)
    csr = ev._ancestor_csr()
    n = len(model.nodes)
    want = torch.zeros((3, MAXL + 1, ops.SETS_COLS), dtype=torch.int64)
    member, key = ev.sets.member.cpu().numpy(), ev.sets.tie_key.cpu().numpy()
    for i in range(meta["batches"]):
        lg = torch.from_numpy(z["logits"][i]).to(DEV)
        t = meta["targets"][i]
        ev.add_batch(lg, t)
        plain.add_batch(lg, t)
        lv, p1, _ = ops.eval_rows(lg, ev.index, K)
        tg = [t] * lg.shape[0]
        rank, _ = _ranks_restated(lg, member, key, 3, tg)
        want += _table_restated(rank, p1.cpu().view(-1, 1).expand(-1, 3), tg, lv, *csr, n, ev.n_levels)
    got = ev.sets_table()
    assert torch.equal(got, want)
    rep = ev.sets_dict()["sets"]
    c = plain.counters()
    a = rep[0]
    print(f"[measured] {case}: rest {[a[f'hits@{k}'] for k in evaluate.TOPK]} hits_all {a['hits_all']} of {a['num_sample']}; "
          f"shallow ({len(shallow)} classes) {rep[1]['num_sample']} rows; rest+train {[rep[2][f'hits@{k}'] for k in evaluate.TOPK]}")
    assert [a[f"hits@{k}"] for k in evaluate.TOPK] == [int(c[f"hits@{k}"]) for k in evaluate.TOPK] == [int(meta["counters"][f"hits@{k}"]) for k in evaluate.TOPK]
    assert a["hits_all"] == int(c["hits_all"]) == int(meta["counters"]["hits_all"]) and a["num_sample"] == int(meta["counters"]["num_sample"])
    assert a["path_all"] == pytest.approx(c["path_all"], rel=1e-9) and a["point_all"] == pytest.approx(c["point_all"], rel=1e-9)
    assert evaluate.format_sets({"sets": [a]}).endswith(meta["metric"].strip("\n"))
    if hits is not None:
        assert [a[f"hits@{k}"] for k in evaluate.TOPK] == hits and a["hits_all"] == hits_all and a["num_sample"] == num and len(shallow) == 22
    else:
        assert a["hits@20"] == 3
    # more candidates can only push a target down; a subset of the classes can only hold a subset of the rows
    assert all(rep[2][f"hits@{k}"] <= a[f"hits@{k}"] for k in evaluate.TOPK) and rep[2]["num_sample"] == a["num_sample"]
    assert rep[1]["num_sample"] == meta["bsz"] * sum(len(model.c2p[t]) + 1 <= 5 for t in meta["targets"])


# ---- 7. wiring ---------------------------------------------------------------------------------------------------------------------------
SIZES = [5, 16, 9, 3, 12]
B = 16


@pytest.fixture(scope="module")
def e2e(golden_dir, tmp_path_factory):
    """The tiny ViT tree model with its classifier; S = every second test class, in the test order; a second model built with
    candidates_test = S; ragged one-class batches of images, three of classes of S and two of other test classes."""
    tmp = tmp_path_factory.mktemp("sets_e2e")
    model, meta, cfg, splits, _ = _model("tinyvit_n90", golden_dir, tmp)
    model.update_classifier()
    sub_wnids = splits["rest"][::2]
    model_s, _, _, _, _ = _model("tinyvit_n90", golden_dir, tmp_path_factory.mktemp("sets_e2e_s"), test_wnids=sub_wnids)
    model_s.update_classifier()
    pos = {w: i for i, w in enumerate(model.nodes)}
    sub = [pos[w] for w in sub_wnids]
    assert sub == model_s.test_index.cpu().tolist() and len(sub) == 20
    other = [t for t in model.test_index.cpu().tolist() if t not in sub]
    classes = [sub[1], other[2], sub[7], sub[12], other[5]]
    imgs = [synth.images(k, cfg["image_resolution"], 900 + i) for i, k in enumerate(SIZES)]
    splits = dict(splits, S=sub_wnids)
    return model, model_s, classes, imgs, sub, splits, tmp


def _sets_of(model, sub, splits):
    pos = {w: i for i, w in enumerate(model.nodes)}
    rest = model.test_index.cpu().tolist()
    return {"S": sub, "rest": rest, "S+train": sub + [pos[w] for w in splits["train"]]}


def test_a_set_counts_what_a_model_built_with_it_counts(e2e):
    model, model_s, classes, imgs, sub, splits, _ = e2e
    ev = evaluate.Evaluator(model, sets=_sets_of(model, sub, splits))
    plain, ev_s = evaluate.Evaluator(model), evaluate.Evaluator(model_s)
    for x, cl in zip(imgs, classes):
        lg = model(x.to(DEV)).clone()
        assert torch.equal(lg, model_s(x.to(DEV)))                                      # the same towers, the same classifier
        ev.add_batch(lg, cl)
        plain.add_batch(lg, cl)
        if cl in sub:                                                                   # the run over the classes of S
            ev_s.add_batch(lg, cl)
    assert ev.summary() == plain.summary() and torch.equal(ev.acc.cpu(), plain.acc.cpu())   # the main metric string is unchanged
    rep = ev.sets_dict()["sets"]
    c = ev_s.counters()
    s = rep[0]
    ints = ["hits@1", "hits@2", "hits@5", "hits@10", "hits@20", "hits_all", "num_sample"]
    assert [s[k] for k in ints] == [int(c[k]) for k in ints] and s["num_sample"] == SIZES[0] + SIZES[2] + SIZES[3] and s["classes"] == 20
    assert s["path_all"] == pytest.approx(c["path_all"], rel=1e-9) and s["point_all"] == pytest.approx(c["point_all"], rel=1e-9)
    line = evaluate.format_sets({"sets": [s]})
    assert line == "set S (20 classes, {} images): ".format(s["num_sample"]) + ev_s.summary().strip("\n")
    # the set that is the model's own test set repeats the main counters
    c = plain.counters()
    assert [rep[1][k] for k in ints] == [int(c[k]) for k in ints] and rep[1]["num_sample"] == sum(SIZES)
    assert rep[2]["num_sample"] == s["num_sample"] and all(rep[2][k] <= s[k] for k in ints[:5])


def test_sets_with_path_decoding_and_row_targets(e2e):
    """decode="path": the ranks are those of the path scores; add_batch_rows with a padding row; both against the restatement."""
    model, _, classes, imgs, sub, splits, _ = e2e
    sets = _sets_of(model, sub, splits)
    ev = evaluate.Evaluator(model, decode="path", decode_weights="increasing", sets=sets)
    rows_ev = evaluate.Evaluator(model, decode="path", decode_weights="increasing", sets=sets)
    flat = evaluate.Evaluator(model, sets=sets)
    csr = ev._ancestor_csr()
    n = len(model.nodes)
    member, key = ev.sets.member.cpu().numpy(), ev.sets.tie_key.cpu().numpy()
    want = torch.zeros((3, MAXL + 1, ops.SETS_COLS), dtype=torch.int64)
    want_rows = want.clone()
    wtab = evaluate.path_weight_table(model, "increasing")
    for x, cl in zip(imgs, classes):
        lg = model(x.to(DEV)).clone()
        ev.add_batch(lg, cl)
        flat.add_batch(lg, cl)
        tg = torch.full((x.shape[0],), cl, dtype=torch.int64, device=DEV)
        tg[0] = -1
        rows_ev.add_batch_rows(lg, tg)
        scores = ops.path_scores(lg, csr[0], csr[1], wtab)
        lv, p1, _ = ops.eval_rows(scores, ev.index, K)
        for table, targets in ((want, [cl] * x.shape[0]), (want_rows, tg.tolist())):
            rank, _ = _ranks_restated(scores, member, key, 3, targets)
            table += _table_restated(rank, p1.cpu().view(-1, 1).expand(-1, 3), targets, lv, *csr, n, ev.n_levels)
    assert torch.equal(ev.sets_table(), want) and torch.equal(rows_ev.sets_table(), want_rows)
    assert int(want[1, :, 0].sum()) == sum(SIZES) and int(want_rows[1, :, 0].sum()) == sum(SIZES) - len(SIZES)
    assert not torch.equal(flat.sets_table(), want)                                     # the path scores rank differently


def test_predict_with_sets(e2e):
    model, _, classes, imgs, sub, splits, _ = e2e
    sets = _sets_of(model, sub, splits)
    x = imgs[1]
    assert set(evaluate.predict(model, x)) == {"topk", "top1", "levels"}
    out = evaluate.predict(model, x, sets=sets)
    assert set(out) == {"topk", "top1", "levels", "set_top1"}
    ev = evaluate.Evaluator(model, sets=sets)
    lg = model(x.to(DEV)).clone()
    tg = [classes[1]] * (x.shape[0] - 1) + [sub[0]]
    want = _ranks_restated(lg, ev.sets.member.cpu().numpy(), ev.sets.tie_key.cpu().numpy(), 3, tg)
    assert out["set_top1"].dtype == torch.int32 and torch.equal(out["set_top1"].cpu().long(), want[1])
    assert torch.equal(out["set_top1"][:, 1], out["topk"][:, 0])                        # the model's own test set
    out = evaluate.predict(model, x, evaluator=ev, targets=torch.tensor(tg))
    assert set(out) == {"topk", "top1", "levels", "set_top1", "set_rank"}
    assert out["set_rank"].dtype == torch.int32 and torch.equal(out["set_rank"].cpu().long(), want[0])
    assert bool((out["set_rank"][:-1, 0] == -1).all()) and int(out["set_rank"][-1, 0]) >= 0
    with pytest.raises(ValueError):
        evaluate.predict(model, x, sets={})


def test_evaluate_test_with_eval_sets_flags(e2e, capsys):
    model, model_s, classes, imgs, sub, splits, tmp = e2e

    def loader():
        return [{"img": x[None], "label": torch.full((1, x.shape[0]), c, dtype=torch.long)} for x, c in zip(imgs, classes)]

    def run(**kw):
        o = types.SimpleNamespace(**vars(model.opts))
        o.test_batch_size = B
        o.hier_report = None
        o.__dict__.update(kw)
        capsys.readouterr()
        out = evaluate.test(o, model, DEV, splits, loader=loader(), log=False)
        return out, capsys.readouterr().out

    flat, flat_log = run()
    assert "set S" not in flat_log
    ev = evaluate.Evaluator(model, sets=_sets_of(model, sub, splits))
    for x, cl in zip(imgs, classes):
        ev.add_batch(model(x.to(DEV)), cl)
    want = ev.sets_dict()
    assert [e["name"] for e in want["sets"]] == ["S", "rest", "S+train"] and want["sets"][1]["num_sample"] == sum(SIZES)
    for pack in (False, True):
        path = tmp / f"sets_{int(pack)}.json"
        out, log = run(eval_sets="S,rest,S+train", eval_sets_report=str(path), pack_batches=pack)
        assert out == flat                                                            # the metric string is unchanged
        got = json.loads(path.read_text())
        for g, w in zip(got["sets"], want["sets"]):                                   # packed batches: the same integers, sums in another order
            assert {k: v for k, v in g.items() if isinstance(v, (int, str))} == {k: v for k, v in w.items() if isinstance(v, (int, str))}
            assert g["path_all"] == pytest.approx(w["path_all"], rel=1e-12) and g["by_depth"] == w["by_depth"]
        lines = evaluate.format_sets(want)
        assert lines in log and log.index(out) < log.index(lines) and len(lines.split("\n")) == 3
    extra = tmp / "extra.json"
    extra.write_text(json.dumps({"hop": splits["S"][:5]}))
    out, log = run(eval_sets="hop+train,S", eval_sets_file=str(extra))               # a second file, no report
    assert out == flat and "set hop+train (35 classes" in log and "set S (20 classes" in log
    with pytest.raises(ValueError, match="'nothing'"):
        run(eval_sets="S,nothing")
    extra.write_text(json.dumps({"S": splits["S"][:5]}))
    with pytest.raises(ValueError, match="'S'"):
        run(eval_sets="S", eval_sets_file=str(extra))


def test_an_evaluator_without_sets_is_as_before(golden_dir, tmp_path):
    """The small ViT model (the smallest fixture the fused route takes): without sets fused_ok() holds and nothing of the sets is
    allocated; with sets the images go through the logits route and count the same."""
    model, meta, cfg, splits, _ = _model("smallvit_n300", golden_dir, tmp_path)
    model.update_classifier()
    plain = evaluate.Evaluator(model)
    assert plain.fused_ok() and plain.sets is None and plain.sets_tab is None and plain._sets_buf is None
    te = model.test_index.cpu().tolist()
    ev = evaluate.Evaluator(model, sets={"rest": te, "few": te[:30]})
    assert not ev.fused_ok() and ev._sets_buf is None
    x = synth.images(7, cfg["image_resolution"], 41).to(DEV)
    plain.add_images(x, te[3])
    ev.add_images(x, te[3])
    assert plain.counters() == ev.counters() and ev._sets_buf is not None and plain._sets_buf is None
    tab = ev.sets_table()
    assert tab[:, :, 0].sum(1).tolist() == [7, 7] and tab[0, :, 1:6].sum(0).tolist() == [int(v) for v in plain.acc[:5].tolist()]
    assert tab[0, :, 6].sum().item() == int(plain.acc[5].item())
