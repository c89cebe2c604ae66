"""GPU: hedged predictions - hgr_subtree_hedge against an fp64 restatement of its definition (include/hgr.h) with the derived bound,
the exact integer identities of the masses, the picks against an integer restatement of the device's own masses, a hand-built CSR with
exactly representable probabilities, the shapes at which the launch changes, independence of row order and of the cut into launches,
hgr_hedge_counters_rows against a Python restatement, the rejected arguments, and the wiring: Evaluator(hedge=), evaluate.predict and
evaluate.test with --hedge / --hedge_report."""
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
SCALE = 2 ** 30
# |sum of q - 2^30| <= half a unit per candidate + 2^30 times the fp32 error of the normaliser and the division: at most 36 terms per lane
# (HGR_HEDGE_MAXN / 1024), 6 levels of the wave's tree, 16 waves and the division, one rounding of 2^-24 each - 59 * 64 < 4096
TOTAL_SLACK = 4096
THETAS = (0.1, 0.25, 0.5, 0.75, 0.9)


# ---- helpers of test_gpu_path_decode.py (copied: test modules do not import each other) -------------------------------------------------
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


def _model(case, golden_dir, tmp_path):
    meta, z, cfg, edges = _tree_case(case, golden_dir)
    sd = synth.clip_state_dict(cfg, 0)
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], meta["n_train"], meta["n_test"], meta["split_seed"])
    model = tree_model(_opts(tmp_path, edges), splits["all"], splits["rest"],
                       node_tokens=torch.from_numpy(z["node_tokens"].astype(np.int64)), clip_model=build_model(sd).to(DEV))
    with torch.no_grad():
        model.layer_weight.copy_((0.3 * torch.rand(model.layer_weight.shape, generator=torch.Generator().manual_seed(3))).to(DEV))
    return model, meta, cfg


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def _csr(paths):
    ptr, nodes = [0], []
    for p in paths:
        nodes += p
        ptr.append(len(nodes))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(nodes, dtype=torch.int32)


def _flat_csr(n):
    return torch.arange(n + 1, dtype=torch.int32), torch.arange(n, dtype=torch.int32)


def _lengths(ptr):
    """L(n), 0 where the path does not hold 1..32 nodes (such a node is never picked)."""
    L = (ptr[1:] - ptr[:-1]).cpu().long()
    return torch.where((L >= 1) & (L <= 32), L, torch.zeros_like(L))


def _edges(ptr, nodes, cand, n):
    """(src, dst) int64: candidate src adds its q to mass[dst] - the definition's scatter as an edge list."""
    ptr, nodes = ptr.cpu().tolist(), nodes.cpu().tolist()
    src, dst = [], []
    for c in range(n):
        if cand is not None and cand[c] < 0:
            continue
        o, L = ptr[c], ptr[c + 1] - ptr[c]
        if L < 1 or L > 32:
            src.append(c)
            dst.append(c)
            continue
        for a in nodes[o:o + L]:
            if 0 <= a < n:
                src.append(c)
                dst.append(a)
    return torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64)


def _scatter(q, src, dst, n):
    """mass[r, a] = sum of q[r, c] over the edges (c, a); q int64 (exact) or float64."""
    return torch.zeros((q.shape[0], n), dtype=q.dtype).index_add_(1, dst, q[:, src])


def _mass64(x, cand, src, dst, tau, n):
    """(M64 [rows, n], cnt [n]): the subtree masses of softmax(tau x) over the candidates in float64, and how many candidates add to a."""
    x = x.detach().cpu().double()
    mask = torch.ones(n, dtype=torch.bool) if cand is None else torch.as_tensor(cand).cpu() >= 0
    p = torch.zeros_like(x)
    if bool(mask.any()):
        p[:, mask] = torch.softmax(tau * x[:, mask], dim=1)
    return _scatter(p, src, dst, n), torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))


def _picks(mass, L, thr, total):
    """The pick rule on integer masses [rows, n] (int64): per threshold the node with 1 <= L <= 32 and mass >= thr of the largest
    L, then the largest mass, then the smallest id; -1 and the row's total where there is none.  Returns (pick, pick's mass) int64."""
    n = mass.shape[1]
    key = (L[None, :] << 47) | (mass << 16) | (0xFFFF - torch.arange(n, dtype=torch.int64))[None, :]
    pick, pm = [], []
    for t in thr:
        k = torch.where((L[None, :] >= 1) & (mass >= t), key, torch.zeros_like(key))
        best, arg = k.max(dim=1)
        pick.append(torch.where(best > 0, arg, torch.full_like(arg, -1)))
        pm.append(torch.where(best > 0, mass.gather(1, arg[:, None])[:, 0], total))
    return torch.stack(pick, 1), torch.stack(pm, 1)


def _hedge(x, cand, ptr, nodes, tau, thetas=THETAS, want_mass=True):
    """One launch on device copies: (pick [rows, T] int64, pick_mass fp32, mass int64 [rows, n]) on the CPU."""
    n = ptr.numel() - 1
    xd = x.to(DEV)
    thr = torch.tensor(ops.hedge_thresholds(thetas), dtype=torch.int32, device=DEV)
    mass = torch.full((x.shape[0], n), -7, dtype=torch.int32, device=DEV) if want_mass else None
    cd = None if cand is None else torch.as_tensor(cand, dtype=torch.int32).to(DEV)
    pick, pm = ops.subtree_hedge(xd, cd, ptr.to(DEV), nodes.to(DEV), tau, thr, mass_out=mass)
    return pick.cpu().long(), pm.cpu(), (mass.cpu().long() if want_mass else None)


def _check_picks(pick, pm, mass, q_total, ptr, thetas=THETAS):
    want, want_m = _picks(mass, _lengths(ptr), ops.hedge_thresholds(thetas), q_total)
    assert torch.equal(pick, want)
    assert torch.equal(pm, want_m.to(torch.float32) * (1.0 / SCALE))                     # bit-equal: one int -> fp32 rounding, an exact scale
    return want


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tinyvit_n90", "smallvit_n300", "dag_n3000"])
def tree(request, golden_dir, tmp_path_factory):
    """(n, ancestor CSR, candidate map, 64 rows of 0.05 * randn logits, seed 5, edge list of the scatter): on the CPU, shared, never
    written.  The two model hierarchies take the CSR and the test classes from an Evaluator; the larger one is
    synth.make_dag(3000, 12, 11, 0.1) with 1 500 candidates."""
    if request.param == "dag_n3000":
        h = build_hierarchy(synth.make_dag(3000, 12, 11, 0.1))
        n = len(h.nodes)
        ptr, nodes = _csr([list(h.c2p[t]) + [t] for t in range(n)])
        cand = np.full(n, -1, dtype=np.int32)
        chosen = np.sort(np.random.default_rng(11).choice(n, 1500, replace=False))
        cand[chosen] = np.arange(1500)
    else:
        model, meta, cfg = _model(request.param, golden_dir, tmp_path_factory.mktemp(request.param))
        ev = evaluate.Evaluator(model)
        ptr, nodes, _ = (t.cpu() for t in ev._ancestor_csr())
        n = len(model.nodes)
        cand = ev.index.test_pos.cpu().numpy()
    assert ptr.numel() == n + 1 and int((cand >= 0).sum()) >= 30
    x = 0.05 * torch.randn(64, n, generator=torch.Generator().manual_seed(5))
    return n, ptr, nodes, cand, x, _edges(ptr, nodes, cand, n)


@pytest.fixture(scope="module")
def runs(tree):
    """Per temperature: the device's (pick, pick_mass, mass) of the 64 shared rows from one launch, and q = the masses of a launch on
    the flat CSR (every path the node itself: mass = q)."""
    n, ptr, nodes, cand, x, _ = tree
    out = {}
    for tau in (100.0, 1.0):
        out[tau] = _hedge(x, cand, ptr, nodes, tau) + (_hedge(x, cand, *_flat_csr(n), tau)[2],)
    return out


# ---- 1. the masses against the fp64 restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [100.0, 1.0])
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_mass_within_the_derived_bound_of_the_fp64_restatement(tree, tau, rows):
    """|mass 2^-30 - M64| <= cnt(a) 2^-30 + M64 (tau 2^-21 + 2^-16), elementwise, no case left out.  cnt(a) = the candidates whose
    path holds a: one rounding per summand of q, doubled.  The relative term: one rounding each of the difference and the product in the
    exponent (|t| <= 2 tau), expf, the tree sum and the division, with a factor of two on top.  (An fp32 emulation on the CPU at
    N = 300 and N = 3 000 reached 0.5 of this bound.)"""
    n, ptr, nodes, cand, x, (src, dst) = tree
    _, _, mass = _hedge(x[:rows], cand, ptr, nodes, tau)
    m64, cnt = _mass64(x[:rows], cand, src, dst, tau, n)
    err = (mass.double() / SCALE - m64).abs()
    bound = cnt[None, :] / SCALE + m64 * (tau * 2.0 ** -21 + 2.0 ** -16)
    print(f"[measured] n={n} rows={rows} tau={tau}: max err {float(err.max()):.3e}, max err / bound "
          f"{float((err / bound.clamp_min(1e-300))[bound > 0].max()):.3f}, nodes with mass {int((mass > 0).sum())}")
    assert bool((err <= bound).all())
    assert int((mass > 0).sum()) >= rows * 3 and bool((mass >= 0).all())           # nothing kept the sentinel


# ---- 2. exact identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [100.0, 1.0])
def test_exact_identities_of_the_masses(tree, runs, tau):
    n, ptr, nodes, cand, x, (src, dst) = tree
    pick, pm, mass, q = runs[tau]
    L = _lengths(ptr)
    assert bool((q[:, torch.as_tensor(cand) < 0] == 0).all()) and bool((q >= 0).all())
    total = q.sum(1)
    assert bool(((total - SCALE).abs() <= n / 2 + TOTAL_SLACK).all())
    assert torch.equal(mass[:, L == 1].sum(1), total)                                # every path starts at a node of the top level
    assert bool((mass >= q).all())
    assert torch.equal(mass, _scatter(q, src, dst, n))                               # given q, the masses are integer sums: exact
    # a second run whose candidate set drops half the classes: the dropped ones contribute nothing
    kept = np.where(cand >= 0)[0][::2]
    cand2 = np.full(n, -1, dtype=np.int32)
    cand2[kept] = np.arange(len(kept))
    _, _, mass2 = _hedge(x, cand2, ptr, nodes, tau)
    q2 = _hedge(x, cand2, *_flat_csr(n), tau)[2]
    assert bool((q2[:, cand2 < 0] == 0).all()) and bool(((q2.sum(1) - SCALE).abs() <= n / 2 + TOTAL_SLACK).all())
    assert torch.equal(mass2, _scatter(q2, *_edges(ptr, nodes, cand2, n), n)) and not torch.equal(mass2, mass)
    assert bool((q2[:, kept] >= q[:, kept]).all())                                   # the same exponentials over a smaller normaliser


# ---- 3. the picks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [100.0, 1.0])
def test_picks_equal_the_integer_restatement_of_the_device_masses(tree, runs, tau):
    n, ptr, nodes, cand, x, _ = tree
    pick, pm, mass, q = runs[tau]
    _check_picks(pick, pm, mass, q.sum(1), ptr)                                      # every row, every threshold
    L = torch.cat([_lengths(ptr), torch.zeros(1, dtype=torch.int64)])                # L(-1) = 0
    depth = L[pick]
    assert bool((depth[:, 1:] <= depth[:, :-1]).all())                               # L(pick) is non-increasing in theta
    n_abstain = int((pick < 0).sum())
    print(f"[measured] n={n} tau={tau}: {n_abstain} of {pick.numel()} abstain, pick depths {sorted(set(depth.view(-1).tolist()))}")
    if tau == 100.0:
        assert n_abstain < pick.numel() and len(set(depth.view(-1).tolist())) >= 3   # the case decides something: picks at several depths


# ---- 4. a hand-built CSR with exactly representable probabilities ------------------------------------------------------------------------
def _hand():
    """20 nodes.  Top level: 0, 1.  Under 0: 2, 3; under 1: 4.  Candidates, three nodes deep: 5 under 2; 6, 7 under 3; 8, 9, 10 under 4.
    11: a candidate with an EMPTY path (its mass stays on itself; never picked).  12: [0, 25, 12] - 25 is outside the tree, skipped.
    13..15: candidates whose score underflows.  16..19 and the inner nodes 0..4: no candidates."""
    paths = [[0], [1], [0, 2], [0, 3], [1, 4], [0, 2, 5], [0, 3, 6], [0, 3, 7], [1, 4, 8], [1, 4, 9], [1, 4, 10], [], [0, 25, 12],
             [1, 13], [0, 2, 14], [1, 4, 15], [0, 16], [0, 2, 17], [1, 18], [1, 4, 19]]
    cand = np.full(20, -1, dtype=np.int32)
    cand[5:16] = np.arange(11)
    return _csr(paths), cand


def test_hand_built_csr():
    """tau = 100.  Row 0: the 8 candidates 5..12 at score 0, 13..15 at -10 (exp(-1000) = 0 exactly): q = 2^27 each, in units of 1/8:
    mass[0] = 4 (5, 6, 7, 12), mass[1] = 3, mass[2] = 1, mass[3] = 2, mass[4] = 3, every candidate 1.  The non-candidates hold score
    +5: they must not move the maximum.  Row 1: candidates 11 and 12 alone at 0: q = 2^29 each."""
    (ptr, nodes), cand = _hand()
    x = torch.full((2, 20), 5.0)
    x[0, 5:13], x[0, 13:16] = 0.0, -10.0
    x[1, 5:16], x[1, 11:13] = -10.0, 0.0
    thetas = (0.125, 0.25, 0.375, 0.5, 0.51)
    pick, pm, mass = _hedge(x, cand, ptr, nodes, 100.0, thetas)
    u = 2 ** 27
    assert mass[0].tolist() == [4 * u, 3 * u, u, 2 * u, 3 * u] + [u] * 8 + [0] * 7
    assert mass[1].tolist() == [4 * u] + [0] * 10 + [4 * u, 4 * u] + [0] * 7
    # 0.125: the seven candidates of three nodes tie in L and in mass - the smallest id; 0.25: nodes 3 (2/8) and 4 (3/8) tie in L - the
    # larger mass, although the larger id; 0.375: mass == threshold counts; 0.5: node 0 alone; 0.51: nobody - abstain, the row's total
    assert pick[0].tolist() == [5, 4, 4, 0, -1] and pm[0].tolist() == [0.125, 0.375, 0.375, 0.5, 1.0]
    # row 1: node 12 (three nodes, 1/2) wins over 0 (one node, 1/2); node 11 has no path and is never picked
    assert pick[1].tolist() == [12, 12, 12, 12, -1] and pm[1].tolist() == [0.5, 0.5, 0.5, 0.5, 1.0]
    # no candidate at all: abstain with mass 0, every mass zero
    pick, pm, mass = _hedge(x, np.full(20, -1, dtype=np.int32), ptr, nodes, 100.0, thetas)
    assert bool((pick == -1).all()) and bool((pm == 0).all()) and bool((mass == 0).all())
    # a null candidate map: every node is a candidate - the nine nodes at +5 (0..4, 16..19) share the row, 1/9 each; at 0.125 nodes
    # 2 (itself and 17) and 4 (itself and 19) tie with 2/9; node 0 holds 5/9 (0, 2, 3, 16, 17), enough for every other threshold
    pick, pm, mass = _hedge(x[:1], None, ptr, nodes, 100.0, thetas)
    assert int(mass[0, 5:16].sum()) == 0 and int(mass[0, 16]) == int(mass[0, 19]) > 0 and int(mass[0, 2]) == int(mass[0, 4]) == 2 * int(mass[0, 16])
    assert pick[0].tolist() == [2, 0, 0, 0, 0]


# ---- 5. shapes ---------------------------------------------------------------------------------------------------------------------------
def test_one_node_and_more_rows_than_the_grid():
    pick, pm, mass = _hedge(torch.tensor([[0.3], [-2.0]]), None, *_flat_csr(1), 7.0)
    assert bool((pick == 0).all()) and bool((pm == 1.0).all()) and mass.tolist() == [[SCALE], [SCALE]]
    # 1 024 workgroups at the most: the rows behind them are taken in a second round
    rows = 1024 + 37
    x = torch.randn(rows, 3, generator=torch.Generator().manual_seed(3))
    ptr, nodes = _csr([[0], [0, 1], [0, 2]])
    pick, pm, mass = _hedge(x, None, ptr, nodes, 2.0)
    m64, cnt = _mass64(x, None, *_edges(ptr, nodes, None, 3), 2.0, 3)
    assert bool(((mass.double() / SCALE - m64).abs() <= cnt[None, :] / SCALE + m64 * (2.0 * 2.0 ** -21 + 2.0 ** -16)).all())
    _check_picks(pick, pm, mass, mass[:, 0], ptr)                                    # node 0 holds the row's total
    assert len(set(pick.view(-1).tolist())) >= 3


def test_the_full_lds_launch():
    """n_nodes = HGR_HEDGE_MAXN with a flat CSR, 2 rows: the mass row takes all 147 456 B.  Its masses are q."""
    n = ops.HEDGE_MAXN
    x = torch.randn(2, n, generator=torch.Generator().manual_seed(9))
    ptr, nodes = _flat_csr(n)
    thetas = (2.0 ** -16, 2.0 ** -12, 2.0 ** -9, 0.5)
    pick, pm, mass = _hedge(x, None, ptr, nodes, 1.0, thetas)
    p = torch.softmax(x.double(), dim=1)
    assert bool(((mass.double() / SCALE - p).abs() <= 1.0 / SCALE + p * (2.0 ** -21 + 2.0 ** -16)).all())
    assert bool(((mass.sum(1) - SCALE).abs() <= n / 2 + TOTAL_SLACK).all())
    want = _check_picks(pick, pm, mass, mass.sum(1), ptr, thetas)
    assert bool((want[:, 0] >= 0).all()) and bool((want[:, 3] == -1).all())
    assert torch.equal(pick[:, 0], mass.argmax(1))                                   # every L is 1: the largest mass


# ---- 6. independence -----------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_row_order_cut_or_leading_dimensions(tree, runs):
    n, ptr, nodes, cand, x, _ = tree
    pick, pm, mass, _ = runs[100.0]
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(6))
    a = _hedge(x[perm], cand, ptr, nodes, 100.0)
    assert all(torch.equal(g, w[perm]) for g, w in zip(a, (pick, pm, mass)))
    for cuts in ([0, 1, 6, 64], [0, 33, 64]):
        parts = [_hedge(x[lo:hi], cand, ptr, nodes, 100.0) for lo, hi in zip(cuts, cuts[1:])]
        assert all(torch.equal(torch.cat([p[i] for p in parts]), w) for i, w in enumerate((pick, pm, mass)))
    # views of wider buffers: ld = n + 8, ld_mass = n + 24; the columns beyond n_nodes keep their sentinel, the logits are not written
    xb = torch.full((64, n + 8), 1000.0)
    xb[:, :n] = x
    xd = xb.to(DEV)
    mb = torch.full((64, n + 24), -7, dtype=torch.int32, device=DEV)
    thr = torch.tensor(ops.hedge_thresholds(THETAS), dtype=torch.int32, device=DEV)
    p2, pm2 = ops.subtree_hedge(xd[:, :n], torch.as_tensor(cand).to(DEV), ptr.to(DEV), nodes.to(DEV), 100.0, thr, mass_out=mb[:, :n])
    assert torch.equal(p2.cpu().long(), pick) and torch.equal(pm2.cpu(), pm) and torch.equal(mb[:, :n].cpu().long(), mass)
    assert bool((mb[:, n:] == -7).all()) and torch.equal(xd.cpu(), xb)
    # and without a mass dump the picks are the same
    p3, pm3, _ = _hedge(x, cand, ptr, nodes, 100.0, want_mass=False)
    assert torch.equal(p3, pick) and torch.equal(pm3, pm)


# ---- 7. the outcome counters -------------------------------------------------------------------------------------------------------------
def _counters_restated(pick, targets, ptr, nodes, n):
    ptr, nodes = ptr.cpu().tolist(), nodes.cpu().tolist()
    T = pick.shape[1]
    tab = np.zeros((T, ops.HEDGE_COLS), dtype=np.int64)
    col = {k: i for i, k in enumerate(ops.HEDGE_COL_NAMES)}

    def path(a):
        if not 0 <= a < n:
            return None
        p = nodes[ptr[a]:ptr[a + 1]]
        return p if 1 <= len(p) <= 32 else None

    for r, t in enumerate(targets.cpu().tolist()):
        pt = path(t)
        if pt is None:
            continue
        for i, xk in enumerate(pick[r].tolist()):
            px = path(xk) or []
            c = 0
            while c < min(len(px), len(pt)) and px[c] == pt[c]:
                c += 1
            Lx, Lt = len(px), len(pt)
            if xk == -1:
                name = "abstain"
            elif Lx == 0:
                name = "wrong"
            elif xk == t:
                name = "exact"
            elif c == Lx < Lt:
                name = "ancestor"
            elif c == Lt < Lx:
                name = "below"
            else:
                name = "wrong"
            row = tab[i]
            row[col["rows"]] += 1
            row[col[name]] += 1
            row[col["sum_lpick"]] += Lx
            row[col["sum_common"]] += c
            row[col["sum_lt"]] += Lt
            row[ops.HEDGE_COL_HIST + Lx] += 1
    return torch.from_numpy(tab)


def test_hedge_counters_rows_against_the_python_restatement(tree, runs):
    """The device's picks of the shared rows with every outcome planted: the target itself, its ancestors, a node below it, another
    branch, abstentions, ids outside the tree (-2, n + 5); targets of every kind with padding rows (-1, >= n_nodes)."""
    n, ptr, nodes, cand, x, _ = tree
    pick = runs[100.0][0].clone()
    rng = np.random.default_rng(21)
    ids = np.where(cand >= 0)[0]
    tg = torch.from_numpy(ids[rng.integers(0, len(ids), 64)].astype(np.int64))
    pl, nl = ptr.tolist(), nodes.tolist()
    for r in range(0, 64, 2):
        p = nl[pl[int(tg[r])]:pl[int(tg[r]) + 1]]
        pick[r, 0] = p[-1]                                                            # exact
        pick[r, 1] = p[0]                                                             # an ancestor (the target itself when L == 1)
        pick[r, 2] = p[len(p) // 2]
        pick[r, 3] = [-1, -2, n + 5, n - 1][(r // 2) % 4]
    for r in range(1, 64, 4):                                                         # the target is an inner node, the pick lies below it
        p = nl[pl[int(pick[r - 1, 0])]:pl[int(pick[r - 1, 0]) + 1]]
        tg[r] = p[0]
        pick[r, 0], pick[r, 1] = p[-1], p[0]
    tg[5], tg[17], tg[40], tg[63] = -1, n, n + 9, -3
    want = _counters_restated(pick, tg, ptr, nodes, n)
    names = dict(zip(ops.HEDGE_COL_NAMES, want.sum(0).tolist()))
    assert all(names[k] > 0 for k in ("abstain", "exact", "ancestor", "below", "wrong")) and int(want[0, 0]) == 60
    assert bool((want[:, 1:6].sum(1) == want[:, 0]).all()) and bool((want[:, ops.HEDGE_COL_HIST:].sum(1) == want[:, 0]).all())
    pd, td, ptd, nd = pick.to(torch.int32).to(DEV), tg.to(DEV), ptr.to(DEV), nodes.to(DEV)

    def run(order, cuts):
        tab = torch.zeros((pick.shape[1], ops.HEDGE_COLS), dtype=torch.int64, device=DEV)
        for lo, hi in zip(cuts, cuts[1:]):
            ops.hedge_counters_rows(pd[order[lo:hi]].contiguous(), td[order[lo:hi]].contiguous(), ptd, nd, tab)
        return tab.cpu()

    ident = torch.arange(64, device=DEV)
    assert torch.equal(run(ident, [0, 64]), want)
    assert torch.equal(run(torch.randperm(64, generator=torch.Generator().manual_seed(7)).to(DEV), [0, 64]), want)
    assert torch.equal(run(ident, [0, 1, 6, 39, 64]), want)
    # ROWS is the counters' num_sample: the same padding rule (the counters' other operands do not matter for it)
    acc = torch.zeros(9, dtype=torch.float64, device=DEV)
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    ops.eval_counters_rows(zeros(64, K), td, zeros(64), zeros(64, 1), ptd, nd, torch.zeros_like(nd), acc)
    assert float(acc[8]) == 60 == int(want[0, 0])


# ---- 8. rejected arguments ---------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    """Real, amply sized device tensors: a missing check would give a wrong number, never a bad access."""
    (ptr, nodes), cand = _hand()
    ptr, nodes, cand = ptr.to(DEV), nodes.to(DEV), torch.from_numpy(cand).to(DEV)
    big_ptr, big_nodes = (t.to(DEV) for t in _flat_csr(ops.HEDGE_MAXN + 1))
    n = 20
    x = torch.zeros((8, ops.HEDGE_MAXN + 1), device=DEV)
    thr = torch.tensor([2 ** 28] + [2 ** 29 + i for i in range(8)], dtype=torch.int32, device=DEV)          # nine, for "T = 9"
    pick = torch.full((8, 9), -7, dtype=torch.int32, device=DEV)
    pm = torch.full((8, 9), 7.5, device=DEV)
    mass = torch.full((8, ops.HEDGE_MAXN + 1), -7, dtype=torch.int32, device=DEV)
    tab = torch.zeros((8, ops.HEDGE_COLS), dtype=torch.int64, device=DEV)
    tg = torch.zeros(8, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(x=x.data_ptr(), ld=x.stride(0), n=n, cand=cand.data_ptr(), ptr=ptr.data_ptr(), nodes=nodes.data_ptr(), tau=1.0, thr=thr.data_ptr(),
              t=2, pick=pick.data_ptr(), pm=pm.data_ptr(), mass=mass.data_ptr(), ldm=mass.stride(0), rows=8)

    def call(**kw):
        a = dict(ok, **kw)
        _lib.call("hgr_subtree_hedge", a["x"], a["ld"], a["n"], a["cand"], a["ptr"], a["nodes"], a["tau"], a["thr"], a["t"], a["pick"], a["pm"],
                  a["mass"], a["ldm"], a["rows"], st)

    cases = {"null scores": dict(x=0), "null anc_ptr": dict(ptr=0), "null anc_nodes": dict(nodes=0), "null thr": dict(thr=0),
             "null pick": dict(pick=0), "null pick_mass": dict(pm=0), "rows = 0": dict(rows=0), "n_nodes = 0": dict(n=0),
             "n_nodes = MAXN + 1": dict(n=ops.HEDGE_MAXN + 1, cand=0, ptr=big_ptr.data_ptr(), nodes=big_nodes.data_ptr()),
             "ld < n_nodes": dict(ld=19), "ld_mass < n_nodes": dict(ldm=19), "T = 0": dict(t=0), "T = 9": dict(t=9), "tau = 0": dict(tau=0.0),
             "tau < 0": dict(tau=-1.0), "tau = inf": dict(tau=float("inf")), "tau = nan": dict(tau=float("nan"))}
    for name, kw in cases.items():
        with pytest.raises(_lib.HgrError, match="hgr_subtree_hedge"):
            call(**kw)
    for kw in (dict(pick=0), dict(tg=0), dict(tab=0), dict(rows=0), dict(t=0), dict(t=9), dict(n=0)):
        a = dict(dict(pick=pick.data_ptr(), t=2, tg=tg.data_ptr(), n=n, tab=tab.data_ptr(), rows=8), **kw)
        with pytest.raises(_lib.HgrError, match="hgr_hedge_counters_rows"):
            _lib.call("hgr_hedge_counters_rows", a["pick"], a["t"], a["tg"], ptr.data_ptr(), nodes.data_ptr(), a["n"], a["tab"], a["rows"], st)
    with pytest.raises(_lib.HgrError, match="hgr_subtree_hedge"):
        ops.subtree_hedge(x[:, :n], cand, ptr, nodes, 0.0, thr[:2])
    torch.cuda.synchronize()
    assert bool((pick == -7).all()) and bool((pm == 7.5).all()) and bool((mass == -7).all()) and int(tab.abs().sum()) == 0
    call()                                                                            # the same operands, accepted: the sentinels go
    call(mass=0, ldm=0, t=8)                                                          # no mass dump: ld_mass is not looked at
    torch.cuda.synchronize()
    assert bool((pick[:2] != -7).all()) and bool((mass[:, :n] >= 0).all()) and bool((mass[:, n:] == -7).all())


# ---- 9. wiring ---------------------------------------------------------------------------------------------------------------------------
SIZES = [5, 37, 64, 3]
B = 64


@pytest.fixture(scope="module")
def e2e(golden_dir, tmp_path_factory):
    """The small ViT tree model (the smallest fixture the fused evaluation route takes) with its classifier, and ragged one-class
    batches of images."""
    tmp = tmp_path_factory.mktemp("hedge_e2e")
    model, meta, cfg = _model("smallvit_n300", golden_dir, tmp)
    model.update_classifier()
    te = model.test_index.cpu().tolist()
    classes = [te[i] for i in np.random.default_rng(5).choice(len(te), len(SIZES), replace=False)]
    imgs = [synth.images(n, cfg["image_resolution"], 700 + i) for i, n in enumerate(SIZES)]
    return model, classes, imgs, tmp


def _direct_table(model, batches, tau, decode_weights=None):
    """The hedge table from the kernels called one by one on (logits, row targets) batches."""
    ev = evaluate.Evaluator(model)
    ptr, nodes, _ = ev._ancestor_csr()
    thr = torch.tensor(ops.hedge_thresholds(THETAS), dtype=torch.int32, device=DEV)
    tab = torch.zeros((len(THETAS), ops.HEDGE_COLS), dtype=torch.int64, device=DEV)
    for logits, tg in batches:
        if decode_weights is not None:
            logits = ops.path_scores(logits, ptr, nodes, evaluate.path_weight_table(model, decode_weights))
        pick, _ = ops.subtree_hedge(logits, ev.index.test_pos, ptr, nodes, tau, thr)
        ops.hedge_counters_rows(pick, tg, ptr, nodes, tab)
    return tab.cpu()


def test_hedge_leaves_counters_and_report_alone_on_every_route(e2e):
    model, classes, imgs, _ = e2e
    tau = float(model.clip_model.logit_scale.detach().exp())
    plain = [evaluate.Evaluator(model, report=True) for _ in range(4)]
    hedged = [evaluate.Evaluator(model, report=True, hedge=THETAS) for _ in range(4)]
    assert plain[0].fused_ok() and not hedged[0].fused_ok() and hedged[0].hedge_temperature == tau
    assert all(e.hedge is None and e.hedge_tab is None and e._hedge_thr is None and e._hedge_pick is None for e in plain)
    class_batches, row_batches = [], []
    for x, cl in zip(imgs, classes):
        xd = x.to(DEV)
        tg = torch.full((x.shape[0],), cl, dtype=torch.int64, device=DEV)
        class_batches.append((model(xd).clone(), tg.clone()))
        tg[0] = -1                                                                    # a padding row for the row scorers
        row_batches.append((class_batches[-1][0], tg))
        for evs in (plain, hedged):
            oa = evs[0].add_batch(model(xd), cl)
            ob = evs[1].add_images(xd, cl, want_outputs=True)
            assert all(torch.equal(p, q) for p, q in zip(oa, ob))
            evs[2].add_batch_rows(model(xd), tg)
            evs[3].add_images_rows(xd, tg)
    for p, h in zip(plain, hedged):
        assert torch.equal(p.acc.cpu(), h.acc.cpu()) and torch.equal(p.report_table(), h.report_table())
    assert float(hedged[0].acc[8]) == sum(SIZES) and float(hedged[2].acc[8]) == sum(SIZES) - len(SIZES)
    want_class, want_rows = _direct_table(model, class_batches, tau), _direct_table(model, row_batches, tau)
    assert torch.equal(hedged[0].hedge_table(), want_class) and torch.equal(hedged[1].hedge_table(), want_class)
    assert torch.equal(hedged[2].hedge_table(), want_rows) and torch.equal(hedged[3].hedge_table(), want_rows)
    assert want_class[:, 0].tolist() == [sum(SIZES)] * 5 and want_rows[:, 0].tolist() == [sum(SIZES) - len(SIZES)] * 5
    # path decoding and the hedge compose: the hedge runs on the path scores
    ev = evaluate.Evaluator(model, decode="path", decode_weights="increasing", hedge=THETAS, hedge_temperature=60.0)
    for (logits, tg), cl in zip(class_batches, classes):
        ev.add_batch(logits, cl)
    assert torch.equal(ev.hedge_table(), _direct_table(model, class_batches, 60.0, "increasing"))
    logits = class_batches[-1][0]                                                     # the pick buffers hold the last batch
    ptr, nodes, _ = ev._ancestor_csr()
    thr = torch.tensor(ops.hedge_thresholds(THETAS), dtype=torch.int32, device=DEV)
    scores = ops.path_scores(logits, ptr, nodes, evaluate.path_weight_table(model, "increasing"))
    on_scores, on_logits = (ops.subtree_hedge(t, ev.index.test_pos, ptr, nodes, 60.0, thr) for t in (scores, logits))
    got = [b[:logits.shape[0] * 5].view(-1, 5) for b in ev._hedge_pick]
    assert torch.equal(got[0], on_scores[0]) and torch.equal(got[1], on_scores[1]) and not torch.equal(got[1], on_logits[1])


def test_predict_with_hedge(e2e):
    model, classes, imgs, _ = e2e
    x = imgs[1]
    logits = model(x.to(DEV)).clone()
    ev = evaluate.Evaluator(model)
    ptr, nodes, _ = ev._ancestor_csr()
    n = ev.index.n_nodes
    thr = torch.tensor(ops.hedge_thresholds(THETAS), dtype=torch.int32, device=DEV)
    assert set(evaluate.predict(model, x)) == {"topk", "top1", "levels"}
    for kw, scores in (({}, logits), ({"decode": "path", "decode_weights": "equal"},
                                      ops.path_scores(logits, ptr, nodes, evaluate.path_weight_table(model, "equal")))):
        mass = torch.empty((x.shape[0], n), dtype=torch.int32, device=DEV)
        pick, pm = ops.subtree_hedge(scores, ev.index.test_pos, ptr, nodes, 30.0, thr, mass_out=mass)
        out = evaluate.predict(model, x, hedge=THETAS, hedge_temperature=30.0, want_mass=True, **kw)
        assert set(out) == {"topk", "top1", "levels", "hedge", "hedge_mass", "mass"}
        assert out["hedge"].dtype == torch.int32 and out["hedge"].shape == (x.shape[0], 5) and torch.equal(out["hedge"], pick)
        assert out["hedge_mass"].dtype == torch.float32 and torch.equal(out["hedge_mass"], pm)
        assert out["mass"].dtype == torch.float32 and out["mass"].shape == (x.shape[0], n)
        assert torch.equal(out["mass"], mass.float() * 2.0 ** -30)
        assert torch.equal(out["topk"], ops.eval_rows(scores, ev.index, K)[2])
    assert "mass" not in evaluate.predict(model, x, hedge=(0.5,))
    with pytest.raises(ValueError):
        evaluate.predict(model, x, want_mass=True)
    with pytest.raises(ValueError):
        evaluate.predict(model, x, hedge=(0.5, 0.25))


def test_evaluate_test_with_hedge_flags(e2e, capsys):
    model, classes, imgs, tmp = e2e

    def loader():
        return [{"img": x[None], "label": torch.full((1, x.shape[0]), c, dtype=torch.long)} for x, c in zip(imgs, classes)]

    def run(**kw):
        o = types.SimpleNamespace(**vars(model.opts))
        o.test_batch_size = B
        o.hier_report = None
        o.__dict__.update(kw)
        capsys.readouterr()
        out = evaluate.test(o, model, DEV, None, loader=loader(), log=False)
        return out, capsys.readouterr().out

    flat, flat_log = run()
    assert "hedge" not in flat_log
    tau = float(model.clip_model.logit_scale.detach().exp())
    batches = [(model(x.to(DEV)).clone(), torch.full((x.shape[0],), c, dtype=torch.int64, device=DEV)) for x, c in zip(imgs, classes)]
    want = evaluate.hedge_from_table(_direct_table(model, batches, tau), THETAS, temperature=tau)
    assert want["by_threshold"][0]["rows"] == sum(SIZES)
    for pack in (False, True):
        path = tmp / f"hedge_{int(pack)}.json"
        out, log = run(hedge=",".join(str(t) for t in THETAS), hedge_report=str(path), pack_batches=pack)
        assert out == flat                                                            # the metric string is unchanged
        assert json.loads(path.read_text()) == json.loads(json.dumps(want))
        lines = evaluate.format_hedge(want)
        assert lines in log and log.index(out) < log.index(lines) and len(lines.split("\n")) == 6
    out, log = run(hedge=THETAS, hedge_temperature=5.0)                               # a sequence, another temperature, no file
    assert out == flat and evaluate.format_hedge(evaluate.hedge_from_table(_direct_table(model, batches, 5.0), THETAS)) in log
