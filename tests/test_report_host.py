"""CPU: the hierarchy report without a device - the argument validation of hgr_eval_report_rows (nothing is launched), the conversion
of its int64 table into the report (evaluate.report_from_table), the sum over ranks and the --hier_report switch."""
import ctypes as C

import pytest
import torch

from hgr_net_amd import evaluate, ops

COLS = ops.REPORT_DEPTH_COLS


def test_layout_mirrors_the_header():
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "hgr.h").read_text()
    assert re.search(r"#define HGR_REPORT_MAXL 32\b", header) and re.search(r"#define HGR_REPORT_DEPTH_COLS 10\b", header)
    assert (ops.REPORT_DEPTH, ops.REPORT_LEVEL, ops.REPORT_DIST_TEST, ops.REPORT_DIST_ALL, ops.REPORT_HEIGHT, ops.REPORT_LEN) == (0, 330, 394, 460, 526, 531)
    for name, want in (("LEVEL", 330), ("DIST_TEST", 394), ("DIST_ALL", 460), ("HEIGHT", 526), ("LEN", 531)):
        assert re.search(r"#define HGR_REPORT_%s .*/\* %d " % (name, want), header), name
    assert len(COLS) == 10 and ops.REPORT_DIST_BINS == 66 and ops.REPORT_DIST_UNKNOWN == 65


def test_eval_report_rows_rejects_bad_arguments_without_launching():
    """Null targets, a null table, k = 33, n_levels = 33 and rows = 0 come back as the library's error code before anything touches a
    device (the pointers are never dereferenced on this path)."""
    from hgr_net_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(k=20, targets=p, n_levels=8, rows=4, table=p):
        return lib.hgr_eval_report_rows(p, k, targets, p, p, n_levels, p, p, p, 10, table, rows, None)

    for kw in (dict(targets=None), dict(table=None), dict(k=33), dict(n_levels=33), dict(rows=0)):
        rc = call(**kw)
        assert rc != 0, kw
        assert b"hgr_eval_report_rows" in lib.hgr_last_error()
    for args in ((p, 33, p, p, p, 8, p, p, p, 10, p, 4, None), (p, 20, p, p, p, 8, p, p, p, 10, None, 4, None),
                 (p, 20, None, p, p, 8, p, p, p, 10, p, 4, None), (p, 20, p, p, p, 33, p, p, p, 10, p, 4, None),
                 (p, 20, p, p, p, 8, p, p, p, 10, p, 0, None)):
        with pytest.raises(_lib.HgrError, match="hgr_eval_report_rows"):
            _lib.call("hgr_eval_report_rows", *args)


def test_wrapper_checks_the_table():
    z32 = torch.zeros(4, dtype=torch.int32)
    ok = dict(pred=torch.zeros(4, 20, dtype=torch.int32), targets=torch.zeros(4, dtype=torch.int64), top1=z32, lv=torch.zeros(4, 8, dtype=torch.int32),
              anc_ptr=torch.zeros(11, dtype=torch.int32), anc_nodes=z32, anc_levels=z32)
    for table in (torch.zeros(ops.REPORT_LEN, dtype=torch.float64), torch.zeros(ops.REPORT_LEN - 1, dtype=torch.int64)):
        with pytest.raises(AssertionError):
            ops.eval_report_rows(table=table, **ok)
    with pytest.raises(AssertionError):
        ops.eval_report_rows(table=torch.zeros(ops.REPORT_LEN, dtype=torch.int64), **dict(ok, targets=torch.zeros(4, dtype=torch.int32)))


def _depth(table, L, **kw):
    for name, v in kw.items():
        table[ops.REPORT_DEPTH + L * len(COLS) + COLS.index(name)] += v


def _hand_table():
    """12 rows: 4 of path length 1 (depth 0) and 8 of path length 4 (depth 3); nothing at any other depth."""
    t = torch.zeros(ops.REPORT_LEN, dtype=torch.int64)
    _depth(t, 1, rows=4, **{"hit@1": 1, "hit@2": 2, "hit@5": 2, "hit@10": 3, "hit@20": 4}, anc_hit=3, point=2, edge=2, chain=2)
    _depth(t, 4, rows=8, **{"hit@1": 2, "hit@2": 2, "hit@5": 4, "hit@10": 4, "hit@20": 6}, anc_hit=10, point=20, edge=9, chain=1)
    for i, (n, m) in enumerate(((12, 7), (8, 6), (8, 5), (8, 4))):             # level rows: 12 rows have a position 0, 8 have 1..3
        t[ops.REPORT_LEVEL + 2 * i], t[ops.REPORT_LEVEL + 2 * i + 1] = n, m
    for d, c in ((0, 3), (2, 4), (5, 4)):                                      # 3 right, 8 wrong at distances 2 and 5, 1 unknown
        t[ops.REPORT_DIST_TEST + d] = c
    t[ops.REPORT_DIST_TEST + ops.REPORT_DIST_UNKNOWN] = 1
    t[ops.REPORT_DIST_ALL + 0] = 12                                            # no row wrong
    for i, h in enumerate((18, 40, 110, 230, 470)):
        t[ops.REPORT_HEIGHT + i] = h
    return t


def test_report_from_table_on_a_hand_written_table():
    rep = evaluate.report_from_table(_hand_table())
    assert rep["num_sample"] == 12
    assert [e["depth"] for e in rep["by_depth"]] == [0, 3]                     # empty depths are left out
    d0, d3 = rep["by_depth"]
    assert d0["rows"] == 4 and d0["hits@1"] == 1 and d0["acc@1"] == 25.0 and d0["acc@20"] == 100.0
    assert d0["hit_ratio"] == 75.0 and d0["path_ratio"] == 50.0 and d0["point_ratio"] == 50.0 and d0["chain_ratio"] == 50.0   # L = 1: edge / rows
    assert d3["rows"] == 8 and d3["hits@5"] == 4 and d3["acc@5"] == 50.0
    assert d3["hit_ratio"] == 125.0                                            # anc_hit counts path nodes, as summary()'s hits_all / n does
    assert d3["path_ratio"] == pytest.approx(9 / 3 / 8 * 100, rel=1e-12) and d3["point_ratio"] == pytest.approx(20 / 4 / 8 * 100, rel=1e-12)
    assert d3["chain_ratio"] == 12.5
    assert [(e["level"], e["rows"], e["matches"]) for e in rep["by_level"]] == [(0, 12, 7), (1, 8, 6), (2, 8, 5), (3, 8, 4)]
    assert rep["by_level"][1]["accuracy"] == 75.0
    m = rep["mistakes"]["test_top1"]
    assert m["histogram"] == {"0": 3, "2": 4, "5": 4} and m["unknown"] == 1
    assert m["mean_distance"] == pytest.approx(28 / 11, rel=1e-12) and m["mean_distance_wrong"] == pytest.approx(28 / 8, rel=1e-12)
    a = rep["mistakes"]["all_top1"]
    assert a["histogram"] == {"0": 12} and a["unknown"] == 0 and a["mean_distance"] == 0.0
    assert a["mean_distance_wrong"] is None                                    # no row wrong: no division by zero
    h = rep["height_at_k"]
    assert h["1"]["per_row"] == 1.5 and h["1"]["per_prediction"] == 1.5
    assert h["20"]["per_row"] == pytest.approx(470 / 12, rel=1e-12) and h["20"]["per_prediction"] == pytest.approx(470 / 240, rel=1e-12)
    assert evaluate.report_from_table(_hand_table(), k=5)["height_at_k"]["20"]["per_prediction"] == pytest.approx(470 / 60, rel=1e-12)
    import json
    assert json.loads(json.dumps(rep)) == rep                                  # plain Python values
    assert "depth" in evaluate.format_report(rep)


def test_empty_table_converts():
    rep = evaluate.report_from_table(torch.zeros(ops.REPORT_LEN, dtype=torch.int64))
    assert rep["num_sample"] == 0 and rep["by_depth"] == [] and rep["by_level"] == []
    assert rep["mistakes"]["test_top1"]["mean_distance"] is None and rep["height_at_k"]["5"]["per_row"] is None


# ---- two "ranks" -----------------------------------------------------------------------------------------------------------------------
def _count_rows(rows):
    """A table from (L, first hit position or None, anc_hit, matched positions as bits, chain, dist_test, dist_all, heights[20]) rows:
    what the kernel adds for a row, written down per row (the kernel itself is checked on the GPU)."""
    t = torch.zeros(ops.REPORT_LEN, dtype=torch.int64)
    for L, j, anc, mm, chain, dt, da, hs in rows:
        hit = {f"hit@{k}": int(j is not None and j < k) for k in evaluate.TOPK}
        point = bin(mm).count("1")
        edge = (mm & 1) if L == 1 else bin(mm & (mm >> 1)).count("1")
        _depth(t, L, rows=1, anc_hit=anc, point=point, edge=edge, chain=chain, **hit)
        for i in range(L):
            t[ops.REPORT_LEVEL + 2 * i] += 1
            t[ops.REPORT_LEVEL + 2 * i + 1] += (mm >> i) & 1
        t[ops.REPORT_DIST_TEST + dt] += 1
        t[ops.REPORT_DIST_ALL + da] += 1
        for i, k in enumerate(ops.REPORT_HEIGHT_K):
            t[ops.REPORT_HEIGHT + i] += sum(hs[:k])
    return t


def test_tables_of_two_ranks_sum_to_the_table_of_the_whole_run():
    import random
    rng = random.Random(3)
    rows = []
    for _ in range(57):
        L = rng.choice((1, 2, 5, 32))
        rows.append((L, rng.choice((None, 0, 1, 4, 9, 19)), rng.randint(0, 1), rng.getrandbits(L), rng.randint(0, 1),
                     rng.choice((0, 1, 2, 7, 64, 65)), rng.choice((0, 3, 65)), [rng.randint(0, L) for _ in range(20)]))
    a, b, whole = _count_rows(rows[:20]), _count_rows(rows[20:]), _count_rows(rows)
    assert torch.equal(a + b, whole)
    assert evaluate.report_from_table(a + b) == evaluate.report_from_table(whole)
    assert evaluate.report_from_table(whole)["num_sample"] == 57


def test_report_table_sums_over_a_gloo_group(tmp_path):
    """Evaluator.report_table(group) on CPU tensors over gloo: world size 1 is enough to run the all-reduce path (the int64 sum)."""
    import types
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        ev = evaluate.Evaluator.__new__(evaluate.Evaluator)
        ev.model = types.SimpleNamespace()
        ev.report = _hand_table()
        got = ev.report_table(dist.group.WORLD)
        assert got.dtype == torch.int64 and torch.equal(got, _hand_table())
        assert ev.report_dict(dist.group.WORLD) == evaluate.report_from_table(_hand_table())
    finally:
        dist.destroy_process_group()


def test_parser_has_hier_report_off_by_default():
    from hgr_net_amd import main
    assert main.build_parser().parse_args([]).hier_report is None
    assert main.build_parser().parse_args(["--hier_report", "rep.json"]).hier_report == "rep.json"
