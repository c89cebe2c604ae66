"""Zero-shot evaluation loop: what the reference's ``main.test`` computes (main.py:104-222), with
the per-level masking moved off the host.

Per batch the reference does, on the host, L x (Python set difference over all N nodes, list ->
tensor -> .cuda(), a [B, N] clone + index_fill + gather + topk) and an O(B.L) Python loop of 0-dim
tensor compares.  Here one batch is: the forward (libhgr GEMMs), two top-k
launches, ONE level-segmented arg-max launch that yields every depth level at once, and a handful of
tiny tensor ops on [B, 20] / [B, L] integer arrays; counters stay on the device and are read once.
Outputs (counter values and the printed string) are identical to the reference's.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, Optional

import torch

from . import ops
from .utils import count_acc

TOPK = (1, 2, 5, 10, 20)
COUNTERS = ["hits@1", "hits@2", "hits@5", "hits@10", "hits@20", "hits_all", "path_all", "point_all", "num_sample"]
DECODES = ("flat", "path")
# the weights of path decoding: tree_model.get_weights' methods, and "self" (all weight on the node itself: path scores = logits)
DECODE_WEIGHTS = ("equal", "increasing", "decreasing", "nl_increasing", "nl_decreasing", "adaptive", "self")


@torch.no_grad()
def path_weight_table(model, method: str) -> torch.Tensor:
    """The weight table of hgr_path_scores, fp32 [ops.PATH_MAXL + 1, ops.PATH_MAXL] on the model's device: row L, for every path
    length L = 1 .. max_depth + 1 of the model's hierarchy, is ``model.get_weights(method, L)`` bit for bit (column 0 = the top-most
    ancestor, column L - 1 = the node itself); every other entry is 0.  ``"self"`` - one-hot at column L - 1 - exists here only: it
    is no training weighting.  ``"adaptive"`` is made from ``model.layer_weight`` by tensor operations, without a host read."""
    if method not in DECODE_WEIGHTS:
        raise ValueError(f"decode_weights {method!r}: one of {DECODE_WEIGHTS}")
    if method == "adaptive" and not hasattr(model, "layer_weight"):
        raise ValueError("decode_weights 'adaptive' needs a model built with opts.weights == 'adaptive' (model.layer_weight)")
    dev = model.train_index.device
    n_rows = model.max_depth + 1
    assert n_rows <= ops.PATH_MAXL, "a path holds at most 32 nodes"
    tab = torch.zeros((ops.PATH_MAXL + 1, ops.PATH_MAXL), dtype=torch.float32, device=dev)
    for L in range(1, n_rows + 1):
        if method == "self":
            tab[L, L - 1] = 1.0
        else:
            tab[L, :L] = model.get_weights(method, L).detach().to(device=dev, dtype=torch.float32)
    return tab


class Evaluator:
    def __init__(self, model, report: bool = False, decode: str = "flat", decode_weights: str = "increasing", hedge=None,
                 hedge_temperature: Optional[float] = None, sets=None):
        """``decode``: what the predictions are taken from - "flat": the logits (the reference); "path": the path scores of
        hgr_path_scores, every node scored by the ``decode_weights``-weighted logits along its root-to-node path.  Everything behind
        hgr_eval_rows (counters, report, packed batches, all-reduces) is the same for both.
        ``hedge``: 1..8 thresholds in (0, 1], strictly increasing - hedged predictions (hgr_subtree_hedge on what hgr_eval_rows gets,
        candidates = the test classes; hgr_hedge_counters_rows behind the counters), read with hedge_table() / hedge_dict().
        ``hedge_temperature``: the softmax's, default the model's ``logit_scale.exp()``, read once here.
        ``sets``: an ordered mapping name -> node ids, 1..16 candidate sets scored in the same run (hgr_set_ranks on what
        hgr_eval_rows gets, hgr_set_counters_rows behind the counters), read with sets_table() / sets_dict().  A row counts in a set
        when its class is a member; its hits are the rank of its class among the set's columns, its hit / path / point ratios come
        from the train columns like the main counters' - per set, what a model built with that set as candidates_test counts."""
        if decode not in DECODES:
            raise ValueError(f"decode {decode!r}: one of {DECODES}")
        thr = None if hedge is None else ops.hedge_thresholds(hedge)          # ValueError before anything is allocated
        if hedge is not None and hedge_temperature is not None and not (0.0 < float(hedge_temperature) < float("inf")):
            raise ValueError(f"hedge_temperature {hedge_temperature!r}: finite, > 0")
        if sets is not None:
            sets = ops.check_sets(sets, len(model.nodes))                      # ValueError before anything is allocated
        self.model = model
        self.decode = decode
        # path decoding: the weight table, made once, and one scores buffer, grown to the largest batch seen; flat: nothing extra
        self._wtab = path_weight_table(model, decode_weights) if decode == "path" else None
        self._scores = None
        dev = model.train_index.device
        self.acc = torch.zeros(len(COUNTERS), dtype=torch.float64, device=dev)
        # the hierarchy report (hgr_eval_report_rows): an int64 table advanced beside the counters, or None = nothing extra is launched
        self.report = torch.zeros(ops.REPORT_LEN, dtype=torch.int64, device=dev) if report else None
        # hedged predictions: thresholds (fixed point, on the device), temperature, the int64 outcome table [T, HEDGE_COLS] and the pick
        # buffers of the current batch (grown to the largest batch seen) - or None = nothing is allocated, nothing extra is launched
        self.hedge = None if hedge is None else tuple(float(t) for t in hedge)
        self.hedge_temperature = self._hedge_thr = self.hedge_tab = self._hedge_pick = None
        if thr is not None:
            self.hedge_temperature = float(model.clip_model.logit_scale.detach().exp()) if hedge_temperature is None else float(hedge_temperature)
            self._hedge_thr = torch.tensor(thr, dtype=torch.int32).to(dev)
            self.hedge_tab = torch.zeros((len(thr), ops.HEDGE_COLS), dtype=torch.int64, device=dev)
        self.n_levels = model.max_depth + 1
        self.index = ops.EvalIndex(model.depth32, model.train_index32, model.test_index32, self.n_levels)   # dense per-column maps, built once
        # candidate sets: the per-column maps, the int64 table [S, 33, SETS_COLS] and the rank / top-1 buffers of the current batch (grown
        # to the largest batch seen) - or None = nothing is allocated, nothing extra is launched
        self.sets = self.sets_tab = self._sets_buf = None
        if sets is not None:
            self.sets = ops.SetIndex(self.index, sets)
            self.sets_tab = torch.zeros((self.sets.n_sets, ops.REPORT_MAXL + 1, ops.SETS_COLS), dtype=torch.int64, device=dev)
        self._anc = None         # ancestor paths of every node as a device CSR (see _ancestor_tables)
        self._plan = None        # level-sorted class matrix of the fused logits + evaluation kernel, built on first use

    def _ancestor_tables(self):
        """Every node's path (its ancestors + itself, main.py:163) and the depth of each node on it (main.py:164) as ONE
        device-resident CSR, uploaded once: a new batch's target then costs two tensor views, not three pageable H2D
        copies - those are stream-ordered behind the forward just launched, so each one stalled the host until the step
        had finished and exposed the next step's launch latency (0.3 ms of a 6.3 ms step at ViT-B/32, batch 512)."""
        if self._anc is None:
            m = self.model
            keys = sorted(m.c2p.keys()) if isinstance(m.c2p, dict) else list(range(len(m.c2p)))
            ptr, nodes, levels, off = {}, [], [], 0
            for t in keys:
                path = list(m.c2p[t]) + [t]
                ptr[t] = (off, len(path))
                nodes.extend(path)
                levels.extend(len(m.c2p[q]) for q in path)
                off += len(path)
            dev = m.train_index.device
            lv = torch.tensor(levels, dtype=torch.int64)
            self._anc = (ptr, torch.tensor(nodes, dtype=torch.int32).to(dev), lv.to(dev), lv.to(torch.int32).to(dev))
            # the same CSR with its pointer array on the device, for batches of mixed classes (hgr_eval_counters_rows reads the
            # path of every row's own target): int32 [n_nodes + 1]; a node absent from c2p gets an empty range = a padding row
            n_nodes = len(m.nodes)
            starts, off = [0] * (n_nodes + 1), 0
            for t in range(n_nodes):
                starts[t] = off
                o, n = ptr.get(t, (off, 0))
                assert n == 0 or (o == off and n <= 32), "paths are laid out in node order, at most 32 nodes long"
                off += n
            starts[n_nodes] = off
            self._anc_ptr = torch.tensor(starts, dtype=torch.int32).to(dev)
        return self._anc

    def _ancestor_csr(self):
        """(anc_ptr [n_nodes + 1], anc_nodes, anc_levels) int32 on the device: the operands of hgr_eval_counters_rows."""
        _, nodes, _, lv32 = self._ancestor_tables()
        return self._anc_ptr, nodes, lv32

    def _parents(self, target: int):
        ptr, nodes, lv64, lv32 = self._ancestor_tables()
        o, n = ptr[target]
        return nodes[o:o + n], lv64[o:o + n], lv32[o:o + n], n

    # ---- scoring: two scorers x three routes -----------------------------------------------------------------------------------------
    # A scorer is (score(lv, p1, pred, pick=None), [tensors score reads that this batch made], view(lv)): score advances the counters and, directly
    # behind them on the same stream, the report (if kept); view gives the level output the caller gets back.  Scorers are built on the
    # CALLER's stream before anything of the step is launched: whatever they make there (converted targets, the report's row targets,
    # the first upload of the ancestor CSR) is ordered ahead of the head, hence ahead of the tail that reads it.
    @staticmethod
    def _row_targets(targets: torch.Tensor) -> torch.Tensor:
        return (targets if targets.dtype == torch.int64 else targets.to(torch.int64)).contiguous().view(-1)

    def _class_scorer(self, target: int, targets: Optional[torch.Tensor], like: torch.Tensor):
        """One class for every row of the batch ``like`` (hgr_eval_counters); ``targets``: the same class per row, if the caller has it."""
        parents, levels64, levels32, _ = self._parents(target)
        tg = None if targets is None else self._row_targets(targets)
        rt = csr = None
        if self.report is not None or self.hedge is not None or self.sets is not None:    # all three score rows: without targets, ``target`` for every row
            rt = tg if tg is not None else torch.full((like.shape[0],), int(target), dtype=torch.int64, device=like.device)
            csr = self._ancestor_csr()

        def score(lv, p1, pred, pick=None, set_rank=None):
            ops.eval_counters(pred, tg, int(target), p1.view(-1), lv, parents, levels32, self.acc)
            if self.report is not None:
                ops.eval_report_rows(pred, rt, p1.view(-1), lv, *csr, self.report)
            if pick is not None:
                ops.hedge_counters_rows(pick, rt, csr[0], csr[1], self.hedge_tab)
            if set_rank is not None:
                ops.set_counters_rows(set_rank, self._sets_top1(p1), rt, lv, *csr, self.sets_tab)
        score.row_targets = rt
        return score, [t for t in (tg, rt) if t is not None], lambda lv: lv[:, levels64]        # dict_path [B, L]

    def _rows_scorer(self, targets: torch.Tensor):
        """Every row against the path of its own class (hgr_eval_counters_rows); the paths differ per row, so there is no dict_path view."""
        tg = self._row_targets(targets)
        csr = self._ancestor_csr()

        def score(lv, p1, pred, pick=None, set_rank=None):
            ops.eval_counters_rows(pred, tg, p1.view(-1), lv, *csr, self.acc)
            if self.report is not None:
                ops.eval_report_rows(pred, tg, p1.view(-1), lv, *csr, self.report)
            if pick is not None:
                ops.hedge_counters_rows(pick, tg, csr[0], csr[1], self.hedge_tab)
            if set_rank is not None:
                ops.set_counters_rows(set_rank, self._sets_top1(p1), tg, lv, *csr, self.sets_tab)
        score.row_targets = tg
        return score, [tg], lambda lv: lv

    def _join_tail(self) -> None:
        """Counters and report may still be in flight on the tail stream of earlier pipelined batches: order this stream behind them."""
        if hasattr(self.model, "join_tail"):
            self.model.join_tail()

    def _fused_plan(self) -> "ops.LogitsEvalPlan":
        if self._plan is None:
            self._plan = ops.LogitsEvalPlan(self.index)
        return self._plan

    def path_scores(self, logits: torch.Tensor) -> torch.Tensor:
        """hgr_path_scores of ``logits`` [B, >= N] with this Evaluator's weight table, into its scores buffer: valid until the next
        batch.  One launch; the ancestor CSR is the report's."""
        assert self._wtab is not None, "Evaluator(model, decode='path') keeps the weight table"
        rows, n = logits.shape[0], self.index.n_nodes
        if self._scores is None or self._scores.numel() < rows * n or self._scores.device != logits.device:
            self._scores = torch.empty(rows * n, dtype=torch.float32, device=logits.device)
        ptr, nodes, _ = self._ancestor_csr()
        return ops.path_scores(logits, ptr, nodes, self._wtab, out=self._scores[:rows * n].view(rows, n))

    def hedge_picks(self, scores: torch.Tensor, mass_out: Optional[torch.Tensor] = None):
        """hgr_subtree_hedge of ``scores`` [B, >= N] (what hgr_eval_rows gets) with this Evaluator's thresholds and temperature over
        the test classes, into its pick buffers: (pick int32 [B, T], pick_mass fp32 [B, T]), valid until the next batch."""
        assert self.hedge is not None, "Evaluator(model, hedge=(...)) keeps the thresholds"
        rows, t = scores.shape[0], len(self.hedge)
        if self._hedge_pick is None or self._hedge_pick[0].numel() < rows * t or self._hedge_pick[0].device != scores.device:
            self._hedge_pick = (torch.empty(rows * t, dtype=torch.int32, device=scores.device),
                                torch.empty(rows * t, dtype=torch.float32, device=scores.device))
        ptr, nodes, _ = self._ancestor_csr()
        pick, pmass = (b[:rows * t].view(rows, t) for b in self._hedge_pick)
        return ops.subtree_hedge(scores, self.index.test_pos, ptr, nodes, self.hedge_temperature, self._hedge_thr, pick, pmass, mass_out)

    def set_ranks(self, scores: torch.Tensor, targets: Optional[torch.Tensor] = None):
        """hgr_set_ranks of ``scores`` [B, >= N] (what hgr_eval_rows gets) for this Evaluator's candidate sets, into its buffers:
        (rank int32 [B, S] or None without targets, top1 int32 [B, S]), valid until the next batch."""
        assert self.sets is not None, "Evaluator(model, sets={...}) keeps the candidate sets"
        rows, s = scores.shape[0], self.sets.n_sets
        if self._sets_buf is None or self._sets_buf.numel() < 3 * rows * s or self._sets_buf.device != scores.device:
            self._sets_buf = torch.empty(3 * rows * s, dtype=torch.int32, device=scores.device)
        rank, top1 = (self._sets_buf[i * rows * s:(i + 1) * rows * s].view(rows, s) for i in range(2))
        return ops.set_ranks(scores, self.sets, targets, rank if targets is not None else None, top1)

    def _sets_top1(self, p1: torch.Tensor) -> torch.Tensor:
        """The prediction whose ancestor hits every set counts: the top-1 over the TRAIN columns (main.py:157-160), the same for every
        set like the level arg-maxes - hgr_set_counters_rows takes one prediction per row and set, so it is repeated per set."""
        rows, s = p1.numel(), self.sets.n_sets
        out = self._sets_buf[2 * rows * s:3 * rows * s].view(rows, s)          # behind this batch's rank and top-1 (set_ranks sized it)
        out.copy_(p1.view(-1, 1).expand(rows, s))
        return out

    def _add_logits(self, logits: torch.Tensor, scorer, want_outputs: bool):
        score, _, view = scorer
        self._join_tail()
        if self.decode == "path":                      # path decoding IS hgr_eval_rows on the path scores
            logits = self.path_scores(logits)
        lv, p1, pred = ops.eval_rows(logits, self.index, max(TOPK))
        # the hedge and the candidate sets read the tensor hgr_eval_rows got: both compose with the two decodings
        pick = None if self.hedge is None else self.hedge_picks(logits)[0]
        set_rank = None if self.sets is None else self.set_ranks(logits, score.row_targets)[0]
        if pick is None and set_rank is None:
            score(lv, p1, pred)
        else:
            score(lv, p1, pred, pick, set_rank)
        return (pred, view(lv)) if want_outputs else None

    def _add_images(self, imgs: torch.Tensor, scorer, want_outputs: bool):
        score, reads, view = scorer
        if self.decode == "path" or self.hedge is not None or self.sets is not None:     # the fused kernel never has the whole row: logits -> (path scores, hedge, sets) -> hgr_eval_rows
            return self._add_logits(self.model(imgs, None, static_output=True), scorer, want_outputs)
        plan = self._fused_plan()
        if not plan.supported:                        # a hierarchy beyond hgr_logits_eval's capacity: logits + hgr_eval_rows
            return self._add_logits(self.model(imgs), scorer, want_outputs)
        if not want_outputs and hasattr(self.model, "forward_eval_overlapped"):
            # the loop's own route: the step as a two-stage pipeline (the class-token tail of this batch beside the next batch's tower);
            # score runs on the tail's stream, so what it reads must outlive this call there; counters() / summary() join that stream
            side = self.model._pipe_state(imgs.device).side
            for t in reads:
                t.record_stream(side)
            if self.model.forward_eval_overlapped(imgs, plan, max(TOPK), score):
                return None
        self._join_tail()
        lv, p1, pred = self.model.forward_eval(imgs, plan, max(TOPK))
        score(lv, p1, pred)
        return (pred, view(lv)) if want_outputs else None

    @torch.no_grad()
    def add_batch(self, logits: torch.Tensor, target: int, targets: Optional[torch.Tensor] = None, want_outputs: bool = True):
        """One iteration of main.py:131-191 on device.  ``target`` = the batch's single class
        (every batch is one group).  Two launches: hgr_eval_rows (top-20 over the test columns :136-139,
        top-1 over the train columns :157, arg-max per depth level :162-176) and hgr_eval_counters (hits, hit / path /
        point ratios :139-148,157-160,177-191).  Returns (pred_top20, dict_path) int32 tensors unless ``want_outputs``
        is False (the evaluation loop itself does not need them)."""
        return self._add_logits(logits, self._class_scorer(target, targets, logits), want_outputs)

    @torch.no_grad()
    def add_batch_rows(self, logits: torch.Tensor, targets: torch.Tensor, want_outputs: bool = False):
        """add_batch for a batch packed from SEVERAL classes (dataset.packing): ``targets`` int64 [B] on the device names every row's
        own class, and hgr_eval_counters_rows scores each row against that class's path (the reference's counters are row-additive,
        main.py:139-191).  Rows with a target outside [0, n_nodes) are padding and count nothing.  Returns (pred_top20, level
        arg-max [B, n_levels]) with ``want_outputs``; the paths differ per row, so there is no dict_path view."""
        return self._add_logits(logits, self._rows_scorer(targets), want_outputs)

    def fused_ok(self) -> bool:
        """hgr_logits_eval needs an embedding width that is a multiple of 128 (<= 1024) and <= 32 levels - and flat decoding: the path
        scores of a column read other columns of its row, which the fused kernel never holds together; so do the softmax of a hedge and the ranks of
        the candidate sets."""
        if self.decode == "path" or self.hedge is not None or self.sets is not None:
            return False
        d = self.model._zsl16.shape[1] if self.model._zsl16 is not None else 0
        if not (d % 128 == 0 and 128 <= d <= 1024 and self.n_levels <= 32 and self.index.n_test >= max(TOPK)):
            return False
        return self._fused_plan().supported          # <= 32 768 level-padded columns

    @torch.no_grad()
    def add_images(self, imgs: torch.Tensor, target: int, targets: Optional[torch.Tensor] = None, want_outputs: bool = False):
        """One iteration of main.py:131-191 WITHOUT materialising the logits: image tower -> L2 norm -> hgr_logits_eval (the
        class-logits GEMM with top-20 / top-1 / per-level arg-max in its epilogue) -> hgr_eval_counters.  Same counters, bit for
        bit, as add_batch(model(imgs), ...); use add_batch when the caller needs the logits themselves."""
        return self._add_images(imgs, self._class_scorer(target, targets, imgs), want_outputs)

    @torch.no_grad()
    def add_images_rows(self, imgs: torch.Tensor, targets: torch.Tensor, want_outputs: bool = False):
        """add_images for a batch packed from SEVERAL classes: the same three routes (two-graph pipeline, single graph, logits +
        hgr_eval_rows for a hierarchy beyond hgr_logits_eval's capacity), with hgr_eval_counters_rows in the place of
        hgr_eval_counters.  Same counters as add_batch_rows(model(imgs), targets)."""
        return self._add_images(imgs, self._rows_scorer(targets), want_outputs)

    def counters(self, group=None) -> Dict[str, float]:
        """Read the counters (one D2H copy); with a process group, all-reduce(sum) them first."""
        self._join_tail()                               # pipelined steps advance the counters on the tail stream
        acc = self.acc
        if group is not None:
            import torch.distributed as dist
            acc = acc.clone()
            from .parallel import native_comm
            nc = native_comm() if acc.is_cuda else None
            if nc is not None:
                nc.allreduce(acc)                        # hgr_allreduce (fp64 sum) on the current stream
            else:
                dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
        return dict(zip(COUNTERS, acc.cpu().tolist()))

    def summary(self, group=None) -> str:
        """The string main.test prints and logs (main.py:205-216)."""
        c = self.counters(group)
        tripped = getattr(self.model.clip_model, "ln_guard_tripped", lambda: {})()
        if tripped:                                        # activations left the guarded 16-bit range AFTER the first-pass check
            import warnings
            warnings.warn(f"hgr_net_amd: LayerNorm-folding range guard tripped during this evaluation {tripped}: rerun with HGR_LN_FUSED=0")
        return "\n" + metric_text(c)

    def report_table(self, group=None) -> torch.Tensor:
        """The hierarchy report's table as a CPU int64 tensor [ops.REPORT_LEN] (one D2H copy); with a process group the tables of
        all ranks are summed first - an int64 all-reduce, exact, on the device (nccl) as on CPU tensors (gloo)."""
        assert self.report is not None, "Evaluator(model, report=True) keeps the hierarchy report"
        return self._read_table(self.report, group)

    def _read_table(self, table: torch.Tensor, group) -> torch.Tensor:
        self._join_tail()                               # pipelined steps advance the tables on the tail stream
        if group is not None:
            import torch.distributed as dist
            table = table.clone()
            dist.all_reduce(table, op=dist.ReduceOp.SUM, group=group)
        return table.cpu()

    def hedge_table(self, group=None) -> torch.Tensor:
        """The hedge outcome table as a CPU int64 tensor [T, ops.HEDGE_COLS] (one D2H copy); with a process group summed over the
        ranks first, through the int64 all-reduce of report_table."""
        assert self.hedge_tab is not None, "Evaluator(model, hedge=(...)) keeps the hedge table"
        return self._read_table(self.hedge_tab, group)

    def sets_table(self, group=None) -> torch.Tensor:
        """The candidate sets' table as a CPU int64 tensor [S, ops.REPORT_MAXL + 1, ops.SETS_COLS] (one D2H copy); with a process group
        summed over the ranks first, through the int64 all-reduce of report_table."""
        assert self.sets_tab is not None, "Evaluator(model, sets={...}) keeps the candidate sets' table"
        return self._read_table(self.sets_tab, group)

    def sets_dict(self, group=None) -> dict:
        """The candidate sets' results as plain Python values (sets_from_table), ready for json.dump."""
        return sets_from_table(self.sets_table(group), self.sets.names, self.sets.sizes)

    def hedge_dict(self, group=None) -> dict:
        """The hedge outcomes as plain Python values (hedge_from_table), ready for json.dump."""
        return hedge_from_table(self.hedge_table(group), self.hedge, temperature=self.hedge_temperature)

    def report_dict(self, group=None) -> dict:
        """The hierarchy report as plain Python values (report_from_table), ready for json.dump."""
        return report_from_table(self.report_table(group), k=max(TOPK))


def metric_text(c: Dict[str, float]) -> str:
    """The metric line of main.test (main.py:205-214, without its leading newline) from the nine counters."""
    n = c["num_sample"]
    s, _ = count_acc({k: c[f"hits@{k}"] for k in TOPK}, n)
    s += " hit_ratio(%):{:.2f}".format(c["hits_all"] / n * 100.0)
    s += " path_ratio(%):{:.2f}".format(c["path_all"] / n * 100.0)
    s += " point_ratio(%):{:.2f}".format(c["point_all"] / n * 100.0)
    return s


def _mistakes(hist) -> dict:
    """One distance histogram [ops.REPORT_DIST_BINS] -> counts, the rows without a distance ("unknown": the prediction has no path
    of 1..32 nodes) and the mean tree distance over the rows that have one and over the wrong ones among them (None without any)."""
    known = hist[:ops.REPORT_DIST_UNKNOWN]
    n, total = sum(known), sum(d * c for d, c in enumerate(known))
    wrong = n - known[0]
    return {"histogram": {str(d): c for d, c in enumerate(known) if c}, "unknown": hist[ops.REPORT_DIST_UNKNOWN],
            "mean_distance": total / n if n else None, "mean_distance_wrong": total / wrong if wrong else None}


def report_from_table(table: torch.Tensor, k: int = max(TOPK)) -> dict:
    """The table of hgr_eval_report_rows (CPU int64 [ops.REPORT_LEN], layout in include/hgr.h) as plain Python values; a pure
    function of the table.  Depths (= path length - 1) and levels without rows are left out.  The ratios are those of
    Evaluator.summary() restricted to a depth: hits / rows, anc_hit / rows, edge / (L - 1) / rows (edge / rows at L = 1),
    point / L / rows, all in percent.  ``k`` = the number of predictions per row the table was counted with (height_at_k averages
    over min(K, k) predictions)."""
    assert table.dtype == torch.int64 and table.numel() == ops.REPORT_LEN and not table.is_cuda
    t = table.view(-1).tolist()
    cols = ops.REPORT_DEPTH_COLS
    by_depth, num_sample = [], 0
    for L in range(1, ops.REPORT_MAXL + 1):
        row = dict(zip(cols, t[ops.REPORT_DEPTH + L * len(cols):ops.REPORT_DEPTH + (L + 1) * len(cols)]))
        n = row["rows"]
        if n == 0:
            continue
        num_sample += n
        e = {"depth": L - 1, "rows": n}
        for kk in TOPK:
            e[f"hits@{kk}"] = row[f"hit@{kk}"]
            e[f"acc@{kk}"] = row[f"hit@{kk}"] / n * 100.0
        e["hit_ratio"] = row["anc_hit"] / n * 100.0
        e["path_ratio"] = row["edge"] / max(L - 1, 1) / n * 100.0
        e["point_ratio"] = row["point"] / L / n * 100.0
        e["chain_ratio"] = row["chain"] / n * 100.0
        by_depth.append(e)
    by_level = []
    for i in range(ops.REPORT_MAXL):
        n, m = t[ops.REPORT_LEVEL + 2 * i], t[ops.REPORT_LEVEL + 2 * i + 1]
        if n:
            by_level.append({"level": i, "rows": n, "matches": m, "accuracy": m / n * 100.0})
    height = {}
    for i, kk in enumerate(ops.REPORT_HEIGHT_K):
        h = t[ops.REPORT_HEIGHT + i]
        height[str(kk)] = {"sum": h, "per_row": h / num_sample if num_sample else None,
                           "per_prediction": h / (num_sample * min(kk, k)) if num_sample else None}
    return {"num_sample": num_sample, "by_depth": by_depth, "by_level": by_level,
            "mistakes": {"test_top1": _mistakes(t[ops.REPORT_DIST_TEST:ops.REPORT_DIST_TEST + ops.REPORT_DIST_BINS]),
                         "all_top1": _mistakes(t[ops.REPORT_DIST_ALL:ops.REPORT_DIST_ALL + ops.REPORT_DIST_BINS])},
            "height_at_k": height}


def format_report(rep: dict) -> str:
    """The short per-depth table evaluate.test prints beside the report file."""
    lines = ["depth     rows  acc@1(%)  acc@5(%)  hit(%)  path(%)  point(%)  chain(%)"]
    for e in rep["by_depth"]:
        lines.append("{:5d} {:8d}  {:8.2f}  {:8.2f}  {:6.2f}  {:7.2f}  {:8.2f}  {:8.2f}".format(
            e["depth"], e["rows"], e["acc@1"], e["acc@5"], e["hit_ratio"], e["path_ratio"], e["point_ratio"], e["chain_ratio"]))
    for name in ("test_top1", "all_top1"):
        m = rep["mistakes"][name]
        if m["mean_distance_wrong"] is not None:
            lines.append("{}: mean tree distance of a wrong prediction {:.2f} ({} without a path)".format(name, m["mean_distance_wrong"], m["unknown"]))
    return "\n".join(lines)


def hedge_from_table(table: torch.Tensor, thresholds, temperature: Optional[float] = None) -> dict:
    """The table of hgr_hedge_counters_rows (CPU int64 [T, ops.HEDGE_COLS], layout in include/hgr.h) as plain Python values; a pure
    function of the table.  Per threshold: the rows, the five outcomes as counts and as percentages of the rows (None without rows),
    correct = abstain + exact + ancestor (a pick that names the target or something above it says nothing wrong), the mean pick depth
    SUM_LPICK / ROWS (path length: 0 = abstained), hierarchical precision SUM_COMMON / SUM_LPICK (None when nothing was picked) and
    recall SUM_COMMON / SUM_LT, and the histogram of the picks' path lengths with empty bins left out."""
    thresholds = [float(t) for t in thresholds]
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(thresholds), ops.HEDGE_COLS) and not table.is_cuda
    out = []
    for theta, row in zip(thresholds, table.tolist()):
        c = dict(zip(ops.HEDGE_COL_NAMES, row))
        n = c["rows"]
        e = {"threshold": theta, "rows": n}
        for name in ("abstain", "exact", "ancestor", "below", "wrong"):
            e[name] = c[name]
            e[name + "_pct"] = c[name] / n * 100.0 if n else None
        e["correct"] = c["abstain"] + c["exact"] + c["ancestor"]
        e["correct_pct"] = e["correct"] / n * 100.0 if n else None
        e["mean_pick_depth"] = c["sum_lpick"] / n if n else None
        e["h_precision"] = c["sum_common"] / c["sum_lpick"] if c["sum_lpick"] else None
        e["h_recall"] = c["sum_common"] / c["sum_lt"] if c["sum_lt"] else None
        e["pick_depth_histogram"] = {str(d): v for d, v in enumerate(row[ops.HEDGE_COL_HIST:]) if v}
        out.append(e)
    rep = {"thresholds": thresholds, "by_threshold": out}
    if temperature is not None:
        rep["temperature"] = float(temperature)
    return rep


def format_hedge(rep: dict) -> str:
    """One line per threshold: what evaluate.test prints behind the metric string."""
    def f(v, spec):
        return format(v, spec) if v is not None else "-".rjust(int(spec.split(".")[0]))
    lines = ["hedge theta     rows  abstain(%)  exact(%)  ancestor(%)  below(%)  wrong(%)  correct(%)  depth  h_prec  h_rec"]
    for e in rep["by_threshold"]:
        lines.append("hedge {:5.3f} {:8d}  {}  {}  {}  {}  {}  {}  {}  {}  {}".format(
            e["threshold"], e["rows"], f(e["abstain_pct"], "10.2f"), f(e["exact_pct"], "8.2f"), f(e["ancestor_pct"], "11.2f"),
            f(e["below_pct"], "8.2f"), f(e["wrong_pct"], "8.2f"), f(e["correct_pct"], "10.2f"), f(e["mean_pick_depth"], "5.2f"),
            f(e["h_precision"], "6.3f"), f(e["h_recall"], "5.3f")))
    return "\n".join(lines)


def sets_from_table(table: torch.Tensor, names, sizes) -> dict:
    """The table of hgr_set_counters_rows (CPU int64 [S, ops.REPORT_MAXL + 1, ops.SETS_COLS], layout in include/hgr.h) as plain Python
    values; a pure function of the table.  Per set: its name, ``classes`` (its size), the nine counters of Evaluator.counters() - the
    hits are sums over the path lengths, path_all = sum of edge / (L - 1) (edge at L = 1) and point_all = sum of point / L, one division
    per path length in hgr_eval_counters_rows' order - acc@k and the three ratios in percent (None for a set without rows), and
    ``by_depth`` with report_from_table's formulas (depth = L - 1; depths without rows are left out)."""
    names, sizes = [str(n) for n in names], [int(n) for n in sizes]
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(names), ops.REPORT_MAXL + 1, ops.SETS_COLS) and not table.is_cuda
    assert len(sizes) == len(names)
    out = []
    for name, size, tab in zip(names, sizes, table.tolist()):
        tot = {k: 0 for k in COUNTERS}
        tot["path_all"] = tot["point_all"] = 0.0
        by_depth = []
        for L in range(1, ops.REPORT_MAXL + 1):
            row = dict(zip(ops.SETS_COL_NAMES, tab[L]))
            n = row["rows"]
            tot["path_all"] += row["edge"] / max(L - 1, 1)
            tot["point_all"] += row["point"] / L
            if n == 0:
                continue
            tot["num_sample"] += n
            tot["hits_all"] += row["anc_hit"]
            e = {"depth": L - 1, "rows": n}
            for kk in TOPK:
                tot[f"hits@{kk}"] += row[f"hit@{kk}"]
                e[f"hits@{kk}"] = row[f"hit@{kk}"]
                e[f"acc@{kk}"] = row[f"hit@{kk}"] / n * 100.0
            e["hit_ratio"] = row["anc_hit"] / n * 100.0
            e["path_ratio"] = row["edge"] / max(L - 1, 1) / n * 100.0
            e["point_ratio"] = row["point"] / L / n * 100.0
            by_depth.append(e)
        n = tot["num_sample"]
        e = {"name": name, "classes": size}
        e.update(tot)
        for kk in TOPK:
            e[f"acc@{kk}"] = tot[f"hits@{kk}"] / n * 100.0 if n else None
        for ratio, counter in (("hit_ratio", "hits_all"), ("path_ratio", "path_all"), ("point_ratio", "point_all")):
            e[ratio] = tot[counter] / n * 100.0 if n else None
        e["by_depth"] = by_depth
        out.append(e)
    return {"sets": out}


def format_sets(rep: dict) -> str:
    """One line per candidate set: name, classes and images, then the text Evaluator.summary() makes from the set's counters."""
    lines = []
    for e in rep["sets"]:
        head = "set {} ({} classes, {} images): ".format(e["name"], e["classes"], e["num_sample"])
        lines.append(head + (metric_text(e) if e["num_sample"] else "no images"))
    return "\n".join(lines)


def parse_eval_sets(text):
    """``--eval_sets hop2,hop3,hop3+train`` -> (("hop2", ("hop2",)), ("hop3", ("hop3",)), ("hop3+train", ("hop3", "train"))): the
    names of the candidate sets in their order, each the union of one or more split keys joined by ``+``."""
    if text is None:
        return None
    if not isinstance(text, str):
        return tuple((str(n), tuple(k)) for n, k in text)
    out = []
    for name in (t.strip() for t in text.split(",")):
        keys = tuple(k.strip() for k in name.split("+"))
        if not name or not all(keys):
            raise ValueError(f"--eval_sets {text!r}: comma-separated names, each one split key or several joined by '+'")
        if name in (n for n, _ in out):
            raise ValueError(f"--eval_sets {text!r}: {name!r} is listed twice")
        out.append((name, keys))
    if not 1 <= len(out) <= ops.SETS_MAXS:
        raise ValueError(f"--eval_sets {text!r}: {len(out)} candidate sets (1..{ops.SETS_MAXS})")
    return tuple(out)


def resolve_eval_sets(spec, splits, nodes, extra=None) -> dict:
    """The candidate sets of ``spec`` (parse_eval_sets) as an ordered mapping name -> node ids (positions in ``nodes``): every split
    key is looked up in ``splits`` (--split_path) and in ``extra`` (--eval_sets_file, a second mapping name -> wnids); the ids of a
    union keep the order of its keys, a wnid listed by several of them counts once.  ValueError, naming the offender: a key found in
    neither mapping or in both, a wnid absent from the hierarchy."""
    extra = extra or {}
    both = sorted(set(splits) & set(extra))
    if both:
        raise ValueError(f"--eval_sets_file: key {both[0]!r} is also a key of the split file")
    pos = {w: i for i, w in enumerate(nodes)}
    out = {}
    for name, keys in spec:
        ids, seen = [], set()
        for k in keys:
            if k not in splits and k not in extra:
                raise ValueError(f"--eval_sets: unknown split key {k!r} (known: {sorted(set(splits) | set(extra))})")
            for w in (splits[k] if k in splits else extra[k]):
                if w not in pos:
                    raise ValueError(f"--eval_sets: {w!r} of split {k!r} is not a node of the hierarchy")
                if pos[w] not in seen:
                    seen.add(pos[w])
                    ids.append(pos[w])
        out[name] = ids
    return out


def parse_hedge(text):
    """``--hedge 0.25,0.5,0.9`` -> (0.25, 0.5, 0.9); the values are checked by ops.hedge_thresholds."""
    if text is None or isinstance(text, (tuple, list)):
        return None if text is None else tuple(float(t) for t in text)
    try:
        th = tuple(float(t) for t in str(text).split(","))
    except ValueError:
        raise ValueError(f"--hedge {text!r}: comma-separated numbers") from None
    ops.hedge_thresholds(th)
    return th


@torch.no_grad()
def predict(model, imgs: torch.Tensor, k: int = max(TOPK), decode: str = "flat", decode_weights: str = "increasing",
            want_scores: bool = False, evaluator: Optional[Evaluator] = None, hedge=None, hedge_temperature: Optional[float] = None,
            want_mass: bool = False, sets=None, targets: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Classify a batch of images (after ``model.update_classifier()``): {"topk": int32 [B, k] node ids among the test classes, best
    first, "top1": int32 [B] the best train class, "levels": int32 [B, n_levels] the best train class of every depth level (the
    reference's -1 filler competes, as in hgr_eval_rows)} - hgr_eval_rows on the logits (``decode="flat"``) or on their path scores (``"path"``, weights
    ``decode_weights``).  ``want_scores`` adds "scores": fp32 [B, N], what the predictions were taken from.  ``evaluator``: an
    Evaluator of this model to reuse (its index, weight table and scores buffer; its decode settings then hold) - without one, a
    new one is built per call.  ``hedge`` (thresholds, with ``hedge_temperature``; or an ``evaluator`` built with them) adds "hedge":
    int32 [B, T], per threshold the deepest node whose subtree holds that much of the row's probability among the test classes (-1: none
    does), and "hedge_mass": fp32 [B, T], that node's mass; ``want_mass`` adds "mass": fp32 [B, N], every node's subtree mass.
    ``sets`` (a mapping name -> node ids; or an ``evaluator`` built with it) adds "set_top1": int32 [B, S], the best member of every
    candidate set (-1: an empty set), and with ``targets`` (one class id per row) "set_rank": int32 [B, S], the number of the set's
    members that come before the row's class (-1: the class is no member)."""
    ev = evaluator if evaluator is not None else Evaluator(model, decode=decode, decode_weights=decode_weights, hedge=hedge,
                                                           hedge_temperature=hedge_temperature, sets=sets)
    if want_mass and ev.hedge is None:
        raise ValueError("want_mass needs hedge thresholds")
    scores = model(imgs.to(model.train_index.device), None, static_output=True)
    if ev.decode == "path":
        scores = ev.path_scores(scores)
    lv, p1, topk = ops.eval_rows(scores, ev.index, k)
    out = {"topk": topk, "top1": p1.view(-1), "levels": lv}
    if want_scores:
        out["scores"] = scores[:, :ev.index.n_nodes].clone()          # the logits / the scores buffer are reused by the next batch
    if ev.hedge is not None:
        mass = torch.empty((scores.shape[0], ev.index.n_nodes), dtype=torch.int32, device=scores.device) if want_mass else None
        pick, pmass = ev.hedge_picks(scores, mass)
        out["hedge"], out["hedge_mass"] = pick.clone(), pmass.clone()   # the pick buffers are reused by the next batch
        if want_mass:
            out["mass"] = mass.to(torch.float32) * (1.0 / ops.HEDGE_SCALE)
    if ev.sets is not None:
        tg = None if targets is None else Evaluator._row_targets(torch.as_tensor(targets).to(scores.device))
        rank, top1 = ev.set_ranks(scores, tg)
        out["set_top1"] = top1.clone()                                  # the buffers are reused by the next batch
        if rank is not None:
            out["set_rank"] = rank.clone()
    return out


@torch.no_grad()
def test(opts, model, device, splits=None, loader: Optional[Iterable] = None, group=None, log: bool = True) -> str:
    """Drop-in for the reference's ``test(opts, model, device, splits)`` (main.py:104-222).
    ``loader`` yields the reference's batch dicts {'img': [1,B,3,R,R], 'label': [1,B]}.  With ``opts.pack_batches`` the batches are
    repacked into full ones of ``opts.test_batch_size`` rows of mixed classes (dataset.packing.PackedBatches); same metrics."""
    print("out", opts.out_ratio)
    print("in", opts.in_ratio)
    model.eval()
    model.update_classifier(group=group)
    if loader is None:                                   # main.py:111-114
        print("Loading datasets", flush=True)
        from .dataset import DataManager_test
        data = DataManager_test(opts=opts, split=opts.data_split_test, node_set=model.nodes, candidates=splits[opts.data_test],
                                resolution=model.resolution)
        # ViT towers take the uint8 crops directly (normalisation fused into the patch kernel): a quarter of the bytes
        from .clip.model import VisionTransformer
        v = model.clip_model.visual
        u8_ok = isinstance(v, VisionTransformer) and (3 * v.patch_size ** 2) % 64 == 0
        loader = data.get_data_loader(device=device, output="u8" if u8_ok else "f32",
                                      rank=int(os.environ.get("RANK", "0")) if group is not None else 0,
                                      world_size=int(os.environ.get("WORLD_SIZE", "1")) if group is not None else 1,
                                      workers=getattr(opts, "num_workers", 8))
        print("number of batches:{}".format(loader.batch_sampler.num_batch))
    print("Running.", flush=True)
    report_path = getattr(opts, "hier_report", None)
    decode, decode_weights = getattr(opts, "decode", "flat"), getattr(opts, "decode_weights", "increasing")
    kw = {"report": True} if report_path else {}
    if decode != "flat":
        kw.update(decode=decode, decode_weights=decode_weights)
    hedge, hedge_path = parse_hedge(getattr(opts, "hedge", None)), getattr(opts, "hedge_report", None)
    if hedge is not None:
        kw.update(hedge=hedge, hedge_temperature=getattr(opts, "hedge_temperature", None))
    set_spec, sets_path = parse_eval_sets(getattr(opts, "eval_sets", None)), getattr(opts, "eval_sets_report", None)
    if set_spec is not None:
        extra = getattr(opts, "eval_sets_file", None)
        kw.update(sets=resolve_eval_sets(set_spec, splits or {}, model.nodes, json.load(open(extra)) if extra else None))
    ev = Evaluator(model, **kw)
    fused = ev.fused_ok() and os.environ.get("HGR_EVAL_FUSED", "1") != "0"
    packed = bool(getattr(opts, "pack_batches", False))
    if packed:
        # full batches packed from several classes (dataset.packing): one input shape = one graph generation for the whole run, every
        # row scored against its own class; the labels arrive on the device and are never read on the host
        from .dataset.packing import PackedBatches
        loader = PackedBatches(loader, opts.test_batch_size, device)
    for data in loader:
        if packed:
            imgs, targets = data["img"][0], data["label"][0]
            if fused:
                ev.add_images_rows(imgs, targets)
            else:
                ev.add_batch_rows(model(imgs, None, static_output=True), targets)
            continue
        imgs, targets = data["img"].to(device, non_blocking=True)[0], data["label"].to(device, non_blocking=True)[0]
        target = int(data["label"][0][0])           # host copy of the label: no device sync in the loop
        if fused:                                   # the loop never looks at the logits: GEMM + evaluation in one pass, nothing [B, N] written
            ev.add_images(imgs, target, targets)
            continue
        logits = model(imgs, targets, static_output=True)     # consumed by add_batch before the next forward
        ev.add_batch(logits, target, targets, want_outputs=False)
    print("End of testing.")
    out = ev.summary(group)
    if decode != "flat":
        print("decode: {} ({})".format(decode, decode_weights))
    print(out, flush=True)
    if report_path:                                      # every rank joins the all-reduce, rank 0 writes
        rep = ev.report_dict(group)
        import torch.distributed as dist
        if group is None or dist.get_rank() == 0:
            with open(report_path, "w") as f:
                json.dump(rep, f, indent=1)
            print(format_report(rep), flush=True)
    if hedge is not None:                                # behind the metric string, which stays as it is
        rep = ev.hedge_dict(group)
        import torch.distributed as dist
        if group is None or dist.get_rank() == 0:
            if hedge_path:
                with open(hedge_path, "w") as f:
                    json.dump(rep, f, indent=1)
            print(format_hedge(rep), flush=True)
    if set_spec is not None:                             # one line per candidate set behind the metric string
        rep = ev.sets_dict(group)
        import torch.distributed as dist
        if group is None or dist.get_rank() == 0:
            if sets_path:
                with open(sets_path, "w") as f:
                    json.dump(rep, f, indent=1)
            print(format_sets(rep), flush=True)
    if log:
        with open(model.save_path + "arugements.log", "a") as f:
            f.writelines(out + "\n")
        with open("{}.txt".format(opts.weights), "a") as f:
            f.writelines("{},{},{}:".format(opts.weights, opts.out_ratio, opts.in_ratio) + "\n" + out + "\n")
    return out
