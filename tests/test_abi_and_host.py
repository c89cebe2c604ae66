"""CPU: the C-ABI library loads and exports every symbol include/hgr.h declares (no compute calls
without a GPU), host logic of tree_model / parallel sharding, and a world-size-2 gloo run."""
import json
import os
import time
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    from hgr_net_amd import _lib
    lib = _lib.load()
    header = (ROOT / "include" / "hgr.h").read_text()
    declared = set(re.findall(r"\b(hgr_[a-z0-9_]+)\s*\(", header))
    assert {"hgr_gemm_nt", "hgr_mha", "hgr_layernorm", "hgr_level_argmax", "hgr_topk_rows"} <= declared
    for name in declared:
        assert hasattr(lib, name), f"libhgr.so does not export {name}"
    assert declared - {"hgr_abi_version", "hgr_last_error"} == set(_lib.SIGNATURES), "ctypes table out of sync with hgr.h"
    assert lib.hgr_abi_version() == _lib.ABI_VERSION == 5


def test_gemm_plans_match_golden(tmp_path, golden_dir):
    """Which kernel, tile plan and grid every route of the NT GEMM family takes (hgr_gemm_plan_capture: validated and planned, nothing
    launched, no device needed) against tests/golden/gemm_plans.json.  The table was recorded from the host code BEFORE the plan step
    existed - a scratch build of that commit with a tagged print in front of every launch_* call of hgr_gemm.hip and of the post-adjustment
    grid / total inside launch_duo and launch_p8, run on a machine without a GPU (256 CUs assumed, as on an MI355X) - so it
    pins the routes the GPU parity tests name in their docstrings: the shapes of test_gemm_tail_plan_is_bit_identical,
    test_gemm_res_stats_persistent_is_bit_identical and test_gemm_p8_equals_duo under their switches, the
    ViT-B/32 batch-512 tower launches, the corners of the tail plan and of the cost model, split-K and every branch of the convolution
    ladder.  A changed threshold shows up here instead of silently moving a parity test off the path it was written for.  The library
    reads its environment once, so every environment of the table gets a fresh process, one after another, started without HGR_*
    variables of the caller and with the device hidden: the plan is then the 256-CU one the table holds on any machine, and no
    child opens the GPU."""
    from hgr_net_amd import _lib, ops
    sys.path.insert(0, str(ROOT / "tests" / "workers"))
    try:
        import gemm_plan_replay as replay
    finally:
        sys.path.pop(0)
    assert all(_lib.SIGNATURES[name] == argtypes for name, argtypes in replay.ARGTYPES.items())
    rows = json.loads((golden_dir / "gemm_plans.json").read_text())
    assert 100 < len(rows) < 500 and all(row["launches"] for row in rows)
    got = [None] * len(rows)
    by_env = {}
    for i, row in enumerate(rows):
        by_env.setdefault(json.dumps(row["env"], sort_keys=True), []).append(i)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HGR_")}
    for n, (key, idx) in enumerate(by_env.items()):
        (tmp_path / f"rows{n}.json").write_text(json.dumps([rows[i] for i in idx]))
        child = subprocess.run([sys.executable, replay.__file__, str(_lib.LIB_PATH), str(tmp_path / f"rows{n}.json")], capture_output=True, text=True, timeout=120,
                               env=dict(clean, **json.loads(key), HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES=""))
        assert child.returncode == 0, child.stderr[-2000:]
        for i, launches in zip(idx, json.loads(child.stdout)):
            got[i] = launches
    for row, launches in zip(rows, got):
        assert launches == row["launches"], {k: row[k] for k in ("entry", "args", "knobs", "env")}

    # ops.gemm_plan is the same capture (in this process: whatever card and environment it has); it never leaves the thread armed
    lib, row = _lib.load(), rows[0]
    plan = ops.gemm_plan(lambda: replay.call(lib, row["entry"], row["args"]))
    assert plan and plan == replay.replay(lib, [dict(row, knobs={})])[0]
    with pytest.raises(ZeroDivisionError):
        ops.gemm_plan(lambda: 1 // 0)
    assert lib.hgr_gemm_plan_capture(None, 0) == 0
    with pytest.raises(_lib.HgrError):
        ops.gemm_plan(lambda: None)
    assert lib.hgr_gemm_plan_capture(None, 0) == 0


def test_gemm_32bit_offset_guard_flips_at_4gb():
    """gemm_nt_duo, gemm_nt_p8, the LayerNorm forms and hgr_gemm_nt_ln_mha address their operands with 32-bit byte offsets.
    One step below M * lda * 2 = 2^32 (and N * ldw * 2 = 2^32) hgr_gemm_nt plans them, at the limit it falls back to the 128 / 256
    kernels (64-bit pointers); the entry points that have no other kernel reject the call, and ops.ln_mha_ok / ops.gelu_dual_ok say
    the same as the library on both sides.  With the plan capture armed nothing is launched and no operand is read, and a rejected
    call launches nothing either: a small real tensor with a huge leading dimension is safe."""
    from hgr_net_amd import _lib, ops
    from hgr_net_amd._lib import EPI_BIAS, EPI_NONE, HGR_F16
    lib = _lib.load()
    p = torch.zeros(64, dtype=torch.float16).data_ptr()
    assert p % 16 == 0
    small, narrow = (1, 2), (3, 5)                                     # HGR_KERNEL_128 / _256; _DUO / _P8

    def nt(m, n, k, lda, ldw, epi=EPI_NONE, out32=1):
        return [d["kernel"] for d in ops.gemm_plan(lambda: _lib.call("hgr_gemm_nt", p, lda, p, ldw, p, n, p, p, n, m, n, k, HGR_F16, epi, out32, 0))]

    def limit(rows):                                                   # the smallest leading dimension with rows * ld * 2 >= 2^32, % 8 == 0
        return -(-(1 << 32) // (2 * rows * 8)) * 8

    prev_tile = ops.gemm_set_tile(0)
    try:
        for tile, (m, n, k), epi, out32, kernel in ((0, (8192, 4096, 128), EPI_NONE, 1, 3),       # gemm_nt_duo by shape
                                                    (2, (1024, 256, 128), EPI_NONE, 1, 3)):       # ... and pinned
            ops.gemm_set_tile(tile)
            la, lw = limit(m), limit(n)
            assert (m * (la - 8) * 2 < 1 << 32 <= m * la * 2) and (n * (lw - 8) * 2 < 1 << 32 <= n * lw * 2)
            assert nt(m, n, k, la - 8, lw - 8, epi, out32) == [kernel]
            for lda, ldw in ((la, k), (k, lw), (la, lw)):
                plan = nt(m, n, k, lda, ldw, epi, out32)
                assert plan and all(kn in small for kn in plan) and not any(kn in narrow for kn in plan), (tile, lda, ldw, plan)
    finally:
        ops.gemm_set_tile(prev_tile)

    m, n, k = 1024, 256, 128
    la, lw = limit(m), limit(n)
    entries = {"hgr_gemm_nt_ln": lambda lda, ldw: (p, lda, p, ldw, p, n, p, p, p, 1e-5, m, n, k, HGR_F16, 0, 0),
               "hgr_gemm_nt_res_stats": lambda lda, ldw: (p, lda, p, ldw, p, p, n, p, p, m, n, k, HGR_F16, 0),
               "hgr_gemm_nt_res_stats_guard": lambda lda, ldw: (p, lda, p, ldw, p, p, n, p, p, 1.0, p, m, n, k, HGR_F16, 0),
               "hgr_gemm_nt_bias_gelu_dual": lambda lda, ldw: (p, lda, p, ldw, p, n, p, n, p, m, n, k, HGR_F16, 0),
               "hgr_gemm_nt_qgelu_grad_colsum": lambda lda, ldw: (p, lda, p, ldw, p, n, p, n, p, m, n, k, HGR_F16, 0)}
    for name, args in entries.items():
        plan = ops.gemm_plan(lambda: _lib.call(name, *args(la - 8, lw - 8)))             # one step below: planned on gemm_nt_duo
        assert [d["kernel"] for d in plan] == [3], (name, plan)
        for lda, ldw in ((la, k), (k, lw)):
            with pytest.raises(_lib.HgrError, match="beyond 4 GB"):
                _lib.call(name, *args(lda, ldw))
    assert ops.gelu_dual_ok(m, n, k, la - 8, lw - 8) and not ops.gelu_dual_ok(m, n, k, la, k) and not ops.gelu_dual_ok(m, n, k, k, lw)

    # hgr_gemm_nt_ln_mha is outside the capture: it would launch.  Its dtype check comes after the 4 GB check, so a bad dtype tells the
    # two sides of the limit apart without a launch: "bad dtype" = the operand sizes were accepted.
    b, l, heads = 16, 64, 2                                            # 1024 rows of width 128, in_proj weight [384, 128]
    w = heads * 64
    lw3 = limit(3 * w)
    mha = lambda ldx, ldw: _lib.call("hgr_gemm_nt_ln_mha", p, ldx, p, ldw, p, p, p, 1e-5, p, w, b, l, heads, 0, 7, 0)
    with pytest.raises(_lib.HgrError, match="bad dtype"):
        mha(la - 8, lw3 - 8)
    for ldx, ldw in ((la, w), (w, lw3)):
        with pytest.raises(_lib.HgrError, match="beyond 4 GB"):
            mha(ldx, ldw)
    assert ops.ln_mha_ok(w, l, rows=b * l, ldx=la - 8) and not ops.ln_mha_ok(w, l, rows=b * l, ldx=la)
    assert lib.hgr_gemm_plan_capture(None, 0) == 0


def test_product_library_has_no_ablation_switches():
    """Round-5 verdict, hygiene: the wrong-result ablation switches (parts of a kernel left out for timing experiments) exist in
    `make lab` builds only.  The product library must not even contain their environment-variable names, and the lab-only entry
    point must not be exported."""
    from hgr_net_amd import _lib
    blob = Path(_lib.__file__).resolve().parent.joinpath("lib", "libhgr.so").read_bytes()
    for name in (b"HGR_GEMM_DBG", b"HGR_LS_DBG", b"HGR_LE_DBG"):
        assert name not in blob, f"{name.decode()} is compiled into libhgr.so"
    assert not hasattr(_lib.load(), "hgr_lab_qa_stamps")
    common = (ROOT / "hgr-net_amd" / "csrc" / "hgr_common.h").read_text()
    assert "#define HGR_LAB_ON(expr) false" in common


def test_class_operand_split_is_the_default():
    """Round-5 verdict: the ~22-bit class operand of the logits product (clip_tree.LOGITS_SPLIT = "class") is the default of both
    routes; HGR_LOGITS_SPLIT=none switches it off."""
    code = "import os; os.environ.pop('HGR_LOGITS_SPLIT', None); from hgr_net_amd.model import clip_tree; print(clip_tree.LOGITS_SPLIT)"
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), timeout=300).stdout.strip() == "class"
    env = dict(os.environ, HGR_LOGITS_SPLIT="none")
    assert subprocess.run([sys.executable, "-c", code.replace("os.environ.pop('HGR_LOGITS_SPLIT', None); ", "")], capture_output=True, text=True, cwd=str(ROOT),
                          env=env, timeout=300).stdout.strip() == "none"


def test_product_path_has_no_cpu_fallback():
    """CPU tensors must be refused loudly: the product never computes on the host."""
    from hgr_net_amd import synth
    from hgr_net_amd._lib import HgrError
    from hgr_net_amd.clip.model import build_model
    model = build_model(synth.clip_state_dict("tiny-vit", 0))
    with pytest.raises(HgrError):
        model.encode_image(synth.images(1, 64, 0))
    with pytest.raises(HgrError):
        model.encode_text(synth.make_tokens(2, 11, 512))
    rn = build_model(synth.clip_state_dict("tiny-rn", 0))
    with pytest.raises(HgrError):
        rn.encode_image(synth.images(1, 64, 0))


def test_state_dict_schema_roundtrip():
    from hgr_net_amd import synth
    from hgr_net_amd.clip.model import build_model, infer_config
    for name in ("tiny-vit", "tiny-rn", "small-vit"):
        sd = synth.clip_state_dict(name, 0)
        m = build_model(sd)
        out = m.state_dict()
        assert set(out) == set(sd)
        assert all(torch.equal(out[k].float(), sd[k].float()) for k in sd)
        assert infer_config(out) == {**synth.CLIP_CONFIGS[name]}


def test_tree_model_host_logic(tmp_path, golden_dir):
    """ctor attributes, OM schedule and negative sampling follow the reference's rules (clip_tree.py:116-141,228-251)."""
    import random
    from hgr_net_amd import synth
    from hgr_net_amd.clip.model import build_model
    from hgr_net_amd.hierarchy import build_hierarchy
    from hgr_net_amd.model import tree_model
    edges = synth.make_dag(120, depth=8, seed=3, multi_parent=0.05)
    g = tmp_path / "g.json"
    g.write_text(json.dumps(edges))
    h = build_hierarchy(edges)
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], 40, 50, 13)
    o = types.SimpleNamespace(device="cpu", folder=str(tmp_path), exp_name="HGR", weights="adaptive", out_ratio=0.25, in_ratio=0.5,
                              from_epoch=-1, graph_path=str(g), arch="x", fetch=False, load=False, load_path="none", scale=1.0,
                              num_compare=16, k=1, sample_strategy="topk", weighting="both")
    m = tree_model(o, splits["all"], splits["rest"], node_tokens=synth.make_tokens(120, 11, 512),
                   clip_model=build_model(synth.clip_state_dict("tiny-vit", 0)))
    assert m.train_index.dtype == torch.int64 and len(m.train_index) == 120 and len(m.test_index) == 50
    assert m.max_depth == max(m.d2n) and m.resolution == 64
    assert isinstance(m.layer_weight, torch.nn.Parameter) and m.layer_weight.is_leaf      # F11-ii fixed on purpose
    assert os.path.isdir(m.save_path)
    deep = max(range(120), key=lambda i: len(m.c2p[i]))
    plan = m.outer_inner_plan(deep)
    L = len(m.c2p[deep]) + 1
    import math
    assert plan[0]["K"] == max(1, math.ceil(0.25 * L)) and plan[0]["p_out"] == deep
    for st in plan:
        random.seed(0)
        ids, pos = m.get_contra_ids("topk", st["p_out"], st["depth"], st["parents_in"])
        assert ids[pos] == st["p_out"] and len(ids) <= 17 and len(set(ids)) == len(ids)
        assert not (set(ids) - {st["p_out"]}) & set(st["parents_in"])
        lo = max(min(m.d2n), st["depth"] - 1)
        allowed = set(sum([m.d2n[d] for d in range(lo, st["depth"])], [])) | (set(m.d2n[0]) if st["depth"] == 0 else set())
        assert set(ids) - {st["p_out"]} <= allowed
    w = m.get_weights("increasing", 4)
    assert torch.allclose(w, torch.tensor([0.1, 0.2, 0.3, 0.4]))
    table = json.load(open(golden_dir / "tree_tinyvit_n90.json"))["weights_table"]       # captured from the reference
    for method, by_depth in table.items():
        for d, ref in by_depth.items():
            assert torch.allclose(m.get_weights(method, int(d)).float().cpu(), torch.tensor(ref), rtol=0, atol=1e-7), (method, d)
            assert torch.equal(m.get_weights(method, int(d), device="cpu"), m.get_weights(method, int(d)).cpu()), (method, d)   # the training step's host copy
    assert abs(float(m.get_weights("adaptive", 3).sum()) - 1) < 1e-6


def test_shard_bounds_cover_everything():
    from hgr_net_amd.parallel import batches_of_rank, shard_bounds
    for n in (1, 7, 8, 21841):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    assert sorted(sum([list(batches_of_rank(10, 4, r)) for r in range(4)], [])) == list(range(10))


_WORKER = r'''
import os, sys, json
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from hgr_net_amd import parallel
from hgr_net_amd.evaluate import COUNTERS
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(0)
table = torch.randn(50, 6)                    # "encode" = a deterministic row-wise function
enc = lambda rows: table[rows] * 2.0 + 1.0
for n in (10, 11, 37):                         # even and uneven shards
    rows = torch.arange(n) % 50
    full = parallel.sharded_rows(enc, rows)
    assert torch.equal(full, enc(rows)), n
# counters: every rank adds its own batches; the all-reduced sum equals the single-process sum
acc = torch.zeros(len(COUNTERS), dtype=torch.float64)
for b in parallel.batches_of_rank(9, world, rank):
    acc += torch.arange(len(COUNTERS), dtype=torch.float64) * (b + 1)
dist.all_reduce(acc)
want = sum(torch.arange(len(COUNTERS), dtype=torch.float64) * (b + 1) for b in range(9))
assert torch.equal(acc, want)
# bucketed gradient averaging of DP training: rank r holds grad = (r + 1) * base; None grads count as zeros
ps = [torch.nn.Parameter(torch.zeros(s)) for s in ((300, 7), (5,), (64, 64), (1,))]
for i, p in enumerate(ps):
    p.grad = None if (i == 1 and rank == 0) else torch.full_like(p.data, float((rank + 1) * (i + 1)))
parallel.allreduce_grads(ps, bucket_bytes=4096)
for i, p in enumerate(ps):
    contrib = [0.0 if (i == 1 and r == 0) else float((r + 1) * (i + 1)) for r in range(world)]
    assert torch.allclose(p.grad, torch.full_like(p.data, sum(contrib) / world)), i
# overlapped all-reduce of FusedAdamW (early = everything but the image tower, late = the image tower): same sums as allreduce()
from hgr_net_amd.training import FusedAdamW
qs = [torch.nn.Parameter(torch.zeros(s)) for s in ((70,), (3, 5), (129,), (64,), (10, 10))]
opt = FusedAdamW(qs, lr=1e-3)
for i, q in enumerate(qs):
    q.grad.fill_(float((rank + 1) * (i + 1)))
opt.set_late_params([qs[1], qs[2]])
assert sum(h - l for l, h in opt._ranges["early"] + opt._ranges["late"]) == opt.gflat.numel()
opt.allreduce_part("early", bucket_bytes=256)
opt.allreduce_part("late", bucket_bytes=256)
for i, q in enumerate(qs):
    assert torch.equal(q.grad, torch.full_like(q.data, float(sum(r + 1 for r in range(world)) * (i + 1)))), i
assert opt.grad_scale == 1.0 / world
dist.barrier()
if rank == 0: print("OK")
dist.destroy_process_group()
'''


def test_splitk_slice_count_fills_the_chip():
    """ops.splitk_slices (host plan of hgr_gemm_tn_splitk): from the smallest slice count that fills >= 85 % of whole rounds of the
    workgroup slots up to 1.25 x that count, the best-filling one; every slice at least 512 rows deep; one slice when rows are few."""
    from hgr_net_amd import ops
    fill = lambda tiles, s, slots: tiles * s / (-(-(tiles * s) // slots) * slots)
    assert ops.splitk_slices(16, 65792, 256) == 16                    # out_proj of ViT-L/14: 100 % instead of 14 slices = 87.5 %
    assert ops.splitk_slices(48, 65792, 256) == 5 and ops.splitk_slices(64, 65792, 256) == 4
    assert ops.splitk_slices(9, 81397, 256) == 28
    assert ops.splitk_slices(1, 1000, 256) == 1 and ops.splitk_slices(300, 100, 256) == 1
    for tiles in (1, 3, 9, 16, 27, 36, 48, 64, 100, 300, 1000):
        for m in (600, 5000, 65792, 81397):
            for slots in (256, 512):
                s = ops.splitk_slices(tiles, m, slots)
                assert 1 <= s <= max(1, m // 512)
                reachable = [fill(tiles, t, slots) for t in range(1, max(1, min(m // 512, 4096)) + 1)]
                if max(reachable) >= 0.85:
                    first = next(t for t, f in enumerate(reachable, 1) if f >= 0.85)
                    assert first <= s <= max(first + 1, int(first * 1.25)) and fill(tiles, s, slots) >= reachable[first - 1] - 1e-9
                else:
                    assert abs(fill(tiles, s, slots) - max(reachable)) < 1e-9


def test_world_size_2_gloo_sharding(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(ROOT)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "OK" in outs[0]


def test_tokenizer_matches_reference_ids(golden_dir):
    """BPE ids captured from the reference's tokenizer (tools/make_golden_tokenizer.py -> tests/golden/tokenizer_ids.json), encoded
    with the merges it reads (tests/golden/bpe_merges.txt.gz, same tool; HGR_BPE_VOCAB points at another copy of the merges file)."""
    from hgr_net_amd.clip import simple_tokenizer as st
    import os
    path = os.environ.get("HGR_BPE_VOCAB") or str(golden_dir / "bpe_merges.txt.gz")
    os.environ["HGR_BPE_VOCAB"] = path
    tok = st.SimpleTokenizer(path)
    gold = json.load(open(golden_dir / "tokenizer_ids.json"))
    for text, ids in zip(gold["texts"], gold["ids"]):
        assert tok.encode(text) == ids
    from hgr_net_amd import clip
    t = clip.tokenize(["a photo of a cat.", "x"])
    assert t.shape == (2, 77) and t[0, 0] == 49406 and t[0].max() == 49407 and t[1, 3:].sum() == 0
    with pytest.raises(RuntimeError):
        clip.tokenize(["word " * 200])


# ---- input pipeline: host side of the device transform ----------------------------------------------
def test_resize_taps_match_oracle():
    """The vectorised tap tables of the product (hgr_net_amd.preprocess) equal the scalar Pillow restatement."""
    from oracle import resample_ref
    from hgr_net_amd import preprocess
    for ins, outs in [(53, 22), (375, 224), (500, 298), (32, 33), (17, 32), (224, 224), (1200, 298), (4000, 224)]:
        b, k = resample_ref.precompute_coeffs(ins, outs)
        for start, count in [(0, outs), (outs // 4, outs // 2)]:
            b2, k2 = preprocess.resize_taps(ins, outs, start, count)
            assert np.array_equal(b[start:start + count], b2) and np.array_equal(k[start:start + count], k2)


def test_resize_and_crop_rules():
    from oracle import resample_ref
    from hgr_net_amd import preprocess
    for w, h in [(500, 375), (375, 500), (224, 224), (225, 224), (640, 427), (333, 1000), (100, 37)]:
        assert preprocess.resized_size(w, h, 224) == resample_ref.resized_size(w, h, 224)
        nw, nh = preprocess.resized_size(w, h, 224)
        assert min(nw, nh) == 224
        assert preprocess.crop_origin(nw, nh, 224) == resample_ref.crop_origin(nw, nh, 224)
    assert preprocess.resized_size(500, 375, 224) == (298, 224)
    assert preprocess.crop_origin(298, 224, 224) == (37, 0)
    assert preprocess.crop_origin(229, 224, 224) == (2, 0)          # (229 - 224) / 2 = 2.5 rounds half to even


def test_product_package_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under the product package may import it."""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent / "hgr-net_amd"
    offenders = [str(p) for p in root.rglob("*.py") if re.search(r"^\s*(from|import)\s+oracle\b", p.read_text(), re.M)]
    assert not offenders, offenders


def test_cosine_lr_schedule_values():
    """utils.py:78-95 of the reference: linear warm-up base*(step+1)/warmup, then 0.5*(1+cos(pi*e/es))*base."""
    import math
    from hgr_net_amd.utils import cosine_lr
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.0}, {"lr": 0.0}])
    sched = cosine_lr(opt, 3e-7, 5, 105)
    sched(0); assert all(abs(g["lr"] - 3e-7 * 1 / 5) < 1e-20 for g in opt.param_groups)
    sched(4); assert abs(opt.param_groups[0]["lr"] - 3e-7) < 1e-20
    sched(55); assert abs(opt.param_groups[1]["lr"] - 0.5 * (1 + math.cos(math.pi * 50 / 100)) * 3e-7) < 1e-20
    sched(105); assert abs(opt.param_groups[0]["lr"]) < 1e-20
    sched2 = cosine_lr(opt, [1.0, 2.0], 0, 10)
    sched2(0); assert [g["lr"] for g in opt.param_groups] == [1.0, 2.0]


def test_bench_parent_launcher_never_loads_torch(tmp_path, monkeypatch):
    """`python bench.py --gpus N` (N > 1, no WORLD_SIZE): the parent only builds the torch.distributed.run command line and
    relays the children's JSON line - it must not import torch (let alone touch the GPU) before or after spawning."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    code = (ROOT / "bench.py").read_text()
    assert "import torch" not in code.split("def launch_ranks")[0]            # nothing heavy at module import
    fake = tmp_path / "fake_run.py"
    fake.write_text("import sys, json\nprint('banner noise')\nprint(json.dumps({'ok': 1, 'argv': sys.argv[1:]}))\n")
    probe = tmp_path / "probe.py"
    probe.write_text(
        "import sys, subprocess, importlib.util\n"
        f"spec = importlib.util.spec_from_file_location('b', r'{ROOT / 'bench.py'}')\n"
        "b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)\n"
        "real = subprocess.Popen\n"
        "def popen(cmd, **kw):\n"
        "    assert cmd[1:3] == ['-m', 'torch.distributed.run'] and '--nproc-per-node=2' in cmd and '127.0.0.1' in cmd, cmd\n"
        f"    return real([sys.executable, r'{fake}'] + cmd[cmd.index(str(b.Path(b.__file__).resolve())) + 1:], **kw)\n"
        "subprocess.Popen = popen\n"
        "rc = b.launch_ranks(['--gpus', '2', '--steps', '3'], 2)\n"
        "assert 'torch' not in sys.modules, 'the launcher parent imported torch'\n"
        "sys.exit(rc)\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(probe)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["argv"] == ["--gpus", "2", "--steps", "3"]
    assert "banner noise" in p.stderr                                          # non-JSON child output goes to stderr


def test_host_asan_build_of_the_abi_shim():
    """SURVEY section 5 (sanitizers): `make -C hgr-net_amd/csrc asan` builds the C-ABI shim's HOST code under AddressSanitizer and
    runs tests/abi_asan_driver.cpp against it (argument validation + error formatting of every family of entry points; no
    kernel is launched, device code is not instrumented).  Building takes about a minute, so this test only (re)builds when
    HGR_ASAN_TEST=1; otherwise it runs an existing driver, or skips."""
    csrc = ROOT / "hgr-net_amd" / "csrc"
    drv = csrc / "build_asan" / "abi_asan_driver"
    if os.environ.get("HGR_ASAN_TEST") == "1":
        p = subprocess.run(["make", "-C", str(csrc), "-j8", "asan"], capture_output=True, text=True, timeout=1800)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "0 failures" in p.stdout
        return
    if not drv.exists():
        pytest.skip("ASan driver not built (HGR_ASAN_TEST=1 builds it)")
    p = subprocess.run([str(drv)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    assert p.returncode == 0 and "0 failures" in p.stdout, p.stdout[-1500:] + p.stderr[-1500:]


def test_comm_file_bootstrap_ignores_a_stale_id_file(tmp_path, monkeypatch):
    """Round-2 advisor finding: a unique-id file left by an earlier run must not be fed to ncclCommInitRank.  The file carries the
    run's nonce; rank 0 replaces whatever it finds, a waiting rank accepts only a file with THIS run's nonce and times out with a
    diagnostic on a foreign one; rank 0's destroy() removes the file.  (No RCCL call: unique_id / init are stand-ins here.)"""
    from hgr_net_amd import _lib, comm
    seen = []
    monkeypatch.setattr(comm, "unique_id", lambda: b"\x07" * comm.ID_BYTES)
    monkeypatch.setattr(comm, "init", lambda rank, world, uid: seen.append((rank, world, bytes(uid))))
    monkeypatch.setattr(_lib, "call", lambda *a, **k: 0)
    path = str(tmp_path / "uid.bin")
    with open(path, "wb") as f:                                   # what an earlier run left behind: same size, other nonce
        f.write(comm._run_nonce("earlier run") + b"\x09" * comm.ID_BYTES)
    with pytest.raises(_lib.HgrError, match="stale"):
        comm.init_from_file(path, rank=1, world=2, timeout_s=0.3, nonce="this run")
    assert not seen
    comm.init_from_file(path, rank=0, world=2, timeout_s=5.0, nonce="this run")       # replaces the stale file
    comm.init_from_file(path, rank=1, world=2, timeout_s=5.0, nonce="this run")
    assert seen == [(0, 2, b"\x07" * comm.ID_BYTES), (1, 2, b"\x07" * comm.ID_BYTES)]
    comm.destroy()
    assert not os.path.exists(path)
    os.environ.pop("HGR_COMM_NONCE", None)
    monkeypatch.setenv("MASTER_PORT", "29512")
    a = comm._run_nonce(None)
    monkeypatch.setenv("MASTER_PORT", "29513")
    assert a != comm._run_nonce(None) and len(a) == 16


def test_comm_file_bootstrap_default_nonce_rejects_an_old_file(tmp_path, monkeypatch):
    """Round-3 advisor finding: without a per-run nonce (static MASTER_PORT, TORCHELASTIC_RUN_ID unset / 'none') a crashed run's id
    file carries the SAME nonce as this run.  A waiting rank then also requires the file to be no older than this process (minus the
    publish slack); rank 0 warns that the default is degenerate."""
    from hgr_net_amd import _lib, comm
    seen = []
    monkeypatch.setattr(comm, "unique_id", lambda: b"\x07" * comm.ID_BYTES)
    monkeypatch.setattr(comm, "init", lambda rank, world, uid: seen.append((rank, world, bytes(uid))))
    monkeypatch.setattr(_lib, "call", lambda *a, **k: 0)
    monkeypatch.delenv("HGR_COMM_NONCE", raising=False)
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "none")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29500")
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    assert not comm._nonce_is_per_run(None) and comm._nonce_is_per_run("x")
    path = str(tmp_path / "uid.bin")
    with open(path, "wb") as f:                                   # a crashed earlier run: same (degenerate) nonce, written long ago
        f.write(comm._run_nonce(None) + b"\x09" * comm.ID_BYTES)
    old = comm._T_START - comm.STALE_SLACK_S - 100.0
    os.utime(path, (old, old))
    with pytest.raises(_lib.HgrError, match="stale"):
        comm.init_from_file(path, rank=1, world=2, timeout_s=0.3)
    assert not seen
    with pytest.warns(UserWarning, match="no per-run nonce"):
        comm.init_from_file(path, rank=0, world=2, timeout_s=5.0)
    comm.init_from_file(path, rank=1, world=2, timeout_s=5.0)     # the file rank 0 just published is fresh
    assert seen == [(0, 2, b"\x07" * comm.ID_BYTES), (1, 2, b"\x07" * comm.ID_BYTES)]
    comm.destroy()
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "job-4711")
    assert comm._nonce_is_per_run(None)
    # round-5 advisor finding: nothing rank-local (the parent pid of round 5) enters the nonce - ranks behind per-rank wrappers must
    # derive the same one; a launcher-provided HGR_COMM_NONCE makes a static-run-id launch per-run
    monkeypatch.setenv("TORCHELASTIC_RUN_ID", "none")
    a = comm._run_nonce(None)
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "2")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert not comm._nonce_is_per_run(None) and comm._run_nonce(None) == a
    monkeypatch.setenv("HGR_COMM_NONCE", "launcher-made")
    assert comm._nonce_is_per_run(None) and comm._run_nonce(None) != a
    # the age rule counts from the PROCESS start (not the module import): a slow import does not lock a rank out
    assert comm._T_START <= time.time() and comm.STALE_SLACK_S <= 60
