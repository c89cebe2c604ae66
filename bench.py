#!/usr/bin/env python3
"""bench.py - images/sec of the HGR-Net zero-shot evaluation step on MI355X.

Workload (BASELINE.json configs[1], metric "images/sec over 21K-class hierarchy, batch 512"):
ViT-B/32 CLIP, N = 21 841 hierarchy nodes, batch 512 synthetic 224x224 images per GPU.  One step =
the body of the reference's hot loop (main.py:131-191): ``logits = model(imgs)`` (image tower -> L2
norm -> [512x512].[512x21841] logits GEMM, model/clip_tree.py:328-333) followed by the top-20 /
top-1 / per-level arg-max metrics.  ``update_classifier`` (text tower over all prompts) is one-off per
evaluation and runs before the timed region, sharded over ranks + RCCL all-gather when N > 1.

    python bench.py [--gpus N] [--steps K] [--warmup W]            (N > 1: spawns the N ranks itself, see launch_ranks)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
    python bench.py ... --full                                     (+ every measurement and check beside the headline)
    python bench.py ... --dump-outputs DIR                         (+ the last timed step's outputs as DIR/<name>.npy)

A plain run sets up, warms up, times the K steps and prints the line.  --full adds what needs runs of its own: the warm
update_classifier, the unblocked host time, power / clock samples, the roofline pass, the PCIe-inclusive leg, the CPU
baseline + parity against the oracle, the multi-rank self-check (dp_check), the host probe and the secondary configs.

Prints ONE JSON line (rank 0) - see DESIGN.md "Measurement" for how each field is obtained.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

N_NODES, BATCH, ARCH = 21841, 512, "ViT-B/32"
PEAK_TFLOPS_BF16 = 2500.0        # dense bf16 MFMA peak, MI355X_MICROARCH.md


def launch_ranks(argv, n: int) -> int:
    """`python bench.py --gpus N` typed without a launcher: start the N ranks as CHILD processes
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same args>`), relay rank 0's single
    JSON line, return non-zero if any rank failed.  This parent never touches the GPU (it does not even import torch):
    replacing or re-executing a process that has initialised HIP is not allowed on this pool."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + list(argv)
    import uuid
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HGR_COMM_NONCE", uuid.uuid4().hex)       # one per-run value every rank inherits (hgr_net_amd.comm's file bootstrap)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)          # stderr passes through
    lines = []
    for line in p.stdout:
        if line.startswith("{"):
            lines.append(line)
        else:
            sys.stderr.write(line)
    rc = p.wait()
    if rc == 0 and len(lines) != 1:
        sys.stderr.write(f"[bench] expected one JSON line from rank 0, got {len(lines)}\n")
        rc = 1
    if lines:
        sys.stdout.write(lines[-1])
        sys.stdout.flush()
    return rc


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays: dict) -> None:
    """--dump-outputs: every array as out_dir/<name>.npy (float32 / float64 only, at most DUMP_LIMIT_BYTES in all), so that two
    builds run with the same arguments can be compared output for output."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes > {DUMP_LIMIT_BYTES}"
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    log(f"[bench] outputs of the last timed step -> {out_dir}: " + ", ".join(f"{k} {tuple(v.shape)}" for k, v in arrays.items()))


def _timed(fn):
    t0 = time.time()
    out = fn()
    return time.time() - t0, out


def _thread_sweep(fn, candidates, calls: int = 1):
    """Seconds per call of fn under torch.set_num_threads(c) for every candidate (one untimed call + the best of `calls` timed ones
    each): an fp32 batch-32 forward does not scale to every core of a 256-thread host, and oversubscribed it is slow AND noisy
    (round 3: 6.7 img/s on 128 threads where 8 threads gave 61 - 64).  Returns ({threads: s}, best threads)."""
    import torch
    sweep = {}
    for c in candidates:
        torch.set_num_threads(c)
        fn()
        sweep[c] = min(_timed(fn)[0] for _ in range(calls))
    return sweep, min(sweep, key=sweep.get)


def _thread_candidates():
    n = os.cpu_count() or 1
    c = [t for t in (8, 16, 32, 64, 128) if t <= n]
    return c or [n]


def _median_rate(fn, bs: int, repeats: int, warm: int = 2):
    """images/sec from the MEDIAN of `repeats` timed calls of fn after `warm` untimed ones."""
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(repeats):
        dt, out = _timed(fn)
        ts.append(dt)
    ts.sort()
    return bs / ts[len(ts) // 2], repeats, out, (bs / ts[-1], bs / ts[0])


def cpu_baseline(sd, zsl_cpu, arch="ViT-B/32", c1=True):
    """The oracle (CPU fp32 restatement of the reference path, oracle/) timed on this box's host cores on a bounded
    sample of the same workload: batches of 32 images through the same tower + N-class logits + top-20.  The thread count is
    swept first (8 ... 128, one warm + one timed batch each) and the value is the median of 7 repeats after 2 warm-ups at the best
    setting; `cores` = that setting, the sweep is reported beside it.  Next to it the SURVEY 8(d) C1 line (RN50, N = 1 000,
    batch 32, fp32: BASELINE configs[0], the reference's own CPU-runnable case), measured the same way."""
    import torch
    from hgr_net_amd import synth
    from oracle import tree_ref
    bs = 32
    pool = synth.images(bs * 8, 224, 99)     # every timed call takes another slice: all of them feed the parity check below
    img = pool[:bs]
    calls = []
    threads0 = torch.get_num_threads()

    def run():
        i = len(calls) % 8
        lg = tree_ref.forward(sd, pool[i * bs:(i + 1) * bs], zsl_cpu)
        lg.topk(20, dim=1)
        calls.append((i, lg))
        return lg

    sweep, best = _thread_sweep(run, _thread_candidates())
    torch.set_num_threads(best)
    rate, reps, lg, (lo, hi) = _median_rate(run, bs, 7)
    seen = dict(calls)
    idx = sorted(seen)
    # the oracle's logits of every slice it was timed on: checked against the HIP path below (one HIP batch of all of them)
    cpu_baseline.last = (torch.cat([pool[i * bs:(i + 1) * bs] for i in idx]), torch.cat([seen[i] for i in idx]))
    out = {"value": round(rate, 2), "unit": "images/sec", "cores": best, "kind": "port",
           "sample": f"median of {reps} x batch {bs} (after 2 warm-ups) of the same {arch} N={zsl_cpu.shape[0]} forward+top20 (min {lo:.1f}, max {hi:.1f}), "
                     f"oracle/ (torch fp32 CPU) at torch.set_num_threads({best}) = the fastest of the sweep, host cpu_count={os.cpu_count()}",
           "thread_sweep_img_per_s": {str(c): round(bs / t, 1) for c, t in sweep.items()}}
    if not c1:
        torch.set_num_threads(threads0)
        return out
    # C1: RN50, 1 000 classes, batch 32 (update_classifier excluded: the class matrix is a seeded unit-norm stand-in, the
    # timed arithmetic - tower, L2 norm, [32x1024].[1024x1000], top-20 - does not depend on its values)
    try:
        cfg = synth.CLIP_CONFIGS["RN50"]
        sd_rn = synth.clip_state_dict(cfg, 0)
        g = torch.Generator().manual_seed(5)
        z = torch.randn(1000, cfg["embed_dim"], generator=g)
        z = z / z.norm(dim=1, keepdim=True)

        def run_c1():
            lgc = tree_ref.forward(sd_rn, img, z)
            lgc.topk(20, dim=1)
            return lgc

        sweep1, best1 = _thread_sweep(run_c1, _thread_candidates())
        torch.set_num_threads(best1)
        r1, n1, _, (lo1, hi1) = _median_rate(run_c1, bs, 5, warm=1)
        out["c1"] = {"value": round(r1, 2), "unit": "images/sec", "cores": best1,
                     "sample": f"BASELINE configs[0]: RN50 N=1000 batch {bs} fp32 forward+top20, median of {n1} at torch.set_num_threads({best1}) (min {lo1:.1f}, max {hi1:.1f})",
                     "thread_sweep_img_per_s": {str(c): round(bs / t, 1) for c, t in sweep1.items()}}
    except Exception as e:  # noqa: BLE001 - the C1 line is informative; the headline sample above is the contract
        out["c1"] = {"error": repr(e)}
    torch.set_num_threads(threads0)
    return out


def power_probe(run_step, fence, want: int = 5, max_s: float = 6.0):
    """Socket power and shader clock WHILE the steps run: rocm-smi polled from a thread over extra steps behind the timed region (a child
    process per sample: nothing of it runs inside the timed loop).  The tower GEMMs hold the package at its power limit and the clock
    below its 2.4 GHz maximum, so `roofline.peak` (quoted at 2.4 GHz) is not reachable at any utilisation - the line says at which
    clock the measured rate was obtained.  None if rocm-smi is absent or prints something else."""
    import shutil
    import subprocess
    import threading
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(exe):
        return None
    samples, stop = [], threading.Event()
    # the card THIS process drives, by PCI address (round-5 advisor finding: "the card that draws most" can be another job's GPU on a
    # shared node or under HIP_VISIBLE_DEVICES); a node whose cards cannot be told apart is not probed rather than misattributed
    mine = None
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        want_bus = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}".lower()
        buses = json.loads(subprocess.run([exe, "--showbus", "--json"], capture_output=True, text=True, timeout=10).stdout)
        hits = [c for c, d in buses.items() if any(want_bus in str(v).lower() for v in d.values())]
        mine = hits[0] if len(hits) == 1 else (next(iter(buses)) if len(buses) == 1 else None)
    except Exception:  # noqa: BLE001
        mine = None
    if mine is None:
        return None

    def poll():
        while not stop.is_set() and len(samples) < want + 1:
            try:
                out = subprocess.run([exe, "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout
                d = json.loads(out).get(mine, {})
                pw = [float(v) for k, v in d.items() if "power (w)" in k.lower() and str(v).replace(".", "", 1).isdigit()]
                ck = [float(str(v).strip("()").lower().replace("mhz", "")) for k, v in d.items() if k.lower().startswith("sclk clock speed")]
                if pw and ck:
                    samples.append((pw[0], ck[0]))
            except Exception:  # noqa: BLE001 - a probe: any failure just ends it
                return
            time.sleep(0.1)
    th = threading.Thread(target=poll, daemon=True)
    t0 = time.perf_counter()
    th.start()
    i = 0
    while th.is_alive() and time.perf_counter() - t0 < max_s:
        run_step(i)
        i += 1
        if i % 8 == 0:
            fence()
    stop.set()
    th.join(timeout=15)
    fence()
    use = samples[1:] if len(samples) > 1 else samples              # the first sample may predate the ramp
    if not use:
        return None
    return {"socket_w": round(sum(p for p, _ in use) / len(use), 1), "sclk_mhz": round(sum(c for _, c in use) / len(use), 1), "samples": len(use),
            "steps_run": i, "how": "rocm-smi --showpower --showclocks polled over extra steps behind the timed region"}


def step_time_stats(events) -> dict:
    """Per-step intervals from the hipEvents recorded on the launch stream behind every timed step (event i = end of step i's
    launches in stream order): median / p95 / min / max in ms.  A slow box or a hiccup shows up here; the headline stays the loop mean."""
    ts = sorted(events[i].elapsed_time(events[i + 1]) for i in range(len(events) - 1))
    if not ts:
        return {}
    q = lambda f: ts[min(len(ts) - 1, int(round(f * (len(ts) - 1))))]
    return {"n": len(ts), "p50": round(q(0.5), 3), "p95": round(q(0.95), 3), "min": round(ts[0], 3), "max": round(ts[-1], 3),
            "how": "hipEvent intervals between consecutive steps on the launch stream"}


def plant_signal(model, targets, res: int, dev) -> dict:
    """Random-init towers give every class a logit of +-0.05 and the evaluation counters of main.py:139-191 never move: the
    metric string would be all zeros at any class count.  Plant signal: the class rows of the batches' target classes and of
    all their ancestors are replaced by normalise(alpha_a * f + sqrt(1 - alpha_a^2) * z_a), f = mean direction of the image
    features of a FIXED probe batch (identical on every rank), z_a = the row's own text embedding, alpha_a in [0.25, 0.75)
    hashed from the node id.  Planted rows then outrank the ~21 K unplanted ones for every image and compete with EACH OTHER
    by alpha: a batch's target is top-1 only when its alpha is the largest of the planted test classes, top-5 when among the
    five largest, ... so Top@k / hit / path / point ratios come out as non-trivial fractions.  Same arithmetic in the timed
    region; the CPU oracle of the parity leg is handed the same planted matrix."""
    import torch
    from hgr_net_amd import ops, synth
    probe = synth.images(64, res, 4321).to(dev)
    f = model.clip_model.encode_image(probe).float()
    f = f / f.norm(dim=1, keepdim=True)
    fbar = f.mean(0)
    fbar = fbar / fbar.norm()
    nodes = sorted({a for t in set(targets) for a in list(model.c2p[t]) + [t]})
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    alpha = torch.tensor([0.25 + 0.5 * ((a * 2654435761) % (1 << 32)) / float(1 << 32) for a in nodes], dtype=torch.float32, device=dev)
    z = model.zsl_weights.float().clone()
    z[idx] = alpha[:, None] * fbar[None, :] + (1.0 - alpha * alpha).sqrt()[:, None] * z[idx]
    z32 = torch.empty_like(z)
    z16 = torch.empty(z.shape, dtype=model._zsl16.dtype, device=dev)
    ops.l2norm_rows(z, y16=z16, y32=z32)
    model.zsl_weights, model._zsl16 = z32, z16
    return {"planted_rows": len(nodes), "probe_cohesion": round(float((f @ fbar).mean()), 4),
            "note": "class rows of the step targets + their ancestors mixed with the probe batch's mean image-feature direction (bench.py:plant_signal)"}


def _checksum(t) -> list:
    """Two order-independent 64-bit checksums of a tensor's BYTES (sum of the 32-bit words, and of word x (position % 65521 + 1)):
    equal tensors <=> equal pairs for all practical purposes, and cheap enough to gather from every rank."""
    import torch
    w = t.detach().contiguous().view(-1).view(torch.int32).to(torch.int64)
    pos = torch.arange(w.numel(), device=w.device, dtype=torch.int64) % 65521 + 1
    return [int(w.sum().item()), int((w * pos).sum().item())]


def _gather_obj(obj, world: int):
    import torch.distributed as dist
    box = [None] * world
    dist.all_gather_object(box, obj)
    return box


def dp_check_eval(model, ev, group, world: int, rank: int, elapsed_local: float, steps: int, dev) -> dict:
    """Self-check of a data-parallel evaluation run (the build side never sees more than one RCCL rank, so the first N > 1
    run verifies itself): (a) the all-gathered class matrix has the same bytes on every rank, (b) 256 of its rows equal this
    rank's OWN text encoding of those prompts, (c) the all-reduced counters equal the sum of the per-rank counters gathered
    separately, (d) ranks seen / per-rank step time.  `ok` False => every rank exits non-zero after rank 0 printed the line."""
    import torch
    import torch.distributed as dist
    from hgr_net_amd import ops
    zs = _gather_obj(_checksum(model.zsl_unplanted) + _checksum(model.zsl_weights), world)      # as all-gathered, and as evaluated (planted)
    n = model.zsl_unplanted.shape[0]
    rows = torch.arange(0, n, max(1, n // 256), device=dev)[:256]
    own = model.clip_model.encode_text(model.node_tokens[rows], ctx=model.ctx)
    own32 = torch.empty_like(own)
    ops.l2norm_rows(own, y32=own32)
    own_err = float((own32 - model.zsl_unplanted[rows]).abs().max())
    own_errs = _gather_obj(own_err, world)
    local = ev.acc.detach().cpu().tolist()
    locals_ = _gather_obj(local, world)
    red = ev.acc.clone()
    dist.all_reduce(red, op=dist.ReduceOp.SUM, group=group)
    red = red.cpu().tolist()
    summed = [sum(l[i] for l in locals_) for i in range(len(local))]
    cnt_ok = all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(red, summed))
    reds = _gather_obj(red, world)
    ms = _gather_obj(elapsed_local / steps * 1e3, world)
    ok = all(z == zs[0] for z in zs) and max(own_errs) <= 1e-6 and cnt_ok and all(r == reds[0] for r in reds) and dist.get_world_size(group) == world
    return {"ok": bool(ok), "ranks_seen": dist.get_world_size(group), "zsl_checksum_equal": all(z == zs[0] for z in zs), "zsl_checksum": zs[0],
            "own_encode_rows": int(rows.numel()), "own_encode_max_abs_diff": max(own_errs),
            "counters_allreduce_equals_sum_of_ranks": bool(cnt_ok), "counters_identical_on_all_ranks": all(r == reds[0] for r in reds),
            "num_sample_per_rank": [l[-1] for l in locals_], "ms_per_step_min": round(min(ms), 3), "ms_per_step_max": round(max(ms), 3)}


# ranks of the host-time probe: a GPU box admits at most 6 processes on its card; this process, the rank launcher's children and a
# rocm-smi poll are among them - 4 ranks fit, 5 were killed by the box's process guard (round 6) - so 4, not 8.  What an 8-rank node
# takes from a rank is its share of the host's cores, and that IS reproduced: every probe rank confines itself to
# 1 / HOST_PROBE_SHARE of them (HGR_HOST_SHARE, os.sched_setaffinity), the slice rank r of an 8-rank job would own
HOST_PROBE_RANKS = 4
HOST_PROBE_SHARE = 8


def run_secondary(args_extra, timeout_s: int, env_extra=None, keep_extra=()):
    """One of the other BASELINE configs as a CHILD process of this (finished) measurement: `python bench.py <args> --full --secondary`;
    its single JSON line, reduced to the fields a reader needs.  Never raises: a failure is reported in place."""
    import subprocess
    cmd = [sys.executable, str(Path(__file__).resolve())] + args_extra + ["--full", "--secondary"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra or {})
    t0 = time.time()
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout_s, env=env)
    except subprocess.TimeoutExpired:
        return {"error": f"timed out after {timeout_s}s", "cmd": " ".join(args_extra)}
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        return {"error": f"rc {p.returncode}", "stderr_tail": p.stderr[-400:], "cmd": " ".join(args_extra)}
    d = json.loads(lines[0])
    keep = ("metric", "value", "unit", "ms_per_step", "step_ms", "steps", "warmup", "dtype", "config", "roofline", "parity", "metrics_string", "loss_first", "loss_last",
            "peak_memory_gib", "cpu_baseline") + tuple(keep_extra)
    out = {k: d[k] for k in keep if k in d}
    out["wall_s"] = round(time.time() - t0, 1)
    out["cmd"] = "python bench.py " + " ".join(args_extra)
    return out


def tower_forward_flops(cfg, n_img: int, n_txt: int, l_txt: int) -> float:
    """Algorithmic forward FLOPs (2 x MAC, attention included) of `n_img` images and `n_txt` prompts of `l_txt` tokens:
    per token and layer 24 W^2 (qkv, out, fc, proj) + 4 L W (q k^T and p v), plus patch embedding and the projections
    (ModifiedResNet towers: the survey's measured per-image figure)."""
    wt, d = cfg["transformer_width"], cfg["embed_dim"]
    txt = n_txt * (l_txt * cfg["transformer_layers"] * (24.0 * wt * wt + 4.0 * l_txt * wt) + 2.0 * wt * d)
    if cfg["vision_patch_size"]:
        w, ps = cfg["vision_width"], cfg["vision_patch_size"]
        g = cfg["image_resolution"] // ps
        L = g * g + 1
        img = n_img * (L * cfg["vision_layers"] * (24.0 * w * w + 4.0 * L * w) + 2.0 * g * g * 3 * ps * ps * w + 2.0 * w * d)
    else:
        img = n_img * {"RN50": 12.22e9, "RN101": 19.6e9}.get("RN50" if cfg["vision_layers"] == (3, 4, 6, 3) else "RN101", 12.22e9)
    return img + txt


def train_mode(a, model, cfg, h, rank, world, group, ranks_seen, dev, real_stdout):
    """`--mode train`: one step = one OM training step of the reference's loop (main.py:79-94 around
    model/clip_tree.py:222-281): zero_grad, train_batch('OM', 'topk') on ONE single-class batch sharded over the ranks
    (SURVEY H7), gradient all-reduce, clip_grad_norm_(1.0) + AdamW as fused kernels.  BASELINE configs[4] =
    `--arch ViT-L/14 --n-ctx 16 --train-dtype bf16`.  Reports images/sec and the achieved rate over 3 x the forward FLOPs
    the step executes (each distinct prompt of the K x M inner steps is encoded once: identical arithmetic, fewer passes)."""
    import random
    from hgr_net_amd import synth
    from hgr_net_amd.training import FusedAdamW
    params = [p for n, p in model.named_parameters() if p.requires_grad and n != "layer_weight"]
    opt = FusedAdamW(params, lr=3e-7, weight_decay=0.0, max_norm=1.0)
    img = synth.images(a.batch * world, cfg["image_resolution"], 1234)[rank * a.batch: (rank + 1) * a.batch].to(dev)
    target = max(model.train_index.tolist(), key=lambda i: (len(model.c2p[i]), -i))     # a deepest class: the longest OM schedule
    tg = torch.full((a.batch,), target, dtype=torch.long, device=dev)
    random.seed(0)                                                                     # identical negatives on every rank

    model._dp_group = group            # data-parallel: the step's distinct prompts are sharded over the ranks (training.OMTrainer)

    def step():
        opt.zero_grad()
        tr = getattr(model, "_trainer", None)
        if group is not None and tr is not None and tr.grad_ready_hook is None:
            # overlapped: text-tower / head buckets are all-reduced while the image tower back-propagates
            opt.set_late_params(model.clip_model.visual.parameters())
            tr.grad_ready_hook = lambda part: opt.allreduce_part(part, group)
        overlapped = group is not None and tr is not None
        loss = model.train_batch(img, tg, "OM", "topk")
        if group is not None and not overlapped:               # first step only: the trainer is built inside train_batch
            opt.allreduce(group)
        opt.step()
        return loss

    def fence():
        torch.cuda.synchronize()
        if group is not None:
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()

    loss0 = None
    for _ in range(a.warmup):
        loss0 = step()
    fence()
    torch.cuda.reset_peak_memory_stats()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        loss = step()
        marks[i + 1].record()
    fence()
    elapsed = time.perf_counter() - t0
    step_ms = step_time_stats(marks)
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if a.dump_outputs and rank == 0:
        # what the last step hands its caller: the loss, and the weights it left behind (a fixed, seeded sample of the flat fp32 buffer)
        n_ = opt.flat.numel()
        pick = torch.randint(0, n_, (min(n_, 1 << 20),), generator=torch.Generator().manual_seed(0)).sort().values.to(dev)
        dump_outputs(a.dump_outputs, {"loss": np.array([float(loss)], dtype=np.float64),
                                      "weights_sample": opt.flat[pick].cpu().numpy(), "weights_sample_index": pick.cpu().numpy().astype(np.float64)})
    dp_check = None
    if world > 1 and a.full:
        # self-check of the data-parallel step (first real N > 1 run): after the overlapped all-reduce every rank holds the SAME
        # summed gradient buffer and, after the fused clip + AdamW, the same weights; every rank drew the same negatives.  The
        # per-rank loss is the mean CE over that rank's shard of the global batch: it legitimately differs, all of them are listed.
        import hashlib
        import torch.distributed as dist
        gs = _gather_obj(_checksum(opt.gflat), world)
        ws_ = _gather_obj(_checksum(opt.flat), world)
        cs = _gather_obj(hashlib.sha256(repr(model._trainer.last_contra).encode()).hexdigest()[:16], world)
        losses = _gather_obj(float(loss), world)
        ok = all(g == gs[0] for g in gs) and all(w == ws_[0] for w in ws_) and all(c == cs[0] for c in cs) and all(l == l for l in losses) \
            and dist.get_world_size(group) == world
        dp_check = {"ok": bool(ok), "ranks_seen": dist.get_world_size(group), "grad_buffer_checksum_equal": all(g == gs[0] for g in gs),
                    "weights_checksum_equal": all(w == ws_[0] for w in ws_), "negatives_equal": all(c == cs[0] for c in cs),
                    "loss_per_rank": losses, "loss_global_mean": sum(losses) / world}
    traffic, traffic_src = None, "null: no PMC summary of this kernel build / configuration under profiles/"
    if a.arch == "ViT-L/14" and a.n_ctx == 16 and a.batch == 256:
        sys.path.insert(0, str(ROOT / "tools"))
        from pmc_summary import kernel_source_hash
        for pmc in sorted((ROOT / "profiles").glob("r*pmc_summary.json"), reverse=True):
            d = json.load(open(pmc))
            if d.get("kernel_source_hash") == kernel_source_hash() and d.get("config") == "train_l14":
                traffic = d["tower_gemm"]["hbm_bytes_per_launch"]
                traffic_src = f"HBM bytes per GEMM launch (gemm_nt / gemm_tn, rocprofv3 PMC, profiles/{pmc.name})"
                break
    picks = model._trainer.last_contra
    uniq = len({i for ids, _ in picks for i in ids})
    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        # the oracle's OM step (oracle/train_ref.py: fp32 autograd over the functional towers, pinned by the reference's train_batch
        # fixtures) on a REDUCED batch with this step's own negatives, once, at the thread count that runs its image tower fastest.
        # The text-tower passes (len(picks) x <= 257 prompts) do not shrink with the batch, so this UNDER-states the CPU's rate at the
        # full batch; it is a reported baseline, the batch is stated.
        from oracle import train_ref
        cb = max(1, min(4, a.batch))
        plan = model.outer_inner_plan(target)
        wts = [float(model.get_weights("equal", st["M"])[st["m_loop"]] * model.get_weights("equal", st["K"])[st["k_loop"]]) for st in plan]
        sd_cpu = {k: v.detach().float().cpu() for k, v in model.clip_model.state_dict().items()}
        ctx_cpu = model.ctx.detach().float().cpu() if model.ctx is not None else None
        img_cpu = img[:cb].float().cpu()
        threads0 = torch.get_num_threads()
        from oracle import clip_ref
        with torch.no_grad():
            sweep, best = _thread_sweep(lambda: clip_ref.encode_image(sd_cpu, img_cpu[:1]), _thread_candidates())
        torch.set_num_threads(best)
        dt, (ref_loss, _, _) = _timed(lambda: train_ref.om_step(sd_cpu, img_cpu, model.node_tokens.cpu(), picks, wts[:len(picks)], ctx=ctx_cpu))
        torch.set_num_threads(threads0)
        cpu = {"value": round(cb / dt, 3), "unit": "images/sec", "cores": best, "kind": "port",
               "sample": f"ONE oracle OM step (oracle/train_ref.om_step, fp32 autograd, forward + backward of both towers, no optimizer) at batch {cb} "
                         f"with this step's {len(picks)} negative lists ({uniq} distinct prompts): {dt:.1f} s at torch.set_num_threads({best}); the text passes "
                         f"do not shrink with the batch, so the full-batch CPU rate is higher than this figure",
               "oracle_loss_at_that_batch": round(float(ref_loss), 5)}
    l_txt = int(model.node_tokens[:, :].argmax(dim=-1).max().item()) + 1
    fl = 3.0 * tower_forward_flops(cfg, a.batch, uniq, l_txt)
    ms = elapsed / a.steps * 1e3
    if rank == 0:
        line = {"metric": "images/sec, OM training step (model/clip_tree.py:222-281 + clip/AdamW, main.py:79-94)",
                "value": round(a.batch * world * a.steps / elapsed, 1), "unit": "images/sec", "n_gpus": world, "ranks_seen": ranks_seen,
                "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3), "step_ms": step_ms, "higher_is_better": True, "scaling": "weak",
                "vs_baseline": None, "dtype": a.train_dtype, "data": "synthetic",
                "config": {"arch": a.arch, "nodes": a.nodes, "batch_per_gpu": a.batch, "n_ctx": a.n_ctx,
                           "workload": f"{a.arch} OM training step, {a.n_ctx} CoOp context vectors, N={a.nodes} nodes, depth-{len(model.c2p[target])} class: "
                                       f"{len(picks)} inner steps x <= 257 prompts ({uniq} distinct, {l_txt} tokens), batch {a.batch}/GPU",
                           "global_batch": a.batch * world, "parallelism": f"dp{world}", "weights": "random-init (hash-seeded)"},
                "roofline": {"kernel": "whole step (forward + backward GEMMs of both towers)", "bound": "mfma", "achieved": round(fl / (ms * 1e-3) / 1e12, 1),
                             "peak": PEAK_TFLOPS_BF16, "unit": "TFLOP/s", "frac": round(fl / (ms * 1e-3) / 1e12 / PEAK_TFLOPS_BF16, 4), "traffic": traffic, "traffic_unit": traffic_src,
                             "flops_per_step": fl, "note": "3 x forward FLOPs of the executed passes (per rank)"},
                "cpu_baseline": cpu, "loss_first": loss0, "loss_last": loss,
                "parity": {"note": "the true-dimension OM step is checked against oracle/train_ref in tests/test_gpu_training.py "
                                   "(test_vit_l14_coop_true_dimension_om_step_vs_oracle); a CPU oracle step at this batch takes minutes"},
                "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        if dp_check is not None:
            line["dp_check"] = dp_check
            if not dp_check["ok"]:
                log(f"[bench] dp_check FAILED: {json.dumps(dp_check)}")
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if group is not None:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if dp_check is not None and not dp_check["ok"]:
        sys.exit(3)


def main():
    global np, torch                                  # imported after the launcher decision (the parent never loads torch)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    ap.add_argument("--arch", default=ARCH)
    ap.add_argument("--image-dtype", default="f16")
    ap.add_argument("--text-dtype", default="f16")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pcie", dest="pcie", action="store_false", help="skip the PCIe-inclusive (host uint8 input) measurement")
    ap.add_argument("--unfused-eval", action="store_true", help="materialise the logits and run hgr_eval_rows on them (the first build's path)")
    ap.add_argument("--mode", default="eval", choices=["eval", "train"], help="eval: the BASELINE metric (zero-shot step); "
                    "train: one OM training step per step (configs[4] shape with --arch ViT-L/14 --n-ctx 16)")
    ap.add_argument("--n-ctx", type=int, default=0, help="train mode: CoOp learnable context vectors")
    ap.add_argument("--train-dtype", default="bf16")
    ap.add_argument("--no-plant", dest="plant", action="store_false", help="leave the class matrix as the random-init text tower produced it (metric string all zeros)")
    ap.add_argument("--no-c1", dest="c1", action="store_false", help="skip the BASELINE configs[0] CPU line (RN50, N=1000, batch 32)")
    ap.add_argument("--no-secondary", dest="secondary", action="store_false", help="default run only: skip the configs[2] / configs[4] child measurements")
    ap.add_argument("--secondary", dest="is_secondary", action="store_true", help="(internal) this process IS a secondary child: no grandchildren")
    ap.add_argument("--no-host-probe", dest="host_probe", action="store_false", help="default run only: skip the multi-process host-time probe")
    ap.add_argument("--no-power-probe", dest="power_probe", action="store_false", help="skip the rocm-smi power / clock samples taken over extra steps behind the timed region")
    ap.add_argument("--full", action="store_true", help="also run every measurement and check beside the headline (warm update_classifier, "
                    "unblocked host time, power probe, roofline pass, PCIe leg, CPU baseline + parity, dp_check, host probe, secondary configs); "
                    "the --no-* switches above act within it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as DIR/<name>.npy")
    a = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(sys.argv[1:], a.gpus))        # parent: no GPU call before or after this point

    import numpy as np
    import torch

    # stdout carries exactly ONE line (the JSON): libraries that print banners to fd 1 (RCCL's version banner does)
    # are sent to stderr for the whole run, the result is written to the saved original descriptor at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}"
    # HGR_TEST_ONE_GPU=1 (development only): every rank on cuda:0 with the gloo backend, so the multi-rank control flow
    # (sharded text encode + all-gather, batch dealing, counter all-reduce, max-over-ranks timing) can be exercised on a
    # single-GPU box; RCCL itself refuses two ranks on one device.  Never set by the driver.
    one_gpu = os.environ.get("HGR_TEST_ONE_GPU") == "1"
    if one_gpu:
        local = 0
    share = int(os.environ.get("HGR_HOST_SHARE", "0") or 0)
    if share > 1 and hasattr(os, "sched_setaffinity"):
        # host probe: this rank on the cores rank (rank % share) of a `share`-rank job would have to itself
        cores = sorted(os.sched_getaffinity(0))
        per = max(1, len(cores) // share)
        mine = cores[(rank % share) * per:(rank % share + 1) * per] or cores[:per]
        os.sched_setaffinity(0, mine)
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    group = None
    if world > 1 or os.environ.get("HGR_FORCE_DIST") == "1":              # world 1 under torchrun: exercises the RCCL path on one GPU
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(dev))     # "nccl" is RCCL on ROCm
        group = dist.group.WORLD
    ranks_seen = 1
    if group is not None:
        import torch.distributed as dist
        ranks_seen = dist.get_world_size()                     # what the communicator (RCCL) itself reports
        if os.environ.get("HGR_COMM") == "native" and not one_gpu:
            # libhgr's own RCCL communicator (C-ABI collectives, hgr_net_amd.comm) for the blocking exchanges; the process
            # group above only ships the 128-byte unique id
            from hgr_net_amd import comm
            comm.init_from_torch(group)
            ranks_seen = comm.world()

    from hgr_net_amd import evaluate, ops, synth
    from hgr_net_amd.clip.model import build_model
    from hgr_net_amd.hierarchy import build_hierarchy
    from hgr_net_amd.model import tree_model

    t0 = time.time()
    cfg = synth.CLIP_CONFIGS[a.arch]
    sd = synth.clip_state_dict(cfg, 0)
    edges = synth.make_dag(a.nodes, depth=12, seed=7, multi_parent=0.03)
    h = build_hierarchy(edges)
    n_test = int(round(a.nodes * 13442 / 20842))                 # seen/unseen proportion of BASELINE configs[2]
    splits = synth.make_splits(h.nodes, [len(c) == 0 for c in h.p2c], a.nodes - n_test, n_test, 13)
    tokens = synth.make_tokens(a.nodes, 11, cfg["vocab_size"], n_ctx=a.n_ctx if a.mode == "train" else 0)
    tmp = tempfile.mkdtemp(prefix="hgr_bench_")
    gp = os.path.join(tmp, "graph.json")
    json.dump(edges, open(gp, "w"))
    opts = types.SimpleNamespace(device=dev, folder=tmp, exp_name="HGR", weights="equal", out_ratio=0.25, in_ratio=0.5,
                                 from_epoch=-1, graph_path=gp, arch=a.arch, fetch=False, load=False, load_path="none", scale=1.0,
                                 num_compare=256, k=1, sample_strategy="topk", weighting="both", train_dtype=a.train_dtype,
                                 n_ctx=a.n_ctx if a.mode == "train" else 0)
    clip_model = build_model(sd, image_dtype=a.image_dtype, text_dtype=a.text_dtype).to(dev)
    model = tree_model(opts, splits["all"], splits["rest"], node_tokens=tokens, clip_model=clip_model)
    if a.mode == "train":
        train_mode(a, model, cfg, h, rank, world, group, ranks_seen, dev, real_stdout)
        return
    # synthetic single-class batches (every batch is one group), resident in HBM
    base = synth.images(a.batch, cfg["image_resolution"], 1234 + rank).to(dev)
    batches = [base, base.flip(0).contiguous()]
    te = model.test_index.cpu().tolist()
    targets = [te[(7 * i + rank) % len(te)] for i in range(a.steps + a.warmup)]
    log(f"[bench] setup {time.time() - t0:.1f}s: {a.arch}, N={a.nodes} nodes (depth {h.max_depth}), batch {a.batch}/GPU, world {world}")

    t0 = time.time()
    model.update_classifier(group=group)
    torch.cuda.synchronize()
    t_uc_first = time.time() - t0
    uc_info = {"first_call_s": round(t_uc_first, 2), "prompts_per_rank": -(-a.nodes // world)}
    if a.full:
        # once more, warm (prepared weights and workspace exist): what the one-off costs a rank - with N > 1 its own shard of the prompts
        # plus the all-gather of the class rows (hgr_net_amd.parallel.sharded_text_features)
        if group is not None:
            import torch.distributed as dist
            dist.barrier()
        t0 = time.time()
        model.update_classifier(group=group)
        torch.cuda.synchronize()
        t_uc = time.time() - t0
        uc_all = _gather_obj(round(t_uc, 4), world) if world > 1 else [round(t_uc, 4)]
        uc_info = {"s_per_rank_max": max(uc_all), "s_per_rank_min": min(uc_all), **uc_info,
                   "how": "second (warm) call of update_classifier: text tower over this rank's shard of the N prompts" + (" + all-gather of the class rows" if world > 1 else "") + "; one-off per evaluation, outside the timed region"}
        log(f"[bench] update_classifier (text tower, {a.nodes} prompts, one-off, untimed): first {t_uc_first:.2f}s, warm {t_uc:.3f}s")
    else:
        log(f"[bench] update_classifier (text tower, {a.nodes} prompts, one-off, untimed): {t_uc_first:.2f}s")
    model.zsl_unplanted = model.zsl_weights
    # the planted rows are those of EVERY rank's step targets, so that all ranks evaluate against the same class matrix
    all_targets = [te[(7 * i + r) % len(te)] for r in range(world) for i in range(a.steps + a.warmup)]
    planted = plant_signal(model, all_targets, cfg["image_resolution"], dev) if a.plant else None

    ev = evaluate.Evaluator(model)
    # the evaluation loop never looks at the logits themselves: the class-logits GEMM runs with the top-20 / top-1 / per-level
    # arg-max consumers in its epilogue (hgr_logits_eval), nothing [B, N] is written (--unfused-eval: logits + hgr_eval_rows)
    fused_eval = ev.fused_ok() and not a.unfused_eval

    def step(i):
        if fused_eval:
            ev.add_images(batches[i & 1], targets[i])
            return
        logits = model(batches[i & 1], None, static_output=True)      # consumed by add_batch before the next forward
        ev.add_batch(logits, targets[i], want_outputs=False)

    def fence():
        torch.cuda.synchronize()
        if group is not None:
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()

    for i in range(a.warmup):
        step(i)
    fence()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    host_s = 0.0                               # wall time the HOST spends inside step() - Python, two graph launches, Evaluator bookkeeping
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        th = time.perf_counter()
        step(a.warmup + i)
        host_s += time.perf_counter() - th     # (no device sync inside: the queue is a few steps deep, the device is the slower side)
        marks[i + 1].record()                  # stream-ordered marker, no host wait: per-step p50 / p95 beside the loop mean
    fence()
    elapsed = time.perf_counter() - t0
    elapsed_local = elapsed
    step_ms = step_time_stats(marks)
    host_ms_loop = host_s / a.steps * 1e3
    if hasattr(model, "join_tail"):
        model.join_tail()
    if a.dump_outputs:
        # the counters every step advanced (all-reduced with N > 1: every rank takes part), then the last timed step once more with the
        # outputs its caller can ask for - same batch, same target, same class matrix - its counter increments taken back out
        counters = ev.counters(group)
        acc_keep = ev.acc.clone()
        j = a.warmup + a.steps - 1
        if fused_eval:
            pred, path = ev.add_images(batches[j & 1], targets[j], want_outputs=True)
        else:
            pred, path = ev.add_batch(model(batches[j & 1], None, static_output=True), targets[j])
        ev.acc.copy_(acc_keep)
        if rank == 0:
            dump_outputs(a.dump_outputs, {"pred_top20": pred.float().cpu().numpy(), "dict_path": path.float().cpu().numpy(),
                                          "counters": np.array([counters[k] for k in evaluate.COUNTERS], dtype=np.float64)})
    host_ms = power = None
    if a.full:
        # ... inside the loop that figure includes BACK-PRESSURE: a HIP graph cannot be launched again while its previous replay is running,
        # and the steps alternate two graph pairs - the host runs at most two steps ahead and then waits in hipGraphLaunch, so in steady
        # state it reads ~ms_per_step whatever the host's own cost is.  The host's own cost: pairs of steps (one of each parity) behind
        # a fence, when nothing blocks
        host_free = []
        fence()
        acc_keep = ev.acc.clone()                  # (these extra steps must not enter the counters the line and dp_check report)
        for rep in range(4):
            fence()
            th = time.perf_counter()
            step(a.warmup + (2 * rep) % a.steps)
            step(a.warmup + (2 * rep + 1) % a.steps)
            host_free.append((time.perf_counter() - th) / 2 * 1e3)
        fence()
        if hasattr(model, "join_tail"):
            model.join_tail()
        torch.cuda.synchronize()
        if world == 1 and a.power_probe:           # (one rank only: the extra steps are not matched on other ranks)
            power = power_probe(lambda i: step(a.warmup + i % a.steps), fence)
            if hasattr(model, "join_tail"):
                model.join_tail()
            torch.cuda.synchronize()
        ev.acc.copy_(acc_keep)
        host_ms = sorted(host_free)[len(host_free) // 2]
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([elapsed, host_ms or 0.0, host_ms_loop], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, host_ms_loop = float(t[0].item()), float(t[2].item())
        host_ms = float(t[1].item()) if host_ms is not None else None
    ms = elapsed / a.steps * 1e3
    value = a.batch * world * a.steps / elapsed
    dp_check = dp_check_eval(model, ev, group, world, rank, elapsed_local, a.steps, dev) if world > 1 and a.full else None
    summary = ev.summary(group)

    # roofline of the dominant kernel (gemm_nt_128, the tower GEMMs): algorithmic FLOPs of every launch
    # (2*M*N*K) / that launch's duration, from HIP events recorded on the launch stream around each call
    # in a second, instrumented pass over the same steps (events perturb the timed pass, so it is separate).
    roof = None
    if rank == 0 and a.full:
        ops.PROFILE = []
        graph_mode, model.use_graph = model.use_graph, False     # per-launch events need eager launches (a replayed graph has no host calls)
        for i in range(min(a.steps, 5)):
            step(a.warmup + i)
        torch.cuda.synchronize()
        model.use_graph = graph_mode
        recs, ops.PROFILE = ops.PROFILE, None
        tower = [(s_.elapsed_time(e_) * 1e-3, fl, by) for (name, s_, e_, fl, by, tag) in recs if name == "gemm_nt" and tag != "logits" and fl > 2e10]
        if tower:
            tsum = sum(t for t, _, _ in tower)
            fsum = sum(f for _, f, _ in tower)
            ach = fsum / tsum / 1e12
            # HBM bytes per launch of the same kernels come from the rocprofv3 PMC passes of this very command
            # (FETCH_SIZE / WRITE_SIZE, separate runs, gfx950 FETCH x2 correction; tools/pmc_summary.py) - PMC counters
            # cannot be read from inside the process, so a committed summary is quoted ONLY if it was measured on this very
            # build of the kernels (its recorded source hash == tools/pmc_summary.py:kernel_source_hash() now); else null.
            traffic, traffic_src = None, "null: no PMC summary of this kernel build under profiles/ (tools/profile_round.sh regenerates it)"
            want = "vitb32" if (a.arch == ARCH and a.batch == BATCH and a.nodes == N_NODES) else \
                   "rn50" if (a.arch == "RN50" and a.batch == BATCH and a.nodes == 20842) else None
            if want:
                sys.path.insert(0, str(ROOT / "tools"))
                from pmc_summary import kernel_source_hash
                now = kernel_source_hash()
                for pmc in sorted((ROOT / "profiles").glob("r*pmc_summary.json"), reverse=True):
                    d = json.load(open(pmc))
                    if d.get("kernel_source_hash") == now and d.get("config", "vitb32") == want:
                        traffic = d["tower_gemm"]["hbm_bytes_per_launch"]
                        traffic_src = f"HBM bytes per launch (rocprofv3 PMC, profiles/{pmc.name}, kernel sources {now})"
                        break
            roof = {"kernel": "gemm_nt_duo + qkv_attn (image-tower GEMMs: in_proj fused with its attention [tag qkv_mha: GEMM + attention FLOPs], out, fc, proj, patch)" if a.arch.startswith("ViT") else "gemm_nt_256 / gemm_nt_128 (image-tower 1x1 GEMMs and implicit-GEMM 3x3 convolutions)", "bound": "mfma",
                    "achieved": round(ach, 1), "peak": PEAK_TFLOPS_BF16, "unit": "TFLOP/s", "frac": round(ach / PEAK_TFLOPS_BF16, 4),
                    "traffic": traffic, "traffic_unit": traffic_src,
                    "algorithmic_bytes_per_launch": round(sum(b for _, _, b in tower) / len(tower)),
                    "launches": len(tower), "avg_launch_us": round(tsum / len(tower) * 1e6, 1)}
            shapes = {}
            for (name, s_, e_, fl, by, tag) in recs:
                if name == "gemm_nt" and tag != "logits" and fl > 2e10:
                    shapes.setdefault(tag or "untagged", []).append((s_.elapsed_time(e_) * 1e-3, fl))
            roof["by_shape"] = {k: {"launches": len(v), "avg_us": round(sum(t for t, _ in v) / len(v) * 1e6, 1),
                                    "tflops": round(sum(f for _, f in v) / sum(t for t, _ in v) / 1e12, 1)} for k, v in sorted(shapes.items())}
        if roof and power:
            # `peak` is the nominal figure at the 2.4 GHz maximum; under the tower GEMMs the package sits at its power limit and the clock
            # below that: the same peak at the clock the steps actually ran at, and the fraction of THAT
            at = PEAK_TFLOPS_BF16 * power["sclk_mhz"] / 2400.0
            roof["power"] = dict(power, peak_at_sclk=round(at, 1), frac_at_sclk=round(roof["achieved"] / at, 4))
        if roof:
            # the launches of the last image block and the visual head, which act on the class-token rows only ("the last image block")
            small = {}
            for (name, s_, e_, fl, by, tag) in recs:
                if tag in ("kv", "q_cls", "out_cls", "fc_cls", "proj_cls", "head"):
                    small.setdefault(tag, []).append(s_.elapsed_time(e_) * 1e3)
            if small:
                roof["class_token_tail_us"] = {k: round(sum(v) / len(v), 1) for k, v in sorted(small.items())}
        lg = [(s_.elapsed_time(e_) * 1e-3, fl, by) for (name, s_, e_, fl, by, tag) in recs if tag in ("logits", "logits_eval")]     # tagged, not guessed from sizes
        if lg and roof:
            tl = sum(t for t, _, _ in lg) / len(lg)
            roof["logits_gemm"] = {"us": round(tl * 1e6, 1), "tflops": round(lg[0][1] / tl / 1e12, 1),
                                   "frac_mfma": round(lg[0][1] / tl / 1e12 / PEAK_TFLOPS_BF16, 4),
                                   "gbps": round(lg[0][2] / tl / 1e9, 1), "frac_hbm": round(lg[0][2] / tl / 8e12, 4),
                                   "what": ("hgr_logits_eval: logits GEMM + top-20 / top-1 / level arg-max in its epilogue, both stages, no logits written "
                                            "(target of north_star: >= 0.40 of the MFMA peak)") if fused_eval else "hgr_gemm_nt writing fp32 logits (hgr_eval_rows runs behind it)"}
            if fused_eval:
                # the two stages on their own (hgr_logits_eval_tile_stage / _row_stage: the same launches, timed one at a time, eager, after
                # a tower pass so that the operands are as cold as in the step): the tile stage IS the logits GEMM north_star prices
                ops.PROFILE = []
                f16 = torch.empty((a.batch, cfg["embed_dim"]), dtype=model._zsl16.dtype, device=dev)
                for _ in range(5):
                    ops.l2norm_rows(model.clip_model.encode_image(batches[0]), y16=f16)
                    fin = f16 if ev._plan.zsl.shape[1] == f16.shape[1] else torch.cat([f16, f16], dim=1).contiguous()     # (HGR_LOGITS_SPLIT: K doubled)
                    ops.logits_eval(fin, ev._plan, 20, stage="tile")
                    ops.logits_eval(fin, ev._plan, 20, stage="row")
                torch.cuda.synchronize()
                st, ops.PROFILE = ops.PROFILE, None
                for nm in ("tile", "row"):
                    ts = sorted(s_.elapsed_time(e_) * 1e3 for (name, s_, e_, fl, by, tag) in st if tag == "logits_eval_" + nm)
                    if ts:
                        roof["logits_gemm"][nm + "_stage_us"] = round(ts[len(ts) // 2], 1)
                tile = roof["logits_gemm"].get("tile_stage_us")
                if tile:
                    roof["logits_gemm"]["tile_stage_frac_mfma"] = round(lg[0][1] / (tile * 1e-6) / 1e12 / PEAK_TFLOPS_BF16, 4)
                if ev._plan.zsl.shape[1] != f16.shape[1]:
                    # ... and the tile stage on the plain 16-bit class operand (K = D, HGR_LOGITS_SPLIT=none): what the ~22-bit operand of the
                    # default route costs the kernel north_star prices (its K is doubled for the same algorithmic product)
                    ops.PROFILE = []
                    ev._plan.bind(model._zsl16, model._zsl16.shape[1])
                    for _ in range(5):
                        ops.l2norm_rows(model.clip_model.encode_image(batches[0]), y16=f16)
                        ops.logits_eval(f16, ev._plan, 20, stage="tile")
                    torch.cuda.synchronize()
                    st2, ops.PROFILE = ops.PROFILE, None
                    ev._plan.bind(model._eval_class_operand(), model._zsl16.shape[1])
                    ts = sorted(s_.elapsed_time(e_) * 1e3 for (name, s_, e_, fl, by, tag) in st2 if tag == "logits_eval_tile")
                    if ts:
                        t11 = ts[len(ts) // 2]
                        roof["logits_gemm"]["tile_stage_us_plain_16bit_operand"] = round(t11, 1)
                        roof["logits_gemm"]["tile_stage_frac_mfma_plain_16bit_operand"] = round(lg[0][1] / (t11 * 1e-6) / 1e12 / PEAK_TFLOPS_BF16, 4)
                # beside it: the PLAIN product - hgr_gemm_nt writing the fp32 logits (forward()'s kernel on the 11-bit class operand, K = D) -
                # against both of its roofs: 2 B N D flop, 2 B D + 2 N D + 4 B N bytes (the fp32 output co-binds it to HBM, H2)
                n_, d_ = model._zsl16.shape
                ld_ = (n_ + 63) // 64 * 64
                lgt = torch.empty((a.batch, ld_), dtype=torch.float32, device=dev)
                ts = []
                for _ in range(7):
                    ops.l2norm_rows(model.clip_model.encode_image(batches[0]), y16=f16)          # operands as cold as in the step
                    e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0_.record()
                    ops.gemm_nt(f16, model._zsl16, lgt, n=n_)
                    e1_.record()
                    torch.cuda.synchronize()
                    ts.append(e0_.elapsed_time(e1_) * 1e-3)
                tp = sorted(ts)[len(ts) // 2]
                fl_, by_ = 2.0 * a.batch * n_ * d_, 2.0 * a.batch * d_ + 2.0 * n_ * d_ + 4.0 * a.batch * n_
                roof["logits_gemm"]["plain_gemm_nt_fp32_out"] = {"us": round(tp * 1e6, 1), "tflops": round(fl_ / tp / 1e12, 1), "frac_mfma": round(fl_ / tp / 1e12 / PEAK_TFLOPS_BF16, 4),
                                                                "gbps": round(by_ / tp / 1e9, 1), "frac_hbm": round(by_ / tp / 8e12, 4),
                                                                "bound_at_hbm_peak_us": round(by_ / 8e12 * 1e6, 1), "bound_at_mfma_peak_us": round(fl_ / (PEAK_TFLOPS_BF16 * 1e12) * 1e6, 1)}
                del lgt

    # PCIe-inclusive rate (never `value`): the same step fed from pinned HOST memory with uint8 NHWC crops (what a
    # JPEG decoder hands over), H2D on a copy stream double-buffered against compute, normalisation fused into the
    # patch kernel (hgr_im2col_patches_u8).
    pcie = None
    if a.full and a.pcie and cfg["vision_patch_size"]:
        r = cfg["image_resolution"]
        g = torch.Generator().manual_seed(1234 + rank)
        host = [torch.randint(0, 256, (a.batch, r, r, 3), dtype=torch.uint8, generator=g).pin_memory() for _ in range(2)]
        dbuf = [torch.empty((a.batch, r, r, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        cs = torch.cuda.Stream()
        ready = [torch.cuda.Event(), torch.cuda.Event()]
        free = [torch.cuda.Event(), torch.cuda.Event()]
        for e_ in free:
            e_.record()

        def prefetch(i):
            with torch.cuda.stream(cs):
                cs.wait_event(free[i & 1])
                dbuf[i & 1].copy_(host[i & 1], non_blocking=True)
                ready[i & 1].record(cs)

        def ustep(i):
            prefetch(i + 1)
            torch.cuda.current_stream().wait_event(ready[i & 1])
            if fused_eval:
                ev.add_images(dbuf[i & 1], targets[i % len(targets)])
            else:
                logits = model(dbuf[i & 1], None, static_output=True)
                ev.add_batch(logits, targets[i % len(targets)], want_outputs=False)
            free[i & 1].record()

        prefetch(0)
        for i in range(min(3, a.warmup)):
            ustep(i)
        fence()
        base_i = min(3, a.warmup)
        t0 = time.perf_counter()
        for i in range(a.steps):
            ustep(base_i + i)
        fence()
        el = time.perf_counter() - t0
        if world > 1:
            import torch.distributed as dist
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        pcie = {"value": round(a.batch * world * a.steps / el, 1), "unit": "images/sec", "ms_per_step": round(el / a.steps * 1e3, 3),
                "input": f"uint8 NHWC crops in pinned host memory ({a.batch * r * r * 3 / 1e6:.0f} MB/batch), H2D double-buffered on a copy stream"}

    cpu = parity = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        from oracle import tree_ref
        cpu = cpu_baseline(sd, model.zsl_weights.float().cpu(), arch=a.arch, c1=a.c1)
        # the metric's parity clause at full size, on the oracle's batch (same weights, same - planted - class matrix):
        #   logits:  forward() (the drop-in route that returns them) vs the oracle's logits, tolerance 1e-3;
        #   ids:     the TIMED route - Evaluator.add_images -> forward_eval -> hgr_logits_eval, nothing [B, N] written - vs the ids
        #            derived from the oracle's logits by the oracle's own restatement of main.py:131-191 (tree_ref.EvalState);
        #   string:  the metric string of that batch from the HIP counters vs the oracle's string.
        img_c, lg_c = cpu_baseline.last
        dimg_c = img_c.to(dev)
        lg_g = model(dimg_c, None).float().cpu()
        err = float((lg_g - lg_c).abs().max())
        # where that error comes from (round 5): the class-logits GEMM rounds BOTH operands to 16 bits (unit features, unit class rows);
        # against the fp32 product of the SAME fp32 features and class matrix that is the operand-rounding share, the rest is the image
        # tower (the oracle is handed this model's class matrix, so the text tower does not enter)
        f32 = model.clip_model.encode_image(dimg_c).float()
        f32 = f32 / f32.norm(dim=1, keepdim=True)
        lg_f32 = (f32 @ model.zsl_weights.float().t()).cpu()
        err_split = {"operand_rounding_of_the_logits_gemm": round(float((lg_g - lg_f32).abs().max()), 7),
                     "image_tower_features": round(float((lg_f32 - lg_c).abs().max()), 7),
                     "rms": {"operand_rounding": round(float((lg_g - lg_f32).pow(2).mean().sqrt()), 8), "image_tower": round(float((lg_f32 - lg_c).pow(2).mean().sqrt()), 8)}}
        te = model.test_index.cpu()
        # target classes of the parity batches: the step targets with the largest planted weight (so that hits, paths and points
        # actually occur) plus the first timed step's own; the same images are evaluated once per target class
        step_t = list(dict.fromkeys(int(t) for t in targets))
        alpha_of = lambda t: (t * 2654435761) % (1 << 32)
        tg_list = sorted(step_t, key=alpha_of, reverse=True)[:5] + [int(targets[a.warmup])]
        # ... plus step targets whose ancestor path holds the strongest planted node of a level (so that path / point / hit ratios move too)
        planted_nodes = {n_ for t in step_t for n_ in list(model.c2p[t]) + [t]}
        best_of_level = {}
        for n_ in planted_nodes:
            l_ = len(model.c2p[n_])
            if l_ not in best_of_level or alpha_of(n_) > alpha_of(best_of_level[l_]):
                best_of_level[l_] = n_
        score = lambda t: sum(1 for n_ in list(model.c2p[t]) + [t] if best_of_level.get(len(model.c2p[n_])) == n_)
        tg_list = list(dict.fromkeys(tg_list + sorted(step_t, key=score, reverse=True)[:3]))
        ev_p = evaluate.Evaluator(model)
        st = tree_ref.EvalState()
        tr_np, te_np = model.train_index.cpu().numpy(), te.numpy()
        depth_c = model.depth32.cpu().long()
        tr_c = model.train_index.cpu()
        lvl_eq = lvl_tot = lvl_dec = lvl_eq_dec = 0
        rank_diff = rank_diff_dec = 0
        for tgt in tg_list:
            if fused_eval:
                pred_g, path_g = ev_p.add_images(dimg_c, tgt, want_outputs=True)
            else:
                pred_g, path_g = ev_p.add_batch(model(dimg_c, None, static_output=True), tgt)
            pred_g, path_g = pred_g.cpu().long(), path_g.cpu().long()
            pred_o, path_o = st.add_batch(lg_c.numpy(), tgt, model.c2p, model.d2n, tr_np, te_np)
            pred_o, path_o = torch.from_numpy(np.asarray(pred_o)).long(), torch.from_numpy(np.asarray(path_o)).long()
            # rank of the target class among the top-20 (20 = absent), HIP vs oracle; a difference is 'decidable' only when the
            # oracle separates the target from every class it changed places with by more than 2 x the logit error
            rk_g = torch.where((pred_g == tgt).any(1), (pred_g == tgt).float().argmax(1), torch.full((pred_g.shape[0],), 20))
            rk_o = torch.where((pred_o == tgt).any(1), (pred_o == tgt).float().argmax(1), torch.full((pred_o.shape[0],), 20))
            for rix in torch.nonzero(rk_g != rk_o).flatten().tolist():
                rank_diff += 1
                lo_, hi_ = int(min(rk_g[rix], rk_o[rix])), int(max(rk_g[rix], rk_o[rix]))
                others = [int(c) for c in pred_o[rix, lo_:min(hi_ + 1, 20)].tolist() if int(c) != tgt]
                gap = min(abs(float(lg_c[rix, tgt]) - float(lg_c[rix, c])) for c in others) if others else 0.0
                rank_diff_dec += int(gap > 2 * err)
            for j, node in enumerate(list(model.c2p[tgt]) + [tgt]):               # per ancestor level: is the oracle's arg-max decided?
                cols_l = tr_c[depth_c[tr_c] == len(model.c2p[node])]
                eq = path_g[:, j] == path_o[:, j]
                dec = torch.ones_like(eq)
                if cols_l.numel() >= 2:
                    v2 = lg_c[:, cols_l].topk(2, dim=1).values
                    dec = (v2[:, 0] - v2[:, 1]) > 2 * err
                lvl_eq += int(eq.sum()); lvl_tot += int(eq.numel()); lvl_dec += int(dec.sum()); lvl_eq_dec += int((eq & dec).sum())
        sub_c = lg_c[:, te]
        top21 = sub_c.topk(21, dim=1)
        gaps = top21.values[:, :-1] - top21.values[:, 1:]
        decidable = gaps[:, 0] > 2 * err                                          # outside the error band of the two paths
        dec20 = (gaps > 2 * err).all(dim=1)
        same = pred_g[:, 0] == pred_o[:, 0]
        same20 = (pred_g == pred_o).all(dim=1)
        string_g, string_o = ev_p.summary().strip(), st.summary().strip()
        parity = {"images": int(img_c.shape[0]), "max_abs_logit_err": round(err, 6), "tolerance": 1e-3, "logit_err_decomposition": err_split,
                  "ids_from": "hgr_logits_eval (the timed, fused route)" if fused_eval else "hgr_eval_rows on forward() logits",
                  "hit1_equal": int(same.sum()), "hit1_decidable": int(decidable.sum()), "hit1_equal_decidable": int((same & decidable).sum()),
                  "top20_rows_equal": int(same20.sum()), "top20_rows_decidable": int(dec20.sum()), "top20_rows_equal_decidable": int((same20 & dec20).sum()),
                  "level_ids_equal": lvl_eq, "level_ids_total": lvl_tot, "level_ids_decidable": lvl_dec, "level_ids_equal_decidable": lvl_eq_dec,
                  "target_classes": len(tg_list), "target_rank_differs": rank_diff, "target_rank_differs_decidable": rank_diff_dec,
                  "metrics_string_hip": string_g, "metrics_string_oracle": string_o, "metrics_string_equal": string_g == string_o,
                  "metrics_string_explained": string_g == string_o or (rank_diff_dec == 0 and lvl_eq_dec == lvl_dec),
                  "note": "logit error: forward() vs the CPU oracle's logits of every slice its timing leg ran (one HIP batch of all of them); ids and the "
                          "metric string of those images evaluated once per target class (the 5 step targets with the largest planted weight + the first timed step's): timed route vs oracle/tree_ref.EvalState on the oracle's "
                          "logits; 'decidable' = the oracle's margins at the compared ranks exceed 2 x the max logit error; the strings may differ by the undecidable samples only "
                          "(target_rank_differs - target_rank_differs_decidable of images x target_classes samples): metrics_string_explained"}

    if rank == 0:
        # short scalar copies of the nested blocks (a record that keeps only the scalar fields of `roofline` / `config` still shows them)
        if roof:
            for k_, v_ in (roof.get("by_shape") or {}).items():
                roof["us_" + k_] = v_.get("avg_us")
            tail_ = roof.get("class_token_tail_us") or {}
            if tail_:
                roof["us_cls_tail_wo_kv"] = round(sum(v for k, v in tail_.items() if k != "kv"), 1)
            lgm = roof.get("logits_gemm") or {}
            for k_, n_ in (("us", "us_logits_eval"), ("tile_stage_us", "us_logits_tile"), ("tile_stage_frac_mfma", "frac_logits_tile"), ("row_stage_us", "us_logits_row")):
                if k_ in lgm:
                    roof[n_] = lgm[k_]
            pl_ = lgm.get("plain_gemm_nt_fp32_out") or {}
            if pl_:
                roof["us_logits_plain"], roof["frac_logits_plain_mfma"], roof["frac_logits_plain_hbm"] = pl_["us"], pl_["frac_mfma"], pl_["frac_hbm"]
        parity_short = None
        if parity:
            parity_short = (f"hit1 {parity['hit1_equal']}/{parity['images']} top20rows {parity['top20_rows_equal']}/{parity['images']} "
                            f"levelids {parity['level_ids_equal']}/{parity['level_ids_total']} maxerr {parity['max_abs_logit_err']:.1e} string_equal {parity['metrics_string_equal']}")
        line = {"metric": "images/sec over 21K-class hierarchy, batch 512; hit@1 parity vs reference",
                "value": round(value, 1), "unit": "images/sec", "n_gpus": world, "ranks_seen": ranks_seen, "steps": a.steps, "warmup": a.warmup,
                "ms_per_step": round(ms, 3), "step_ms": step_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                # max over ranks: what one rank's host thread spends per step when nothing blocks it (Python + two graph launches + Evaluator
                # bookkeeping; median of 4 unblocked pairs) / the same inside the timed loop, where graph re-launch back-pressure is included
                "host_ms_per_step": round(host_ms, 3) if host_ms is not None else None, "host_ms_per_step_in_loop": round(host_ms_loop, 3),
                "dtype": a.image_dtype, "data": "synthetic",
                "config": {"arch": a.arch, "nodes": a.nodes, "batch_per_gpu": a.batch, "embed_dim": cfg["embed_dim"],
                           "workload": f"{a.arch} zero-shot eval step: encode_image + L2 + [{a.batch}x{cfg['embed_dim']}]x[{cfg['embed_dim']}x{a.nodes}] logits "
                                       f"+ top-20/top-1/level-argmax metrics (main.py:131-191; {'fused into the logits GEMM' if fused_eval else 'hgr_eval_rows on materialised logits'}), N={a.nodes} nodes, batch {a.batch}/GPU",
                           "tower_notes": ("LayerNorms folded into the GEMMs; the last image block runs out_proj / MLP / its attention row on the class-token rows only - "
                                           "the rows ln_post reads (clip/model.py:231), same bits; HGR_CLS_LAST=0 carries every token") if cfg["vision_patch_size"] else
                                          "ModifiedResNet: NHWC 16-bit activations, BatchNorm folded, 1x1 convolutions as GEMMs, 3x3 as implicit GEMMs",
                           "global_batch": a.batch * world, "parallelism": f"dp{world}", "text_dtype": a.text_dtype,
                           "weights": "random-init (hash-seeded), no checkpoint offline", "parity_ids": parity_short},
                "roofline": roof, "cpu_baseline": cpu, "parity": parity, "pcie_inclusive": pcie, "metrics_string": summary.strip(),
                "planted_signal": planted, "update_classifier": uc_info}
        if dp_check is not None:
            line["dp_check"] = dp_check
            if not dp_check["ok"]:
                log(f"[bench] dp_check FAILED: {json.dumps(dp_check)}")
        default_run = a.full and a.arch == ARCH and a.batch == BATCH and a.nodes == N_NODES and world == 1 and group is None
        if a.host_probe and not a.is_secondary and default_run:
            # 8-GPU readiness that one GPU can show: the per-rank HOST cost of a step with several ranks' processes sharing the box's
            # cores (an 8-GPU node runs 8 of these next to each other; what caps weak scaling is a host that cannot keep 8 queues
            # fed).  HOST_PROBE_RANKS ranks time-share THIS GPU over gloo (HGR_TEST_ONE_GPU=1: RCCL refuses two ranks per device, and
            # a GPU box admits at most 6 processes on its card - this one included), so their ms_per_step means nothing - host_ms_per_step does.
            log(f"[bench] host probe: {HOST_PROBE_RANKS} ranks time-sharing the GPU (gloo), host time per step")
            hp = run_secondary(["--gpus", str(HOST_PROBE_RANKS), "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-pcie", "--no-c1", "--no-plant"], 300,
                               env_extra={"HGR_TEST_ONE_GPU": "1", "HGR_HOST_SHARE": str(HOST_PROBE_SHARE)}, keep_extra=("host_ms_per_step", "n_gpus"))
            line["host_probe"] = {"ranks": HOST_PROBE_RANKS, "cores_per_rank": max(1, len(os.sched_getaffinity(0)) // HOST_PROBE_SHARE) if hasattr(os, "sched_getaffinity") else None,
                                  "host_ms_per_step": hp.get("host_ms_per_step"), "host_cores": os.cpu_count(),
                                  "share_of_step": round(hp["host_ms_per_step"] / ms, 3) if hp.get("host_ms_per_step") else None,
                                  "note": f"max over {HOST_PROBE_RANKS} concurrent ranks (what a one-GPU box admits beside this process), each confined to 1/{HOST_PROBE_SHARE} "
                                          f"of this host's cores - the share of a rank of an 8-GPU job; the GPU is time-shared, so only the host figure is meaningful",
                                  **({"error": hp["error"], "stderr_tail": hp.get("stderr_tail")} if "error" in hp else {})}
            line[f"host_ms_per_step_{HOST_PROBE_RANKS}proc"] = hp.get("host_ms_per_step")
        if a.secondary and not a.is_secondary and default_run:
            # BASELINE configs[2] and configs[4] beside the headline, each as a child process after the headline measurement is over
            # (its memory is released first): same harness, own JSON line, reduced here
            del ev, model, clip_model
            torch.cuda.empty_cache()
            log("[bench] secondary: configs[2] RN50 + hierarchy, N=20842, batch 512")
            sec = {"rn50_hier": run_secondary(["--arch", "RN50", "--nodes", "20842", "--steps", "15", "--warmup", "3", "--no-pcie", "--no-c1"], 280)}
            log("[bench] secondary: configs[4] ViT-L/14 + 16 CoOp context vectors, OM training step, batch 256")
            sec["train_l14_coop"] = run_secondary(["--mode", "train", "--arch", "ViT-L/14", "--n-ctx", "16", "--batch", "256", "--steps", "3", "--warmup", "2"], 420)
            line["secondary"] = sec
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if group is not None:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if dp_check is not None and not dp_check["ok"]:
        sys.exit(3)                                        # every rank: torch.distributed.run reports the failure


if __name__ == "__main__":
    main()
