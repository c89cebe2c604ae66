#!/usr/bin/env python3
"""Times the DGP baseline's ResNet-50 (baseline/resnet.py) on one MI355X: batch 256 x 224 x 224, f16, SYNTHETIC weights and images.
One process, device events, the routes of every comparison interleaved round by round (A B A B ...), medians reported:

  forward   the whole net with the fused stem (hgr_stem7_pool) and with HGR_TV_STEM_FUSED=0's route, beside the same network in
            torch's own half-precision operations (conv2d / batch_norm / max_pool2d, channels_last) on the same GPU
  stem      hgr_stem7_pool against hgr_stem7_im2col + gemm_nt + hgr_maxpool3s2_nhwc, and the fused launch beside its byte floor:
            the fp32 image read once + the pooled tensor written once (257 MB at this size) at the 8.0 TB/s HBM peak and at the
            6.3 TB/s a copy reaches

Prints one JSON line per section as soon as it is measured (`--no-torch` leaves the torch network out)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch                                                           # noqa: E402
import torch.nn.functional as F                                        # noqa: E402

from hgr_net_amd import ops, synth                                     # noqa: E402
from hgr_net_amd.baseline import resnet                                # noqa: E402


def interleaved(routes: dict, rounds: int, warmup: int) -> dict:
    """{name: median ms}: every round runs every route once, in turn."""
    times = {k: [] for k in routes}
    for i in range(warmup + rounds):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def torch_half_net(sd, dev):
    """The same network in torch's own half-precision operations (inference BatchNorm kept as its own op, as torch users run it)."""
    w = {k: (v.to(dev).half() if v.dtype == torch.float32 else v.to(dev)) for k, v in sd.items()}
    for k in list(w):
        if k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight") or k.endswith("downsample.0.weight"):
            w[k] = w[k].contiguous(memory_format=torch.channels_last)

    def cbn(t, conv, bn, stride=1, padding=0):
        t = F.conv2d(t, w[conv + ".weight"], None, stride=stride, padding=padding)
        return F.batch_norm(t, w[bn + ".running_mean"], w[bn + ".running_var"], w[bn + ".weight"], w[bn + ".bias"], False, 0.0, 1e-5)

    @torch.no_grad()
    def run(x):
        a = F.max_pool2d(F.relu(cbn(x.half().contiguous(memory_format=torch.channels_last), "conv1", "bn1", 2, 3)), 3, 2, 1)
        for li in (1, 2, 3, 4):
            j = 0
            while f"layer{li}.{j}.conv1.weight" in w:
                p, stride = f"layer{li}.{j}", 2 if (li > 1 and j == 0) else 1
                t = F.relu(cbn(a, p + ".conv1", p + ".bn1"))
                t = F.relu(cbn(t, p + ".conv2", p + ".bn2", stride, 1))
                idn = cbn(a, p + ".downsample.0", p + ".downsample.1", stride) if p + ".downsample.0.weight" in w else a
                a = F.relu(cbn(t, p + ".conv3", p + ".bn3") + idn)
                j += 1
        return a.flatten(2).mean(2)
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("dgp_resnet_bench needs the GPU: nothing is timed on the CPU")
    dev, dt = "cuda:0", torch.float16
    b, r = args.batch, args.size
    sd = synth.resnet_state_dict("resnet50", 0)
    net = resnet.make_resnet_base("resnet50")
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    one = synth.images(8, r, 1234).to(dev)
    x = one.repeat((b + 7) // 8, 1, 1, 1)[:b].contiguous()
    say = lambda **kw: print(json.dumps(dict(kw, batch=b, size=r, dtype="f16", data="SYNTHETIC")), flush=True)

    # ---- the stem alone
    w1, b1 = net._prepared()["stem"]
    hc, hp = ops.stem7_geometry(r)
    pooled = torch.empty((b * hp * hp, 64), dtype=dt, device=dev)
    pooled_u = torch.empty_like(pooled)
    col = torch.empty((b * hc * hc, w1.shape[1]), dtype=dt, device=dev)
    c1 = torch.empty((b * hc * hc, 64), dtype=dt, device=dev)

    def unfused():
        ops.stem7_im2col(x, col)
        ops.gemm_nt(col, w1, c1, bias=b1, epilogue=ops.EPI_BIAS_RELU)
        ops.maxpool3s2_nhwc(c1, pooled_u, b, hc, hc, 64)
    res = interleaved({"fused": lambda: ops.stem7_pool(x, w1, b1, pooled), "unfused": unfused}, args.rounds, args.warmup)
    floor_bytes = x.numel() * 4 + pooled.numel() * 2
    say(section="stem", **res, floor_mb=round(floor_bytes / 1e6, 1), floor_ms_at_8_0_tbs=round(floor_bytes / 8.0e9, 4),
        floor_ms_at_6_3_tbs=round(floor_bytes / 6.3e9, 4), same_bits=bool(torch.equal(pooled, pooled_u)),
        max_abs_diff=float((pooled.float() - pooled_u.float()).abs().max()))

    # ---- the whole forward, both stems
    def forward(fused):
        def run():
            resnet.STEM_FUSED = fused
            return net(x)
        return run
    keep = resnet.STEM_FUSED
    routes = {"hgr_fused_stem": forward(True), "hgr_unfused_stem": forward(False)}
    say(section="forward", **interleaved(routes, args.rounds, args.warmup))
    if not args.no_torch:
        tnet = torch_half_net(sd, dev)
        ref = tnet(x[:8]).float()
        resnet.STEM_FUSED = True
        err = float((net(x[:8]) - ref).abs().max())
        print(f"torch half network built; max |hgr - torch half| on 8 images = {err:.4f} (max |feature| {float(ref.abs().max()):.2f})", flush=True)
        routes["torch_half"] = lambda: tnet(x)
        say(section="forward_vs_torch", **interleaved(routes, args.rounds, args.warmup))
    resnet.STEM_FUSED = keep


if __name__ == "__main__":
    main()
