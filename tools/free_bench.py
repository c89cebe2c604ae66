#!/usr/bin/env python3
"""FREE validation route at the reference's sizes on SYNTHETIC material (A = nz = 1024, ngh = 4096, N = 18 278 classes, batches of
512 real + 1000 synthetic rows): one process, one GPU, the routes interleaved round by round, medians over the rounds.

  synthesis            rows / s of free.synthesize
  fit step             ms of FREEClassifier.step: fused, with HGR_FREE_NLL_FUSED=0, with HGR_FREE_ADAM_FUSED=0, and the same
                       arithmetic restated in torch ops (bf16 matmuls, log_softmax, the closed-form gradient, Adam by hand)
  kernels              each new kernel alone beside its byte floor (bytes moved / ms = GB/s)

A sample is STEP_REPS steps or KERNEL_REPS kernel calls back to back between two events; every figure is the median of --rounds
samples with their minimum and maximum beside it.  Prints one JSON line.  Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402

from hgr_net_amd import ops                                            # noqa: E402
from hgr_net_amd.baseline import free                                  # noqa: E402
from hgr_net_amd.baseline.dgp_eval import ListTree                     # noqa: E402

DEV = "cuda:0"
STEP_REPS, KERNEL_REPS, WARMUP = 5, 20, 3


def timed(fn, reps: int = 1) -> float:
    """ms per call: `reps` calls back to back between two events (a sample of one short kernel would mostly time the launch)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def spread(samples) -> dict:
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4), "max": round(max(samples), 4)}


def make_classifier(netG, netFR, tree, te, att, n, syn, nll: bool, adam: bool):
    os.environ["HGR_FREE_NLL_FUSED"], os.environ["HGR_FREE_ADAM_FUSED"] = str(int(nll)), str(int(adam))
    return free.FREEClassifier(netG, netFR, tree, te, att, n, dtype="bf16", seed=1, syn=syn)


class TorchStep:
    """The step's arithmetic in torch ops on the same GPU (bf16 operands, fp32 accumulation, fp32 master weights and moments)."""

    def __init__(self, cl):
        self.fr, self.b = cl.netFR, cl.batch_size
        self.w, self.bias = cl.wp[:cl.nclass].clone(), cl.bp[:cl.nclass].clone()
        self.m, self.v, self.mb, self.vb = (torch.zeros_like(t) for t in (self.w, self.w, self.bias, self.bias))
        self.w16, self.t = self.w.bfloat16(), 0
        self.f1, self.f3 = self.fr.fc1.weight.data.bfloat16(), self.fr.fc3.weight.data.bfloat16()

    def adam(self, p, g, m, v, lr=1e-3, b1=0.5, b2=0.999, eps=1e-8):
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        p.addcdiv_(m, v.sqrt().div_((1 - b2 ** self.t) ** 0.5).add_(eps), value=-lr / (1 - b1 ** self.t))

    def step(self, x16, labels):
        a = self.fr.attSize
        hidden = torch.nn.functional.leaky_relu((x16 @ self.f1.t()).float() + self.fr.fc1.bias.data, 0.2).bfloat16()
        lat = (hidden @ self.f3.t()).float() + self.fr.fc3.bias.data
        h = torch.sigmoid(lat[:, :a] + torch.randn_like(lat[:, :a]) * torch.sigmoid(lat[:, a:])).bfloat16()
        big = torch.cat((x16, hidden, h), 1)
        logp = torch.log_softmax((big @ self.w16.t()).float() + self.bias, 1)
        loss = -logp.gather(1, labels[:, None]).mean()
        d = logp.exp_()
        d.scatter_add_(1, labels[:, None], torch.full((len(labels), 1), -1.0, device=d.device))
        d16 = d.bfloat16()
        self.t += 1
        self.adam(self.w, (d16.t() @ big).float().div_(self.b), self.m, self.v)
        self.adam(self.bias, d16.float().sum(0).div_(self.b), self.mb, self.vb)
        self.w16 = self.w.bfloat16()
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--classes", type=int, default=18278)
    ap.add_argument("--syn-classes", type=int, default=200)
    args = ap.parse_args()
    a, ngh, n, real, syn_b = 1024, 4096, args.classes, 512, 1000
    opt = free.make_opt(attSize=a, ngh=ngh, latensize=ngh // 2)
    netG, netFR = free.Generator(opt), free.FR(opt, a)
    netG.load_state_dict({k: torch.from_numpy(v) for k, v in free.synth_state(0, opt, "netG").items()})
    netFR.load_state_dict({k: torch.from_numpy(v) for k, v in free.synth_state(0, opt, "netFR").items()})
    netG, netFR = netG.to(DEV).eval(), netFR.to(DEV).eval()
    att = torch.nn.functional.normalize(torch.randn(n, a, generator=torch.Generator().manual_seed(0)), dim=1).to(DEV)
    te = np.arange(983, 983 + args.syn_classes)
    depth = np.zeros(n, dtype=np.int32)
    tree = ListTree([str(i) for i in range(n)], [[] for _ in range(n)], depth, {0: list(range(n))}, 1)
    out = {"sizes": {"A": a, "ngh": ngh, "N": n, "batch": real + syn_b}, "material": "SYNTHETIC"}
    syn = free.synthesize(netG, te, att, 100, seed=1)
    torch.cuda.synchronize()
    ts = [timed(lambda: free.synthesize(netG, te, att, 100, seed=1), STEP_REPS) for _ in range(args.rounds)]
    out["synthesis_ms"] = spread(ts)
    out["synthesis_rows_per_s"] = round(len(te) * 100 / (statistics.median(ts) * 1e-3))
    routes = {"fused": make_classifier(netG, netFR, tree, te, att, n, syn, True, True),
              "nll_unfused": make_classifier(netG, netFR, tree, te, att, n, syn, False, True),
              "adam_unfused": make_classifier(netG, netFR, tree, te, att, n, syn, True, False)}
    ref = TorchStep(routes["fused"])
    x = torch.rand(real, free.RES, device=DEV)
    y = torch.randint(0, 983, (real,), device=DEV)
    x16 = torch.cat((x, syn[0][:syn_b].float()), 0).bfloat16()
    y_all = torch.cat((y, syn[1][:syn_b]))
    times = {k: [] for k in list(routes) + ["torch"]}
    for r in range(args.rounds + WARMUP):
        for k, cl in routes.items():
            t = timed(lambda: cl.step(x, y), STEP_REPS)
            if r >= WARMUP:
                times[k].append(t)
        t = timed(lambda: ref.step(x16, y_all), STEP_REPS)
        if r >= WARMUP:
            times["torch"].append(t)
    out["fit_step_ms"] = {k: spread(v) for k, v in times.items()}
    # the kernels alone
    cl = routes["fused"]
    b, npad, k = cl.batch_size, cl.npad, cl.input_dim
    logits, lab = torch.randn(b, npad, device=DEV), y_all.to(torch.int32)
    loss, d16, d32 = torch.empty(b, device=DEV), torch.empty(b, npad, dtype=torch.bfloat16, device=DEV), torch.zeros(b, npad, device=DEV)
    part = cl._bufs["part"]
    s = part.shape[0]
    lat = torch.randn(b, 2 * a, device=DEV)
    hid = torch.randn(b, ngh, device=DEV)
    big = torch.empty(b, k, dtype=torch.bfloat16, device=DEV)
    inp = torch.empty(20000, 2 * a, dtype=torch.bfloat16, device=DEV)
    cls32 = torch.from_numpy(te.astype(np.int32)).to(DEV)
    gw = torch.empty(npad, k, device=DEV)
    cs = torch.empty(npad * k, device=DEV)
    nw = npad * k
    kernels = {
        "nll_rows16": (lambda: ops.nll_rows16(logits, lab, n=n, loss_rows=loss, dlogits=d16), 6 * b * npad),
        "ce_rows+cast16": (lambda: (ops.ce_rows(logits[:, :n], lab, loss, d32), ops.cast16(d32, d16)), 3 * 4 * b * npad + 4 * b * npad + 4 * b * npad + 2 * b * npad),
        "adam_l2_cast16": (lambda: ops.adam_l2_cast16(cl.wp, part, cl.mw, cl.vw, cl.w16, 1e-3, 1, slices=s, alpha=1 / b, betas=(0.5, 0.999)), nw * (4 * (s + 3) + 14)),
        "colsum+adam_l2+cast16": (lambda: (ops.colsum(part.view(s, nw), gw.view(-1), cs, accumulate=False, alpha=1 / b), ops.adam_l2(cl.wp, gw, cl.mw, cl.vw, 1e-3, 1, (0.5, 0.999)),
                                           ops.cast16(cl.wp, cl.w16)), nw * (4 * s + 4 + 16 + 12 + 4 + 2)),
        "bias_act_rows": (lambda: ops.bias_act_rows(hid, netFR.fc1.bias.data, big, ops.ACT_LRELU02, col0=free.RES), b * ngh * 6),
        "free_fr_tail": (lambda: ops.free_fr_tail(lat, big, col0=free.RES + ngh, bias=netFR.fc3.bias.data, seed=1, stream=1), b * a * 10),
        "free_gen_input": (lambda: ops.free_gen_input(inp, att, cls32, 100, a, seed=1), 20000 * (2 * a * 2 + a * 4)),
    }
    out["kernels"] = {}
    for name, (fn, byts) in kernels.items():
        timed(fn, WARMUP)
        ts = [timed(fn, KERNEL_REPS) for _ in range(args.rounds)]
        ms = statistics.median(ts)
        out["kernels"][name] = {"ms": spread(ts), "bytes": int(byts), "GB_per_s": round(byts / ms * 1e-6)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
