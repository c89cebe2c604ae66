"""Dev-tool helpers: operand sets of the tower GEMM forms through the public entry points (hgr_gemm_nt, hgr_gemm_nt_ln,
hgr_gemm_nt_res_stats_guard) and an event timer.  Every case keeps two output sets; run(slot) writes set `slot`, so that an A/B tool
can run two settings of a knob side by side and compare the sets for bits (same()).  Used by tools/p8_bench.py,
tools/duo_dma_ablate.py and tools/experiments/."""
import torch
from hgr_net_amd import ops
from hgr_net_amd._lib import EPI_NONE


def mk(m, n, k, dt=torch.float16, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = ((torch.rand(m, k, device="cuda", generator=g) * 2 - 1)).to(dt)
    w = ((torch.rand(n, k, device="cuda", generator=g) * 2 - 1) * 0.05).to(dt)
    return a, w, g


class Plain:
    def __init__(self, m, n, k, epi, dt=torch.float16):
        self.a, self.w, g = mk(m, n, k, dt)
        self.bias = torch.rand(n, device="cuda", generator=g) - 0.5 if epi != EPI_NONE else None
        self.epi, self.flops = epi, 2.0 * m * n * k
        self.out = [torch.full((m, n), float("nan"), dtype=dt, device="cuda") for _ in range(2)]

    def run(self, slot):
        ops.gemm_nt(self.a, self.w, self.out[slot], bias=self.bias, epilogue=self.epi)

    def same(self):
        return bool(torch.equal(self.out[0].view(torch.int16), self.out[1].view(torch.int16)))


class LnC:
    def __init__(self, m, n, k, act, dt=torch.float16):
        self.a, self.w, g = mk(m, n, k, dt)
        self.s = torch.rand(n, device="cuda", generator=g) - 0.5
        self.c = torch.rand(n, device="cuda", generator=g) - 0.5
        x = self.a.float().view(m, k // 64, 64)
        self.stats = torch.stack([x.sum(-1), (x * x).sum(-1)], dim=-1).contiguous()
        self.act, self.flops = act, 2.0 * m * n * k
        self.out = [torch.full((m, n), float("nan"), dtype=dt, device="cuda") for _ in range(2)]

    def run(self, slot):
        ops.gemm_nt_ln(self.a, self.w, self.out[slot], self.s, self.c, self.stats, quickgelu=self.act)

    def same(self):
        return bool(torch.equal(self.out[0].view(torch.int16), self.out[1].view(torch.int16)))


class LnP:
    def __init__(self, m, n, k, dt=torch.float16):
        self.a, self.w, g = mk(m, n, k, dt)
        self.bias = torch.rand(n, device="cuda", generator=g) - 0.5
        self.xh0 = (torch.rand(m, n, device="cuda", generator=g) * 4 - 2).to(dt)
        self.xl0 = torch.randint(0, 256, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
        self.flops = 2.0 * m * n * k
        self.xh = [torch.empty_like(self.xh0) for _ in range(2)]
        self.xl = [torch.empty_like(self.xl0) for _ in range(2)]
        self.st = [torch.full((m, n // 64, 2), float("nan"), device="cuda") for _ in range(2)]
        self.flag = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]

    def reset(self):
        for i in range(2):
            self.xh[i].copy_(self.xh0); self.xl[i].copy_(self.xl0)

    def run(self, slot):
        ops.gemm_nt_res_stats(self.a, self.w, self.xh[slot], self.xl[slot], self.bias, self.st[slot], flag=self.flag[slot])

    def same(self):
        return bool(torch.equal(self.xh[0].view(torch.int16), self.xh[1].view(torch.int16)) and torch.equal(self.xl[0], self.xl[1])
                    and torch.equal(self.st[0].view(torch.int32), self.st[1].view(torch.int32)) and int(self.flag[0]) == int(self.flag[1]))


def timeit(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3
