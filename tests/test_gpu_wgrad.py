"""GPU: hgr_net_amd.wgrad.WeightGrad.add driven directly, on the smallest shapes at which each of its branches can go wrong:
TN with one / several slices on 128- and 256-tiles, the 3x3 loader, the transposing fallback with split-K and with the
accumulate epilogue, exact-width and K-padded accumulators, every form of the bias gradient.

Expected values: float64 dY^T . X on the CPU.  Small-integer operands make every fp32 sum exact in any order, so those
comparisons are bit for bit; one pass of random operands per case is held to the forward error bound of an fp32 sum of
n = m + slices + 1 terms, gamma_n = n u / (1 - n u) with u = 2^-24 (products of two 16-bit values are exact in fp32).
Accumulators and bias gradients sit between guard bands; the bands and the padding columns must keep their sentinel."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops, wgrad

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]
GUARD, SENTINEL = 64, -1234.5
U = 2.0 ** -24

# name: route, cout, k (conv: 9 C), m, accumulator width, slices, operand layout
#   lay = (dy buffer width, dy first column, x buffer width, x first column); conv: (b, h, C)
CASES = {
    "1 tn one slice, strided operands": dict(route="tn", cout=136, k=72, m=300, kw=72, slices=1, lay=(152, 8, 88, 8)),
    "2 tn two slices": dict(route="tn", cout=136, k=72, m=1100, kw=72, slices=2, lay=(136, 0, 72, 0)),
    "3 tn 256-tile, two slices": dict(route="tn", cout=256, k=256, m=1100, kw=256, slices=2, lay=(256, 0, 256, 0)),
    "4a tn one slice, padded gw": dict(route="tn", cout=136, k=72, m=300, kw=128, slices=1, lay=(152, 8, 88, 8)),
    "4b tn two slices, padded gw": dict(route="tn", cout=136, k=72, m=1100, kw=128, slices=2, lay=(136, 0, 72, 0)),
    "5 conv one slice, padded gw": dict(route="tn_conv", cout=16, k=72, m=720, kw=128, slices=1, conv=(5, 12, 8)),
    "6 conv six slices": dict(route="tn_conv", cout=64, k=576, m=3136, kw=576, slices=6, conv=(4, 28, 64)),
    "7 nt k=588 in a 640-wide x": dict(route="nt", cout=136, k=588, m=300, kw=588, slices=5, lay=(136, 0, 640, 0)),
    "8a nt one slice, EPI_ACCUM": dict(route="nt", cout=40, k=20, m=50, kw=20, slices=1, lay=(40, 0, 20, 0)),
    "8b nt one slice, padded gw": dict(route="nt", cout=40, k=20, m=50, kw=64, slices=1, lay=(40, 0, 20, 0)),
    "9a nt dy row stride 140": dict(route="nt", cout=136, k=72, m=300, kw=72, slices=5, lay=(140, 0, 72, 0), dy_unaligned=True),
    "9b nt dy row stride 140, padded gw": dict(route="nt", cout=136, k=72, m=300, kw=128, slices=5, lay=(140, 0, 72, 0), dy_unaligned=True),
}
BIAS = ["none", "dy16", "dy_colsum"]


def _operands(name, kind, dt):
    """dy [m, cout], x [m, k] (conv: [m, C]) as 16-bit CPU tensors: integers in [-2, 2], or normal values rounded to dt."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) * 2 + (kind == "random"))
    xc = c["conv"][2] if "conv" in c else c["k"]
    if kind == "int":
        dy, x = (torch.randint(-2, 3, (c["m"], n), generator=gen).float() for n in (c["cout"], xc))
    else:
        dy, x = (torch.randn((c["m"], n), generator=gen) * 0.5 for n in (c["cout"], xc))
    return dy.to(dt), x.to(dt)


def _product(c, dy, x):
    """float64 dY^T . X, or dY^T . im2col(X) in (ky, kx, c) order through autograd's conv2d weight gradient."""
    if "conv" not in c:
        return dy.t() @ x
    b, h, ch = c["conv"]
    w = torch.zeros(c["cout"], ch, 3, 3, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(x.view(b, h, h, ch).permute(0, 3, 1, 2), w, padding=1)
    out.backward(dy.view(b, h, h, c["cout"]).permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(c["cout"], 9 * ch)


@functools.lru_cache(maxsize=None)
def _reference(name, kind, dt):
    """(dy16, x16, dW, sum |dy| |x|, column sums of dy, of |dy|), the last four in float64; computed once per key, read only.
    The integer operands are the same values in both 16-bit types, so is their reference."""
    if kind == "int" and dt != torch.bfloat16:
        return _reference(name, kind, torch.bfloat16)
    c = CASES[name]
    dy, x = _operands(name, kind, dt)
    dy64, x64 = dy.double(), x.double()
    return dy, x, _product(c, dy64, x64), _product(c, dy64.abs(), x64.abs()), dy64.sum(0), dy64.abs().sum(0)


class _Banded:
    """A contiguous fp32 [rows, width] between two guard bands, everything preset to the sentinel."""

    def __init__(self, rows, width):
        self.flat = torch.full((2 * GUARD + rows * width,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.flat[GUARD: GUARD + rows * width].view(rows, width)

    def guards_intact(self):
        return bool((self.flat[:GUARD] == SENTINEL).all() and (self.flat[-GUARD:] == SENTINEL).all())


def _on_device(c, dy, x, dt):
    """The operands laid out as the case asks: columns [c0, c0 + n) of a wider zero buffer."""
    if "conv" in c:
        return dy.to(DEV), x.to(DEV)
    wdy, c0dy, wx, c0x = c["lay"]
    bdy = torch.zeros(c["m"], wdy, dtype=dt, device=DEV)
    bx = torch.zeros(c["m"], wx, dtype=dt, device=DEV)
    bdy[:, c0dy: c0dy + c["cout"]] = dy.to(DEV)
    bx[:, c0x: c0x + c["k"]] = x.to(DEV)
    return bdy[:, c0dy: c0dy + c["cout"]], bx[:, c0x: c0x + c["k"]]


def _expected_launches(c, bias):
    """The ops calls of one `add`, in order."""
    reduce = ["colsum"] if c["slices"] > 1 else []
    tail = ["colsum"] if bias != "none" else []
    if c["route"] == "tn":
        return ["gemm_tn_splitk"] + reduce + tail
    if c["route"] == "tn_conv":
        return ["conv3x3_wgrad_splitk"] + reduce + tail
    fused = bias != "none" and not c.get("dy_unaligned")
    return [("transpose16_colsum" if fused else "transpose16"), "transpose16", ("gemm_nt_splitk" if c["slices"] > 1 else "gemm_nt")] \
        + reduce + ([] if fused else tail)


LAUNCHERS = ["gemm_tn_splitk", "conv3x3_wgrad_splitk", "gemm_nt_splitk", "gemm_nt", "transpose16", "transpose16_colsum", "colsum", "im2col3x3_t"]


@pytest.fixture
def launches(monkeypatch):
    log = []
    for fn in LAUNCHERS:
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _real=real, _fn=fn, **kw: (log.append(_fn), _real(*a, **kw))[1])
    return log


@functools.lru_cache(maxsize=None)
def _wg(dt):
    """One WeightGrad per type for the whole module: its buffers are reused and grown from case to case, as in a training step."""
    box = []

    def scratch(n):
        if not box or box[0].numel() < n:
            box[:] = [torch.empty(max(n, 1 << 16), dtype=torch.float32, device=DEV)]
        return box[0]

    return wgrad.WeightGrad(dt, DEV, scratch)


def _check_plan(c, dy16, x16):
    why = wgrad.tn_blocker(c["cout"], c["k"], dy16.stride(), x16.stride(), dy16.data_ptr(), x16.data_ptr(), conv="conv" in c,
                           x_contiguous=x16.is_contiguous())
    assert (why is None) == (c["route"] != "nt"), why
    p = wgrad.plan(c["cout"], c["k"], c["m"], conv="conv" in c, tn_ok=why is None)
    assert (p.route, p.slices) == (c["route"], c["slices"]), p
    return p


def _start(shape, seed, integer):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=gen).float() if integer else torch.randn(shape, generator=gen)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("bias", BIAS)
@pytest.mark.parametrize("name", CASES)
def test_add_is_exact_on_integers_and_accumulates(name, bias, dt, launches):
    """Two consecutive `add` calls onto non-zero gw / gb: every entry equals start + 2 * (float64 product), bit for bit."""
    c = CASES[name]
    dy, x, dw, _, db, _ = _reference(name, "int", dt)
    dy16, x16 = _on_device(c, dy, x, dt)
    _check_plan(c, dy16, x16)
    gw, gb = _Banded(c["cout"], c["kw"]), _Banded(1, c["cout"])
    gw0, gb0 = _start((c["cout"], c["k"]), 1, True), _start((c["cout"],), 2, True)
    gw.t[:, : c["k"]] = gw0.to(DEV)
    gb.t[0] = gb0.to(DEV)
    sums = None
    if bias == "dy_colsum":      # what a producer leaves: fp32 column sums of every 64 rows (exact on integers)
        pad = torch.zeros((c["m"] + 63) // 64 * 64, c["cout"])
        pad[: c["m"]] = dy.float()
        sums = pad.view(-1, 64, c["cout"]).sum(1).to(DEV)
    for _ in range(2):
        del launches[:]
        _wg(dt).add(gw.t, dy16, x16, gb=None if bias == "none" else gb.t[0], dy_colsum=sums, conv=c.get("conv"))
        assert launches == _expected_launches(c, bias)
    assert torch.equal(gw.t[:, : c["k"]].cpu().double(), gw0.double() + 2 * dw)
    assert torch.equal(gb.t[0].cpu().double(), gb0.double() + (0 if bias == "none" else 2) * db)
    assert bool((gw.t[:, c["k"]:] == SENTINEL).all()) and gw.guards_intact() and gb.guards_intact()


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", CASES)
def test_add_random_operands_within_the_fp32_sum_bound(name, dt):
    """|err| <= gamma_n (sum |dy| |x| + |start|), n = m + slices + 1: at most m products and `slices` partials are added, then
    the start value.  The bias gradient (from dy16): n = m + ceil(m / 64) + 1, whichever of the column-sum kernels ran."""
    c = CASES[name]
    dy, x, dw, dw_abs, db, db_abs = _reference(name, "random", dt)
    dy16, x16 = _on_device(c, dy, x, dt)
    p = _check_plan(c, dy16, x16)
    gw, gb = _Banded(c["cout"], c["kw"]), _Banded(1, c["cout"])
    gw0, gb0 = _start((c["cout"], c["k"]), 3, False), _start((c["cout"],), 4, False)
    gw.t[:, : c["k"]] = gw0.to(DEV)
    gb.t[0] = gb0.to(DEV)
    _wg(dt).add(gw.t, dy16, x16, gb=gb.t[0], conv=c.get("conv"))
    for got, start, want, mag, n in ((gw.t[:, : c["k"]], gw0, dw, dw_abs, c["m"] + p.slices + 1),
                                     (gb.t[0], gb0, db, db_abs, c["m"] + (c["m"] + 63) // 64 + 1)):
        gamma = n * U / (1 - n * U)
        err = (got.cpu().double() - (start.double() + want)).abs()
        bound = gamma * (mag + start.double().abs())
        print(f"\n[{name} {dt}] n = {n}: worst err / bound = {float((err / bound).max()):.3e}, worst |err| = {float(err.max()):.3e}")
        assert bool((err <= bound).all())
    assert bool((gw.t[:, c["k"]:] == SENTINEL).all()) and gw.guards_intact() and gb.guards_intact()


def test_unaligned_3x3_raises_on_the_device():
    """A 3x3 input that is a column slice of a wider buffer: no route reads it, and nothing may have been launched or written."""
    b, h, ch, cout = 2, 4, 8, 16
    dy16 = torch.zeros(b * h * h, cout, dtype=torch.bfloat16, device=DEV)
    x16 = torch.zeros(b * h * h, 2 * ch, dtype=torch.bfloat16, device=DEV)[:, :ch]
    gw = _Banded(cout, 9 * ch)
    with pytest.raises(ops._lib.HgrError, match="contiguous"):
        _wg(torch.bfloat16).add(gw.t, dy16, x16, conv=(b, h, ch))
    assert bool((gw.flat == SENTINEL).all())
