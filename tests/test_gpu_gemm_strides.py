"""GPU: strided and offset operands on every kernel and tile plan of the NT GEMM family, hgr_vit_head and the template edges of hgr_mha.

The model calls the GEMM entry points with real strided views (the class-token rows of a [B, L, W] stream, `qkv[:, w:]`, weights
offset by rows), the other kernel tests almost always with lda == K, ldw == K and operands at the start of their buffers.  Here every
operand that has a leading dimension is embedded in a larger buffer whose every other byte is poison: a NaN pattern of the operand's
type, so that a read outside the view reaches the output and a write outside it changes bits that are compared afterwards.  Every case
captures the plan (ops.gemm_plan) of the strided and of the packed call and asserts the kernel and tile plan it was written for."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import _lib, ops, synth
from hgr_net_amd._lib import (EPI_ACCUM, EPI_BIAS, EPI_BIAS_ADD16_RELU, EPI_BIAS_QUICKGELU, EPI_BIAS_RELU, EPI_BIAS_RESIDUAL, EPI_NONE,
                              EPI_QGELU_GRAD16)

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]
K128, K256, DUO, P8 = 1, 2, 3, 5                           # HGR_KERNEL_* of include/hgr.h


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((scale * synth.normal(seed, "t", int(np.prod(shape)))).astype(np.float32).reshape(shape))


def _pair(x, dt):
    """Reference encoder of the residual pair (include/hgr.h), on the bits of x: t = bits(x) + half an ulp of the MFMA type; hi = t with
    the S dropped mantissa bits cleared (S = 13 for f16, 16 for bf16: exactly representable), q = the next 8 bits of t."""
    s_ = 13 if dt == torch.float16 else 16
    t = x.float().contiguous().view(torch.int32) + (1 << (s_ - 1))
    q = (t >> (s_ - 8)) & 255
    if dt == torch.float16:                              # below the f16 normal range hi is not a bit copy: no extra bits there
        q = torch.where((t & 0x7FFFFFFF) < 0x38800000, torch.full_like(q, 128), q)
    hi = (t & ~((1 << s_) - 1)).view(torch.float32).to(dt)
    return hi, q.to(torch.uint8)


# ---- the view helper ---------------------------------------------------------------------------------------------------------
# Poison = one bit pattern per element type, a NaN wherever the type has one.  Inputs: a correct kernel never uses these bytes, and any
# use reaches the output.  Outputs and in-place operands: the same pattern is the sentinel that must still be there after the call.
_INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
_POISON = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FC5A5A5, torch.uint8: 0xA5}


def _same(a, b):
    """Bit equality (NaN patterns included) of two tensors of one element type."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype]))


class _Emb:
    """A logical [rows, cols] tensor inside a poisoned buffer [lead + rows * mul, off + cols + pad]: logical row i is buffer row
    lead + i * mul, logical column j is buffer column off + j; `view` is that strided view (row stride mul * (off + cols + pad))."""

    def __init__(self, x, pad=0, off=0, mul=1, lead=0):
        rows, cols = x.shape
        self.sel = (slice(lead, None, mul), slice(off, off + cols))
        self.buf = torch.full((lead + rows * mul, off + cols + pad), _POISON[x.dtype], dtype=_INT[x.dtype], device=DEV).view(x.dtype)
        self.view = self.buf[self.sel]
        assert self.view.shape == x.shape and self.view.stride() == (mul * (off + cols + pad), 1)
        self.view.copy_(x)

    def intact(self):
        """Every element outside the view still holds the poison: padding columns, gap rows (the other tokens of a class-token
        layout) and leading rows."""
        b = self.buf.view(_INT[self.buf.dtype]).clone()
        b[self.sel] = _POISON[self.buf.dtype]
        return bool((b == _POISON[self.buf.dtype]).all())


def _embed(x, lay):
    return _Emb(x.to(DEV), **lay)


def _vec(v, off=4):
    """A vector `off` entries into a poisoned buffer (s_in[w:], c_in[w:], bias[w:]: 16-byte aligned, NaN on both sides)."""
    buf = torch.full((off + v.numel() + 4,), _POISON[torch.float32], dtype=torch.int32, device=DEV).view(torch.float32)
    buf[off:off + v.numel()] = v.to(DEV)
    return buf[off:off + v.numel()]


PACKED = dict()
PAD = dict(pad=8)                        # ld = cols + 8: the smallest legal pad of a 16-bit operand
OFF = dict(pad=16, off=8)                # 8 elements (16 bytes of a 16-bit operand) into a buffer 24 columns wider
ROWS = dict(pad=8, lead=3)               # offset by whole rows (wf_in[w:]), ld = cols + 8


def TOK(l):                              # the class-token layout: ld = l * cols, the rows between are the other tokens
    return dict(mul=l)


# layouts of (A, W, C, second operand) per set; every set runs on every case, "tok" with l = 50 where the case is small
def _layout_sets(toks):
    sets = [("pad", PAD, PAD, PAD, PAD), ("off", OFF, OFF, OFF, OFF)]
    sets += [("tok%d" % l, TOK(l), ROWS, TOK(l), TOK(l)) for l in toks]
    return sets


@contextlib.contextmanager
def _knobs(tile=None, tail=None, p8=None):
    """Plan knobs for the duration of a case; the previous settings come back whatever happens."""
    lib = _lib.load()
    undo = []
    try:
        if tile is not None:
            prev = ops.gemm_set_tile(tile)
            undo.append(lambda: ops.gemm_set_tile(prev))
        if tail is not None:
            prev_t = ops.gemm_set_tail(*tail)
            undo.append(lambda: ops.gemm_set_tail(bool(prev_t)))
        if p8 is not None:
            prev_p = lib.hgr_gemm_set_p8(p8)
            undo.append(lambda: lib.hgr_gemm_set_p8(prev_p))
        yield
    finally:
        for fn in reversed(undo):
            fn()


_PLAN_KEYS = ("kernel", "variant", "epilogue", "out_f32", "act", "grid_x", "grid_y", "tiles_m", "tiles_n", "total", "nbig", "big_panels", "tiles_m_half",
              "row0", "rows")


def _check_plan(strided, packed, want):
    """The strided and the packed call take the same kernel and tile plan, and it is the one the case was written for: `want` = one
    dict of expected fields per launch."""
    ps, pp = ops.gemm_plan(strided), ops.gemm_plan(packed)
    assert [{k: d[k] for k in _PLAN_KEYS} for d in ps] == [{k: d[k] for k in _PLAN_KEYS} for d in pp], (ps, pp)
    assert len(ps) == len(want), ps
    for d, w in zip(ps, want):
        assert {k: d[k] for k in w} == w, (d, w)


# ---- hgr_gemm_nt, linear epilogues: exact ---------------------------------------------------------------------------------------
_EPIS = {"none32": (EPI_NONE, True), "none16": (EPI_NONE, False), "bias16": (EPI_BIAS, False), "relu16": (EPI_BIAS_RELU, False),
         "res32": (EPI_BIAS_RESIDUAL, True), "accum32": (EPI_ACCUM, True), "add16relu": (EPI_BIAS_ADD16_RELU, False)}
_ALL = tuple(_EPIS)
# name: m, n, k, knobs, expected launches, epilogues, class-token lengths.  Shapes = the smallest that reach the plan (ops.gemm_plan on
# the host): ragged in both dimensions wherever the plan allows it.
_NT_CASES = {
    # 3 x 2 tiles of 128 x 128: one interior tile, ragged last row and column tiles
    "k128": (300, 200, 128, dict(tile=128), [dict(kernel=K128, variant=0, tiles_m=3, tiles_n=2)], _ALL, (2, 50)),
    # the tall 256 x 64 arrangement: N <= 64, M >= 1024, BIAS_RELU, 16-bit out
    "tall": (1100, 40, 128, dict(), [dict(kernel=K128, variant=1, tiles_m=5, tiles_n=1)], ("relu16",), (2, 50)),
    # 3 x 3 tiles of 256 x 256, ragged
    "k256": (600, 520, 128, dict(tile=256), [dict(kernel=K256, variant=0, tiles_m=3, tiles_n=3)], _ALL, (2, 50)),
    # the two-launch split plan: N = 264 wastes too much of a 128-column tile for gemm_nt_duo (duo_fits), 128 row panels x 2 column
    # tiles = one full round of 256^2 tiles, the remaining rows start at row0 = 32768 on the 128^2 kernel (gemm_rows)
    "split": (43664, 264, 128, dict(), [dict(kernel=K256, row0=0, rows=32768, tiles_m=128, tiles_n=2), dict(kernel=K128, row0=32768, rows=10896, tiles_n=3)],
              ("none32", "bias16", "relu16", "res32", "accum32"), (2,)),
    # gemm_nt_duo, full 256 x 128 tiles only (tail plan off), ragged last panel
    "duo_full": (600, 384, 192, dict(tile=2, tail=(False, -1)), [dict(kernel=DUO, variant=0, nbig=9, big_panels=3, tiles_m_half=0)], _ALL, (2, 50)),
    # its tail plan: 544 tiles > 512 slots, 15 full panels forced, the last 412 rows on 4 half panels, the last one ragged
    "duo_tail": (4252, 4096, 128, dict(tile=2, tail=(True, 15)), [dict(kernel=DUO, variant=0, nbig=480, big_panels=15, tiles_m_half=4)], _ALL, (2,)),
    # all half tiles (few tiles, 128 < M: the class-token tail of a ViT's last block), ragged last half panel
    "duo_half": (500, 256, 256, dict(tile=2), [dict(kernel=DUO, variant=0, nbig=0, big_panels=0, tiles_m_half=4)], _ALL, (2, 50)),
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(_NT_CASES))
def test_gemm_nt_linear_epilogues_strided_exact(dt, case):
    """hgr_gemm_nt with A, W, C and the residual / identity operand strided or offset, on every kernel and tile plan it can take, every
    linear epilogue.  Small-integer operands: every sum is exact, so the result equals the fp64 product (and the packed call) bit for
    bit; the padding of every buffer keeps its poison."""
    m, n, k, knobs, want, epis, toks = _NT_CASES[case]
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float()
    a, w, bias, res = ri(-2, 2, (m, k)).to(dt), ri(-1, 1, (n, k)).to(dt), ri(-4, 4, (n,)), ri(-8, 8, (m, n))
    base = a.double() @ w.double().t()                                    # |sum| <= 2 K: exact in fp32, and in 16 bit after one rounding
    bd, rd = bias.double(), res.double()
    ref = {"none32": base.float(), "none16": base.to(dt), "bias16": (base + bd).to(dt), "relu16": torch.relu(base + bd).to(dt),
           "res32": (base + bd + rd).float(), "accum32": (base + rd).float(), "add16relu": torch.relu(base + bd + rd).to(dt)}
    ap, wp = a.contiguous(), w.contiguous()
    sets = [("packed", PACKED, PACKED, PACKED, PACKED)] + _layout_sets(toks)
    if m <= 1100:                                                          # odd leading dimensions of C and of the second operand: the scalar store path
        sets.append(("odd", PAD, PAD, dict(pad=3, off=3), dict(pad=5, off=1)))
    with _knobs(**knobs):
        for name, la, lw, lc, lr in sets:
            A, W = _embed(a, la), _embed(w, lw)
            bv = _vec(bias) if name != "packed" else bias
            for e in epis:
                epi, out32 = _EPIS[e]
                hasb = epi not in (EPI_NONE, EPI_ACCUM)
                c0 = res if e in ("res32", "accum32") else torch.zeros(m, n, dtype=torch.float32 if out32 else dt, device=DEV)
                C = _embed(c0, lc)
                R = _embed(res.to(dt), lr) if e == "add16relu" else None
                second = C.view if e == "res32" else R.view if R is not None else None
                call = lambda: ops.gemm_nt(A.view, W.view, C.view, bias=bv if hasb else None, residual=second, epilogue=epi)
                if name != "packed":
                    cp = torch.empty(m, n, dtype=C.view.dtype, device=DEV)
                    rp = cp if e == "res32" else res.to(dt) if R is not None else None
                    _check_plan(call, lambda: ops.gemm_nt(ap, wp, cp, bias=bias if hasb else None, residual=rp, epilogue=epi), want)
                call()
                assert torch.equal(C.view, ref[e]), (case, name, e)        # the fp64 product; the packed call gives it too (first set)
                assert C.intact(), (case, name, e)
                assert R is None or R.intact(), (case, name, e)
            assert A.intact() and W.intact(), (case, name)


# ---- non-linear forms: the bits of the packed call ------------------------------------------------------------------------------
def _randn(g, shape, scale=1.0):
    return scale * torch.randn(shape, generator=g, device=DEV)


# the plans of gemm_nt_duo an entry point of the LayerNorm family / the training fusions can take: m, n, k, knobs, expected fields
_DUO_CASES = {
    "half": (500, 256, 256, dict(), dict(kernel=DUO, nbig=0, big_panels=0, tiles_m_half=4), (2, 50)),
    "full": (600, 384, 256, dict(tail=(False, -1)), dict(kernel=DUO, nbig=9, big_panels=3, tiles_m_half=0), (2, 50)),
    "tail": (4252, 4096, 128, dict(tail=(True, 15)), dict(kernel=DUO, nbig=480, big_panels=15, tiles_m_half=4), (2,)),
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", ["k128", "k256", "split", "duo_full", "duo_tail", "duo_half"])
def test_gemm_nt_nonlinear_epilogues_strided_bits(dt, case):
    """hgr_gemm_nt with BIAS_QUICKGELU and QGELU_GRAD16 (its 16-bit `pre` operand strided too) on random operands: stride changes no
    arithmetic, so the strided call must give the bits of the packed call on the same kernel and plan."""
    m, n, k, knobs, want, _, toks = _NT_CASES[case]
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 1)
    a, w = _randn(g, (m, k)).to(dt), _randn(g, (n, k), 0.1).to(dt)
    bias, pre = _randn(g, (n,)), _randn(g, (m, n), 2.0).to(dt)
    with _knobs(**knobs):
        for e, epi in (("gelu16", EPI_BIAS_QUICKGELU), ("qgrad16", EPI_QGELU_GRAD16)):
            if e == "qgrad16" and case == "split":                       # the 16-bit second operand keeps the 128^2 kernel
                w_e = [dict(kernel=K128, variant=0, row0=0, rows=m)]
            else:
                w_e = want
            kw = lambda b_, r_: dict(bias=b_ if e == "gelu16" else None, residual=r_ if e == "qgrad16" else None, epilogue=epi)
            cp = torch.empty(m, n, dtype=dt, device=DEV)
            ops.gemm_nt(a, w, cp, **kw(bias, pre))
            for name, la, lw, lc, lr in _layout_sets(toks):
                A, W, C, R = _embed(a, la), _embed(w, lw), _embed(torch.zeros(m, n, dtype=dt, device=DEV), lc), _embed(pre, lr)
                bv = _vec(bias)
                call = lambda: ops.gemm_nt(A.view, W.view, C.view, **kw(bv, R.view))
                c2 = torch.empty_like(cp)
                _check_plan(call, lambda: ops.gemm_nt(a, w, c2, **kw(bias, pre)), w_e)
                call()
                assert _same(C.view, cp), (case, name, e)
                assert C.intact() and A.intact() and W.intact() and R.intact(), (case, name, e)
            assert bool(torch.isfinite(cp.float()).all())


_PRODUCER_CASES = dict(_DUO_CASES)
# the persistent walk: 690 tiles (510 full + 180 half) on 512 workgroups
_PRODUCER_CASES["persist"] = (25600, 768, 128, dict(), dict(kernel=DUO, grid_x=512, total=690, nbig=510, big_panels=85, tiles_m_half=30), ())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(_PRODUCER_CASES))
def test_gemm_nt_res_stats_strided_bits(dt, case):
    """hgr_gemm_nt_res_stats / _guard: A and the pair (xh, xl) strided, the class-token layout among them, compact statistics.  Pair
    and statistics carry the bits of the packed call; the gap rows of the pair (the other tokens) and its padding keep their bits;
    the guard flag stays 0."""
    m, n, k, knobs, want, toks = _PRODUCER_CASES[case]
    want = dict(want, variant=want.get("variant", 1))
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 2)
    a, w = _randn(g, (m, k)).to(dt), _randn(g, (n, k), 0.1).to(dt)
    bias, x0 = _randn(g, (n,)), _randn(g, (m, n), 2.0)
    xh0, xl0 = _pair(x0, dt)
    with _knobs(**knobs):
        xh, xl = xh0.clone(), xl0.clone()
        st = torch.full((m, n // 64, 2), float("nan"), device=DEV)
        ops.gemm_nt_res_stats(a, w, xh, xl, bias, st)
        assert bool(torch.isfinite(st).all())
        for name, la, lw, lc, _ in _layout_sets(toks):
            if lc is OFF:                                                 # xl is one byte per element: 16 elements = its 16-byte alignment
                lc = dict(pad=16, off=16)
            A, W, XH, XL = _embed(a, la), _embed(w, lw), _embed(xh0, lc), _embed(xl0, lc)
            bv = _vec(bias)
            stats = torch.full((m, n // 64, 2), float("nan"), device=DEV)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV) if name != "pad" else None      # with and without the guard
            call = lambda: ops.gemm_nt_res_stats(A.view, W.view, XH.view, XL.view, bv, stats, flag=flag)
            h2, l2, s2 = xh0.clone(), xl0.clone(), torch.empty_like(stats)
            _check_plan(call, lambda: ops.gemm_nt_res_stats(a, w, h2, l2, bias, s2, flag=flag), [want])
            call()
            assert _same(XH.view, xh) and _same(XL.view, xl) and _same(stats, st), (case, name)
            assert XH.intact() and XL.intact() and A.intact() and W.intact(), (case, name)
            assert flag is None or int(flag) == 0


_CONSUMER_CASES = dict(_DUO_CASES)
_CONSUMER_CASES["p8"] = (4096, 4096, 256, dict(p8=1), dict(kernel=P8, tiles_m=16, tiles_n=16, grid_x=256), (2,))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("case", list(_CONSUMER_CASES))
def test_gemm_nt_ln_strided_bits(dt, gelu, case):
    """hgr_gemm_nt_ln: X16 strided (the class-token layout among them) with compact statistics, W offset by rows, ln_s / ln_c offset
    by entries, C as qkv[:, w:] (a column offset into a wider buffer) and as qkv.view(b, l, 3 w)[:, 0, :w] (row stride 3 w l); both
    `act` values.  The bits of the packed call."""
    m, n, k, knobs, want, toks = _CONSUMER_CASES[case]
    want = dict(want, variant=want.get("variant", 2 if want["kernel"] == DUO else 0), act=1 if gelu and want["kernel"] != DUO else 0)
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 3)
    x = _randn(g, (m, k), 1.5) + 0.3 * _randn(g, (m, 1)) + 0.2
    x16, xlo, stats = torch.empty(m, k, dtype=dt, device=DEV), torch.empty(m, k, dtype=ops.PAIR_LO, device=DEV), torch.empty(m, k // 64, 2, device=DEV)
    ops.row_stats16(x, x16, xlo, stats)
    w = _randn(g, (n, k), 0.05).to(dt)
    s, c = w.float().sum(1), _randn(g, (n,))
    with _knobs(**knobs):
        cp = torch.empty(m, n, dtype=dt, device=DEV)
        ops.gemm_nt_ln(x16, w, cp, s, c, stats, 1e-5, quickgelu=gelu)
        assert bool(torch.isfinite(cp.float()).all())
        # C: the smallest pad; qkv[:, w:] = n columns at offset n / 2 of a row 1.5 n wide; the class-token rows of a [b, l, 3 n] tensor
        c_layouts = [("pad", PAD, PAD), ("cols", OFF, dict(off=n // 2))] + [("tok%d" % l, TOK(l), dict(pad=2 * n, mul=l)) for l in toks]
        for name, lx, lc in c_layouts:
            X, W, C = _embed(x16, lx), _embed(w, ROWS if name != "pad" else PAD), _embed(torch.zeros(m, n, dtype=dt, device=DEV), lc)
            sv, cv = _vec(s, 8), _vec(c, 4)
            call = lambda: ops.gemm_nt_ln(X.view, W.view, C.view, sv, cv, stats, 1e-5, quickgelu=gelu)
            c2 = torch.empty_like(cp)
            _check_plan(call, lambda: ops.gemm_nt_ln(x16, w, c2, s, c, stats, 1e-5, quickgelu=gelu), [want])
            call()
            assert _same(C.view, cp), (case, name)
            assert C.intact() and X.intact() and W.intact(), (case, name)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(_DUO_CASES))
def test_gemm_nt_bias_gelu_dual_strided_bits(dt, case):
    """hgr_gemm_nt_bias_gelu_dual: A and W strided, ldpre != ldpost.  The bits of the packed call in both outputs."""
    m, n, k, knobs, want, toks = _DUO_CASES[case]
    want = dict(want, variant=4)
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 4)
    a, w, bias = _randn(g, (m, k)).to(dt), _randn(g, (n, k), 0.1).to(dt), _randn(g, (n,))
    with _knobs(**knobs):
        pre, post = torch.empty(m, n, dtype=dt, device=DEV), torch.empty(m, n, dtype=dt, device=DEV)
        ops.gemm_nt_bias_gelu_dual(a, w, pre, post, bias)
        assert bool(torch.isfinite(pre.float()).all())
        for name, la, lw, lc, lr in _layout_sets(toks):
            lr = OFF if lc is PAD else PAD if lc is OFF else dict(pad=8, mul=lc["mul"])              # never the layout of `pre`
            A, W = _embed(a, la), _embed(w, lw)
            PRE, POST = _embed(torch.zeros(m, n, dtype=dt, device=DEV), lc), _embed(torch.zeros(m, n, dtype=dt, device=DEV), lr)
            assert PRE.view.stride(0) != POST.view.stride(0)
            bv = _vec(bias)
            call = lambda: ops.gemm_nt_bias_gelu_dual(A.view, W.view, PRE.view, POST.view, bv)
            p2, q2 = torch.empty_like(pre), torch.empty_like(post)
            _check_plan(call, lambda: ops.gemm_nt_bias_gelu_dual(a, w, p2, q2, bias), [want])
            call()
            assert _same(PRE.view, pre) and _same(POST.view, post), (case, name)
            assert PRE.intact() and POST.intact() and A.intact() and W.intact(), (case, name)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", list(_DUO_CASES))
def test_gemm_nt_qgelu_grad_colsum_strided_bits(dt, case):
    """hgr_gemm_nt_qgelu_grad_colsum: A, W, C and `pre` strided, compact column sums.  The bits of the packed call."""
    m, n, k, knobs, want, toks = _DUO_CASES[case]
    want = dict(want, variant=0, epilogue=EPI_QGELU_GRAD16)
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 5)
    a, w, pre = _randn(g, (m, k)).to(dt), _randn(g, (n, k), 0.1).to(dt), _randn(g, (m, n), 2.0).to(dt)
    units = (m + 63) // 64
    with _knobs(**knobs):
        cp, part = torch.empty(m, n, dtype=dt, device=DEV), torch.full((units, n), float("nan"), device=DEV)
        ops.gemm_nt_qgelu_grad_colsum(a, w, cp, pre, part)
        assert bool(torch.isfinite(part).all())
        for name, la, lw, lc, lr in _layout_sets(toks):
            A, W, C, R = _embed(a, la), _embed(w, lw), _embed(torch.zeros(m, n, dtype=dt, device=DEV), lc), _embed(pre, OFF if lr is PAD else lr)
            got = torch.full((units, n), float("nan"), device=DEV)
            call = lambda: ops.gemm_nt_qgelu_grad_colsum(A.view, W.view, C.view, R.view, got)
            c2, p2 = torch.empty_like(cp), torch.empty_like(part)
            _check_plan(call, lambda: ops.gemm_nt_qgelu_grad_colsum(a, w, c2, pre, p2), [want])
            call()
            assert _same(C.view, cp) and _same(got, part), (case, name)
            assert C.intact() and A.intact() and W.intact() and R.intact(), (case, name)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("b,l,heads,causal", [(7, 50, 4, False), (33, 17, 2, True)])
def test_gemm_nt_ln_mha_strided_bits(dt, b, l, heads, causal):
    """hgr_gemm_nt_ln_mha with ldx > K and ldatt > heads * 64 (no caller passes either today, the ABI promises both): the bits of the
    packed call and of hgr_gemm_nt_ln + hgr_mha; the padding of `att` keeps its bits."""
    wd, m = heads * 64, b * l
    g = torch.Generator(device=DEV).manual_seed(m + wd)
    x = _randn(g, (m, wd), 1.2) + 0.2 * _randn(g, (m, 1))
    x16, xlo, stats = torch.empty(m, wd, dtype=dt, device=DEV), torch.empty(m, wd, dtype=ops.PAIR_LO, device=DEV), torch.empty(m, wd // 64, 2, device=DEV)
    ops.row_stats16(x, x16, xlo, stats)
    w = _randn(g, (3 * wd, wd), wd ** -0.5).to(dt)
    s, c = w.float().sum(1), 0.1 * _randn(g, (3 * wd,))
    packed = torch.empty(m, wd, dtype=dt, device=DEV)
    ops.gemm_nt_ln_mha(x16, w, packed, s, c, stats, b, l, heads, causal, 1e-5)
    qkv, two = torch.empty(m, 3 * wd, dtype=dt, device=DEV), torch.empty(m, wd, dtype=dt, device=DEV)
    ops.gemm_nt_ln(x16, w, qkv, s, c, stats, 1e-5)
    ops.mha(qkv, two, b, l, heads, causal)
    assert _same(packed, two) and bool(torch.isfinite(packed.float()).all())
    # att: ldatt % 4 == 0 and an 8-byte aligned start are all the entry point asks for
    for name, lx, lw, latt in (("pad", PAD, PAD, dict(pad=4)), ("off", OFF, OFF, dict(pad=8, off=4)), ("tok2", TOK(2), ROWS, TOK(2))):
        X, W, ATT = _embed(x16, lx), _embed(w, lw), _embed(torch.zeros(m, wd, dtype=dt, device=DEV), latt)
        ops.gemm_nt_ln_mha(X.view, W.view, ATT.view, _vec(s, 8), _vec(c, 4), stats, b, l, heads, causal, 1e-5)
        assert _same(ATT.view, packed), name
        assert ATT.intact() and X.intact() and W.intact(), name


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("m,n,k,kc,kernel", [(100, 200, 384, 128, K128), (300, 260, 384, 128, K256)])
def test_gemm_nt_splitk_strided_exact(dt, m, n, k, kc, kernel):
    """hgr_gemm_nt_splitk with A and W strided and ldc > N, on both of its kernels: every slice equals the fp64 product of its K range
    (small integers: exact) and the packed call; the padding columns of the partials keep their bits."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    a = torch.randint(-2, 3, (m, k), generator=g, device=DEV).to(dt)
    w = torch.randint(-1, 2, (n, k), generator=g, device=DEV).to(dt)
    s = (k + kc - 1) // kc
    ref = torch.stack([a[:, i * kc:(i + 1) * kc].double() @ w[:, i * kc:(i + 1) * kc].double().t() for i in range(s)]).float()
    packed = torch.empty(s, m, n, device=DEV)
    ops.gemm_nt_splitk(a, w, packed, kc)
    assert _same(packed, ref)
    want = [dict(kernel=kernel, variant=0, grid_y=s, tiles_m=(m + 127) // 128 if kernel == K128 else (m + 255) // 256)]
    for name, la, lw, lc, _ in _layout_sets((2,)):
        A, W = _embed(a, la), _embed(w, lw)
        ldc = n + 4 if name == "pad" else n + 12                        # ldc % 4 == 0 is all the entry point asks for
        P = _Emb(torch.zeros(s * m, n, device=DEV), pad=ldc - n)        # slice i at partial + i * m * ldc
        dtc = ops.DT_OF[dt]
        call = lambda: _lib.call("hgr_gemm_nt_splitk", A.view.data_ptr(), A.view.stride(0), W.view.data_ptr(), W.view.stride(0), P.buf.data_ptr(), ldc,
                                 m, n, k, kc, dtc, ops._stream())
        p2 = torch.empty_like(packed)
        _check_plan(call, lambda: ops.gemm_nt_splitk(a, w, p2, kc), want)
        call()
        assert _same(P.view.reshape(s, m, n), ref), name
        assert P.intact() and A.intact() and W.intact(), name


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("m,na,nb,kc,tile", [(200, 192, 128, 64, 128), (333, 256, 256, 64, 256)])
def test_gemm_tn_splitk_strided_q_exact(dt, m, na, nb, kc, tile):
    """hgr_gemm_tn_splitk with Q strided (P as well), on both tile edges: every slice equals the fp64 product (small integers: exact)."""
    assert _lib.load().hgr_gemm_tn_tile(na, nb) == tile
    g = torch.Generator(device=DEV).manual_seed(m + na + nb)
    p = torch.randint(-2, 3, (m, na), generator=g, device=DEV).to(dt)
    q = torch.randint(-2, 3, (m, nb), generator=g, device=DEV).to(dt)
    s = (m + kc - 1) // kc
    ref = torch.stack([p[i * kc:(i + 1) * kc].double().t() @ q[i * kc:(i + 1) * kc].double() for i in range(s)]).float()
    for name, lp, lq in (("pad", PAD, PAD), ("off", PAD, OFF), ("tok2", OFF, TOK(2)), ("tok50", TOK(2), TOK(50))):
        P, Q = _embed(p, lp), _embed(q, lq)
        part = torch.full((s, na, nb), float("nan"), device=DEV)
        ops.gemm_tn_splitk(P.view, Q.view, part, kc)
        assert _same(part, ref), name
        assert P.intact() and Q.intact(), name


# ---- hgr_vit_head, direct ---------------------------------------------------------------------------------------------------------
def _head_case(dt, w, b, d, mul, pad, low_byte, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if low_byte:
        # every high part of a row holds the same value: the LayerNorm signal is in the low byte alone.  A kernel that drops or
        # mis-indexes xl is then off by O(1), not by one rounding step.
        xh = torch.full((b, w), 64.0, dtype=dt, device=DEV)
        xl = torch.randint(0, 256, (b, w), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    else:
        x = _randn(g, (b, w), 1.5) * (0.5 + torch.rand((b, 1), generator=g, device=DEV)) + 0.3 * _randn(g, (b, 1))
        xh, xl = _pair(x, dt)
    gamma, beta = 1.0 + 0.2 * _randn(g, (w,)), 0.1 * _randn(g, (w,))
    proj_t = _randn(g, (d, w), w ** -0.5).to(dt)
    XH, XL = _Emb(xh, pad=pad, mul=mul), _Emb(xl, pad=pad, mul=mul)       # the rows outside the selection: NaN (xh), poison (xl)
    out = torch.full((b, d), float("nan"), device=DEV)
    ops.vit_head(XH.buf[:, :w], XL.buf[:, :w], mul, gamma, beta, 1e-5, proj_t, out)      # ldx = w + pad, row b of the result reads buffer row b * mul
    assert XH.intact() and XL.intact()
    # fp64 restatement: decode the pair (ops.pair_value: the kernels' own decoder, pinned elsewhere), LayerNorm in fp64, round to
    # the operand type, multiply by proj_t in fp64
    v = ops.pair_value(xh, xl).double()
    mu = v.mean(1, keepdim=True)
    h = (v - mu) / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    ref = h.to(dt).double() @ proj_t.double().t()
    # Tolerance, derived: rounding h to a t-bit significand (t = 8 bf16, 11 f16) perturbs an output by at most 2^-t sum_k |h_k| |p_k|;
    # the fp32 accumulation of W products adds at most W 2^-24 of the same sum.  (The fp32 statistics of the kernel move h by parts
    # in 2^-20, which decides a rounding only next to a tie.)
    t = 8 if dt == torch.bfloat16 else 11
    bound = (2.0 ** -t + w * 2.0 ** -24) * (h.abs() @ proj_t.double().abs().t())
    err = (out.double() - ref).abs()
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all()), (float((err / bound).max()), float(err.max()))
    # cross-check: the composite of kernels that are tested on their own
    x32 = torch.empty(b, w, device=DEV)
    ops.pair_rows_f32(xh, xl, x32)
    h16 = torch.empty(b, w, dtype=dt, device=DEV)
    ops.layernorm(x32, gamma, beta, h16)
    kp = (w + 63) // 64 * 64                                               # hgr_gemm_nt wants K % 64 == 0: zero columns add nothing
    hp, pp = torch.zeros(b, kp, dtype=dt, device=DEV), torch.zeros(d, kp, dtype=dt, device=DEV)
    hp[:, :w], pp[:, :w] = h16, proj_t
    comp = torch.empty(b, d, device=DEV)
    ops.gemm_nt(hp, pp, comp)
    err2 = (out.double() - comp.double()).abs()
    assert bool((err2 <= bound).all()), (float((err2 / bound).max()), float(err2.max()))


# W: 64 and 96 (two and three k-steps through the 8-way unrolled loop), the tower widths, 1920 = the LDS limit; B: one row, one full
# block of 16 rows, 16 + 1, two blocks + 5; D: a single group of 4 columns, a column block cut short (124), a whole one (128), a
# second block of one group (132) and of four blocks (512); row_mul 1 and 50, each with ldx = W and ldx = W + 8
_HEAD_SHAPES = [(64, 1, 4, 1, 0), (64, 16, 132, 50, 8), (96, 17, 124, 50, 0), (96, 37, 512, 1, 8), (768, 16, 512, 50, 0), (768, 37, 132, 1, 8),
                (1024, 17, 128, 50, 8), (1024, 1, 124, 1, 0), (1920, 37, 4, 50, 0), (1920, 16, 128, 1, 8), (1920, 17, 512, 50, 8)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("w,b,d,mul,pad", _HEAD_SHAPES)
def test_vit_head_vs_fp64(dt, w, b, d, mul, pad):
    """hgr_vit_head (ln_post on the class tokens of the residual pair + visual.proj, clip/model.py:231-234) against its fp64
    restatement and against pair_rows_f32 -> layernorm -> gemm_nt, with the derived per-element bound."""
    _head_case(dt, w, b, d, mul, pad, False, w + b + d)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("w,b,d,mul,pad", [(768, 17, 132, 50, 8), (96, 37, 124, 1, 0)])
def test_vit_head_signal_in_the_low_byte(dt, w, b, d, mul, pad):
    _head_case(dt, w, b, d, mul, pad, True, w + b + d + 1)


# ---- hgr_mha: the edges of its template dispatch -------------------------------------------------------------------------------
def _mha_ref(qkv, b, L, heads, causal):
    w = heads * 64
    q, k, v = qkv.float().cpu().view(b, L, 3 * w).split(w, dim=-1)
    sh = lambda t: t.reshape(b, L, heads, 64).transpose(1, 2)
    s = (sh(q) @ sh(k).transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf")).triu_(1)
    return (torch.softmax(s, -1) @ sh(v)).transpose(1, 2).reshape(b * L, w)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [32, 64, 65, 96, 97, 128, 160, 161, 288])
def test_mha_dispatch_edges_vs_oracle(dt, L, causal):
    """hgr_mha switches templates at 32, 64, 96 and 160 keys and admits L <= 288: both sides of every switch and the largest L, with
    the fp32 reference and the tolerances of test_gpu_kernels.test_mha_vs_oracle; on 65 and 288 also the leading-rows form."""
    b, heads = 3, 2
    w = heads * 64
    qkv = _rand((b * L, 3 * w), 20 + L, 1.0).to(dt).to(DEV)
    out = torch.full((b * L, w), float("nan"), dtype=dt, device=DEV)
    ops.mha(qkv, out, b, L, heads, causal)
    tol = 2e-2 if dt == torch.bfloat16 else 3e-3
    assert float((out.float().cpu() - _mha_ref(qkv, b, L, heads, causal)).abs().max()) < tol
    if L in (65, 288):
        for q_rows in (1, 17):
            part = torch.full((b * L, w), 7.0, dtype=dt, device=DEV)
            ops.mha(qkv, part, b, L, heads, causal, q_rows=q_rows)
            f, p_ = out.view(b, L, w), part.view(b, L, w)
            assert torch.equal(p_[:, :q_rows], f[:, :q_rows]), q_rows
            assert bool((p_[:, q_rows:] == 7.0).all()), q_rows


@pytest.mark.parametrize("dt", DTS)
def test_mha_rejects_289_keys_and_writes_nothing(dt):
    b, heads, L = 2, 2, 289
    qkv = _rand((b * L, 3 * heads * 64), 5, 1.0).to(dt).to(DEV)
    out = torch.full((b * L, heads * 64), 7.0, dtype=dt, device=DEV)
    for q_rows in (0, 1):
        with pytest.raises(_lib.HgrError, match="L=289"):
            ops.mha(qkv, out, b, L, heads, False, q_rows=q_rows)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
