"""GPU: the small kernels around the GEMM family at every width branch and edge - the register-resident row normalisers and their
backward, hgr_matmul_f32, the loss head, the gathers / scatters and the training-time input assembly.

Every case is compared with a plain float64 restatement of the operation on the CPU, made from the same input bits.  Every operand lives
inside a larger buffer whose other elements hold a NaN pattern of its type (`_POISON`): an input read outside its view reaches the
output, a write outside an output's view changes bits that are compared afterwards - a stray edge lane shows without anything faulting.
Kernels that do not check an index (ce_rows labels, rows_gather / rows_axpy indices) are only ever given indices in range."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops, synth
from hgr_net_amd._lib import HgrError

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]
F32 = torch.float32


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((scale * synth.normal(seed, "rk", int(np.prod(shape)))).astype(np.float32).reshape(shape))


def _ints(seed, n, lo, hi):
    return torch.from_numpy(synth.randint(seed, "rk", n, lo, hi).astype(np.int32))


# ---- the view helper ---------------------------------------------------------------------------------------------------------
# Poison = one bit pattern per element type, a NaN wherever the type has one.  Inputs: a correct kernel never uses these bytes, and any
# use reaches the output.  Outputs and in-place operands: the same pattern is the sentinel that must still be there after the call.
_INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
_POISON = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA, torch.float32: 0x7FC5A5A5, torch.uint8: 0xA5}
# Pure inputs are poisoned with a SECOND NaN pattern: arithmetic hands a NaN operand's payload on, so a stray fp32 store of a value
# computed from poisoned inputs would otherwise put the very sentinel bits back into an output's guard band and go unseen.
_POISON_IN = {torch.float16: 0x7EA5, torch.bfloat16: 0x7FC3, torch.float32: 0x7FD1C2B3, torch.uint8: 0x5A}
_G = 64                                  # guard elements in front of and behind every operand (a multiple of 16 bytes for every type)


def _same(a, b):
    """Bit equality (NaN patterns included) of two tensors of one element type."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype]))


class _Band:
    """A logical [rows, cols] (or 1-D) tensor inside a flat poisoned buffer: `lead` guard elements, then rows of `ld` elements of which
    columns coff .. coff + cols - 1 are the operand, then _G guard elements.  ld == cols: `t` is contiguous.  x = None: the operand itself
    starts out as poison too (an output every element of which must be written).  lead = _G + 1: 4-byte but not 16-byte aligned."""

    def __init__(self, x=None, shape=None, dtype=None, ld=None, coff=0, lead=_G, poison=_POISON):
        shape = tuple(x.shape if x is not None else shape)
        dtype = x.dtype if x is not None else dtype
        self.poison = poison[dtype]
        rows, cols = (shape if len(shape) == 2 else (1, shape[0]))
        ld = cols if ld is None else ld
        assert coff + cols <= ld
        self.dtype, self.lead, self.span, self.coff, self.cols = dtype, lead, rows * ld, coff, cols
        self.buf = torch.full((lead + rows * ld + _G,), self.poison, dtype=_INT[dtype], device=DEV).view(dtype)
        self.mat = self.buf[lead:lead + rows * ld].view(rows, ld)
        self.t = self.mat[:, coff:coff + cols]
        if len(shape) == 1:
            self.t = self.t[0]
        if x is not None:
            self.t.copy_(x)

    def intact(self):
        """Every element outside the operand still holds the poison: both guard bands and the padding columns."""
        b = self.buf.view(_INT[self.dtype]).clone()
        b[self.lead:self.lead + self.span].view(self.mat.shape)[:, self.coff:self.coff + self.cols] = self.poison
        return bool((b == self.poison).all())

    def cpu(self):
        return self.t.detach().cpu().contiguous()


def _in(x, **kw):
    """An input operand in guard bands (of the input pattern); the device view."""
    return _Band(x, poison=_POISON_IN, **kw).t


def _half_ulp(ref64, dt):
    """Half a unit in the last place of the 16-bit type at |ref64| (the subnormal step below the normal range): the error of one
    round-to-nearest of an exact value.  Relative to |ref64| that is between 2^-9 and 2^-8 for bf16 and between 2^-12 and 2^-11 for f16,
    so a flat 2^-9 / 2^-12 relative bound would refuse correctly rounded values."""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref64.abs().double())                 # |ref| = m * 2^e, m in [0.5, 1)
    return torch.pow(2.0, (e.double() - 1).clamp_min(emin) - mant - 1)


def _within(got, ref64, rtol, atol, extra=None, what=""):
    """|got - ref64| <= atol + rtol |ref64| (+ extra), element-wise in float64; the worst ratio is reported."""
    got = got.double().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), (what, "non-finite output")
    bound = atol + rtol * ref64.abs() + (0.0 if extra is None else extra)
    bound = bound + torch.zeros_like(ref64)
    err = (got - ref64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool((err > bound).any()), (what, "error / bound = %.3g, max |err| = %.3g" % (worst, float(err.max())))


# ==== 1. register-resident row kernels ===========================================================================================
# NV = float4 per lane: 1 (W <= 256), 2 (<= 512), 4 (<= 1024), 8 (<= 2048), 16 (<= 4096).  256 / 512 / 1024 / 2048 / 4096 fill the last
# 64-lane vector of their instantiation, 4 / 64 / 68 / 260 / 640 / 1028 / 2052 leave lanes of it idle.
WIDTHS = [4, 64, 68, 256, 260, 512, 640, 1024, 1028, 2048, 2052, 4096]
ROWS = [1, 5, 37]
LN_TOL = dict(rtol=1e-5, atol=1e-5)          # test_gpu_kernels.py::test_layernorm_and_l2norm
L2_TOL = dict(rtol=1e-6, atol=1e-7)


def _ln64(x, g, b, eps=1e-5):
    x = x.double()
    m = x.mean(dim=-1, keepdim=True)
    v = ((x - m) ** 2).mean(dim=-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * g.double() + b.double()


def _ln_outputs(x_dev, g_dev, b_dev, n_out, w, ref64, what, **kw):
    for dt in [F32] + DTS:
        out = _Band(shape=(n_out, w), dtype=dt)
        ops.layernorm(x_dev, g_dev, b_dev, out.t, **kw)
        assert out.intact(), (what, dt, "wrote outside its rows")
        _within(out.cpu(), ref64, extra=None if dt == F32 else _half_ulp(ref64, dt), what=(what, dt), **LN_TOL)


@pytest.mark.parametrize("w", WIDTHS)
def test_layernorm_every_width(w):
    g, b = 1 + 0.1 * _rand((w,), 2), 0.1 * _rand((w,), 3)
    g_dev, b_dev = _in(g), _in(b)
    for rows in ROWS:
        x = _rand((rows, w), 100 + rows, 3.0) + 0.5
        _ln_outputs(_in(x), g_dev, b_dev, rows, w, _ln64(x, g, b), ("plain", rows, w))
        # rows / row_mul / row_idx: output row i = LN(x[i * L + idx[i]])  (ln_post on token 0, ln_final on the EOT row)
        L = 3
        xs = _rand((rows * L, w), 200 + rows, 2.0) - 0.25
        xs_dev = _in(xs)
        for name, idx in (("random", _ints(4 + rows, rows, 0, L)), ("first", torch.zeros(rows, dtype=torch.int32)),
                          ("last", torch.full((rows,), L - 1, dtype=torch.int32))):
            pick = xs.view(rows, L, w)[torch.arange(rows), idx.long()]
            _ln_outputs(xs_dev, g_dev, b_dev, rows, w, _ln64(pick, g, b), ("row_idx " + name, rows, w), rows=rows, row_mul=L, row_idx=idx.to(DEV))


@pytest.mark.parametrize("w", WIDTHS)
def test_l2norm_rows_every_width(w):
    for rows in ROWS:
        x = _rand((rows, w), 300 + rows, 3.0) + 0.5
        x_dev = _in(x)
        ref = x.double() / x.double().norm(dim=-1, keepdim=True)
        for dt in DTS:
            for want16, want32 in ((True, False), (False, True), (True, True)):
                y16, y32 = _Band(shape=(rows, w), dtype=dt), _Band(shape=(rows, w), dtype=F32)
                ops.l2norm_rows(x_dev, y16=y16.t if want16 else None, y32=y32.t if want32 else None)
                assert y16.intact() and y32.intact(), (rows, w, dt)
                poison16, poison32 = _Band(shape=(rows, w), dtype=dt), _Band(shape=(rows, w), dtype=F32)
                if want16:
                    _within(y16.cpu(), ref, extra=_half_ulp(ref, dt), what=("y16", rows, w, dt), **L2_TOL)
                else:
                    assert _same(y16.buf, poison16.buf)                  # the output that was not asked for is untouched
                if want32:
                    _within(y32.cpu(), ref, what=("y32", rows, w), **L2_TOL)
                else:
                    assert _same(y32.buf, poison32.buf)


@pytest.mark.parametrize("w", WIDTHS)
def test_vit_embed_ln_every_width(w):
    ga, be = 1 + 0.1 * _rand((w,), 14), 0.1 * _rand((w,), 15)
    cls = _rand((w,), 12)
    for b, g in ((1, 1), (1, 4), (1, 36), (3, 4)):                       # 2, 5, 37 and 15 rows: a class row and patch rows per image
        pe, pos = _rand((b * g, w), 400 + g, 1.5), _rand((g + 1, w), 13)
        x = _Band(shape=(b * (g + 1), w), dtype=F32)
        ops.vit_embed_ln(_in(pe), _in(cls), _in(pos), _in(ga), _in(be), x.t, b, g)
        assert x.intact(), (b, g, w)
        t = torch.cat([cls.expand(b, 1, w), pe.view(b, g, w)], 1) + pos   # one fp32 add, as the kernel's
        _within(x.cpu(), _ln64(t, ga, be).view(-1, w), what=(b, g, w), **LN_TOL)


def test_row_kernels_reject_bad_widths_and_misaligned_operands():
    """W % 4 != 0, W > 4096 and operands that are not 16-byte aligned are refused before anything is launched."""
    for w in (6, 4100):
        x, v = torch.zeros(2 * w + 4, device=DEV), torch.ones(w + 4, device=DEV)
        xv = x[:2 * w].view(2, w)
        out = torch.zeros(2, w, device=DEV)
        with pytest.raises(HgrError):
            ops.layernorm(xv, v[:w], v[:w], out)
        with pytest.raises(HgrError):
            ops.l2norm_rows(xv, y32=out)
        with pytest.raises(HgrError):
            ops.vit_embed_ln(xv[:1], v[:w], xv, v[:w], v[:w], out, 1, 1)
        assert not bool(out.any())
    w = 64
    x, v = torch.zeros(2 * w + 4, device=DEV), torch.ones(w + 4, device=DEV)
    ok, off = x[:2 * w].view(2, w), x[1:2 * w + 1].view(2, w)              # one float into the buffer: 4-byte aligned only
    out = torch.zeros(2, w, device=DEV)
    for args in ((off, v[:w], v[:w], out), (ok, v[1:w + 1], v[:w], out), (ok, v[:w], v[1:w + 1], out), (ok, v[:w], v[:w], off)):
        with pytest.raises(HgrError):
            ops.layernorm(*args)
    with pytest.raises(HgrError):
        ops.l2norm_rows(off, y32=out)
    with pytest.raises(HgrError):
        ops.l2norm_rows(ok, y32=off)
    with pytest.raises(HgrError):
        ops.vit_embed_ln(off[:1], v[:w], ok, v[:w], v[:w], out, 1, 1)
    assert not bool(out.any()) and not bool(x.any())


def _lib_layernorm_bwd(dy, x, g, dx, dg, db, sc, rows, w):
    """hgr_layernorm_bwd without the wrapper's scratch-size query (which has no meaning for a width the ABI refuses)."""
    from hgr_net_amd import _lib
    p = lambda t: t.data_ptr()
    _lib.call("hgr_layernorm_bwd", p(dy), 1, p(x), p(g), p(dx), p(dg), p(db), p(sc), rows, w, 1, None, 1e-5, _lib.HGR_BF16, torch.cuda.current_stream().cuda_stream)


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------
def _ln_bwd_reference(x, g, b, dy):
    x64, g64, b64 = (t.double().clone().requires_grad_(True) for t in (x, g, b))
    torch.nn.functional.layer_norm(x64, (x.shape[1],), g64, b64, 1e-5).backward(dy.double())
    xhat = (_ln64(x, torch.ones_like(g), torch.zeros_like(b))).detach()
    terms_g = (dy.double() * xhat).abs().sum(dim=0)                       # sum over rows of |term|, per column, in float64
    terms_b = dy.double().abs().sum(dim=0)
    return x64.grad, g64.grad, b64.grad, terms_g, terms_b


def _ln_bwd_run(x, g, dy, dx0, dg0, db0, cs0, dt16, mode, lead=_G):
    """One call of hgr_layernorm_bwd (`plain`), _cast (`cast`) or _cast_colsum (`colsum`); dgamma / dbeta / dx16_colsum `lead` elements
    into their buffers.  Returns the bands and the partial rows the kernel left in the scratch."""
    rows, w = x.shape
    dx, dg, db, cs = _Band(dx0), _Band(dg0, lead=lead), _Band(db0, lead=lead), _Band(cs0, lead=lead)
    c16 = _Band(shape=(rows, w), dtype=dt16)
    sc = _Band(shape=(ops.layernorm_bwd_scratch(rows, w),), dtype=F32)
    kw = {}
    if mode != "plain":
        kw["dx16"] = c16.t
    if mode == "colsum":
        kw["dx16_colsum"] = cs.t
    ops.layernorm_bwd(_in(dy), _in(x), _in(g), dx.t, dg.t, db.t, sc.t, **kw)
    for name, band in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("dx16_colsum", cs), ("dx16", c16), ("scratch", sc)):
        assert band.intact(), (mode, rows, w, name, "wrote outside its operand")
    if mode == "plain":
        assert _same(c16.buf, _Band(shape=(rows, w), dtype=dt16).buf)
    if mode != "colsum":
        assert _same(cs.cpu(), cs0)
    # one partial row per wave (include/hgr.h, hgr_layernorm_bwd_scratch_floats): [nw, w] for dgamma, [nw, w] for dbeta, the column-sum
    # scratch of ceil(nw / 512) rows, then [nw, w] for dx16_colsum
    nw = 4 * ((rows + 3) // 4 if rows < 2048 else 512)
    s = sc.cpu().double()
    third = 2 * nw * w + (nw + 511) // 512 * w
    part = [s[:nw * w].view(nw, w), s[nw * w:2 * nw * w].view(nw, w), s[third:third + nw * w].view(nw, w) if mode == "colsum" else None]
    return dx, dg, db, cs, c16, part


def _ln_bwd_check(rows, w, dyt, seed):
    x = _rand((rows, w), seed, 2.0) + 0.3
    g, b = 1 + 0.1 * _rand((w,), seed + 1), 0.1 * _rand((w,), seed + 2)
    dy = _rand((rows, w), seed + 3).to(dyt)
    dx0, dg0, db0, cs0 = _rand((rows, w), seed + 4), _rand((w,), seed + 5), _rand((w,), seed + 6), _rand((w,), seed + 7, 2.0)
    gx, gg, gb, terms_g, terms_b = _ln_bwd_reference(x, g, b, dy)
    bound_g, bound_b = 1e-5 * (1 + float(terms_g.max())), 1e-5 * (1 + float(terms_b.max()))
    for mode, dt16 in [("plain", torch.bfloat16)] + [(m, d) for m in ("cast", "colsum") for d in (DTS if dyt == F32 else [dyt])]:
        what = (mode, rows, w, dyt, dt16)
        dx, dg, db, cs, c16, _ = _ln_bwd_run(x, g, dy, dx0, dg0, db0, cs0, dt16, mode)
        _within(dx.cpu(), dx0.double() + gx, rtol=1e-4, atol=1e-4, what=("dx",) + what)     # test_layernorm_bwd's bound
        _within(dg.cpu(), dg0.double() + gg, rtol=0.0, atol=bound_g, what=("dgamma",) + what)
        _within(db.cpu(), db0.double() + gb, rtol=0.0, atol=bound_b, what=("dbeta",) + what)
        if mode != "plain":
            want16 = torch.empty(rows, w, dtype=dt16, device=DEV)
            ops.cast16(dx.t, want16)
            assert _same(c16.t, want16), ("dx16 is not hgr_cast16 of the returned dx",) + what
        if mode == "colsum":
            c64 = c16.cpu().double()                                     # the rows AS ROUNDED are what the column sums are of
            _within(cs.cpu(), cs0.double() + c64.sum(dim=0), rtol=0.0, atol=1e-5 * (1 + float(c64.abs().sum(dim=0).max())), what=("dx16_colsum",) + what)


@pytest.mark.parametrize("dyt", [F32] + DTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_layernorm_bwd_every_width(w, dyt):
    for rows in ROWS:
        _ln_bwd_check(rows, w, dyt, 500 + rows)


@pytest.mark.parametrize("dyt", [F32] + DTS)
@pytest.mark.parametrize("rows,w", [(2051, 260), (4100, 64)])
def test_layernorm_bwd_grid_stride_rows(rows, w, dyt):
    """From 2048 rows the launch is 512 blocks whose waves walk rows wid, wid + 2048, ...: 2051 rows give three waves a second row, 4100
    give every wave two or three."""
    _ln_bwd_check(rows, w, dyt, 600)


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("w", [64, 1028])
def test_layernorm_bwd_unaligned_targets_take_the_colsum_route(w, colsum):
    """dgamma / dbeta / dx16_colsum one float into their buffers (4-byte but not 16-byte aligned): the entry point reduces the partial rows
    with three hgr_colsum calls in place of the one 16-byte-vector launch.  Same bounds, and the same sums as the aligned call up to the
    order of the adds."""
    rows, dt16 = 37, torch.bfloat16
    x = _rand((rows, w), 700, 2.0) + 0.3
    g, b = 1 + 0.1 * _rand((w,), 701), 0.1 * _rand((w,), 702)
    dy = _rand((rows, w), 703)
    dx0, dg0, db0, cs0 = _rand((rows, w), 704), _rand((w,), 705), _rand((w,), 706), _rand((w,), 707, 2.0)
    gx, gg, gb, terms_g, terms_b = _ln_bwd_reference(x, g, b, dy)
    mode = "colsum" if colsum else "cast"
    al = _ln_bwd_run(x, g, dy, dx0, dg0, db0, cs0, dt16, mode)
    un = _ln_bwd_run(x, g, dy, dx0, dg0, db0, cs0, dt16, mode, lead=_G + 1)
    assert un[1].t.data_ptr() % 16 == 4 and al[1].t.data_ptr() % 16 == 0
    assert _same(al[0].t, un[0].t) and _same(al[4].t, un[4].t)             # dx, dx16: the row kernel is the same launch
    _within(un[0].cpu(), dx0.double() + gx, rtol=1e-4, atol=1e-4, what="dx")
    _within(un[1].cpu(), dg0.double() + gg, rtol=0.0, atol=1e-5 * (1 + float(terms_g.max())), what="dgamma")
    _within(un[2].cpu(), db0.double() + gb, rtol=0.0, atol=1e-5 * (1 + float(terms_b.max())), what="dbeta")
    part = al[5]                                                         # the partial rows both routes add up
    assert all(torch.equal(p, q) for p, q in zip(part, un[5]) if p is not None)
    if colsum:
        c64 = un[4].cpu().double()
        _within(un[3].cpu(), cs0.double() + c64.sum(dim=0), rtol=0.0, atol=1e-5 * (1 + float(c64.abs().sum(dim=0).max())), what="dx16_colsum")
    for i, name in ((1, "dgamma"), (2, "dbeta")) + (((3, "dx16_colsum"),) if colsum else ()):
        tol = 1e-6 * (1 + float(part[i - 1].abs().sum(dim=0).max()))
        assert float((un[i].cpu().double() - al[i].cpu().double()).abs().max()) <= tol, name


def test_layernorm_bwd_rejects_bad_widths():
    for w in (6, 4100):
        x = torch.zeros(2, w, device=DEV)
        v = torch.ones(w, device=DEV)
        dx = torch.zeros(2, w, device=DEV)
        with pytest.raises(HgrError):
            _lib_layernorm_bwd(x, x, v, dx, v.clone(), v.clone(), torch.zeros(64 * w, device=DEV), 2, w)
        assert not bool(dx.any())


# ==== 2. hgr_matmul_f32 ==========================================================================================================
def _mm_store(x, lay, trans):
    """Logical matrix x as the view the product is given: stored row-major (its transpose when `trans`, handed over as `.t()`), in a layout
    `lay` = "ld4" (leading dimension rounded up to 4, 16-byte aligned base: the 16-byte loads run), "packed" (ld = columns), "off1" (ld4, one
    float into the buffer), ("slice", j) (columns j .. of a matrix 16 columns wider) or "step" (every 2nd row and 3rd column)."""
    s = x.t().contiguous() if trans else x.contiguous()
    r, c = s.shape
    if lay == "step":
        big = _Band(shape=(2 * r, 3 * c), dtype=F32, poison=_POISON_IN)
        v = big.t[::2, ::3]
        v.copy_(s)
        assert v.stride() == (6 * c, 3)
    else:
        ld, coff, lead = c, 0, _G
        if lay in ("ld4", "off1"):
            ld = (c + 3) // 4 * 4
            lead = _G + (1 if lay == "off1" else 0)
        elif isinstance(lay, tuple):
            ld, coff = c + 16, lay[1]
        v = _in(s, ld=ld, coff=coff, lead=lead)
        assert v.stride(1) == 1 and (r == 1 or v.stride(0) == ld)
    return v.t() if trans else v


_MM_CASES = [(128, 64, 64, "ld4"),                       # every load a 16-byte one
             (66, 68, 36, "ld4"), (65, 63, 34, "ld4"),   # aligned strides, ragged sizes: the vector path runs into its `+ 3 <` guards
             (70, 90, 45, "packed"),                     # strides 45 / 90: scalar loads
             (1, 1, 300, "ld4"), (1, 90, 45, "ld4"), (70, 1, 45, "ld4"), (70, 90, 1, "ld4"), (1, 90, 45, "packed"), (70, 1, 45, "packed"),
             (52, 28, 40, ("slice", 4)), (52, 28, 40, ("slice", 3)),    # x[:, j:e] @ p[:, j:e].t() of CNZSL: aligned and unaligned first column
             (37, 41, 29, "step"), (66, 68, 36, "off1")]


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("m,n,k,lay", _MM_CASES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else None)
def test_matmul_f32_layouts_and_edges(m, n, k, lay, ta, tb):
    a, b, c0 = _rand((m, k), 800 + m), _rand((k, n), 801 + n), _rand((m, n), 802 + k, 2.0)
    a_dev, b_dev = _mm_store(a, lay, ta), _mm_store(b, lay, tb)
    if lay == "ld4" and (m, n, k) == (128, 64, 64):
        for t in (a_dev, b_dev):                         # the condition of the entry point for 16-byte loads holds for both operands
            assert t.data_ptr() % 16 == 0 and ((t.stride(1) == 1 and t.stride(0) % 4 == 0) or (t.stride(0) == 1 and t.stride(1) % 4 == 0))
    ab = a.double().abs() @ b.double().abs()
    prod = a.double() @ b.double()
    for accumulate in (False, True):
        for alpha in (1.0, -2.5):
            out = _Band(c0 if accumulate else None, shape=(m, n), dtype=F32, ld=n + 3)
            ops.matmul_f32(a_dev, b_dev, out.t, alpha=alpha, accumulate=accumulate)
            assert out.intact(), ("wrote outside C", accumulate, alpha)
            ref = alpha * prod + (c0.double() if accumulate else 0.0)
            # the bound of a sequential fp32 sum, twice over, + one rounding of the accumulating add: worst-case, so plain fp32 torch on
            # the CPU reaching 0.49 of it (accumulate, where the last add dominates) is no sign that it is too tight; it is kept as it is
            bound =2 * (k + 4) * 2.0 ** -24 * abs(alpha) * ab + (2.0 ** -23 * c0.double().abs() if accumulate else 0.0)
            _within(out.cpu(), ref, rtol=0.0, atol=bound, what=(accumulate, alpha))


# ==== 3. loss head and scatters ==================================================================================================
def _ce_check(lg, lab, pad, with_grad, what):
    rows, n = lg.shape
    gscale = 0.37 / rows
    lg_dev = _in(lg, ld=n + pad)
    loss = _Band(shape=(rows,), dtype=F32)
    dl = _Band(shape=(rows, n), dtype=F32, ld=n + pad)
    ops.ce_rows(lg_dev, lab.to(DEV), loss.t, dl.t if with_grad else None, gscale=gscale)
    assert loss.intact() and dl.intact(), what
    logp = torch.log_softmax(lg.double(), dim=-1)
    ref_loss = -logp[torch.arange(rows), lab.long()]
    _within(loss.cpu(), ref_loss, rtol=1e-5, atol=1e-5, what=("loss",) + what)
    if with_grad:
        onehot = torch.zeros(rows, n, dtype=torch.float64)
        onehot[torch.arange(rows), lab.long()] = 1.0
        _within(dl.cpu(), (logp.exp() - onehot) * gscale, rtol=1e-4, atol=1e-6 * gscale, what=("dlogits",) + what)
    else:
        assert _same(dl.buf, _Band(shape=(rows, n), dtype=F32, ld=n + pad).buf)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 21841])
def test_ce_rows_class_counts_and_views(n):
    for rows in (1, 3, 37):
        lg = _rand((rows, n), 900 + rows, 3.0)
        lab = _ints(901 + rows, rows, 0, n)
        first, last = lab.clone(), lab.clone()
        first[0], last[-1] = 0, n - 1                    # a label at column 0 and one at column n - 1
        for pad in (0, 5):                               # ld = n, and rows of a matrix 5 columns wider (logits and dlogits)
            for lb in (first, last):
                _ce_check(lg, lb, pad, True, (rows, n, pad))
            _ce_check(lg, last, pad, False, (rows, n, pad, "no dlogits"))


@pytest.mark.parametrize("shift", [80.0, -80.0])
def test_ce_rows_subtracts_the_row_maximum(shift):
    """Rows moved by +-80: exp() of the raw logits would overflow / vanish; every other row is left where it was."""
    rows, n = 37, 1000
    lg = _rand((rows, n), 910, 3.0)
    lg[::2] += shift
    lab = _ints(911, rows, 0, n)
    _ce_check(lg, lab, 5, True, (shift,))


@pytest.mark.parametrize("d", [1, 4, 63, 64, 65, 512, 1024])
def test_l2norm_bwd_widths(d):
    for rows in (1, 5, 37):
        x, dy, dx0 = _rand((rows, d), 920 + rows, 2.0), _rand((rows, d), 921 + rows), _rand((rows, d), 922 + rows)
        x64 = x.double().requires_grad_(True)
        (x64 / x64.norm(dim=-1, keepdim=True)).backward(dy.double())
        # D = 1, 5 rows: the gradient is exactly 0 (y = +-1), every fp32 evaluation cancels two terms of size |dy / x| (28 in row 3, where
        # |x| = 0.046), and plain fp32 torch autograd on the CPU is off by 1.91e-6 there, more than the whole 1e-6: 4 x that error.  (1 and 37
        # rows: 1.2e-7 and 2.4e-7, under a quarter of the bound, which stays.)
        atol = 4 * 1.91e-6 if (d, rows) == (1, 5) else 1e-6
        for accumulate in (False, True):
            dx = _Band(dx0)
            ops.l2norm_bwd(_in(x), _in(dy), dx.t, accumulate=accumulate)
            assert dx.intact(), (rows, d, accumulate)
            _within(dx.cpu(), x64.grad + (dx0.double() if accumulate else 0.0), rtol=1e-4, atol=atol, what=(rows, d, accumulate))


@pytest.mark.parametrize("w", [1, 3, 32, 512])
@pytest.mark.parametrize("case", ["random", "one_id"])
def test_embed_scatter_add_views_clamp_and_contention(case, w):
    """Token ids from a column slice of a wider token matrix (ld_tokens > L); ids of -1 and vocab + 7 are clamped by the kernel as by the
    reference; `one_id`: 2000 contributions to one table row.  The order of the atomics is free."""
    vocab, n, L, lt = 97, 40, 50, 77
    tok = torch.from_numpy(synth.randint(930, "rk", n * lt, 0, vocab)).view(n, lt).clone()
    if case == "one_id":
        tok[:, :L] = 41
    else:
        tok[0, 0], tok[1, 3], tok[n - 1, L - 1], tok[5, 7] = -1, vocab + 7, vocab + 7, -1
    tok[:, L:] = 10 ** 9                                  # the columns behind the slice are never read
    dx, tab0 = _rand((n * L, w), 931), _rand((vocab, w), 932)
    tab = _Band(tab0)
    ops.embed_scatter_add(tok.to(DEV)[:, :L], _in(dx), tab.t, L)
    assert tab.intact()
    ids = tok[:, :L].reshape(-1).clamp(0, vocab - 1)
    ref = tab0.double().index_add(0, ids, dx.double())
    mass = tab0.double().abs().index_add(0, ids, dx.double().abs())
    _within(tab.cpu(), ref, rtol=0.0, atol=1e-6 * (1 + mass), what=(case, w))


@pytest.mark.parametrize("alpha", [1.0, -1.5])
@pytest.mark.parametrize("w", [1, 33, 512])
def test_rows_axpy_forms(w, alpha):
    """dst[r * dst_mul + idx[r]] += alpha * src[r] for DISTINCT destination rows: dst_mul = 0 with a permutation and with a strict
    subset (the text-feature gradients of an inner step), dst_mul = L with an index per group, and no index at all."""
    nd, L = 24, 6
    perm = torch.from_numpy(np.argsort(synth.uniform(940, "rk", nd), kind="stable").astype(np.int32))
    forms = [("permutation", nd, 0, perm, perm.long()), ("subset", 9, 0, perm[:9].contiguous(), perm[:9].long())]
    idx = _ints(941, nd // L, 0, L)
    forms.append(("grouped", nd // L, L, idx, torch.arange(nd // L) * L + idx.long()))
    forms.append(("no index", nd, 1, None, torch.arange(nd)))
    forms.append(("no index, stride L", nd // L, L, None, torch.arange(nd // L) * L))
    for name, rows, mul, ix, dest in forms:
        dst0, src = _rand((nd, w), 942, 2.0), _rand((rows, w), 943)
        dst = _Band(dst0)
        ops.rows_axpy(dst.t, _in(src), dst_mul=mul, dst_idx=None if ix is None else ix.to(DEV), alpha=alpha)
        assert dst.intact(), name
        got = dst.cpu()
        ref = dst0.double().clone()
        ref[dest] += alpha * src.double()
        # two roundings (alpha * src, then the add) of at most 2^-24 each: a worst-case bound that no fp32 evaluation exceeds.  Plain fp32
        # torch on the CPU comes to 0.88 of it, which is what a worst-case bound of two roundings looks like, so it is kept as it is.
        bound = torch.zeros(nd, w, dtype=torch.float64)
        bound[dest] = 2.0 ** -23 * (dst0.double()[dest].abs() + (alpha * src.double()).abs())
        _within(got, ref, rtol=0.0, atol=bound, what=(name, w, alpha))
        rest = torch.ones(nd, dtype=torch.bool)
        rest[dest] = False
        assert _same(got[rest], dst0[rest]), (name, "a row that is no destination changed")


@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("w", [1, 4, 33, 512])
def test_rows_gather_exact(w, rows):
    ns = 50
    src = _rand((ns, w), 950)
    idx = _ints(951, rows, 0, ns)                         # 300 draws from 50 rows: repeats
    idx[0] = ns - 1                                       # the last source row
    if rows > 2:
        idx[1], idx[2] = 0, 0
    out = _Band(shape=(rows, w), dtype=F32)
    ops.rows_gather(_in(src), idx.to(DEV), out.t)
    assert out.intact() and _same(out.cpu(), src[idx.long()])


@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 100003, 512 * 257])
def test_dot_f32_lengths_and_fixed_order(n):
    """One workgroup of 1024 threads, each a sequential sum of n / 1024 products, then a 6 + 16 step reduction: hence the
    bound (n / 1024 + 24) 2^-24 sum |a_i b_i|, times |alpha|.  The starting value of the accumulating form is 0.37 sum |a_i b_i|: not
    zero, and small enough that the rounding of the last add (2^-24 of at most 1.37 |alpha| sum |a_i b_i|) is inside the 24."""
    a, b = _rand((n,), 960), _rand((n,), 961)
    mass = float((a.double() * b.double()).abs().sum())
    dot = float((a.double() * b.double()).sum())
    a_dev, b_dev = _in(a), _in(b)
    for alpha in (1.0, -0.75):
        start = np.float32(0.37 * abs(alpha) * mass)
        for accumulate in (False, True):
            got = []
            for _ in range(2):
                out = _Band(torch.tensor([float(start)], dtype=F32) if accumulate else None, shape=(1,), dtype=F32)
                ops.dot_f32(a_dev, b_dev, out.t, alpha=alpha, accumulate=accumulate)
                assert out.intact()
                got.append(out.cpu())
            assert _same(got[0], got[1]), "two calls on the same data differ"
            ref = alpha * dot + (float(start) if accumulate else 0.0)
            assert abs(float(got[0][0]) - ref) <= (n / 1024 + 24) * 2.0 ** -24 * abs(alpha) * mass, (n, alpha, accumulate, float(got[0][0]), ref)


_CTX = [(1, 3, 1, 4), (5, 77, 16, 512), (130, 20, 4, 65)]


@pytest.mark.parametrize("n,L,n_ctx,w", _CTX)
def test_ctx_splice_exact(n, L, n_ctx, w):
    x0, ctx, pos = _rand((n * L, w), 970), _rand((n_ctx, w), 971), _rand((L, w), 972)
    x = _Band(x0)
    ops.ctx_splice(x.t, _in(ctx), _in(pos), n, L)
    assert x.intact()
    want = x0.clone().view(n, L, w)
    want[:, 1:1 + n_ctx] = ctx + pos[1:1 + n_ctx]            # one fp32 add; row 0 and the rows behind the context stay as they were
    assert _same(x.cpu(), want.view(n * L, w))


@pytest.mark.parametrize("n,L,n_ctx,w", _CTX + [(3, 20, 4, 65), (4, 20, 4, 65)])
def test_ctx_splice_bwd(n, L, n_ctx, w):
    dx0, dctx0 = _rand((n * L, w), 980), _rand((n_ctx, w), 981)
    runs = []
    for _ in range(2):
        dx, dctx = _Band(dx0), _Band(dctx0)
        ops.ctx_splice_bwd(dx.t, dctx.t, n, L)
        assert dx.intact() and dctx.intact()
        runs.append((dx.cpu(), dctx.cpu()))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "two runs differ"
    rows64 = dx0.double().view(n, L, w)[:, 1:1 + n_ctx]
    _within(runs[0][1], dctx0.double() + rows64.sum(dim=0), rtol=0.0, atol=1e-6 * (dctx0.double().abs() + rows64.abs().sum(dim=0)), what="dctx")
    want = dx0.clone().view(n, L, w)
    want[:, 1:1 + n_ctx] = 0.0                               # the context rows are cleared (+0.0), every other row keeps its bits
    assert _same(runs[0][0], want.view(n * L, w))


# ==== 4. input assembly ==========================================================================================================
@pytest.mark.parametrize("b,L,w", [(1, 1, 4), (3, 50, 768), (2, 5, 260)])
def test_vit_assemble_exact(b, L, w):
    t0, cls, pos = _rand((b * L, w), 990), _rand((w,), 991), _rand((L, w), 992)
    t = _Band(t0)
    ops.vit_assemble(t.t, _in(cls), _in(pos), b, L)
    assert t.intact()
    want = t0.view(b, L, w) + pos
    want[:, 0] = want[:, 0] + cls
    assert _same(t.cpu(), want.view(b * L, w))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("r,p", [(64, 32), (28, 14), (224, 16)])
def test_im2col_patches_tokens_equals_im2col_rows(dt, r, p):
    b, g = 2, r // p
    L, k = g * g + 1, 3 * p * p
    kp = (k + 63) // 64 * 64
    img = synth.images(b, r, 7).to(DEV)
    flat = torch.empty(b * g * g, kp, dtype=dt, device=DEV)
    ops.im2col_patches(img, flat, p)
    tok = _Band(shape=(b * L, kp), dtype=dt)
    ops.im2col_patches_tokens(img, tok.t, p, L)
    assert tok.intact()
    got = tok.cpu().view(b, L, kp)
    assert _same(got[:, 1:].reshape(b * g * g, kp), flat.cpu())          # row b * L + 1 + q = row b * g^2 + q of the flat form
    assert kp == k or bool((got[:, 1:, k:].float() == 0).all())             # the K padding is zero (28 / 14: K = 588 in Kp = 640)
    assert _same(got[:, 0], _Band(shape=(b, kp), dtype=dt).cpu())          # the class rows keep their bits
    assert _same(flat.cpu()[:, :k].float(), _patches(img.cpu(), p).to(dt).float())


def _patches(img, p):
    """[B, 3, R, R] -> [B * g * g, 3 * p * p] in (c, py, px) order (the unfold of a stride-p convolution)."""
    b, c, r, _ = img.shape
    g = r // p
    return img.view(b, c, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, c * p * p)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("norm", ["clip", "custom"])
@pytest.mark.parametrize("p,gr", [(p, gr) for p in (4, 16, 32) for gr in (1, 2, 7)])
def test_im2col_patches_u8_normalises_every_byte_value(p, gr, norm, dt):
    r = p * gr
    b = max(2, -(-256 // (3 * r * r)))                           # enough images for all 256 byte values
    flat = (torch.arange(b * r * r * 3, dtype=torch.int64) * 37 + 11) % 256      # 37 is odd: any 256 consecutive bytes are all values
    assert flat.unique().numel() == 256
    img = flat.to(torch.uint8).view(b, r, r, 3)
    kw = {} if norm == "clip" else dict(mean=(0.5, 0.25, 0.125), std=(0.5, 0.3, 1.7))
    mean, std = (ops.CLIP_MEAN, ops.CLIP_STD) if norm == "clip" else (kw["mean"], kw["std"])
    out = _Band(shape=(b * gr * gr, 3 * p * p), dtype=dt)
    ops.im2col_patches_u8(_in(img.view(-1)).view(b, r, r, 3), out.t, p, **kw)
    assert out.intact()
    v = (img.double() / 255 - torch.tensor(mean, dtype=torch.float64)) / torch.tensor(std, dtype=torch.float64)
    ref = v.view(b, gr, p, gr, p, 3).permute(0, 1, 3, 2, 4, 5).reshape(b * gr * gr, p * p * 3)      # (py, px, c) within a patch row
    # The first bound, half an ulp + 2^-22 (1 + |ref|), is too tight for fp32 arithmetic: v * (1 / (255 std)) + (-mean / std) in plain
    # fp32 torch on the CPU, over all 256 byte values and 3 channels (every case holds them all), is off the float64 reference by up to
    # 5.13e-7 = 1.07 of that bound with the CLIP constants (|ref| <= 2.2: three roundings of values up to 3.8, then a cancellation) and by
    # 1.98e-7 = 0.41 of it with the custom ones.  Hence 4 x the CPU fp32 error, per normalisation.
    _within(out.cpu(), ref, rtol=0.0, atol=4 * (5.13e-7 if norm == "clip" else 1.98e-7), extra=_half_ulp(ref, dt), what=(p, gr, norm, dt))


def test_im2col_patches_u8_rejects_padded_k_and_odd_patches():
    img = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 3 * 16 * 16 + 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(HgrError):
        ops.im2col_patches_u8(img, out, 16)                   # Kp != 3 * P * P: no K padding on this path
    img6 = torch.zeros(1, 12, 12, 3, dtype=torch.uint8, device=DEV)
    out6 = torch.zeros(4, 3 * 6 * 6, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(HgrError):
        ops.im2col_patches_u8(img6, out6, 6)                  # P % 4 != 0
    assert not bool(out.any()) and not bool(out6.any())
