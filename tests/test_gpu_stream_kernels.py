"""GPU: the streaming kernels of the OM training step - hgr_transpose16, hgr_transpose16_colsum, hgr_colsum, hgr_cast16,
hgr_cast16_transpose, hgr_quickgelu16, hgr_sumsq, hgr_adamw, hgr_bn_fold, hgr_bn_unfold_grad - on every dispatch route, finish and
ragged edge, at the smallest shape that reaches it.  tests/test_stream_host.py holds the case tables (with the route each case takes),
the float64 references and the error bounds, and tests them on the CPU.

Every operand lives in guard bands of a NaN pattern (tests/test_gpu_row_kernels.py: inputs one pattern, outputs and in-place operands
another): a read outside an input reaches the output, a write outside an output's view - the padding columns of a transposed output and
the floats behind the `nrb * cols` of column-sum scratch included - changes bits that are compared afterwards, and an output element that
was not written still holds the pattern.  Results are exact on bit patterns, planted values and integers, and within a bound derived
from the arithmetic on random data (the worst error / bound is printed as a RATIO line).  Misaligned operands are only ever given to an
entry point that takes its element-wise route for them or refuses them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops
from hgr_net_amd._lib import HgrError

import test_stream_host as H
from test_stream_host import BF16, F16, DTS, F32, NS, tag
from test_gpu_row_kernels import _Band, _G, _INT, _POISON, _POISON_IN, _same

DEV = "cuda"
_AVOID = sorted({_POISON[BF16], _POISON[F16], _POISON_IN[BF16], _POISON_IN[F16]})
_BIG = 1 << 20                          # operands above this many elements are made on the device


def _report(kernel, what, worst):
    print("RATIO %s %s %.3f" % (kernel, what, worst))


def _inb(x, **kw):
    """An input operand in guard bands of the input pattern (the band, not the view: it is checked after the call)."""
    return _Band(x, poison=_POISON_IN, **kw)


def _written(band):
    """No element of the output still holds the poison it started with."""
    return not bool((band.t.contiguous().view(_INT[band.dtype]) == band.poison).any())


def _intact(*bands):
    torch.cuda.synchronize()
    for i, b in enumerate(bands):
        assert b.intact(), "operand %d: a guard band or padding column changed" % i


def _bits_equal(a, b):
    """Bit equality on the device."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype])))


def _dev_ints(shape, seed, dt):
    """Integers in [-3, 3] made on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-3, 4, shape, device=DEV, dtype=torch.int8, generator=g).to(dt)


def _dev_normal(shape, seed, dt):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, device=DEV, generator=g).to(dt)


def _refused(call, outs, name=None):
    """tests/test_gpu_attention.py::_refused for several outputs: the entry point raises, and after a synchronize every output still
    holds its sentinel."""
    with pytest.raises(HgrError) as err:
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all()), "a refused call wrote"
    assert name is None or name in str(err.value), str(err.value)


def _off1(numel, dt, fill=None):
    """`numel` elements that start one element behind a 16-byte aligned address."""
    buf = torch.full((numel + 8,), 7.0 if fill is None else fill, dtype=dt, device=DEV)
    return buf[1:1 + numel]


# ==== transposition ================================================================================================================
@pytest.mark.parametrize("dt", DTS, ids=tag)
@pytest.mark.parametrize("c", H.TRANSPOSE_CASES, ids=lambda c: c.name)
def test_transpose16_bit_patterns(c, dt):
    x = H.bit_patterns((c.rows, c.cols), 7 + c.rows, _AVOID).view(dt)
    xb = _inb(x, ld=c.ldx, coff=c.coff, lead=_G + c.lead_x)
    yb = _Band(shape=(c.cols, c.rows), dtype=dt, ld=c.ldy, lead=_G + c.lead_y)
    ops.transpose16(xb.t, yb.t)
    _intact(xb, yb)                                         # the padding columns of y (ldy > rows) still hold poison
    assert _same(yb.cpu(), x.t().contiguous()), c.name


def _tcs_run(c, x, start, accumulate, alpha=0.5):
    """One hgr_transpose16_colsum call on banded operands: x the case's view (ldx, coff, lead), y its view (ldy, lead), the scratch
    exactly nrb * cols floats.  The transposition is checked here, bit for bit; returns (yt band, out band, scratch band)."""
    nrb = (c.rows + 63) // 64
    xb = _inb(x, ld=c.ldx, coff=c.coff, lead=_G + c.lead_x)
    yb = _Band(shape=(c.cols, c.rows), dtype=c.dt, ld=c.ldy, lead=_G + c.lead_y)
    sb = _Band(shape=(nrb * c.cols,), dtype=F32)
    ob = _Band(start) if accumulate else _Band(shape=(c.cols,), dtype=F32)
    ops.transpose16_colsum(xb.t, yb.t, ob.t, sb.t, accumulate=accumulate, alpha=alpha)
    _intact(xb, yb, sb, ob)                                 # y's padding columns and the floats behind nrb * cols still hold poison
    # a sum of 16-bit NaNs never carries the fp32 poison: a widened 16-bit payload has zeros in its low 13 bits, the poison has not
    assert _written(yb) and _written(ob) and _written(sb), c.name
    assert _bits_equal(yb.t, x.to(DEV).t()), c.name
    return yb, ob, sb


@pytest.mark.parametrize("c", H.TCS_CASES, ids=lambda c: c.name)
def test_transpose16_colsum_integers_exact(c):
    x = _dev_ints((c.rows, c.cols), c.rows + c.cols, c.dt)
    want = x.double().sum(0)
    start = _dev_ints((c.cols,), 5, F32)
    _, ob, _ = _tcs_run(c, x, start, True)                  # every (band, column) partial is written: _tcs_run
    assert torch.equal(ob.t.double(), start.double() + 0.5 * want), c.name
    _, ob, _ = _tcs_run(c, x, None, False)
    assert torch.equal(ob.t.double(), 0.5 * want), c.name
    if c.rows <= 3000:                                      # any bit pattern through the CS instantiations, on the case's own views
        bits = H.bit_patterns((c.rows, c.cols), 9 + c.rows, _AVOID).view(c.dt)
        yb, _, _ = _tcs_run(c, bits, None, False)           # (the sums are not looked at: the patterns hold NaNs and infinities)
        assert _same(yb.cpu(), bits.t().contiguous()), c.name


@pytest.mark.parametrize("c", [c for c in H.TCS_CASES if c.rows in H.TCS_RANDOM_ROWS], ids=lambda c: c.name)
def test_transpose16_colsum_random_within_bound(c):
    x = _dev_normal((c.rows, c.cols), 3 * c.rows + c.cols, c.dt)
    start = _dev_normal((c.cols,), 11, F32)
    _, ob, _ = _tcs_run(c, x, start, True)
    ref = (start.double() + 0.5 * x.double().sum(0)).cpu()
    bound = H.sum_bound(x.double().abs().sum(0).cpu(), ref, H.tcs_depth(c.rows), 0.5)
    _report("transpose16_colsum", "%s rows=%d" % (tag(c.dt), c.rows), H.within(ob.cpu(), ref, bound, c.name))


@pytest.mark.parametrize("c", H.TCS_REFUSED, ids=lambda c: c.name)
def test_transpose16_colsum_refuses_unaligned_rows(c):
    xbuf = torch.zeros(c.rows * c.ldx + 8, dtype=c.dt, device=DEV)
    ybuf = torch.full((c.cols * c.ldy + 8,), 7.0, dtype=c.dt, device=DEV)
    x = xbuf[c.lead_x:c.lead_x + c.rows * c.ldx].view(c.rows, c.ldx)[:, :c.cols]
    y = ybuf[c.lead_y:c.lead_y + c.cols * c.ldy].view(c.cols, c.ldy)[:, :c.rows]
    out = torch.full((c.cols,), 7.0, device=DEV)
    scratch = torch.full((2 * c.cols,), 7.0, device=DEV)
    _refused(lambda: ops.transpose16_colsum(x, y, out, scratch), [ybuf, out, scratch], "hgr_transpose16_colsum")


# ==== column sums ==================================================================================================================
def _colsum_run(c, x, start, accumulate, alpha=0.5):
    nrb = (c.rows + 511) // 512
    xb = _inb(x, ld=c.ldx, coff=c.coff, lead=_G + c.lead_x)
    sb = _Band(shape=(nrb * c.cols,), dtype=F32)
    ob = _Band(start, lead=_G + c.lead_o) if accumulate else _Band(shape=(c.cols,), dtype=F32, lead=_G + c.lead_o)
    ops.colsum(xb.t, ob.t, sb.t, accumulate=accumulate, alpha=alpha)
    _intact(xb, sb, ob)
    assert _written(ob), c.name
    assert c.route == "rows_f32" or _written(sb), c.name           # rows_f32 is one pass: it leaves the scratch alone
    return ob


@pytest.mark.parametrize("c", H.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_integers_exact(c):
    x = _dev_ints((c.rows, c.cols), c.rows + c.cols, c.dt)
    want = x.double().sum(0)
    start = _dev_ints((c.cols,), 5, F32)
    ob = _colsum_run(c, x, start, True)
    assert torch.equal(ob.t.double(), start.double() + 0.5 * want), c.name
    if c.rows * c.cols <= _BIG:
        ob = _colsum_run(c, x, None, False)
        assert torch.equal(ob.t.double(), 0.5 * want), c.name


@pytest.mark.parametrize("c", [c for c in H.COLSUM_CASES if c.random], ids=lambda c: c.name)
def test_colsum_random_within_bound(c):
    x = _dev_normal((c.rows, c.cols), 3 * c.rows + c.cols, c.dt)
    start = _dev_normal((c.cols,), 13, F32)
    ob = _colsum_run(c, x, start, True)
    ref = (start.double() + 0.5 * x.double().sum(0)).cpu()
    bound = H.sum_bound(x.double().abs().sum(0).cpu(), ref, H.colsum_depth(c), 0.5)
    _report("colsum", "%s %s" % (c.route, tag(c.dt)), H.within(ob.cpu(), ref, bound, c.name))


# ==== casts ========================================================================================================================
@pytest.mark.parametrize("dt", DTS, ids=tag)
@pytest.mark.parametrize("n", [n for n, _ in H.CAST_NS])
def test_cast16_rounds_to_nearest_even(n, dt):
    pat, tail = H.cast_pattern(dt)
    body = n - 4
    reps = (body + H.CAST_PATTERN - 1) // H.CAST_PATTERN
    xd = torch.cat([pat.to(DEV).repeat(reps)[:body], tail.to(DEV)])
    xb = _inb(xd)
    yb = _Band(shape=(n,), dtype=dt)
    ops.cast16(xb.t, yb.t)
    _intact(xb, yb)
    assert _written(yb)
    head = min(body, H.CAST_PATTERN)
    got = torch.cat([yb.t[:head], yb.t[body:]]).cpu()
    want = torch.cat([pat[:head], tail]).to(dt)
    if not H.same_bits16(got, want):                        # name the values that went wrong
        src = torch.cat([pat[:head], tail])
        bad = [i for i in range(got.numel()) if not H.same_bits16(got[i:i + 1], want[i:i + 1])]
        assert not bad, (n, tag(dt), [(i, float(src[i]), hex(int(got.view(torch.int16)[i]) & 0xFFFF)) for i in bad[:8]])
    whole = body // H.CAST_PATTERN
    if whole > 1:                                           # every further block carries the first block's bits
        blocks = yb.t[:whole * H.CAST_PATTERN].view(whole, H.CAST_PATTERN).view(torch.int16)
        assert bool((blocks == blocks[0:1]).all())
        rest = body - whole * H.CAST_PATTERN
        assert rest == 0 or _bits_equal(yb.t[whole * H.CAST_PATTERN:body], yb.t[:rest])


@pytest.mark.parametrize("dt", DTS, ids=tag)
@pytest.mark.parametrize("c", H.CAST_T_CASES, ids=lambda c: c.name)
def test_cast16_transpose_both_copies(c, dt):
    x = H.normal((c.rows, c.cols), 17 + c.rows, 0.7)
    s = H.cast_specials(dt)
    k = min(s.numel(), x.numel())
    x.view(-1)[:k] = s[:k]
    xb = _inb(x, ld=c.ldx, lead=_G + c.lead_x)
    yb = _Band(shape=(c.rows, c.cols), dtype=dt, ld=c.ldy, lead=_G + c.lead_y)
    tb = _Band(shape=(c.cols, c.rows), dtype=dt, ld=c.ldyt, lead=_G + c.lead_t)
    ops.cast16_transpose(xb.t, yb.t, tb.t)
    _intact(xb, yb, tb)                                     # y's columns beyond cols and yt's beyond rows are untouched
    assert _written(yb) and _written(tb)
    want = x.to(dt)
    assert H.same_bits16(yb.cpu(), want) and H.same_bits16(tb.cpu(), want.t().contiguous()), c.name


# ==== QuickGELU ====================================================================================================================
def _gelu_call(x, du, dt, n):
    ab, db = _inb(x), _inb(du)
    fb, gb = _Band(shape=(n,), dtype=dt), _Band(shape=(n,), dtype=dt)
    ops.quickgelu16(ab.t, fb.t)
    ops.quickgelu16(ab.t, gb.t, du=db.t)
    _intact(ab, db, fb, gb)
    assert _written(fb) and _written(gb)
    return fb, gb


@pytest.mark.parametrize("dt", DTS, ids=tag)
@pytest.mark.parametrize("n", [n for n, _ in H.GELU_NS])
def test_quickgelu_within_bounds(n, dt):
    px, pdu = H.gelu_inputs(H.GELU_PATTERN, dt)
    reps = (n + H.GELU_PATTERN - 1) // H.GELU_PATTERN
    x, du = px.to(DEV).repeat(reps)[:n], pdu.to(DEV).repeat(reps)[:n]
    fb, gb = _gelu_call(x, du, dt, n)
    head = min(n, H.GELU_PATTERN)
    rf, rb = H.gelu_ref64(px[:head], pdu[:head])
    assert bool(torch.isfinite(rf).all()) and bool(torch.isfinite(rb).all())
    wf = H.ratio(fb.t[:head].cpu(), rf, H.gelu_fwd_bound(rf, dt))
    wb = H.ratio(gb.t[:head].cpu(), rb, H.gelu_bwd_bound(rb, pdu[:head].double(), dt))
    _report("quickgelu_fwd", tag(dt), wf)
    _report("quickgelu_bwd", tag(dt), wb)
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)
    whole = n // H.GELU_PATTERN
    for band in (fb, gb):
        if whole > 1:
            blocks = band.t[:whole * H.GELU_PATTERN].view(whole, H.GELU_PATTERN).view(torch.int16)
            assert bool((blocks == blocks[0:1]).all())
            rest = n - whole * H.GELU_PATTERN
            assert rest == 0 or _bits_equal(band.t[whole * H.GELU_PATTERN:], band.t[:rest])


@pytest.mark.parametrize("dt", DTS, ids=tag)
def test_quickgelu_planted_values(dt):
    x, du = H.gelu_planted(dt)
    fb, gb = _gelu_call(x, du, dt, x.numel())
    f, g = fb.cpu(), gb.cpu()
    assert _same(f[:8], x[:8]) and _same(g[:8], du[:8])                                    # x >= 16: out == x, grad == du, bit for bit
    assert bool((f[8:16].float() == 0).all()) and bool((g[8:16].float() == 0).all())       # x <= -64: the value 0
    assert bool((f[16:].float() == 0).all())                                                # x = +-0: 0 and du / 2 rounded once
    want = (du[16:].double() * 0.5).to(dt)
    assert torch.equal(g[16:].float(), want.float())
    # bit for bit, but for one thing: f16 rounds the product once through an FMA with a +0 addend, which returns +0 where the product is
    # -0 (du = -0) - there the value 0 stands, as above; bf16 is a plain product and keeps the sign
    keep = torch.ones_like(want, dtype=torch.bool) if dt == BF16 else want.view(torch.int16) != -32768
    assert dt == F16 or bool(keep.all())
    assert int(keep.sum()) >= want.numel() - 1 and _same(g[16:][keep], want[keep])


@pytest.mark.parametrize("dt", DTS, ids=tag)
def test_quickgelu_refusals_write_nothing(dt):
    ok = lambda n=16: torch.full((n,), 7.0, dtype=dt, device=DEV)
    out = ok()
    _refused(lambda: ops.quickgelu16(ok(12), out[:12]), [out], "hgr_quickgelu16")                          # n % 8 != 0
    _refused(lambda: ops.quickgelu16(ok(4), out[:4]), [out], "hgr_quickgelu16")                            # n < 8
    _refused(lambda: ops.quickgelu16(_off1(16, dt), out), [out], "hgr_quickgelu16")                        # a misaligned
    _refused(lambda: ops.quickgelu16(ok(), out, du=_off1(16, dt)), [out], "hgr_quickgelu16")               # du misaligned
    buf = torch.full((24,), 7.0, dtype=dt, device=DEV)
    _refused(lambda: ops.quickgelu16(ok(), buf[1:17]), [buf], "hgr_quickgelu16")                           # out misaligned
    _refused(lambda: ops.quickgelu16(ok(), buf[1:17], du=ok()), [buf], "hgr_quickgelu16")


def test_cast16_refusals_write_nothing():
    out = torch.full((16,), 7.0, dtype=BF16, device=DEV)
    x = torch.ones(16, device=DEV)
    _refused(lambda: ops.cast16(x[:6], out[:6]), [out], "hgr_cast16")                                      # n % 4 != 0
    _refused(lambda: ops.cast16(_off1(8, F32, 1.0), out[:8]), [out], "hgr_cast16")                         # x 4-byte aligned only
    _refused(lambda: ops.cast16(x[:8], out[1:9]), [out], "hgr_cast16")                                     # y 2-byte aligned only


# ==== sum of squares ===============================================================================================================
def _sumsq_ints(n, seed):
    x = _dev_ints((n,), seed, F32)
    return x, float((x.double() ** 2).sum())


@pytest.mark.parametrize("n", [n for n, _ in H.SUMSQ_NS])
def test_sumsq_exact_deterministic_and_within_bound(n):
    x, want = _sumsq_ints(n, n)
    xb = _inb(x)
    ob = _Band(torch.tensor([5.0]))
    ops.sumsq(xb.t, ob.t)
    _intact(xb, ob)
    assert float(ob.t[0]) == 5.0 + want
    xr = _dev_normal((n,), n + 1, F32)
    xb = _inb(xr)
    tots = []
    for _ in range(5):
        ob = _Band(torch.tensor([0.0]))
        ops.sumsq(xb.t, ob.t)
        _intact(xb, ob)
        tots.append(ob.cpu())
    assert all(_same(t, tots[0]) for t in tots), [float(t) for t in tots]
    ref = (xr.double() ** 2).sum().cpu().reshape(1)
    _report("sumsq", "n=%d" % n, H.within(tots[0], ref, H.sum_bound(ref, ref, H.sumsq_depth(n)), "sumsq"))


def test_sumsq_slot_ring_one_stream_then_two():
    """40 launches of mixed sizes in a row (more than twice round the 16 scratch slots), then 8 + 8 alternating on two streams - at most
    16 in flight, the bound include/hgr.h states."""
    sizes = [1, 255, 257, 262145, 1000, 786449, 262144]
    data = {n: _sumsq_ints(n, 100 + n) for n in sizes}
    outs = torch.zeros(40, device=DEV)
    torch.cuda.synchronize()
    for i in range(40):
        ops.sumsq(data[sizes[i % len(sizes)]][0], outs[i:i + 1])
    torch.cuda.synchronize()
    assert outs.cpu().tolist() == [data[sizes[i % len(sizes)]][1] for i in range(40)]
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs2 = torch.zeros(16, device=DEV)
    torch.cuda.synchronize()
    for i in range(16):
        with torch.cuda.stream(s[i % 2]):
            ops.sumsq(data[sizes[i % len(sizes)]][0], outs2[i:i + 1])
    torch.cuda.synchronize()
    assert outs2.cpu().tolist() == [data[sizes[i % len(sizes)]][1] for i in range(16)]


# ==== AdamW ========================================================================================================================
@pytest.mark.parametrize("n", [n for n, _ in H.ADAMW_NS])
@pytest.mark.parametrize("br", H.ADAMW_BRANCHES, ids=lambda b: b.name)
def test_adamw_three_steps(br, n):
    sc = H.adamw_scalars()
    hp = H.ADAMW_HP
    small = n if n <= 1000 else H.ADAMW_PATTERN + 3                  # the large case: a 1024 pattern repeated, and 3 tail elements
    reps = (n - 3) // H.ADAMW_PATTERN if n > 1000 else 0
    assert n <= 1000 or reps * H.ADAMW_PATTERN + 3 == n

    def spread(t):
        t = t.to(DEV)
        return t if not reps else torch.cat([t[:H.ADAMW_PATTERN].repeat(reps), t[H.ADAMW_PATTERN:]])

    def gather(band):
        if reps:
            blocks = band.t[:reps * H.ADAMW_PATTERN].view(reps, H.ADAMW_PATTERN).view(torch.int32)
            assert bool((blocks == blocks[0:1]).all()), "a block of the grid-stride loop differs from the first"
            return torch.cat([band.t[:H.ADAMW_PATTERN], band.t[reps * H.ADAMW_PATTERN:]]).cpu()
        return band.cpu()

    p, m, v, gs = H.adamw_inputs(small, br)
    pb, mb, vb = _Band(spread(p)), _Band(spread(m)), _Band(spread(v))
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        step = br.step0 + k
        g = gs[k]
        gd = spread(g)
        gb = _inb(gd)
        tb = _inb(H.sumsq_total_of(g)) if br.total else None
        ref = H.adamw_ref64(p, g, m, v, step, br, sc)
        bounds = H.adamw_bounds(p, g, m, v, step, br, sc, ref)
        ops.adamw(pb.t, gb.t, mb.t, vb.t, lr=hp["lr"], step=step, betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], wd=br.wd,
                  sumsq_total=None if tb is None else tb.t, max_norm=hp["max_norm"], grad_scale=br.gscale)
        _intact(pb, gb, mb, vb, *([] if tb is None else [tb]))
        assert _bits_equal(gb.t, gd), "g was written"
        got = gather(pb), gather(mb), gather(vb)
        for i in range(3):
            assert bool(torch.isfinite(ref[i]).all())
            worst[i] = max(worst[i], H.ratio(got[i], ref[i], bounds[i]))
        if k == 0 and br.zero and (not br.total or br.norm * br.gscale <= sc.max_norm):
            # no clip or an inactive one: the factor is exactly grad_scale, a power of two - m' and v' from a zero state are single products
            one, gi = np.float32(1.0), g * np.float32(br.gscale)
            assert _same(got[1], (one - np.float32(sc.b1)) * gi) and _same(got[2], (one - np.float32(sc.b2)) * gi * gi), br.name
        p, m, v = got                                               # the next step's reference starts from the kernel's own state bits
    print("RATIO adamw %s n=%d p %.3f m %.3f v %.3f" % (br.name, n, worst[0], worst[1], worst[2]))
    assert max(worst) <= 1.0, worst


# ==== batch-norm fold / unfold =========================================================================================================
def _bn_bands(cout, cin, khw):
    w, gamma, beta, mean, var = H.bn_inputs(cout, cin, khw, 41 + cin)
    bands = [_inb(t.reshape(-1)) for t in (w, gamma, beta, mean, var)]
    bn = NS(weight=bands[1].t, bias=bands[2].t, running_mean=bands[3].t, running_var=bands[4].t, eps=H.BN_EPS)
    return (w, gamma, beta, mean, var), bands, bn


@pytest.mark.parametrize("dt", DTS, ids=tag)
@pytest.mark.parametrize("cout", H.BN_COUT)
@pytest.mark.parametrize("pad", [False, True], ids=["Kp=K", "Kp=K_up_64"])
@pytest.mark.parametrize("cin,khw", H.BN_SHAPES)
def test_bn_fold_within_bound(cin, khw, pad, cout, dt):
    host, bands, bn = _bn_bands(cout, cin, khw)
    K = cin * khw
    kp = H.up(K, 64) if pad else K
    wb = _Band(shape=(cout, kp), dtype=dt)
    bb = _Band(shape=(cout,), dtype=F32)
    ops.bn_fold(bands[0].t.view(host[0].shape), bn, wb.t, bb.t)
    _intact(wb, bb, *bands)
    assert _written(wb) and _written(bb)
    rw, rb, _ = H.bn_fold_ref64(*host)
    bw, bbnd = H.bn_fold_bounds(*host, dt)
    got = wb.cpu()
    assert bool((got[:, K:].view(torch.int16) == 0).all()), "padding columns must be +0"
    worst = max(H.within(got[:, :K], rw, bw, "w16"), H.within(bb.cpu(), rb, bbnd, "bias"))
    _report("bn_fold", "%s K=%d" % (tag(dt), K), worst)


@pytest.mark.parametrize("cout", H.BN_COUT)
@pytest.mark.parametrize("pad", [False, True], ids=["ldg=K", "ldg=Kp"])
@pytest.mark.parametrize("cin,khw", H.BN_SHAPES)
def test_bn_unfold_grad_adds_within_bound(cin, khw, pad, cout):
    host, bands, bn = _bn_bands(cout, cin, khw)
    w, gamma, beta, mean, var = host
    K = cin * khw
    gwf, gbf = H.normal((cout, K), 51 + cin), H.normal((cout,), 52 + cin)
    start = (H.normal(tuple(w.shape), 53 + cin), H.normal((cout,), 54 + cin), H.normal((cout,), 55 + cin))
    gb = _inb(gwf, ld=H.up(K, 64) if pad else K)                     # the padding columns of gwf hold poison
    fb = _inb(gbf)
    outs = [_Band(start[0].reshape(-1)), _Band(start[1]), _Band(start[2])]
    ops.bn_unfold_grad(gb.t, fb.t, bands[0].t.view(w.shape), bn, outs[0].t.view(w.shape), outs[1].t, outs[2].t)
    _intact(gb, fb, *outs, *bands)
    ref = H.bn_unfold_ref64(gwf, gbf, w, gamma, beta, mean, var, start)
    bounds = H.bn_unfold_bounds(gwf, gbf, w, gamma, mean, var, start)
    got = outs[0].cpu().view(w.shape), outs[1].cpu(), outs[2].cpu()
    worst = max(H.within(got[i], ref[i], bounds[i], "unfold %d" % i) for i in range(3))
    _report("bn_unfold_grad", "K=%d" % K, worst)


def test_bn_refusals_write_nothing():
    z = lambda *s: torch.ones(*s, device=DEV)
    bn = NS(weight=z(2), bias=z(2), running_mean=z(2), running_var=z(2), eps=H.BN_EPS)
    w = z(2, 3, 2, 2)                                                 # khw = 4
    w16 = torch.full((2, 16), 7.0, dtype=F16, device=DEV)
    bias = torch.full((2,), 7.0, device=DEV)
    _refused(lambda: ops.bn_fold(w, bn, w16, bias), [w16, bias], "hgr_bn_fold")
    _refused(lambda: ops.bn_fold(z(2, 3, 3, 3), bn, w16, bias), [w16, bias], "hgr_bn_fold")          # Kp 16 < K 27
    outs = [torch.full((2, 3, 2, 2), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)]
    _refused(lambda: ops.bn_unfold_grad(z(2, 12), z(2), w, bn, *outs), outs, "hgr_bn_unfold_grad")
