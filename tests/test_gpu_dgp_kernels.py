"""GPU: the DGP graph kernels - hgr_csr_group_aggregate, hgr_csr_group_att_grad, hgr_dgp_loss_head, hgr_dropout_counter, hgr_adam_l2 - on
planted graphs whose result is exact and on random inputs inside an element-wise bound made from the arithmetic.
tests/test_dgp_kernels_host.py holds the graph table, the float64 references, the bounds and their derivation, and tests them on the CPU.

Every operand lives in guard bands of a NaN pattern (tests/test_gpu_row_kernels.py: inputs one pattern, outputs another), contiguous and
as a view with ld = C + 4, coff = 4: a float4 read one slice too far reaches the output, a write outside an output's view changes bits
that are compared afterwards, an output element that was not written is still a NaN.  The partial buffers of the split rows are band
views too (`op._partial`, `op._partial_groups`).  Planted cases compare every element for equality with the float64 result (which is an
fp32 number: see the host file) and run twice with bit-equal output; random cases compare EVERY element with its bound.

Worst error / bound over all cases, views and elements (printed per case as RATIO ...), beside the fp32 emulation of the host file:

                             MI355X    emulation (CPU)
    aggregate                0.228     0.251
    aggregate normalised     0.119     0.135
    att_grad                 0.050     0.050
    loss head: loss rows     0.138     0.130
    loss head: loss          0.064     0.023
    loss head: dO            0.335     0.335
    adam_l2 p / m / v        0.997 / 0.993 / 0.912     0.964 / 0.863 / 0.825

The Adam bound is sharp by construction - m' and p' end in one rounding of a value the rest of the error is small against, so the
worst of 3 * 2^20 elements comes close to u |value| - and the device stays inside it at every element of every step.

No kernel bug showed: the 0-edge row, the item that opens a new group on the chunk boundary, D = 32, dout aliasing g on a split row
and ld_dout > C in the head's 2-D clear all give the exact planted result with every band intact.

Time on the MI355X: 6 s for the 75 tests of this file, the slowest 0.4 s; the whole GPU suite takes 384 s with them (2416 tests),
378 s without (2341)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import _lib, ops
from hgr_net_amd._lib import HgrError
from hgr_net_amd.baseline import dgp

import test_dgp_kernels_host as H
from test_gpu_row_kernels import _Band, _in, _G, _INT, _same

DEV = "cuda"
F32 = torch.float32
VIEWS = [("contiguous", lambda c: {}), ("banded", lambda c: dict(ld=c + 4, coff=4))]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _written(band):
    """No element of the output still holds the poison it started with."""
    return not bool((band.t.contiguous().view(_INT[band.dtype]) == band.poison).any())


def _untouched(band):
    return bool((band.buf.view(_INT[band.dtype]) == band.poison).all())


def _np(band):
    return band.cpu().numpy()


def _report(kernel, worst):
    print("RATIO %s %.3f" % (kernel, worst))


def _band_partials(op, c):
    """The split rows' partial buffers as band views of the right shape; `partial(c)` reuses a buffer whose width matches."""
    if op.n_slots == 0:
        return []
    pb, pg = _Band(shape=(op.n_slots, c), dtype=F32), _Band(shape=(op.n_slots, op.D), dtype=F32)
    op._partial, op._partial_groups = pb.t, pg.t
    assert op.partial(c) is pb.t and op.partial_groups() is pg.t
    return [pb, pg]


def _aggregate(op, S, att, bias, slope, normalize, kw):
    """Two calls into fresh poisoned outputs, bit-equal; all bands checked; the output on the CPU."""
    c = S.shape[1]
    s_dev, a_dev, b_dev = _in(_t(S), **kw(c)), _in(_t(att)), (None if bias is None else _in(_t(bias)))
    got = []
    for _ in range(2):
        parts = _band_partials(op, c)
        out = _Band(shape=S.shape, dtype=F32, **kw(c))
        ops.csr_group_aggregate(s_dev, op, a_dev, b_dev, out.t, slope, normalize)
        torch.cuda.synchronize()
        assert out.intact() and all(p.intact() for p in parts), "wrote outside its view"
        assert _written(out), "a row or slice was not written"
        got.append(out.cpu())
    assert _same(got[0], got[1])
    return got[0].numpy()


def _att_grad(op, S, bias, g, y, slope, kw, mode):
    """mode: 'dout' (a separate dout), 'alias' (dout is g), 'none' (no dout; y must be None).  -> (P, dO or None) on the CPU."""
    c = S.shape[1]
    s_dev, b_dev = _in(_t(S), **kw(c)), _in(_t(bias))
    y_dev = None if y is None else _in(_t(y), **kw(c))
    got = []
    for _ in range(2):
        parts = _band_partials(op, c)
        P = _Band(shape=(op.n, op.D), dtype=F32)
        gb = _Band(_t(g), **kw(c)) if mode == "alias" else None
        g_dev = gb.t if gb is not None else _in(_t(g), **kw(c))
        db = gb if mode == "alias" else (_Band(shape=S.shape, dtype=F32, **kw(c)) if mode == "dout" else None)
        ops.csr_group_att_grad(s_dev, op, b_dev, g_dev, y_dev, None if db is None else db.t, P.t, slope)
        torch.cuda.synchronize()
        assert P.intact() and (db is None or db.intact()) and all(p.intact() for p in parts), "wrote outside its view"
        assert _written(P) and (db is None or _written(db)), "a row was not written"
        got.append((P.cpu(), None if db is None else db.cpu()))
    assert _same(got[0][0], got[1][0]) and (got[0][1] is None or _same(got[0][1], got[1][1]))
    return got[0][0].numpy(), (None if got[0][1] is None else got[0][1].numpy())


def _device_sides(name, planted):
    a, r = H.build(name, False, DEV, planted), H.build(name, True, DEV, planted)
    return {"a": a, "r": r, "a^T": a.adjoint(), "r^T": r.adjoint()}


# ==== planted graphs: exact ===================================================================================================================
@pytest.mark.parametrize("name,C", H.GRID)
def test_planted_exact(name, C):
    n, D = H.CASES[name][0], H.CASES[name][1]
    x = H.planted_inputs(n, D, C)
    sides = _device_sides(name, True) if C == 64 else {"a": H.build(name, False, DEV, True)}
    for side, op in sides.items():
        for bias in (x["bias"], None):
            H.exact_aggregate(op._coo, n, x["S"], x["att"], bias)
            for slope in (0.25, 1.0):
                ref = H.agg_ref(op._coo, n, x["S"], x["att"], bias, slope)[0]
                for view, kw in VIEWS:
                    got = _aggregate(op, x["S"], x["att"], bias, slope, False, kw)
                    assert H.same_values(got, ref), (name, side, C, slope, bias is None, view)
        if side in ("a", "r"):
            for y, slope, modes in ((x["y"], 0.25, ("dout", "alias")), (None, 1.0, ("none", "dout", "alias"))):
                H.exact_att_grad(op._coo, n, D, x["S"], x["bias"], x["g"], y, slope)
                P, _, _, _, d = H.att_grad_ref(op._coo, n, D, x["S"], x["bias"], x["g"], y, slope)
                for view, kw in VIEWS:
                    for mode in modes:
                        gP, gd = _att_grad(op, x["S"], x["bias"], x["g"], y, slope, kw, mode)
                        assert H.same_values(gP, P), (name, side, C, view, mode, y is None)
                        assert gd is None or H.bit_equal(gd, d), (name, side, C, view, mode, y is None)


# ==== random inputs: every element inside its bound ==========================================================================================
@pytest.mark.parametrize("name,C", H.GRID)
def test_random_within_bound(name, C):
    n, D = H.CASES[name][0], H.CASES[name][1]
    x = H.random_inputs(n, D, C)
    sides = _device_sides(name, False)
    if C != 64:
        sides = {k: sides[k] for k in ("a", "r")}
    worst = dict(aggregate=0.0, aggregate_normalised=0.0, att_grad=0.0)
    for side, op in sides.items():
        for normalize in (False, True):
            ref, bound = H.agg_ref(op._coo, n, x["S"], x["att"], x["bias"], 0.2, normalize)[:2]
            for view, kw in VIEWS:
                r = H.ratio(_aggregate(op, x["S"], x["att"], x["bias"], 0.2, normalize, kw), ref, bound)
                key = "aggregate_normalised" if normalize else "aggregate"
                worst[key] = max(worst[key], r)
                assert r <= 1, (name, side, C, normalize, view, r)
        P, bound, _, _, d = H.att_grad_ref(op._coo, n, D, x["S"], x["bias"], x["g"], x["y"], 0.2)
        for view, kw in VIEWS:
            for mode in ("dout", "alias"):
                gP, gd = _att_grad(op, x["S"], x["bias"], x["g"], x["y"], 0.2, kw, mode)
                r = H.ratio(gP, P, bound)
                worst["att_grad"] = max(worst["att_grad"], r)
                assert r <= 1 and H.bit_equal(gd, d), (name, side, C, view, mode, r)
    for k, v in worst.items():
        _report("%s %s C=%d" % (k, name, C), v)


# ==== loss head ===============================================================================================================================
def _head(O, rows, Fm, kw):
    n, c = O.shape
    o_dev, f_dev, r_dev = _in(_t(O), **kw(c)), _in(_t(Fm), **kw(c)), _t(rows).to(DEV)
    got = []
    for _ in range(2):
        lrows, loss, dout = _Band(shape=(len(rows),), dtype=F32), _Band(shape=(1,), dtype=F32), _Band(shape=(n, c), dtype=F32, **kw(c))
        ops.dgp_loss_head(o_dev, r_dev, f_dev, lrows.t, loss.t, dout.t)
        torch.cuda.synchronize()
        assert lrows.intact() and loss.intact() and dout.intact(), "wrote outside its view (padding columns of dout included)"
        assert _written(lrows) and _written(loss) and _written(dout)
        got.append((lrows.cpu(), loss.cpu(), dout.cpu()))
    assert all(_same(a, b) for a, b in zip(*got))
    unselected = torch.from_numpy(np.setdiff1d(np.arange(n), rows))
    assert not bool(got[0][2][unselected].view(torch.int32).any()), "unselected rows must be exactly +0 in columns < C"
    return tuple(t.numpy() for t in got[0])


@pytest.mark.parametrize("n,n_t,C", [(40, 8, 4), (40, 16, 64), (640, 512, 64), (16, 4, 4096)])
def test_loss_head_planted_exact(n, n_t, C):
    O, rows, Fm = H.head_planted(n, n_t, C)
    lrow, loss, dO = H.head_planted_expected(O, rows, Fm)
    for view, kw in VIEWS:
        gl, gL, gd = _head(O, rows, Fm, kw)
        assert H.bit_equal(gl, lrow) and H.bit_equal(gL, np.array([loss])), (view, "loss")
        assert H.same_values(gd, dO.astype(np.float64)), (view, "dO")
        assert bool(np.isfinite(gd).all())


@pytest.mark.parametrize("C", [4, 64, 1028, 4096])
@pytest.mark.parametrize("n_t", [1, 255, 256, 257, 600])
def test_loss_head_random_within_bound(n_t, C):
    O, rows, Fm = H.head_random(640, n_t, C, tiny_row=True)
    (lrow, loss, dO), (b_rows, b_loss, b_dO) = H.head_ref(O, rows, Fm)
    for view, kw in VIEWS:
        gl, gL, gd = _head(O, rows, Fm, kw)
        r = (H.ratio(gl, lrow, b_rows), H.ratio(gL, np.array([loss]), np.array([b_loss])), H.ratio(gd, dO, b_dO))
        for what, v in zip(("loss_rows", "loss", "dO"), r):
            _report("loss_head %s n_t=%d C=%d %s" % (what, n_t, C, view), v)
        assert max(r) <= 1, (n_t, C, view, r)


# ==== adam ====================================================================================================================================
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])             # the last one alone strides the 4096-block grid
def test_adam_l2_within_bound(n, wd):
    cfg = H.AdamCfg(wd=wd)
    p0, g0, m0, v0 = H.adam_inputs(n)
    p, m, v = _Band(_t(p0)), _Band(_t(m0)), _Band(_t(v0))
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3):
        g = g0 if step == 1 else H._normal(30 + step, (n,))
        before = (_np(p), g, _np(m), _np(v))
        ref, bnd = H.adam_ref(*before, step, cfg)
        ops.adam_l2(p.t, _in(_t(g)), m.t, v.t, cfg.lr, step, (cfg.b1, cfg.b2), cfg.eps, wd)
        torch.cuda.synchronize()
        assert p.intact() and m.intact() and v.intact()
        for k, (band, r64, b) in enumerate(zip((p, m, v), ref, bnd)):
            r = H.ratio(_np(band), r64, b)
            worst[k] = max(worst[k], r)
            assert r <= 1, (n, wd, step, "pmv"[k], r)
        assert not np.array_equal(_np(p), before[0])
    for what, v in zip("pmv", worst):
        _report("adam_l2 %s n=%d wd=%g" % (what, n, wd), v)


# ==== dropout ================================================================================================================================
@pytest.mark.parametrize("rows,C", [(1, 4), (3, 1020), (157, 40), (5, 4096)])
def test_dropout_counter_is_dropout_keep(rows, C):
    x = H._normal(50, (rows, C))
    for seed, step, layer in ((0, 1, 0), (0xDEADBEEF, 7, 2)):
        keep = dgp.dropout_keep(seed, step, layer, rows, C)
        want = _t(np.where(keep, x * np.float32(2.0), np.float32(0.0)).astype(np.float32))
        for view, kw in VIEWS:
            y = _Band(shape=(rows, C), dtype=F32, **kw(C))
            ops.dropout_counter(_in(_t(x), **kw(C)), y.t, seed, step, layer)
            inplace = _Band(_t(x), **kw(C))
            ops.dropout_counter(inplace.t, inplace.t, seed, step, layer)
            torch.cuda.synchronize()
            assert y.intact() and inplace.intact(), (rows, C, view)
            assert _same(y.cpu(), want) and _same(inplace.cpu(), want), (rows, C, view)
        # input and output with different leading dimensions
        y = _Band(shape=(rows, C), dtype=F32, ld=C + 8, coff=8)
        ops.dropout_counter(_in(_t(x), ld=C + 4, coff=0), y.t, seed, step, layer)
        assert y.intact() and _same(y.cpu(), want)


# ==== refusals ================================================================================================================================
def _refused(call, outs):
    with pytest.raises(HgrError):
        call()
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in outs), "a refused call wrote an output"


def _strided(band_rows, n, c, ld):
    """[n, c] with leading dimension ld (possibly < c: overlapping rows) over a poisoned buffer; (band, view)."""
    b = _Band(shape=(band_rows,), dtype=F32)
    return b, b.t.as_strided((n, c), (ld, 1))


def test_refusals_launch_nothing():
    name = H.WIDTH_CASE
    n, D = H.CASES[name][0], H.CASES[name][1]
    op = H.build(name, False, DEV)
    parts = _band_partials(op, 64)

    def agg(S, out, att=None, bias=None, o=op):
        ops.csr_group_aggregate(S, o, att if att is not None else _in(torch.ones(o.D)), bias, out, 0.2, False)

    def grad(S, g, y, dout, P, bias=None, o=op):
        ops.csr_group_att_grad(S, o, bias, g, y, dout, P, 0.2)

    def head(O, Fm, dout, lrows, loss, n_t=2):
        ops.dgp_loss_head(O, torch.zeros(n_t, dtype=torch.int32, device=DEV), Fm, lrows, loss, dout)

    P = _Band(shape=(n, D), dtype=F32)
    lrows, loss = _Band(shape=(n + 1,), dtype=F32), _Band(shape=(1,), dtype=F32)
    # C in {0, 6, 4100}: C = 0 as an empty column slice of a real operand, 6 inside ld = 8
    for c, kw in ((0, dict(ld=4)), (6, dict(ld=8)), (4100, {})):
        w = max(c, 4)
        mk_in = lambda rows=n: _in(torch.ones(rows, w), **kw)[:, :c]
        out = _Band(shape=(n, w), dtype=F32, **kw)
        ov = out.t[:, :c]
        vec = _in(torch.ones(w))[:c]
        _refused(lambda: agg(mk_in(), ov, bias=vec), [out] + parts)
        _refused(lambda: grad(mk_in(), mk_in(), mk_in(), ov, P.t, bias=vec), [out, P] + parts)
        _refused(lambda: head(mk_in(), mk_in(2), ov, lrows.t, loss.t), [out, lrows, loss])
        if c != 4100:                                              # the dropout kernel has no upper width
            _refused(lambda: ops.dropout_counter(mk_in(), ov, 0, 1, 0), [out])
    c = 64
    S = _in(torch.ones(n, c))
    good = lambda: _Band(shape=(n, c), dtype=F32)
    # ld not a multiple of 4 (c + 2), ld < C (c - 4: overlapping rows)
    for ld in (c + 2, c - 4):
        for which in range(5):
            ob, ov = _strided(n * (c + 4), n, c, ld)
            ib, iv = _strided(n * (c + 4), n, c, ld)
            fresh = good()
            if which == 0:
                _refused(lambda: agg(iv, fresh.t), [fresh] + parts)
                _refused(lambda: agg(S, ov), [ob] + parts)
            elif which == 1:
                _refused(lambda: grad(iv, S, None, None, P.t), [P] + parts)
            elif which == 2:
                _refused(lambda: grad(S, iv, None, None, P.t), [P] + parts)
                _refused(lambda: grad(S, S, iv, ov, P.t), [P, ob] + parts)
            elif which == 3:
                _refused(lambda: grad(S, S, None, ov, P.t), [P, ob] + parts)
                _refused(lambda: head(S, _in(torch.ones(2, c)), ov, lrows.t, loss.t), [ob, lrows, loss])
                _refused(lambda: ops.dropout_counter(S, ov, 0, 1, 0), [ob])
            else:
                _refused(lambda: head(iv, _in(torch.ones(2, c)), fresh.t, lrows.t, loss.t), [fresh, lrows, loss])
                _refused(lambda: head(S, ib.t.as_strided((2, c), (ld, 1)), fresh.t, lrows.t, loss.t), [fresh, lrows, loss])
                _refused(lambda: ops.dropout_counter(iv, fresh.t, 0, 1, 0), [fresh])
    # 4-byte but not 16-byte aligned operands
    off_in = lambda rows=n: _in(torch.ones(rows, c), lead=_G + 1)
    off_out = _Band(shape=(n, c), dtype=F32, lead=_G + 1)
    out = good()
    _refused(lambda: agg(off_in(), out.t), [out] + parts)
    _refused(lambda: agg(S, off_out.t), [off_out] + parts)
    _refused(lambda: agg(S, out.t, bias=_in(torch.ones(c), lead=_G + 1)), [out] + parts)
    _refused(lambda: grad(off_in(), S, None, None, P.t), [P] + parts)
    _refused(lambda: grad(S, off_in(), None, None, P.t), [P] + parts)
    _refused(lambda: grad(S, S, off_in(), out.t, P.t), [P, out] + parts)
    _refused(lambda: grad(S, S, None, off_out.t, P.t), [P, off_out] + parts)
    _refused(lambda: grad(S, S, None, None, P.t, bias=_in(torch.ones(c), lead=_G + 1)), [P] + parts)
    _refused(lambda: head(off_in(), _in(torch.ones(2, c)), out.t, lrows.t, loss.t), [out, lrows, loss])
    _refused(lambda: head(S, off_in(2), out.t, lrows.t, loss.t), [out, lrows, loss])
    _refused(lambda: head(S, _in(torch.ones(2, c)), off_out.t, lrows.t, loss.t), [off_out, lrows, loss])
    _refused(lambda: ops.dropout_counter(off_in(), out.t, 0, 1, 0), [out])
    _refused(lambda: ops.dropout_counter(S, off_out.t, 0, 1, 0), [off_out])
    # the partial buffer misaligned
    op_off = copy.copy(op)
    pb = _Band(shape=(op.n_slots, c), dtype=F32, lead=_G + 1)
    op_off._partial = pb.t
    _refused(lambda: agg(S, out.t, o=op_off), [out, pb])
    # D in {0, 33}: the tables of a real operator under another D
    for d in (0, 33):
        od = copy.copy(op)
        od.D = d
        Pd = _Band(shape=(n, max(d, 1)), dtype=F32)
        _refused(lambda: agg(S, out.t, att=_in(torch.ones(max(d, 1)))[:d], o=od), [out] + parts)
        _refused(lambda: grad(S, S, None, None, Pd.t[:, :d], o=od), [Pd] + parts)
    # split tables without a partial buffer
    bare = copy.copy(op)
    bare.partial, bare.partial_groups = (lambda c_: None), (lambda: None)
    _refused(lambda: agg(S, out.t, o=bare), [out])
    _refused(lambda: grad(S, S, None, None, P.t, o=bare), [P])
    # y without dout: the wrapper refuses it first, so the C entry point is called as the wrapper would call it
    y = _in(torch.ones(n, c))
    with pytest.raises(AssertionError):
        grad(S, S, y, None, P.t)
    p_ = lambda t: t.data_ptr()
    _refused(lambda: _lib.call("hgr_csr_group_att_grad", p_(S), c, 0, p_(S), c, p_(y), c, 0, 0, p_(op.item_row), p_(op.item_e0), p_(op.item_e1),
                               p_(op.item_slot), op.item_row.numel(), p_(op.col), p_(op.inv_deg), p_(op.grp), op.D, p_(op.split_row),
                               p_(op.split_slot0), p_(op.split_n), op.split_row.numel(), p_(op.partial_groups()), p_(P.t), c, 0.2,
                               torch.cuda.current_stream().cuda_stream), [P] + parts)
    # n_t > n
    _refused(lambda: head(S, _in(torch.ones(n + 1, c)), out.t, lrows.t, loss.t, n_t=n + 1), [out, lrows, loss])
    # rows * C past the 32-bit element index of the dropout: argument values only, nothing that large exists
    _refused(lambda: _lib.call("hgr_dropout_counter", p_(S), 4096, p_(out.t), 4096, (1 << 20) + 1, 4096, 0, 1, 0,
                               torch.cuda.current_stream().cuda_stream), [out])
    assert _untouched(P) and all(_untouched(b) for b in parts)
