"""GPU: the attention kernels (hgr_mha, hgr_mha_rows, hgr_mha_stats, hgr_mha_bwd, hgr_mha_bwd_stats, hgr_mha_bwd_colsum,
hgr_attnpool_attend) against planted inputs whose result is exact and against float64 restatements within an element-wise bound made
from the arithmetic - tests/test_attention_host.py holds the builders, the references and the bounds, and tests them on the CPU.

Every operand lives in guard bands of a NaN pattern (tests/test_gpu_row_kernels.py: inputs one pattern, outputs another): a read outside
an input reaches the output, a write outside an output's view changes bits that are compared afterwards, an output element that was
not written is still a NaN.  Shapes are tiny: b = 3, heads = 3 (blockIdx -> (b, h) with no power of two), once b = 1, heads = 12; one
length per code path and edge.  Which D the backward's reference uses at each length: test_attention_host.definition_of_d."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops
from hgr_net_amd._lib import HgrError

import test_attention_host as H
from test_attention_host import BF16, DTS, FWD_LENGTHS, BWD_LENGTHS, POOL_LENGTHS
from test_gpu_row_kernels import _Band, _in, _INT, _POISON_IN, _same

DEV = "cuda"
F32 = torch.float32
B, HEADS = 3, 3
W = HEADS * 64


def _tag(dt):
    return "bf16" if dt == BF16 else "f16"


def _report(kernel, dt, worst):
    print("RATIO %s %s %.3f" % (kernel, _tag(dt), worst))


def _written(band):
    """No element of the output still holds the poison it started with."""
    return not bool((band.t.contiguous().view(_INT[band.dtype]) == band.poison).any())


def _poison_like(band, rows):
    return torch.full(rows.shape, band.poison, dtype=_INT[band.dtype]).view(band.dtype)


def _forward(qkv_dev, b, L, heads, causal, dt, stats=False, q_rows=0):
    """One forward call into fresh poisoned outputs; the bands are checked, (out on the CPU, stats on the CPU or None) returned."""
    out = _Band(shape=(b * L, heads * 64), dtype=dt)
    st = _Band(shape=(b * heads * L, 2), dtype=F32) if stats else None
    ops.mha(qkv_dev, out.t, b, L, heads, causal, stats=st.t if stats else None, q_rows=q_rows)
    torch.cuda.synchronize()
    assert out.intact() and (st is None or st.intact()), "wrote outside its view"
    if q_rows in (0, L):
        assert _written(out)
    assert st is None or _written(st)
    return out.cpu(), (st.cpu().view(b, heads, L, 2) if stats else None)


def _leading_rows(qkv_dev, want, L, causal, dt):
    """hgr_mha_rows at q_rows in {1, 16, 17, L}: the first q_rows rows of every sequence carry the bits of `want`, the others are untouched."""
    for q_rows in sorted({r for r in (1, 16, 17, L) if r <= L}):
        band = _Band(shape=(B * L, W), dtype=dt)
        ops.mha(qkv_dev, band.t, B, L, HEADS, causal, q_rows=q_rows)
        torch.cuda.synchronize()
        assert band.intact()
        got = band.cpu().view(B, L, W)
        assert _same(got[:, :q_rows], want.view(B, L, W)[:, :q_rows]), q_rows
        assert _same(got[:, q_rows:], _poison_like(band, got[:, q_rows:])), q_rows


# ==== forward ==============================================================================================================================
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", FWD_LENGTHS)
def test_forward_planted(dt, causal, L):
    """One-hot: out[i] == v[pi(i)] bit for bit from hgr_mha, hgr_mha_stats (stats == (512, 1)) and hgr_mha_rows (rows beyond q_rows
    untouched).  Uniform at score -512: the mean of the allowed V rows within one rounding - an unmasked padding or future key would
    score 0 and take the softmax."""
    pl = H.plant_onehot(B, L, HEADS, causal, dt)
    qkv = _in(pl["qkv"])
    out, _ = _forward(qkv, B, L, HEADS, causal, dt)
    assert _same(out, pl["out"]), int((out.double() != pl["out"].double()).sum())
    out, st = _forward(qkv, B, L, HEADS, causal, dt, stats=True)
    assert _same(out, pl["out"])
    assert bool((st[..., 0] == 512).all()) and bool((st[..., 1] == 1).all())
    _leading_rows(qkv, pl["out"], L, causal, dt)
    un = H.plant_uniform(B, L, HEADS, causal, dt)
    out, st = _forward(_in(un["qkv"]), B, L, HEADS, causal, dt, stats=True)
    H.within(out, un["ref"], un["bound"], "uniform")
    assert _same(_forward(_in(un["qkv"]), B, L, HEADS, causal, dt)[0], out)
    _leading_rows(_in(un["qkv"]), out, L, causal, dt)
    n = torch.arange(1, L + 1, dtype=torch.float64) if causal else torch.full((L,), float(L), dtype=torch.float64)
    assert bool((st[..., 0] == -512).all())
    assert bool(((st[..., 1].double() - 1 / n).abs() <= 2.0 ** -23 / n).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", FWD_LENGTHS)
def test_forward_random_within_bound(dt, causal, L):
    """N(0, 1) and N(0, 9) inputs (at scale 3 the softmax is peaked, the scores reach +-30) against float64 within the bound, and the
    statistics hgr_mha_stats writes: the maximum within 2^-20 (|q| . |k|) / 8, 1 / sum within 2^-14 relative."""
    for scale in (1.0, 3.0):
        qkv16 = H.rand_qkv(B, L, HEADS, scale, dt, 100 * L + int(scale))
        f = H.ref_forward(qkv16, B, L, HEADS, causal)
        qkv = _in(qkv16)
        out, st = _forward(qkv, B, L, HEADS, causal, dt, stats=True)
        plain, _ = _forward(qkv, B, L, HEADS, causal, dt)
        assert _same(out, plain)
        _report("forward", dt, H.within(H.split_heads(out, B, L, HEADS), f["out"], H.bound_forward(f, dt), (L, scale)))
        assert bool(((st[..., 0].double() - f["mx"]).abs() <= f["mx_bound"]).all()), (L, scale, "max")
        assert bool(((st[..., 1].double() - f["inv"]).abs() <= H.F32_ALLOW * f["inv"]).all()), (L, scale, "1 / sum")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L,causal", [(33, True), (257, False)])
def test_forward_one_sequence_twelve_heads(dt, L, causal):
    b, heads = 1, 12
    pl = H.plant_onehot(b, L, heads, causal, dt)
    out, st = _forward(_in(pl["qkv"]), b, L, heads, causal, dt, stats=True)
    assert _same(out, pl["out"]) and bool((st[..., 0] == 512).all()) and bool((st[..., 1] == 1).all())
    qkv16 = H.rand_qkv(b, L, heads, 3.0, dt, 7 * L)
    f = H.ref_forward(qkv16, b, L, heads, causal)
    out, _ = _forward(_in(qkv16), b, L, heads, causal, dt)
    _report("forward", dt, H.within(H.split_heads(out, b, L, heads), f["out"], H.bound_forward(f, dt), L))


# ==== backward =============================================================================================================================
def _backward_variants(qkv16, o16, do16, b, L, heads, causal, dt):
    """hgr_mha_bwd, hgr_mha_bwd_stats (L <= 288: statistics from the forward on the device) and hgr_mha_bwd_colsum with and without
    them, each into fresh poisoned outputs; yields (name, dqkv on the CPU).  colsum_part is checked here against the float64 column
    sums of the rows as rounded (the tolerance of test_gpu_train_kernels.py::test_mha_bwd_vs_autograd)."""
    w = heads * 64
    qkv, o, do = _in(qkv16), _in(o16), _in(do16)
    st = None
    if L <= 288:
        stb = _Band(shape=(b * heads * L, 2), dtype=F32, poison=_POISON_IN)        # an INPUT of the backward
        scratch = _Band(shape=(b * L, w), dtype=dt)
        ops.mha(qkv, scratch.t, b, L, heads, causal, stats=stb.t)
        torch.cuda.synchronize()
        assert stb.intact() and _written(stb)
        st = stb.t
    for name, stats, colsum in (("bwd", None, False), ("bwd_stats", st, False), ("bwd_colsum", None, True), ("bwd_colsum_stats", st, True)):
        if "stats" in name and st is None:
            continue
        dqkv = _Band(shape=(b * L, 3 * w), dtype=dt)
        part = _Band(shape=(b, 3 * w), dtype=F32) if colsum else None
        ops.mha_bwd(qkv, o, do, dqkv.t, b, L, heads, causal, stats=stats, colsum_part=part.t if colsum else None)
        torch.cuda.synchronize()
        assert dqkv.intact() and _written(dqkv), (name, "dqkv")
        got = dqkv.cpu()
        if colsum:
            assert part.intact() and _written(part), (name, "colsum_part")
            rows = got.double().view(b, L, 3 * w)
            ref = rows.sum(dim=1)
            assert float((part.cpu().double() - ref).abs().max()) <= 1e-6 * float(rows.abs().sum(dim=1).max()) + 1e-7, name
        yield name, got


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", BWD_LENGTHS)
def test_backward_planted(dt, causal, L):
    """One-hot P, O = v[pi], integer dO: dQ == dK == 0 and dV[j] == the exact sum of dO[i] over pi(i) = j, rounded once."""
    pl = H.plant_onehot(B, L, HEADS, causal, dt)
    do16, want = H.onehot_backward(pl, B, L, HEADS, dt)
    for name, got in _backward_variants(pl["qkv"], pl["out"], do16, B, L, HEADS, causal, dt):
        assert H.same_values(got, want), (name, int((got.double() != want.double()).sum()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", BWD_LENGTHS)
def test_backward_random_within_bound(dt, causal, L):
    """Against the float64 restatement of the kernel's own formula (D from the ROUNDED O it is given when L > 32, from P * dP below)."""
    for scale in (1.0, 3.0):
        qkv16 = H.rand_qkv(B, L, HEADS, scale, dt, 200 * L + int(scale))
        do16 = H.rand_rows(B, L, HEADS, 0.5, dt, 201 * L + int(scale))
        o16 = H.merge_heads(H.ref_forward(qkv16, B, L, HEADS, causal)["out"]).to(dt)
        ref, bound = H.ref_backward(qkv16, o16, do16, B, L, HEADS, causal, dt)
        for name, got in _backward_variants(qkv16, o16, do16, B, L, HEADS, causal, dt):
            for n, worst in zip(("dQ", "dK", "dV"), H.check_backward(got, ref, bound, B, L, HEADS, (name, L, scale))):
                _report("backward_" + n, dt, worst)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L,causal", [(31, True), (257, False)])
def test_backward_one_sequence_twelve_heads(dt, L, causal):
    b, heads = 1, 12
    pl = H.plant_onehot(b, L, heads, causal, dt)
    do16, want = H.onehot_backward(pl, b, L, heads, dt)
    for name, got in _backward_variants(pl["qkv"], pl["out"], do16, b, L, heads, causal, dt):
        assert H.same_values(got, want), name


# ==== attnpool_attend ======================================================================================================================
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", POOL_LENGTHS)
def test_attnpool_attend(dt, L):
    def run(q, k, v):
        out = _Band(shape=(B, W), dtype=dt)
        ops.attnpool_attend(_in(q), _in(k), _in(v), out.t, B, L, HEADS)
        torch.cuda.synchronize()
        assert out.intact() and _written(out)
        return out.cpu()

    for uniform in (False, True):
        pp = H.plant_pool(B, L, HEADS, dt, uniform)
        got = run(pp["q"], pp["k"], pp["v"]).double()
        assert bool(torch.isfinite(got).all()) and bool(((got - pp["ref"]).abs() <= pp["bound"]).all()), ("uniform" if uniform else "one-hot")
    for scale in (1.0, 3.0):
        q = H.rand_rows(B, 1, HEADS, scale, F32, 300 * L + int(scale))
        k, v = H.rand_rows(B, L, HEADS, scale, dt, 301 * L + int(scale)), H.rand_rows(B, L, HEADS, scale, dt, 302 * L + int(scale))
        ref, bound = H.ref_pool(q, k, v, B, L, HEADS, dt)
        _report("attnpool_attend", dt, H.within(run(q, k, v), ref, bound, (L, scale)))


# ==== refusals =============================================================================================================================
def _refused(call, out, name=None):
    with pytest.raises(HgrError) as err:
        call()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote"
    assert name is None or name in str(err.value), str(err.value)


@pytest.mark.parametrize("dt", DTS)
def test_refusals_launch_nothing(dt):
    b, heads, w = 1, 1, 64
    z = lambda rows, cols: torch.zeros(rows, cols, dtype=dt, device=DEV)
    L = 321
    dqkv = torch.full((b * L, 3 * w), 7.0, dtype=dt, device=DEV)
    _refused(lambda: ops.mha_bwd(z(b * L, 3 * w), z(b * L, w), z(b * L, w), dqkv, b, L, heads, False), dqkv, "hgr_mha_bwd")
    L = 257
    out = torch.full((b, w), 7.0, dtype=dt, device=DEV)
    _refused(lambda: ops.attnpool_attend(torch.zeros(b, w, device=DEV), z(b * L, w), z(b * L, w), out, b, L, heads), out, "hgr_attnpool_attend")
    L = 16
    out = torch.full((b * L, w), 7.0, dtype=dt, device=DEV)
    _refused(lambda: ops.mha(z(b * L, 3 * w), out, b, L, heads, True, q_rows=L + 1), out, "hgr_mha_rows")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", [16, 65])
def test_backward_refuses_misaligned_operands(dt, L):
    """A qkv, out, dout or dqkv view that starts one element past a 16-byte boundary is refused by all three entry points before anything
    is launched (the kernels load 16 bytes at a time)."""
    b, heads, w = 2, 2, 128

    def views(rows, cols, fill):
        buf = torch.full((rows * cols + 8,), fill, dtype=dt, device=DEV)
        return buf[:rows * cols].view(rows, cols), buf[1:rows * cols + 1].view(rows, cols)

    qkv, qkv1 = views(b * L, 3 * w, 0.0)
    o, o1 = views(b * L, w, 0.0)
    do, do1 = views(b * L, w, 0.0)
    dqkv, dqkv1 = views(b * L, 3 * w, 7.0)
    st = torch.zeros(b, heads, L, 2, device=DEV)
    part = torch.full((b, 3 * w), 7.0, device=DEV)
    for args in ((qkv1, o, do, dqkv), (qkv, o1, do, dqkv), (qkv, o, do1, dqkv), (qkv, o, do, dqkv1)):
        assert all(a.is_contiguous() for a in args) and sum(a.data_ptr() % 16 != 0 for a in args) == 1
        for name, kw in (("hgr_mha_bwd", {}), ("hgr_mha_bwd_stats", dict(stats=st)), ("hgr_mha_bwd_colsum", dict(colsum_part=part))):
            _refused(lambda: ops.mha_bwd(*args, b, L, heads, False, **kw), args[3], name)
            assert bool((part == 7.0).all())
