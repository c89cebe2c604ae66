"""GPU: the ModifiedResNet convolution and pool kernels, one case per dispatch route and edge (hgr_conv3x3_nhwc and
hgr_conv3x3_nhwc_plain on the 128 x 128, tall 256 x 64 and 256 x 256 implicit GEMMs, gemm_nt_duo with the implicit loader, the direct
halo-tile kernels for C = 32 and C = Cout = 64; hgr_conv3x3_pool2_nhwc; hgr_stem_conv1) and the streaming kernels around them, against
planted inputs whose result is exact and against float64 within an element-wise bound made from the arithmetic -
tests/test_conv_host.py holds the builders, the references, the bounds and the case tables, tests them on the CPU and pins every case's
route.

Every operand lives in guard bands of a NaN pattern (tests/test_gpu_row_kernels.py: inputs one pattern, outputs another): a read outside
an input reaches the output, a write outside an output's view changes bits that are compared afterwards, an output element that was not
written is still a NaN.  After each call: the bands, then every element written, then the comparison."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops
from hgr_net_amd._lib import HgrError

import test_conv_host as H
from test_attention_host import BF16, DTS, half_ulp16, same_values, within
from test_gpu_attention import _written
from test_gpu_row_kernels import _Band, _G, _in, _POISON_IN, _same

DEV = "cuda"
F32 = torch.float32


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """Nothing more is launched on a device that has reported an error."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                                    # noqa: BLE001
        pytest.exit("device error, stopping: %s" % e, returncode=3)


def _tag(dt):
    return "bf16" if dt == BF16 else "f16"


def _report(kernel, dt, worst):
    print("RATIO %s %s %.3f" % (kernel, _tag(dt), worst))


def _conv(cs, x16, w16, bias, dt, lead=_G):
    """One call of the case's entry point into a fresh poisoned output; the bands and `every element written` are checked; out on the CPU."""
    ho, wo = H.out_hw(cs.H, cs.W, cs.stride)
    out = _Band(shape=(cs.B * ho * wo, cs.Cout), dtype=dt, lead=lead)
    x, w = _in(x16.reshape(-1, cs.C)), _in(w16)
    prev = ops.gemm_set_tile(cs.tile) if cs.tile else None
    try:
        if cs.relu:
            ops.conv3x3_nhwc(x, w, _in(bias), out.t, cs.B, cs.H, cs.W, cs.C, cs.stride)
        else:
            ops.conv3x3_plain(x, w, out.t, cs.B, cs.H, cs.W, cs.C)
    finally:
        if prev is not None:
            ops.gemm_set_tile(prev)
    torch.cuda.synchronize()
    assert out.intact(), "wrote outside its view"
    assert _written(out), "an output element was not written"
    return out.cpu()


def _planted(cs, dt, lead=_G):
    for kind in H.kinds_of(cs):
        x, w, bias, want = H.planted_expect(cs, kind, dt)
        got = _conv(cs, x, w, bias, dt, lead)
        assert same_values(got, want), (kind, int((got.double() != want.double()).sum()), "elements differ")


def _random(cs, dt):
    rows = H.sample_rows(cs) if cs in H.SAMPLED else None
    for scale in (1.0, 3.0):
        x, w, bias = H.rand_inputs(cs, scale, dt)
        got = _conv(cs, x, H.pack_w(w, dt), bias, dt)
        ref, bound = H.ref_random(cs, x, w, bias, dt, rows)
        _report(cs.route, dt, within(got if rows is None else got[rows], ref, bound, (H.case_id(cs), scale)))


# ==== the 3 x 3 convolutions, one case per route and edge =====================================================================================
@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("cs", H.CONV_CASES, ids=H.case_id)
def test_conv3x3_planted(cs, dt):
    """Sparse, dense and (with a bias) tie inputs: the exact sum rounded once, bit for bit; for a plain case autograd's dX of F.conv2d."""
    _planted(cs, dt)


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("cs", [c for c in H.CONV_CASES if c.rnd], ids=H.case_id)
def test_conv3x3_random_within_bound(cs, dt):
    """N(0, 1) and N(0, 9) activations against float64 within half_ulp16 + (9C + 1) 2^-23 (sum |w| |x| + |bias|); the two large
    gemm_nt_duo cases on a row sample (first and last image, both rows at every 256-row tile edge, 4096 random rows)."""
    _random(cs, dt)


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("cs,off", H.MISALIGNED_OUT_CASES, ids=lambda v: H.case_id(v) if isinstance(v, H.Case) else "off%d" % v)
def test_conv3x3_output_8_byte_aligned_only(cs, off, dt):
    """An output view 8 but not 16 bytes aligned keeps C = 32 off the direct kernel (tests/test_conv_host.py pins the plan) and is exact."""
    _planted(cs, dt, lead=_G + off // 2)


# ==== conv + ReLU + 2 x 2 average pool =======================================================================================================
@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("cs", H.POOL_CASES, ids=H.case_id)
def test_conv3x3_pool2(cs, dt):
    """The planted conv output rounded to 16 bits, then the fp32 average of four, rounded; and bit-equal to hgr_conv3x3_nhwc followed by
    hgr_avgpool2_nhwc on the device.  The output band ends with the last pooled row: a row written beyond H / 2 breaks it."""
    hp, wp = cs.H // 2, cs.W // 2
    for kind in H.kinds_of(cs):
        x, w, bias, want = H.planted_expect(cs, kind, dt)
        xd, wd, bd = _in(x.reshape(-1, 32)), _in(w), _in(bias)
        out = _Band(shape=(cs.B * hp * wp, cs.Cout), dtype=dt)
        ops.conv3x3_pool2_nhwc(xd, wd, bd, out.t, cs.B, cs.H, cs.W, 32)
        torch.cuda.synchronize()
        assert out.intact() and _written(out)
        got = out.cpu()
        assert same_values(got, H.pool_expect(want, cs.B, cs.H, cs.W, cs.Cout)), kind
        full = _Band(shape=(cs.B * cs.H * cs.W, cs.Cout), dtype=dt)
        ops.conv3x3_nhwc(xd, wd, bd, full.t, cs.B, cs.H, cs.W, 32)
        two = _Band(shape=(cs.B * hp * wp, cs.Cout), dtype=dt)
        ops.avgpool2_nhwc(full.t, two.t, cs.B, cs.H, cs.W, cs.Cout)
        torch.cuda.synchronize()
        assert full.intact() and two.intact() and _same(two.cpu(), got), kind


# ==== stem conv1 ===========================================================================================================================
def _stem(img, w16, bias, b, r, cout, dt):
    out = _Band(shape=(b * (r // 2) ** 2, cout), dtype=dt)
    ops.stem_conv1(_in(img.reshape(-1)).view(b, 3, r, r), _in(w16), _in(bias), out.t)
    torch.cuda.synchronize()
    assert out.intact() and _written(out)
    return out.cpu()


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("b,r,cout", H.STEM_CASES)
def test_stem_conv1(b, r, cout, dt):
    """Integer images and ternary weights in the 27 live columns: exact against F.conv2d(stride 2, pad 1).  The kernel reads weight
    columns 0 .. 31 only, and columns 27 .. 31 multiply a LIVE pixel (tap 0, channel 0): zeros there are a requirement of the layout
    (include/hgr.h and the entry point's comment), so only columns >= 32 may hold anything - asserted with NaNs there.  What ones in
    columns 27 .. 31 do is printed, not asserted (it is no contract): on the MI355X every case gave other bits."""
    img, w, bias, s = H.stem_inputs(b, r, cout, 40 + r)
    w16 = H.pack_w(w, dt, 64)
    want = H.expect(s, bias, True, dt)
    got = _stem(img, w16, bias, b, r, cout, dt)
    assert same_values(got, want), int((got.double() != want.double()).sum())
    beyond = w16.clone()
    beyond[:, 32:] = float("nan")
    assert _same(_stem(img, beyond, bias, b, r, cout, dt), got)
    tail = w16.clone()
    tail[:, 27:32] = 1.0
    print("STEM_COLUMNS_27_31 R=%d Cout=%d %s same_bits=%s" % (r, cout, _tag(dt), _same(_stem(img, tail, bias, b, r, cout, dt), got)))
    if (b, r, cout) == H.STEM_RANDOM:
        for scale in (1.0, 3.0):
            cs = H._c(b, r, r, 3, cout, 2, True, "stem")
            n = b * 3 * r * r
            im = torch.from_numpy((scale * H.synth.normal(77 + int(scale), "stem.x", n)).astype("float32")).view(b, 3, r, r)
            wr = torch.from_numpy((0.3 * H.synth.normal(78, "stem.w", cout * 27)).astype("float32")).view(cout, 27).to(dt)
            br = torch.from_numpy((0.2 * H.synth.normal(79, "stem.b", cout)).astype("float32"))
            ref, bound = H.ref_random(cs, im.to(dt).permute(0, 2, 3, 1), wr, br, dt)      # the kernel rounds the image to 16 bits first
            _report("stem_conv1", dt, within(_stem(im, H.pack_w(wr, dt, 64), br, b, r, cout, dt), ref, bound, scale))


# ==== streaming kernels =====================================================================================================================
@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("r", H.STEM_IM2COL_R)
def test_stem_im2col(r, dt):
    b = 2
    img = H.plant_x(b, r, r, 3, 300 + r, -128, 128)                            # NHWC integers, exact in both types
    ho = (r - 1) // 2 + 1
    out = _Band(shape=(b * ho * ho, 64), dtype=dt)
    ops.stem_im2col(_in(img.permute(0, 3, 1, 2).reshape(-1)).view(b, 3, r, r), out.t)
    torch.cuda.synchronize()
    assert out.intact() and _written(out)
    got = out.cpu()
    assert same_values(got[:, :27], H.im2col(img, 2).to(dt)) and bool((got[:, 27:] == 0).all())


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("b,h,w,c", H.AVGPOOL_SHAPES)
def test_avgpool2_forward_and_backward(b, h, w, c, dt):
    x, fwd, dy, dx = H.avgpool_inputs(b, h, w, c, dt)
    out = _Band(shape=fwd.shape, dtype=dt)
    ops.avgpool2_nhwc(_in(x), out.t, b, h, w, c)
    back = _Band(shape=dx.shape, dtype=dt)
    ops.avgpool2_bwd_nhwc(_in(dy), back.t, b, h, w, c)
    torch.cuda.synchronize()
    assert out.intact() and _written(out) and same_values(out.cpu(), fwd)
    assert back.intact() and _written(back) and same_values(back.cpu(), dx)


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("b,s,c", H.ATTNPOOL_SHAPES)
def test_attnpool_tokens_forward_and_backward(b, s, c, dt):
    g = s * s
    x = H.plant_x(b, g, 1, c, 500 + s, -8, 8).reshape(b * g, c).to(dt)
    pos = 0.25 * H.plant_x(1, g + 1, 1, c, 501 + s, -16, 16).reshape(g + 1, c)
    tok = _Band(shape=(b * (g + 1), c), dtype=dt)
    ops.attnpool_tokens(_in(x), _in(pos), tok.t, b, s, c)
    dtok = (0.125 * H.plant_x(b, g + 1, 1, c, 502 + s, -64, 64)).reshape(b * (g + 1), c).to(dt)
    dx = _Band(shape=(b * g, c), dtype=dt)
    ops.attnpool_tokens_bwd(_in(dtok), dx.t, b, g, c)                         # the backward's S is the cell count
    torch.cuda.synchronize()
    assert tok.intact() and _written(tok) and dx.intact() and _written(dx)
    ref, bound = H.attnpool_tokens_ref(x, pos, b, s, c, dt)
    _report("attnpool_tokens", dt, within(tok.cpu(), ref, bound, (b, s, c)))
    ref, bound = H.attnpool_tokens_bwd_ref(dtok, b, g, c, dt)
    _report("attnpool_tokens_bwd", dt, within(dx.cpu(), ref, bound, (b, s, c)))


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("b,h,w", H.IM2COL_T_SHAPES)
def test_im2col3x3_t(b, h, w, dt):
    """Eight-pixel groups that wrap rows and images (W < 8); the padding columns up to ld are written as zeros, those of the INPUT never read."""
    c, m = 8, b * h * w
    ld = (m + 63) // 64 * 64
    x = H.plant_x(b, h, w, c, 600 + m, -128, 128)
    xt = torch.full((c, ld), float("nan"))
    xt[:, :m] = x.reshape(m, c).t()
    out = _Band(shape=(9 * c, ld), dtype=dt)
    ops.im2col3x3_t(_in(xt.to(dt)), out.t, b, h, w)
    torch.cuda.synchronize()
    assert out.intact() and _written(out)
    got = out.cpu()
    assert same_values(got[:, :m], H.im2col(x, 1).t().to(dt)) and bool((got[:, m:] == 0).all())


def _elementwise(n, dt):
    g = torch.Generator(device=DEV).manual_seed(n % 1000)
    a = torch.randn(n, generator=g, device=DEV).to(dt)
    y = torch.randn(n, generator=g, device=DEV).to(dt)
    want = {"relu_bwd16": torch.where(y.float() > 0, a, torch.zeros_like(a)), "add16": (a.float() + y.float()).to(dt)}
    for name, fn in (("relu_bwd16", ops.relu_bwd16), ("add16", ops.add16)):
        first, second = _Band(a, poison=_POISON_IN), _Band(y, poison=_POISON_IN)
        out = _Band(shape=(n,), dtype=dt)
        fn(first.t, second.t, out.t)
        torch.cuda.synchronize()
        assert out.intact() and first.intact() and second.intact() and _same(first.t, a) and _same(second.t, y), name
        assert torch.equal(out.t.view(torch.int16), want[name].view(torch.int16)), (name, "out of place")
        del out
        inplace = _Band(a)
        fn(inplace.t, second.t)
        torch.cuda.synchronize()
        assert inplace.intact() and torch.equal(inplace.t.view(torch.int16), want[name].view(torch.int16)), (name, "in place")
        del inplace, first, second


@pytest.mark.parametrize("dt", DTS, ids=_tag)
@pytest.mark.parametrize("n", H.ELEMWISE_N + [H.ELEMWISE_BIG])
def test_relu_bwd16_and_add16(n, dt):
    """One vector, a ragged last block, and the second pass of the grid-stride loop (more than 32768 x 256 vectors); the large case is
    compared on the device with torch.where and a float add then cast."""
    _elementwise(n, dt)


# ==== refusals =============================================================================================================================
def _refused(call, outs, name):
    with pytest.raises(HgrError) as err:
        call()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs), "a refused call wrote"
    assert name in str(err.value), str(err.value)


@pytest.mark.parametrize("dt", DTS, ids=_tag)
def test_refusals_launch_nothing(dt):
    z = lambda *shape: torch.zeros(*shape, dtype=dt, device=DEV)
    seven = lambda *shape: torch.full(shape, 7.0, dtype=dt, device=DEV)
    b, h, w = 2, 6, 6
    bias = torch.zeros(64, device=DEV)
    out = seven(b * h * w, 16)
    _refused(lambda: ops.conv3x3_nhwc(z(b * h * w, 12), z(16, 128), bias, out, b, h, w, 12), [out], "hgr_conv3x3_nhwc")           # C % 8
    out18 = seven(b * h * w, 18)
    _refused(lambda: ops.conv3x3_nhwc(z(b * h * w, 8), z(18, 128), bias, out18, b, h, w, 8), [out18], "hgr_conv3x3_nhwc")         # Cout % 4
    _refused(lambda: ops.conv3x3_nhwc(z(b * h * w, 16), z(16, 128), bias, out, b, h, w, 16), [out], "hgr_conv3x3_nhwc")           # Kp < 9C
    _refused(lambda: ops.conv3x3_plain(z(b * h * w, 16), z(16, 128), out, b, h, w, 16), [out], "hgr_conv3x3_nhwc")
    x1 = z(b * h * w * 8 + 8)[1:b * h * w * 8 + 1].view(b * h * w, 8)                                                            # 2 bytes off
    assert x1.is_contiguous() and x1.data_ptr() % 16 == 2
    _refused(lambda: ops.conv3x3_nhwc(x1, z(16, 128), bias, out, b, h, w, 8), [out], "hgr_conv3x3_nhwc")
    _refused(lambda: ops.conv3x3_plain(x1, z(16, 128), out, b, h, w, 8), [out], "hgr_conv3x3_nhwc")
    pooled = seven(2 * 3 * 32)
    _refused(lambda: ops.conv3x3_pool2_nhwc(z(5 * 6, 32), z(32, 320), bias, pooled, 1, 5, 6, 32), [pooled], "hgr_conv3x3_pool2_nhwc")   # odd H
    img = lambda r: torch.zeros(1, 3, r, r, device=DEV)
    stem = seven(9, 32)
    _refused(lambda: ops.stem_conv1(img(6), z(32, 64), bias, stem), [stem], "hgr_stem_conv1")                                   # R % 4
    stem56 = seven(16, 56)
    _refused(lambda: ops.stem_conv1(img(8), z(56, 64), bias, stem56), [stem56], "hgr_stem_conv1")                               # Cout = 56
    a, y, o = seven(12), seven(12), seven(12)
    _refused(lambda: ops.relu_bwd16(a, y, o), [a, y, o], "hgr_relu_bwd16")                                                       # n % 8
    _refused(lambda: ops.add16(a, y, o), [a, y, o], "hgr_add16")
    _refused(lambda: ops.relu_bwd16(a, y), [a, y], "hgr_relu_bwd16")
    _refused(lambda: ops.add16(a, y), [a, y], "hgr_add16")
