"""GPU: the residual producer on 320 x 256 tiles (hgr_gemm_nt_res_stats_wide, csrc/hgr_gemm_wide.hip) against hgr_gemm_nt_res_stats -
the same bits in the pair, the slot statistics and the guard word - and its route in the ViT tower (clip/model.py: PROJ_WIDE)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops, synth
from hgr_net_amd.clip.model import build_model

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]
SENTINEL_H, SENTINEL_L = 0x5A5A, 0xA5


def _pair(x, dt):
    """Reference encoder of the residual pair (include/hgr.h), on the bits of x: t = bits(x) + half an ulp of the MFMA type; hi = t with
    the S dropped mantissa bits cleared (S = 13 for f16, 16 for bf16), q = the next 8 bits of t (128 below the f16 normal range)."""
    s_ = 13 if dt == torch.float16 else 16
    t = x.float().contiguous().view(torch.int32) + (1 << (s_ - 1))
    q = (t >> (s_ - 8)) & 255
    if dt == torch.float16:
        q = torch.where((t & 0x7FFFFFFF) < 0x38800000, torch.full_like(q, 128), q)
    hi = (t & ~((1 << s_) - 1)).view(torch.float32).to(dt)
    return hi, q.to(torch.uint8)


def _operands(dt, m, n, k, lda=None, seed=0, xscale=2.0):
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + m + n + k)
    rnd = lambda shape, scale=1.0: scale * torch.randn(shape, generator=g, device=DEV)
    lda = lda or k
    a = rnd((m, lda)).to(dt)[:, :k]
    w = rnd((n, k), 0.1).to(dt)
    return a, w, rnd((n,)), rnd((m, n), xscale)


def _strided_pair(x0, dt, ldx):
    """The pair of x0 as views of width n into sentinel-filled buffers of row stride ldx."""
    m, n = x0.shape
    bh = torch.full((m, ldx), SENTINEL_H, dtype=torch.int16, device=DEV).view(dt)
    bl = torch.full((m, ldx), SENTINEL_L, dtype=torch.uint8, device=DEV)
    h, l = _pair(x0, dt)
    bh[:, :n] = h
    bl[:, :n] = l
    return bh, bl


def _both(a, w, bias, x0, dt, ldx=None, flag=False):
    """(xh, xl, stats, flag word) of hgr_gemm_nt_res_stats and of the wide entry on the same operands; the full buffers are returned."""
    m, n = x0.shape
    out = []
    for fn in (ops.gemm_nt_res_stats, ops.gemm_nt_res_stats_wide):
        bh, bl = _strided_pair(x0, dt, ldx or n)
        stats = torch.full((m, n // 64, 2), -1.0, dtype=torch.float32, device=DEV)
        fl = torch.zeros(1, dtype=torch.int32, device=DEV) if flag else None
        fn(a, w, bh[:, :n], bl[:, :n], bias, stats, flag=fl)
        out.append((bh, bl, stats, fl))
    return out


def _assert_same(ref, got):
    assert torch.equal(got[0].view(torch.int16), ref[0].view(torch.int16)), int((got[0].view(torch.int16) != ref[0].view(torch.int16)).sum())
    assert torch.equal(got[1], ref[1]), int((got[1] != ref[1]).sum())
    assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32)), int((got[2].view(torch.int32) != ref[2].view(torch.int32)).sum())
    if ref[3] is not None:
        assert torch.equal(got[3], ref[3]), (int(got[3]), int(ref[3]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("m,n,k,lda,ldx", [(320, 256, 256, None, None),       # one tile, the minimum K-tile count
                                           (640, 768, 384, None, None),       # several tiles per XCD, 6 K-tiles
                                           (320, 256, 3072, None, None),      # the real K: 48 K-tiles, steady-state loop
                                           (960, 512, 256, 264, 520)])        # strided rows
def test_wide_equals_res_stats_bits(dt, m, n, k, lda, ldx):
    """Same operand roles, same K order from a zero accumulator, the producer epilogue expression for expression: pair, slot statistics
    and the (untouched) guard word must be the bits of hgr_gemm_nt_res_stats.  With ldx > n the bytes between row ends keep their
    sentinel."""
    assert ops.gemm_nt_res_stats_wide_ok(m, n, k, lda or k, k, ldx or n, dt)
    a, w, bias, x0 = _operands(dt, m, n, k, lda)
    assert a.stride(0) == (lda or k)
    ref, got = _both(a, w, bias, x0, dt, ldx, flag=True)
    _assert_same(ref, got)
    assert int(got[3]) == 0
    assert not torch.equal(got[0][:, :n].view(torch.int16), _pair(x0, dt)[0].view(torch.int16))       # it did write
    assert bool((got[2][..., 1] >= 0.0).all())                                                         # no slot kept its -1 fill
    if ldx:
        assert bool((got[0].view(torch.int16)[:, n:] == SENTINEL_H).all())
        assert bool((got[1][:, n:] == SENTINEL_L).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", ["in_range", "one_slot", "inf"])
def test_wide_range_guard(dt, case):
    """The guard word behaves as in hgr_gemm_nt_res_stats_guard: 0 while every slot's sum of squares stays below LN_GUARD_SUMSQ, the
    largest offending bit pattern when one slot exceeds it, inf's pattern with an inf in the stream."""
    m, n, k = 320, 256, 256
    a, w, bias, x0 = _operands(dt, m, n, k, seed=3)
    if case == "one_slot":
        x0[123, 64:128] = 3000.0                      # 64 x 3000^2 = 5.76e8 > 16384^2 = 2.68e8, every element far inside the f16 range
    if case == "inf":
        x0[200, 130] = float("inf")
    ref, got = _both(a, w, bias, x0, dt, flag=True)
    _assert_same(ref, got)
    word = int(got[3])
    if case == "in_range":
        assert word == 0
    else:
        want = got[2][..., 1].contiguous().view(torch.int32).max()
        assert word == int(want) and word > torch.tensor(ops.LN_GUARD_SUMSQ).view(torch.int32).item()
    if case == "inf":
        assert word == 0x7F800000
    # without a flag the same call leaves pair and statistics as they were with it
    bh, bl = _strided_pair(x0, dt, n)
    stats = torch.empty_like(got[2])
    ops.gemm_nt_res_stats_wide(a, w, bh, bl, bias, stats)
    _assert_same((got[0], got[1], got[2], None), (bh, bl, stats, None))


# zeros of both signs, fp32 denormals, the f16 subnormal range and its upper edge, mantissa carries into the next binade, the largest
# f16, negative twins: the values that separate the forms of the pair split
SPECIAL = [0.0, -0.0, 1e-40, -1e-40, 1e-8, -1e-8, 5.9e-8, 2.98e-8, 6e-5, -6e-5, 6.2e-5, 6.103515625e-05, 6.1035e-05, -6.1035e-05, 3.0517578125e-05,
           1.9999, -1.9999, 2047.9999, -2047.9999, 65000.0, -65000.0, 0.999755859375, 0.99987793, 1.0, -1.0, 3.14159, 1e-3, -1e-3, 0.33333334, 1024.5,
           7.62939453125e-06, -7.62939453125e-06]


@pytest.mark.parametrize("dt", DTS)
def test_wide_pair_corner_cases(dt):
    """With A = 0 the product vanishes: the new pair must be the reference encoder's split of (old value + bias), in the kernel's
    association (product + bias) + old value, on the special values above with their low mantissa bits walked row by row."""
    m, n, k = 320, 256, 256
    sp = torch.tensor(SPECIAL, dtype=torch.float32)
    x0 = sp.repeat((m * n + sp.numel() - 1) // sp.numel())[: m * n].view(m, n).contiguous().to(DEV)
    x0 = x0 * (1.0 + 2.0 ** -12 * (torch.arange(m, device=DEV) % 7).float()[:, None])
    xh0, xl0 = _pair(x0, dt)
    old = ops.pair_value(xh0, xl0)
    a = torch.zeros(m, k, dtype=dt, device=DEV)
    w = _operands(dt, m, n, k, seed=5)[1]
    for bias_val in (0.0, 2.0 ** -20, -3.0e-5):
        bias = torch.full((n,), bias_val, dtype=torch.float32, device=DEV)
        xh, xl = xh0.clone(), xl0.clone()
        stats = torch.empty(m, n // 64, 2, dtype=torch.float32, device=DEV)
        ops.gemm_nt_res_stats_wide(a, w, xh, xl, bias, stats)
        want = (0.0 + bias[None, :]) + old
        rh, rl = _pair(want, dt)
        assert torch.equal(xh.view(torch.int16), rh.view(torch.int16)), (bias_val, int((xh != rh).sum()))
        assert torch.equal(xl, rl), (bias_val, int((xl != rl).sum()))
        assert torch.isfinite(ops.pair_value(xh, xl)).all()
        xs = want.double().view(m, n // 64, 64)
        assert torch.allclose(stats[..., 0].double(), xs.sum(-1), rtol=1e-5, atol=1e-2)
        assert torch.allclose(stats[..., 1].double(), (xs * xs).sum(-1), rtol=1e-5, atol=1e2)


def test_wide_route_in_the_vit_tower_gives_the_same_features():
    """ViT-B/32 at batch 32 (1 600 rows = 5 x 3 tiles): encode_image with the c_proj route forced (PROJ_WIDE = 2) and off (0).  The
    features must be the same bits, and the wide entry must have run in the forced arm (once per block that carries every token)
    and not in the other."""
    from hgr_net_amd.clip import model as clip_model
    cfg = synth.CLIP_CONFIGS["ViT-B/32"]
    m = build_model(synth.clip_state_dict(cfg, 0)).to(DEV)
    img = synth.images(32, cfg["image_resolution"], 77).to(DEV)
    prev = clip_model.PROJ_WIDE
    try:
        clip_model.PROJ_WIDE = 0
        c0 = ops.WIDE_CALLS[0]
        off = m.encode_image(img).clone()
        assert ops.WIDE_CALLS[0] == c0
        clip_model.PROJ_WIDE = 2
        on = m.encode_image(img).clone()
        ran = ops.WIDE_CALLS[0] - c0
    finally:
        clip_model.PROJ_WIDE = prev
    layers = cfg["vision_layers"]
    assert ran in (layers - 1, layers), ran                  # the last block works on the class tokens alone (CLS_LAST)
    assert torch.isfinite(on).all() and torch.equal(on, off)
