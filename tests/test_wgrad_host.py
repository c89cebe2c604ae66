"""Host: the weight-gradient plan (hgr_net_amd.wgrad.plan), the route predicate and the 3x3 error.  No device work: the expected
values were computed from the slice formulas the training step, the ModifiedResNet tower and the FREE step each carried before
wgrad.py held the only copy (HGR_TN_TILE unset: the library picks the tile of the linear product)."""
import os

import pytest
import torch

from hgr_net_amd import wgrad
from hgr_net_amd._lib import HgrError

TN = {  # (cout, k, m) -> (slices, kc)
    (2304, 768, 12800): (9, 1472), (768, 768, 12800): (25, 512), (3072, 768, 12800): (7, 1856), (768, 3072, 12800): (7, 1856),
    (3072, 1024, 16448): (5, 3328), (1024, 1024, 16448): (16, 1088), (1024, 4096, 16448): (4, 4160),
    (64, 64, 802816): (502, 1600), (256, 64, 802816): (256, 3136), (2048, 512, 12544): (16, 832),
    (136, 72, 300): (1, 320), (136, 72, 1100): (2, 576), (128, 128, 2048): (4, 512), (264, 40, 2100): (4, 576),
}
TN_CONV = {(64, 576, 802816): (102, 7872), (512, 4608, 12544): (7, 1792), (16, 72, 720): (1, 768), (64, 576, 3136): (6, 576)}
NT = {  # (cout, k, m) -> (mp, slices, kc); kc None: one hgr_gemm_nt launch with EPI_ACCUM
    (1024, 588, 16448): (16448, 22, 768), (768, 588, 12850): (12864, 29, 448), (136, 588, 300): (320, 5, 64),
    (264, 260, 1000): (1024, 8, 128), (40, 20, 100): (128, 2, 64), (1024, 1100, 100): (128, 1, None),
}


@pytest.fixture(autouse=True)
def _library_picks_the_tile():
    assert "HGR_TN_TILE" not in os.environ


@pytest.mark.parametrize("shape", TN, ids=str)
def test_plan_tn(shape):
    assert wgrad.plan(*shape) == ("tn",) + TN[shape] + (shape[2],)


@pytest.mark.parametrize("shape", TN_CONV, ids=str)
def test_plan_tn_conv(shape):
    assert wgrad.plan(*shape, conv=True) == ("tn_conv",) + TN_CONV[shape] + (shape[2],)


@pytest.mark.parametrize("shape", NT, ids=str)
def test_plan_nt(shape):
    mp, slices, kc = NT[shape]
    assert wgrad.plan(*shape, tn_ok=False) == ("nt", slices, kc, mp)


def test_plan_covers_every_row():
    for table, kw in ((TN, {}), (TN_CONV, dict(conv=True)), (NT, dict(tn_ok=False))):
        for cout, k, m in table:
            p = wgrad.plan(cout, k, m, **kw)
            assert p.mp >= m and p.mp - m < 64
            if p.kc is not None:
                assert p.kc % 64 == 0 and (p.slices - 1) * p.kc < p.mp <= p.slices * p.kc


def test_no_transposing_3x3_plan():
    with pytest.raises(HgrError, match="3x3"):
        wgrad.plan(16, 72, 720, conv=True, tn_ok=False)


def test_route_predicate():
    ok = dict(cout=136, k=72, dy_stride=(144, 1), x_stride=(80, 1), dy_ptr=4096, x_ptr=4096 + 16)
    assert wgrad.tn_blocker(**ok) is None
    assert wgrad.tn_blocker(**ok, conv=True, x_contiguous=True) is None
    for change, word in ((dict(k=588), "multiples of 8"), (dict(cout=20), "multiples of 8"),
                         (dict(dy_stride=(148, 1)), "row strides"), (dict(x_stride=(76, 1)), "row strides"),
                         (dict(dy_stride=(144, 2)), "column strides"), (dict(x_stride=(1, 80)), "column strides"),
                         (dict(dy_ptr=4096 + 8), "16-byte"), (dict(x_ptr=4096 + 2), "16-byte")):
        assert word in wgrad.tn_blocker(**{**ok, **change}), change
    assert wgrad.tn_blocker(**ok, conv=False, x_contiguous=False) is None        # a Linear / 1x1 reads X at any row stride
    assert "contiguous" in wgrad.tn_blocker(**ok, conv=True, x_contiguous=False)


@pytest.mark.parametrize("what", ["pointer", "row stride", "contiguous"])
def test_unaligned_3x3_raises_before_any_launch(what):
    """b, h, c, cout = 1, 4, 8, 16 on host tensors: `add` must name the failed condition and stop before it touches a buffer."""
    b, h, c, cout = 1, 4, 8, 16
    m = b * h * h
    dy = torch.zeros(m, cout, dtype=torch.bfloat16)
    x = torch.zeros(m, c, dtype=torch.bfloat16)
    if what == "pointer":
        x = torch.zeros(m * c + 1, dtype=torch.bfloat16)[1:].view(m, c)
        word = "16-byte"
    elif what == "row stride":
        dy = torch.zeros(m, cout + 4, dtype=torch.bfloat16)[:, :cout]
        word = "row strides"
    else:
        x = torch.zeros(m, 2 * c, dtype=torch.bfloat16)[:, :c]
        word = "contiguous"
    gw = torch.zeros(cout, 9 * c)

    def scratch(n):
        raise AssertionError("no scratch before the route is known")

    wg = wgrad.WeightGrad(torch.bfloat16, "cpu", scratch)
    with pytest.raises(HgrError, match=word):
        wg.add(gw, dy, x, conv=(b, h, c))
    assert not wg._bufs and not gw.any()
