"""GPU: hgr_vit_patch_embed_ln (pixels -> residual pair + slot statistics in one launch) against the three-launch chain
im2col_patches -> gemm_nt (fp32 out) -> vit_embed_ln_stats called through ops on the same inputs.  The contract is bit equality of all
three outputs: same conversion of the pixels, same MFMA instruction and K order, one copy of the row routine (csrc/hgr_common.h)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hgr_net_amd import ops, synth

DEV = "cuda"
DTS = [torch.bfloat16, torch.float16]
W, P = 768, 32


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((scale * synth.normal(seed, "pe", int(np.prod(shape)))).astype(np.float32).reshape(shape))


_PARAMS = {}


def _params(dt, r):
    """conv1 weight [W, 3 P P] in dt, class / positional embedding, ln_pre gamma / beta: made once per (dtype, resolution), never modified."""
    key = (dt, r)
    if key not in _PARAMS:
        gg = (r // P) ** 2
        _PARAMS[key] = (_rand((W, 3 * P * P), 11, 0.02).to(dt).to(DEV), _rand((W,), 12, 0.5).to(DEV), _rand((gg + 1, W), 13, 0.5).to(DEV),
                        (1.0 + _rand((W,), 14, 0.1)).to(DEV), _rand((W,), 15, 0.1).to(DEV))
    return _PARAMS[key]


def _chain(image, dt):
    """The three launches of the parent path; returns (xh, xl, stats)."""
    b, r = image.shape[0], image.shape[2]
    gg = (r // P) ** 2
    cw, cls, pos, gamma, beta = _params(dt, r)
    patches = torch.empty(b * gg, 3 * P * P, dtype=dt, device=DEV)
    ops.im2col_patches(image, patches, P)
    pe = torch.empty(b * gg, W, dtype=torch.float32, device=DEV)
    ops.gemm_nt(patches, cw, pe)
    rows = b * (gg + 1)
    xh = torch.empty(rows, W, dtype=dt, device=DEV)
    xl = torch.empty(rows, W, dtype=ops.PAIR_LO, device=DEV)
    stats = torch.empty(rows, W // 64, 2, dtype=torch.float32, device=DEV)
    ops.vit_embed_ln_stats(pe, cls, pos, gamma, beta, xh, xl, stats, b, gg)
    return xh, xl, stats


def _one_launch(image, dt, extra_rows=0, fill=None):
    b, r = image.shape[0], image.shape[2]
    gg = (r // P) ** 2
    cw, cls, pos, gamma, beta = _params(dt, r)
    rows = b * (gg + 1) + extra_rows
    xh = torch.empty(rows, W, dtype=dt, device=DEV)
    xl = torch.empty(rows, W, dtype=ops.PAIR_LO, device=DEV)
    stats = torch.empty(rows, W // 64, 2, dtype=torch.float32, device=DEV)
    if fill is not None:
        xh.view(torch.int16).fill_(fill[0]); xl.fill_(fill[1]); stats.fill_(fill[2])
    assert ops.vit_patch_embed_ln_ok(b, r, P, W, dt)
    ops.vit_patch_embed_ln(image, cw, cls, pos, gamma, beta, xh[:rows - extra_rows], xl[:rows - extra_rows], stats[:rows - extra_rows], P)
    return xh, xl, stats


def _bits(t):
    return t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t


def _assert_same(got, ref, what):
    for name, g, e in zip(("xh", "xl", "stats"), got, ref):
        assert torch.equal(_bits(g), _bits(e)), (what, name, int((_bits(g) != _bits(e)).sum()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("r,b", [(64, 1), (64, 2), (64, 3), (224, 2), (224, 5)])
def test_patch_embed_equals_chain(dt, r, b):
    """One tile with one image, one full tile, an odd last tile (R = 64: 4 patches per image, most tile rows are padding) and the
    ViT-B/32 geometry (49 patches: 98 of 112 rows, three epilogue passes) with an even and an odd batch."""
    image = _rand((b, 3, r, r), 100 + r + b).to(DEV)
    _assert_same(_one_launch(image, dt), _chain(image, dt), (r, b))


@pytest.mark.parametrize("dt", DTS)
def test_patch_embed_writes_its_rows_only(dt):
    """Outputs pre-filled with a sentinel and 8 spare rows behind them: every one of the B (gg + 1) rows is written (equal to the chain,
    which leaves no sentinel) and nothing behind them is touched - the padding rows of the odd last tile included."""
    r, b = 224, 3
    rows = b * 50
    image = _rand((b, 3, r, r), 301).to(DEV)
    fill = (0x7BFF, 0xA5, -12345.0)
    xh, xl, stats = _one_launch(image, dt, extra_rows=8, fill=fill)
    _assert_same((xh[:rows], xl[:rows], stats[:rows]), _chain(image, dt), "rows")
    assert (xh[rows:].view(torch.int16) == fill[0]).all() and (xl[rows:] == fill[1]).all() and (stats[rows:] == fill[2]).all()


@pytest.mark.parametrize("dt", DTS)
def test_patch_embed_images_of_a_tile_do_not_mix(dt):
    """A tile whose first image is large (|x| about 50) and whose second image is all zeros: the second image's rows are those of a
    zero image alone (no leak from the neighbour or from padding rows), and the whole tile equals the chain."""
    r = 224
    image = torch.zeros(2, 3, r, r)
    image[0] = 50.0 * torch.sign(_rand((3, r, r), 401)) + _rand((3, r, r), 402)
    image = image.to(DEV)
    got = _one_launch(image, dt)
    _assert_same(got, _chain(image, dt), "pair of images")
    alone = _one_launch(image[1:2].contiguous(), dt)
    _assert_same(tuple(t[50:] for t in got), alone, "zero image")


def test_patch_embed_race_screen():
    """Counted waits and raw barriers around LDS-DMA pieces in flight: a mis-placed wait shows up as rare wrong rows.  The R = 224,
    B = 6 case twenty times, every result bit-identical to the first, the first equal to the chain."""
    dt = torch.float16
    image = _rand((6, 3, 224, 224), 501).to(DEV)
    first = _one_launch(image, dt)
    _assert_same(first, _chain(image, dt), "first")
    for it in range(19):
        _assert_same(_one_launch(image, dt, fill=(0x7BFF, 0xA5, -12345.0)), first, it)
