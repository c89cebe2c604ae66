"""CPU: argument validation of hgr_vit_patch_embed_ln and its shape predicate.  Every call here is rejected in front of the launch
(validate, then launch), so the operands are small host buffers that are never read."""
import ctypes as C

import numpy as np
import pytest
import torch

from hgr_net_amd import _lib, ops
from hgr_net_amd._lib import HGR_BF16, HGR_F16

EINVAL = -1
NAMES = ("image", "conv_w", "cls", "pos", "gamma", "beta", "xh", "xl", "stats")


def _operands():
    """Nine 16-byte aligned host addresses (one buffer, 64 bytes apart), kept alive by the caller."""
    buf = np.zeros(1024 + 16, dtype=np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    return buf, [base + 64 * i for i in range(len(NAMES))]


def _call(ptrs, b=2, r=224, p=32, w=768, dtype=HGR_F16):
    lib = _lib.load()
    rc = lib.hgr_vit_patch_embed_ln(*[C.c_void_p(x) for x in ptrs], b, r, p, w, 1e-5, dtype, None)
    return rc, lib.hgr_last_error().decode()


def test_rejects_null_and_misaligned_operands():
    buf, ptrs = _operands()
    for i, name in enumerate(NAMES):
        rc, msg = _call(ptrs[:i] + [0] + ptrs[i + 1:])
        assert rc == EINVAL and "hgr_vit_patch_embed_ln" in msg and "null" in msg, (name, rc, msg)
        rc, msg = _call(ptrs[:i] + [ptrs[i] + 4] + ptrs[i + 1:])
        assert rc == EINVAL and "hgr_vit_patch_embed_ln" in msg and "aligned" in msg, (name, rc, msg)


@pytest.mark.parametrize("kw,word", [(dict(p=16), "P=16"), (dict(p=14, r=224), "P=14"), (dict(r=256), "64 patches"), (dict(r=225), "R=225"),
                                     (dict(r=16), "R=16"), (dict(w=512), "W=512"), (dict(w=1024), "W=1024"), (dict(dtype=7), "dtype 7"),
                                     (dict(b=0), "B=0")])
def test_rejects_unsupported_geometry(kw, word):
    buf, ptrs = _operands()
    rc, msg = _call(ptrs, **kw)
    assert rc == EINVAL and rc < 0 and "hgr_vit_patch_embed_ln" in msg and word in msg, (kw, rc, msg)


def test_predicate_agrees_with_the_entry_point_on_both_sides_of_each_limit():
    """ops.vit_patch_embed_ln_ok == "the entry point gets past its geometry checks" (told apart from a launch by one misaligned operand:
    a supported geometry is then rejected for alignment, an unsupported one for its geometry - nothing is ever launched)."""
    buf, ptrs = _operands()
    bad_align = ptrs[:8] + [ptrs[8] + 4]
    cases = [(dict(), True), (dict(r=224), True), (dict(r=256), False),           # gg = 49 | 64 around the limit of 56
             (dict(r=32), True), (dict(r=16), False), (dict(r=64), True), (dict(r=72), False),
             (dict(p=32), True), (dict(p=16), False), (dict(p=64, r=256), False),
             (dict(w=768), True), (dict(w=704), False), (dict(w=832), False),
             (dict(b=1), True), (dict(b=0), False), (dict(b=513), True),
             (dict(dtype=HGR_F16), True), (dict(dtype=HGR_BF16), True), (dict(dtype=2), False), (dict(dtype=-1), False)]
    for kw, want in cases:
        a = dict(b=2, r=224, p=32, w=768, dtype=HGR_F16)
        a.update(kw)
        assert ops.vit_patch_embed_ln_ok(a["b"], a["r"], a["p"], a["w"], a["dtype"]) is want, kw
        rc, msg = _call(bad_align, **a)
        assert rc == EINVAL
        assert ("aligned" in msg) is want, (kw, msg)
    assert ops.vit_patch_embed_ln_ok(2, 224, 32, 768, torch.float16) and ops.vit_patch_embed_ln_ok(2, 224, 32, 768, torch.bfloat16)
    assert not ops.vit_patch_embed_ln_ok(2, 224, 32, 768, torch.float32)
