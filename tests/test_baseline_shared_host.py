"""CPU: the pieces the three baselines share on the host (hgr_net_amd/baseline/_shared.py) - the buffer pool's one re-allocation
rule, the slice plan of the fp32 product, and the counter mix on fixed vectors."""
import types

import numpy as np
import pytest
import torch

from hgr_net_amd import ops
from hgr_net_amd.baseline import _shared, dgp, free


def test_buffer_pool_reallocates_on_shape_dtype_or_device_only():
    pool = _shared.BufferPool(torch.device("cpu"))
    a = pool.pool("x", (3, 4))
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 4)
    assert pool.pool("x", (3, 4)) is a and pool.pool("x", [3, 4]) is a and pool.bufs["x"] is a          # same key and shape: same storage
    b = pool.pool("x", (3, 5))
    assert b is not a and tuple(b.shape) == (3, 5) and b.data_ptr() != a.data_ptr() and pool.bufs["x"] is b
    c = pool.pool("x", (3, 5), torch.bfloat16)
    assert c is not b and c.dtype == torch.bfloat16 and pool.pool("x", (3, 5), torch.bfloat16) is c
    assert pool.pool(("y", 1), (2,)) is not pool.pool(("y", 2), (2,))                                   # keys are independent
    # zero=True fills a NEW buffer with zeros; a kept buffer is handed back as it is
    z = pool.pool("z", (64, 8), zero=True)
    assert not z.any()
    z.fill_(3.0)
    assert pool.pool("z", (64, 8), zero=True) is z and bool((z == 3.0).all())
    assert not pool.pool("z", (64, 9), zero=True).any()
    # a pool made from a parameter reads its device at every call: once the owner has moved, it allocates again
    assert _shared.BufferPool(torch.nn.Parameter(torch.zeros(1))).pool("x", (2, 2)).device.type == "cpu"
    owner = types.SimpleNamespace(device=torch.device("cpu"))          # stands in for a parameter: only `.device` is read
    moving = _shared.BufferPool(owner)
    m = moving.pool("x", (2, 2))
    assert moving.pool("x", (2, 2)) is m
    owner.device = torch.device("meta")
    m2 = moving.pool("x", (2, 2))
    assert m2 is not m and m2.device.type == "meta"


@pytest.mark.parametrize("accumulate_first", [False, True])
@pytest.mark.parametrize("k", [1, 511, 512, 513, 1024, 1300])
def test_sliced_matmul_slice_plan(monkeypatch, k, accumulate_first):
    """The calls `ops.matmul_f32` receives: slices [j, min(k, j + 512)) in ascending order, operands x[:, j:e] and wt[:, j:e].t(), every
    slice with the caller's alpha, the first overwriting unless `accumulate_first`, all later ones accumulating."""
    calls = []

    def record(a, b, out, alpha=1.0, accumulate=False):
        calls.append((a.storage_offset(), a.shape[1], tuple(b.shape), b.storage_offset(), tuple(b.stride()), out.data_ptr(), alpha, accumulate))
        return out
    monkeypatch.setattr(ops, "matmul_f32", record)
    x, wt, out = torch.zeros(3, k), torch.zeros(5, k), torch.zeros(3, 5)
    alpha = 25.0 if not accumulate_first else 1.0
    assert _shared.sliced_matmul_f32(x, wt, out, alpha=alpha, accumulate_first=accumulate_first) is out
    plan = [(j, min(k, j + 512), alpha, accumulate_first or j > 0) for j in range(0, k, 512)]
    assert _shared.K_SLICE == free.K_SLICE == 512 and len(plan) == -(-k // 512)
    assert calls == [(j, e - j, (e - j, 5), j, (1, k), out.data_ptr(), a, acc) for j, e, a, acc in plan]
    assert [(c[0], c[0] + c[1], c[6], c[7]) for c in calls] == plan


def test_sliced_matmul_call_sites(monkeypatch):
    """What the call sites pass: cosine_logits alpha = 5^2 (logits = 25 cos) and a fresh first slice; free.product a fresh first
    slice; the classifier module's logits accumulate onto the bias written first."""
    from hgr_net_amd.baseline import cnzsl
    calls = []
    monkeypatch.setattr(ops, "matmul_f32", lambda a, b, out, alpha=1.0, accumulate=False: calls.append((a.storage_offset(), alpha, accumulate)) or out)
    cnzsl.cosine_logits(torch.zeros(2, 600), torch.zeros(4, 600), torch.zeros(2, 4))
    assert calls == [(0, 25.0, False), (512, 25.0, True)]
    calls.clear()
    free.product(torch.zeros(2, 600), torch.nn.Linear(600, 4), "fp32")
    assert calls == [(0, 1.0, False), (512, 1.0, True)]
    calls.clear()
    free.LinearLogSoftmaxClassifier(600, 4, "fp32").logits(torch.zeros(2, 600))
    assert calls == [(0, 1.0, True), (512, 1.0, True)]


def test_fmix32_fixed_vectors_and_its_two_users():
    """murmur3's finaliser on the edge values, against constants computed with the trainer's earlier copy of the function (the FREE
    copy agreed with it on these and on 10^6 random 32-bit values before the two became one)."""
    edge = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    want = [0x00000000, 0x514E28B7, 0xF9CC0EA8, 0x6D3C65A0, 0x81F16F39]
    assert _shared.fmix32(edge).tolist() == want
    assert [int(_shared.fmix32(np.array(int(v), dtype=np.uint64))) for v in edge] == want            # 0-d input, as normal_bits_host's key
    assert _shared.fmix32(edge + (7 << 32)).tolist() == want                                             # bits above 32 are dropped
    assert edge.tolist() == [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]                                   # the input is left alone
    assert dgp.fmix32 is _shared.fmix32 and free.fmix32 is _shared.fmix32
    # both users through it: pure functions of their arguments with the documented shapes
    keep = dgp.dropout_keep(5, 1, 0, 3, 4)
    assert keep.shape == (3, 4) and keep.dtype == bool and np.array_equal(keep, dgp.dropout_keep(5, 1, 0, 3, 4))
    a, b = free.normal_bits_host(5, 1, 0, 3, 4)
    assert a.shape == b.shape == (3, 4) and a.dtype == b.dtype == np.uint32
