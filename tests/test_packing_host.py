"""CPU: dataset.packing.PackedBatches on host tensors (row order, splitting, padding, buffer rotation, fresh labels), the
argument validation of hgr_eval_counters_rows (nothing is launched) and the --pack_batches switch of the command line."""
import ctypes as C
import math

import pytest
import torch

from hgr_net_amd.dataset.packing import PackedBatches

SIZES = [5, 37, 64, 1, 130, 3]
B = 64


def _source(sizes, res=4, dtype=torch.float32, first_label=100):
    """One class per source batch, every image filled with its own global row number."""
    out, row = [], 0
    for c, n in enumerate(sizes):
        ids = torch.arange(row, row + n)
        img = (ids % 251).to(dtype).view(n, 1, 1, 1).expand(n, 3, res, res).contiguous()
        out.append({"img": img[None], "label": torch.full((1, n), first_label + c, dtype=torch.long)})
        row += n
    return out


def test_packed_batches_keep_rows_labels_and_order():
    src = _source(SIZES)
    want_img = torch.cat([d["img"][0] for d in src])
    want_lab = torch.cat([d["label"][0] for d in src])
    total = sum(SIZES)
    packer = PackedBatches(src, B, "cpu")
    assert len(packer) == math.ceil(total / B) == 4
    imgs, labs, ptrs, objs = [], [], [], []
    for d in packer:
        assert d["img"].shape == (1, B, 3, 4, 4) and d["label"].shape == (1, B) and d["label"].dtype == torch.int64
        imgs.append(d["img"][0].clone())                  # the buffers rotate: copy before the next batch is packed
        labs.append(d["label"][0])
        ptrs.append(d["img"].data_ptr())
        objs.append(d["label"])
    assert len(imgs) == 4
    got_img, got_lab = torch.cat(imgs), torch.cat(labs)
    assert torch.equal(got_img[:total], want_img) and torch.equal(got_lab[:total], want_lab)
    pad = 4 * B - total
    assert pad == 16 and torch.equal(labs[-1][B - pad:], torch.full((pad,), -1, dtype=torch.long)) and (got_lab[:total] >= 0).all()
    # the 130-row source (rows 107 .. 236) spans the packed batches 1, 2 and 3
    big = 100 + SIZES.index(130)
    assert [i for i, l in enumerate(labs) if (l == big).any()] == [1, 2, 3]
    assert int((labs[2] == big).sum()) == B
    # image buffers alternate between exactly two addresses; every label tensor is its own object with its own storage
    assert len(set(ptrs)) == 2 and ptrs[0] == ptrs[2] and ptrs[1] == ptrs[3] and ptrs[0] != ptrs[1]
    assert len({id(o) for o in objs}) == 4 and len({o.data_ptr() for o in objs}) == 4
    assert torch.equal(objs[0][0], got_lab[:B])           # an earlier label tensor is not overwritten by later batches


def test_padding_rows_are_never_uninitialised():
    """First (and only) batch: the rows behind the data are the zeros the buffers were created with."""
    (d,) = list(PackedBatches(_source([3]), 8, "cpu"))
    assert torch.equal(d["img"][0, 3:], torch.zeros(5, 3, 4, 4)) and d["label"][0].tolist() == [100, 100, 100, -1, -1, -1, -1, -1]


def test_source_batch_larger_than_the_packed_batch_and_exact_fit():
    out = list(PackedBatches(_source([20]), 8, "cpu", n_buffers=2))
    assert [int((d["label"] >= 0).sum()) for d in out] == [8, 8, 4]
    out = list(PackedBatches(_source([8, 8]), 8, "cpu"))
    assert len(out) == 2 and all(int((d["label"] >= 0).sum()) == 8 for d in out)      # no empty trailing batch


def test_empty_source_yields_nothing():
    assert list(PackedBatches([], B, "cpu")) == []
    assert list(PackedBatches(iter(()), B, "cpu")) == []


def test_generator_source_has_no_length():
    with pytest.raises(TypeError):
        len(PackedBatches(iter(_source([3, 4])), B, "cpu"))


def test_mismatched_resolution_or_dtype_raises():
    with pytest.raises(ValueError):
        list(PackedBatches(_source([5]) + _source([5], res=6), B, "cpu"))
    with pytest.raises(ValueError):
        list(PackedBatches(_source([5]) + _source([5], dtype=torch.uint8), B, "cpu"))


def test_uint8_source_stays_uint8():
    src = _source([5, 70], dtype=torch.uint8)
    out = list(PackedBatches(src, B, "cpu"))
    assert len(out) == 2 and all(d["img"].dtype == torch.uint8 for d in out)
    assert torch.equal(out[0]["img"][0, :5], src[0]["img"][0])


def test_eval_counters_rows_rejects_bad_arguments_without_launching():
    """hgr_eval_counters_rows validates on the host before anything touches a device: null targets, k = 33, n_levels = 33 and
    rows = 0 come back as the library's error code (the pointers are never dereferenced on this path)."""
    from hgr_net_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(k=20, targets=p, n_levels=8, rows=4):
        return lib.hgr_eval_counters_rows(p, k, targets, p, p, n_levels, p, p, p, 10, p, rows, None)

    for kw in (dict(targets=None), dict(k=33), dict(n_levels=33), dict(rows=0)):
        rc = call(**kw)
        assert rc != 0, kw
        assert b"hgr_eval_counters_rows" in lib.hgr_last_error()
    with pytest.raises(_lib.HgrError, match="hgr_eval_counters_rows"):
        _lib.call("hgr_eval_counters_rows", p, 33, p, p, p, 8, p, p, p, 10, p, 4, None)


def test_parser_has_pack_batches_off_by_default():
    from hgr_net_amd import main
    assert main.build_parser().parse_args([]).pack_batches is False
    assert main.build_parser().parse_args(["--pack_batches", "True"]).pack_batches is True
