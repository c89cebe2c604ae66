"""Full, fixed-shape evaluation batches packed from the group loaders' one-class batches.

The group loaders hand out one class per batch (the reference's GroupBatchSampler contract), so on a real split - a few hundred
images per class, many classes below the batch size - most batches are partial and every class ends in a remainder of its own size.
tree_model keys its HIP graphs on the input shape: every new shape drops the captured graphs and runs the step eagerly before
capturing again.  Nothing in the image tower or in the per-row evaluation needs a batch to be one class, and the counters are
row-additive (hgr_eval_counters_rows scores every row against its own class), so PackedBatches refills the rows into batches of
exactly ``batch_size``: one shape for the whole run, only the last batch padded.
"""
from __future__ import annotations

from typing import Iterable, Iterator, List

import torch


class PackedBatches:
    """Wraps an iterable of batch dicts {"img": [1, b, ...] (f32 or u8), "label": [1, b] int64} and yields
    {"img": [1, B, ...], "label": [1, B]} with B = ``batch_size``, rows in arrival order.

    * ``img`` is a view of one of ``n_buffers`` persistent buffers on ``device``, filled row range by row range with
      ``copy_(non_blocking=True)`` on the current stream, so the input addresses recur and the graphs captured for them are
      replayed.  tree_model keeps 4 graphs keyed by the input address on the single-graph route and 8 keyed by (address, step
      parity) on the pipelined route: two buffers give 2 entries on the first and, whichever way buffers and parities pair up
      (they pair up one to one as long as every step takes the same route), at most 4 on the second - inside both caches, while
      the buffer being filled is never the one the step just launched reads on the same stream ahead of the copy.  A larger ring
      buys nothing: filling and reading are ordered on one stream anyway.
    * Only the image buffers rotate.  Every packed batch gets a FRESH label tensor (assembled on the host, staged through pinned
      memory when the target is a GPU): the pipelined route reads the labels on its tail stream, after the next batch is already
      being packed.  The images may rotate because nothing behind the split point of a pipelined step reads the input tensor
      (tree_model._eager_phase / forward_eval_overlapped: the tail starts after the keys / values GEMM of the last block and works
      on workspace buffers only; the pixels are consumed by the patch embedding at the very start of the head, on the stream the
      next fill is queued on).
    * The last batch keeps the shape: its unused rows are labelled -1 (padding for hgr_eval_counters_rows).  The buffers are
      zero-filled when created; later a padding row holds whatever an earlier batch left there, i.e. a valid image - never
      uninitialised memory, which the LayerNorm range guard (it looks at every row) could trip on.
    * dtype and the per-image shape (resolution, channel layout) are those of the first source batch; a later batch that differs
      raises ValueError.  An empty source yields nothing.  Works on CPU tensors too (``device="cpu"``; no pinned memory then).
    """

    def __init__(self, loader: Iterable, batch_size: int, device, n_buffers: int = 2):
        if batch_size < 1 or n_buffers < 1:
            raise ValueError(f"PackedBatches: batch_size={batch_size}, n_buffers={n_buffers}")
        self.loader, self.batch_size, self.device, self.n_buffers = loader, int(batch_size), torch.device(device), int(n_buffers)
        self._bufs: List[torch.Tensor] = []
        self._next = 0                       # buffer of the next packed batch: keeps rotating across iterations of the same object

    def __len__(self) -> int:
        """Number of packed batches - defined only for a source whose per-batch sizes are known without consuming it (a list or
        tuple of batch dicts); TypeError otherwise, as for an object without a length."""
        if not isinstance(self.loader, (list, tuple)):
            raise TypeError("PackedBatches has a length only over a list / tuple of batches")
        return -(-sum(int(d["label"].shape[-1]) for d in self.loader) // self.batch_size)

    def _labels(self, host: List[int]) -> torch.Tensor:
        """[1, B] int64 on the device, a fresh tensor: -1 behind the real rows."""
        host = host + [-1] * (self.batch_size - len(host))
        if self.device.type == "cpu":
            return torch.tensor(host, dtype=torch.int64).view(1, -1)
        # the pinned block goes back to the caching host allocator when `pin` dies; it is handed out again only after this copy
        pin = torch.empty(self.batch_size, dtype=torch.int64, pin_memory=True)
        pin.numpy()[:] = host
        dev = torch.empty(self.batch_size, dtype=torch.int64, device=self.device)
        dev.copy_(pin, non_blocking=True)
        return dev.view(1, -1)

    def _buffer(self, like: torch.Tensor) -> torch.Tensor:
        if not self._bufs:
            self._bufs = [torch.zeros((self.batch_size,) + tuple(like.shape[1:]), dtype=like.dtype, device=self.device)
                          for _ in range(self.n_buffers)]
        buf = self._bufs[self._next]
        self._next = (self._next + 1) % self.n_buffers
        return buf

    def __iter__(self) -> Iterator[dict]:
        B = self.batch_size
        buf, fill, labels = None, 0, []
        for data in self.loader:
            src, lab = data["img"][0], data["label"].reshape(-1)
            if src.shape[0] != lab.numel():
                raise ValueError(f"PackedBatches: {src.shape[0]} images with {lab.numel()} labels")
            if self._bufs and (src.dtype != self._bufs[0].dtype or tuple(src.shape[1:]) != tuple(self._bufs[0].shape[1:])):
                raise ValueError(f"PackedBatches: a batch of {src.dtype} {tuple(src.shape[1:])} images after "
                                 f"{self._bufs[0].dtype} {tuple(self._bufs[0].shape[1:])} ones")
            lab = lab.tolist()                                   # the loaders make their labels on the host
            done = 0
            while done < len(lab):                               # a source batch may end one packed batch and start the next
                if buf is None:
                    buf, fill, labels = self._buffer(src), 0, []
                n = min(B - fill, len(lab) - done)
                buf[fill:fill + n].copy_(src[done:done + n], non_blocking=True)
                labels.extend(lab[done:done + n])
                fill, done = fill + n, done + n
                if fill == B:
                    yield {"img": buf[None], "label": self._labels(labels)}
                    buf = None
        if buf is not None:
            yield {"img": buf[None], "label": self._labels(labels)}
