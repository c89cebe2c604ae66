"""Which captured HIP graph replays for which input buffer: the one cache policy behind tree_model.forward / forward_eval (one
slot) and forward_eval_overlapped (two slots = the step parities).

A graph is bound to the buffers it was captured on, so entries live for one GENERATION (whatever the caller puts into the key:
shape, classifier, weights, workspace epoch); a new generation drops everything.  Inside a generation entries are keyed by
(address of the input buffer, slot) - loaders recycle a few buffers - and bounded in number.  After STATIC_AFTER misses in a row the
addresses evidently never repeat: from then on the input is copied into one static buffer per slot and that buffer's entry is
looked up instead.

The class owns the policy and nothing else.  Capturing (with its warm-up and stream waits), allocating and copying are callables
of the caller, so the policy runs on the CPU with fakes (tests/test_graph_cache_host.py).  Nothing here imports the GPU runtime.
"""
from __future__ import annotations

from typing import Callable, Optional

STATIC_AFTER = 8          # consecutive misses that are still captured per address


def _empty_like(x):
    import torch
    return torch.empty_like(x)


class GraphCache:
    """``max_entries`` / ``evict``: at the bound, "oldest" drops the entry inserted first (the others keep hitting), "all" drops
    every entry, after ``pre_drop()``: their graphs may still be in flight, the caller orders and synchronises its streams there
    (before renew() it does so itself).  ``alloc(x)`` makes a static buffer like ``x``, ``copy(dst, src)`` fills it, ``address(x)``
    is the key of a buffer."""

    def __init__(self, max_entries: int, evict: str = "oldest", pre_drop: Optional[Callable[[], None]] = None,
                 alloc: Callable = _empty_like, copy: Callable = lambda dst, src: dst.copy_(src),
                 address: Callable = lambda x: x.data_ptr()):
        assert evict in ("oldest", "all") and max_entries >= 1
        self.max_entries, self.evict, self.pre_drop = max_entries, evict, pre_drop
        self.alloc, self.copy, self.address = alloc, copy, address
        self.gen = None
        self.entries = {}         # (address, slot) -> what capture() returned; dicts keep insertion order
        self.static = {}          # slot -> static input buffer (its entry lives in `entries` under the buffer's address)
        self.misses = 0

    def renew(self, gen) -> bool:
        """False when ``gen`` is the current generation.  Otherwise entries, static buffers and the miss count of the old one go
        and True is returned; a caller whose warm-up moves the key then stores the settled one in ``self.gen``."""
        if gen == self.gen:
            return False
        self.entries.clear()
        self.static.clear()
        self.misses = 0
        self.gen = gen
        return True

    def lookup(self, inputs, slot: int, capture: Callable):
        """The entry to replay for ``inputs`` in ``slot``; ``capture(buffer, slot)`` makes a missing one, on ``inputs`` itself or
        on the slot's static buffer (which by then holds a copy of ``inputs``)."""
        key = (self.address(inputs), slot)
        ent = self.entries.get(key)
        if ent is not None:
            self.misses = 0
            return ent
        self.misses += 1
        if self.misses > STATIC_AFTER:
            buf = self.static.get(slot)
            if buf is None:
                buf = self.static[slot] = self.alloc(inputs)
            self.copy(buf, inputs)               # on the caller's stream, behind the replay that last read the buffer
            inputs, key = buf, (self.address(buf), slot)
            ent = self.entries.get(key)
            if ent is not None:
                return ent
        if len(self.entries) >= self.max_entries:
            if self.evict == "all":
                if self.pre_drop is not None:
                    self.pre_drop()
                self.entries.clear()
            else:
                self.entries.pop(next(iter(self.entries)))
        ent = self.entries[key] = capture(inputs, slot)
        return ent
