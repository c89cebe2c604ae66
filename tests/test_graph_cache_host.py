"""CPU: the graph-cache policy of hgr_net_amd.graphs.GraphCache, driven with fake capture / alloc / copy callables and integers for
buffer addresses - the policy tree_model.forward (one slot, 4 entries, oldest evicted) and forward_eval_overlapped (two slots, 8
entries, all dropped) share."""
from hgr_net_amd.graphs import STATIC_AFTER, GraphCache


class _Fakes:
    """A "buffer" is its integer address; static buffers are handed out from 1000; an entry is ("graph", buffer, slot)."""

    def __init__(self, max_entries=4, evict="oldest"):
        self.log, self.captured, self.copies, self.allocs = [], [], [], 0
        self.cache = GraphCache(max_entries, evict, pre_drop=self.pre_drop, alloc=self.alloc, copy=self.copy, address=lambda x: x)

    def pre_drop(self):
        self.log.append(("pre_drop", len(self.cache.entries)))

    def alloc(self, like):
        self.allocs += 1
        return 999 + self.allocs

    def copy(self, dst, src):
        self.copies.append((dst, src))

    def capture(self, buf, slot):
        self.captured.append((buf, slot))
        return ("graph", buf, slot)

    def step(self, addr, slot=0):
        return self.cache.lookup(addr, slot, self.capture)


def test_new_generation_clears_everything_and_the_same_one_does_not():
    f = _Fakes()
    assert f.cache.renew("g0") is True and f.cache.gen == "g0"
    for a in range(10, 10 + STATIC_AFTER + 1):           # 9 misses: entries, a static buffer and a miss count exist
        f.step(a)
    assert f.cache.entries and f.cache.static and f.cache.misses == STATIC_AFTER + 1
    before = (dict(f.cache.entries), dict(f.cache.static), f.cache.misses)
    assert f.cache.renew("g0") is False
    assert (f.cache.entries, f.cache.static, f.cache.misses) == before and f.log == []
    assert f.cache.renew("g1") is True
    assert f.cache.entries == {} and f.cache.static == {} and f.cache.misses == 0 and f.cache.gen == "g1"
    assert f.log == []                                   # the caller synchronises before renew(): the hook is for evict="all"


def test_a_hit_resets_the_miss_count():
    f = _Fakes()
    f.cache.renew("g")
    for a in (1, 2, 3):
        f.step(a)
    assert f.cache.misses == 3
    assert f.step(2) == ("graph", 2, 0) and f.cache.misses == 0 and len(f.captured) == 3
    for a in range(20, 20 + STATIC_AFTER):               # 8 more misses in a row: still one capture per address, no static buffer
        f.step(a)
    assert f.cache.misses == STATIC_AFTER and not f.cache.static and not f.copies


def test_eight_misses_capture_per_address_then_one_static_buffer_per_slot():
    f = _Fakes(max_entries=64)
    f.cache.renew("g")
    for i in range(13):                                  # never-repeating addresses, alternating slots like the step parities
        ent = f.step(100 + i, i & 1)
        if i < STATIC_AFTER:
            assert ent == ("graph", 100 + i, i & 1)
        else:
            assert ent == ("graph", 1000 + (i & 1), i & 1)          # slot 0 got buffer 1000, slot 1 buffer 1001
    assert f.captured[:STATIC_AFTER] == [(100 + i, i & 1) for i in range(STATIC_AFTER)]
    assert f.captured[STATIC_AFTER:] == [(1000, 0), (1001, 1)]       # capture once per slot
    assert f.copies == [(1000 + (i & 1), 100 + i) for i in range(STATIC_AFTER, 13)]    # copy every time
    assert f.allocs == 2 and f.cache.static == {0: 1000, 1: 1001}


def test_bound_evict_oldest_keeps_the_others_hitting():
    f = _Fakes(max_entries=4, evict="oldest")
    f.cache.renew("g")
    for a in (1, 2, 3, 4, 5):
        f.step(a)
    assert list(f.cache.entries) == [(2, 0), (3, 0), (4, 0), (5, 0)] and f.log == []
    for a in (2, 3, 4, 5):
        f.step(a)
    assert len(f.captured) == 5                          # all four hit
    f.step(1)                                            # the evicted one is captured again, and 2 - the oldest inserted - goes
    assert len(f.captured) == 6 and list(f.cache.entries) == [(3, 0), (4, 0), (5, 0), (1, 0)]


def test_bound_clear_all_runs_the_hook_before_the_entries_go():
    f = _Fakes(max_entries=4, evict="all")
    f.cache.renew("g")
    for a in (1, 2, 3, 4):
        f.step(a, a & 1)
    assert f.log == []
    f.step(5, 1)
    assert f.log == [("pre_drop", 4)] and list(f.cache.entries) == [(5, 1)]
    f.step(1, 1)
    assert len(f.captured) == 6                          # gone with the others


def test_slots_do_not_see_each_other():
    f = _Fakes(max_entries=64)
    f.cache.renew("g")
    assert f.step(7, 0) == ("graph", 7, 0)
    assert f.step(7, 1) == ("graph", 7, 1) and f.captured == [(7, 0), (7, 1)]        # same address, other slot: a miss
    assert f.step(7, 0) == ("graph", 7, 0) and len(f.captured) == 2
    for i in range(STATIC_AFTER + 1):                    # slot 1 alone goes static
        f.step(50 + i, 1)
    assert f.cache.static == {1: 1000}
    f.step(90, 0)                                        # 10th miss in a row, in slot 0: its own static buffer and its own capture
    assert f.cache.static == {1: 1000, 0: 1001} and f.captured[-1] == (1001, 0)
