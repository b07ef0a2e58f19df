"""Order of destruction in the ctypes binding: a batch or a device tree holds a pointer to its context, so its native object has
to go first, whichever Python object is closed or finalised first.  No GPU: the library is a stand-in that records the calls.

The case that matters is the garbage collector finalising a context and its batches in ONE pass (a failed test's traceback
keeps them in a reference cycle until the interpreter ends): weak references to them are cleared before any __del__ runs and
the context's __del__ may run first.  The context then no longer saw its batches, destroyed itself, and the batches' own
__del__ handed rrt_batch_destroy a batch whose context was freed memory: the process aborted inside the HIP runtime."""
import gc

from rrtplanner_amd import _ffi


class _FakeLib:
    def __init__(self):
        self.calls, self.live_ctx, self.next = [], set(), 100

    def _new(self, ref):
        self.next += 1
        ref._obj.value = self.next
        return self.next

    def rrt_ctx_create(self, dev, ref):
        self.live_ctx.add(self._new(ref))
        return 0

    def rrt_batch_create(self, ctx, Q, n, flags, ref):
        self._new(ref)
        return 0

    def rrt_tree_create(self, ctx, cap, ref):
        self._new(ref)
        return 0

    def rrt_ctx_destroy(self, h):
        self.live_ctx.discard(h.value)
        self.calls.append(("ctx", h.value, True))
        return 0

    def _child(self, kind, h):
        self.calls.append((kind, h.value, 101 in self.live_ctx))  # (the one context of a test is handle 101)
        return 0

    def rrt_batch_destroy(self, h):
        return self._child("batch", h)

    def rrt_tree_destroy(self, h):
        return self._child("tree", h)


def _objects(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_ffi, "_lib", fake)
    ctx = _ffi.Context(0)
    return fake, ctx, _ffi.Batch(ctx, 1, 10), _ffi.Batch(ctx, 2, 10), _ffi.DeviceTree(ctx, 4)


def _check(fake):
    assert sorted(c[:2] for c in fake.calls) == [("batch", 102), ("batch", 103), ("ctx", 101), ("tree", 104)]  # each once
    assert all(alive for _, _, alive in fake.calls), fake.calls  # every child while its context existed
    assert fake.calls[-1][0] == "ctx"


def test_children_closed_first_then_the_context(monkeypatch):
    fake, ctx, b1, b2, t = _objects(monkeypatch)
    b1.close()
    t.close()
    b1.close()
    ctx.close()
    b2.close()
    ctx.close()
    _check(fake)
    assert not b2._h and not t._h and not ctx._h


def test_context_closed_first_takes_its_children_along(monkeypatch):
    fake, ctx, b1, b2, t = _objects(monkeypatch)
    ctx.close()
    for o in (b1, b2, t):
        assert not o._h
        o.close()
    _check(fake)


def test_dropped_in_the_order_of_reference_counts(monkeypatch):
    fake, ctx, b1, b2, t = _objects(monkeypatch)
    del ctx  # the children keep it alive
    assert fake.calls == []
    del b1, b2, t
    gc.collect()
    _check(fake)


def test_context_and_children_finalised_in_one_collector_pass(monkeypatch):
    fake, ctx, b1, b2, t = _objects(monkeypatch)
    gc.collect()
    gc.disable()
    try:
        cycle = [ctx, b1, b2, t]
        cycle.append(cycle)  # what the frames of a failed test's traceback do
        del ctx, b1, b2, t, cycle
        assert fake.calls == []
        gc.collect()
    finally:
        gc.enable()
    _check(fake)
