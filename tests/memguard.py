"""Memory-contract helpers: poisoned, guard-banded tensors and an allocation seam for `interpol._hip`.

Every output and workspace of the HIP library is allocated by `interpol/_hip.py` through ONE callable, `_hip._empty`.  The
kernels therefore owe three things: they write every output element, they zero what they accumulate into, and they never
depend on what a buffer held before the call.  A value test cannot see a breach: the caching allocator hands the next call
the block that still holds the previous route's correct answer, fresh device memory is mostly zero, and a write (or a read
weighted by zero) a few elements past a tensor lands in a neighbouring block.

`guarded()` builds a dense tensor INSIDE a larger buffer whose every other byte is poison; `installed()` replaces
`_hip._empty` by it for the duration of a `with` block, records what it hands out and offers the three checks
(`assert_guards_intact`, `assert_fully_written`, `workspace_was_written`).  `place()` puts an input tensor between poisoned
guards the same way: a read outside the tensor turns the result NaN.

Poison: every byte 0xFF in floating-point tensors (a NaN in float64 / float32 / float16 / bfloat16) and in uint8 workspaces;
every byte 0xA5 in int32 tensors (`LABEL_POISON`, a value no label map of the tests contains).

A plain module (no fixtures, no pytest hooks): it works on CPU tensors too, which is how tests/test_memguard_cpu.py tests it.
"""
import contextlib

import torch

GUARD_BYTES = 4096            # smallest guard band on either side
ALIGN = 256                   # base alignment of every guarded tensor before `misalign` (the brick routes want 256-byte workspaces)
LABEL_POISON = int.from_bytes(b"\xa5" * 4, "little", signed=True)


def poison_byte(dtype):
    if dtype.is_floating_point or dtype == torch.uint8:
        return 0xFF
    if dtype == torch.int32:
        return 0xA5
    raise TypeError("memguard: no poison defined for %s" % dtype)


def _shape_list(shape):
    if isinstance(shape, int):
        return [int(shape)]
    return [int(s) for s in shape]


class Guarded:
    """One guarded allocation: `raw` (uint8, the whole buffer), `tensor` (the interior view), the byte range of the view."""

    def __init__(self, raw, tensor, lo, hi, workspace):
        self.raw, self.tensor, self.lo, self.hi, self.workspace = raw, tensor, lo, hi, workspace
        self.poison = poison_byte(tensor.dtype)

    def guard_damage(self):
        """Number of guard bytes that no longer hold poison (front, back)."""
        front, back = self.raw[:self.lo], self.raw[self.hi:]
        return int((front != self.poison).sum()), int((back != self.poison).sum())

    def interior_bytes(self):
        return self.raw[self.lo:self.hi]


def _guarded(shape, dtype, device, misalign=0, fill=None, workspace=False):
    shape = _shape_list(shape)
    es = torch.empty(0, dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    if not 0 <= misalign <= 3:
        raise ValueError("memguard: misalign is 0..3 elements")
    if (dtype == torch.uint8 or workspace) and misalign:
        raise ValueError("memguard: workspaces keep their 256-byte alignment (a misaligned one makes the library decline the brick routes)")
    plane = 1
    for s in shape[-2:]:
        plane *= s
    guard = max(GUARD_BYTES, plane * es)
    guard = (guard + ALIGN - 1) // ALIGN * ALIGN
    nbytes = numel * es
    total = guard + ALIGN + misalign * es + nbytes + guard
    raw = torch.empty(total, dtype=torch.uint8, device=device)
    raw.fill_(poison_byte(dtype))
    lo = guard + (-(raw.data_ptr() + guard)) % ALIGN + misalign * es
    hi = lo + nbytes
    assert lo >= guard and total - hi >= guard
    tensor = raw[lo:hi].view(dtype).view(shape)
    if fill is not None:
        if torch.is_tensor(fill):
            tensor.copy_(fill)
        else:
            tensor.fill_(fill)
    return Guarded(raw, tensor, lo, hi, workspace or dtype == torch.uint8)


def guarded(shape, dtype, device, misalign=0, fill=None):
    """A dense tensor of `shape` that is an interior view of a larger poisoned buffer: a guard band of at least 4096 bytes and at
    least one innermost plane of the tensor on each side, so that a small overrun stays inside this allocation.  `misalign`
    (0..3 elements) shifts the base pointer off its 256-byte alignment.  `fill`: None leaves the interior poisoned, a number or a
    tensor initialises it.  The record is reachable as `tensor._memguard`."""
    g = _guarded(shape, dtype, device, misalign, fill)
    g.tensor._memguard = g
    return g.tensor


def place(t, device, misalign=0):
    """Input builder: a copy of `t` on `device` between poisoned guards (`misalign` elements off 16-byte alignment)."""
    return guarded(list(t.shape), t.dtype, device, misalign, fill=t)


def unwritten(t, ref=None):
    """Number of elements of an output that still hold poison.  Floating point: NaN where the reference (`ref`, optional) is
    not NaN itself -- an unwritten element, or one computed from a read outside an input's bounds."""
    if t.dtype.is_floating_point:
        bad = torch.isnan(t)
        if ref is not None:
            bad = bad & ~torch.isnan(torch.as_tensor(ref).to(bad.device))
        return int(bad.sum())
    if t.dtype == torch.int32:
        return int((t == LABEL_POISON).sum())
    raise TypeError("memguard: no coverage check for %s outputs" % t.dtype)


def assert_fully_written(t, ref=None, what=""):
    n = unwritten(t, ref)
    assert n == 0, "%s: %d of %d output elements hold poison (never written, or computed from memory outside a tensor)" % (what, n, t.numel())


def assert_guard_intact(t, what=""):
    """The guards of one `guarded()` / `place()` tensor."""
    front, back = t._memguard.guard_damage()
    assert front == 0 and back == 0, "%s: guard bytes overwritten: %d in front of the tensor, %d behind it" % (what, front, back)


class Seam:
    """The `_empty` replacement and its record.  Outputs (a shape list) take `misalign`; workspaces and scratch accumulators --
    uint8, or a flat size given as an int -- stay 256-byte aligned."""

    def __init__(self, misalign=0):
        self.misalign = misalign
        self.records = []

    def empty(self, *size, dtype=None, device=None):
        shape = size[0] if len(size) == 1 else list(size)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        flat = isinstance(shape, int)
        workspace = flat or dtype == torch.uint8
        g = _guarded(shape, dtype, device if device is not None else "cpu", 0 if workspace else self.misalign, None, workspace)
        g.tensor._memguard = g
        self.records.append(g)
        return g.tensor

    def outputs(self):
        return [g for g in self.records if not g.workspace]

    def workspaces(self):
        return [g for g in self.records if g.workspace]

    def assert_guards_intact(self, what=""):
        for i, g in enumerate(self.records):
            front, back = g.guard_damage()
            assert front == 0 and back == 0, ("%s: guard bytes overwritten around allocation %d (%s %s%s): %d in front, %d behind"
                                              % (what, i, g.tensor.dtype, list(g.tensor.shape), ", workspace" if g.workspace else "", front, back))

    def assert_fully_written(self, t, ref=None, what=""):
        assert_fully_written(t, ref, what)

    def workspace_was_written(self):
        """Did the library change a byte of a workspace it was handed?  (The proof that a workspace-driven organisation ran.)"""
        return any(bool((g.interior_bytes() != g.poison).any()) for g in self.workspaces() if g.tensor.numel())

    def reset(self):
        self.records.clear()


@contextlib.contextmanager
def installed(hip, misalign=0, monkeypatch=None):
    """Install a `Seam` as `hip._empty` (`hip`: the interpol._hip module, or any object with `_empty`).  Every workspace of the
    block is a fresh, poisoned one: the workspace cache is emptied and bypassed.  With `monkeypatch` (pytest's fixture) the
    replacement goes through it; either way the previous state is back on exit."""
    seam = Seam(misalign)
    saved = {}

    def swap(name, value):
        if not hasattr(hip, name):
            return
        saved[name] = getattr(hip, name)
        if monkeypatch is not None:
            monkeypatch.setattr(hip, name, value)
        else:
            setattr(hip, name, value)

    release = getattr(hip, "release_workspaces", lambda: None)
    release()
    swap("_empty", seam.empty)
    swap("_WS_NOCACHE", True)
    try:
        yield seam
    finally:
        for name, value in saved.items():
            setattr(hip, name, value)
        release()
