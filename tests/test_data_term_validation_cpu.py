"""The rejections of the four fused data terms (csrc/ssd.hip, lcc.hip, ssd_affine.hip, mi_affine.hip), without a device.

Every rejection of `interpol_ssd`, `interpol_lcc`, `interpol_ssd_affine`, `interpol_mi_affine` and of their `*_workspace` queries
happens on the host before the first launch, so the library answers them on a machine without a GPU.  The pointers here are
fabricated addresses -- integers laid out like a real set of tensors, 256-byte aligned, one after the other -- and are never
dereferenced on the host.

NO CALL HERE IS ONE THAT WOULD BE ACCEPTED: an accepted call launches.  Every call of an entry point is expected to return a
negative code (`rejected` asserts it); where the accepting side of a limit is pinned, it is pinned through the `*_workspace` query,
which only computes.

The table is the one the four `test_entry_points_validate_before_launching` tests assert on the device (they also show that nothing
was written), with what they leave out: the batch limit of the affine terms (65535 accepted, 65536 refused; 2^31 - 1 for the
field terms), the 4 GiB span of one image of `moving`, a stride of 2 GiB, N above 2^32, and which of two coinciding failures is
reported.  The codes were recorded from the library as it was before the validation of the four terms was folded into one
(csrc/data_term.hpp) and hold unchanged since.
"""
import ctypes

import pytest
import torch

from interpol import _hip

F32, F64 = torch.float32, torch.float64
E_DIM, E_ORDER, E_BOUND, E_DTYPE, E_SHAPE, E_NULL, E_EXTRAP, E_SCRATCH, E_STRIDE = -1, -2, -3, -4, -5, -6, -7, -9, -10
INSHAPE, SHAPE = (6, 5, 4), (5, 4, 7)
N = 5 * 4 * 7
BINS = 16


class Fake:
    """a dense tensor that is an address and a shape"""
    next_address = 1 << 33                                               # (above 4 GiB, as device pointers are)

    def __init__(self, shape, itemsize=4):
        self.shape, self.itemsize = tuple(shape), itemsize
        self.numel = 1
        for s in shape:
            self.numel *= s
        self.address = Fake.next_address
        Fake.next_address += -(-self.numel * itemsize // 256) * 256 + 256
        self.strides, acc = [], 1
        for s in reversed(shape):
            self.strides.insert(0, acc)
            acc *= s

    def __repr__(self):
        return "Fake(%s at %#x)" % (list(self.shape), self.address)

    def stride(self, d):
        return self.strides[d]

    def at(self, element):
        """the address `element` elements into the tensor"""
        return self.address + element * self.itemsize


def address(t):
    return 0 if t is None else (t if isinstance(t, int) else t.address)


def rejected(rc, want, what, failures):
    """an entry point's answer: negative, and the code of the table"""
    assert rc < 0, "%s was ACCEPTED (%d): this test must never make a call that launches" % (what, rc)
    if rc != want:
        failures.append("%s: %d, the table says %d" % (what, rc, want))


def queried(got, want, what, failures):
    if got != want:
        failures.append("%s: %d, the table says %d" % (what, got, want))


class Operands:
    """the tensors of one call: moving (2, C, 6, 5, 4), fixed (2, C, 5, 4, 7), weight (2, 5, 4, 7), the lattice and the outputs"""

    def __init__(self, C, affine):
        self.C, self.affine = C, affine
        self.moving, self.fixed, self.weight = Fake((2, C) + INSHAPE), Fake((2, C) + SHAPE), Fake((2,) + SHAPE)
        self.loss = Fake((2,))
        if affine:
            self.lattice, self.grad, self.hess = Fake((2, 3, 4)), Fake((2, 3, 4)), Fake((2, 12, 12))
        else:
            self.lattice, self.grad, self.hess = Fake((2,) + SHAPE + (3,)), Fake((2,) + SHAPE + (3,)), Fake((2,) + SHAPE + (6,))
        self.ranges, self.hist = Fake((2, 5), 8), Fake((2, BINS, BINS))

    def problem(self, dtype=F32, gdtype=None, dim=3, order=(3, 3, 3), bound=3, extrapolate=1, C=None, B=2, mstr=None, dstr=None,
                fstr=None, flags=None, inshp=INSHAPE, shp=SHAPE):
        m, f, u = self.moving, self.fixed, self.lattice
        mstr = mstr or [m.stride(0), m.stride(1), *m.strides[2:]]
        fstr = fstr or [f.stride(0), f.stride(1), *f.strides[2:], 0, 0]
        if self.affine:
            dstr = [0] * 5
        else:
            dstr = dstr or [u.stride(0), *u.strides[1:4], 1]
        flags = (_hip.FLAG_AFFINE_GRID if self.affine else 0) if flags is None else flags
        return _hip.make_problem(dim, dtype, gdtype or dtype, [bound] * 3, list(order), extrapolate, B, self.C if C is None else C,
                                 inshp, shp, mstr, dstr, fstr, flags)


# what every one of the four refuses in the problem itself, as (keywords of `problem`, code): the checks in their order
def problem_table(ops):
    m, f = ops.moving, ops.fixed
    big = (1 << 16, 1 << 16, 2)                                          # 2^33 samples
    big_f, big_d = [0, 0, 1 << 17, 2, 1, 0, 0], [0, 3 << 17, 6, 3, 1]
    edge = (1 << 16, 1 << 16, 1)                                         # 2^32 samples: one too many
    edge_f, edge_d = [0, 0, 1 << 16, 1, 1, 0, 0], [0, 3 << 16, 3, 3, 1]
    table = [(dict(dim=0), E_DIM), (dict(dim=4), E_DIM), (dict(dim=-1), E_DIM)]
    table += [(dict(order=o), E_ORDER) for o in ((0, 0, 0), (4, 4, 4), (1, 2, 3), (3, 3, 1), (8, 8, 8), (-1, -1, -1), (7, 7, 7), (2, 3, 3))]
    table += [(dict(bound=b), E_BOUND) for b in (-1, 7)]
    table += [(dict(dtype=torch.bfloat16, gdtype=F32), E_DTYPE), (dict(dtype=torch.float16, gdtype=F32), E_DTYPE),
              (dict(gdtype=F64), E_DTYPE), (dict(dtype=F64, gdtype=F32), E_DTYPE)]
    table += [(dict(C=0), E_SHAPE), (dict(B=0), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(C=1 << 31), E_SHAPE), (dict(B=1 << 31), E_SHAPE),
              (dict(inshp=(6, 0, 4)), E_SHAPE), (dict(inshp=(6, 5, 1 << 30)), E_SHAPE), (dict(shp=(5, 0, 7)), E_SHAPE),
              (dict(shp=(5, 4, 1 << 31)), E_SHAPE)]
    table += [(dict(extrapolate=e), E_EXTRAP) for e in (-1, 3)]
    table += [(dict(fstr=[f.stride(0), 1, 84, 21, 3, 0, 0]), E_STRIDE),                     # a channel-last fixed image
              (dict(fstr=[f.stride(0), f.stride(1), 4, 28, 7, 0, 0]), E_STRIDE),               # ... one that is not row-major
              (dict(mstr=[m.stride(0), m.stride(1), -20, 4, 1]), E_STRIDE), (dict(mstr=[-1, m.stride(1), 20, 4, 1]), E_STRIDE),
              (dict(mstr=[m.stride(0), -1, 20, 4, 1]), E_STRIDE),
              (dict(fstr=[-1, f.stride(1), 28, 7, 1, 0, 0]), E_STRIDE), (dict(fstr=[f.stride(0), -1, 28, 7, 1, 0, 0]), E_STRIDE),
              (dict(flags=_hip.FLAG_SEPARABLE_GRID), E_STRIDE),
              (dict(flags=_hip.FLAG_DISPLACEMENT if ops.affine else _hip.FLAG_AFFINE_GRID), E_STRIDE)]
    # one image of `moving` spans less than 4 GiB, and no stride of it reaches 2 GiB
    table += [(dict(inshp=(1 << 10, 1 << 10, 1 << 10), mstr=[0, 0, 1 << 20, 1 << 10, 1]), E_SHAPE),       # 2^32 bytes exactly
              (dict(inshp=(3, 5, 4), mstr=[0, 0, 1 << 29, 4, 1]), E_STRIDE),                              # a stride of 2^31 bytes
              (dict(dtype=F64, inshp=(1 << 9, 1 << 10, 1 << 10), mstr=[0, 0, 1 << 20, 1 << 10, 1]), E_SHAPE),
              (dict(inshp=(2, 3, 2), mstr=[0, 0, (1 << 29) - 1, (1 << 29) - 1, 1]), E_SHAPE)]             # small extents, wide strides
    # N above 2^32 - 1: the sample index is split in 32 bits
    table += [(dict(shp=big, fstr=big_f, dstr=big_d), E_SHAPE), (dict(shp=edge, fstr=edge_f, dstr=edge_d), E_SHAPE)]
    # two failures at once: the earlier check answers
    table += [(dict(dim=0, order=(9, 9, 9), B=0), E_DIM), (dict(extrapolate=3, dtype=torch.bfloat16), E_EXTRAP),
              (dict(dtype=torch.float16, B=0), E_DTYPE), (dict(B=0, flags=_hip.FLAG_SEPARABLE_GRID), E_SHAPE),
              (dict(flags=_hip.FLAG_SEPARABLE_GRID, order=(0, 0, 0)), E_STRIDE), (dict(order=(8, 8, 8), bound=7), E_ORDER),
              (dict(order=(3, 8, 3), bound=7), E_BOUND), (dict(order=(4, 4, 4), inshp=(6, 0, 4)), E_SHAPE),
              (dict(order=(4, 4, 4), mstr=[0, 0, -20, 4, 1]), E_ORDER),
              (dict(inshp=(1 << 10, 1 << 10, 1 << 10), mstr=[-1, 0, 1 << 20, 1 << 10, 1]), E_SHAPE),
              (dict(shp=big, fstr=[0, 0, 1 << 17, 2, 2, 0, 0], dstr=big_d), E_STRIDE),                    # the stride of the last dim first
              (dict(shp=big, fstr=[0, 0, 7, 2, 1, 0, 0], dstr=big_d), E_STRIDE),                          # ... the stride of a dim before the N it brings
              (dict(shp=(2, 1 << 16, 1 << 17), fstr=[0, 0, 7, 1 << 17, 1, 0, 0], dstr=[0, 3 << 33, 3 << 17, 3, 1]), E_SHAPE),   # ... N before the strides of the dims in front
              (dict(shp=big, fstr=[-1, 0, 1 << 17, 2, 1, 0, 0], dstr=big_d), E_SHAPE)]
    if not ops.affine:
        d = ops.lattice
        table += [(dict(dstr=[d.stride(0), 28, 7, 1, N]), E_STRIDE),                         # a channel-first displacement
                  (dict(dstr=[d.stride(0), 84, 21, 3, 2]), E_STRIDE), (dict(dstr=[-1, 84, 21, 3, 1]), E_STRIDE),
                  (dict(dstr=[d.stride(0), 84, 22, 3, 1]), E_STRIDE),
                  (dict(dstr=[-1, 84, 21, 3, 1], mstr=[-1, 0, 20, 4, 1]), E_STRIDE)]
    return table


def run_problem_table(ops, call, workspace, name, failures):
    for kw, want in problem_table(ops):
        rejected(call(ops.problem(**kw)), want, "%s(%s)" % (name, kw), failures)
        queried(workspace(ops.problem(**kw)), want, "%s_workspace(%s)" % (name, kw), failures)
    queried(workspace(None), E_NULL, "%s_workspace(NULL)" % name, failures)


def field_cases(name, L, failures, lcc):
    ops = Operands(3, affine=False)
    entry, query = getattr(L, name), getattr(L, name + "_workspace")
    workspace = lambda p: query(None if p is None else ctypes.byref(p))
    need = workspace(ops.problem())
    slots = 2 * 2 * 2 * 1 * 8                                            # one double per 4 x 2 x 32 box and item
    # lcc: the slots of its 1 x 1 x 1 tiles of 32 x 8 x 32, a, c, f as doubles, the pulled image
    queried(need, 2 * 1 * 8 + 3 * 2 * 3 * N * 8 + 2 * 3 * N * 4 if lcc else slots, name + "_workspace", failures)
    ws = Fake((need,), 1)
    o = ops

    def call(p, m=o.moving, f=o.fixed, u=o.lattice, w=o.weight, lo=o.loss, g=o.grad, h=o.hess, kind=2, window=(3, 5, 9), eps=1e-3,
             wbs=N, gbs=3 * N, hbs=6 * N, work=ws, nbytes=None):
        nbytes = (0 if work is None else need) if nbytes is None else nbytes
        ptrs = [address(t) for t in (m, f, u, w, lo, g, h)]
        tail = (wbs, gbs, hbs, address(work), nbytes, None)
        if lcc:
            return entry(ctypes.byref(p), *ptrs, kind, None if window is None else (ctypes.c_int * 3)(*window), eps, *tail)
        return entry(ctypes.byref(p), *ptrs, kind, *tail)

    run_problem_table(ops, call, workspace, name, failures)
    P = ops.problem
    table = [(dict(kind=-1), E_SHAPE), (dict(kind=3), E_SHAPE),
             (dict(wbs=-1), E_STRIDE), (dict(gbs=-1), E_STRIDE), (dict(hbs=-1), E_STRIDE),
             (dict(gbs=3 * N - 1), E_STRIDE), (dict(hbs=6 * N - 1), E_STRIDE),             # items of an output that overlap
             (dict(g=o.lattice), E_STRIDE),                                                # the gradient is the displacement
             (dict(g=o.moving.at(7)), E_STRIDE),                                           # ... starts inside the moving image
             (dict(h=o.fixed), E_STRIDE), (dict(lo=o.weight), E_STRIDE),
             (dict(h=o.grad, hbs=3 * N, kind=1), E_STRIDE),                                # two outputs that are one buffer
             (dict(lo=o.hess.at(11)), E_STRIDE),
             (dict(g=o.moving.at(o.moving.numel - 1)), E_STRIDE), (dict(lo=o.fixed.at(o.fixed.numel - 1)), E_STRIDE),
             (dict(g=o.weight.at(-3 * N * 2 + 1)), E_STRIDE),                              # the last element of the gradient is the first of the weight
             (dict(work=o.grad), E_STRIDE), (dict(work=o.lattice), E_STRIDE),              # the workspace is an output, an input
             (dict(work=o.loss.address - need + 8), E_STRIDE),                             # ... ends inside the loss
             (dict(work=ws.at(4)), E_STRIDE),                                              # a workspace that is not 8-byte aligned
             (dict(nbytes=need - 1), E_SCRATCH), (dict(nbytes=0), E_SCRATCH), (dict(nbytes=-1), E_SCRATCH),
             (dict(work=None, nbytes=need), E_NULL)]
    table += [({k: None}, E_NULL) for k in ("m", "f", "u", "lo", "g", "h")]
    # two at once: the Hessian kind before the strides, the strides before the NULLs, those before the alignment, that before the size
    table += [(dict(kind=3, gbs=-1), E_SHAPE), (dict(gbs=-1, g=None), E_STRIDE), (dict(m=None, work=ws.at(4)), E_NULL),
              (dict(work=ws.at(4), nbytes=0), E_STRIDE), (dict(nbytes=0, g=o.lattice), E_SCRATCH)]
    if lcc:
        table += [(dict(window=w), E_SHAPE) for w in ((3, 4, 5), (0, 3, 3), (3, 3, 11), (-1, 3, 3))]      # the window: odd, 1..9
        table += [(dict(eps=e), E_SHAPE) for e in (0.0, -1.0, float("nan"), float("inf"))]
        table += [(dict(window=None), E_NULL), (dict(window=None, kind=3), E_SHAPE), (dict(window=None, eps=0.0), E_NULL),
                  (dict(eps=0.0, window=(3, 4, 5)), E_SHAPE), (dict(window=(3, 3, 11), gbs=-1), E_SHAPE)]
    for kw, want in table:
        rejected(call(P(), **kw), want, "%s(%s)" % (name, kw), failures)
    rejected(call(P(order=(0, 0, 0)), kind=3), E_ORDER, name + ": the problem before the arguments", failures)
    # no Hessian asked for: its pointer and its stride are not looked at, the others still are
    rejected(call(P(), kind=0, h=None, hbs=-1, g=o.lattice), E_STRIDE, name + " without a Hessian", failures)
    if lcc:
        rejected(entry(None, *[None] * 7, 2, None, 1.0, 0, 0, 0, None, 0, None), E_NULL, name + "(NULL)", failures)
    else:
        rejected(entry(None, *[None] * 7, 2, 0, 0, 0, None, 0, None), E_NULL, name + "(NULL)", failures)
    # the batch of a field term: up to 2^31 - 1 (the kernels loop over gridDim.y)
    queried(workspace(P(B=65536)), need // 2 * 65536, name + "_workspace(B=65536)", failures)
    queried(workspace(P(B=(1 << 31) - 1)), need // 2 * ((1 << 31) - 1), name + "_workspace(B=2^31-1)", failures)
    # the accepting side of the limits, by the query alone: 2^32 - 4 bytes of `moving`, 2^32 - 1 samples
    queried(workspace(P(inshp=(1 << 10, 1 << 10, (1 << 10) - 1), mstr=[0, 0, 1 << 20, 1 << 10, 1])), need,
            name + "_workspace(an image of 2^32 - 4 bytes)", failures)
    almost = workspace(P(shp=(65535, 65537, 1), fstr=[0, 0, 65537, 1, 1, 0, 0], dstr=[0, 3 * 65537, 3, 3, 1]))
    if almost <= 0:
        failures.append("%s_workspace(2^32 - 1 samples): %d" % (name, almost))


def affine_cases(name, L, failures, mi):
    ops = Operands(1 if mi else 3, affine=True)
    entry, query = getattr(L, name), getattr(L, name + "_workspace")
    workspace = lambda p, nb=BINS: (query(None if p is None else ctypes.byref(p), nb) if mi
                                    else query(None if p is None else ctypes.byref(p)))
    need = workspace(ops.problem())
    sums = lambda ns: ns * 1024 * 8                                      # ns sums of 1024 workgroups per item
    tables = lambda nb: (2 * nb * nb * 8 + 8) if mi else 0               # mi: two tables and 1 / W per item
    queried(need, 2 * (tables(BINS) + sums(73)), name + "_workspace", failures)
    queried(workspace(ops.problem(dim=2, fstr=[0, 0, 4, 1, 0, 0, 0]), 64), 2 * (tables(64) + sums(25)), name + "_workspace 2-D", failures)
    queried(workspace(ops.problem(dim=1, fstr=[0, 0, 1, 0, 0, 0, 0]), 8), 2 * (tables(8) + sums(6)), name + "_workspace 1-D", failures)
    ws = Fake((need,), 1)
    o = ops

    def call(p, m=o.moving, f=o.fixed, a=o.lattice, w=o.weight, r=o.ranges, lo=o.loss, g=o.grad, h=o.hess, hi=o.hist, wh=1, nb=BINS,
             mbs=12, wbs=N, work=ws, nbytes=None):
        nbytes = (0 if work is None else need) if nbytes is None else nbytes
        tail = (mbs, wbs, address(work), nbytes, None)
        if mi:
            return entry(ctypes.byref(p), *[address(t) for t in (m, f, a, w, r, lo, g, h, hi)], wh, nb, *tail)
        return entry(ctypes.byref(p), *[address(t) for t in (m, f, a, w, lo, g, h)], wh, *tail)

    run_problem_table(ops, call, workspace, name, failures)
    P = ops.problem
    # the batch of an affine term: the item sits on gridDim.y
    rejected(call(P(B=65536)), E_SHAPE, name + "(B=65536)", failures)
    queried(workspace(P(B=65536)), E_SHAPE, name + "_workspace(B=65536)", failures)
    queried(workspace(P(B=65535)), need // 2 * 65535, name + "_workspace(B=65535)", failures)
    queried(workspace(P(inshp=(1 << 10, 1 << 10, (1 << 10) - 1), mstr=[0, 0, 1 << 20, 1 << 10, 1])), need,
            name + "_workspace(an image of 2^32 - 4 bytes)", failures)
    queried(workspace(P(shp=(65535, 65537, 1), fstr=[0, 0, 65537, 1, 1, 0, 0])), need, name + "_workspace(2^32 - 1 samples)", failures)
    table = [(dict(wh=-1), E_SHAPE), (dict(wh=2), E_SHAPE),
             (dict(mbs=-1), E_STRIDE), (dict(wbs=-1), E_STRIDE),
             (dict(g=o.lattice), E_STRIDE),                                                # the gradient is the matrix
             (dict(g=o.moving.at(7)), E_STRIDE),                                           # ... starts inside the moving image
             (dict(h=o.fixed), E_STRIDE), (dict(lo=o.weight), E_STRIDE),
             (dict(h=o.grad), E_STRIDE),                                                   # two outputs that overlap
             (dict(lo=o.hess.at(11)), E_STRIDE),
             (dict(g=o.moving.at(o.moving.numel - 1)), E_STRIDE), (dict(lo=o.fixed.at(o.fixed.numel - 1)), E_STRIDE),
             (dict(g=o.weight.at(-2 * 12 + 1)), E_STRIDE),                                 # the last element of the gradient is the first of the weight
             (dict(work=o.hess), E_STRIDE), (dict(work=o.moving), E_STRIDE),               # the workspace is an output, an input
             (dict(work=o.loss.address - need + 8), E_STRIDE),                             # ... ends inside the loss
             (dict(work=ws.at(4)), E_STRIDE),                                              # a workspace that is not 8-byte aligned
             (dict(nbytes=need - 1), E_SCRATCH), (dict(nbytes=0), E_SCRATCH), (dict(nbytes=-1), E_SCRATCH),
             (dict(work=None, nbytes=need), E_NULL)]
    table += [({k: None}, E_NULL) for k in ("m", "f", "a", "lo", "g", "h")]
    table += [(dict(wh=2, mbs=-1), E_SHAPE), (dict(mbs=-1, g=None), E_STRIDE), (dict(m=None, work=ws.at(4)), E_NULL),
              (dict(work=ws.at(4), nbytes=0), E_STRIDE), (dict(nbytes=0, g=o.lattice), E_SCRATCH)]
    if mi:
        table += [(dict(nb=nb), E_SHAPE) for nb in (7, 65, 0, -1)]                                       # 8 <= bins <= 64
        table += [(dict(hi=o.moving), E_STRIDE), (dict(lo=o.ranges), E_STRIDE),                          # the histogram, the ranges
                  (dict(hi=o.hess), E_STRIDE), (dict(r=o.ranges.address + 4), E_STRIDE),                 # ranges that are not 8-byte aligned
                  (dict(r=None), E_NULL), (dict(nb=7, wh=2), E_SHAPE), (dict(r=o.ranges.address + 4, nbytes=0), E_STRIDE)]
    for kw, want in table:
        rejected(call(P(), **kw), want, "%s(%s)" % (name, kw), failures)
    if mi:
        rejected(call(P(C=2)), E_SHAPE, name + "(C=2)", failures)                                        # one channel
        queried(workspace(P(C=2)), E_SHAPE, name + "_workspace(C=2)", failures)
        for nb in (7, 65, 0, -1):
            queried(workspace(P(), nb), E_SHAPE, name + "_workspace(bins=%d)" % nb, failures)
        rejected(call(P(C=2, order=(0, 0, 0)), nb=7), E_ORDER, name + ": the problem before the channels and the bins", failures)
        rejected(call(P(C=2), nb=7, wh=2), E_SHAPE, name + "(C=2, bins=7)", failures)
        rejected(entry(None, *[None] * 9, 1, BINS, 0, 0, None, 0, None), E_NULL, name + "(NULL)", failures)
    else:
        rejected(entry(None, *[None] * 7, 1, 0, 0, None, 0, None), E_NULL, name + "(NULL)", failures)
    rejected(call(P(order=(0, 0, 0)), wh=2), E_ORDER, name + ": the problem before the arguments", failures)
    # no Hessian asked for: its pointer is not looked at, the others still are
    rejected(call(P(), wh=0, h=None, g=o.lattice), E_STRIDE, name + " without a Hessian", failures)


@pytest.mark.parametrize("name", ["interpol_ssd", "interpol_lcc", "interpol_ssd_affine", "interpol_mi_affine"])
def test_rejections_on_the_host(name):
    L = _hip.lib()
    failures = []
    if name in ("interpol_ssd", "interpol_lcc"):
        field_cases(name, L, failures, lcc=name == "interpol_lcc")
    else:
        affine_cases(name, L, failures, mi=name == "interpol_mi_affine")
    assert not failures, "\n".join(failures)
