"""The rejections of `interpol_mi` and `interpol_mi_workspace` (csrc/mi.hip), without a device, in the manner of
tests/test_data_term_validation_cpu.py, whose fabricated operands, problem table and helpers are used here: every rejection happens
on the host before the first launch, the pointers are integers that are never dereferenced, and NO CALL HERE IS ONE THAT WOULD BE
ACCEPTED (an accepted call launches): the accepting side of a limit is pinned through the workspace query, which only computes.

The order of the checks (include/interpol_hip.h): the problem, as every field term checks it; then one channel, 8 <= bins <= 64 and a
batch of at most 65535 (INTERPOL_E_SHAPE each); then hessian_kind, the batch strides, the NULL pointers, the 8-byte alignment of the
workspace and of the ranges, the size of the workspace; last the overlap test over every input and every output, `ranges` and
`histogram` included.  Where two conditions fail at once the earlier check answers.

The workspace: two tables of bins^2 entries of 8 bytes and one double (1 / W) per item, whatever the number of dimensions.
"""
import ctypes

from interpol import _hip
import test_data_term_validation_cpu as dt
from test_data_term_validation_cpu import (E_ORDER, E_SHAPE, E_NULL, E_SCRATCH, E_STRIDE, E_DIM, BINS, N, Fake, address, rejected,
                                           queried)


def workspace_bytes(B, bins):
    return B * (2 * bins * bins * 8 + 8)


def test_rejections_on_the_host():
    L = _hip.lib()
    failures = []
    name = "interpol_mi"
    ops = dt.Operands(1, affine=False)
    entry, query = L.interpol_mi, L.interpol_mi_workspace
    workspace = lambda p, nb=BINS: query(None if p is None else ctypes.byref(p), nb)
    need = workspace(ops.problem())
    queried(need, workspace_bytes(2, BINS), name + "_workspace", failures)
    ws = Fake((need,), 1)
    o = ops

    def call(p, m=o.moving, f=o.fixed, u=o.lattice, w=o.weight, r=o.ranges, lo=o.loss, g=o.grad, h=o.hess, hi=o.hist, kind=2, nb=BINS,
             wbs=N, gbs=3 * N, hbs=6 * N, work=ws, nbytes=None):
        nbytes = (0 if work is None else need) if nbytes is None else nbytes
        return entry(ctypes.byref(p), *[address(t) for t in (m, f, u, w, r, lo, g, h, hi)], kind, nb, wbs, gbs, hbs, address(work), nbytes,
                     None)

    # the problem itself: the table of the field terms, the entry point and the query alike
    dt.run_problem_table(ops, call, workspace, name, failures)
    P = ops.problem
    # one channel, the bins, the batch: each INTERPOL_E_SHAPE, from the entry point and from the query
    rejected(call(P(C=2)), E_SHAPE, name + "(C=2)", failures)
    queried(workspace(P(C=2)), E_SHAPE, name + "_workspace(C=2)", failures)
    for nb in (7, 65, 0, -1):
        rejected(call(P(), nb=nb), E_SHAPE, name + "(bins=%d)" % nb, failures)
        queried(workspace(P(), nb), E_SHAPE, name + "_workspace(bins=%d)" % nb, failures)
    rejected(call(P(B=65536)), E_SHAPE, name + "(B=65536)", failures)
    queried(workspace(P(B=65536)), E_SHAPE, name + "_workspace(B=65536)", failures)
    queried(workspace(P(B=65535)), workspace_bytes(65535, BINS), name + "_workspace(B=65535)", failures)
    queried(workspace(P(), 8), workspace_bytes(2, 8), name + "_workspace(bins=8)", failures)
    queried(workspace(P(), 64), workspace_bytes(2, 64), name + "_workspace(bins=64)", failures)
    # the workspace does not depend on the number of dimensions
    queried(workspace(P(dim=2, fstr=[0, 0, 4, 1, 0, 0, 0], dstr=[0, 8, 2, 0, 1]), 64), workspace_bytes(2, 64), name + "_workspace 2-D", failures)
    queried(workspace(P(dim=1, fstr=[0, 0, 1, 0, 0, 0, 0], dstr=[0, 1, 0, 0, 0]), 8), workspace_bytes(2, 8), name + "_workspace 1-D", failures)
    # the accepting side of the limits of the problem, by the query alone
    queried(workspace(P(inshp=(1 << 10, 1 << 10, (1 << 10) - 1), mstr=[0, 0, 1 << 20, 1 << 10, 1])), need,
            name + "_workspace(an image of 2^32 - 4 bytes)", failures)
    queried(workspace(P(shp=(65535, 65537, 1), fstr=[0, 0, 65537, 1, 1, 0, 0], dstr=[0, 3 * 65537, 3, 3, 1])), need,
            name + "_workspace(2^32 - 1 samples)", failures)
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
             (dict(hi=o.moving), E_STRIDE), (dict(hi=o.lattice), E_STRIDE),                # the histogram is an input
             (dict(hi=o.hess), E_STRIDE), (dict(hi=o.grad.at(3 * N * 2 - 1)), E_STRIDE),   # ... an output, the end of one
             (dict(lo=o.ranges), E_STRIDE), (dict(g=o.ranges.address - (3 * N * 2 - 1) * 4), E_STRIDE),   # the ranges are read
             (dict(work=o.grad), E_STRIDE), (dict(work=o.lattice), E_STRIDE),              # the workspace is an output, an input
             (dict(work=o.hist), E_STRIDE), (dict(work=o.ranges), E_STRIDE),
             (dict(work=o.loss.address - need + 8), E_STRIDE),                             # ... ends inside the loss
             (dict(work=ws.at(4)), E_STRIDE),                                              # a workspace that is not 8-byte aligned
             (dict(r=o.ranges.address + 4), E_STRIDE),                                     # ranges that are not 8-byte aligned
             (dict(nbytes=need - 1), E_SCRATCH), (dict(nbytes=0), E_SCRATCH), (dict(nbytes=-1), E_SCRATCH),
             (dict(work=None, nbytes=need), E_NULL)]
    table += [({k: None}, E_NULL) for k in ("m", "f", "u", "r", "lo", "g", "h")]
    # two at once: the earlier check answers
    table += [(dict(nb=7, kind=3), E_SHAPE), (dict(nb=7, gbs=-1), E_SHAPE), (dict(nb=65, m=None), E_SHAPE),   # the bins before the arguments
              (dict(kind=3, gbs=-1), E_SHAPE),                                             # the Hessian kind before the strides
              (dict(gbs=-1, g=None), E_STRIDE),                                            # the strides before the NULLs
              (dict(m=None, work=ws.at(4)), E_NULL), (dict(r=None, work=ws.at(4)), E_NULL),   # the NULLs before the alignment
              (dict(work=ws.at(4), nbytes=0), E_STRIDE), (dict(r=o.ranges.address + 4, nbytes=0), E_STRIDE),   # the alignment before the size
              (dict(nbytes=0, g=o.lattice), E_SCRATCH), (dict(nbytes=need - 1, hi=o.moving), E_SCRATCH)]       # the size before the overlap
    for kw, want in table:
        rejected(call(P(), **kw), want, "%s(%s)" % (name, kw), failures)
    # the problem before the channels, the bins and the batch; those before the arguments
    rejected(call(P(C=2, order=(0, 0, 0)), nb=7), E_ORDER, name + ": the problem before the channels and the bins", failures)
    rejected(call(P(C=2, dim=4, B=65536), nb=7, kind=3), E_DIM, name + ": the problem first", failures)
    rejected(call(P(C=2), nb=7, kind=3), E_SHAPE, name + "(C=2, bins=7)", failures)
    rejected(call(P(B=65536), gbs=-1), E_SHAPE, name + ": the batch before the strides", failures)
    rejected(call(P(order=(0, 0, 0)), kind=3), E_ORDER, name + ": the problem before the arguments", failures)
    queried(workspace(P(C=2, order=(0, 0, 0)), 7), E_ORDER, name + "_workspace: the problem before the channels and the bins", failures)
    # no Hessian asked for: its pointer and its stride are not looked at, the others still are
    rejected(call(P(), kind=0, h=None, hbs=-1, g=o.lattice), E_STRIDE, name + " without a Hessian", failures)
    # no histogram asked for: the others still are
    rejected(call(P(), hi=None, g=o.lattice), E_STRIDE, name + " without a histogram", failures)
    rejected(entry(None, *[None] * 9, 2, BINS, 0, 0, 0, None, 0, None), E_NULL, name + "(NULL)", failures)
    assert not failures, "\n".join(failures)
