"""ctypes binding of libinterpol_hip.so (C-ABI: include/interpol_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; the
sampling itself runs in the hand-written gfx950 kernels of `csrc/`.  There is
NO CPU fallback: without the built library, or with CPU tensors, every
operator raises.
"""
import ctypes
import threading
import os

import torch

from .sepgrid import SeparableGrid, AffineGrid, LazyGrid

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# INTERPOL_HIP_LIB: another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("INTERPOL_HIP_LIB") or os.path.join(_PKG_ROOT, "lib", "libinterpol_hip.so")

ABI_VERSION = 1
F32, F64, BF16, F16 = 0, 1, 2, 3
FLAG_NO_FASTPATH = 1
FLAG_ACCUMULATE = 2
FLAG_FORCE_TILED = 4
FLAG_SEPARABLE_GRID = 8
FLAG_DISPLACEMENT = 16
FLAG_WITH_COUNT = 32
FLAG_BINNED_SCATTER = 64
FLAG_AUTO_SCATTER = 1 << 24
_ROUTED_2D = (torch.float32, torch.bfloat16, torch.float16)   # storage types of the 2-D bricks (csrc/scatter2d.hip)
FLAG_SMALL_TILES = 1 << 25           # (experimental, opt-in: experiments/pull_direct.hip)
FLAG_SERIAL_ITEMS = 1 << 26          # owner-computes push / count: every batch item on the caller's stream, no item chains (csrc/push_owner.hip)
FLAG_GENERAL_KERNELS = 1 << 27       # owner-computes push / count: the general own_accumulate for the colour launches too (A/B; never set by the API)
FLAG_SHELL_RUNS = 1 << 28            # owner-computes push / count: publish every run of a shell brick, a tile's few strays included (A/B; never set by the API)
FLAG_RMW_FLUSH = 1 << 29             # owner-computes push / count: load + add + store for every flushed point, no first-writer stores (A/B; never set by the API)
_POISON_SCRATCH = os.environ.get("INTERPOL_POISON_SCRATCH", "0") not in ("", "0")
_WS_NOCACHE = os.environ.get("INTERPOL_WS_NOCACHE", "0") not in ("", "0")     # (debugging aid: a fresh workspace per call, as inside a hipGraph capture)
FLAG_AFFINE_GRID = 128

# THE allocation seam: every output, workspace and scratch accumulator of this module is allocated through `_empty` (tests replace
# it to hand out poisoned, guard-banded buffers: tests/memguard.py).  The kernels write every output element, zero what they
# accumulate into and never depend on what a buffer held before the call.  (A function, not an alias: torch.empty is looked up per call.)
def _empty(*size, **kw):
    return torch.empty(*size, **kw)


def _scratch(t):
    """A workspace / scratch accumulator about to be handed to the library: every byte 0xFF (a NaN in every float) under
    INTERPOL_POISON_SCRATCH=1 -- a debugging aid, the kernels must not depend on stale workspace contents."""
    if _POISON_SCRATCH and t is not None:
        t.view(torch.uint8).fill_(0xff)
    return t


_DTYPE_CODE = {torch.float32: F32, torch.float64: F64, torch.bfloat16: BF16, torch.float16: F16}

# exported symbols, as declared in include/interpol_hip.h
SYMBOLS = (
    "interpol_pull", "interpol_push", "interpol_count", "interpol_grad", "interpol_pushgrad",
    "interpol_hess", "interpol_pull_backward", "interpol_push_backward", "interpol_count_backward",
    "interpol_spline_filter", "interpol_spline_filter_to", "interpol_resample_1d", "interpol_resample_1d_gathers", "interpol_pull_labels",
    "interpol_push_bricks", "interpol_push_bricks_workspace", "interpol_host_bound_index", "interpol_host_bound_sign",
    "interpol_host_weight", "interpol_host_weight_f32", "interpol_abi_version",
    "interpol_error_string", "interpol_kernel_name", "interpol_scatter_workspace",
    "interpol_set_handback", "interpol_release_stream", "interpol_has_experiments", "interpol_pull_workspace", "interpol_pull_ws", "interpol_push_backward_ws", "interpol_grad_ws",
    "interpol_affine_backward_workspace", "interpol_pull_backward_affine", "interpol_push_backward_affine",
    "interpol_compose", "interpol_compose_backward_right",
    "interpol_jacobian", "interpol_jacdet_backward_field",
    "interpol_regulariser", "interpol_regulariser_energy_workspace", "interpol_regulariser_energy",
    "interpol_regulariser_solve_workspace", "interpol_regulariser_solve",
    "interpol_regulariser_elastic", "interpol_regulariser_elastic_energy_workspace", "interpol_regulariser_elastic_energy",
    "interpol_regulariser_elastic_solve_workspace", "interpol_regulariser_elastic_solve",
    "interpol_regulariser_multigrid_solve_workspace", "interpol_regulariser_multigrid_solve",
    "interpol_regulariser_multigrid_cycle_workspace", "interpol_regulariser_multigrid_cycle",
    "interpol_ssd_workspace", "interpol_ssd",
    "interpol_ssd_affine_workspace", "interpol_ssd_affine",
    "interpol_mi_affine_workspace", "interpol_mi_affine",
    "interpol_mi_workspace", "interpol_mi",
    "interpol_lcc_workspace", "interpol_lcc",
    "interpol_lcc_affine_workspace", "interpol_lcc_affine",
)


class Problem(ctypes.Structure):
    """`interpol_problem` of include/interpol_hip.h."""
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("dim", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("grid_dtype", ctypes.c_int32),
        ("extrapolate", ctypes.c_int32),
        ("bound", ctypes.c_int32 * 3),
        ("order", ctypes.c_int32 * 3),
        ("flags", ctypes.c_int32),
        ("batch", ctypes.c_int64),
        ("channels", ctypes.c_int64),
        ("vol_shape", ctypes.c_int64 * 3),
        ("grid_shape", ctypes.c_int64 * 3),
        ("vol_stride", ctypes.c_int64 * 5),
        ("grid_stride", ctypes.c_int64 * 5),
        ("val_stride", ctypes.c_int64 * 7),
    ]


_lib = None


class HipExtensionMissing(ImportError):
    pass


# Workspaces of the probe-routed organisations (bricks of the target / of the image) are OPTIONAL: every operator has an
# organisation that needs none.  ONE buffer per (device, stream, HOST THREAD) is kept between calls and grown on demand (pull, push
# and the backward passes of a stream share it: their kernels are ordered by the stream.  A hipGraph capture never sees the cached
# buffer: `_optional_workspace` gives it a fresh one that belongs to the graph's pool).  The host thread is part of the key because ctypes releases the GIL inside the library: two threads issuing routed
# operators on ONE stream could otherwise interleave their kernel enqueues on one buffer (A's bin, B's header zeroing and bin, A's
# accumulate).  At most _WS_MAX buffers are kept (least recently used first out -- a warm-up on a side stream, the usual hipGraph
# recipe, does not pin a second 1 - 2 GB buffer for good); `release_workspaces()` gives them all back (call it next to
# `torch.cuda.empty_cache()`).  A miss asks torch's caching allocator, but only when the request fits
# comfortably: asking for more than it can give makes the allocator synchronise the device and flush its cache before it
# raises -- on every call, if the caller runs near capacity.  So a new buffer never takes more than half of what is available
# (free device memory + the allocator's own free blocks) and a request that failed is not repeated until noticeably more
# memory is available.  (The allocator's statistics cost ~0.25 ms of host time: they are consulted on misses only.)
_WS_CACHE = {}                                       # (device index, stream handle, host thread) -> uint8 tensor; insertion order = age
_WS_MAX = 4
_WS_DENIED = {}                                      # device index -> (bytes asked for, bytes available at the time)
_WS_CHECK_ABOVE = 64 << 20


def release_workspaces():
    """Drop the cached workspaces (they return to torch's caching allocator)."""
    _WS_CACHE.clear()
    _WS_DENIED.clear()


def _available(idx):
    free, _ = torch.cuda.mem_get_info(idx)
    return free + torch.cuda.memory_reserved(idx) - torch.cuda.memory_allocated(idx)


def _optional_workspace(nbytes, dev):
    """nbytes of device scratch, or None when the call should do without (no exception, no allocator flush)."""
    if nbytes <= 0:
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if torch.cuda.is_current_stream_capturing() or _WS_NOCACHE:
        # inside a hipGraph capture the buffer must belong to the graph (its private pool keeps it alive for the replays): a cached
        # buffer could be replaced by a larger one -- and freed -- after the capture
        try:
            return _empty(nbytes, dtype=torch.uint8, device=dev)
        except torch.cuda.OutOfMemoryError:
            return None
    key = (idx, int(torch.cuda.current_stream(dev).cuda_stream), threading.get_ident())
    ws = _WS_CACHE.get(key)
    if ws is not None and ws.numel() >= nbytes:
        _WS_CACHE[key] = _WS_CACHE.pop(key)          # (most recently used: last)
        return ws
    avail = None
    if nbytes > _WS_CHECK_ABOVE:
        if ws is not None:
            del _WS_CACHE[key]                       # (the old buffer goes back to the allocator first: it counts as available)
            ws = None
        avail = _available(idx)
        denied = _WS_DENIED.get(idx)
        if denied is not None and nbytes >= denied[0] and avail < denied[1] + denied[0] // 2:
            return None
        if 2 * nbytes > avail:
            return None
    try:
        ws = _empty(nbytes, dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError:
        _WS_DENIED[idx] = (nbytes, avail if avail is not None else _available(idx))
        return None
    if _WS_DENIED:
        _WS_DENIED.pop(idx, None)
    _WS_CACHE.pop(key, None)
    _WS_CACHE[key] = ws
    while len(_WS_CACHE) > _WS_MAX:                  # (the kernels that use an evicted buffer are enqueued: the caching allocator
        _WS_CACHE.pop(next(iter(_WS_CACHE)))         #  hands its memory to later work of the same stream only)
    return ws


def lib():
    """Load the HIP library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionMissing(
            "libinterpol_hip.so not found at %s: build it with `make -C %s -j8` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback." % (LIB_PATH, _PKG_ROOT))
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    pp = ctypes.POINTER(Problem)
    L.interpol_pull.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_grad.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_hess.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_push.argtypes = [pp, vp, vp, vp, vp, i64, vp]
    L.interpol_pushgrad.argtypes = [pp, vp, vp, vp, vp, i64, vp]
    L.interpol_count.argtypes = [pp, vp, vp, vp, i64, vp]
    L.interpol_pull_backward.argtypes = [pp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.interpol_push_backward.argtypes = [pp, vp, vp, vp, vp, vp, vp]
    L.interpol_count_backward.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_spline_filter.argtypes = [vp, i32, i64, i64, i64, i32, i32, vp]
    L.interpol_spline_filter_to.argtypes = [vp, vp, i32, i64, i64, i64, i32, i32, vp]
    L.interpol_pull_labels.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_push_bricks.argtypes = [pp, vp, vp, vp, vp, i64, vp]
    L.interpol_push_bricks.restype = ctypes.c_int
    L.interpol_push_bricks_workspace.argtypes = [pp]
    L.interpol_push_bricks_workspace.restype = i64
    L.interpol_scatter_workspace.argtypes = [pp, i32]
    L.interpol_scatter_workspace.restype = i64
    L.interpol_pull_workspace.argtypes = [pp]
    L.interpol_pull_workspace.restype = i64
    L.interpol_pull_ws.argtypes = [pp, vp, vp, vp, vp, i64, vp]
    L.interpol_pull_ws.restype = ctypes.c_int
    L.interpol_grad_ws.argtypes = [pp, vp, vp, vp, vp, i64, vp]
    L.interpol_grad_ws.restype = ctypes.c_int
    L.interpol_push_backward_ws.argtypes = [pp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.interpol_push_backward_ws.restype = ctypes.c_int
    L.interpol_affine_backward_workspace.argtypes = [pp]
    L.interpol_affine_backward_workspace.restype = i64
    L.interpol_pull_backward_affine.argtypes = [pp, vp, vp, vp, vp, vp, i64, vp]
    L.interpol_pull_backward_affine.restype = ctypes.c_int
    L.interpol_push_backward_affine.argtypes = [pp, vp, vp, vp, vp, vp, i64, vp]
    L.interpol_push_backward_affine.restype = ctypes.c_int
    L.interpol_compose.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_compose.restype = ctypes.c_int
    L.interpol_compose_backward_right.argtypes = [pp, vp, vp, vp, vp, vp]
    L.interpol_compose_backward_right.restype = ctypes.c_int
    L.interpol_jacobian.argtypes = [pp, vp, vp, i32, i32, vp]
    L.interpol_jacobian.restype = ctypes.c_int
    L.interpol_jacdet_backward_field.argtypes = [pp, vp, vp, vp, vp]
    L.interpol_jacdet_backward_field.restype = ctypes.c_int
    f64, dp = ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    L.interpol_regulariser.argtypes = [pp, vp, vp, f64, f64, f64, dp, vp]
    L.interpol_regulariser.restype = ctypes.c_int
    L.interpol_regulariser_energy_workspace.argtypes = [pp]
    L.interpol_regulariser_energy_workspace.restype = i64
    L.interpol_regulariser_energy.argtypes = [pp, vp, vp, f64, f64, f64, dp, vp, i64, vp]
    L.interpol_regulariser_energy.restype = ctypes.c_int
    L.interpol_regulariser_solve_workspace.argtypes = [pp, i32]
    L.interpol_regulariser_solve_workspace.restype = i64
    L.interpol_regulariser_solve.argtypes = [pp, vp, vp, i32, i64, vp, f64, f64, f64, dp, i32, f64, vp, vp, i64, vp]
    L.interpol_regulariser_solve.restype = ctypes.c_int
    L.interpol_regulariser_elastic.argtypes = [pp, vp, vp, dp, dp, vp]
    L.interpol_regulariser_elastic.restype = ctypes.c_int
    L.interpol_regulariser_elastic_energy_workspace.argtypes = [pp]
    L.interpol_regulariser_elastic_energy_workspace.restype = i64
    L.interpol_regulariser_elastic_energy.argtypes = [pp, vp, vp, dp, dp, vp, i64, vp]
    L.interpol_regulariser_elastic_energy.restype = ctypes.c_int
    L.interpol_regulariser_elastic_solve_workspace.argtypes = [pp, i32]
    L.interpol_regulariser_elastic_solve_workspace.restype = i64
    L.interpol_regulariser_elastic_solve.argtypes = [pp, vp, vp, i32, i64, vp, dp, dp, i32, f64, vp, vp, i64, vp]
    L.interpol_regulariser_elastic_solve.restype = ctypes.c_int
    L.interpol_regulariser_multigrid_solve_workspace.argtypes = [pp, i32]
    L.interpol_regulariser_multigrid_solve_workspace.restype = i64
    L.interpol_regulariser_multigrid_solve.argtypes = [pp, vp, vp, i32, i64, vp, dp, dp, i32, i32, f64, vp, vp, i64, vp]
    L.interpol_regulariser_multigrid_solve.restype = ctypes.c_int
    L.interpol_regulariser_multigrid_cycle_workspace.argtypes = [pp, i32]
    L.interpol_regulariser_multigrid_cycle_workspace.restype = i64
    L.interpol_regulariser_multigrid_cycle.argtypes = [pp, vp, vp, i32, i64, vp, dp, dp, i32, vp, i64, vp]
    L.interpol_regulariser_multigrid_cycle.restype = ctypes.c_int
    L.interpol_ssd_workspace.argtypes = [pp]
    L.interpol_ssd_workspace.restype = i64
    L.interpol_ssd.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i64, i64, vp, i64, vp]
    L.interpol_ssd.restype = ctypes.c_int
    L.interpol_ssd_affine_workspace.argtypes = [pp]
    L.interpol_ssd_affine_workspace.restype = i64
    L.interpol_ssd_affine.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i64, vp, i64, vp]
    L.interpol_ssd_affine.restype = ctypes.c_int
    L.interpol_mi_affine_workspace.argtypes = [pp, i32]
    L.interpol_mi_affine_workspace.restype = i64
    L.interpol_mi_affine.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, i64, vp, i64, vp]
    L.interpol_mi_affine.restype = ctypes.c_int
    L.interpol_mi_workspace.argtypes = [pp, i32]
    L.interpol_mi_workspace.restype = i64
    L.interpol_mi.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, i64, i64, vp, i64, vp]
    L.interpol_mi.restype = ctypes.c_int
    L.interpol_lcc_workspace.argtypes = [pp]
    L.interpol_lcc_workspace.restype = i64
    L.interpol_lcc.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, i32, ctypes.POINTER(ctypes.c_int), ctypes.c_double, i64, i64, i64, vp, i64, vp]
    L.interpol_lcc.restype = ctypes.c_int
    L.interpol_lcc_affine_workspace.argtypes = [pp]
    L.interpol_lcc_affine_workspace.restype = i64
    L.interpol_lcc_affine.argtypes = [pp, vp, vp, vp, vp, vp, vp, vp, i32, ctypes.POINTER(ctypes.c_int), ctypes.c_double, i64, i64, vp, i64, vp]
    L.interpol_lcc_affine.restype = ctypes.c_int
    L.interpol_set_handback.argtypes = [i32]
    L.interpol_set_handback.restype = i32
    L.interpol_release_stream.argtypes = [ctypes.c_void_p]
    L.interpol_release_stream.restype = i32
    L.interpol_resample_1d.argtypes = [i32, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, vp, vp, vp, vp]
    L.interpol_resample_1d_gathers.argtypes = [i32, i64, i64]
    L.interpol_resample_1d_gathers.restype = i32
    for name in ("interpol_pull", "interpol_grad", "interpol_hess", "interpol_push", "interpol_pushgrad",
                 "interpol_count", "interpol_pull_backward", "interpol_push_backward",
                 "interpol_count_backward", "interpol_spline_filter", "interpol_spline_filter_to", "interpol_resample_1d", "interpol_pull_labels"):
        getattr(L, name).restype = ctypes.c_int
    L.interpol_host_bound_index.argtypes = [i32, i32, i32]
    L.interpol_host_bound_index.restype = i32
    L.interpol_host_bound_sign.argtypes = [i32, i32, i32]
    L.interpol_host_bound_sign.restype = i32
    L.interpol_host_weight.argtypes = [i32, ctypes.c_double, i32]
    L.interpol_host_weight.restype = ctypes.c_double
    L.interpol_host_weight_f32.argtypes = [i32, ctypes.c_float, i32]
    L.interpol_host_weight_f32.restype = ctypes.c_float
    L.interpol_abi_version.restype = i32
    L.interpol_error_string.argtypes = [ctypes.c_int]
    L.interpol_error_string.restype = ctypes.c_char_p
    L.interpol_kernel_name.argtypes = [pp, ctypes.c_char_p]
    L.interpol_kernel_name.restype = ctypes.c_char_p
    if L.interpol_abi_version() != ABI_VERSION:
        raise HipExtensionMissing("libinterpol_hip.so has ABI version %d, expected %d: rebuild it"
                                  % (L.interpol_abi_version(), ABI_VERSION))
    _lib = L
    return L


def _check(rc, what):
    if rc == 0:
        return
    msg = lib().interpol_error_string(rc).decode()
    if rc == -2:
        raise NotImplementedError("%s: %s" % (what, msg))          # reference interpol/splines.py:80
    if rc == -8:
        raise NotImplementedError("%s: %s" % (what, msg))          # reference interpol/coeff.py:243-244
    if rc in (-1, -3, -5, -7):
        raise ValueError("%s: %s" % (what, msg))
    raise RuntimeError("%s failed: %s (code %d)" % (what, msg, rc))


def _require_gpu(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "interpol (MI355X build): tensors must live on a ROCm GPU; got a %s tensor. "
                "This build has no CPU path." % t.device.type)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("interpol: all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def common_dtypes(img, grid):
    """Storage / coordinate dtypes the kernels run in.
    (f32, f32), (f64, f64), (bf16|f16 image, f32 coordinates); anything else is
    promoted the way the reference's elementwise ops would."""
    if not grid.dtype.is_floating_point:
        raise TypeError("grid must be a floating point tensor")
    idt = img.dtype if img is not None else grid.dtype
    if not idt.is_floating_point:
        raise TypeError("image must be a floating point tensor")
    if idt == torch.float64 or grid.dtype == torch.float64:
        return torch.float64, torch.float64
    if idt in (torch.bfloat16, torch.float16):
        return idt, torch.float32
    return torch.float32, torch.float32


def _spatially_contiguous(t, first_spatial):
    """True when dims [first_spatial:] are row-major contiguous."""
    expect = 1
    for d in range(t.dim() - 1, first_spatial - 1, -1):
        if t.shape[d] > 1 and t.stride(d) != expect:
            return False
        expect *= t.shape[d]
    return True


def _bstride(t, B):
    """Batch stride with broadcasting of a singleton batch."""
    return 0 if (t.shape[0] == 1 and B > 1) else t.stride(0)


def make_problem(dim, dtype, grid_dtype, bound, order, extrapolate, B, C, vol_shape, grid_shape,
                 vol_stride, grid_stride, val_stride, flags=0):
    p = Problem()
    p.abi_version = ABI_VERSION
    p.dim = dim
    p.dtype = _DTYPE_CODE[dtype]
    p.grid_dtype = _DTYPE_CODE[grid_dtype]
    p.extrapolate = int(extrapolate)
    for d in range(3):
        p.bound[d] = int(bound[d]) if d < dim else 1
        p.order[d] = int(order[d]) if d < dim else 0
        p.vol_shape[d] = int(vol_shape[d]) if d < dim else 1
        p.grid_shape[d] = int(grid_shape[d]) if d < dim else 1
    p.flags = flags
    p.batch, p.channels = int(B), int(C)
    for i, s in enumerate(vol_stride):
        p.vol_stride[i] = int(s)
    for i, s in enumerate(grid_stride):
        p.grid_stride[i] = int(s)
    for i, s in enumerate(val_stride):
        p.val_stride[i] = int(s)
    return p


def _dense_strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= int(s)
    return list(reversed(st))


def _pad_to(lst, n, fill=0):
    return list(lst) + [fill] * (n - len(lst))


def _grid_strides(grid, B, dim):
    if isinstance(grid, _PackedLattice):
        return [0] * 5
    return [_bstride(grid, B)] + _pad_to([grid.stride(1 + d) for d in range(dim)], 3) + [grid.stride(-1)]


class _PackedLattice:
    """A SeparableGrid prepared for the C-ABI: the packed coordinate vectors + the shape the
    host code sees, (1, *out, D).  Adds INTERPOL_FLAG_SEPARABLE_GRID to the call."""

    def __init__(self, sep, gdt):
        self.buf = sep.packed(gdt)
        self.shape = sep.shape

    def data_ptr(self):
        return self.buf.data_ptr()

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n


def _prep_grid(grid, gdt):
    """-> (grid object to pass on, extra flags)."""
    if isinstance(grid, LazyGrid):
        return _PackedLattice(grid, gdt), (FLAG_AFFINE_GRID if isinstance(grid, AffineGrid) else FLAG_SEPARABLE_GRID)
    grid = grid.to(gdt)
    if not _spatially_contiguous(grid, 1):
        grid = grid.contiguous()
    return grid, 0


def gather(op, vol, grid, bound, order, extrapolate, flags=0, out=None):
    """pull / grad / hess: vol (B,C,*in), grid (B,*out,D) -> val (B,C,*out[,D[,D]]).
    `out`: a dense tensor of that shape and dtype to write into instead of allocating one."""
    dev = _require_gpu(vol, grid)
    dim = grid.shape[-1]
    if dim not in (1, 2, 3):
        raise NotImplementedError("interpol (MI355X build): only 1-D, 2-D and 3-D grids are supported")
    dt, gdt = common_dtypes(vol, grid)
    out_dt = dt
    if op in ("hess",) and dt in (torch.bfloat16, torch.float16):
        dt = torch.float32                                 # second-order operator: f32 / f64 kernels only
    vol = vol.to(dt)
    grid, gflag = _prep_grid(grid, gdt)
    flags |= gflag
    routed = False
    lin3 = op == "pull" and dim == 3 and dt in (torch.bfloat16, torch.float16) and gdt == torch.float32 and all(int(o) == 1 for o in order[:3])   # trilinear: routed in 16 bits too
    if (((op in ("pull", "grad") and dim == 3 and dt == torch.float32) or lin3 or (op == "pull" and dim == 2 and dt in _ROUTED_2D and gdt == torch.float32))
            and not (flags & (FLAG_NO_FASTPATH | FLAG_FORCE_TILED | FLAG_BINNED_SCATTER)) and (flags >> 8) == 0):
        # the router of the pull (csrc/push_owner.hip: own_gather; 2-D: csrc/scatter2d.hip: gather2d): like the push's, see interpol/backend.py
        from . import backend
        if backend.rough_deformations is None:
            flags |= FLAG_AUTO_SCATTER
        elif backend.rough_deformations:
            flags |= FLAG_BINNED_SCATTER
    if op in ("pull", "grad") and (flags & (FLAG_AUTO_SCATTER | FLAG_BINNED_SCATTER)):
        routed = True
    B = max(vol.shape[0], grid.shape[0])
    C = vol.shape[1]
    oshape = list(grid.shape[1:-1])
    trailing = {"pull": [], "grad": [dim], "hess": [dim, dim]}[op]
    if out is None:
        val = _empty([B, C] + oshape + trailing, dtype=dt, device=dev)
    else:
        val = out
        if not (val.is_contiguous() and val.dtype == dt and list(val.shape) == [B, C] + oshape + trailing):
            raise ValueError("gather output: expected a contiguous %s tensor of shape %s, got %s %s"
                             % (dt, [B, C] + oshape + trailing, val.dtype, list(val.shape)))
    if val.numel() == 0:
        return val.to(out_dt)
    vstr = [_bstride(vol, B), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    valstr = [val.stride(0), val.stride(1)] + _pad_to([val.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, vol.shape[2:], oshape,
                     vstr, _grid_strides(grid, B, dim), valstr, flags)
    L = lib()
    if routed:
        # workspace of the routed pull (18 B per sample + 2 KiB per brick of the image; 0: the organisation does not apply).  When
        # it cannot be allocated the call is the plain interpol_pull: the sample tiles need none.
        wbytes = int(L.interpol_pull_workspace(ctypes.byref(p)))
        ws = _scratch(_optional_workspace(wbytes, dev))
        if ws is not None:
            with torch.cuda.device(dev):
                rc = (L.interpol_pull_ws if op == "pull" else L.interpol_grad_ws)(ctypes.byref(p), _ptr(vol), _ptr(grid), _ptr(val), _ptr(ws), wbytes, _stream(dev))
            _check(rc, "interpol_%s_ws" % op)
            return val.to(out_dt)
        p.flags &= ~(FLAG_AUTO_SCATTER | FLAG_BINNED_SCATTER)
    fn = getattr(L, "interpol_" + op)
    with torch.cuda.device(dev):
        rc = fn(ctypes.byref(p), _ptr(vol), _ptr(grid), _ptr(val), _stream(dev))
    _check(rc, "interpol_" + op)
    return val.to(out_dt)


def scatter(op, val, grid, shape, bound, order, extrapolate, flags=0, out=None, shared=False, with_count=False, need_workspace=False):
    """push / count / pushgrad: val (B,C,*in[,D]) , grid (B,*in,D) -> vol (B,C,*shape).
    `out` (dense, same dtype) + FLAG_ACCUMULATE adds into an existing target.
    `shared=True`: ONE target (1,C,*shape) that all batch items accumulate into
    (the reference's grid_push(...).sum(0), without the B per-item volumes).
    `with_count=True` (push only): the target has C + 1 channels and channel C receives the count
    image of the same grid, splatted in the same pass (INTERPOL_FLAG_WITH_COUNT).
    `need_workspace=True`: return None (nothing launched) when the probe-routed organisation's workspace is denied, so that the caller
    can pick another organisation instead of the tiles."""
    dev = _require_gpu(val, grid)
    dim = grid.shape[-1]
    if dim not in (1, 2, 3):
        raise NotImplementedError("interpol (MI355X build): only 1-D, 2-D and 3-D grids are supported")
    from . import backend
    if backend.want_exact_scatter():
        flags |= FLAG_NO_FASTPATH                       # float atomics, like the reference's scatter_add_
    elif op in ("push", "count") and not (flags & (FLAG_NO_FASTPATH | FLAG_FORCE_TILED | FLAG_BINNED_SCATTER)) and (flags >> 8) == 0:
        if backend.rough_deformations is None:
            flags |= FLAG_AUTO_SCATTER                  # a probe of this call picks tiles or owner-computes (csrc/push_owner.hip)
        elif backend.rough_deformations:
            flags |= FLAG_BINNED_SCATTER                # owner-computes organisation, always
    dt, gdt = common_dtypes(val, grid)
    out_dt = dt
    if op == "pushgrad" and dt in (torch.bfloat16, torch.float16):
        dt = torch.float32
    grid, gflag = _prep_grid(grid, gdt)
    flags |= gflag
    gshape = list(grid.shape[1:-1])
    if shape is None:
        shape = gshape
    shape = [int(s) for s in shape]
    if op == "count":
        B, C = grid.shape[0], 1
        valstr = [0] * 7
    else:
        val = val.to(dt)
        if not _spatially_contiguous(val, 2):
            val = val.contiguous()
        B = max(val.shape[0], grid.shape[0])
        C = val.shape[1]
        valstr = [_bstride(val, B), val.stride(1)] + _pad_to([val.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    Bv = 1 if shared else B
    if with_count:
        if op != "push":
            raise ValueError("with_count applies to push only")
        flags |= FLAG_WITH_COUNT
    Cv = C + (1 if with_count else 0)
    if out is None:
        vol = _empty([Bv, Cv] + shape, dtype=dt, device=dev)
    else:
        vol = out
        if not (vol.is_contiguous() and vol.dtype == dt and list(vol.shape) == [Bv, Cv] + shape):
            raise ValueError("scatter target: expected a contiguous %s tensor of shape %s, got %s %s"
                             % (dt, [Bv, Cv] + shape, vol.dtype, list(vol.shape)))
        if (flags & FLAG_ACCUMULATE) and dt in (torch.bfloat16, torch.float16):
            raise ValueError("FLAG_ACCUMULATE needs a float32 / float64 target (a low-precision target is narrowed once, not accumulated)")
    if vol.numel() == 0:
        return vol.to(out_dt)
    if grid.numel() == 0:
        return vol.zero_().to(out_dt) if out is None else vol
    vstr = [0 if shared else vol.stride(0), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, shape, gshape,
                     vstr, _grid_strides(grid, B, dim), valstr, flags)
    L = lib()
    # scratch: the fp32 accumulator of a 16-bit target, followed by the workspace of the binned
    # organisation when the library wants one for this problem (interpol_hip.h)
    scratch, sbytes = None, 0
    if op in ("push", "count"):
        sbytes = int(L.interpol_scatter_workspace(ctypes.byref(p), 1 if op == "count" else 0))
    if dt in (torch.bfloat16, torch.float16):
        sbytes = max(sbytes, vol.numel() * 4)
    if sbytes > 0:
        if flags & FLAG_AUTO_SCATTER:
            # The probe-routed default asks for the owner-computes workspace (~22 B per sample + 1 KiB per brick, api.py)
            # whether or not the probe will pick that organisation; when it does not fit comfortably (_optional_workspace), the
            # call falls back to the tiles, which need none -- a push that fitted without the router still fits.
            scratch = _optional_workspace(sbytes, dev)
            if scratch is None and need_workspace:
                return None
            if scratch is None:
                flags &= ~FLAG_AUTO_SCATTER
                p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, shape, gshape,
                                 vstr, _grid_strides(grid, B, dim), valstr, flags)
                sbytes = int(L.interpol_scatter_workspace(ctypes.byref(p), 1 if op == "count" else 0))
                if dt in (torch.bfloat16, torch.float16):
                    sbytes = max(sbytes, vol.numel() * 4)
                scratch = _empty(sbytes, dtype=torch.uint8, device=dev) if sbytes > 0 else None
        else:
            scratch = _empty(sbytes, dtype=torch.uint8, device=dev)
        _scratch(scratch)
    with torch.cuda.device(dev):
        if op == "count":
            rc = L.interpol_count(ctypes.byref(p), _ptr(grid), _ptr(vol), _ptr(scratch), sbytes, _stream(dev))
        else:
            rc = getattr(L, "interpol_" + op)(ctypes.byref(p), _ptr(val), _ptr(grid), _ptr(vol),
                                              _ptr(scratch), sbytes, _stream(dev))
    _check(rc, "interpol_" + op)
    return vol.to(out_dt)


def pull_backward(gout, vol, grid, bound, order, extrapolate, need_vol, need_grid, flags=0):
    """Fused backward of pull: (grad_vol (B,C,*in) | None, grad_grid (B,*out,D) | None)."""
    dev = _require_gpu(gout, vol, grid)
    dim = grid.shape[-1]
    from . import backend
    if (need_vol and flags == 0 and dim == 3 and torch.is_tensor(grid) and len(set(order[:3])) == 1
            and order[0] in (0, 1, 2, 3)
            and vol.dtype == torch.float32 and gout.dtype == torch.float32 and grid.dtype == torch.float32
            and vol.shape[0] == grid.shape[0] == gout.shape[0] and not backend.want_exact_scatter()
            and backend.rough_deformations is not False):
        # 3-D quadratic / cubic: the image gradient IS grid_push of grad_out (pushpull.py:252-255) and the library computes it
        # with the push kernels anyway; through `scatter` it also gets the push's routing (rough / folding fields take the
        # owner-computes organisation: 31 -> 10 ms for the backward of a field of 8 voxels amplitude)
        # (trilinear and nearest neighbour as well -- trilinear, sigma = 6: 15.9 -> 3.1 ms; nearest, sigma = 2: 5.7 -> 2.5 ms.  The library
        # splits every backward since round 5: its fused tile kernel for both gradients was wrong under rough fields)
        gvol = scatter("push", gout, grid, list(vol.shape[2:]), bound, order, extrapolate)
        ggrid = pull_backward(gout, vol, grid, bound, order, extrapolate, False, True, flags)[1] if need_grid else None
        return gvol, ggrid
    if (need_vol and flags == 0 and dim == 2 and torch.is_tensor(grid) and 1 <= min(order[:2]) and max(order[:2]) <= 3
            and vol.dtype == gout.dtype and vol.dtype in _ROUTED_2D and grid.dtype == torch.float32
            and vol.shape[0] == grid.shape[0] == gout.shape[0]
            and not backend.want_exact_scatter() and backend.rough_deformations is not False):
        # 2-D, orders 1..3: the library splits this backward into a push of grad_out and the contracted grid gradient anyway
        # (csrc/abi.hip: interpol_pull_backward); through `scatter` the push gets its router (csrc/scatter2d.hip), and so does
        # the grid gradient below
        gvol = scatter("push", gout, grid, list(vol.shape[2:]), bound, order, extrapolate)
        ggrid = pull_backward(gout, vol, grid, bound, order, extrapolate, False, True, flags)[1] if need_grid else None
        return gvol, ggrid
    if (need_vol and flags == 0 and dim == 3 and torch.is_tensor(grid) and max(order[:3]) <= 3 and max(order[:3]) > 0
            and vol.dtype == gout.dtype == grid.dtype == torch.float64 and vol.shape[0] == grid.shape[0] == gout.shape[0]
            and grid[0, ..., 0].numel() >= 4096 and not backend.want_exact_scatter()):
        # float64, orders <= 3: the same split -- the image gradient through the float64 LDS tiles of grid_push (csrc/push_f64.hip)
        # instead of one scattered global atomic per tap inside the fused kernel (1 x 2 x 128^3, sigma = 2: 12.7 -> 2 ms)
        gvol = scatter("push", gout, grid, list(vol.shape[2:]), bound, order, extrapolate)
        ggrid = pull_backward(gout, vol, grid, bound, order, extrapolate, False, True, flags)[1] if need_grid else None
        return gvol, ggrid
    if backend.want_exact_scatter() and need_vol:
        flags |= FLAG_NO_FASTPATH                       # grad_vol is a scatter
    dt, gdt = common_dtypes(vol, grid)
    vol = vol.to(dt)
    gout = gout.to(dt)
    grid_c, gflag = _prep_grid(grid, gdt)
    flags |= gflag
    if gflag and need_grid:
        raise RuntimeError("interpol: a SeparableGrid / AffineGrid is a constant lattice, it has no gradient")
    if not _spatially_contiguous(vol, 2):
        vol = vol.contiguous()
    if not _spatially_contiguous(gout, 2):
        gout = gout.contiguous()
    B = max(vol.shape[0], grid_c.shape[0])
    C = vol.shape[1]
    ishape = list(vol.shape[2:])
    oshape = list(grid_c.shape[1:-1])
    gvol = _empty([B, C] + ishape, dtype=dt, device=dev) if need_vol else None
    ggrid = _empty([B] + oshape + [dim], dtype=gdt, device=dev) if need_grid else None
    if gout.numel() == 0:
        return (gvol.zero_() if need_vol else None), ggrid
    scratch, sbytes = None, 0
    if need_vol and dt in (torch.bfloat16, torch.float16):
        scratch = _scratch(_empty(gvol.numel(), dtype=torch.float32, device=dev))
        sbytes = scratch.numel() * 4
    vstr = [_bstride(vol, B), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    valstr = [_bstride(gout, B), gout.stride(1)] + _pad_to([gout.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    routed = 0
    high = dim == 3 and all(int(o) == int(order[0]) for o in order[:3]) and int(order[0]) in (4, 5)   # image gradient through scatter5
    two_d = dim == 2 and need_grid and dt in _ROUTED_2D and (not need_vol or dt == torch.float32)   # (a 16-bit image gradient keeps `scratch` for its accumulator)
    if ((((need_grid or (need_vol and high)) and dim == 3 and dt == torch.float32) or two_d) and gdt == torch.float32 and (flags >> 8) == 0
            and not (flags & (FLAG_NO_FASTPATH | FLAG_FORCE_TILED | FLAG_BINNED_SCATTER))):
        # the grid gradient takes the router of the pull (csrc/push_owner.hip: own_gather<K, true>): tiles whose samples leave the
        # LDS box go to the bricks of the image; the workspace rides in the `scratch` argument (interpol_hip.h)
        routed = FLAG_AUTO_SCATTER if backend.rough_deformations is None else (FLAG_BINNED_SCATTER if backend.rough_deformations else 0)
    elif (need_grid or (need_vol and high)) and (flags & FLAG_BINNED_SCATTER) and (dim == 3 or two_d) and sbytes == 0:
        # (sbytes != 0: `scratch` is the float32 accumulator of a 16-bit image gradient, which no bricks workspace may replace -- the
        #  library then serves the call with the tiles and the generic kernels, as it does for 16-bit storage anyway)
        routed = FLAG_BINNED_SCATTER
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, ishape, oshape,
                     vstr, _grid_strides(grid_c, B, dim), valstr, flags | routed)
    if routed:
        wbytes = int(lib().interpol_pull_workspace(ctypes.byref(p)))
        scratch = _scratch(_optional_workspace(wbytes, dev))
        sbytes = wbytes if scratch is not None else 0
        if scratch is None:
            p.flags &= ~(FLAG_AUTO_SCATTER | FLAG_BINNED_SCATTER)
    with torch.cuda.device(dev):
        rc = lib().interpol_pull_backward(ctypes.byref(p), _ptr(gout), _ptr(vol), _ptr(grid_c), _ptr(gvol),
                                          _ptr(ggrid), _ptr(scratch), sbytes, _stream(dev))
    _check(rc, "interpol_pull_backward")
    return gvol, ggrid


def push_backward(gvol_out, val, grid, bound, order, extrapolate, need_val, need_grid, flags=0):
    """Fused backward of push (val given) or count (val None):
    (grad_val (B,C,*in) | None, grad_grid (B,*in,D) | None)."""
    dev = _require_gpu(gvol_out, val, grid)
    dim = grid.shape[-1]
    dt, gdt = common_dtypes(gvol_out, grid)
    gvol_out = gvol_out.to(dt)
    grid_c, gflag = _prep_grid(grid, gdt)
    flags |= gflag
    if gflag and need_grid:
        raise RuntimeError("interpol: a SeparableGrid / AffineGrid is a constant lattice, it has no gradient")
    gshape = list(grid_c.shape[1:-1])
    B = max(gvol_out.shape[0], grid_c.shape[0])
    C = gvol_out.shape[1]
    count = val is None
    if not count:
        val = val.to(dt)
        if not val.is_contiguous():
            val = val.contiguous()
        B = max(B, val.shape[0])
        if val.shape[0] != B:
            val = val.expand([B] + list(val.shape[1:])).contiguous()
    gval = _empty([B, C] + gshape, dtype=dt, device=dev) if (need_val and not count) else None
    ggrid = _empty([B] + gshape + [dim], dtype=gdt, device=dev) if need_grid else None
    if grid_c.numel() == 0 or (gval is None and ggrid is None):
        return gval, ggrid
    vstr = [_bstride(gvol_out, B), gvol_out.stride(1)] + _pad_to([gvol_out.stride(2 + d) for d in range(dim)], 3)
    dense = _dense_strides([B, C] + gshape)
    valstr = dense[:2] + _pad_to(dense[2:], 3) + [0, 0]
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, gvol_out.shape[2:], gshape,
                     vstr, _grid_strides(grid_c, B, dim), valstr, flags)
    L = lib()
    from . import backend
    routed = 0
    if (((dim == 3 and dt == torch.float32) or (dim == 2 and dt in _ROUTED_2D)) and gdt == torch.float32 and (flags >> 8) == 0
            and not (flags & (FLAG_NO_FASTPATH | FLAG_FORCE_TILED | FLAG_BINNED_SCATTER))):
        # both gradients are gathers: they take the router of the pull (bricks of the image, csrc/push_owner.hip: own_gather)
        routed = FLAG_AUTO_SCATTER if backend.rough_deformations is None else (FLAG_BINNED_SCATTER if backend.rough_deformations else 0)
    elif flags & FLAG_BINNED_SCATTER:
        routed = FLAG_BINNED_SCATTER
    if routed:
        p.flags |= routed
        wbytes = int(L.interpol_pull_workspace(ctypes.byref(p)))
        ws = _scratch(_optional_workspace(wbytes, dev))
        if ws is not None:
            with torch.cuda.device(dev):
                rc = L.interpol_push_backward_ws(ctypes.byref(p), _ptr(gvol_out), _ptr(None if count else val), _ptr(grid_c),
                                                 _ptr(gval), _ptr(ggrid), _ptr(ws), wbytes, _stream(dev))
            _check(rc, "interpol_push_backward_ws")
            return gval, ggrid
        p.flags &= ~(FLAG_AUTO_SCATTER | FLAG_BINNED_SCATTER)
    with torch.cuda.device(dev):
        if count:
            rc = L.interpol_count_backward(ctypes.byref(p), _ptr(gvol_out), _ptr(grid_c), _ptr(ggrid), _stream(dev))
        else:
            rc = L.interpol_push_backward(ctypes.byref(p), _ptr(gvol_out), _ptr(val), _ptr(grid_c),
                                          _ptr(gval), _ptr(ggrid), _stream(dev))
    _check(rc, "interpol_push_backward")
    return gval, ggrid


def _affine_lattice(lattice, gdt):
    if not isinstance(lattice, AffineGrid):
        raise TypeError("interpol: the gradient of a lattice's matrix needs an AffineGrid, got %s" % type(lattice).__name__)
    return _PackedLattice(lattice, gdt)


def _affine_reduce(entry, p, a, b, grid_c, gdt, dim, dev):
    """The two launches of csrc/affine_grad.hip -> grad_mat (D, D+1).  The workspace (one row of D (D+1) doubles per persistent
    workgroup, 192 KiB in 3-D) is a plain allocation: too small for the workspace cache, and it then belongs to a captured graph."""
    L = lib()
    wbytes = int(L.interpol_affine_backward_workspace(ctypes.byref(p)))
    if wbytes < 0:
        _check(wbytes, "interpol_affine_backward_workspace")
    ws = _scratch(_empty(wbytes, dtype=torch.uint8, device=dev))
    gmat = _empty([dim, dim + 1], dtype=gdt, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(L, entry)(ctypes.byref(p), _ptr(a), _ptr(b), _ptr(grid_c), _ptr(gmat), _ptr(ws), wbytes, _stream(dev))
    _check(rc, entry)
    return gmat


def affine_pull_backward(gout, vol, lattice, bound, order, extrapolate, flags=0):
    """Gradient of grid_pull(vol, AffineGrid(mat, shape)) with respect to `mat`: gout (B,C,*shape), vol (B,C,*in) -> (D, D+1) in the
    coordinate dtype, summed over the batch (interpol_pull_backward_affine)."""
    dev = _require_gpu(gout, vol, lattice)
    dim = lattice.shape[-1]
    dt, gdt = common_dtypes(vol, lattice)
    grid_c = _affine_lattice(lattice, gdt)
    vol = vol.to(dt)
    gout = gout.to(dt)
    if not _spatially_contiguous(gout, 2):
        gout = gout.contiguous()
    B = max(vol.shape[0], gout.shape[0])
    C = vol.shape[1]
    oshape = list(grid_c.shape[1:-1])
    if gout.numel() == 0:
        return torch.zeros([dim, dim + 1], dtype=gdt, device=dev)
    vstr = [_bstride(vol, B), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    valstr = [_bstride(gout, B), gout.stride(1)] + _pad_to([gout.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, list(vol.shape[2:]), oshape,
                     vstr, [0] * 5, valstr, flags | FLAG_AFFINE_GRID)
    return _affine_reduce("interpol_pull_backward_affine", p, gout, vol, grid_c, gdt, dim, dev)


def affine_push_backward(gvol_out, val, lattice, bound, order, extrapolate, flags=0):
    """Gradient of grid_push(val, AffineGrid(mat, inshape), shape) -- val None: of grid_count -- with respect to `mat`:
    gvol_out (B,C,*shape), val (B,C,*inshape) -> (D, D+1), summed over the batch (interpol_push_backward_affine)."""
    dev = _require_gpu(gvol_out, val, lattice)
    dim = lattice.shape[-1]
    dt, gdt = common_dtypes(gvol_out, lattice)
    grid_c = _affine_lattice(lattice, gdt)
    gvol_out = gvol_out.to(dt)
    gshape = list(grid_c.shape[1:-1])
    B = gvol_out.shape[0]
    C = gvol_out.shape[1]
    if val is not None:
        val = val.to(dt)
        if not _spatially_contiguous(val, 2):
            val = val.contiguous()
        B = max(B, val.shape[0])
        valstr = [_bstride(val, B), val.stride(1)] + _pad_to([val.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    else:
        valstr = [0] * 7
    if grid_c.numel() == 0 or gvol_out.numel() == 0:
        return torch.zeros([dim, dim + 1], dtype=gdt, device=dev)
    vstr = [_bstride(gvol_out, B), gvol_out.stride(1)] + _pad_to([gvol_out.stride(2 + d) for d in range(dim)], 3)
    p = make_problem(dim, dt, gdt, bound, order, extrapolate, B, C, gvol_out.shape[2:], gshape,
                     vstr, [0] * 5, valstr, flags | FLAG_AFFINE_GRID)
    return _affine_reduce("interpol_push_backward_affine", p, gvol_out, val, grid_c, gdt, dim, dev)


def compose_covered(left, right, order):
    """Does interpol_compose take these fields?  (csrc/compose.hip: D <= 3, one order 1..3, float32 / float64 fields of one dtype)"""
    dim = right.shape[-1]
    order = [int(o) for o in list(order)[:dim]]
    return (left.is_cuda and right.is_cuda and 1 <= dim <= 3 and left.shape[-1] == dim
            and left.dtype == right.dtype and left.dtype in (torch.float32, torch.float64)
            and len(set(order)) == 1 and 1 <= order[0] <= 3)


def _byte_range(t):
    span = 1 + sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


def _overlap(a, b):
    if a.numel() == 0 or b.numel() == 0:
        return False
    (a0, a1), (b0, b1) = _byte_range(a), _byte_range(b)
    return a0 < b1 and b0 < a1


def _point_by_point(t):
    return t if _spatially_contiguous(t, 1) else t.contiguous()


def _compose_problem(left, right, out, bound, order, extrapolate):
    """left (B|1,*lshape,D), right (B|1,*oshape,D), out (B,*oshape,D): all point by point (include/interpol_hip.h)"""
    dim = right.shape[-1]
    B = out.shape[0]
    lstr = [_bstride(left, B), 1] + _pad_to([left.stride(1 + d) for d in range(dim)], 3)
    vstr = [out.stride(0), 1] + _pad_to([out.stride(1 + d) for d in range(dim)], 3) + [0, 0]
    return make_problem(dim, right.dtype, right.dtype, bound, order, extrapolate, B, dim, left.shape[1:-1], right.shape[1:-1],
                        lstr, _grid_strides(right, B, dim), vstr, 0)


def compose(left, right, bound, order, extrapolate, out=None):
    """interpol_compose: left (B|1,*lshape,D), right (B|1,*oshape,D) -> right + pull(left, id + right), (B,*oshape,D).
    `out`: a dense tensor of that shape and dtype to write into; it may be `right` itself, it must not share memory with `left`."""
    dev = _require_gpu(left, right)
    if not compose_covered(left, right, order):
        raise NotImplementedError("interpol_compose: D <= 3, one order 1..3, float32 / float64 fields of one dtype only")
    dim = right.shape[-1]
    left, right = _point_by_point(left), _point_by_point(right)
    B = max(left.shape[0], right.shape[0])
    shape = [B] + list(right.shape[1:])
    if out is None:
        out = _empty(shape, dtype=right.dtype, device=dev)
    else:
        if not (out.is_contiguous() and out.dtype == right.dtype and list(out.shape) == shape and out.device == dev):
            raise ValueError("compose output: expected a contiguous %s tensor of shape %s, got %s %s"
                             % (right.dtype, shape, out.dtype, list(out.shape)))
        if _overlap(out, left):
            raise ValueError("compose output must not share memory with `left` (other samples gather from it); it may be `right`")
    if out.numel() == 0:
        return out
    p = _compose_problem(left, right, out, bound, order, extrapolate)
    with torch.cuda.device(dev):
        rc = lib().interpol_compose(ctypes.byref(p), _ptr(left), _ptr(right), _ptr(out), _stream(dev))
    _check(rc, "interpol_compose")
    return out


def compose_backward_right(gout, left, right, bound, order, extrapolate):
    """interpol_compose_backward_right: gout (B,*oshape,D) -> the gradient of compose(left, right) with respect to `right`,
    one per batch item of gout (B,*oshape,D): the caller sums over the batch when `right` was broadcast."""
    dev = _require_gpu(gout, left, right)
    if not compose_covered(left, right, order) or gout.dtype != right.dtype:
        raise NotImplementedError("interpol_compose_backward_right: D <= 3, one order 1..3, float32 / float64 fields of one dtype only")
    left, right = _point_by_point(left), _point_by_point(right)
    gout = gout.contiguous()
    gright = _empty(list(gout.shape), dtype=gout.dtype, device=dev)
    if gright.numel() == 0:
        return gright
    p = _compose_problem(left, right, gright, bound, order, extrapolate)
    with torch.cuda.device(dev):
        rc = lib().interpol_compose_backward_right(ctypes.byref(p), _ptr(gout), _ptr(left), _ptr(right), _ptr(gright), _stream(dev))
    _check(rc, "interpol_compose_backward_right")
    return gright


def jacobian_covered(disp, order):
    """Does interpol_jacobian take this field?  (csrc/jacobian.hip: (B,*shape,D) with D <= 3, one order 1..3, float32 / float64)"""
    dim = disp.shape[-1]
    order = [int(o) for o in list(order)[:dim]]
    return (disp.is_cuda and 1 <= dim <= 3 and disp.dim() == dim + 2 and disp.dtype in (torch.float32, torch.float64)
            and len(set(order)) == 1 and 1 <= order[0] <= 3)


def _jacobian_problem(disp, out, bound, order):
    """disp (B,*shape,D) point by point, out dense with a batch stride (include/interpol_hip.h)"""
    dim = disp.shape[-1]
    dstr = [disp.stride(0), 1] + _pad_to([disp.stride(1 + d) for d in range(dim)], 3)
    shape = disp.shape[1:-1]
    return make_problem(dim, disp.dtype, disp.dtype, bound, order, 1, disp.shape[0], dim, shape, shape,
                        dstr, [0] * 5, [out.stride(0)] + [0] * 6, 0)


def jacobian(disp, bound, order, det_only=False, add_identity=True, out=None):
    """interpol_jacobian: disp (B,*shape,D) -> the Jacobian of id + disp at the lattice points, (B,*shape,D,D) (row = component,
    column = direction; `add_identity=False`: of disp alone), or with `det_only` its determinant, (B,*shape).
    A field that is not point by point is made dense first.  `out`: a dense tensor of that shape and dtype to write into; it
    must not share memory with `disp`, which every lattice point gathers from."""
    dev = _require_gpu(disp)
    if not jacobian_covered(disp, order):
        raise NotImplementedError("interpol_jacobian: (B,*shape,D) with D <= 3, one order 1..3, float32 / float64 only")
    dim = disp.shape[-1]
    disp = _point_by_point(disp)
    shape = list(disp.shape[:-1]) + ([] if det_only else [dim, dim])
    if out is None:
        out = _empty(shape, dtype=disp.dtype, device=dev)
    elif not (out.is_contiguous() and out.dtype == disp.dtype and list(out.shape) == shape and out.device == dev):
        raise ValueError("jacobian output: expected a contiguous %s tensor of shape %s, got %s %s"
                         % (disp.dtype, shape, out.dtype, list(out.shape)))
    if _overlap(out, disp):
        raise ValueError("jacobian output must not share memory with the displacement field (other lattice points gather from it)")
    if out.numel() == 0:
        return out
    p = _jacobian_problem(disp, out, bound, order)
    with torch.cuda.device(dev):
        rc = lib().interpol_jacobian(ctypes.byref(p), _ptr(disp), _ptr(out), int(bool(det_only)), int(bool(add_identity)), _stream(dev))
    _check(rc, "interpol_jacobian")
    return out


def jacdet_backward_field(gout, disp, bound, order):
    """interpol_jacdet_backward_field: gout (B,*shape), disp (B,*shape,D) -> gout * cofactor(jacobian(disp)) in the layout
    `pushgrad` reads, (B,D,*shape,D): pushed along a zero displacement it is the gradient of the determinant."""
    dev = _require_gpu(gout, disp)
    if not jacobian_covered(disp, order) or gout.dtype != disp.dtype or list(gout.shape) != list(disp.shape[:-1]):
        raise NotImplementedError("interpol_jacdet_backward_field: (B,*shape,D) with D <= 3, one order 1..3, float32 / float64, "
                                  "and a gradient (B,*shape) of the same dtype only")
    dim = disp.shape[-1]
    disp = _point_by_point(disp)
    gout = gout.contiguous()
    gfield = _empty([disp.shape[0], dim] + list(disp.shape[1:]), dtype=disp.dtype, device=dev)
    if gfield.numel() == 0:
        return gfield
    p = _jacobian_problem(disp, gfield, bound, order)
    with torch.cuda.device(dev):
        rc = lib().interpol_jacdet_backward_field(ctypes.byref(p), _ptr(gout), _ptr(disp), _ptr(gfield), _stream(dev))
    _check(rc, "interpol_jacdet_backward_field")
    return gfield


def regulariser_covered(field):
    """Does interpol_regulariser take this field?  (csrc/regulariser.hip: (B,*shape,D) with D <= 3, float32 / float64)"""
    dim = field.shape[-1]
    return field.is_cuda and 1 <= dim <= 3 and field.dim() == dim + 2 and field.dtype in (torch.float32, torch.float64)


def _regulariser_problem(field, bound, out_stride):
    """field (B,*shape,D) point by point, L v dense with a batch stride (include/interpol_hip.h)"""
    dim = field.shape[-1]
    fstr = [field.stride(0), 1] + _pad_to([field.stride(1 + d) for d in range(dim)], 3)
    shape = field.shape[1:-1]
    return make_problem(dim, field.dtype, field.dtype, bound, [0] * dim, 1, field.shape[0], dim, shape, shape,
                        fstr, [0] * 5, [out_stride] + [0] * 6, 0)


def _regulariser_weights(weights, voxel_size, dim):
    absolute, membrane, bending = (float(x) for x in weights)
    vx = (ctypes.c_double * 3)(*_pad_to([float(h) for h in voxel_size][:dim], 3, 1.0))
    return absolute, membrane, bending, vx


BOUND_SLIDING = 7                                                # INTERPOL_BOUND_SLIDING: the interpol_regulariser_elastic* entry points only


def _regulariser_elastic(weights, bound):
    """None where the three-term entry points serve the call (three weights, or shears = div = 0, and no sliding dimension);
    else the five weights as a host array for the interpol_regulariser_elastic* entry points"""
    if not any(weights[3:]) and BOUND_SLIDING not in bound:
        return None
    return (ctypes.c_double * 5)(*_pad_to([float(x) for x in weights], 5, 0.0))


def regulariser(field, weights, voxel_size, bound, out=None):
    """interpol_regulariser: field (B,*shape,D) -> L field, (B,*shape,D).  weights = (absolute, membrane, bending), not all zero,
    or five with (shears, div) (interpol_regulariser_elastic, as is every call with a sliding dimension, code 7);
    voxel_size: D positive numbers; bound: D codes.  A field that is not point by point is made dense first.  `out`: a dense
    tensor of that shape and dtype to write into; it must not share memory with `field`, which every lattice point gathers from."""
    dev = _require_gpu(field)
    if not regulariser_covered(field):
        raise NotImplementedError("interpol_regulariser: (B,*shape,D) with D <= 3, float32 / float64 only")
    dim = field.shape[-1]
    field = _point_by_point(field)
    shape = list(field.shape)
    if out is None:
        out = _empty(shape, dtype=field.dtype, device=dev)
    elif not (out.is_contiguous() and out.dtype == field.dtype and list(out.shape) == shape and out.device == dev):
        raise ValueError("regulariser output: expected a contiguous %s tensor of shape %s, got %s %s"
                         % (field.dtype, shape, out.dtype, list(out.shape)))
    if _overlap(out, field):
        raise ValueError("regulariser output must not share memory with the field (other lattice points gather from it)")
    if out.numel() == 0:
        return out
    p = _regulariser_problem(field, bound, out.stride(0))
    a, m, b, vx = _regulariser_weights(weights[:3], voxel_size, dim)
    w5 = _regulariser_elastic(weights, bound)
    with torch.cuda.device(dev):
        if w5 is None:
            rc = lib().interpol_regulariser(ctypes.byref(p), _ptr(field), _ptr(out), a, m, b, vx, _stream(dev))
        else:
            rc = lib().interpol_regulariser_elastic(ctypes.byref(p), _ptr(field), _ptr(out), w5, vx, _stream(dev))
    _check(rc, "interpol_regulariser" if w5 is None else "interpol_regulariser_elastic")
    return out


def regulariser_energy(field, weights, voxel_size, bound):
    """interpol_regulariser_energy: field (B,*shape,D) -> 0.5 <field, L field> per batch item, (B) in the dtype of the field.
    The workspace (8 KiB per batch item) comes from the workspace cache of this module; inside a hipGraph capture it is a fresh
    buffer of the graph's pool."""
    dev = _require_gpu(field)
    if not regulariser_covered(field):
        raise NotImplementedError("interpol_regulariser_energy: (B,*shape,D) with D <= 3, float32 / float64 only")
    dim = field.shape[-1]
    field = _point_by_point(field)
    if field.numel() == 0:
        return _empty([field.shape[0]], dtype=field.dtype, device=dev).zero_()
    L = lib()
    p = _regulariser_problem(field, bound, 0)
    w5 = _regulariser_elastic(weights, bound)
    wbytes = int((L.interpol_regulariser_energy_workspace if w5 is None else L.interpol_regulariser_elastic_energy_workspace)(ctypes.byref(p)))
    if wbytes < 0:
        _check(wbytes, "interpol_regulariser_energy_workspace")
    ws = _scratch(_optional_workspace(wbytes, dev))
    if ws is None:                                   # (8 KiB per item: only an allocator that is out of memory denies it)
        raise torch.cuda.OutOfMemoryError("interpol_regulariser_energy: no memory for a workspace of %d bytes" % wbytes)
    energy = _empty([field.shape[0]], dtype=field.dtype, device=dev)
    a, m, b, vx = _regulariser_weights(weights[:3], voxel_size, dim)
    with torch.cuda.device(dev):
        if w5 is None:
            rc = L.interpol_regulariser_energy(ctypes.byref(p), _ptr(field), _ptr(energy), a, m, b, vx, _ptr(ws), wbytes, _stream(dev))
        else:
            rc = L.interpol_regulariser_elastic_energy(ctypes.byref(p), _ptr(field), _ptr(energy), w5, vx, _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_regulariser_energy" if w5 is None else "interpol_regulariser_elastic_energy")
    return energy


def regulariser_solve_covered(gradient, hessian=None):
    """Does interpol_regulariser_solve take these?  (csrc/regulariser_solve.hip: a gradient that interpol_regulariser takes, and no
    Hessian or one (B|1,*shape,K) of the same dtype and device with K = D (diagonal) or D (D + 1) / 2 (symmetric))"""
    if not regulariser_covered(gradient):
        return False
    if hessian is None:
        return True
    dim = gradient.shape[-1]
    return (hessian.is_cuda and hessian.device == gradient.device and hessian.dtype == gradient.dtype and hessian.dim() == dim + 2
            and hessian.shape[0] in (1, gradient.shape[0]) and list(hessian.shape[1:-1]) == list(gradient.shape[1:-1])
            and hessian.shape[-1] in (dim, dim * (dim + 1) // 2))


def regulariser_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance):
    """interpol_regulariser_solve: gradient (B,*shape,D), hessian None or (B|1,*shape,K) -> (x, info): x (B,*shape,D) after at most
    `max_iter` preconditioned conjugate-gradient iterations on (H + L) x = gradient, info (B,2) float64 = (iterations, relative
    residual) per item.  bound: D codes out of zero, dct2, dst2, dft.  Nothing synchronises: every iteration is enqueued here and
    the stopping test stays on the device.  A gradient that is not point by point and a Hessian that is not dense are made dense
    first; a Hessian with a batch of 1 serves every item (batch stride 0).  The workspace (three fields, the reduction slots, the
    scalars of the items) comes from the workspace cache of this module; inside a hipGraph capture it is a fresh buffer of the
    graph's pool."""
    dev = _require_gpu(gradient, hessian)
    if not regulariser_solve_covered(gradient, hessian):
        raise NotImplementedError("interpol_regulariser_solve: a gradient (B,*shape,D) with D <= 3, float32 / float64, and no Hessian "
                                  "or one (B|1,*shape,K) of the same dtype with K = D or D (D + 1) / 2 only")
    dim = gradient.shape[-1]
    gradient = _point_by_point(gradient)
    B = gradient.shape[0]
    x = _empty(list(gradient.shape), dtype=gradient.dtype, device=dev)
    info = _empty([B, 2], dtype=torch.float64, device=dev)
    if x.numel() == 0:
        return x, info.zero_()
    K, hstride = 0, 0
    if hessian is not None:
        hessian = hessian.contiguous()
        K = hessian.shape[-1]
        hstride = hessian.stride(0) if hessian.shape[0] == B and B > 1 else 0
    L = lib()
    p = _regulariser_problem(gradient, bound, 0)
    w5 = _regulariser_elastic(weights, bound)
    wbytes = int((L.interpol_regulariser_solve_workspace if w5 is None else L.interpol_regulariser_elastic_solve_workspace)(ctypes.byref(p), K))
    if wbytes < 0:
        _check(wbytes, "interpol_regulariser_solve_workspace")
    ws = _scratch(_optional_workspace(wbytes, dev))
    if ws is None:
        raise torch.cuda.OutOfMemoryError("interpol_regulariser_solve: no memory for a workspace of %d bytes" % wbytes)
    a, m, b, vx = _regulariser_weights(weights[:3], voxel_size, dim)
    with torch.cuda.device(dev):
        if w5 is None:
            rc = L.interpol_regulariser_solve(ctypes.byref(p), _ptr(gradient), _ptr(hessian), K, hstride, _ptr(x), a, m, b, vx,
                                              int(max_iter), float(tolerance), _ptr(info), _ptr(ws), wbytes, _stream(dev))
        else:
            rc = L.interpol_regulariser_elastic_solve(ctypes.byref(p), _ptr(gradient), _ptr(hessian), K, hstride, _ptr(x), w5, vx,
                                                      int(max_iter), float(tolerance), _ptr(info), _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_regulariser_solve" if w5 is None else "interpol_regulariser_elastic_solve")
    return x, info


def _multigrid_call(name, field, hessian, weights, voxel_size, bound, smoothing, tail):
    """What interpol_regulariser_multigrid_solve and _cycle share: the dense operands, the problem, the five host weights, the
    workspace and the call.  field: the gradient / residual (B,*shape,D); tail(info) -> the arguments between `smoothing` and the
    workspace.  -> (out (B,*shape,D), info (B,2) float64)"""
    dev = _require_gpu(field, hessian)
    if not regulariser_solve_covered(field, hessian):
        raise NotImplementedError("%s: a field (B,*shape,D) with D <= 3, float32 / float64, and no Hessian or one (B|1,*shape,K) of "
                                  "the same dtype with K = D or D (D + 1) / 2 only" % name)
    dim = field.shape[-1]
    field = _point_by_point(field)
    B = field.shape[0]
    out = _empty(list(field.shape), dtype=field.dtype, device=dev)
    info = _empty([B, 2], dtype=torch.float64, device=dev)
    if out.numel() == 0:
        return out, info.zero_()
    K, hstride = 0, 0
    if hessian is not None:
        hessian = hessian.contiguous()
        K = hessian.shape[-1]
        hstride = hessian.stride(0) if hessian.shape[0] == B and B > 1 else 0
    L = lib()
    p = _regulariser_problem(field, bound, 0)
    wbytes = int(getattr(L, name + "_workspace")(ctypes.byref(p), K))
    if wbytes < 0:
        _check(wbytes, name + "_workspace")
    ws = _scratch(_optional_workspace(wbytes, dev))
    if ws is None:
        raise torch.cuda.OutOfMemoryError("%s: no memory for a workspace of %d bytes" % (name, wbytes))
    w5 = (ctypes.c_double * 5)(*_pad_to([float(x) for x in weights], 5, 0.0))
    vx = _regulariser_weights(weights[:3], voxel_size, dim)[3]
    with torch.cuda.device(dev):
        rc = getattr(L, name)(ctypes.byref(p), _ptr(field), _ptr(hessian), K, hstride, _ptr(out), w5, vx, int(smoothing), *tail(info),
                              _ptr(ws), wbytes, _stream(dev))
    _check(rc, name)
    return out, info


def regulariser_multigrid_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing):
    """interpol_regulariser_multigrid_solve: `regulariser_solve` with one multigrid V-cycle as the preconditioner of the conjugate
    gradients (csrc/regulariser_multigrid.hip) -> (x, info).  Nothing synchronises; the workspace (five fields, the slots, the
    scalars and the levels of the cycle with their Hessian pyramid) comes from the workspace cache of this module."""
    return _multigrid_call("interpol_regulariser_multigrid_solve", gradient, hessian, weights, voxel_size, bound, smoothing,
                           lambda info: (int(max_iter), float(tolerance), _ptr(info)))


def regulariser_multigrid_cycle(residual, hessian, weights, voxel_size, bound, smoothing):
    """interpol_regulariser_multigrid_cycle: z = V(residual), one V-cycle alone, (B,*shape,D)"""
    return _multigrid_call("interpol_regulariser_multigrid_cycle", residual, hessian, weights, voxel_size, bound, smoothing,
                           lambda info: ())[0]


SSD_HESSIAN_KINDS = {None: 0, 'diagonal': 1, 'full': 2}               # hessian_kind of interpol_ssd


def ssd_covered(moving, fixed, disp, weight, order):
    """Does interpol_ssd take these?  (csrc/ssd.hip: D <= 3, one order 1..3, float32 / float64 tensors of one dtype on one GPU)"""
    dim = disp.shape[-1]
    order = [int(o) for o in list(order)[:dim]]
    tensors = [t for t in (moving, fixed, disp, weight) if t is not None]
    return (all(t.is_cuda and t.device == disp.device and t.dtype == disp.dtype for t in tensors)
            and disp.dtype in (torch.float32, torch.float64) and 1 <= dim <= 3
            and moving.dim() == dim + 2 and fixed.dim() == dim + 2 and disp.dim() == dim + 2
            and len(set(order)) == 1 and 1 <= order[0] <= 3)


def _ssd_problem(moving, fixed, disp, bound, order, extrapolate, B):
    """moving (B|1,C,*inshape) with any strides, fixed (B|1,C,*shape) spatially row-major, disp (B|1,*shape,D) point by point
    (include/interpol_hip.h: interpol_ssd)"""
    dim = disp.shape[-1]
    mstr = [_bstride(moving, B), moving.stride(1)] + _pad_to([moving.stride(2 + d) for d in range(dim)], 3)
    fstr = [_bstride(fixed, B), fixed.stride(1)] + _pad_to([fixed.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    return make_problem(dim, disp.dtype, disp.dtype, bound, order, extrapolate, B, moving.shape[1], moving.shape[2:], disp.shape[1:-1],
                        mstr, _grid_strides(disp, B, dim), fstr, 0)


def _data_term_operands(entry, moving, fixed, lattice, weight, bound, order, extrapolate, affine, C="C", extra=None):
    """The operands of a fused data term as its entry point takes them; `lattice` is disp (B|1,*shape,D) or, `affine`, mat
    (B|1,D,D+1).  A `fixed` / `weight` that is not row-major over the sample lattice, a `disp` that is not point by point and a
    matrix that is not dense are made dense; an operand with a batch of 1 serves every item (batch stride 0).  The library sees
    pointers and one set of extents: what the tensors really hold is checked here (extra: f(B) -> (ok, what, got) adds one more
    operand to the check and to its message).
    -> fixed, lattice, weight, B, shape, the batch stride of the weight, and the problem -- None when there is no sample (the
    sums are empty)."""
    if affine:
        dim = lattice.shape[-1] - 1
        if not _spatially_contiguous(lattice, 1):
            lattice = lattice.contiguous()
    else:
        dim = lattice.shape[-1]
        lattice = _point_by_point(lattice)
    if not _spatially_contiguous(fixed, 2):
        fixed = fixed.contiguous()
    B = max(moving.shape[0], fixed.shape[0], lattice.shape[0], 1 if weight is None else weight.shape[0])
    shape = list(fixed.shape[2:]) if affine else list(lattice.shape[1:-1])
    ok, what, got = extra(B) if extra else (True, "", [])
    if ((lattice.shape[1] != dim if affine else list(fixed.shape[2:]) != shape) or fixed.shape[1] != moving.shape[1]
            or (weight is not None and list(weight.shape[1:]) != shape)
            or any(t.shape[0] not in (1, B) for t in (moving, fixed, lattice, weight) if t is not None) or not ok):
        got = [list(moving.shape), list(fixed.shape), list(lattice.shape), None if weight is None else list(weight.shape)] + got
        raise ValueError("%s: moving (B|1,%s,*inshape), fixed (B|1,%s,*shape), %s, weight (B|1,*shape)%s, got %s"
                         % (entry, C, C, "mat (B|1,D,D+1)" if affine else "disp (B|1,*shape,D)", what, ", ".join("%s" % (g,) for g in got)))
    wstride = 0
    if weight is not None:
        if not _spatially_contiguous(weight, 1):
            weight = weight.contiguous()
        wstride = _bstride(weight, B)
    # no sample: an affine term looks at `fixed` (no channel is no sample either), a field term at its gradient (B,*shape,D)
    if (fixed.numel() == 0) if affine else (0 in [B] + shape):
        return fixed, lattice, weight, B, shape, wstride, None
    if moving.numel() == 0:                          # (samples, and nothing to sample: there is no stencil to speak of)
        raise ValueError("%s: `moving` is empty, %s, while the lattice of `fixed` has points" % (entry, list(moving.shape)))
    if affine:
        mstr = [_bstride(moving, B), moving.stride(1)] + _pad_to([moving.stride(2 + d) for d in range(dim)], 3)
        fstr = [_bstride(fixed, B), fixed.stride(1)] + _pad_to([fixed.stride(2 + d) for d in range(dim)], 3) + [0, 0]
        p = make_problem(dim, lattice.dtype, lattice.dtype, bound, order, extrapolate, B, moving.shape[1], moving.shape[2:], shape,
                         mstr, [0] * 5, fstr, FLAG_AFFINE_GRID)
    else:
        p = _ssd_problem(moving, fixed, lattice, bound, order, extrapolate, B)
    return fixed, lattice, weight, B, shape, wstride, p


def _data_term_workspace(entry, dev, p, *args):
    """The workspace of `entry` for the problem `p` (args: what its `_workspace` query takes besides), from the workspace cache of
    this module -> (buffer, bytes).  These workspaces are small next to the images: only an allocator that is out of memory
    denies one."""
    wbytes = int(getattr(lib(), entry + "_workspace")(ctypes.byref(p), *args))
    if wbytes < 0:
        _check(wbytes, entry + "_workspace")
    ws = _scratch(_optional_workspace(wbytes, dev))
    if ws is None:
        raise torch.cuda.OutOfMemoryError("%s: no memory for a workspace of %d bytes" % (entry, wbytes))
    return ws, wbytes


def ssd(moving, fixed, disp, weight, bound, order, extrapolate, hessian):
    """interpol_ssd: moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape) -> (loss (B),
    gradient (B,*shape,D), hessian (B,*shape,K) | None) of 0.5 sum weight (moving(id + disp) - fixed)^2 with respect to `disp`;
    hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2).  `moving` is read through its strides; a `fixed` / `weight` that
    is not row-major over the lattice and a `disp` that is not point by point are made dense first; an operand with a batch of 1
    serves every item (batch stride 0).  The workspace (one double per workgroup) comes from the workspace cache of this module;
    inside a hipGraph capture it is a fresh buffer of the graph's pool."""
    dev = _require_gpu(moving, fixed, disp, weight)
    if not ssd_covered(moving, fixed, disp, weight, order):
        raise NotImplementedError("interpol_ssd: D <= 3, one order 1..3, float32 / float64 tensors of one dtype only")
    if hessian not in SSD_HESSIAN_KINDS:
        raise ValueError("interpol_ssd: hessian is None, 'diagonal' or 'full', got %r" % (hessian,))
    dim = disp.shape[-1]
    kind = SSD_HESSIAN_KINDS[hessian]
    K = (0, dim, dim * (dim + 1) // 2)[kind]
    fixed, disp, weight, B, shape, wstride, p = _data_term_operands("interpol_ssd", moving, fixed, disp, weight, bound, order, extrapolate,
                                                                     affine=False)
    loss = _empty([B], dtype=disp.dtype, device=dev)
    gradient = _empty([B] + shape + [dim], dtype=disp.dtype, device=dev)
    hess = _empty([B] + shape + [K], dtype=disp.dtype, device=dev) if K else None
    if p is None:                                    # (no sample: the sums are empty)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if K else None)
    ws, wbytes = _data_term_workspace("interpol_ssd", dev, p)
    with torch.cuda.device(dev):
        rc = lib().interpol_ssd(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(disp), _ptr(weight), _ptr(loss), _ptr(gradient),
                                _ptr(hess), kind, wstride, gradient.stride(0), hess.stride(0) if K else 0, _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_ssd")
    return loss, gradient, hess


LCC_MAX_WINDOW = 9                                                    # csrc/lcc.hip: RMAX = 4


def lcc_covered(moving, fixed, disp, weight, order, window):
    """Does interpol_lcc take these?  (csrc/lcc.hip: what interpol_ssd takes, and odd windows 1..9)"""
    dim = disp.shape[-1]
    window = [int(w) for w in list(window)[:dim]]
    return (ssd_covered(moving, fixed, disp, weight, order) and len(window) == dim
            and all(1 <= w <= LCC_MAX_WINDOW and w % 2 == 1 for w in window))


def lcc(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps):
    """interpol_lcc: moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape) -> (loss (B),
    gradient (B,*shape,D), hessian (B,*shape,K) | None) of the local normalised cross-correlation with respect to `disp`;
    hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2); window: D odd ints 1..9; eps > 0.  The operands are taken as
    by `ssd`.  The workspace (the pulled image, three fields of doubles and one double per workgroup) comes from the workspace cache of this
    module; inside a hipGraph capture it is a fresh buffer of the graph's pool."""
    dev = _require_gpu(moving, fixed, disp, weight)
    if not lcc_covered(moving, fixed, disp, weight, order, window):
        raise NotImplementedError("interpol_lcc: D <= 3, one order 1..3, float32 / float64 tensors of one dtype, odd windows 1..9 only")
    if hessian not in SSD_HESSIAN_KINDS:
        raise ValueError("interpol_lcc: hessian is None, 'diagonal' or 'full', got %r" % (hessian,))
    dim = disp.shape[-1]
    kind = SSD_HESSIAN_KINDS[hessian]
    K = (0, dim, dim * (dim + 1) // 2)[kind]
    fixed, disp, weight, B, shape, wstride, p = _data_term_operands("interpol_lcc", moving, fixed, disp, weight, bound, order, extrapolate,
                                                                     affine=False)
    loss = _empty([B], dtype=disp.dtype, device=dev)
    gradient = _empty([B] + shape + [dim], dtype=disp.dtype, device=dev)
    hess = _empty([B] + shape + [K], dtype=disp.dtype, device=dev) if K else None
    if p is None:                                    # (no sample: the sums are empty)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if K else None)
    ws, wbytes = _data_term_workspace("interpol_lcc", dev, p)
    win = (ctypes.c_int * 3)(*_pad_to([int(w) for w in list(window)[:dim]], 3, 1))
    with torch.cuda.device(dev):
        rc = lib().interpol_lcc(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(disp), _ptr(weight), _ptr(loss), _ptr(gradient),
                                _ptr(hess), kind, win, float(eps), wstride, gradient.stride(0), hess.stride(0) if K else 0, _ptr(ws),
                                wbytes, _stream(dev))
    _check(rc, "interpol_lcc")
    return loss, gradient, hess


# The two affine terms and the dense mutual-information term put the batch item on gridDim.y without a loop: the library refuses
# more items than a launch has rows of workgroups (csrc/data_term.hpp: problem_params, csrc/mi.hip: mi_params) with INTERPOL_E_SHAPE.
MAX_ITEMS_ON_ROWS = 65535


def _items(*tensors):
    return max(t.shape[0] for t in tensors if t is not None)


def ssd_affine_covered(moving, fixed, mat, weight, order):
    """Does interpol_ssd_affine take these?  (csrc/ssd_affine.hip: D <= 3, one order 1..3, float32 / float64 tensors of one dtype on
    one GPU; mat (B|1, D, D+1); at most MAX_ITEMS_ON_ROWS items)"""
    dim = mat.shape[-1] - 1
    order = [int(o) for o in list(order)[:dim]]
    tensors = [t for t in (moving, fixed, mat, weight) if t is not None]
    return (all(t.is_cuda and t.device == mat.device and t.dtype == mat.dtype for t in tensors)
            and mat.dtype in (torch.float32, torch.float64) and 1 <= dim <= 3
            and moving.dim() == dim + 2 and fixed.dim() == dim + 2 and mat.dim() == 3
            and len(set(order)) == 1 and 1 <= order[0] <= 3 and _items(*tensors) <= MAX_ITEMS_ON_ROWS)


def ssd_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian=True):
    """interpol_ssd_affine: moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B),
    gradient (B,D,D+1), hessian (B,P,P) | None, P = D (D+1)) of 0.5 sum weight (moving(A o + t) - fixed)^2 with respect to the matrix
    of each item.  `moving` is read through its strides; a `fixed` / `weight` that is not row-major over the lattice and a matrix
    that is not dense are made dense first; an operand with a batch of 1 serves every item (batch stride 0).  The workspace (73
    x 1024 doubles per item in 3-D) comes from the workspace cache of this module; inside a hipGraph capture it is a fresh buffer of
    the graph's pool."""
    dev = _require_gpu(moving, fixed, mat, weight)
    if not ssd_affine_covered(moving, fixed, mat, weight, order):
        raise NotImplementedError("interpol_ssd_affine: D <= 3, one order 1..3, float32 / float64 tensors of one dtype only")
    dim = mat.shape[-1] - 1
    P = dim * (dim + 1)
    fixed, mat, weight, B, shape, wstride, p = _data_term_operands("interpol_ssd_affine", moving, fixed, mat, weight, bound, order,
                                                                    extrapolate, affine=True)
    loss = _empty([B], dtype=mat.dtype, device=dev)
    gradient = _empty([B, dim, dim + 1], dtype=mat.dtype, device=dev)
    hess = _empty([B, P, P], dtype=mat.dtype, device=dev) if hessian else None
    if p is None:                                    # (no sample: the sums are empty)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if hessian else None)
    ws, wbytes = _data_term_workspace("interpol_ssd_affine", dev, p)
    with torch.cuda.device(dev):
        rc = lib().interpol_ssd_affine(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(mat), _ptr(weight), _ptr(loss), _ptr(gradient),
                                       _ptr(hess), 1 if hessian else 0, _bstride(mat, B), wstride, _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_ssd_affine")
    return loss, gradient, hess


def lcc_affine_covered(moving, fixed, mat, weight, order, window):
    """Does interpol_lcc_affine take these?  (csrc/lcc_affine.hip: D <= 3, one order 1..3, float32 / float64 tensors of one dtype on
    one GPU; mat (B|1, D, D+1); odd windows 1..9.  Its kernels walk the batch in a loop: no cap on the items.)"""
    dim = mat.shape[-1] - 1
    order = [int(o) for o in list(order)[:dim]]
    window = [int(w) for w in list(window)[:dim]]
    tensors = [t for t in (moving, fixed, mat, weight) if t is not None]
    return (all(t.is_cuda and t.device == mat.device and t.dtype == mat.dtype for t in tensors)
            and mat.dtype in (torch.float32, torch.float64) and 1 <= dim <= 3
            and moving.dim() == dim + 2 and fixed.dim() == dim + 2 and mat.dim() == 3
            and len(set(order)) == 1 and 1 <= order[0] <= 3
            and len(window) == dim and all(1 <= w <= LCC_MAX_WINDOW and w % 2 == 1 for w in window))


def lcc_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian=True, window=(9, 9, 9), eps=1e-5):
    """interpol_lcc_affine: moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B),
    gradient (B,D,D+1), hessian (B,P,P) | None, P = D (D+1)) of the local normalised cross-correlation between moving(A o + t) and
    fixed with respect to the matrix of each item; window: D odd ints 1..9; eps > 0.  The operands are taken as by `ssd_affine`.  The
    workspace (the pulled image, dI and C per sample, three fields of doubles, one double per workgroup and 73 x 1024 doubles per
    item in 3-D) comes from the workspace cache of this module; inside a hipGraph capture it is a fresh buffer of the graph's pool."""
    dev = _require_gpu(moving, fixed, mat, weight)
    if not lcc_affine_covered(moving, fixed, mat, weight, order, window):
        raise NotImplementedError("interpol_lcc_affine: D <= 3, one order 1..3, float32 / float64 tensors of one dtype, odd windows "
                                  "1..9 only")
    dim = mat.shape[-1] - 1
    P = dim * (dim + 1)
    fixed, mat, weight, B, shape, wstride, p = _data_term_operands("interpol_lcc_affine", moving, fixed, mat, weight, bound, order,
                                                                    extrapolate, affine=True)
    loss = _empty([B], dtype=mat.dtype, device=dev)
    gradient = _empty([B, dim, dim + 1], dtype=mat.dtype, device=dev)
    hess = _empty([B, P, P], dtype=mat.dtype, device=dev) if hessian else None
    if p is None:                                    # (no sample: the sums are empty)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if hessian else None)
    ws, wbytes = _data_term_workspace("interpol_lcc_affine", dev, p)
    win = (ctypes.c_int * 3)(*_pad_to([int(w) for w in list(window)[:dim]], 3, 1))
    with torch.cuda.device(dev):
        rc = lib().interpol_lcc_affine(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(mat), _ptr(weight), _ptr(loss), _ptr(gradient),
                                       _ptr(hess), 1 if hessian else 0, win, float(eps), _bstride(mat, B), wstride, _ptr(ws), wbytes,
                                       _stream(dev))
    _check(rc, "interpol_lcc_affine")
    return loss, gradient, hess


MI_MIN_BINS, MI_MAX_BINS = 8, 64                                      # csrc/mi_affine.hip


def mi_affine_covered(moving, fixed, mat, weight, order, bins):
    """Does interpol_mi_affine take these?  (csrc/mi_affine.hip: what interpol_ssd_affine takes, one channel, 8 <= bins <= 64)"""
    return (ssd_affine_covered(moving, fixed, mat, weight, order) and moving.shape[1] == 1 and fixed.shape[1] == 1
            and MI_MIN_BINS <= int(bins) <= MI_MAX_BINS)


def mi_affine(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian=True, bins=32, return_histogram=False):
    """interpol_mi_affine: moving (B|1,1,*inshape), fixed (B|1,1,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape), ranges (B,5)
    float64 on the device (m_lo, m_sc, f_lo, f_sc, wmax per item: `torch_kernels.mi_ranges`) -> (loss (B), gradient (B,D,D+1),
    hessian (B,P,P) | None, histogram (B,bins,bins) | None) of minus the mutual information with respect to the matrix of each
    item.  The operands are taken as by `ssd_affine`.  The workspace (two bins x bins tables and 73 x 1024 doubles per item in 3-D)
    comes from the workspace cache of this module; inside a hipGraph capture it is a fresh buffer of the graph's pool."""
    dev = _require_gpu(moving, fixed, mat, weight)
    if not mi_affine_covered(moving, fixed, mat, weight, order, bins):
        raise NotImplementedError("interpol_mi_affine: D <= 3, one order 1..3, one channel, 8 <= bins <= 64, float32 / float64 tensors "
                                  "of one dtype only")
    dim = mat.shape[-1] - 1
    P = dim * (dim + 1)
    bins = int(bins)

    def ranges_operand(B):
        ok = (torch.is_tensor(ranges) and ranges.dtype == torch.float64 and ranges.device == dev and list(ranges.shape) == [B, 5]
              and ranges.is_contiguous())
        return ok, ", ranges (B,5) float64", [list(ranges.shape) if torch.is_tensor(ranges) else ranges]

    fixed, mat, weight, B, shape, wstride, p = _data_term_operands("interpol_mi_affine", moving, fixed, mat, weight, bound, order,
                                                                    extrapolate, affine=True, C="1", extra=ranges_operand)
    loss = _empty([B], dtype=mat.dtype, device=dev)
    gradient = _empty([B, dim, dim + 1], dtype=mat.dtype, device=dev)
    hess = _empty([B, P, P], dtype=mat.dtype, device=dev) if hessian else None
    hist = _empty([B, bins, bins], dtype=mat.dtype, device=dev) if return_histogram else None
    if p is None:                                    # (no sample: W = 0)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if hessian else None), (hist.zero_() if return_histogram else None)
    ws, wbytes = _data_term_workspace("interpol_mi_affine", dev, p, bins)
    with torch.cuda.device(dev):
        rc = lib().interpol_mi_affine(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(mat), _ptr(weight), _ptr(ranges), _ptr(loss),
                                      _ptr(gradient), _ptr(hess), _ptr(hist), 1 if hessian else 0, bins, _bstride(mat, B), wstride,
                                      _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_mi_affine")
    return loss, gradient, hess, hist


def mi_covered(moving, fixed, disp, weight, order, bins):
    """Does interpol_mi take these?  (csrc/mi.hip: what interpol_ssd takes, one channel, 8 <= bins <= 64, at most
    MAX_ITEMS_ON_ROWS items)"""
    return (ssd_covered(moving, fixed, disp, weight, order) and moving.shape[1] == 1 and fixed.shape[1] == 1
            and MI_MIN_BINS <= int(bins) <= MI_MAX_BINS and _items(moving, fixed, disp, weight) <= MAX_ITEMS_ON_ROWS)


def mi(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian='full', bins=32, return_histogram=False):
    """interpol_mi: moving (B|1,1,*inshape), fixed (B|1,1,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape), ranges (B,5)
    float64 on the device (m_lo, m_sc, f_lo, f_sc, wmax per item: `torch_kernels.mi_ranges`) -> (loss (B), gradient (B,*shape,D),
    hessian (B,*shape,K) | None, histogram (B,bins,bins) | None) of minus the mutual information with respect to `disp`; hessian:
    None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2).  The operands are taken as by `ssd`.  The workspace (two bins x bins
    tables and one double per item) comes from the workspace cache of this module; inside a hipGraph capture it is a fresh buffer of
    the graph's pool."""
    dev = _require_gpu(moving, fixed, disp, weight)
    if not mi_covered(moving, fixed, disp, weight, order, bins):
        raise NotImplementedError("interpol_mi: D <= 3, one order 1..3, one channel, 8 <= bins <= 64, float32 / float64 tensors of one "
                                  "dtype only")
    if hessian not in SSD_HESSIAN_KINDS:
        raise ValueError("interpol_mi: hessian is None, 'diagonal' or 'full', got %r" % (hessian,))
    dim = disp.shape[-1]
    kind = SSD_HESSIAN_KINDS[hessian]
    K = (0, dim, dim * (dim + 1) // 2)[kind]
    bins = int(bins)

    def ranges_operand(B):
        ok = (torch.is_tensor(ranges) and ranges.dtype == torch.float64 and ranges.device == dev and list(ranges.shape) == [B, 5]
              and ranges.is_contiguous())
        return ok, ", ranges (B,5) float64", [list(ranges.shape) if torch.is_tensor(ranges) else ranges]

    fixed, disp, weight, B, shape, wstride, p = _data_term_operands("interpol_mi", moving, fixed, disp, weight, bound, order, extrapolate,
                                                                     affine=False, C="1", extra=ranges_operand)
    loss = _empty([B], dtype=disp.dtype, device=dev)
    gradient = _empty([B] + shape + [dim], dtype=disp.dtype, device=dev)
    hess = _empty([B] + shape + [K], dtype=disp.dtype, device=dev) if K else None
    hist = _empty([B, bins, bins], dtype=disp.dtype, device=dev) if return_histogram else None
    if p is None:                                    # (no sample: W = 0)
        return loss.zero_(), gradient.zero_(), (hess.zero_() if K else None), (hist.zero_() if return_histogram else None)
    ws, wbytes = _data_term_workspace("interpol_mi", dev, p, bins)
    with torch.cuda.device(dev):
        rc = lib().interpol_mi(ctypes.byref(p), _ptr(moving), _ptr(fixed), _ptr(disp), _ptr(weight), _ptr(ranges), _ptr(loss),
                               _ptr(gradient), _ptr(hess), _ptr(hist), kind, bins, wstride, gradient.stride(0),
                               hess.stride(0) if K else 0, _ptr(ws), wbytes, _stream(dev))
    _check(rc, "interpol_mi")
    return loss, gradient, hess, hist


def spline_filter_(data, bound, order, dim, src=None):
    """Prefilter of `data` (contiguous) along dimension `dim`: in place, or -- `src` given, same shape
    and dtype, contiguous, not overlapping -- reading `src` and writing `data`."""
    dev = _require_gpu(data) if src is None else _require_gpu(data, src)
    if data.dtype not in _DTYPE_CODE:
        raise TypeError("spline_coeff: unsupported dtype %s" % data.dtype)
    if not data.is_contiguous():
        raise ValueError("spline_filter_: `data` must be contiguous")
    if src is not None and (src.shape != data.shape or src.dtype != data.dtype or not src.is_contiguous()):
        raise ValueError("spline_filter_: `src` must match `data` (shape, dtype, contiguous)")
    dim = dim % data.dim()
    n = data.shape[dim]
    outer = 1
    for s in data.shape[:dim]:
        outer *= s
    inner = 1
    for s in data.shape[dim + 1:]:
        inner *= s
    with torch.cuda.device(dev):
        if src is None:
            rc = lib().interpol_spline_filter(_ptr(data), _DTYPE_CODE[data.dtype], outer, n, inner,
                                              int(bound), int(order), _stream(dev))
        else:
            rc = lib().interpol_spline_filter_to(_ptr(src), _ptr(data), _DTYPE_CODE[data.dtype], outer, n, inner,
                                                 int(bound), int(order), _stream(dev))
    _check(rc, "interpol_spline_filter")
    return data


def resample1d(src, lin, dim, order, bound, extrapolate, mode, adjoint=False, n_lattice=None):
    """One pass of a tensor-product resampling along `dim` (interpol_resample_1d).
    forward: src (..., n_lattice, ...), lin (n_samples,) -> (..., n_samples, ...)
    adjoint: src (..., n_samples, ...) -> (..., n_lattice, ...)   (f32 / f64)."""
    dev = _require_gpu(src, lin)
    if src.dtype not in _DTYPE_CODE:
        raise TypeError("resample1d: unsupported dtype %s" % src.dtype)
    src = src.contiguous()
    ldt = torch.float64 if src.dtype == torch.float64 else torch.float32
    lin = lin.detach().to(ldt).contiguous()
    dim = dim % src.dim()
    n = src.shape[dim]
    outer = 1
    for s_ in src.shape[:dim]:
        outer *= s_
    inner = 1
    for s_ in src.shape[dim + 1:]:
        inner *= s_
    if adjoint:
        if n != lin.numel():
            raise ValueError("resample1d: the resampled dimension must match the lattice vector")
        ns, nl = n, int(n_lattice)
        oshape = list(src.shape[:dim]) + [nl] + list(src.shape[dim + 1:])
    else:
        ns, nl = lin.numel(), n
        oshape = list(src.shape[:dim]) + [ns] + list(src.shape[dim + 1:])
    dst = _empty(oshape, dtype=src.dtype, device=dev)
    if dst.numel() == 0:
        return dst
    if src.numel() == 0:
        return dst.zero_()
    with torch.cuda.device(dev):
        rc = lib().interpol_resample_1d(_DTYPE_CODE[src.dtype], _DTYPE_CODE[ldt], int(order), int(bound), int(extrapolate),
                                        int(mode), int(bool(adjoint)), outer, ns, nl, inner,
                                        _ptr(src), _ptr(lin), _ptr(dst), _stream(dev))
    _check(rc, "interpol_resample_1d")
    return dst


def labels_covered(dim, order):
    """Does interpol_pull_labels take this stencil?  (all dims one order <= 3: up to the 64 taps of the 3-D cubic)"""
    order = list(order)[:dim]
    return len(set(order)) == 1 and order[0] <= 3


def pull_labels(vol, grid, bound, order, extrapolate, flags=0):
    """Label-map pull: vol (B,C,*in) integer labels, grid (B,*out,D) float32 -> (B,C,*out) int32.
    Arg-max over the labels of the interpolated indicator images (reference api.py:194-205)."""
    dev = _require_gpu(vol, grid)
    dim = grid.shape[-1]
    if vol.dtype.is_floating_point:
        raise TypeError("pull_labels: integer label map expected")
    if grid.dtype != torch.float32:
        raise TypeError("pull_labels: float32 coordinates expected")
    vol = vol.to(torch.int32)
    grid, gflag = _prep_grid(grid, torch.float32)
    flags |= gflag
    B = max(vol.shape[0], grid.shape[0])
    C = vol.shape[1]
    oshape = list(grid.shape[1:-1])
    val = _empty([B, C] + oshape, dtype=torch.int32, device=dev)
    if val.numel() == 0:
        return val
    vstr = [_bstride(vol, B), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    valstr = [val.stride(0), val.stride(1)] + _pad_to([val.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    p = make_problem(dim, torch.float32, torch.float32, bound, order, extrapolate, B, C, vol.shape[2:], oshape,
                     vstr, _grid_strides(grid, B, dim), valstr, flags)
    with torch.cuda.device(dev):
        rc = lib().interpol_pull_labels(ctypes.byref(p), _ptr(vol), _ptr(grid), _ptr(val), _stream(dev))
    _check(rc, "interpol_pull_labels")
    return val


def bricks_applicable(val, grid, with_count, order=None):
    """Can interpol_push_bricks take this problem? (3-D, fp32, one order <= 3 for all dims,
    <= 4 target channels, < 2^32 samples)"""
    dim = grid.shape[-1]
    from . import backend
    if backend.want_exact_scatter():                     # the brick kernels accumulate in fixed point too
        return False
    if order is not None:
        o = list(order)[:3]
        if len(set(o)) != 1 or o[0] > 3:
            return False
    return (dim == 3 and val is not None and val.dtype == torch.float32 and grid.dtype == torch.float32
            and val.shape[1] + (1 if with_count else 0) <= 4
            and max(val.shape[0], grid.shape[0]) * int(torch.Size(grid.shape[1:-1]).numel()) < 2 ** 32)


def push_bricks(val, grid, shape, bound, order, extrapolate, flags=0, out=None, shared=False, with_count=False):
    """interpol_push_bricks: push (and count) organised by target brick -- for expanding deformations.
    Same arguments and result as `scatter("push", ...)`."""
    dev = _require_gpu(val, grid)
    dim = grid.shape[-1]
    if not bricks_applicable(val, grid, with_count, order):
        raise ValueError("push_bricks: 3-D float32 problems, one order <= 3, at most 4 target channels only")
    grid, gflag = _prep_grid(grid, torch.float32)
    flags |= gflag | (FLAG_WITH_COUNT if with_count else 0)
    val = val.contiguous()
    gshape = list(grid.shape[1:-1])
    shape = [int(s) for s in (gshape if shape is None else shape)]
    B = max(val.shape[0], grid.shape[0])
    C = val.shape[1]
    Cv = C + (1 if with_count else 0)
    Bv = 1 if shared else B
    if out is None:
        vol = _empty([Bv, Cv] + shape, dtype=torch.float32, device=dev)
    else:
        vol = out
        assert vol.is_contiguous() and vol.dtype == torch.float32 and list(vol.shape) == [Bv, Cv] + shape
    if vol.numel() == 0:
        return vol
    if grid.numel() == 0:
        return vol.zero_() if out is None else vol
    valstr = [_bstride(val, B), val.stride(1)] + _pad_to([val.stride(2 + d) for d in range(dim)], 3) + [0, 0]
    vstr = [0 if shared else vol.stride(0), vol.stride(1)] + _pad_to([vol.stride(2 + d) for d in range(dim)], 3)
    p = make_problem(dim, torch.float32, torch.float32, bound, order, extrapolate, B, C, shape, gshape,
                     vstr, _grid_strides(grid, B, dim), valstr, flags)
    L = lib()
    nbytes = L.interpol_push_bricks_workspace(ctypes.byref(p))
    if nbytes < 0:
        _check(int(nbytes), "interpol_push_bricks_workspace")
    work = _scratch(_empty(int(nbytes), dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        rc = L.interpol_push_bricks(ctypes.byref(p), _ptr(val), _ptr(grid), _ptr(vol), _ptr(work), int(nbytes), _stream(dev))
    _check(rc, "interpol_push_bricks")
    return vol


HANDBACK_MODES = {"adaptive": 0, "always": 1, "never": 2}


def set_handback(mode):
    """Tile hand-back policy of the library (include/interpol_hip.h, interpol_set_handback): 'adaptive' (default: per
    stream, from the flags of its recent launches -- results may differ in the last bits with the stream's history),
    'always' or 'never' (every operator is then a deterministic function of its inputs).  Returns the previous mode."""
    code = HANDBACK_MODES[mode] if isinstance(mode, str) else int(mode)
    prev = int(lib().interpol_set_handback(code))
    return {v: k for k, v in HANDBACK_MODES.items()}.get(prev, prev)


def release_stream(stream=None):
    """Give the hand-back slot of `stream` (a torch.cuda.Stream; default: the current one) back to the library."""
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.device(st.device):
        return bool(lib().interpol_release_stream(ctypes.c_void_p(st.cuda_stream)))
