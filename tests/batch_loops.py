"""Inputs of the batch-loop tests (tests/test_batch_loops_cpu.py, tests/test_batch_loops_gpu.py): nothing device-specific.

A launch has at most 65 535 rows of workgroups; a kernel that puts the batch item on gridDim.y clamps it there and walks the rest of
the batch in a loop.  B_LOOP = 65 535 + 3 items make rows 0, 1, 2 take a second trip (items 65 535, 65 536, 65 537) while every other
row makes one; B_EDGE = 65 535 is the most a kernel without the loop takes.  The problems are built by the builders of the
per-operator test modules with their `B=` argument (`compose_fields` and `solve_system` restate theirs, whose shapes and batch are
fixed), so every item is drawn independently: an item computed from another item's operands shows.

The lattices are the smallest that still have an interior and a border in every dimension, so that the float64 truth of 65 538 items
stays a matter of seconds on the CPU.
"""
import sys


def main():
    """`python tests/batch_loops.py < log`: the `BATCH` lines that tests/test_batch_loops_gpu.py prints under -s, one per line, as
    profiles/batch_loops.txt keeps them"""
    for line in sys.stdin:
        at = line.find("BATCH ")                                        # (under -s the line follows pytest's progress marks)
        if at >= 0:
            print(line[at + 6:].rstrip())


if __name__ == "__main__":                                              # (before the imports below, which need the package on the path)
    main()
    sys.exit(0)

import torch

import test_lcc_cpu as lcc_cpu
import test_regulariser_cpu as reg_cpu
import test_regulariser_solve_cpu as st
import test_ssd_cpu as ssd_cpu

ROWS = 65535                                                         # the most rows of workgroups a launch has
B_LOOP = ROWS + 3
B_EDGE = ROWS
SECOND_TRIP = (ROWS, ROWS + 1, ROWS + 2)
PINNED = (0, 1, 2) + SECOND_TRIP                                     # rows 0 .. 2, first and second trip
SEED = 7
# dim -> (moving lattice, fixed lattice)
SSD_LATTICES = {1: ((5,), (4,)), 2: ((3, 4), (2, 3)), 3: ((3, 2, 4), (2, 3, 2))}
LCC_LATTICES = {1: ((6,), (5,)), 2: ((4, 5), (3, 4)), 3: ((3, 2, 4), (2, 3, 2))}
THIN = ((1, 2, 3), (2, 1, 3))                                        # extents of 1: compose and jacobian only
DT = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
_CACHE = {}

# The cases of tests/test_batch_loops_gpu.py.  They stand here so that tests/test_batch_loops_cpu.py can hold the truth of every one of
# them to its conditions without a device.  `seed` is SEED unless two of the six pinned items then have a loss or an energy (one number
# per item) within 100 bars of each other: the next seed that separates them is taken, and the CPU test asserts that it does.
# (name, dim, dtype, order, bound, extrapolate, sigma, hessian, fixed has its own batch, seed)
SSD_CASES = [
    ("1d-f32-o1-dct2-ex1-full-shared", 1, "f32", 1, "dct2", True, 2.0, "full", False, 7),
    ("1d-f32-o3-zero-ex0-none-own", 1, "f32", 3, "zero", False, 0.4, None, True, 7),
    ("2d-f32-o3-dft-ex1-full-own", 2, "f32", 3, "dft", True, 2.0, "full", True, 7),
    ("2d-f64-o1-dct2-ex0-full-shared", 2, "f64", 1, "dct2", False, 0.4, "full", False, 7),
    ("2d-f64-o3-dct2-ex1-none-own", 2, "f64", 3, "dct2", True, 2.0, None, True, 7),
    ("3d-f32-o1-dct2-ex0-full-shared", 3, "f32", 1, "dct2", False, 0.4, "full", False, 7),
    ("3d-f32-o3-dct2-ex1-none-own", 3, "f32", 3, "dct2", True, 2.0, None, True, 7),
    ("3d-f32-o3-replicate-ex0-full-shared", 3, "f32", 3, "replicate", False, 0.4, "full", False, 7),
]
# (name, dim, dtype, order, bound, extrapolate, sigma, window, hessian, seed, eps).  eps: csrc/lcc.hip stores I = pull(moving) in the
# field's dtype, rounded once, before the window sums (its precision contract); where a window of two or three points has next to no
# contrast, den falls to eps and that one rounding moves the float64 truth by more than the float32 bar -- 40 bars at eps = 1e-5 among
# the 65 538 x 5 windows of the 1-D lattice (tests/test_batch_loops_cpu.py measures it on the CPU, no kernel involved; tests/test_lcc_gpu.py
# leaves its group (offset 10, eps 1e-5) out for the same reason).  The float32 cases take eps = 1, the second group that file compares;
# float64 its first, 1e-5.
LCC_CASES = [
    ("1d-f32-o2-dft-ex1-w3-full", 1, "f32", 2, "dft", True, 2.0, 3, "full", 7, 1.0),
    ("1d-f64-o3-dct2-ex0-w5-full", 1, "f64", 3, "dct2", False, 0.4, 5, "full", 8, 1e-5),
    ("1d-f64-o2-dft-ex1-w3-none", 1, "f64", 2, "dft", True, 2.0, 3, None, 7, 1e-5),
    ("2d-f32-o3-dct2-ex0-w3-full", 2, "f32", 3, "dct2", False, 0.4, 3, "full", 7, 1.0),
    ("2d-f32-o2-dft-ex1-w5-none", 2, "f32", 2, "dft", True, 2.0, 5, None, 7, 1.0),
    ("3d-f32-o2-dft-ex1-w3-full", 3, "f32", 2, "dft", True, 2.0, 3, "full", 7, 1.0),
    ("3d-f32-o3-dct2-ex0-w5-diagonal", 3, "f32", 3, "dct2", False, 0.4, 5, "diagonal", 7, 1.0),
]
# (name, lattice, dtype, order, bound)
JACOBIAN_CASES = [
    ("1d-f32-o1-dct2", (4,), "f32", 1, "dct2"), ("1d-f32-o3-dft", (4,), "f32", 3, "dft"),
    ("2d-f32-o3-dct2", (2, 3), "f32", 3, "dct2"), ("2d-f64-o1-dft", (2, 3), "f64", 1, "dft"), ("2d-f64-o3-zero", (2, 3), "f64", 3, "zero"),
    ("3d-f32-o1-dft", (2, 3, 2), "f32", 1, "dft"), ("3d-f32-o3-dct2", (2, 3, 2), "f32", 3, "dct2"),
    ("thin-f32-o1-dct2", THIN[1], "f32", 1, "dct2"), ("thin-f32-o3-dft", THIN[1], "f32", 3, "dft"),
]
# (name, (lattice of left, lattice of right), dtype, order, bound, extrapolate, batch of left: None = B)
COMPOSE_CASES = [
    ("1d-f32-o1-dct2-ex1", SSD_LATTICES[1], "f32", 1, "dct2", 1, None), ("1d-f32-o3-dft-ex0", SSD_LATTICES[1], "f32", 3, "dft", 0, None),
    ("2d-f32-o3-dct2-ex1-left1", SSD_LATTICES[2], "f32", 3, "dct2", 1, 1), ("2d-f64-o1-dft-ex0", SSD_LATTICES[2], "f64", 1, "dft", 0, None),
    ("3d-f32-o1-dft-ex1-left1", SSD_LATTICES[3], "f32", 1, "dft", 1, 1), ("3d-f32-o3-dct2-ex0", SSD_LATTICES[3], "f32", 3, "dct2", 0, None),
    ("thin-f32-o3-dct2-ex1", THIN, "f32", 3, "dct2", 1, None), ("thin-f32-o1-dft-ex2", THIN, "f32", 1, "dft", 2, None),
]
REG_WEIGHTS = dict(membrane=0.7, bending=1.3)
REG_ABSOLUTE = 2.0                                                   # tests/test_regulariser_gpu.py: "Energy: rtol = tol, with absolute > 0"
# (name, lattice, dtype, bound, seed)
REG_CASES = [
    ("1d-f32-dct2", (4,), "f32", "dct2", 7), ("1d-f64-dct2", (4,), "f64", "dct2", 7), ("1d-f64-replicate", (4,), "f64", "replicate", 7),
    ("2d-f32-dct2", (2, 3), "f32", "dct2", 7), ("2d-f32-replicate", (2, 3), "f32", "replicate", 7),
    ("3d-f32-dct2", (2, 3, 2), "f32", "dct2", 7), ("3d-f32-replicate", (2, 3, 2), "f32", "replicate", 7),
]
# (name, lattice, dtype, weights, bound, Hessian kind): all three weights; with no Hessian `absolute` keeps the system definite
SOLVE_WEIGHTS = dict(absolute=0.3, membrane=0.7, bending=1.3)
EARLY_MAX_ITER, EARLY_TOLERANCE = 3, 0.65                            # between 10 % and 90 % of the items of every case stop before the cap
SOLVE_CASES = [
    ("1d-f32-full", (4,), "f32", "dct2", "full"), ("1d-f64-none", (4,), "f64", "dft", "none"),
    ("2d-f32-diag", (2, 3), "f32", "dct2", "diag"), ("2d-f32-none", (2, 3), "f32", "dct2", "none"),
    ("3d-f32-full", (2, 3, 2), "f32", "dct2", "full"), ("3d-f32-diag", (2, 3, 2), "f32", "dft", "diag"),
]


def chunks(fn, args, size=32768):
    """`fn(*args)` made on slices of the batch of at most `size` items, concatenated: every chunk is a call whose batch loops make one
    trip.  The batch is the largest leading extent among the tensors of `args`; a tensor with that leading extent is sliced, every
    other argument (no batch, a batch of 1, None, a number) goes to every chunk as it is.  `fn` returns a tensor or a tuple of
    tensors and None."""
    B = max(a.shape[0] for a in args if torch.is_tensor(a) and a.dim())
    outs = []
    for lo in range(0, B, size):
        part = [a[lo:lo + size] if torch.is_tensor(a) and a.dim() and a.shape[0] == B else a for a in args]
        outs.append(fn(*part))
    if torch.is_tensor(outs[0]):
        return torch.cat(outs)
    return tuple(None if o[0] is None else torch.cat(o) for o in zip(*outs))


def cached(key, make):
    """computed once, shared by the tests that need it, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ssd_problem(dim, dtype, order, sigma, B=B_LOOP, own_fixed=False, seed=SEED, lattices=SSD_LATTICES, builder=ssd_cpu):
    """(moving (B, 2, *inshape), fixed (2, *shape) or, `own_fixed`, (B, 2, *shape), disp nudged off the knots, weight (B, *shape))"""
    inshape, shape = lattices[dim]
    moving, fixed, disp, weight = builder.problem(inshape, shape, seed, dtype, C=2, B=B, sigma=sigma)
    if own_fixed:
        gen = torch.Generator().manual_seed(seed + 1)
        fixed = (fixed.double()[None] + 0.5 * torch.randn([B, *fixed.shape], generator=gen, dtype=torch.float64)).to(dtype)
    disp, _ = ssd_cpu.nudged(disp, order)
    return moving, fixed, disp, weight


def lcc_problem(dim, dtype, order, sigma, B=B_LOOP, seed=SEED):
    return ssd_problem(dim, dtype, order, sigma, B, False, seed, LCC_LATTICES, lcc_cpu)


def ssd_case(case, B=B_LOOP):
    """-> (args, kw) of one of SSD_CASES"""
    name, dim, dt, order, bound, ex, sigma, hessian, own, seed = case
    return ssd_problem(dim, DT[dt], order, sigma, B, own, seed), dict(interpolation=order, bound=bound, extrapolate=ex, hessian=hessian)


def lcc_case(case, B=B_LOOP):
    name, dim, dt, order, bound, ex, sigma, window, hessian, seed, eps = case
    return lcc_problem(dim, DT[dt], order, sigma, B, seed), dict(interpolation=order, bound=bound, extrapolate=ex, hessian=hessian,
                                                                  window=window, eps=eps)


def field(shape, dtype, B=B_LOOP, seed=SEED, builder=reg_cpu):
    """(B, *shape, D) randn, as tests/test_regulariser_cpu.py draws it (`builder`: tests/test_jacobian_cpu.py has the same recipe
    under the same name)"""
    return builder.field(shape, seed, dtype, B=B)


def compose_fields(lshape, oshape, dtype, B=B_LOOP, lB=None, seed=SEED):
    """left (lB or B, *lshape, D) randn, right (B, *oshape, D) dyadic: the recipe of tests/test_compose_cpu.py (`fields`, whose shapes
    are fixed per dim) on the lattices of this module: multiples of 1 / 64 as its `dyadic` draws them, of at most 3 / 4 of a voxel, so that
    a fifth of the samples and more stay in view of a lattice of two to four points"""
    gen = torch.Generator().manual_seed(seed)
    dim = len(oshape)
    left = torch.randn([B if lB is None else lB, *lshape, dim], generator=gen, dtype=torch.float64).to(dtype)
    right = (torch.randint(-48, 49, [B, *oshape, dim], generator=gen).double() / 64).to(dtype)   # (`dyadic` with an amplitude of 3 / 4)
    return left, right


def solve_system(shape, bound, w, vx, kind, dtype, B=B_LOOP, seed=SEED):
    """tests/test_regulariser_solve_cpu.py: `system` for B items.  g = field; the Hessians follow `fixed_hessians`: even items the
    full 0.5 R R^T / D, odd items the diagonal 0.2 rand, handed over in the one layout `kind` ('full', 'diag', 'none') of the call."""
    dim = len(shape)
    gen = torch.Generator().manual_seed(seed + 1000)
    R = torch.randn([B, *shape, dim, dim], generator=gen, dtype=torch.float64)
    d1 = 0.2 * torch.rand([B, *shape, dim], generator=gen, dtype=torch.float64)
    dense = 0.5 * (R @ R.transpose(-1, -2)) / dim
    dense[1::2] = torch.diag_embed(d1[1::2])
    if kind == "none":
        h, Hd = None, torch.zeros_like(dense)
    else:
        h = (st.pack(dense) if kind == "full" else torch.diagonal(dense, dim1=-2, dim2=-1).contiguous()).to(dtype)
        Hd = st.unpack(h.double(), dim)
    return dict(g=reg_cpu.field(shape, seed, dtype, B=B), h=h, S=reg_cpu.spatial_matrix(shape, bound, voxel_size=vx, **w),
                hh=reg_cpu.h2(dim, vx), Hd=Hd.reshape(B, -1, dim, dim), c=st.centre(st.voxels(dim, vx), **w),
                kw=dict(voxel_size=vx, bound=bound, **w))


def restated_batch(sy, max_iter, history=False):
    """`restated` of tests/test_regulariser_solve_cpu.py at tolerance 0 in float64, every item of the batch at once: the same
    statements with a leading batch dimension; an item leaves the iteration where `restated` breaks (pi <= 0 or rho <= 0, or a
    residual of exactly zero).  -> x (B, N, D), and with `history` the relative residuals sqrt(sigma / gamma) after every
    iteration, (max_iter, B): what a tolerance is compared with.  tests/test_batch_loops_cpu.py holds it to `restated` item by item."""
    S, hh, Hd, c = sy["S"], sy["hh"], sy["Hd"], sy["c"]
    g = sy["g"].double().reshape(Hd.shape[0], -1, Hd.shape[-1])
    A = lambda v: torch.einsum("on,bnd->bod", S, v) * hh + torch.einsum("bnde,bne->bnd", Hd, v)
    M = Hd + torch.diag(c)
    Mi = lambda v: torch.linalg.solve(M, v[..., None])[..., 0]
    dot = lambda a, b: (a * b).flatten(1).sum(1)
    x, r = torch.zeros_like(g), g.clone()
    z = Mi(r)
    p = z.clone()
    rho, gamma = dot(r, z), dot(g, g)
    live = gamma != 0
    res = []
    for _ in range(max_iter):
        q = A(p)
        pi = dot(p, q)
        live = live & (pi > 0) & (rho > 0)
        alpha = torch.where(live, rho / pi.where(live, torch.ones_like(pi)), torch.zeros_like(pi))[:, None, None]
        x, r = x + alpha * p, r - alpha * q
        z = Mi(r)
        rho1, sigma = dot(r, z), dot(r, r)
        res.append((sigma / gamma).sqrt())
        beta = torch.where(live, rho1 / rho.where(live, torch.ones_like(rho)), torch.zeros_like(rho))[:, None, None]
        live = live & (sigma > 0)
        p, rho = torch.where(live[:, None, None], z + beta * p, p), torch.where(live, rho1, rho)
    return (x, torch.stack(res)) if history else x


# (name, dim, dtype, order, bound, extrapolate): the generic kernels (csrc/ops_generic.hpp); the lattices are far below the 4 096
# samples every other organisation needs
GENERIC_CASES = [
    ("3d-f32-o1-dct2-ex1", 3, "f32", 1, "dct2", 1), ("2d-f32-o3-dft-ex1", 2, "f32", 3, "dft", 1),
    ("1d-f32-o2-zero-ex0", 1, "f32", 2, "zero", 0), ("3d-f64-o3-dct2-ex1", 3, "f64", 3, "dct2", 1),
]


def generic_problem(dim, B=B_LOOP, seed=SEED):
    """inp (B, 2, *lattice), val (B, 2, *samples), gout (B, 2, *lattice), grad (B, 2, *samples, D), grid (B, *samples, D): float64
    tensors of float32-representable values, so that one float64 truth serves both precisions.  The coordinates are multiples of
    1 / 64 (tests/test_second_order_cpu.py: `problem`): a line from -1/2 to n - 1/2 plus up to 3/4 of a voxel either way, exact in
    float32, and none lies on a mask threshold."""
    lattice, samples = SSD_LATTICES[dim]
    gen = torch.Generator().manual_seed(seed + 10 * dim)
    lins = [torch.round(torch.linspace(-0.5, n - 0.5, m, dtype=torch.float64) * 64) / 64 for n, m in zip(lattice, samples)]
    grid = torch.stack(torch.meshgrid(*lins, indexing="ij"), -1)[None] + torch.randint(-48, 49, [B, *samples, dim], generator=gen).double() / 64
    r = lambda *s: torch.randn(*s, generator=gen).double()
    return dict(inp=r(B, 2, *lattice), val=r(B, 2, *samples), gout=r(B, 2, *lattice), grad=r(B, 2, *samples, dim), grid=grid.contiguous(),
                lattice=list(lattice), samples=list(samples))


# (name, dim, order, lattice of the map, lattice of the samples, dtype of the grid, labels): csrc/labels.hip -- the plain kernel, the
# hash kernel (3-D cubic, float32 coordinates) and the wide kernel (3-D cubic; drawn in float64, see the device test)
LABEL_CASES = [
    ("plain-2d-o1", 2, 1, (3, 4), (2, 3), "f32", 6), ("hash-3d-o3-f32", 3, 3, (3, 4, 4), (2, 3, 2), "f32", 6),
    ("wide-3d-o3-f64", 3, 3, (3, 4, 4), (2, 3, 2), "f64", 6),
]


def label_problem(case, B=B_LOOP, seed=SEED):
    """lab (B, 2, *map) int64 in [0, labels), grid (B, *samples, D): the lattice of the samples stretched over the map plus N(0, 1)"""
    name, dim, order, ishape, oshape, gdt, labels = case
    gen = torch.Generator().manual_seed(seed + dim)
    lab = torch.randint(0, labels, [B, 2, *ishape], generator=gen)
    lins = [torch.linspace(-1.0, n, m, dtype=torch.float64) for n, m in zip(ishape, oshape)]
    grid = torch.stack(torch.meshgrid(*lins, indexing="ij"), -1)[None] + torch.randn([B, *oshape, dim], generator=gen, dtype=torch.float64)
    return lab, grid.to(DT[gdt])


MI_LATTICE = ((3, 2, 2), (2, 1, 1))
MI_BINS = 8


def mi_problem(order, dtype, B=B_EDGE, seed=SEED):
    """tests/test_mi_affine_cpu.py: `problem` and tests/test_mi_cpu.py: `dyadic_noise` with B items"""
    import test_mi_affine_cpu as aff
    import test_mi_cpu as mi_cpu
    inshape, shape = MI_LATTICE
    moving, fixed, weight = aff.problem(inshape, shape, seed + order, dtype, bins=MI_BINS, B=B)
    disp = mi_cpu.dyadic_noise(shape, len(shape), torch.Generator().manual_seed(seed + order + 100), 2.0, (B,)).to(dtype)
    return moving, fixed, disp, weight

