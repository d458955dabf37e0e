"""`regulariser_solve`: the per-point (Jacobi) preconditioner against the multigrid V-cycle, both fused, on one commit.

Three parts, float32:
  per-iteration : 1 x n^3 x 3 (n = 256) and 32 x m^2 x 2 (m = 1024), i.i.d. normal g, full Hessian 0.5 R R^T / D, dft; weights
                  bending and elastic (membrane 0.5, shears 1, div 2); `tolerance` = 0.  Each call is timed at max_iter = 2 and at
                  max_iter = 6; ms per iteration = (median(6) - median(2)) / 4, which leaves the set-up (the Hessian pyramid, the
                  first cycle) out.  The multigrid lines carry the byte model of one cycle (below) at the measured copy rate.
  to-tolerance  : g, H of `ssd_gauss_newton` (order 1, dct2; moving and fixed: smooth images a few voxels apart, see `images`) on
                  1 x n^3 x 3 displacement lattices; bending (bound dct2) and elastic weights (bound sliding); relative residual
                  1e-3 and 1e-6; both preconditioners.  `max_iter` is capped (--cap, 500): a run that does not reach the tolerance
                  is reported with "reached": false and its residual.  Iterations are read from `info` after the timed calls.
  one cycle     : `ops.regulariser_vcycle` alone on the two per-iteration shapes.

Method: one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read + write); per row `--warmup`
warm-up calls, then `--steps` calls, each timed with a pair of events; median and 10th / 90th percentiles of ms per call.  One JSON
line per row.

The byte model of one cycle, per level l with N_l points, D components and K Hessian entries (elements; a gathered field counts
once): first sweep r, H read and x written (2 D + K); every other sweep x, r, H read and x written (3 D + K), 2 nu - 1 of them
(7 on the last level); the residual the same; restriction reads D N_l and writes D N_{l+1}; prolong-and-add reads D N_{l+1} and
reads and writes D N_l.

`--only WHAT` (jacobi | multigrid | cycle) runs the first per-iteration row on that route alone, `--steps` times after the
warm-up, and prints nothing: the program to put behind a kernel tracer for the per-kernel split (never in the timed run).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))
sys.path.insert(0, PKG)
import interpol  # noqa: E402
from interpol import ops  # noqa: E402

WEIGHTS = dict(bending=dict(bending=1.0), elastic=dict(membrane=0.5, shears=1.0, div=2.0))


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stats(v):
    return dict(median=round(pct(v, 0.5), 4), p10=round(pct(v, 0.1), 4), p90=round(pct(v, 0.9), 4))


def timed(fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return stats(ms)


def copy_rate(dev):
    src = torch.randn(1 << 28, device=dev)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), 20, 5)
    return 2 * src.numel() * 4 / (t["median"] * 1e-3) / 1e12


def full_hessian(B, shape, gen, dev):
    dim = len(shape)
    out = torch.empty([B, *shape, dim * (dim + 1) // 2], device=dev)
    for b in range(B):
        R = torch.randn([*shape, dim, dim], generator=gen).to(dev)
        H = 0.5 * (R[..., :, None, :] * R[..., None, :, :]).sum(-1) / dim
        out[b] = torch.stack([H[..., d, d] for d in range(dim)] + [H[..., i, j] for i in range(dim) for j in range(i + 1, dim)], -1)
    return out


def cycle_bytes(shape, K, nu, es=4):
    """bytes of one V-cycle per batch item (the model of the header)"""
    D, shape, total = len(shape), list(shape), 0
    while True:
        N = 1
        for n in shape:
            N *= n
        halved = [n % 2 == 0 and n // 2 >= 4 for n in shape]
        last = not any(halved)
        total += N * ((2 * D + K) + ((7 if last else 2 * nu - 1) + (0 if last else 1)) * (3 * D + K))
        if last:
            return total * es
        shape = [n // 2 if y else n for n, y in zip(shape, halved)]
        Nc = 1
        for n in shape:
            Nc *= n
        total += D * (N + Nc) + D * (Nc + 2 * N)


def images(shape, gen, dev):
    """moving, fixed (1, 1, *shape): sums of a few low Fourier modes with random phases; fixed is moving shifted by a smooth
    field of a few voxels (sampled with order 1)"""
    dim = len(shape)
    grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=dev) / n for n in shape], indexing="ij")

    def modes(count, kmax):
        v = torch.zeros(shape, device=dev)
        for _ in range(count):
            k = torch.randint(1, kmax, [dim], generator=gen)
            ph = float(torch.rand([], generator=gen)) * 6.2831853
            v += torch.sin(6.2831853 * sum(float(k[d]) * grid[d] for d in range(dim)) + ph)
        return v

    moving = modes(12, 9)[None, None]
    disp = torch.stack([3.0 * modes(3, 3) / 3 for _ in range(dim)], -1)[None]
    fixed = interpol.grid_pull(moving, interpol.add_identity_grid(disp), interpolation=1, bound="dct2", extrapolate=True)
    return moving, fixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice, 1 x n^3 x 3 (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x m^2 x 2 (0: skip)")
    ap.add_argument("--cap", type=int, default=500, help="max_iter of the to-tolerance runs")
    ap.add_argument("--smoothing", type=int, default=2)
    ap.add_argument("--parts", default="iteration,tolerance,cycle")
    ap.add_argument("--only", default=None, choices=["jacobi", "multigrid", "cycle"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_multigrid: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    shapes = ([[1, a.n, a.n, a.n]] if a.n else []) + ([[32, a.m, a.m]] if a.m else [])
    parts = a.parts.split(",")
    rate = None
    if a.only is None:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    for bshape in shapes:
        B, shape = bshape[0], bshape[1:]
        dim = len(shape)
        torch.cuda.empty_cache()
        g = torch.randn([B, *shape, dim], generator=gen).to(dev)
        h = full_hessian(B, shape, gen, dev)
        for wname, w in WEIGHTS.items():
            kw = dict(bound="dft", tolerance=0., smoothing=a.smoothing, **w)
            if a.only is not None:
                for _ in range(a.warmup + a.steps):
                    if a.only == "cycle":
                        ops.regulariser_vcycle(g, h, tuple(w.get(k, 0.) for k in ("absolute", "membrane", "bending", "shears", "div")),
                                               [1.] * dim, [6] * dim, a.smoothing)
                    else:
                        interpol.regulariser_solve(g, h, max_iter=4, preconditioner=a.only, **kw)
                torch.cuda.synchronize()
                return
            if "iteration" in parts:
                for pre in ("jacobi", "multigrid"):
                    t2 = timed(lambda: interpol.regulariser_solve(g, h, max_iter=2, preconditioner=pre, **kw), a.steps, a.warmup)
                    t6 = timed(lambda: interpol.regulariser_solve(g, h, max_iter=6, preconditioner=pre, **kw), a.steps, a.warmup)
                    res = dict(part="iteration", preconditioner=pre, shape=list(g.shape), weights=wname, hessian="full", bound="dft",
                               call_ms_2=t2, call_ms_6=t6, ms_per_iteration=round((t6["median"] - t2["median"]) / 4, 4))
                    if pre == "multigrid":
                        nbytes = B * cycle_bytes(shape, h.shape[-1], a.smoothing)
                        model = nbytes / (rate * 1e12) * 1e3
                        res.update(smoothing=a.smoothing, cycle_model_bytes_per_point=round(nbytes / (g.numel() // dim), 1),
                                   cycle_model_ms=round(model, 4))
                    print(json.dumps(res), flush=True)
            if "cycle" in parts:
                w5 = tuple(w.get(k, 0.) for k in ("absolute", "membrane", "bending", "shears", "div"))
                t = timed(lambda: ops.regulariser_vcycle(g, h, w5, [1.] * dim, [6] * dim, a.smoothing), a.steps, a.warmup)
                nbytes = B * cycle_bytes(shape, h.shape[-1], a.smoothing)
                model = nbytes / (rate * 1e12) * 1e3
                print(json.dumps(dict(part="cycle", shape=list(g.shape), weights=wname, smoothing=a.smoothing, call_ms=t,
                                      cycle_model_ms=round(model, 4), fraction_of_model=round(model / t["median"], 3))), flush=True)
        del g, h
    if "tolerance" in parts and a.n and a.only is None:
        shape = [a.n] * 3
        torch.cuda.empty_cache()
        moving, fixed = images(shape, gen, dev)
        disp = torch.zeros([1, *shape, 3], device=dev)
        _, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, interpolation=1, bound="dct2", extrapolate=True, hessian="full")
        for wname, w, bound in (("bending", WEIGHTS["bending"], "dct2"), ("elastic", WEIGHTS["elastic"], "sliding")):
            for tol in (1e-3, 1e-6):
                for pre in ("jacobi", "multigrid"):
                    kw = dict(bound=bound, tolerance=tol, max_iter=a.cap, preconditioner=pre, smoothing=a.smoothing, return_info=True, **w)
                    t = timed(lambda: interpol.regulariser_solve(g, h, **kw), max(2, a.steps // 3), 1)
                    _, info = interpol.regulariser_solve(g, h, **kw)
                    res = float(info.residual[0])
                    print(json.dumps(dict(part="tolerance", preconditioner=pre, shape=list(g.shape), weights=wname, bound=bound, tolerance=tol,
                                          iterations=int(info.iterations[0]), residual=float("%.3g" % res), reached=res <= tol,
                                          call_ms=t)), flush=True)


if __name__ == "__main__":
    main()
