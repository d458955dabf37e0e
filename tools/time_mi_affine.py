"""The mutual-information data term on the matrix of an affine lattice (loss, gradient, P x P majoriser), composed route against fused.

Workloads, float32, bound dct2, extrapolate = True, ranges None (aminmax on the device), one dyadic rotation-shear-translation
matrix (multiples of 1/32) for every item; the moving image is i.i.d. normal, the fixed image a non-monotone function of it plus
noise (so that the joint histogram is neither flat nor a line):
  1 x 1 x n^3 (n = 256): orders 1, 2, 3, B = 32 and 64 bins, with and without the Hessian;
  4 x 1 x n^3          : cubic, 32 bins, with the Hessian;
  32 x 1 x m^2 (m = 1024): orders 1, 2, 3, 32 bins, with the Hessian.

  composed : interpol.mi_gauss_newton_affine with `interpol.backend.fused_mi_affine_orders = ()` -- a dense lattice per item,
             grid_pull, grid_grad, `index_add_` into a float64 histogram and the float64 contractions with the index moments
             (interpol/torch_kernels.py: mi_gauss_newton_affine_composed);
  fused    : the same call with every order routed to csrc/mi_affine.hip.

Method: one process; per row the two routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after
`--warmup` warm-up calls each, every call timed with a pair of events (the ranges -- two aminmax -- are part of the call on both
routes); the median and the 10th / 90th percentiles of ms per call over all blocks are printed.  One JSON line per (route, row).
After each row the largest difference between the routes' outputs is printed, relative to the largest entry of each output.

`--kernel-split` then runs every fused row `--steps` times under torch.profiler and prints the mean device time per call of each
kernel (the per-kernel split; profiling slows the host: never in the timed run).  `--only-fused-case I` (`--only-composed-case I`)
runs row I on that route alone and prints nothing else: the program to put behind a kernel tracer.
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

ALL_ORDERS = (1, 2, 3)
MATS = {
    3: [[0.96875, 0.125, -0.0625, 2.53125], [-0.125, 1.0, 0.09375, 1.71875], [0.0625, -0.09375, 0.96875, 3.09375]],
    2: [[0.96875, 0.125, 2.53125], [-0.125, 1.03125, 1.71875]],
}


def route(orders):
    interpol.backend.fused_mi_affine_orders = orders


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stats(v):
    return dict(median=round(pct(v, 0.5), 4), p10=round(pct(v, 0.1), 4), p90=round(pct(v, 0.9), 4))


def times(fn, steps, warmup):
    ms = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def rows(n, m):
    work = []
    if n:
        work += [([1, 1, n, n, n], order, bins, hess) for order in ALL_ORDERS for bins in (32, 64) for hess in (True, False)]
        work += [([4, 1, n, n, n], 3, 32, True)]
    if m:
        work += [([32, 1, m, m], order, 32, True) for order in ALL_ORDERS]
    return work


def kernel_split(call, steps):
    """mean device microseconds per call of every kernel, by name (torch.profiler)"""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0)
        if t:
            out[ev.key.split("(")[0][-60:]] = round(t / steps, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x 1 x m^2 (0: skip)")
    ap.add_argument("--kernel-split", action="store_true")
    ap.add_argument("--cases", type=str, default=None, help="comma-separated row numbers (default: every row)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    ap.add_argument("--only-composed-case", type=int, default=None)
    a = ap.parse_args()
    only = a.only_fused_case if a.only_fused_case is not None else a.only_composed_case
    if not torch.cuda.is_available():
        sys.exit("time_mi_affine: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m)
    if only is not None:
        work = [work[only]]
    elif a.cases:
        work = [work[int(i)] for i in a.cases.split(",")]
    cache = {}
    for bshape, order, bins, hess in work:
        B, shape = bshape[0], bshape[2:]
        dim = len(shape)
        key = tuple(bshape)
        if key not in cache:
            cache.clear()
            interpol.backend.release_workspaces()
            torch.cuda.empty_cache()
            moving = torch.randn([B, 1, *shape], generator=gen).to(dev)
            fixed = torch.cos(2.0 * moving) + 0.25 * torch.randn([B, 1, *shape], generator=gen).to(dev)
            cache[key] = (moving, fixed)
        moving, fixed = cache[key]
        mat = torch.tensor(MATS[dim], device=dev)
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian=hess, bins=bins)
        call = lambda: interpol.mi_gauss_newton_affine(moving, fixed, mat, **kw)
        if only is not None:
            route(ALL_ORDERS if a.only_fused_case is not None else ())
            for _ in range(a.warmup + a.steps):
                call()
            torch.cuda.synchronize()
            return
        ms, out = dict(composed=[], fused=[]), {}
        for rnd in range(a.rounds):                                       # the routes alternate: other work shares the machine
            for name in ("composed", "fused"):
                route(ALL_ORDERS if name == "fused" else ())
                ms[name] += times(call, a.steps if name == "fused" else a.composed_steps, a.warmup if rnd == 0 else 1)
                if rnd == 0:
                    out[name] = call()
        for name in ("composed", "fused"):
            res = dict(route=name, shape=bshape, order=order, bins=bins, hessian=hess, calls=len(ms[name]), call_ms=stats(ms[name]))
            if name == "fused":
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
        diff = {k: float("%.3g" % float((f.double() - c.double()).abs().max() / c.double().abs().max()))
                for k, f, c in zip(("loss", "gradient", "hessian"), out["fused"], out["composed"]) if f is not None}
        print(json.dumps(dict(shape=bshape, order=order, bins=bins, hessian=hess, max_difference_fused_composed_over_largest_entry=diff)),
              flush=True)
        out.clear()
        if a.kernel_split:
            route(ALL_ORDERS)
            try:
                split = kernel_split(call, a.steps)
            except Exception as e:                                        # (no tracer in this session: the timed lines stand alone)
                split = dict(error=repr(e))
            print(json.dumps(dict(shape=bshape, order=order, bins=bins, hessian=hess, kernel_us_per_call=split)), flush=True)


if __name__ == "__main__":
    main()
