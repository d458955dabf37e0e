"""The local cross-correlation data term of a Gauss-Newton step (loss, gradient, Hessian), composed route against fused route.

Workloads, float32, bound dct2, extrapolate = True, hessian 'full', fields smooth (a few low Fourier modes, amplitude 2 voxels) or
rough (i.i.d. normal, sigma = 2 voxels), moving i.i.d. normal + 10, fixed = 0.8 moving + 0.3 noise + 10 on one lattice:
  1 x 1 x n^3 (n = 256), windows 5 and 9;  1 x 3 x n^3, window 9;  32 x 1 x m^2 (m = 1024), window 9;  every order of `--orders`.

  composed : interpol.lcc_gauss_newton with `interpol.backend.fused_lcc_orders = ()` -- grid_pull, grid_grad at a displacement, the
             eight separable window sums in float64 and the element-wise passes (interpol/torch_kernels.py:
             lcc_gauss_newton_composed): what a user writes today;
  fused    : the same call with every order routed to csrc/lcc.hip.

Method (that of tools/time_ssd.py): one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read +
write); per row the two routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after `--warmup`
warm-up calls each, every call timed with a pair of events; the median and the 10th / 90th percentiles of ms per call over all
blocks are printed.  One JSON line per (route, row).  The fused lines also carry the time of the byte model (per
sample and channel: stage 1 reads the moving image and writes I, 8 B + the field; stage 2 reads I and fixed and writes a, c, f as
doubles; stage 3 reads a, c, f, I, fixed, the moving image and the field and writes gradient and Hessian) at the measured copy
rate and at 6.29 TB/s, and the fractions of both that were reached.  After each row the largest difference between the routes'
outputs is printed against the largest entry of each output.

`--only-fused-case I` (`--only-composed-case I`) runs row I on that route alone, `--steps` times after the warm-up and prints
nothing else: the program to put behind a kernel tracer for the per-kernel split (tracing slows the host: never in the timed run).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_ssd import ALL_ORDERS, PEAK_COPY_TBPS, copy_rate, smooth_field, stats, times  # noqa: E402  (it puts the package on the path)
import interpol  # noqa: E402


def route(orders):
    interpol.backend.fused_lcc_orders = orders


def model_bytes(C, dim, K, es=4):
    """bytes per sample of the three stages (the moving image counted as read once per stage that gathers it)"""
    one = C * 2 * es + dim * es                                          # moving read, I written; the field read
    two = C * (2 * es + 3 * 8)                                           # I and fixed read; a, c, f written as doubles
    three = C * (3 * 8 + 3 * es) + dim * es + (dim + K) * es             # a, c, f, I, fixed, moving read; field read; outputs written
    return one, two, three


def rows(n, m, orders):
    groups = []
    if n:
        groups += [([1, 1, n, n, n], 5), ([1, 1, n, n, n], 9), ([1, 3, n, n, n], 9)]
    if m:
        groups += [([32, 1, m, m], 9)]
    return [(bshape, window, order, field) for bshape, window in groups for field in ("smooth", "rough") for order in orders]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--orders", default="1,2,3")
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x 1 x m^2 (0: skip)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    ap.add_argument("--only-composed-case", type=int, default=None)
    a = ap.parse_args()
    only = a.only_fused_case if a.only_fused_case is not None else a.only_composed_case
    if not torch.cuda.is_available():
        sys.exit("time_lcc: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m, [int(o) for o in a.orders.split(",")])
    if only is not None:
        work = [work[only]]
    else:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    cache = {}
    for bshape, window, order, fname in work:
        B, C, shape = bshape[0], bshape[1], bshape[2:]
        dim = len(shape)
        key = (tuple(bshape), fname)
        if key not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            noise = torch.randn([B, C, *shape], generator=gen).to(dev)
            moving = noise + 10
            fixed = 0.8 * noise + 0.3 * torch.randn([B, C, *shape], generator=gen).to(dev) + 10
            if fname == "smooth":
                disp = torch.stack([smooth_field(shape, 2.0, gen, dev) for _ in range(B)])
            else:
                disp = (2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev)
            cache[key] = (moving, fixed, disp)
        moving, fixed, disp = cache[key]
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian="full", window=window, eps=1.0)
        call = lambda: interpol.lcc_gauss_newton(moving, fixed, disp, **kw)
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
        K = dim * (dim + 1) // 2
        for name in ("composed", "fused"):
            res = dict(route=name, shape=bshape, window=window, order=order, field=fname, calls=len(ms[name]), call_ms=stats(ms[name]))
            if name == "fused":
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
                per = model_bytes(C, dim, K)
                nbytes = sum(per) * disp.numel() // dim
                res.update(model_bytes_per_sample=list(per), model_ms_at_measured_copy_rate=round(nbytes / (rate * 1e12) * 1e3, 4),
                           model_ms_at_6_29_TBps=round(nbytes / (PEAK_COPY_TBPS * 1e12) * 1e3, 4))
                res.update(fraction_of_measured_copy_rate=round(res["model_ms_at_measured_copy_rate"] / res["call_ms"]["median"], 3),
                           fraction_of_6_29_TBps=round(res["model_ms_at_6_29_TBps"] / res["call_ms"]["median"], 3))
            print(json.dumps(res), flush=True)
        diff = {k: float(((f - c).abs().max() / c.abs().max())) for k, f, c in zip(("loss", "gradient", "hessian"), out["fused"], out["composed"])}
        print(json.dumps(dict(shape=bshape, window=window, order=order, field=fname,
                              max_difference_fused_composed_over_largest_entry={k: float("%.3g" % v) for k, v in diff.items()})), flush=True)
        out.clear()


if __name__ == "__main__":
    main()
