"""The local cross-correlation data term on the matrix of an affine lattice (loss, gradient, P x P Hessian), composed route against fused.

Workloads, float32, bound dct2, extrapolate = True, moving i.i.d. normal and fixed = 0.8 moving + 0.3 noise on one lattice, one dyadic
rotation-shear-translation matrix (multiples of 1/32) for every item:
  1 x 1 x n^3 (n = 256): windows 5 and 9, orders 1, 2, 3, with and without the Hessian;
  4 x 1 x n^3          : cubic, window 9, with the Hessian;
  32 x 1 x m^2 (m = 1024): window 9, orders 1, 2, 3, with the Hessian.

  composed : interpol.lcc_gauss_newton_affine with `interpol.backend.fused_lcc_affine_orders = ()` -- a dense lattice per item,
             `lcc_gauss_newton` at lattice - identity (itself routed as `backend.fused_lcc_orders` says: the fused dense term) and the
             float64 contraction of its per-sample gradient and Hessian with the index moments (interpol/torch_kernels.py:
             lcc_gauss_newton_affine_composed);
  fused    : the same call with every order routed to csrc/lcc_affine.hip.

Method: that of tools/time_ssd_affine.py -- one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read
+ write); per row the two routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after `--warmup`
warm-up calls each, every call timed with a pair of events; the median and the 10th / 90th percentiles of ms per call over all blocks
are printed.  One JSON line per (route, row).  The fused lines also carry the time of the byte model per stage and channel, es = 4:
  pull  : moving read, I written                              2 es
  stats : I and fixed read; a, c, f written as doubles        2 es + 24
  march : a, c, f, I, fixed read; dI, C written               24 + 2 es + 2 es
  sums  : moving, dI, C read                                  es + 2 es
at the measured copy rate and at 6.29 TB/s, and the fractions of both that were reached.  After each row the largest difference
between the routes' outputs is printed, relative to the largest entry of each output.

`--only-fused-case I` (`--only-composed-case I`) runs row I on that route alone, `--steps` times after the warm-up and prints
nothing else: the program to put behind a kernel tracer for the per-kernel split (tracing slows the host: never in the timed run).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interpol  # noqa: E402
from time_ssd_affine import MATS, PEAK_COPY_TBPS, copy_rate, stats, times  # noqa: E402

ALL_ORDERS = (1, 2, 3)


def route(orders):
    interpol.backend.fused_lcc_affine_orders = orders


def model_bytes(C, es=4):
    """bytes per sample of the four stages"""
    return C * 2 * es, C * (2 * es + 24), C * (24 + 4 * es), C * 3 * es


def rows(n, m):
    work = []
    if n:
        work += [([1, 1, n, n, n], window, order, hess) for window in (5, 9) for order in ALL_ORDERS for hess in (True, False)]
        work += [([4, 1, n, n, n], 9, 3, True)]
    if m:
        work += [([32, 1, m, m], 9, order, True) for order in ALL_ORDERS]
    return work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x 1 x m^2 (0: skip)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    ap.add_argument("--only-composed-case", type=int, default=None)
    a = ap.parse_args()
    only = a.only_fused_case if a.only_fused_case is not None else a.only_composed_case
    if not torch.cuda.is_available():
        sys.exit("time_lcc_affine: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m)
    if only is not None:
        work = [work[only]]
    else:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    cache = {}
    for bshape, window, order, hess in work:
        B, C, shape = bshape[0], bshape[1], bshape[2:]
        dim = len(shape)
        key = tuple(bshape)
        if key not in cache:
            cache.clear()
            interpol.backend.release_workspaces()
            torch.cuda.empty_cache()
            moving = torch.randn([B, C, *shape], generator=gen)
            cache[key] = (moving.to(dev), (0.8 * moving + 0.3 * torch.randn([B, C, *shape], generator=gen)).to(dev))
        moving, fixed = cache[key]
        mat = torch.tensor(MATS[dim], device=dev)
        kw = dict(window=window, interpolation=order, bound="dct2", extrapolate=True, hessian=hess)
        call = lambda: interpol.lcc_gauss_newton_affine(moving, fixed, mat, **kw)
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
            res = dict(route=name, shape=bshape, window=window, order=order, hessian=hess, calls=len(ms[name]), call_ms=stats(ms[name]))
            if name == "fused":
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
                per = model_bytes(C)
                nbytes = sum(per) * B * fixed[0, 0].numel()
                res.update(model_bytes_per_sample=list(per), model_ms_at_measured_copy_rate=round(nbytes / (rate * 1e12) * 1e3, 4),
                           model_ms_at_6_29_TBps=round(nbytes / (PEAK_COPY_TBPS * 1e12) * 1e3, 4))
                res.update(fraction_of_measured_copy_rate=round(res["model_ms_at_measured_copy_rate"] / res["call_ms"]["median"], 3),
                           fraction_of_6_29_TBps=round(res["model_ms_at_6_29_TBps"] / res["call_ms"]["median"], 3))
            print(json.dumps(res), flush=True)
        diff = {k: float("%.3g" % float((f.double() - c.double()).abs().max() / c.double().abs().max()))
                for k, f, c in zip(("loss", "gradient", "hessian"), out["fused"], out["composed"]) if f is not None}
        print(json.dumps(dict(shape=bshape, window=window, order=order, hessian=hess, max_difference_fused_composed_over_largest_entry=diff)), flush=True)
        out.clear()


if __name__ == "__main__":
    main()
