"""The sum-of-squares data term on the matrix of an affine lattice (loss, gradient, P x P Hessian), composed route against fused.

Workloads, float32, bound dct2, extrapolate = True, moving and fixed i.i.d. normal images on one lattice, one dyadic
rotation-shear-translation matrix (multiples of 1/32) for every item:
  1 x 1 x n^3 (n = 256): orders 1, 2, 3, with and without the Hessian;
  4 x 2 x n^3          : cubic, with the Hessian (the shape of the README's affine row);
  32 x 1 x m^2 (m = 1024): orders 1, 2, 3, with the Hessian.

  composed : interpol.ssd_gauss_newton_affine with `interpol.backend.fused_ssd_affine_orders = ()` -- a dense lattice per item,
             `ssd_gauss_newton` at lattice - identity (itself routed as `backend.fused_ssd_orders` says) and the float64 contraction
             of its per-sample gradient and Hessian with the index moments (interpol/torch_kernels.py:
             ssd_gauss_newton_affine_composed);
  fused    : the same call with every order routed to csrc/ssd_affine.hip.

Method: one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read + write); per row the two
routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after `--warmup` warm-up calls each, every
call timed with a pair of events; the median and the 10th / 90th percentiles of ms per call over all blocks are printed.  One JSON
line per (route, row).  The fused lines also carry the time of the byte model -- per sample and channel the fixed value and the
footprint of the taps in the moving image, which an affine lattice close to the identity reads once: 4 C (1 + 1) bytes per sample
-- at the measured copy rate and at 6.29 TB/s, and the fractions of both that were reached.  After each row the largest difference
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
import interpol  # noqa: E402

PEAK_COPY_TBPS = 6.29
ALL_ORDERS = (1, 2, 3)
MATS = {
    3: [[0.96875, 0.125, -0.0625, 2.53125], [-0.125, 1.0, 0.09375, 1.71875], [0.0625, -0.09375, 0.96875, 3.09375]],
    2: [[0.96875, 0.125, 2.53125], [-0.125, 1.03125, 1.71875]],
}


def route(orders):
    interpol.backend.fused_ssd_affine_orders = orders


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


def copy_rate(dev):
    """TB/s of a 1 GiB float32 copy (bytes read + bytes written over the median time of 20 copies)"""
    src = torch.randn(1 << 28, device=dev)
    dst = torch.empty_like(src)
    t = stats(times(lambda: dst.copy_(src), 20, 5))
    return 2 * src.numel() * 4 / (t["median"] * 1e-3) / 1e12


def rows(n, m):
    work = []
    if n:
        work += [([1, 1, n, n, n], order, hess) for order in ALL_ORDERS for hess in (True, False)]
        work += [([4, 2, n, n, n], 3, True)]
    if m:
        work += [([32, 1, m, m], order, True) for order in ALL_ORDERS]
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
        sys.exit("time_ssd_affine: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m)
    if only is not None:
        work = [work[only]]
    else:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    cache = {}
    for bshape, order, hess in work:
        B, C, shape = bshape[0], bshape[1], bshape[2:]
        dim = len(shape)
        key = tuple(bshape)
        if key not in cache:
            cache.clear()
            interpol.backend.release_workspaces()
            torch.cuda.empty_cache()
            cache[key] = (torch.randn([B, C, *shape], generator=gen).to(dev), torch.randn([B, C, *shape], generator=gen).to(dev))
        moving, fixed = cache[key]
        mat = torch.tensor(MATS[dim], device=dev)
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian=hess)
        call = lambda: interpol.ssd_gauss_newton_affine(moving, fixed, mat, **kw)
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
            res = dict(route=name, shape=bshape, order=order, hessian=hess, calls=len(ms[name]), call_ms=stats(ms[name]))
            if name == "fused":
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
                per = 4 * C * (1 + 1)
                nbytes = per * B * fixed[0, 0].numel()
                res.update(model_bytes_per_sample=per, model_ms_at_measured_copy_rate=round(nbytes / (rate * 1e12) * 1e3, 4),
                           model_ms_at_6_29_TBps=round(nbytes / (PEAK_COPY_TBPS * 1e12) * 1e3, 4))
                res.update(fraction_of_measured_copy_rate=round(res["model_ms_at_measured_copy_rate"] / res["call_ms"]["median"], 3),
                           fraction_of_6_29_TBps=round(res["model_ms_at_6_29_TBps"] / res["call_ms"]["median"], 3))
            print(json.dumps(res), flush=True)
        diff = {k: float("%.3g" % float((f.double() - c.double()).abs().max() / c.double().abs().max()))
                for k, f, c in zip(("loss", "gradient", "hessian"), out["fused"], out["composed"]) if f is not None}
        print(json.dumps(dict(shape=bshape, order=order, hessian=hess, max_difference_fused_composed_over_largest_entry=diff)), flush=True)
        out.clear()


if __name__ == "__main__":
    main()
