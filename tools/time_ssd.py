"""The sum-of-squares data term of a Gauss-Newton step (loss, gradient, Hessian), composed route against fused route.

Workloads, float32, bound dct2, extrapolate = True, fields smooth (a few low Fourier modes, amplitude 2 voxels) or rough (i.i.d.
normal, sigma = 2 voxels), moving and fixed i.i.d. normal images on one lattice:
  1 x 1 x n^3 (n = 256): every order of `--orders`, both fields, hessian 'full' and None;
  1 x 3 x n^3          : the same orders and fields, hessian 'full';
  32 x 1 x m^2 (m = 1024): the same orders and fields, hessian 'full';
  the step: ssd_gauss_newton + regulariser_solve (membrane, dct2, 16 iterations, tolerance 0) on 1 x 1 x n^3, hessian 'full'.

  composed : interpol.ssd_gauss_newton with `interpol.backend.fused_ssd_orders = ()` -- grid_pull, grid_grad at a displacement and
             the element-wise passes (interpol/torch_kernels.py: ssd_gauss_newton_composed): what a user writes today;
  fused    : the same call with every order routed to csrc/ssd.hip.

Method: one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read + write); per row the two
routes alternate in `--rounds` blocks of `--steps` calls (composed: `--composed-steps`) after `--warmup` warm-up calls each, every
call timed with a pair of events; the median and the 10th / 90th percentiles of ms per call over all blocks are printed.  One JSON
line per (route, row).  The fused lines also carry the time of the byte model (moving and fixed read once per channel, disp read, no
weight, gradient and Hessian written: 4 (2 C + 2 D + K) bytes per sample -- 56 B for 3-D, C = 1, full) at the measured copy
rate and at 6.29 TB/s, and the fractions of both that were reached.  After each row the largest difference between the routes'
outputs is printed against the natural scale of each output.

`--only-fused-case I` (`--only-composed-case I`) runs row I on that route alone, `--steps` times after the warm-up and prints
nothing else: the program to put behind a kernel tracer for the per-kernel split (tracing slows the host: never in the timed run).
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(os.environ.get("INTERPOL_PKG") or os.path.join(ROOT, "torch-interpol_amd"))
sys.path.insert(0, PKG)
import interpol  # noqa: E402

MAX_ITER = 16
PEAK_COPY_TBPS = 6.29
ALL_ORDERS = (1, 2, 3)


def route(orders):
    """the orders that go to the fused kernel, with and without a Hessian"""
    interpol.backend.fused_ssd_orders = interpol.backend.fused_ssd_orders_without_hessian = orders


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


def smooth_field(shape, amp, gen, dev):
    dim = len(shape)
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=dev) / n for n in shape], indexing="ij")
    v = torch.zeros([*shape, dim], device=dev)
    for d in range(dim):
        for _ in range(4):
            k = torch.randint(1, 3, [dim], generator=gen)
            ph = 2 * math.pi * float(torch.rand([], generator=gen))
            v[..., d] += torch.sin(2 * math.pi * sum(float(k[e]) * g[e] for e in range(dim)) + ph)
    return v * (amp / float(v.abs().max()))


def rows(n, m, orders):
    groups = []
    if n:
        groups += [("ssd", [1, 1, n, n, n], ("full", None)), ("step", [1, 1, n, n, n], ("full",)), ("ssd", [1, 3, n, n, n], ("full",))]
    if m:
        groups += [("ssd", [32, 1, m, m], ("full",))]
    # (the images and the field outermost: they are built once per shape and field)
    return [(what, bshape, order, field, kind) for what, bshape, kinds in groups for field in ("smooth", "rough")
            for order in orders for kind in kinds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--orders", default="1,3")
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x 1 x m^2 (0: skip)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    ap.add_argument("--only-composed-case", type=int, default=None)
    a = ap.parse_args()
    only = a.only_fused_case if a.only_fused_case is not None else a.only_composed_case
    if not torch.cuda.is_available():
        sys.exit("time_ssd: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m, [int(o) for o in a.orders.split(",")])
    if only is not None:
        work = [work[only]]
    else:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    cache = {}
    for what, bshape, order, fname, hkind in work:
        B, C, shape = bshape[0], bshape[1], bshape[2:]
        dim = len(shape)
        key = (tuple(bshape), fname)
        if key not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            moving = torch.randn([B, C, *shape], generator=gen).to(dev)
            fixed = torch.randn([B, C, *shape], generator=gen).to(dev)
            if fname == "smooth":
                disp = torch.stack([smooth_field(shape, 2.0, gen, dev) for _ in range(B)])
            else:
                disp = (2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev)
            cache[key] = (moving, fixed, disp)
        moving, fixed, disp = cache[key]
        kw = dict(interpolation=order, bound="dct2", extrapolate=True, hessian=hkind)
        if what == "ssd":
            call = lambda: interpol.ssd_gauss_newton(moving, fixed, disp, **kw)
        else:
            def call():
                loss, g, h = interpol.ssd_gauss_newton(moving, fixed, disp, **kw)
                return loss, interpol.regulariser_solve(g, h, membrane=1.0, bound="dct2", max_iter=MAX_ITER, tolerance=0.)
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
        K = {None: 0, "full": dim * (dim + 1) // 2}[hkind]
        for name in ("composed", "fused"):
            res = dict(route=name, what=what, shape=bshape, order=order, field=fname, hessian=hkind, calls=len(ms[name]),
                       call_ms=stats(ms[name]))
            if name == "fused":
                res["speedup_over_composed"] = round(stats(ms["composed"])["median"] / res["call_ms"]["median"], 2)
            if name == "fused" and what == "ssd":
                per = 4 * (2 * C + 2 * dim + K)
                nbytes = per * disp.numel() // dim
                res.update(model_bytes_per_sample=per, model_ms_at_measured_copy_rate=round(nbytes / (rate * 1e12) * 1e3, 4),
                           model_ms_at_6_29_TBps=round(nbytes / (PEAK_COPY_TBPS * 1e12) * 1e3, 4))
                res.update(fraction_of_measured_copy_rate=round(res["model_ms_at_measured_copy_rate"] / res["call_ms"]["median"], 3),
                           fraction_of_6_29_TBps=round(res["model_ms_at_6_29_TBps"] / res["call_ms"]["median"], 3))
            print(json.dumps(res), flush=True)
        if what == "ssd":
            # the routes order their sums differently: the differences are reported against the natural scale of each output
            m, f = float(moving.abs().max()), float(fixed.abs().max())
            lf, gf, hf = out["fused"]
            lc, gc, hc = out["composed"]
            diff = dict(loss=float(((lf - lc).abs() / lc.abs()).max()), gradient=float((gf - gc).abs().max()) / ((m + f) * m))
            if hf is not None:
                diff["hessian"] = float((hf - hc).abs().max()) / (m * m)
            print(json.dumps(dict(shape=bshape, order=order, field=fname, hessian=hkind,
                                  max_difference_fused_composed_over_scale={k: float("%.3g" % v) for k, v in diff.items()})), flush=True)
        out.clear()


if __name__ == "__main__":
    main()
