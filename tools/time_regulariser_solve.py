"""The conjugate-gradient solve of (H + L) x = g for displacement fields, composed route against fused route.

Workloads, float32, `max_iter` = 16 and `tolerance` = 0 (every iteration runs):
  1 x n^3 x 3 (n = 256): weights membrane only, bending only, all three; Hessian none, diagonal, full; bounds dft and dct2;
  32 x m^2 x 2 (m = 1024): all three terms, full Hessian, dft.
g is i.i.d. normal; the full Hessian is 0.5 R R^T / D (R normal), the diagonal one 0.2 rand.

  composed : interpol.regulariser_solve with `interpol.backend.fused_regulariser_solve = False` -- the same algorithm around
             `ops.regulariser` (the fused L v), element-wise passes, double reductions and torch.where masks
             (interpol/torch_kernels.py): what a user writes today, without the `.item()` synchronisations;
  fused    : the same call with the backend switch on (csrc/regulariser_solve.hip).

Method: one process; the copy rate of the session is measured first (a 1 GiB float32 `copy_`, read + write); per row `--warmup`
warm-up calls, then `--steps` calls (composed: `--composed-steps`), each timed with a pair of events; the median and the
10th / 90th percentiles of ms per call are printed, and ms per iteration = median / max_iter (the set-up -- init and one
scalars launch -- is inside).  One JSON line per (route, shape, bound, weights, hessian).  The fused lines also carry the time of
the byte model per iteration (matvec: p read, q written, H; update: x and r read and written, p, q read, z written, H;
direction: z read, p read and written -- 12 D + 2 K elements per lattice point, 192 B for 3-D float32 with a full Hessian) at
the measured copy rate, and the fraction of it that was reached.

`--only-fused-case I` runs row I on the fused route alone, `--steps` times after the warm-up and prints nothing else: the
program to put behind a kernel tracer for the per-kernel split (tracing slows the host: never in the timed run).
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

WEIGHTS = dict(membrane=dict(membrane=1.0), bending=dict(bending=1.0), all=dict(absolute=0.3, membrane=0.7, bending=1.3))
MAX_ITER = 16


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
    """TB/s of a 1 GiB float32 copy (bytes read + bytes written over the median time of 20 copies)"""
    src = torch.randn(1 << 28, device=dev)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), 20, 5)
    return 2 * src.numel() * 4 / (t["median"] * 1e-3) / 1e12


def hessian(kind, B, shape, gen, dev):
    dim = len(shape)
    if kind == "none":
        return None
    if kind == "diag":
        return (0.2 * torch.rand([B, *shape, dim], generator=gen)).to(dev)
    out = torch.empty([B, *shape, dim * (dim + 1) // 2], device=dev)
    for b in range(B):                                                   # (item by item: R is D times the field)
        R = torch.randn([*shape, dim, dim], generator=gen).to(dev)
        H = 0.5 * (R[..., :, None, :] * R[..., None, :, :]).sum(-1) / dim        # (R R^T per point, element-wise: no batched GEMM)
        out[b] = torch.stack([H[..., d, d] for d in range(dim)] + [H[..., i, j] for i in range(dim) for j in range(i + 1, dim)], -1)
    return out


def rows(n, m):
    work = []
    if n:
        # (the Hessian outermost: it is built once per kind)
        work += [([1, n, n, n], b, w, h) for h in ("none", "diag", "full") for b in ("dft", "dct2") for w in ("membrane", "bending", "all")]
    if m:
        work += [([32, m, m], "dft", "all", "full")]
    return work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["composed", "fused", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice, 1 x n^3 x 3 (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x m^2 x 2 (0: skip)")
    ap.add_argument("--only-fused-case", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_regulariser_solve: needs a GPU (no timing is taken on the CPU)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = rows(a.n, a.m)
    if a.only_fused_case is not None:
        work = [work[a.only_fused_case]]
    else:
        rate = copy_rate(dev)
        print(json.dumps(dict(copy_rate_TBps=round(rate, 3), what="1 GiB float32 copy_, read + write, median of 20")), flush=True)
    last, g, hs = None, None, {}
    for bshape, bound, wname, hkind in work:
        B, shape = bshape[0], bshape[1:]
        dim = len(shape)
        if last != bshape:
            g, hs, last = None, {}, bshape
            torch.cuda.empty_cache()
            g = torch.randn([B, *shape, dim], generator=gen).to(dev)
        if hkind not in hs:
            hs.clear()
            torch.cuda.empty_cache()
            hs[hkind] = hessian(hkind, B, shape, gen, dev)
        h = hs[hkind]
        kw = dict(bound=bound, max_iter=MAX_ITER, tolerance=0., **WEIGHTS[wname])
        call = lambda: interpol.regulariser_solve(g, h, **kw)
        if a.only_fused_case is not None:
            interpol.backend.fused_regulariser_solve = True
            for _ in range(a.warmup + a.steps):
                call()
            torch.cuda.synchronize()
            return
        out = {}
        for route in (("composed", "fused") if a.route == "both" else (a.route,)):
            interpol.backend.fused_regulariser_solve = route == "fused"
            steps = a.steps if route == "fused" else a.composed_steps
            res = dict(route=route, shape=list(g.shape), bound=bound, weights=wname, hessian=hkind, max_iter=MAX_ITER, steps=steps,
                       call_ms=timed(call, steps, a.warmup if route == "fused" else 1))
            res["ms_per_iteration"] = round(res["call_ms"]["median"] / MAX_ITER, 4)
            out[route] = call()
            if route == "fused":
                K = 0 if h is None else h.shape[-1]
                nbytes = (12 * dim + 2 * K) * 4 * (g.numel() // dim)
                model = nbytes / (rate * 1e12) * 1e3
                res.update(model_bytes_per_point=(12 * dim + 2 * K) * 4, model_ms_per_iteration=round(model, 4),
                           fraction_of_model=round(model / res["ms_per_iteration"], 3))
            print(json.dumps(res), flush=True)
        interpol.backend.fused_regulariser_solve = True
        if len(out) == 2:
            # the two routes order their sums differently: the difference is reported against the solution's size
            diff = float((out["fused"] - out["composed"]).abs().max()) / float(out["composed"].abs().max())
            print(json.dumps(dict(shape=list(g.shape), bound=bound, weights=wname, hessian=hkind,
                                  max_difference_fused_composed_over_max=float("%.3g" % diff))), flush=True)
        out.clear()


if __name__ == "__main__":
    main()
