"""The linear-elastic terms of the regulariser (`shears`, `div`) and the 'sliding' bound, composed route against fused route.

Workloads, float32, i.i.d. normal fields (sigma = 2 voxels): 1 x n^3 x 3 (n = 256) and 32 x m^2 x 2 (m = 1024), bounds dft and
sliding.  Configurations: elastic alone, membrane + elastic, bending + elastic, all five -- and membrane alone and bending alone: under
sliding they run the elastic instantiations with a zero cross coefficient, under dft the three-term ones, and bending alone is the line that
bending + elastic is read against (the design claim: the cross taps ride on the diagonal loads of the mixed bending terms).

  composed : `interpol.backend.fused_regulariser = False` (L v, energy) resp. `fused_regulariser_solve = False` (the solve, around
             the fused L v) -- the index_select passes with per-component bounds of interpol/torch_kernels.py;
  fused    : the switches on (csrc/regulariser.hip, csrc/regulariser_solve.hip: the M_EL modes of reg_at).

Measured per (shape, bound, configuration): `regulariser` forward and `regulariser_energy` forward (no_grad), `regulariser_energy`
forward + backward, and `regulariser_solve` (max_iter = 8, tolerance = 0: every iteration runs) with no, a diagonal and a full
Hessian, as ms per iteration = median / max_iter.  Method (that of tools/time_regulariser.py): one process, `--warmup` warm-up
steps, then `--steps` (>= 20; composed: `--composed-steps`) steps, each timed with a pair of events; median and the 10th / 90th
percentiles.  One JSON line per (route, shape, bound, configuration).
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

EL = dict(shears=0.6, div=0.9)
CONFIGS = dict(membrane=dict(membrane=0.7), bending=dict(bending=1.3), elastic=EL, membrane_elastic=dict(membrane=0.7, **EL), bending_elastic=dict(bending=1.3, **EL),
               all_five=dict(absolute=0.3, membrane=0.7, bending=1.3, **EL))
MAX_ITER = 8


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


def hessian(kind, B, shape, gen, dev):
    dim = len(shape)
    if kind == "none":
        return None
    if kind == "diag":
        return (0.2 * torch.rand([B, *shape, dim], generator=gen)).to(dev)
    out = torch.empty([B, *shape, dim * (dim + 1) // 2], device=dev)
    for b in range(B):
        R = torch.randn([*shape, dim, dim], generator=gen).to(dev)
        H = 0.5 * (R[..., :, None, :] * R[..., None, :, :]).sum(-1) / dim
        out[b] = torch.stack([H[..., d, d] for d in range(dim)] + [H[..., i, j] for i in range(dim) for j in range(i + 1, dim)], -1)
    return out


def measure(field, bound, w, steps, warmup):
    kw = dict(bound=bound, **w)
    gy = torch.ones(field.shape[0], dtype=field.dtype, device=field.device)

    def matvec():
        with torch.no_grad():
            interpol.regulariser(field, **kw)

    def energy():
        with torch.no_grad():
            interpol.regulariser_energy(field, **kw)

    def energy_fwd_bwd():
        u = field.detach().requires_grad_()
        torch.autograd.grad(interpol.regulariser_energy(u, **kw), u, gy)

    return dict(matvec_ms=timed(matvec, steps, warmup), energy_ms=timed(energy, steps, warmup),
                energy_forward_backward_ms=timed(energy_fwd_bwd, steps, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["composed", "fused", "both"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--composed-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256, help="edge of the 3-D lattice, 1 x n^3 x 3 (0: skip)")
    ap.add_argument("--m", type=int, default=1024, help="edge of the 2-D lattices, 32 x m^2 x 2 (0: skip)")
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--bounds", nargs="+", default=["dft", "sliding"])
    ap.add_argument("--no-solve", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_elastic: needs a GPU (no timing is taken on the CPU)")
    if a.steps < 20:
        ap.error("--steps must be at least 20 (median of at least 20 steps)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    work = ([[1, a.n, a.n, a.n]] if a.n else []) + ([[32, a.m, a.m]] if a.m else [])
    for bshape in work:
        B, shape = bshape[0], bshape[1:]
        dim = len(shape)
        torch.cuda.empty_cache()
        field = (2.0 * torch.randn([B, *shape, dim], generator=gen)).to(dev)
        hs = {} if a.no_solve else {k: hessian(k, B, shape, gen, dev) for k in ("none", "diag", "full")}
        for bound in a.bounds:
            for name in a.configs:
                for route in (("composed", "fused") if a.route == "both" else (a.route,)):
                    interpol.backend.fused_regulariser = route == "fused"
                    steps = a.steps if route == "fused" else a.composed_steps
                    head = dict(route=route, shape=list(field.shape), bound=bound, config=name, steps=steps)
                    res = measure(field, bound, CONFIGS[name], steps, a.warmup if route == "fused" else 1)
                    interpol.backend.fused_regulariser = True                  # (the composed solve runs around the fused L v)
                    if not a.no_solve:
                        interpol.backend.fused_regulariser_solve = route == "fused"
                        for kind, h in hs.items():
                            kw = dict(bound=bound, max_iter=MAX_ITER, tolerance=0., **CONFIGS[name])
                            t = timed(lambda: interpol.regulariser_solve(field, h, **kw), steps, a.warmup if route == "fused" else 1)
                            res["solve_%s_ms_per_iteration" % kind] = round(t["median"] / MAX_ITER, 4)
                        interpol.backend.fused_regulariser_solve = True
                    print(json.dumps(dict(head, **res)), flush=True)


if __name__ == "__main__":
    main()
