#!/usr/bin/env python
"""Owner-computes push (FLAG_BINNED_SCATTER), cubic, dct2, C = 2, n^3: the colour instantiation of own_accumulate (the default)
against the general kernel for every launch (FLAG_GENERAL_KERNELS) in ONE process -- median over 9 timings of 4 calls each, ms per
call, target zero-filled by the call.
argv: [n = 256] [batch sizes = 4] [fields = sigma2,identity,smooth] [orders = 3]: i.i.d. sigma = 2, the identity, a smooth field
(bench.smooth_grid).  The two sides alternate per field and batch size, the general one first, each measured twice: the difference
between the two measurements of one side is the noise the difference between the sides has to beat.  `equal`: the two results agree
bit for bit (not expected at sigma = 2 without a clamp: the samples furthest out reach the shell bricks, float atomics).
The pull has no second instantiation (profiles/lean_kernels.txt: the census found nothing to remove from its tile loop): the
flag changes nothing there."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-interpol_amd")); sys.path.insert(0, ROOT)
import torch, interpol, bench
from interpol import _hip
dev = torch.device("cuda", 0)
def timeit(fn, reps=9, inner=4):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]
args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 256
batches = [int(b) for b in args[1].split(",")] if len(args) > 1 else [4]
wanted = args[2].split(",") if len(args) > 2 else ["sigma2", "identity", "smooth"]
orders = [int(o) for o in args[3].split(",")] if len(args) > 3 else [3]
SIDES = (("general", _hip.FLAG_GENERAL_KERNELS), ("lean", 0), ("general_again", _hip.FLAG_GENERAL_KERNELS), ("lean_again", 0))
for B in batches:
    inp, grid2 = bench.make_inputs(B, 2, n, 2.0, dev, 1234)
    fields = {"sigma2": grid2, "identity": interpol.identity_grid([n] * 3, device=dev)[None].expand(B, n, n, n, 3).contiguous(),
              "smooth": bench.smooth_grid(B, n, 2.0, dev, 1234)}
    del grid2
    fields = {k: v for k, v in fields.items() if k in wanted}
    out = torch.empty_like(inp)
    for name, grid in fields.items():
        for order in orders:
            res = {"op": "push", "B": B, "n": n, "field": name, "order": order}
            outs = {}
            for label, extra in SIDES:
                fl = _hip.FLAG_BINNED_SCATTER | extra
                med, lo, hi = timeit(lambda: _hip.scatter("push", inp, grid, None, [3] * 3, [order] * 3, 1, flags=fl, out=out))
                res[label] = {"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
                outs[label] = out.clone() if label in ("general", "lean") else None
            res["noise"] = round(max(abs(res["general"]["ms"] - res["general_again"]["ms"]), abs(res["lean"]["ms"] - res["lean_again"]["ms"])), 4)
            res["gain"] = round(min(res["general"]["ms"], res["general_again"]["ms"]) - max(res["lean"]["ms"], res["lean_again"]["ms"]), 4)
            res["equal"] = bool(torch.equal(outs["general"], outs["lean"]))
            print(json.dumps(res), flush=True)
            del outs
    del fields, inp, out
    torch.cuda.empty_cache()
