#!/usr/bin/env python
"""Owner-computes push (FLAG_BINNED_SCATTER), cubic, dct2, C = 2, n^3: the first-writer flush of the colour launches (the default)
against load + add + store for every flushed point (FLAG_RMW_FLUSH) in ONE process -- median over 9 timings of 4 calls each, ms per
call, target zero-filled by the call.
argv: [n = 256] [batch sizes = 4] [fields = sigma2,identity,smooth] [orders = 3]: i.i.d. sigma = 2, the identity, a smooth field
(bench.smooth_grid); sigma6: i.i.d. sigma = 6 (sparser bricks, and own_bin scatters the strays itself: dirty bricks).  The two sides
alternate per field and batch size, the rmw one first, each measured twice: the difference between the two measurements of one side is
the noise the difference between the sides has to beat.  `equal`: the two results agree bit for bit; `maxdiff`: else the largest
difference over max |result| (i.i.d. fields without a clamp: the samples furthest out are scattered with float atomics)."""
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
SIDES = (("rmw", _hip.FLAG_RMW_FLUSH), ("first_writer", 0), ("rmw_again", _hip.FLAG_RMW_FLUSH), ("first_writer_again", 0))
for B in batches:
    inp, grid2 = bench.make_inputs(B, 2, n, 2.0, dev, 1234)
    make = {"sigma2": lambda: grid2, "identity": lambda: interpol.identity_grid([n] * 3, device=dev)[None].expand(B, n, n, n, 3).contiguous(),
            "smooth": lambda: bench.smooth_grid(B, n, 2.0, dev, 1234), "sigma6": lambda: bench.make_inputs(B, 2, n, 6.0, dev, 1234)[1]}
    out = torch.empty_like(inp)
    for name in wanted:
        grid = make[name]()
        for order in orders:
            res = {"op": "push", "B": B, "n": n, "field": name, "order": order}
            outs = {}
            for label, extra in SIDES:
                fl = _hip.FLAG_BINNED_SCATTER | extra
                med, lo, hi = timeit(lambda: _hip.scatter("push", inp, grid, None, [3] * 3, [order] * 3, 1, flags=fl, out=out))
                res[label] = {"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
                outs[label] = out.clone() if label in ("rmw", "first_writer") else None
            res["noise"] = round(max(abs(res["rmw"]["ms"] - res["rmw_again"]["ms"]), abs(res["first_writer"]["ms"] - res["first_writer_again"]["ms"])), 4)
            res["gain"] = round(min(res["rmw"]["ms"], res["rmw_again"]["ms"]) - max(res["first_writer"]["ms"], res["first_writer_again"]["ms"]), 4)
            res["equal"] = bool(torch.equal(outs["rmw"], outs["first_writer"]))
            res["maxdiff"] = float((outs["rmw"] - outs["first_writer"]).abs().max() / outs["rmw"].abs().max())
            print(json.dumps(res), flush=True)
            del outs
        del grid
    del inp, out, grid2
    torch.cuda.empty_cache()
