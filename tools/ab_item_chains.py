#!/usr/bin/env python
"""Owner-computes push (FLAG_BINNED_SCATTER), cubic, dct2, C = 2, n^3: the item chains against the single-stream schedule
(FLAG_SERIAL_ITEMS) in ONE process -- median over 9 timings of 4 calls each, ms per call, target zero-filled by the call.
argv: [n = 256] [batch sizes = 2,4,8] [fields = sigma2,identity,smooth]: i.i.d. sigma = 2, the identity, a smooth field
(bench.smooth_grid).  The two schedules alternate per field and batch size, the serial one first; `equal`: the two results agree
bit for bit (not expected at sigma = 2 without a clamp: the samples furthest out reach the shell bricks, float atomics)."""
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
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
batches = [int(b) for b in sys.argv[2].split(",")] if len(sys.argv) > 2 else [2, 4, 8]
wanted = sys.argv[3].split(",") if len(sys.argv) > 3 else ["sigma2", "identity", "smooth"]
for B in batches:
    inp, grid2 = bench.make_inputs(B, 2, n, 2.0, dev, 1234)
    fields = {"sigma2": grid2, "identity": interpol.identity_grid([n] * 3, device=dev)[None].expand(B, n, n, n, 3).contiguous(),
              "smooth": bench.smooth_grid(B, n, 2.0, dev, 1234)}
    del grid2
    fields = {k: v for k, v in fields.items() if k in wanted}
    out = torch.empty_like(inp)
    for name, grid in fields.items():
        res = {"B": B, "n": n, "field": name}
        outs = {}
        for label, extra in (("serial", _hip.FLAG_SERIAL_ITEMS), ("chains", 0), ("serial_again", _hip.FLAG_SERIAL_ITEMS), ("chains_again", 0)):
            fl = _hip.FLAG_BINNED_SCATTER | extra
            med, lo, hi = timeit(lambda: _hip.scatter("push", inp, grid, None, [3] * 3, [3] * 3, 1, flags=fl, out=out))
            res[label] = {"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
            outs[label] = out.clone() if label in ("serial", "chains") else None
        res["equal"] = bool(torch.equal(outs["serial"], outs["chains"]))
        print(json.dumps(res), flush=True)
        del outs
    del fields, inp, out
    torch.cuda.empty_cache()
