#!/usr/bin/env python
"""Owner-computes push (FLAG_BINNED_SCATTER), cubic, C = 2, n^3: the shell samples of a tile that has few of them scattered by own_bin
(the default) against every run published (FLAG_SHELL_RUNS) in ONE process -- median over 9 timings of 4 calls each, ms per call, target zero-filled by
the call.  argv: [n = 256] [batch sizes = 4] [fields = headline,zoom,dft] [thresholds = 4,16,64]
  headline: bench.make_inputs (identity + N(0, 2^2)), dct2 -- a few dozen stray samples in the shell, each alone in its brick;
  zoom:     the same noise on a zoom of 1.25 about the centre, dct2 -- thick shell runs with a thin fringe;
  dft:      the headline field under dft -- a non-folding bound: every wrapping stencil is shell work.
The thresholds other than THIN_SHELL_RUN (16) are reached through the debug bits 64 / 128 (push_owner.hip: try_owner_push); a
threshold written r4 / r16 / r64 selects, with debug bit 256, the per-RUN rule (every run of at most that many samples, however
many shell samples the tile has) instead of the per-tile one.  The two
sides alternate per field and threshold, the flag side first, each measured twice: the difference between the two measurements of one
side is the noise the difference between the sides has to beat.  `maxdiff`: max |default - flag| / max |flag| (float atomics on both
sides wherever a stencil of the shell lands)."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-interpol_amd")); sys.path.insert(0, ROOT)
import torch, interpol, bench
from interpol import _hip
dev = torch.device("cuda", 0)
DCT2, DFT = 3, 6
DEBUG = {"16": 0, "4": 64 << 8, "64": 128 << 8}       # threshold -> bits of interpol_problem.flags
DEBUG.update({"r" + k: v | (256 << 8) for k, v in list(DEBUG.items())})
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
wanted = args[2].split(",") if len(args) > 2 else ["headline", "zoom", "dft"]
thresholds = args[3].split(",") if len(args) > 3 else ["4", "16", "64"]
for B in batches:
    inp, grid = bench.make_inputs(B, 2, n, 2.0, dev, 1234)
    out = torch.empty_like(inp)
    for name in wanted:
        if name == "zoom":
            c = (n - 1) / 2
            field, bound = (grid + 0.25 * (interpol.identity_grid([n] * 3, device=dev) - c)).contiguous(), DCT2
        else:
            field, bound = grid, DFT if name == "dft" else DCT2
        for thr in thresholds:
            res = {"op": "push", "B": B, "n": n, "field": name, "threshold": thr}
            sides = (("runs", _hip.FLAG_SHELL_RUNS), ("thin", DEBUG[thr]), ("runs_again", _hip.FLAG_SHELL_RUNS), ("thin_again", DEBUG[thr]))
            outs = {}
            for label, extra in sides:
                fl = _hip.FLAG_BINNED_SCATTER | extra
                med, lo, hi = timeit(lambda: _hip.scatter("push", inp, field, None, [bound] * 3, [3] * 3, 1, flags=fl, out=out))
                res[label] = {"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
                if label in ("runs", "thin"):
                    outs[label] = out.clone()
            res["noise"] = round(max(abs(res["runs"]["ms"] - res["runs_again"]["ms"]), abs(res["thin"]["ms"] - res["thin_again"]["ms"])), 4)
            res["gain"] = round(min(res["runs"]["ms"], res["runs_again"]["ms"]) - max(res["thin"]["ms"], res["thin_again"]["ms"]), 4)
            res["maxdiff"] = float((outs["runs"] - outs["thin"]).abs().max() / outs["runs"].abs().max())
            print(json.dumps(res), flush=True)
            del outs
        del field
    del inp, grid, out
    torch.cuda.empty_cache()
