#!/usr/bin/env python
"""CPU census of the samples of a bench.py field whose first tap lies outside the interior bricks of the owner-computes push
(csrc/push_owner.hip: brick_grid): under a folding bound (dct2 / replicate / dct1, n >= 32) the interior first-tap cells of a dim are
[lo, top) = [-9, n + 6); a cubic's first tap is floor(x - 1).  Prints, per batch item: the stray samples, the shell bricks and the
16^3 sample tiles they come from, and the largest number of strays one tile sends into one brick (the run own_bin would publish).
No GPU.  argv: [n = 256] [batch = 4] [sigma = 2.0] [seed = 1234] [zoom = 1.0] -- the defaults are bench.py's headline field."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torch-interpol_amd")); sys.path.insert(0, ROOT)
import torch
args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 256
B = int(args[1]) if len(args) > 1 else 4
sigma = float(args[2]) if len(args) > 2 else 2.0
seed = int(args[3]) if len(args) > 3 else 1234
zoom = float(args[4]) if len(args) > 4 else 1.0
lo, top, BR, TS = -9, n + 6, 16, 16
g = torch.Generator().manual_seed(seed)
torch.randn([B, 2, n, n, n], generator=g, dtype=torch.float32)              # bench.make_inputs draws the sources first
ax = torch.arange(n, dtype=torch.float32)
c = (n - 1) / 2
total, tiles_total = 0, 0
for b in range(B):
    x = torch.randn([n, n, n, 3], generator=g, dtype=torch.float32).mul_(sigma)
    for d in range(3):
        shape = [1, 1, 1]; shape[d] = n
        x[..., d] += (c + zoom * (ax - c)).reshape(shape) if zoom != 1.0 else ax.reshape(shape)
    ft = torch.floor(x - 1.0).to(torch.int64)
    out = ((ft < lo) | (ft >= top)).any(-1)
    idx = out.nonzero()                                                   # (k, 3) sample indices
    f = ft[out]
    # brick per dim as brick_and_cell numbers the shell: below lo from lo downwards, above top from top upwards; interior cells: -1
    brick = torch.where(f < lo, -1 - ((lo - 1 - f) // BR), torch.where(f >= top, 1000 + (f - top) // BR, (f - lo) // BR))
    tile = idx // TS
    runs = {}
    for t, k in zip(map(tuple, tile.tolist()), map(tuple, brick.tolist())):
        runs[(t, k)] = runs.get((t, k), 0) + 1
    ntiles = len({t for t, _ in runs})
    nbricks = len({k for _, k in runs})
    print("item %d: %d stray samples in %d shell bricks from %d tiles, longest (tile, brick) run %d" % (b, len(idx), nbricks, ntiles, max(runs.values()) if runs else 0))
    total += len(idx); tiles_total += ntiles
print("total: %d of %d samples, from %d tiles" % (total, B * n ** 3, tiles_total))
