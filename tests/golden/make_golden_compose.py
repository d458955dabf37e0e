#!/usr/bin/env python
"""Golden vectors for the composition of displacement fields, recorded from the live reference:

    want = right + interpol_ref.grid_pull(left channel-first, interpol_ref.add_identity_grid(right), ...)

in float64.  Run once with the reference checkout on the path,

    INTERPOL_REFERENCE=/path/to/torch-interpol python tests/golden/make_golden_compose.py

-> tests/golden/golden_compose.npz (arrays only).  The reference never travels: only these inputs / outputs do.
The inputs travel with the results (tests/test_compose_cpu.py rebuilds nothing): `left` is randn rounded to float32, `right`
holds multiples of 1/64 in [-6, 6]; both are stored in float32 (exact) and used in float64."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ["INTERPOL_REFERENCE"])
import interpol as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {2: ((13, 22), (19, 11)), 3: ((13, 10, 17), (11, 14, 9))}
# (order, bound, extrapolate) per dim count
CASES = {2: ((1, "dft", 1), (2, "zero", 0), (3, "dct2", 1), (3, "dst1", 2)),
         3: ((1, "dft", 1), (3, "dct2", 0))}


def main():
    gen = torch.Generator().manual_seed(20261)
    out = {}
    for dim, (lshape, oshape) in SHAPES.items():
        left = torch.randn([1, *lshape, dim], generator=gen, dtype=torch.float32)
        right = torch.randint(-384, 385, [1, *oshape, dim], generator=gen).to(torch.float32) / 64
        out["d%d_left" % dim] = left.numpy()
        out["d%d_right" % dim] = right.numpy()
        l64, r64 = left.double(), right.double()
        for k, (order, bound, ex) in enumerate(CASES[dim]):
            pulled = ref.grid_pull(l64.movedim(-1, 1), ref.add_identity_grid(r64), interpolation=order, bound=bound,
                                   extrapolate=ex, prefilter=False)
            out["d%d_c%d_want" % (dim, k)] = (r64 + pulled.movedim(1, -1)).numpy()
            out["d%d_c%d_case" % (dim, k)] = np.array([order, ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"].index(bound), ex],
                                                      dtype=np.int64)
    path = os.path.join(HERE, "golden_compose.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
