#!/usr/bin/env python
"""Golden vectors for the Jacobian of a displacement field at its lattice points, recorded from the live reference:

    want = interpol_ref.grid_grad(u channel-first, interpol_ref.identity_grid(shape), interpolation, bound, extrapolate=True)

in float64, moved to (B, *shape, D, D) (row = component, column = direction); the identity is NOT added.  Run once with
the reference checkout on the path,

    INTERPOL_REFERENCE=/path/to/torch-interpol python tests/golden/make_golden_jacobian.py

-> tests/golden/golden_jacobian.npz (arrays only).  The reference never travels: only these inputs / outputs do.
The inputs travel with the results (tests/test_jacobian_cpu.py rebuilds nothing): `u` is randn rounded to float32, stored
in float32 (exact) and used in float64."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.environ["INTERPOL_REFERENCE"])
import interpol as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]
SHAPES = {2: (19, 11), 3: (9, 5, 13)}
# (order, bound) per dim count
CASES = {2: ((1, "dft"), (1, "dst1"), (2, "zero"), (2, "dct2"), (3, "dct2"), (3, "dst1")),
         3: ((1, "dft"), (1, "zero"), (2, "dst1"), (2, "dft"), (3, "dct2"), (3, "zero"))}


def main():
    gen = torch.Generator().manual_seed(20262)
    out = {}
    for dim, shape in SHAPES.items():
        u = torch.randn([1, *shape, dim], generator=gen, dtype=torch.float32)
        out["d%d_u" % dim] = u.numpy()
        u64 = u.double()
        grid = ref.identity_grid(shape, dtype=torch.float64)[None]
        for k, (order, bound) in enumerate(CASES[dim]):
            g = ref.grid_grad(u64.movedim(-1, 1), grid, interpolation=order, bound=bound, extrapolate=True, prefilter=False)
            out["d%d_c%d_want" % (dim, k)] = g.movedim(1, -2).contiguous().numpy()
            out["d%d_c%d_case" % (dim, k)] = np.array([order, BOUNDS.index(bound)], dtype=np.int64)
    path = os.path.join(HERE, "golden_jacobian.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
