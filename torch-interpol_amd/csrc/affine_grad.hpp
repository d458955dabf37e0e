// ===========================================================================
// affine_grad.hpp -- what affine_grad.hip (the kernels) and abi.hip (the entry points) share.
// ===========================================================================
#pragma once
#include <stdint.h>

namespace ip {

// Persistent workgroups of affine_grad_partial = rows of D (D+1) doubles in the workspace.  A CONSTANT, so that the order of
// the sums -- and with it every bit of the result -- does not depend on the shape: 8 workgroups of 4 waves per CU on 256 CUs.
constexpr int AG_BLOCKS = 2048;

inline int64_t affine_grad_workspace_bytes(int dim) { return (int64_t)AG_BLOCKS * dim * (dim + 1) * (int64_t)sizeof(double); }

} // namespace ip
