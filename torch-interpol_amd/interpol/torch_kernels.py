"""Device-generic kernel table: the operators of `interpol/ops.py` in plain PyTorch.

The HIP library (`_hip.py`) covers D in {1, 2, 3} on the GPU.  Everything else the reference
accepts -- any number of spatial dims through its `nd` path (`pushpull.py:49-66`, `nd.py:80-464`)
and tensors that live on the CPU -- is served here, so that the package stays a drop-in.  This is
product code (the oracle under `oracle/` is test infrastructure and is never imported here); it is
NOT the fast path and is never taken for CUDA tensors of 1-3 spatial dims.

Formulation (not the reference's (K+1)^D sequential passes): per chunk of sample points the whole
stencil is materialised at once -- linear tap indices and tap weights of shape (B, n, T),
T = prod_d (K_d + 1) -- then ONE gather + weighted sum (pull / grad / hess) or ONE `scatter_add_`
(push / count / pushgrad).  Chunks bound the temporary to ~2^24 elements.

Numerical definition: stencil `nd.py:44-61`; weights = centred cardinal B-splines (`splines.py:30-195`),
evaluated with the Cox - de Boor recursion (equal to the reference's Horner forms up to rounding);
boundary conditions `bounds.py:30-89`; extrapolation mask `nd.py:10-27`; `iso0` / `iso1` semantics
for all-nearest / all-linear problems of D <= 3 (`pushpull.py:50-64`); backward compositions
`pushpull.py:237-325`.  Reference quirks kept: B-3 (dst1 sign 0 at index 0) and B-4 (order-1
gradient sign in the nd path); B-1 / B-2 follow the intended semantics, as the HIP kernels do.
"""
import torch

_CHUNK_ELEMS = 1 << 24


# ---------------------------------------------------------------------------
# boundary conditions (bounds.py:30-89): codes 0 zero, 1 replicate, 2 dct1, 3 dct2, 4 dst1, 5 dst2, 6 dft
# ---------------------------------------------------------------------------
def _pymod(a, m):
    return torch.remainder(a, m)


def bound_index(bound, i, n):
    """Bound.index: lattice index of tap position i (int64 tensor) on a lattice of n points."""
    if bound in (0, 1):
        return i.clamp(0, n - 1)
    if bound == 2:
        if n == 1:
            return torch.zeros_like(i)
        m = 2 * (n - 1)
        j = _pymod(i.abs(), m)
        return torch.where(j >= n, m - j, j)
    if bound in (3, 5):
        m = 2 * n
        j = torch.where(i < 0, m - 1 - _pymod(-i - 1, m), _pymod(i, m))
        return torch.where(j >= n, m - 1 - j, j)
    if bound == 4:
        m = 2 * (n + 1)
        j = _pymod(torch.where(i < 0, -i - 2, i), m)
        j = torch.where(j > n, m - 2 - j, j)
        j = torch.where(j == -1, torch.zeros_like(j), j)
        return torch.where(j == n, torch.full_like(j, n - 1), j)
    if bound == 6:
        return _pymod(i, n)
    raise ValueError('Unknown boundary condition code {}'.format(bound))


def bound_sign(bound, i, n):
    """Bound.transform as a multiplicative factor (None -> no tensor: returns None)."""
    if bound == 0:
        return ((i >= 0) & (i < n)).to(torch.int8)
    if bound == 5:
        j = torch.where(i < 0, n - 1 - i, i)
        odd = (torch.div(j, n, rounding_mode='floor') % 2) == 1
        return torch.where(odd, -torch.ones_like(i), torch.ones_like(i)).to(torch.int8)
    if bound == 4:
        if n == 1:
            return None
        m = 2 * (n + 1)
        j = _pymod(torch.where(i < 0, -i + (n - 1), i), m)
        s = (j != 0) & (_pymod(j, n + 1) != n)                       # quirk B-3: 0 at j == 0
        odd = (torch.div(j, n + 1, rounding_mode='floor') % 2) == 1
        return torch.where(odd, -s.to(torch.int8), s.to(torch.int8))
    return None


# ---------------------------------------------------------------------------
# B-spline weights (splines.py:30-195)
# ---------------------------------------------------------------------------
def _bspline(order, x):
    """beta^order(x), Cox - de Boor; exact on the support, 0 outside."""
    if order == 0:
        return torch.ones_like(x)
    if order == 1:
        return (1 - x.abs()).clamp_min(0)
    h = 0.5 * (order + 1)
    return ((x + h) * _bspline(order - 1, x + 0.5) + (h - x) * _bspline(order - 1, x - 0.5)) / order


def _bspline0(x):
    # the order-0 factor of the recursion for derivatives: indicator of [-1/2, 1/2)
    return ((x >= -0.5) & (x < 0.5)).to(x.dtype)


def _bspline_rec(order, x):
    """beta^order with the TRUE order-0 base case (needed below order 1 by the derivative recursions)."""
    if order == 0:
        return _bspline0(x)
    return _bspline(order, x)


def _dbspline(order, x, nd_quirk):
    """d/dx beta^order(x)  (fastgrad).  Order 1 in the reference's nd path returns +sign(x) (quirk B-4)."""
    if order == 0:
        return torch.zeros_like(x)
    if order == 1:
        return torch.sign(x) if nd_quirk else -torch.sign(x)
    return _bspline_rec(order - 1, x + 0.5) - _bspline_rec(order - 1, x - 0.5)


def _d2bspline(order, x):
    """d2/dx2 beta^order(x)  (fasthess; zero for orders 0 and 1)."""
    if order < 2:
        return torch.zeros_like(x)
    if order == 2:
        # piecewise constant: the reference's piece choice at the breakpoints (splines.py:157-158)
        return torch.where(x.abs() < 0.5, torch.full_like(x, -2.0), torch.ones_like(x))
    return _dbspline(order - 1, x + 0.5, False) - _dbspline(order - 1, x - 0.5, False)


# ---------------------------------------------------------------------------
# the stencil of a chunk of samples
# ---------------------------------------------------------------------------
def _mode(order, dim):
    if dim <= 3 and all(o == 1 for o in order):
        return 'iso1'
    if dim <= 3 and all(o == 0 for o in order):
        return 'iso0'
    return 'nd'


class _Stencil:
    """Per dim d: idx[d] (B, n, K_d + 1) int64, w / g / h[d] same shape (sign folded in)."""

    def __init__(self, coords, shape, bound, order, need):
        dim = coords.shape[-1]
        mode = _mode(order, dim)
        self.idx, self.w, self.g, self.h = [], [], [], []
        for d in range(dim):
            x = coords[..., d]
            k = order[d]
            if mode == 'iso0':
                i0 = torch.round(x)                                  # iso0.py:12: half to even
            else:
                i0 = torch.floor(x - 0.5 * (k - 1))                  # nd.py:45 (iso1.py:13 for k = 1)
            t = x - i0                                               # nd.py:46
            i0 = i0.clamp(-2.0 ** 62, 2.0 ** 62).long()
            taps = torch.arange(k + 1, device=x.device)
            pos = i0[..., None] + taps
            xj = t[..., None] - taps.to(t.dtype)
            ii = bound_index(bound[d], pos, shape[d])
            sg = bound_sign(bound[d], pos, shape[d])
            if mode == 'iso1':
                w = torch.stack([1 - t, t], -1)                      # iso1.py:19-20
                g = torch.stack([-torch.ones_like(t), torch.ones_like(t)], -1) if need >= 1 else None
                h = torch.zeros_like(w) if need >= 2 else None
            else:
                w = _bspline(k, xj)
                g = _dbspline(k, xj, mode == 'nd') if need >= 1 else None
                h = _d2bspline(k, xj) if need >= 2 else None
            if sg is not None:
                sf = sg.to(w.dtype)
                w = w * sf
                g = g * sf if g is not None else None
                h = h * sf if h is not None else None
            self.idx.append(ii); self.w.append(w); self.g.append(g); self.h.append(h)
        self.dim = dim

    def _outer(self, factors):
        out = None
        for f in factors:
            out = f if out is None else (out[..., :, None] * f[..., None, :]).flatten(-2)
        return out

    def linear_index(self, shape):
        out, stride = None, 1
        strides = []
        for n in reversed(shape):
            strides.append(stride); stride *= n
        strides = strides[::-1]
        for d in range(self.dim):
            term = self.idx[d] * strides[d]
            out = term if out is None else (out[..., :, None] + term[..., None, :]).flatten(-2)
        return out

    def weights(self, deriv=()):
        """product of per-dim factors; dims listed in `deriv` use the gradient (once) or the hessian (twice)."""
        fs = []
        for d in range(self.dim):
            c = deriv.count(d)
            fs.append(self.w[d] if c == 0 else (self.g[d] if c == 1 else self.h[d]))
        return self._outer(fs)


def _mask(coords, shape, extrapolate):
    """nd.py:10-27: 1 inside the field of view (with tolerance), None when everything is kept."""
    if extrapolate == 1:
        return None
    thr = 0.05 if extrapolate == 0 else 0.55
    m = None
    for d, n in enumerate(shape):
        x = coords[..., d]
        md = (x > -thr) & (x < n - 1 + thr)
        m = md if m is None else m & md
    return m


def _chunks(n, per_sample):
    step = max(1, _CHUNK_ELEMS // max(1, per_sample))
    for a in range(0, n, step):
        yield a, min(n, a + step)


def _prep(grid, displacement):
    if hasattr(grid, 'dense'):
        grid = grid.dense()
    dim = grid.shape[-1]
    coords = grid.reshape(grid.shape[0], -1, dim)
    if displacement:
        from .utils import identity_grid
        ident = identity_grid(grid.shape[1:-1], dtype=grid.dtype, device=grid.device)
        coords = coords + ident.reshape(1, -1, dim)
    return coords, list(grid.shape[1:-1])


def _gather_op(inp, grid, bound, order, extrapolate, displacement, need):
    """pull (need 0) -> (B,C,*out); grad (need 1) -> (B,C,*out,D); hess (need 2) -> (B,C,*out,D,D)."""
    coords, oshape = _prep(grid, displacement)
    dim = coords.shape[-1]
    ishape = list(inp.shape[2:])
    B = max(inp.shape[0], coords.shape[0])
    C = inp.shape[1]
    dtype = torch.promote_types(inp.dtype, coords.dtype)
    flat = inp.reshape(inp.shape[0], C, -1).to(dtype).expand(B, C, -1)
    coords = coords.to(dtype).expand(B, -1, dim)
    N = coords.shape[1]
    trail = [] if need == 0 else ([dim] if need == 1 else [dim, dim])
    out = flat.new_zeros([B, C, N] + trail)
    ntap = 1
    for k in order:
        ntap *= k + 1
    for a, b in _chunks(N, B * C * ntap):
        cc = coords[:, a:b]
        st = _Stencil(cc, ishape, bound, order, need)
        lin = st.linear_index(ishape)                                            # (B, n, T)
        vals = torch.gather(flat, 2, lin.reshape(B, 1, -1).expand(B, C, -1)).reshape(B, C, b - a, -1)
        m = _mask(cc, ishape, extrapolate)
        mf = None if m is None else m.to(dtype)[:, None]
        if need == 0:
            r = (vals * st.weights()[:, None]).sum(-1)
            out[:, :, a:b] = r if mf is None else r * mf
        elif need == 1:
            for d in range(dim):
                r = (vals * st.weights((d,))[:, None]).sum(-1)
                out[:, :, a:b, d] = r if mf is None else r * mf
        else:
            for d in range(dim):
                for e in range(d, dim):
                    r = (vals * st.weights((d, e))[:, None]).sum(-1)
                    r = r if mf is None else r * mf
                    out[:, :, a:b, d, e] = r
                    if e != d:
                        out[:, :, a:b, e, d] = r
    return out.reshape([B, C] + oshape + trail)


def _scatter_op(inp, grid, shape, bound, order, extrapolate, displacement, trailing, out=None):
    """push (trailing 0: inp (B,C,*in)) / pushgrad (trailing 1: inp (B,C,*in,D)) / count (inp None) -> (B,C,*shape).
    `out` (1 or B, C, *shape): accumulate into it (a batch of 1 is shared by all items)."""
    coords, sshape = _prep(grid, displacement)
    dim = coords.shape[-1]
    shape = sshape if shape is None else [int(s) for s in shape]
    B = coords.shape[0] if inp is None else max(inp.shape[0], coords.shape[0])
    dtype = coords.dtype if inp is None else torch.promote_types(inp.dtype, coords.dtype)
    coords = coords.to(dtype).expand(B, -1, dim)
    N = coords.shape[1]
    if inp is None:
        C = 1
        src = None
    else:
        C = inp.shape[1]
        src = inp.to(dtype).reshape([inp.shape[0], C, N] + ([dim] if trailing else [])).expand([B, C, N] + ([dim] if trailing else []))
    nvox = 1
    for n in shape:
        nvox *= n
    if out is None:
        acc = coords.new_zeros([B, C, nvox])
    else:
        acc = out.reshape(out.shape[0], C, nvox)
    ntap = 1
    for k in order:
        ntap *= k + 1
    for a, b in _chunks(N, B * C * ntap):
        cc = coords[:, a:b]
        st = _Stencil(cc, shape, bound, order, 1 if trailing else 0)
        lin = st.linear_index(shape)                                             # (B, n, T)
        m = _mask(cc, shape, extrapolate)
        mf = None if m is None else m.to(dtype)[:, None]
        if trailing:
            contrib = None
            for d in range(dim):
                s = src[:, :, a:b, d]
                s = s if mf is None else s * mf                                  # nd.py:346-347: masked before the scatter
                term = s[..., None] * st.weights((d,))[:, None]
                contrib = term if contrib is None else contrib + term
        else:
            w = st.weights()[:, None]
            if src is None:
                contrib = w if mf is None else w * mf[..., None]
            else:
                s = src[:, :, a:b]
                s = s if mf is None else s * mf                                  # nd.py:201-203
                contrib = s[..., None] * w
        contrib = contrib.expand(B, C, b - a, ntap).reshape(B, C, -1)
        index = lin.reshape(B, 1, -1).expand(B, C, -1)
        if acc.shape[0] == 1 and B > 1:                                          # shared target: every item adds into it
            acc[0].scatter_add_(1, index.permute(1, 0, 2).reshape(C, -1), contrib.permute(1, 0, 2).reshape(C, -1))
        else:
            acc.scatter_add_(2, index, contrib)
    if out is not None:
        return out
    return acc.reshape([B, C] + shape)


def composed(table, left, right, bound, order, extrapolate):
    """compose(left, right) = right + pull(left, id + right) from the operators of a kernel table: the displacement field
    `left` (B,*lshape,D) is pulled as a D-channel image, which costs the two layout changes a fused kernel avoids."""
    pulled = table.pull(left.movedim(-1, 1), right, bound, order, extrapolate, displacement=True)
    return right + pulled.movedim(1, -1).to(right.dtype)


def composed_backward(table, grad, left, right, bound, order, extrapolate, need_left, need_right):
    """-> (grad_left (B,*lshape,D) | None, grad_right (B,*oshape,D) | None), one per batch item of `grad` (pushpull.py:237-258)"""
    gl, gr = table.pull_backward(grad.movedim(-1, 1), left.movedim(-1, 1), right, bound, order, extrapolate,
                                 need_left, need_right, displacement=True)
    if gl is not None:
        gl = gl.movedim(1, -1)
    if gr is not None:
        gr = grad + gr.to(grad.dtype)
    return gl, gr


def _work(t):
    """16-bit storage computes in float32 (and is rounded once, by the caller)"""
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


def _zero_disp(like):
    """the lattice points as a displacement: zero, with a batch of 1 that the kernels broadcast; like (B,*shape,D)"""
    return like.new_zeros([1, *like.shape[1:]])


def det_closed(J):
    """Determinant of (..., D, D) matrices: expanded along row 0 for D <= 3 (what csrc/jacobian.hip evaluates), LU above."""
    D = J.shape[-1]
    if D == 1:
        return J[..., 0, 0]
    if D == 2:
        return J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    if D == 3:
        return (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1])
                - J[..., 0, 1] * (J[..., 1, 0] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 0])
                + J[..., 0, 2] * (J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]))
    return torch.linalg.det(J)


def cofactor_closed(J):
    """d det(J) / dJ of (..., D, D) matrices: the cofactor matrix, det(J) J^-T (closed form for D <= 3)"""
    D = J.shape[-1]
    if D == 1:
        return torch.ones_like(J)
    if D <= 3:
        rows = []
        for d in range(D):
            r = [i for i in range(D) if i != d]
            row = []
            for e in range(D):
                c = [i for i in range(D) if i != e]
                minor = J[..., r[0], c[0]] if D == 2 else J[..., r[0], c[0]] * J[..., r[1], c[1]] - J[..., r[0], c[1]] * J[..., r[1], c[0]]
                row.append(minor if (d + e) % 2 == 0 else -minor)
            rows.append(torch.stack(row, -1))
        return torch.stack(rows, -2)
    return torch.linalg.det(J)[..., None, None] * torch.linalg.inv(J).transpose(-1, -2)


def _jacobian_work(table, disp, bound, order, add_identity):
    dim = disp.shape[-1]
    u = _work(disp)
    J = table.grad(u.movedim(-1, 1), _zero_disp(u), bound, order, 1, displacement=True).movedim(1, -2)
    if add_identity:
        J = J + torch.eye(dim, dtype=J.dtype, device=J.device)
    return J


def jacobian_composed(table, disp, bound, order, add_identity=True):
    """jacobian(disp) from the operators of a kernel table: disp (B,*shape,D) -> grid_grad of the field as a D-channel image at a
    zero displacement (the lattice points; extrapolate: they are in bounds), (B,*shape,D,D) with row = component, column =
    direction, plus the identity."""
    return _jacobian_work(table, disp, bound, order, add_identity).to(disp.dtype)


def jacdet_composed(table, disp, bound, order):
    """det(jacobian(disp)), (B,*shape)"""
    return det_closed(_jacobian_work(table, disp, bound, order, True)).to(disp.dtype)


def jacobian_backward_composed(table, grad, bound, order):
    """grad (B,*shape,D,D) -> the gradient of jacobian(disp) with respect to disp, (B,*shape,D): the adjoint of grid_grad at the
    lattice points is grid_pushgrad along the same zero displacement"""
    g = _work(grad).movedim(-2, 1)                                       # (B, D, *shape, D)
    out = table.pushgrad(g, _zero_disp(g[:, 0]), list(g.shape[2:-1]), bound, order, 1, displacement=True)
    return out.movedim(1, -1).to(grad.dtype)


def jacdet_backward_composed(table, grad, disp, bound, order):
    """grad (B,*shape) -> the gradient of jacdet(disp) with respect to disp: grad * cofactor(J) pushed back like a Jacobian gradient"""
    J = _jacobian_work(table, disp, bound, order, True)
    G = _work(grad)[..., None, None] * cofactor_closed(J)
    return jacobian_backward_composed(table, G, bound, order).to(disp.dtype)


SLIDING = 7                                                              # the regulariser's per-component bound (below)


def _extended(f, axis, t, bound, comp=None):
    """f~[o + t] along tensor dim `axis`: sign * index_select through the bound tables, for every tap (t = 0 included: dst1 has
    the sign 0 at index 0).  bound SLIDING (the regulariser only): the component of this axis, `axis - 1`, is extended by
    dst2 and every other one by dct2 (one index map; the sign differs).  comp: None -- f holds every component in its last
    dim; else the number of the one component that f is."""
    n = f.shape[axis]
    i = torch.arange(n, device=f.device) + t
    own = None
    if bound == SLIDING:
        if comp is None:
            bound, own = 3, bound_sign(5, i, n)
        else:
            bound = 5 if comp == axis - 1 else 3
    sign = bound_sign(bound, i, n)
    if t == 0 and sign is None:
        return f
    g = f.index_select(axis, bound_index(bound, i, n))
    shape = [1] * f.dim()
    shape[axis] = n
    if sign is not None:
        g = g * sign.to(f.dtype).reshape(shape)
    if own is not None:
        factor = torch.ones([n, f.shape[-1]], dtype=f.dtype, device=f.device)
        factor[:, axis - 1] = own.to(f.dtype)
        g = g * factor.reshape(shape[:-1] + [f.shape[-1]])
    return g


def _stencil_1d(f, axis, bound, taps, scale, comp=None):
    """sum_t taps[t] f~[o + t] along `axis`, times `scale`; taps: {offset: coefficient}"""
    out = None
    for t, c in taps.items():
        term = c * _extended(f, axis, t, bound, comp)
        out = term if out is None else out + term
    return out * scale


_TAPS_A = {0: 2.0, -1: -1.0, 1: -1.0}
_TAPS_B = {0: 6.0, -1: -4.0, 1: -4.0, -2: 1.0, 2: 1.0}
_TAPS_C = {-1: -0.5, 1: 0.5}


def regulariser_weights(weights):
    """(absolute, membrane, bending) or (absolute, membrane, bending, shears, div) -> the five, as floats"""
    w = tuple(float(x) for x in weights)
    if len(w) not in (3, 5):
        raise ValueError('regulariser: three weights (absolute, membrane, bending) or five (..., shears, div), got %d' % len(w))
    return w + (0.0, 0.0) if len(w) == 3 else w


def _regulariser_work(field, weights, voxel_size, bound):
    """L v in the work dtype: field (B,*shape,D); weights = (absolute, membrane, bending[, shears, div]); voxel_size, bound: D
    entries (bound: the codes 0..6 and SLIDING)"""
    dim = field.shape[-1]
    absolute, membrane, bending, shears, div = regulariser_weights(weights)
    v = _work(field)
    a = [1.0 / (float(h) * float(h)) for h in voxel_size]
    out = absolute * v if absolute else torch.zeros_like(v)
    elastic = shears + div
    if elastic:
        membrane = membrane + shears                                     # shears acts like a membrane, plus the coupling
    if membrane or bending:
        Av = [_stencil_1d(v, 1 + e, bound[e], _TAPS_A, a[e]) for e in range(dim)]
    if membrane:
        for e in range(dim):
            out = out + membrane * Av[e]
    if elastic:
        # the own-axis extra: (shears + div) A_c v_c
        out = out + elastic * torch.stack([Av[c][..., c] for c in range(dim)], -1)
    if bending:
        for e in range(dim):
            out = out + bending * _stencil_1d(v, 1 + e, bound[e], _TAPS_B, a[e] * a[e])
            for f in range(e + 1, dim):
                # A_e A_f on different axes: the tensor product of the two 1-D stencils on the extended field
                out = out + (2 * bending) * _stencil_1d(Av[f], 1 + e, bound[e], _TAPS_A, a[e])
    h2 = torch.tensor([float(h) * float(h) for h in voxel_size], dtype=v.dtype, device=v.device)
    out = out * h2
    if elastic and dim > 1:
        # X_ce v_e = C_c C_e v_e, the central differences (f~[o + 1] - f~[o - 1]) / 2 on component e extended by ITS bounds
        # (no voxel size: h_c h_e cancels)
        Ce = [_stencil_1d(v[..., e], 1 + e, bound[e], _TAPS_C, 1.0, comp=e) for e in range(dim)]
        cross = []
        for c in range(dim):
            x = None
            for e in range(dim):
                if e != c:
                    term = _stencil_1d(Ce[e], 1 + c, bound[c], _TAPS_C, 1.0, comp=e)
                    x = term if x is None else x + term
            cross.append(x)
        out = out - elastic * torch.stack(cross, -1)
    return out


def regulariser_composed(field, weights, voxel_size, bound):
    """The regulariser's matrix-vector product L v (include/interpol_hip.h: interpol_regulariser) as a sum over taps of
    coefficient * sign * index_select through bound_index / bound_sign: field (B,*shape,D) -> (B,*shape,D).  Any device, any D,
    any floating dtype (16-bit fields compute in float32 and round once), differentiable by autograd for every bound."""
    return _regulariser_work(field, weights, voxel_size, bound).to(field.dtype)


def regulariser_energy_composed(field, weights, voxel_size, bound):
    """0.5 <v, L v> per batch item, (B)"""
    v = _work(field)
    Lv = _regulariser_work(field, weights, voxel_size, bound)
    return (0.5 * (v * Lv).reshape(v.shape[0], -1).sum(1)).to(field.dtype)


def regulariser_solve_centre(weights, voxel_size):
    """c_d = h_d^2 [ absolute + membrane sum_e 2 / h_e^2 + bending ( sum_e 6 / h_e^4 + sum_{e != f} 4 / (h_e^2 h_f^2) ) ]: the
    interior diagonal of L, one float per dimension (unit voxels, 3-D, bending = 1: 42).  Three weights or five: shears and div
    add h_d^2 [ shears sum_e 2 / h_e^2 + (shears + div) 2 / h_d^2 ] (the cross-component taps have none at the centre)."""
    absolute, membrane, bending, shears, div = regulariser_weights(weights)
    a = [1.0 / (float(h) * float(h)) for h in voxel_size]
    mixed = sum(4 * a[e] * a[f] for e in range(len(a)) for f in range(len(a)) if e != f)
    centre = absolute + membrane * sum(2 * x for x in a) + bending * (sum(6 * x * x for x in a) + mixed)
    if not (shears or div):
        return [float(h) * float(h) * centre for h in voxel_size]
    centre = centre + shears * sum(2 * x for x in a)
    return [float(h) * float(h) * (centre + (shears + div) * 2 * x) for h, x in zip(voxel_size, a)]


def symmetric_matrix(h, dim):
    """(..., D (D + 1) / 2) -> (..., D, D): the diagonal first, then the upper triangle row by row"""
    idx = [[0] * dim for _ in range(dim)]
    k = dim
    for i in range(dim):
        idx[i][i] = i
        for j in range(i + 1, dim):
            idx[i][j] = idx[j][i] = k
            k += 1
    return h[..., torch.tensor(idx, device=h.device)]


def _point_operators(c, hessian, dim):
    """(precond, hess) of one level: r -> (H_o + diag(c))^-1 r in closed form and p -> H_o p (None without a Hessian); hessian
    None or (B|1,*shape,K) in the work dtype, c (D)"""
    K = 0 if hessian is None else hessian.shape[-1]
    if K == 0:
        return (lambda r: r / c), None
    if K == dim:
        Hd = hessian
        Md = Hd + c
        return (lambda r: r / Md), (lambda p: Hd * p)
    Hm = symmetric_matrix(hessian, dim)
    M = Hm + torch.diag(c)
    # (symmetric: the cofactor matrix is the adjugate; inv_ex does not synchronise)
    Minv = cofactor_closed(M) / det_closed(M)[..., None, None] if dim <= 3 else torch.linalg.inv_ex(M).inverse
    # (one D x D product per lattice point, written element-wise: as an einsum it becomes a batched GEMM with one tiny
    #  matrix per point -- a hundred times slower at 256^3, and tens of millions of batch items)
    return (lambda r: (Minv * r[..., None, :]).sum(-1)), (lambda p: (Hm * p[..., None, :]).sum(-1))


def _check_hessian_components(hessian, dim):
    K = 0 if hessian is None else hessian.shape[-1]
    if K not in (0, dim, dim * (dim + 1) // 2):
        raise ValueError('regulariser_solve: the Hessian has %d or %d components per point, got %d' % (dim, dim * (dim + 1) // 2, K))


def _conjugate_gradients(gradient, g, apply, precond, max_iter, tolerance):
    """the loop of `regulariser_solve_composed`: apply p -> (H + L) p, precond r -> z, both on (B,*shape,D) in the work dtype"""
    dim = gradient.shape[-1]
    B = g.shape[0]

    def dot(a, b):
        return (a.double() * b.double()).reshape(B, -1).sum(1)

    def col(s):
        return s.reshape([B] + [1] * (dim + 1))

    x = torch.zeros_like(g)
    r = g.clone()
    z = precond(r)
    p = z.clone()
    rho, gamma = dot(r, z), dot(g, g)
    done = gamma == 0
    iterations = torch.zeros(B, dtype=torch.int64, device=g.device)
    sigma = torch.zeros_like(gamma)
    tol2 = float(tolerance) * float(tolerance)
    for _ in range(int(max_iter)):
        q = apply(p)
        pi = dot(p, q)
        done = done | (pi <= 0) | (rho <= 0)
        act = ~done
        alpha = col((rho / pi).to(g.dtype))
        x = torch.where(col(act), x + alpha * p, x)
        r = torch.where(col(act), r - alpha * q, r)
        z = torch.where(col(act), precond(r), z)
        rho1, sig = dot(r, z), dot(r, r)
        sigma = torch.where(act, sig, sigma)
        iterations = iterations + act
        done = done | (act & (sig <= tol2 * gamma))
        act = ~done
        beta = col((rho1 / rho).to(g.dtype))
        p = torch.where(col(act), z + beta * p, p)
        rho = torch.where(act, rho1, rho)
    residual = torch.where((iterations > 0) & (gamma > 0), (sigma / gamma).sqrt(), torch.zeros_like(gamma))
    return x.to(gradient.dtype), iterations, residual


def regulariser_solve_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance):
    """x = (H + L)^-1 gradient by the preconditioned conjugate gradients of include/interpol_hip.h (interpol_regulariser_solve),
    written with `ops.regulariser` for L p (the fused L v on the GPU), element-wise passes and double inner products:
    gradient (B,*shape,D), hessian None or (B|1,*shape,K), K = D or D (D + 1) / 2 -> (x, iterations (B) int64, residual (B)
    float64).  Each item runs on its own; a done item is held by torch.where masks, so nothing synchronises and the loop
    always runs `max_iter` times.  Any device, any D, any floating dtype (16-bit fields compute in float32 and round once)."""
    from . import ops
    dim = gradient.shape[-1]
    g = _work(gradient)
    _check_hessian_components(hessian, dim)
    c = torch.tensor(regulariser_solve_centre(weights, voxel_size), dtype=g.dtype, device=g.device)
    precond, hess = _point_operators(c, None if hessian is None else _work(hessian), dim)

    def apply(p):
        q = ops.regulariser(p, weights, voxel_size, bound)
        return q if hess is None else q + hess(p)

    return _conjugate_gradients(gradient, g, apply, precond, max_iter, tolerance)


MULTIGRID_OMEGA = 0.5                                                    # the damping of the smoother (why 1/2 is safe)
MULTIGRID_COARSEST_SWEEPS = 8


def multigrid_halved(shape):
    """which dimensions the next level halves: n even and n / 2 >= 4"""
    return [n % 2 == 0 and n // 2 >= 4 for n in shape]


def _coarsen_hessian(h, halved):
    """(B|1,*shape,K) -> the next level: the sum over the children, entry (c, e) times s_c s_e (the packed layout: the diagonal
    first, then the upper triangle row by row)"""
    dim = len(halved)
    for d, yes in enumerate(halved):
        if yes:
            shp = list(h.shape)
            h = h.reshape(shp[:1 + d] + [shp[1 + d] // 2, 2] + shp[2 + d:]).sum(2 + d)
    s = [2.0 if yes else 1.0 for yes in halved]
    scale = [s[d] * s[d] for d in range(dim)]
    if h.shape[-1] > dim:
        scale += [s[d] * s[e] for d in range(dim) for e in range(d + 1, dim)]
    return h * torch.tensor(scale, dtype=h.dtype, device=h.device)


def _prolong(e, halved, bound):
    """P e: cell-centred linear interpolation along every halved dimension, coarse indices out of range extended by the bound of
    the dimension for each component; component c times s_c"""
    for d, yes in enumerate(halved):
        if not yes:
            continue
        axis = 1 + d
        even = 0.75 * e + 0.25 * _extended(e, axis, -1, bound[d])
        odd = 0.75 * e + 0.25 * _extended(e, axis, 1, bound[d])
        shp = list(e.shape)
        shp[axis] *= 2
        e = torch.stack([even, odd], axis + 1).reshape(shp)
    return e * torch.tensor([2.0 if yes else 1.0 for yes in halved], dtype=e.dtype, device=e.device)


def _restrict(f, halved, bound):
    """P^T f as a gather: coarse j = 1/4 f~[2j - 1] + 3/4 f[2j] + 3/4 f[2j + 1] + 1/4 f~[2j + 2]; component c times s_c"""
    for d, yes in enumerate(halved):
        if not yes:
            continue
        axis = 1 + d
        n = f.shape[axis]
        below = _extended(f, axis, -1, bound[d]).index_select(axis, torch.arange(0, n, 2, device=f.device))
        above = _extended(f, axis, 1, bound[d]).index_select(axis, torch.arange(1, n, 2, device=f.device))
        lo = f.index_select(axis, torch.arange(0, n, 2, device=f.device))
        hi = f.index_select(axis, torch.arange(1, n, 2, device=f.device))
        f = 0.25 * below + 0.75 * lo + 0.75 * hi + 0.25 * above
    return f * torch.tensor([2.0 if yes else 1.0 for yes in halved], dtype=f.dtype, device=f.device)


def multigrid_levels(shape, hessian, weights, voxel_size, bound, dtype, device):
    """The levels of the V-cycle of include/interpol_hip.h (interpol_regulariser_multigrid_solve), built once per call: a list of
    dicts with `apply` (v -> A_l v), `precond` (r -> M_l^-1 r) and `halved` (None on the last level).  hessian: None or
    (B|1,*shape,K) in the work dtype."""
    from . import ops
    dim = len(shape)
    shape, h, kappa = list(shape), [float(v) for v in voxel_size], 1.0
    weights = regulariser_weights(weights)
    levels = []
    while True:
        w = tuple(kappa * x for x in weights)
        c = torch.tensor(regulariser_solve_centre(w, h), dtype=dtype, device=device)
        precond, hess = _point_operators(c, hessian, dim)

        def apply(v, w=w, h=list(h), hess=hess):
            q = ops.regulariser(v, w, h, bound)
            return q if hess is None else q + hess(v)

        halved = multigrid_halved(shape)
        levels.append(dict(apply=apply, precond=precond, halved=halved if any(halved) else None))
        if not any(halved):
            return levels
        if hessian is not None:
            hessian = _coarsen_hessian(hessian, halved)
        for d in range(dim):
            if halved[d]:
                shape[d] //= 2
                h[d] *= 2
                kappa *= 2


def multigrid_vcycle(levels, r, bound, smoothing, level=0):
    """z = V(r): r (B,*shape of the level,D) in the work dtype"""
    lv = levels[level]
    last = lv['halved'] is None
    nu = MULTIGRID_COARSEST_SWEEPS if last else int(smoothing)
    x = MULTIGRID_OMEGA * lv['precond'](r)
    for _ in range(nu - 1):
        x = x + MULTIGRID_OMEGA * lv['precond'](r - lv['apply'](x))
    if last:
        return x
    d = r - lv['apply'](x)
    x = x + _prolong(multigrid_vcycle(levels, _restrict(d, lv['halved'], bound), bound, smoothing, level + 1), lv['halved'], bound)
    for _ in range(nu):
        x = x + MULTIGRID_OMEGA * lv['precond'](r - lv['apply'](x))
    return x


def regulariser_vcycle_composed(residual, hessian, weights, voxel_size, bound, smoothing):
    """z = V(residual), one V-cycle of `regulariser_multigrid_composed`, (B,*shape,D)"""
    dim = residual.shape[-1]
    r = _work(residual)
    _check_hessian_components(hessian, dim)
    levels = multigrid_levels(r.shape[1:-1], None if hessian is None else _work(hessian), weights, voxel_size, bound, r.dtype, r.device)
    return multigrid_vcycle(levels, r, bound, smoothing).to(residual.dtype)


def regulariser_multigrid_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing):
    """`regulariser_solve_composed` with one multigrid V-cycle z = V(r) in the place of z = M^-1 r (include/interpol_hip.h:
    interpol_regulariser_multigrid_solve): the levels are built once, every level operator is `ops.regulariser` with the
    weights times kappa_l and the voxel sizes of the level, the grid transfers are index_select passes through the bound
    tables.  The cycle also runs for items that are done; the torch.where masks hold their x.  Any device, any D, any floating
    dtype (16-bit fields compute in float32 and round once)."""
    dim = gradient.shape[-1]
    g = _work(gradient)
    _check_hessian_components(hessian, dim)
    levels = multigrid_levels(g.shape[1:-1], None if hessian is None else _work(hessian), weights, voxel_size, bound, g.dtype, g.device)
    return _conjugate_gradients(gradient, g, levels[0]['apply'], lambda r: multigrid_vcycle(levels, r, bound, smoothing),
                                max_iter, tolerance)


def ssd_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian):
    """Loss, gradient and Gauss-Newton Hessian of 0.5 sum weight (moving(id + disp) - fixed)^2 with respect to `disp`, written
    with `ops.grid_pull` / `ops.grid_grad` at a displacement and element-wise passes -- the definition that csrc/ssd.hip fuses:

        w = pull(moving, disp),  G = grad(moving, disp),  r = w - fixed
        loss (B) = 0.5 sum_o sum_c weight r^2,   gradient (B,*shape,D) = sum_c (weight r_c) G_cd,
        hessian (B,*shape,K) = weight sum_c G_cd G_ce

    moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape); hessian: None, 'diagonal'
    (K = D) or 'full' (K = D (D + 1) / 2: the diagonal first, then the upper triangle row by row).  -> (loss, gradient, hessian |
    None).  Nothing synchronises.  Any device, any D, any per-dimension orders, any floating dtype (16-bit storage computes in
    float32 and is rounded once); the loss is summed in double."""
    from . import ops
    dim = disp.shape[-1]
    out_dtype = disp.dtype
    m, f, u = _work(moving), _work(fixed), _work(disp)
    w = ops.grid_pull(m, u, bound, order, extrapolate, displacement=True)                # (B,C,*shape)
    G = ops.grid_grad(m, u, bound, order, extrapolate, displacement=True)                # (B,C,*shape,D)
    r = w - f
    wr = r if weight is None else r * _work(weight).unsqueeze(1)
    B = wr.shape[0]                                                                      # the broadcast batch of all four operands
    loss = 0.5 * (wr * r).reshape(B, -1).sum(1, dtype=torch.float64)
    gradient = (G * wr.unsqueeze(-1)).sum(1)
    hess = None
    if hessian is not None:
        pairs = [(d, d) for d in range(dim)]
        if hessian == 'full':
            pairs += [(d, e) for d in range(dim) for e in range(d + 1, dim)]
        hess = torch.stack([(G[..., d] * G[..., e]).sum(1) for d, e in pairs], -1)
        if weight is not None:
            hess = hess * _work(weight).unsqueeze(-1)
        hess = hess.to(out_dtype)
        if hess.shape[0] != B:                                                           # (moving, disp and weight without a batch)
            hess = hess.expand(B, *hess.shape[1:])
    return loss.to(out_dtype), gradient.to(out_dtype), hess


def window_sum(x, window, dim):
    """The zero-padded window sum of `x` over its last `dim` dims: S(o) = sum of x(p) over |p_d - o_d| <= (window_d - 1) / 2, clipped at
    the edges (not wrapped).  Separable, in a fixed order: the dims from the first to the last; along a dim the window_d shifted,
    zero-padded slices are added from the lowest shift (-r) to the highest (+r).  In the dtype of `x`."""
    for d in range(dim):
        r = (int(window[d]) - 1) // 2
        if r == 0:
            continue
        axis = x.dim() - dim + d
        n = x.shape[axis]
        padded = torch.nn.functional.pad(x, [0, 0] * (dim - 1 - d) + [r, r])
        acc = padded.narrow(axis, 0, n)
        for t in range(1, 2 * r + 1):
            acc = acc + padded.narrow(axis, t, n)
        x = acc
    return x


def lcc_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps):
    """Loss, gradient and the positive part of the Hessian of the local normalised cross-correlation with respect to `disp`, written
    with `ops.grid_pull` / `ops.grid_grad` at a displacement, `window_sum` and element-wise passes -- the definition that csrc/lcc.hip
    fuses.  Per channel, with I = pull(moving, disp), G = grad(moving, disp), J = fixed, box = window_sum, n = box(1):

        S_X = box(X) for X in I, J, I^2, J^2, IJ
        cross = S_IJ - S_I S_J / n,  vI = max(S_II - S_I^2 / n, 0),  vJ = max(S_JJ - S_J^2 / n, 0),  den = vI vJ + eps,  cc = cross^2 / den
        a = weight 2 cross / den,  c = weight 2 cross^2 vJ / den^2,  f = (a S_J - c S_I) / n,   A, C, F = box(a), box(c), box(f)
        dI = -J A + I C + F
        loss (B) = -sum_o weight sum_c cc,   gradient (B,*shape,D) = sum_c dI_c G_cd,   hessian (B,*shape,K) = sum_c C_c G_cd G_ce

    Precision: I, J and G in the working dtype; the five window sums and everything down to a, c, f (the loss included) in float64
    from that I and J; a, c, f stay float64; A, C, F are summed in float64; dI is rounded once.
    moving (B|1,C,*inshape), fixed (B|1,C,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape); hessian: None, 'diagonal'
    (K = D) or 'full' (K = D (D + 1) / 2: the diagonal first, then the upper triangle row by row); window: D odd ints.  -> (loss,
    gradient, hessian | None).  Nothing synchronises.  Any device, any D, any per-dimension orders, any window, any floating dtype
    (16-bit storage computes in float32 and is rounded once)."""
    from . import ops
    dim = disp.shape[-1]
    out_dtype = disp.dtype
    m, f, u = _work(moving), _work(fixed), _work(disp)
    R = u.dtype
    I = ops.grid_pull(m, u, bound, order, extrapolate, displacement=True)                # (B,C,*shape)
    G = ops.grid_grad(m, u, bound, order, extrapolate, displacement=True)                # (B,C,*shape,D)
    box = lambda x: window_sum(x, window, dim)
    Id, Jd = I.double(), f.double()
    n = box(torch.ones(list(f.shape[2:]), dtype=torch.float64, device=f.device))
    SI, SJ, SII, SJJ, SIJ = box(Id), box(Jd), box(Id * Id), box(Jd * Jd), box(Id * Jd)
    cross = SIJ - SI * SJ / n
    vI = (SII - SI * SI / n).clamp_min(0)
    vJ = (SJJ - SJ * SJ / n).clamp_min(0)
    den = vI * vJ + eps
    wt = 1.0 if weight is None else _work(weight).double().unsqueeze(1)
    cc = wt * (cross * cross / den)
    a = wt * 2 * cross / den
    c = wt * 2 * cross * cross * vJ / (den * den)
    ff = (a * SJ - c * SI) / n
    B = cc.shape[0]                                                                      # the broadcast batch of all four operands
    loss = -cc.reshape(B, -1).sum(1)
    A, C, F = box(a), box(c), box(ff)
    dI = (-Jd * A + Id * C + F).to(R)
    gradient = (G * dI.unsqueeze(-1)).sum(1)
    hess = None
    if hessian is not None:
        pairs = [(d, d) for d in range(dim)]
        if hessian == 'full':
            pairs += [(d, e) for d in range(dim) for e in range(d + 1, dim)]
        Cr = C.to(R)
        hess = torch.stack([(Cr * G[..., d] * G[..., e]).sum(1) for d, e in pairs], -1).to(out_dtype)
    return loss.to(out_dtype), gradient.to(out_dtype), hess


def ssd_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian=True):
    """Loss, gradient and Gauss-Newton Hessian of 0.5 sum weight (moving(A o + t) - fixed)^2 with respect to the D (D+1) entries of
    the matrix [A | t] of every batch item, written with operators that exist without csrc/ssd_affine.hip -- its definition:

        lattice_b = AffineGrid(mat_b, shape).dense()                        (the kernels' operation order, unfused)
        loss, g, H = ops.ssd_gauss_newton(moving, fixed, lattice - identity, weight, hessian='full')
        gradient[b, d, e]                      = sum_o g[b, o, d] o~_e,                    o~ = (o_0 .. o_{D-1}, 1)
        hessian[b, d (D+1) + e, d' (D+1) + e'] = sum_o H[b, o, (d, d')] o~_e o~_e'

    The two contractions run in float64 and are rounded once; both triangles of the Hessian come from the same sum.
    moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape) -> (loss (B), gradient (B,D,D+1),
    hessian (B,P,P) | None), P = D (D+1).  Nothing synchronises.  Any device, any D, any per-dimension orders, any floating dtype
    (16-bit storage computes in float32 and is rounded once)."""
    from . import ops
    out_dtype = mat.dtype
    m, f, a = _work(moving), _work(fixed), _work(mat)
    w = None if weight is None else _work(weight)
    o, disp = _affine_displacement(a, list(f.shape[2:]))
    loss, g, H = ops.ssd_gauss_newton(m, f, disp, w, bound, order, extrapolate, 'full' if hessian else None)
    gradient, hess = _affine_contract(g, H, o, out_dtype)
    return loss.to(out_dtype), gradient, hess


def _affine_displacement(a, shape):
    """a (B|1,D,D+1) in the working dtype -> (o (*shape,D) the sample indices, disp (B|1,*shape,D) = AffineGrid(a_b, shape).dense() - o),
    the kernels' operation order, unfused."""
    dim = a.shape[-1] - 1
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=a.dtype, device=a.device) for n in shape], indexing='ij'), -1)
    av = a.reshape([a.shape[0]] + [1] * dim + [dim, dim + 1])
    cols = []
    for d in range(dim):                                             # AffineGrid.dense(), one matrix per item
        s = av[..., d, 0] * o[..., 0]
        for e in range(1, dim):
            s = s + av[..., d, e] * o[..., e]
        cols.append(s + av[..., d, dim])
    return o, torch.stack(cols, -1) - o


def _affine_contract(g, H, o, out_dtype):
    """The two float64 contractions of the affine data terms: g (B,*shape,D) and H None or (B,*shape,K) in the layout of
    hessian='full', o (*shape,D) -> (gradient (B,D,D+1), hessian (B,P,P) | None) in `out_dtype`, rounded once."""
    dim = o.shape[-1]
    B = g.shape[0]
    ot = torch.cat([o, torch.ones_like(o[..., :1])], -1).reshape(-1, dim + 1).double()                  # (N, D+1)
    gradient = torch.matmul(g.reshape(B, -1, dim).double().transpose(1, 2), ot)                         # (B, D, D+1)
    hess = None
    if H is not None:
        # the distinct moments o~_e o~_e', e <= e', and the distinct components of H: one sum per distinct entry
        epairs = [(e, e2) for e in range(dim + 1) for e2 in range(e, dim + 1)]
        mo = torch.stack([ot[:, e] * ot[:, e2] for e, e2 in epairs], -1)                                # (N, M)
        K = H.shape[-1]
        S = torch.matmul(H.reshape(B, -1, K).double().transpose(1, 2), mo)                              # (B, K, M)
        kof = {}
        for d in range(dim):                                         # hessian='full': the diagonal first, then the upper triangle
            kof[(d, d)] = d
        k = dim
        for d in range(dim):
            for d2 in range(d + 1, dim):
                kof[(d, d2)] = k
                k += 1
        mof = {p: i for i, p in enumerate(epairs)}
        kidx = [kof[(min(d, d2), max(d, d2))] for d in range(dim) for e in range(dim + 1) for d2 in range(dim) for e2 in range(dim + 1)]
        midx = [mof[(min(e, e2), max(e, e2))] for d in range(dim) for e in range(dim + 1) for d2 in range(dim) for e2 in range(dim + 1)]
        P = dim * (dim + 1)
        hess = S[:, torch.as_tensor(kidx, device=S.device), torch.as_tensor(midx, device=S.device)].reshape(B, P, P).to(out_dtype)
    return gradient.to(out_dtype), hess


def lcc_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian=True, window=None, eps=1e-5):
    """Loss, gradient and the positive part of the Hessian of the local normalised cross-correlation between moving(A o + t) and
    fixed with respect to the D (D+1) entries of the matrix [A | t] of every batch item, written with operators that exist without
    csrc/lcc_affine.hip -- its definition:

        lattice_b = AffineGrid(mat_b, shape).dense()                        (the kernels' operation order, unfused)
        loss, g, H = ops.lcc_gauss_newton(moving, fixed, lattice - identity, weight, hessian='full', window, eps)
        gradient[b, d, e]                      = sum_o g[b, o, d] o~_e,                    o~ = (o_0 .. o_{D-1}, 1)
        hessian[b, d (D+1) + e, d' (D+1) + e'] = sum_o H[b, o, (d, d')] o~_e o~_e'

    The two contractions are those of `ssd_gauss_newton_affine_composed`: float64, rounded once, both triangles from the same sum.
    moving (B|1,C,*inshape), fixed (B|1,C,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape); window: D odd ints (None: 9 in
    every dim) -> (loss (B), gradient (B,D,D+1), hessian (B,P,P) | None), P = D (D+1).  Nothing synchronises.  Any device, any D, any
    per-dimension orders, any window, any floating dtype (16-bit storage computes in float32 and is rounded once)."""
    from . import ops
    dim = mat.shape[-1] - 1
    out_dtype = mat.dtype
    m, f, a = _work(moving), _work(fixed), _work(mat)
    w = None if weight is None else _work(weight)
    o, disp = _affine_displacement(a, list(f.shape[2:]))
    window = [9] * dim if window is None else list(window)
    loss, g, H = ops.lcc_gauss_newton(m, f, disp, w, bound, order, extrapolate, 'full' if hessian else None, window, eps)
    gradient, hess = _affine_contract(g, H, o, out_dtype)
    return loss.to(out_dtype), gradient, hess


def mi_ranges(moving, fixed, weight, moving_range, fixed_range, B):
    """The five doubles per batch item that the mutual-information data term bins with, (B, 5) float64 on the device of `moving`:
    (m_lo, m_sc, f_lo, f_sc, wmax), m_sc = 1 / (m_hi - m_lo) or 0 for a degenerate range (hi <= lo), f_sc likewise, wmax = max
    |weight| (1 without a weight).  A range is a pair of floats or None = `torch.aminmax` of the tensor per batch item.  Nothing
    synchronises.  moving (B|1,1,*inshape), fixed (B|1,1,*shape), weight None or (B|1,*shape)."""
    dev = moving.device

    def lo_sc(t, rng):
        if rng is None:
            lo, hi = torch.aminmax(_work(t).reshape(t.shape[0], -1), dim=1)
            lo, hi = lo.double(), hi.double()
        else:
            lo = torch.full([1], float(rng[0]), dtype=torch.float64, device=dev)
            hi = torch.full([1], float(rng[1]), dtype=torch.float64, device=dev)
        ok = hi > lo
        sc = torch.where(ok, 1.0 / torch.where(ok, hi - lo, torch.ones_like(lo)), torch.zeros_like(lo))
        return lo.expand(B), sc.expand(B)

    m_lo, m_sc = lo_sc(moving, moving_range)
    f_lo, f_sc = lo_sc(fixed, fixed_range)
    if weight is None:
        wmax = torch.ones([B], dtype=torch.float64, device=dev)
    else:
        wmax = _work(weight).reshape(weight.shape[0], -1).abs().amax(1).double().expand(B)
    return torch.stack([m_lo, m_sc, f_lo, f_sc, wmax], -1).contiguous()


def mi_bins(I, J, ranges, bins):
    """What the mutual-information data term bins a sample into, in the dtype of `I`: I (B,*shape) the pulled image, J (B|1,*shape)
    the fixed one, ranges (B,5) of `mi_ranges` -> (j0 (B,*shape) int64 the first of the four taps on the moving side, f = u -
    floor(u), clamped (bool: t_m left [0, 1]), k (B,*shape) int64 the bin on the fixed side)."""
    R = I.dtype
    r = ranges.to(R).reshape([ranges.shape[0]] + [1] * (I.dim() - 1) + [5])
    raw = (I - r[..., 0]) * r[..., 1]
    clamped = ~((raw >= 0) & (raw <= 1))
    tm = torch.nan_to_num(raw.clamp(0, 1), nan=0.0)
    u = 1.5 + tm * (bins - 4)
    fl = u.floor().clamp(1, bins - 3)
    f = u - fl
    j0 = fl.long() - 1
    tf = torch.nan_to_num(((J - r[..., 2]) * r[..., 3]).clamp(0, 1), nan=0.0)
    k = (tf * (bins - 1) + 0.5).floor().long().clamp(0, bins - 1)
    return j0, f, clamped, k.expand(j0.shape)


def bspline3_taps(f, which=0):
    """The cubic B-spline at the four taps floor(u) - 1 .. floor(u) + 2 for f = u - floor(u) in [0, 1), stacked last: which = 0 the
    weights (they sum to 1), 1 the derivative with respect to u (they sum to 0), 2 the absolute second derivative."""
    g = 1 - f
    if which == 0:
        w = [g * g * g / 6, 2.0 / 3.0 - f * f + 0.5 * f * f * f, 2.0 / 3.0 - g * g + 0.5 * g * g * g, f * f * f / 6]
    elif which == 1:
        w = [-0.5 * g * g, -2 * f + 1.5 * f * f, 2 * g - 1.5 * g * g, 0.5 * f * f]
    else:
        w = [g, (3 * f - 2).abs(), (1 - 3 * f).abs(), f]
    return torch.stack(w, -1)


def mi_sample_terms(I, J, omega, ranges, bins, need_c=True):
    """The middle of the mutual-information data terms, whatever the lattice: I (B,*shape) the pulled image, J (B|1,*shape) the fixed
    one, omega (B,*shape) = weight mask, all in the working dtype, ranges (B,5) of `mi_ranges` -> (loss (B) float64, dI (B,*shape),
    c (B,*shape) | None, P (B,bins,bins) float64): the histogram by `index_add_` into float64, T in float64 rounded once to the
    working dtype, the per-sample terms dI and c in the working dtype (`mi_gauss_newton_affine_composed` states the formulas)."""
    R = I.dtype
    B = ranges.shape[0]
    dim = I.dim() - 1
    bshape = list(I.shape)
    dev = I.device
    j0, fr, clamped, k = mi_bins(I, J, ranges, bins)
    # the histogram in float64
    beta = bspline3_taps(fr, 0)                                                          # (B,*shape,4)
    idx = ((j0.unsqueeze(-1) + torch.arange(4, device=dev)) * bins + k.unsqueeze(-1)).reshape(B, -1)
    idx = idx + (torch.arange(B, device=dev) * (bins * bins)).unsqueeze(-1)
    H = torch.zeros(B * bins * bins, dtype=torch.float64, device=dev)
    H.index_add_(0, idx.reshape(-1), (omega.unsqueeze(-1) * beta).double().reshape(-1))
    H = H.reshape(B, bins, bins)
    W = omega.reshape(B, -1).double().sum(1)
    live = W > 0
    inv_w = torch.where(live, 1.0 / torch.where(live, W, torch.ones_like(W)), torch.zeros_like(W))
    P = H * inv_w.reshape(B, 1, 1)
    pm, pf = P.sum(2, keepdim=True), P.sum(1, keepdim=True)
    pos = P > 0
    T = torch.where(pos, torch.log(torch.where(pos, P / torch.where(pos, pm * pf, torch.ones_like(P)), torch.ones_like(P))),
                    torch.zeros_like(P))
    loss = -(P * T).reshape(B, -1).sum(1)
    # the per-sample terms in the working dtype
    Tr = T.to(R).reshape(-1)
    Tt = Tr[idx.reshape(-1)].reshape(bshape + [4])
    sc = torch.where(clamped, torch.zeros_like(I), (bins - 4) * ranges[:, 1].to(R).reshape([B] + [1] * dim).expand(bshape))
    wn = omega * inv_w.to(R).reshape([B] + [1] * dim)
    dI = -(wn * sc) * (bspline3_taps(fr, 1) * Tt).sum(-1)
    c = (wn * sc) * sc * (bspline3_taps(fr, 2) * Tt.abs()).sum(-1) if need_c else None
    return loss, dI, c, P


def mi_gauss_newton_affine_composed(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian=True, bins=32,
                                    return_histogram=False):
    """Loss, gradient and a majoriser of the Hessian of minus the mutual information between moving(A o + t) and fixed with respect
    to the D (D+1) entries of the matrix [A | t] of every batch item, written with operators that exist without csrc/mi_affine.hip
    -- its definition (`api.mi_gauss_newton_affine` states the formulas):

        lattice_b = AffineGrid(mat_b, shape).dense();  I = ops.grid_pull(moving, lattice),  G = ops.grid_grad(moving, lattice)
        omega = weight mask;  (j0, f, clamped, k) = mi_bins(I, fixed, ranges, bins);  beta = bspline3_taps(f)
        H[j0 + i, k] += omega beta_i   by index_add_ into float64;   W = sum omega;   P = H / W
        T = log(P / (p_m p_f)) where P > 0 else 0 (float64), rounded once to the working dtype;   loss = - sum P T  (float64)
        dI = -(omega / W) s sum_i beta'_i T[j0 + i, k],   c = (omega / W) s^2 sum_i |beta''_i| |T[j0 + i, k]|   (working dtype)
        gradient[b, d, e] = sum_o dI G_d o~_e,   hessian = sum_o c G_d G_d' o~_e o~_e'   (contracted in float64, rounded once)

    moving (B|1,1,*inshape), fixed (B|1,1,*shape), mat (B|1,D,D+1), weight None or (B|1,*shape), ranges (B,5) float64
    (`mi_ranges`) -> (loss (B), gradient (B,D,D+1), hessian (B,P,P) | None, histogram (B,bins,bins) | None).  Nothing synchronises.
    Any device, any D, any per-dimension orders, any bins >= 8, any floating dtype (16-bit storage computes in float32 and is rounded
    once).  On the GPU `index_add_` adds with floating-point atomics: the histogram, and everything behind it, is NOT
    bit-reproducible from run to run there (the fused kernel is).  In float32 the taps' weights at the ends of the B-spline's support
    carry the rounding of I relatively (3 / e at a distance e inside the support); the fused kernel forms its histogram in double."""
    from . import ops
    dim = mat.shape[-1] - 1
    out_dtype = mat.dtype
    m, f, a = _work(moving), _work(fixed), _work(mat)
    R = a.dtype
    shape = list(f.shape[2:])
    B = ranges.shape[0]
    o = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=R, device=a.device) for n in shape], indexing='ij'), -1)
    av = a.reshape([a.shape[0]] + [1] * dim + [dim, dim + 1])
    cols = []
    for d in range(dim):                                             # AffineGrid.dense(), one matrix per item
        s = av[..., d, 0] * o[..., 0]
        for e in range(1, dim):
            s = s + av[..., d, e] * o[..., e]
        cols.append(s + av[..., d, dim])
    x = torch.stack(cols, -1)                                                            # (Ba,*shape,D)
    I = ops.grid_pull(m, x, bound, order, extrapolate)[:, 0]                             # (B',*shape): masked as grid_pull masks
    G = ops.grid_grad(m, x, bound, order, extrapolate)[:, 0]                             # (B',*shape,D)
    mask = _mask(x, m.shape[2:], extrapolate)
    omega = torch.ones([1] + shape, dtype=R, device=a.device) if weight is None else _work(weight)
    if mask is not None:
        omega = omega * mask.to(R)
    bshape = [B] + shape
    I, G, omega = I.expand(bshape), G.expand(bshape + [dim]), omega.expand(bshape)
    N = 1
    for n in shape:
        N *= n
    loss, dI, c, P = mi_sample_terms(I, f[:, 0], omega, ranges, bins, bool(hessian))
    g = (dI.unsqueeze(-1) * G).reshape(B, N, dim)
    ot = torch.cat([o, torch.ones_like(o[..., :1])], -1).reshape(-1, dim + 1).double()                  # (N, D+1)
    gradient = torch.matmul(g.double().transpose(1, 2), ot)                                             # (B, D, D+1)
    hess = None
    if hessian:
        dpairs = [(d, d2) for d in range(dim) for d2 in range(d, dim)]
        epairs = [(e, e2) for e in range(dim + 1) for e2 in range(e, dim + 1)]
        Hs = torch.stack([c * G[..., d] * G[..., d2] for d, d2 in dpairs], -1).reshape(B, N, len(dpairs))
        mo = torch.stack([ot[:, e] * ot[:, e2] for e, e2 in epairs], -1)                                # (N, M)
        S = torch.matmul(Hs.double().transpose(1, 2), mo)                                               # (B, K, M)
        kof = {p: i for i, p in enumerate(dpairs)}
        mof = {p: i for i, p in enumerate(epairs)}
        kidx = [kof[(min(d, d2), max(d, d2))] for d in range(dim) for e in range(dim + 1) for d2 in range(dim) for e2 in range(dim + 1)]
        midx = [mof[(min(e, e2), max(e, e2))] for d in range(dim) for e in range(dim + 1) for d2 in range(dim) for e2 in range(dim + 1)]
        Pn = dim * (dim + 1)
        hess = S[:, torch.as_tensor(kidx, device=S.device), torch.as_tensor(midx, device=S.device)].reshape(B, Pn, Pn).to(out_dtype)
    hist = P.to(out_dtype) if return_histogram else None
    return loss.to(out_dtype), gradient.to(out_dtype), hess, hist


def mi_gauss_newton_composed(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian='full', bins=32,
                             return_histogram=False):
    """Loss, gradient and a majoriser of the Hessian of minus the mutual information between moving(id + disp) and fixed with respect
    to `disp`, written with operators that exist without csrc/mi.hip -- its definition (`api.mi_gauss_newton` states the formulas):

        I = ops.grid_pull(moving, disp, displacement=True),  G = ops.grid_grad(moving, disp, displacement=True),  omega = weight mask
        loss, dI, c, P = mi_sample_terms(I, fixed, omega, ranges, bins)          (shared with `mi_gauss_newton_affine_composed`)
        gradient[b, o, d] = dI G_d,   hessian[b, o, k] = c G_d G_e   (working dtype; the diagonal first, then the upper triangle)

    moving (B|1,1,*inshape), fixed (B|1,1,*shape), disp (B|1,*shape,D), weight None or (B|1,*shape), ranges (B,5) float64
    (`mi_ranges`); hessian: None, 'diagonal' (K = D) or 'full' (K = D (D + 1) / 2) -> (loss (B), gradient (B,*shape,D), hessian
    (B,*shape,K) | None, histogram (B,bins,bins) | None).  Nothing synchronises.  Any device, any D, any per-dimension orders, any
    bins >= 8, any floating dtype (16-bit storage computes in float32 and is rounded once).  On the GPU `index_add_` adds with
    floating-point atomics: the histogram, and everything behind it, is NOT bit-reproducible from run to run there."""
    from . import ops
    from .utils import identity_grid
    dim = disp.shape[-1]
    out_dtype = disp.dtype
    m, f, u = _work(moving), _work(fixed), _work(disp)
    R = u.dtype
    shape = list(f.shape[2:])
    B = ranges.shape[0]
    I = ops.grid_pull(m, u, bound, order, extrapolate, displacement=True)[:, 0]          # (B',*shape): masked as grid_pull masks
    G = ops.grid_grad(m, u, bound, order, extrapolate, displacement=True)[:, 0]          # (B',*shape,D)
    mask = _mask(u + identity_grid(shape, dtype=R, device=u.device), m.shape[2:], extrapolate)
    omega = torch.ones([1] + shape, dtype=R, device=u.device) if weight is None else _work(weight)
    if mask is not None:
        omega = omega * mask.to(R)
    bshape = [B] + shape
    I, G, omega = I.expand(bshape), G.expand(bshape + [dim]), omega.expand(bshape)
    loss, dI, c, P = mi_sample_terms(I, f[:, 0], omega, ranges, bins, hessian is not None)
    gradient = dI.unsqueeze(-1) * G
    hess = None
    if hessian is not None:
        pairs = [(d, d) for d in range(dim)]
        if hessian == 'full':
            pairs += [(d, e) for d in range(dim) for e in range(d + 1, dim)]
        hess = torch.stack([c * G[..., d] * G[..., e] for d, e in pairs], -1).to(out_dtype)
    hist = P.to(out_dtype) if return_histogram else None
    return loss.to(out_dtype), gradient.to(out_dtype), hess, hist


class TorchKernels:
    """Same interface as `ops._HipKernels`; any device, any number of spatial dims."""

    # the mutual-information data term on a dense displacement field: the composed form only (the fused kernels exist on the GPU)
    @staticmethod
    def mi_gauss_newton(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram):
        return mi_gauss_newton_composed(moving, fixed, disp, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram)

    # the mutual-information data term on the matrix of an affine lattice: the composed form only (the fused kernels exist on the GPU)
    @staticmethod
    def mi_gauss_newton_affine(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian, bins, return_histogram):
        return mi_gauss_newton_affine_composed(moving, fixed, mat, weight, ranges, bound, order, extrapolate, hessian, bins,
                                               return_histogram)

    # the data term on the matrix of an affine lattice: the composed form only (the fused kernel exists on the GPU, D <= 3)
    @staticmethod
    def ssd_gauss_newton_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian):
        return ssd_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian)

    # the local cross-correlation data term on the matrix of an affine lattice: the composed form only (fused on the GPU, D <= 3)
    @staticmethod
    def lcc_gauss_newton_affine(moving, fixed, mat, weight, bound, order, extrapolate, hessian, window, eps):
        return lcc_gauss_newton_affine_composed(moving, fixed, mat, weight, bound, order, extrapolate, hessian, window, eps)

    # the local cross-correlation data term: the composed form only (the fused kernels exist on the GPU, D <= 3)
    @staticmethod
    def lcc_gauss_newton(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps):
        return lcc_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian, window, eps)

    # the sum-of-squares data term: the composed form only (the fused kernel exists on the GPU, D <= 3)
    @staticmethod
    def ssd_gauss_newton(moving, fixed, disp, weight, bound, order, extrapolate, hessian):
        return ssd_gauss_newton_composed(moving, fixed, disp, weight, bound, order, extrapolate, hessian)

    # the conjugate-gradient solve of (H + L) x = g: the composed form only (the fused kernels exist on the GPU, D <= 3)
    @staticmethod
    def regulariser_solve(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance):
        return regulariser_solve_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance)

    # ... with the multigrid preconditioner, and one V-cycle alone: the composed form only
    @staticmethod
    def regulariser_multigrid(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing):
        return regulariser_multigrid_composed(gradient, hessian, weights, voxel_size, bound, max_iter, tolerance, smoothing)

    @staticmethod
    def regulariser_vcycle(residual, hessian, weights, voxel_size, bound, smoothing):
        return regulariser_vcycle_composed(residual, hessian, weights, voxel_size, bound, smoothing)

    # the smoothness penalty of a displacement field: the composed form only (the fused kernels exist on the GPU, D <= 3)
    @staticmethod
    def regulariser(field, weights, voxel_size, bound):
        return regulariser_composed(field, weights, voxel_size, bound)

    @staticmethod
    def regulariser_energy(field, weights, voxel_size, bound):
        return regulariser_energy_composed(field, weights, voxel_size, bound)

    # Jacobian of id + displacement at the lattice points: the composed form only (the fused kernels exist on the GPU, D <= 3)
    @staticmethod
    def jacobian(disp, bound, order, add_identity=True):
        return jacobian_composed(TorchKernels, disp, bound, order, add_identity)

    @staticmethod
    def jacdet(disp, bound, order):
        return jacdet_composed(TorchKernels, disp, bound, order)

    @staticmethod
    def jacobian_backward(grad, bound, order):
        return jacobian_backward_composed(TorchKernels, grad, bound, order)

    @staticmethod
    def jacdet_backward(grad, disp, bound, order):
        return jacdet_backward_composed(TorchKernels, grad, disp, bound, order)

    # composition of displacement fields: the composed form only (the fused kernel exists on the GPU, D <= 3)
    @staticmethod
    def compose(left, right, bound, order, extrapolate, out=None):
        res = composed(TorchKernels, left, right, bound, order, extrapolate)
        return res if out is None else out.copy_(res)

    @staticmethod
    def compose_backward(grad, left, right, bound, order, extrapolate, need_left, need_right):
        return composed_backward(TorchKernels, grad, left, right, bound, order, extrapolate, need_left, need_right)

    @staticmethod
    def pull(inp, grid, bound, order, extrapolate, displacement=False):
        return _gather_op(inp, grid, bound, order, extrapolate, displacement, 0)

    @staticmethod
    def grad(inp, grid, bound, order, extrapolate, displacement=False):
        return _gather_op(inp, grid, bound, order, extrapolate, displacement, 1)

    @staticmethod
    def hess(inp, grid, bound, order, extrapolate, displacement=False):
        return _gather_op(inp, grid, bound, order, extrapolate, displacement, 2)

    @staticmethod
    def push(inp, grid, shape, bound, order, extrapolate, displacement=False):
        return _scatter_op(inp, grid, shape, bound, order, extrapolate, displacement, 0)

    @staticmethod
    def count(grid, shape, bound, order, extrapolate, displacement=False):
        return _scatter_op(None, grid, shape, bound, order, extrapolate, displacement, 0)

    @staticmethod
    def pushgrad(inp, grid, shape, bound, order, extrapolate, displacement=False):
        return _scatter_op(inp, grid, shape, bound, order, extrapolate, displacement, 1)

    @staticmethod
    def push_count(inp, grid, shape, bound, order, extrapolate, displacement=False):
        return torch.cat([TorchKernels.push(inp, grid, shape, bound, order, extrapolate, displacement),
                          TorchKernels.count(grid, shape, bound, order, extrapolate, displacement).to(inp.dtype)], 1)

    @staticmethod
    def push_shared_(out, inp, grid, bound, order, extrapolate, with_count=False):
        shape = list(out.shape[2:])
        if with_count:
            TorchKernels.push_shared_(out[:, :-1], inp, grid, bound, order, extrapolate)
            return TorchKernels.push_shared_(out[:, -1:], None, grid, bound, order, extrapolate)
        tmp = _scatter_op(inp, grid, shape, bound, order, extrapolate, False, 0)
        out += tmp.sum(0, keepdim=True).to(out.dtype)
        return out

    # backward compositions (pushpull.py:237-299)
    @staticmethod
    def pull_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, displacement=False):
        dim = grid.shape[-1]
        gi = gg = None
        if need_inp:
            gi = TorchKernels.push(grad, grid, list(inp.shape[-dim:]), bound, order, extrapolate, displacement)
            if inp.shape[0] == 1 and gi.shape[0] > 1:
                gi = gi.sum(0, keepdim=True)
        if need_grid:
            gg = (TorchKernels.grad(inp, grid, bound, order, extrapolate, displacement) * grad.unsqueeze(-1)).sum(1)
        return gi, gg

    @staticmethod
    def push_backward(grad, inp, grid, bound, order, extrapolate, need_inp, need_grid, displacement=False):
        gi = gg = None
        if inp is None:                                               # count: pushpull.py:286-299
            return None, TorchKernels.grad(grad, grid, bound, order, extrapolate, displacement).sum(1)
        if need_inp:
            gi = TorchKernels.pull(grad, grid, bound, order, extrapolate, displacement)
            if inp.shape[0] == 1 and gi.shape[0] > 1:
                gi = gi.sum(0, keepdim=True)
        if need_grid:
            gg = (TorchKernels.grad(grad, grid, bound, order, extrapolate, displacement) * inp.unsqueeze(-1)).sum(1)
        return gi, gg

    @staticmethod
    def count_backward(grad, grid, bound, order, extrapolate, displacement=False):
        return TorchKernels.push_backward(grad, None, grid, bound, order, extrapolate, False, True, displacement)[1]

    # gradient of the matrix of an AffineGrid: the per-sample grid gradient, pulled back through `lattice.dense()` by autograd
    # (the same mathematics as csrc/affine_grad.hip, with the (B,*shape,D) tensors the kernel avoids)
    @staticmethod
    def _through_dense(lattice, grid_gradient):
        from .sepgrid import AffineGrid
        with torch.enable_grad():
            mat = lattice.mat.detach().requires_grad_()
            dense = AffineGrid(mat, lattice.shape[1:-1]).dense()
        gg = grid_gradient(dense.detach()).sum(0, keepdim=True).to(dense.dtype)
        return torch.autograd.grad(dense, mat, gg)[0]

    @staticmethod
    def affine_pull_backward(grad, inp, lattice, bound, order, extrapolate):
        return TorchKernels._through_dense(
            lattice, lambda g: TorchKernels.pull_backward(grad, inp, g, bound, order, extrapolate, False, True)[1])

    @staticmethod
    def affine_push_backward(grad, inp, lattice, bound, order, extrapolate):
        return TorchKernels._through_dense(
            lattice, lambda g: TorchKernels.push_backward(grad, inp, g, bound, order, extrapolate, False, True)[1])

    # prefilter (coeff.py:258-284), one dim, in place
    @staticmethod
    def spline_filter_(data, bound, order, dim, src=None):
        from .filter_torch import spline_filter_
        return spline_filter_(data, bound, order, dim, src=src)

    @staticmethod
    def pull_labels(inp, grid, bound, order, extrapolate, displacement=False):
        raise NotImplementedError('the fused label-map kernel exists on the GPU only; interpol.api loops over the labels instead')

    @staticmethod
    def resample1d(src, lin, dim, order, bound, extrapolate, mode, adjoint, n_lattice):
        raise NotImplementedError('separable resampling passes exist on the GPU only; interpol.resize / restrict use a dense grid instead')
