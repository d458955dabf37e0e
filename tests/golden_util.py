"""Loader for the golden vectors of tests/golden/ (generated from the reference
by tests/golden/make_golden.py in the build container)."""
import json
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def arrays():
    if "npz" not in _CACHE:
        _CACHE["npz"] = np.load(os.path.join(HERE, "golden_ops.npz"))
    return _CACHE["npz"]


def manifest():
    if "ops" not in _CACHE:
        with open(os.path.join(HERE, "golden_ops.json")) as f:
            _CACHE["ops"] = json.load(f)
    return _CACHE["ops"]


def api():
    if "api" not in _CACHE:
        with open(os.path.join(HERE, "golden_api.json")) as f:
            _CACHE["api"] = json.load(f)
    return _CACHE["api"]


def mid():
    """Mid-size cases (>= 4096 samples: they reach the LDS-tile kernels), tests/golden/make_golden_mid.py.
    Returns (manifest, arrays); inputs are float32, expected outputs the reference's float64 results
    stored as float32."""
    if "mid" not in _CACHE:
        with open(os.path.join(HERE, "golden_mid.json")) as f:
            _CACHE["mid"] = (json.load(f), np.load(os.path.join(HERE, "golden_mid.npz")))
    return _CACHE["mid"]


def fold():
    """Scatter cases on lattices of 33 - 40 points (the end bricks of the owner-computes push fold), sample grids that
    overhang the lattice, tests/golden/make_golden_fold.py.  Same conventions as mid()."""
    if "fold" not in _CACHE:
        with open(os.path.join(HERE, "golden_fold.json")) as f:
            _CACHE["fold"] = (json.load(f), np.load(os.path.join(HERE, "golden_fold.npz")))
    return _CACHE["fold"]


def arr(name, dtype=np.float64):
    return np.asarray(arrays()[name], dtype=dtype)


def rel_err(got, want):
    """max |got-want| / max|want| (the `atol = tol*max|ref|` criterion of SURVEY A.8)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    scale = max(float(np.abs(want).max()), 1e-30)
    return float(np.abs(got - want).max()) / scale


def assert_close(got, want, rtol, atol_rel, what=""):
    """|got - want| <= rtol*|want| + atol_rel*max|want| elementwise."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    atol = atol_rel * max(float(np.abs(want).max()), 1e-30)
    bad = np.abs(got - want) > (rtol * np.abs(want) + atol)
    assert not bad.any(), "%s: %d/%d mismatches, max abs err %.3e (scale %.3e)" % (
        what, int(bad.sum()), bad.size, float(np.abs(got - want).max()), float(np.abs(want).max()))



def f32_masked_samples(grid, shape, extrapolate):
    """Samples that the reference masks when it runs in float32 and a float64 evaluation of the SAME float32 coordinates does
    not (nd.py:10-27): the Python scalar threshold (-thr, n - 1 + thr; thr = 0.05 / 0.55) is cast to the tensor's
    dtype for the comparison, so a float32 coordinate EQUAL to the float32-rounded threshold is outside in float32 and -- where
    the rounding went towards the inside -- still inside in float64.  Returns a bool array (B, *out): expected outputs of
    gathers at those samples are zeros (the mask multiplies the result).  The opposite disagreement cannot occur (no float32
    lies strictly between a double and its nearest float32); asserted."""
    g32 = np.asarray(grid, dtype=np.float32)
    out = np.zeros(g32.shape[:-1], dtype=bool)
    if extrapolate == 1:
        return out
    thr = 0.05 if extrapolate == 0 else 0.55
    m32 = np.ones(g32.shape[:-1], dtype=bool)
    m64 = np.ones(g32.shape[:-1], dtype=bool)
    for d, n in enumerate(shape):
        x32, x64 = g32[..., d], g32[..., d].astype(np.float64)
        m32 &= (x32 > np.float32(-thr)) & (x32 < np.float32(n - 1 + thr))
        m64 &= (x64 > -thr) & (x64 < n - 1 + thr)
    assert not (m32 & ~m64).any()
    return m64 & ~m32

def run_case(ops, case, dtype):
    """Run one manifest case through an operator table `ops` exposing the
    pushpull-style functions grid_pull/grid_push/... on numpy arrays."""
    ins = {k: arr(v, dtype) for k, v in case["inputs"].items()}
    b, o, e = case["bound"], case["order"], case["extrapolate"]
    op = case["op"]
    if op == "pull":
        return ops.grid_pull(ins["inp"], ins["grid"], b, o, e)
    if op == "grad":
        return ops.grid_grad(ins["inp"], ins["grid"], b, o, e)
    if op == "hess":
        return ops.grid_hess(ins["inp"], ins["grid"], b, o, e)
    if op == "push":
        return ops.grid_push(ins["inp"], ins["grid"], case["shape"], b, o, e)
    if op == "count":
        return ops.grid_count(ins["grid"], case["shape"], b, o, e)
    if op == "pushgrad":
        return ops.grid_pushgrad(ins["inp"], ins["grid"], case["shape"], b, o, e)
    raise ValueError(op)


def fp32_tol(case_or_order=None):
    """Stated fp32 parity tolerance (rtol, atol relative to max|ref|): north_star's rtol = 1e-5 with atol = 1e-5 max|ref|
    (SURVEY A.8), for EVERY spline order.  The goldens are the reference's float64 outputs; the kernels evaluate the
    middle pieces of the order 4-7 splines about their outer breakpoints (csrc/spline_math.hpp), which keeps the fp32
    weights within 1e-7 of the exact ones where the reference's own fp32 Horner forms (splines.py:56-79) lose five
    digits.  Measured worst errors, in units of this tolerance: tests/tolerance_report.py -> profiles/r04_tolerance.txt."""
    return (1e-5, 1e-5)


def reference_fp32_tol(case_or_order):
    """What the REFERENCE's own fp32 arithmetic achieves against its fp64 outputs (the oracle's fp32 mode restates it,
    tests/test_oracle_golden.py): rtol 1e-5 with atol 1e-5 max|ref| up to order 5; for orders 6 and 7 its Horner polynomials
    (splines.py:56-79) cancel near the knots and it deviates by up to 1.3e-5 max|ref| on these vectors: 5e-5 there.  The HIP
    kernels are held to fp32_tol() for every order."""
    order = case_or_order["order"] if isinstance(case_or_order, dict) else case_or_order
    order = order if isinstance(order, (list, tuple)) else [order]
    return (1e-5, 5e-5) if max(order) >= 6 else (1e-5, 1e-5)


def resize_cases():
    """resize / restrict golden cases (tests/golden/make_golden_resize.py): list of dicts with
    fn, kwargs, inp (float32), out64 (reference on the float64 input), out32 (on the float32 input)."""
    if "resize" not in _CACHE:
        with open(os.path.join(HERE, "golden_resize.json")) as f:
            man = json.load(f)
        npz = np.load(os.path.join(HERE, "golden_resize.npz"))
        _CACHE["resize"] = [dict(c, inp=npz[c["inp"]], out64=npz[c["out64"]], out32=npz[c["out32"]]) for c in man["cases"]]
    return _CACHE["resize"]


def label_cases():
    """label-map golden cases (tests/golden/make_golden_labels.py): dicts with dim, order, bound,
    extrapolate, lab (int64), grid (float32), out (int64: the reference's result)."""
    if "labels" not in _CACHE:
        with open(os.path.join(HERE, "golden_labels.json")) as f:
            man = json.load(f)
        npz = np.load(os.path.join(HERE, "golden_labels.npz"))
        _CACHE["labels"] = [dict(c, lab=npz["l%d/lab" % c["i"]].astype(np.int64), grid=npz["l%d/grid" % c["i"]],
                                 out=npz["l%d/out" % c["i"]].astype(np.int64)) for c in man["cases"]]
    return _CACHE["labels"]


PIN_WHOLE = 64           # reference results of up to this many elements are stored whole
PIN_SAMPLE = 8           # larger ones: the values at this many evenly spaced elements and at the arg-max of |ref|


def digest(a):
    """sha256 (first 32 hex digits) of an array's dtype, shape and bytes."""
    import hashlib
    import torch
    a = np.ascontiguousarray(torch.as_tensor(a).detach().cpu().numpy())
    h = hashlib.sha256()
    h.update(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()[:32]


class Pinned:
    """A reference result too large to store whole: its shape, max |ref|, its values at a few flat indices, and the digest
    of the oracle output that make_golden_pins.py compared with the WHOLE result (and found within the test's tolerance)."""

    def __init__(self, shape, scale, index, values, oracle_digest):
        self.shape, self.scale, self.index, self.values, self.oracle_digest = tuple(shape), scale, index, values, oracle_digest


class Pins:
    """The reference's results for the calls of one test module, stored call by call under tests/golden/<stem>.npz (the
    manifest as JSON text in its member `manifest`) and replayed in the same order.  In a test: `pins.begin(test name)`, then `ref = pins(lambda: <a call of the reference>)`
    gives what that call returned (a tensor, a tuple of tensors, or None); results of more than PIN_WHOLE elements come back
    as Pinned, unless the call says `whole=True`, and the oracle's output is compared with them through
    `pins.diff(got, ref)` only.
    tests/golden/make_golden_pins.py switches the object to recording (`record()`), runs the module under pytest with the
    live reference -- every comparison then sees the whole result -- and writes the files (`save()`); everywhere else the
    lambdas are never called."""

    def __init__(self, stem):
        self.stem, self.recording, self.node, self.k = stem, False, None, 0
        self.manifest, self.arrays, self.seen = {}, {}, {}

    def record(self):
        self.recording, self.manifest, self.arrays, self.seen = True, {}, {}, {}

    def begin(self, node):
        self.node, self.k = node, 0

    def _load(self):
        if self.stem not in _CACHE:
            npz = np.load(os.path.join(HERE, self.stem + ".npz"))
            _CACHE[self.stem] = (json.loads(npz["manifest"].tobytes().decode()), npz)
        return _CACHE[self.stem]

    def __call__(self, fn, whole=False):
        import torch
        key = "%s|%d" % (self.node, self.k)
        self.k += 1
        if self.recording:
            out = fn()
            names = []
            for t in (() if out is None else out if isinstance(out, (tuple, list)) else (out,)):
                names.append("a%d" % len(self.arrays))
                self.arrays[names[-1]] = t.detach().cpu().numpy()
                self.seen[id(t)] = (t, names[-1], "whole" if whole else None)       # (keeps t alive: ids stay unique)
            self.manifest[key] = None if out is None else names if isinstance(out, (tuple, list)) else names[0]
            return out
        man, npz = self._load()
        assert key in man["calls"], "no stored result for %s: regenerate with tests/golden/make_golden_pins.py" % key
        names = man["calls"][key]

        def get(n):
            if n in man["pinned"]:
                p = man["pinned"][n]
                at = slice(p["at"], p["at"] + p["n"])
                return Pinned(p["shape"], p["scale"], npz["sample_i"][at], npz["sample_v"][at], p["oracle"])
            w = man["whole"][n]
            return torch.from_numpy(npz["whole_" + w["dtype"]][w["at"]:w["at"] + int(np.prod(w["shape"]))].reshape(w["shape"]))
        if names is None:
            return None
        return get(names) if isinstance(names, str) else tuple(get(n) for n in names)

    def diff(self, got, ref):
        """(max |got - ref|, max |ref|) for an oracle output `got` and a result `ref` of pins().  For a Pinned result the
        difference is taken at its stored elements, and `got` must be bit-identical to the output that was compared with
        the whole result when it was recorded."""
        import torch
        got = torch.as_tensor(got).detach()
        if isinstance(ref, Pinned):
            assert tuple(got.shape) == ref.shape, (tuple(got.shape), ref.shape)
            d = (got.reshape(-1)[torch.from_numpy(ref.index)].double() - torch.from_numpy(ref.values).double()).abs().max()
            assert digest(got) == ref.oracle_digest, (
                "%s: the oracle's output is not the one compared with the reference's whole result (max difference at the stored "
                "elements %.3g); if the oracle or the inputs changed on purpose, re-record with tests/golden/make_golden_pins.py"
                % (self.node, float(d)))
            return float(d), ref.scale
        if self.recording and id(ref) in self.seen and self.seen[id(ref)][2] != "whole":
            t, name, _ = self.seen[id(ref)]
            self.seen[id(ref)] = (t, name, digest(got))
        ref = torch.as_tensor(ref).detach()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return float((got.double() - ref.double()).abs().max()), float(ref.double().abs().max())

    def save(self):
        oracle = {name: dg for t, name, dg in self.seen.values()}
        store, pinned, sample_i, sample_v, at = {}, {}, [], [], 0
        whole, parts = {}, {}
        for name, a in self.arrays.items():
            if a.size <= PIN_WHOLE or oracle[name] == "whole":
                part = parts.setdefault(a.dtype.name, [])
                whole[name] = {"dtype": a.dtype.name, "shape": list(a.shape), "at": sum(x.size for x in part)}
                part.append(a.reshape(-1))
                continue
            assert oracle[name] is not None, "%s: a large result that no comparison went through pins.diff()" % name
            flat = a.reshape(-1)
            idx = np.unique(np.concatenate([np.linspace(0, flat.size - 1, PIN_SAMPLE).round(), [np.abs(flat).argmax()]]))
            idx = idx.astype(np.int64)
            sample_i.append(idx)
            sample_v.append(flat[idx].astype(np.float64))           # (float32 values are exact in float64)
            pinned[name] = {"shape": list(a.shape), "scale": float(np.abs(flat.astype(np.float64)).max()), "oracle": oracle[name],
                            "at": at, "n": len(idx)}
            at += len(idx)
        for dt, part in parts.items():
            store["whole_" + dt] = np.concatenate(part)
        store["sample_i"] = np.concatenate(sample_i).astype(np.int32)
        store["sample_v"] = np.concatenate(sample_v)
        man = json.dumps({"generator": "tests/golden/make_golden_pins.py", "reference": "balbasty/torch-interpol @2024_10_08",
                          "calls": self.manifest, "whole": whole, "pinned": pinned}, separators=(",", ":"), sort_keys=True)
        store["manifest"] = np.frombuffer(man.encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, self.stem + ".npz"), **store)
