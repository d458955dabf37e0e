"""tests/memguard.py on CPU tensors (no GPU, no library), and the one-seam rule of interpol/_hip.py."""
import os
import re
import types

import pytest
import torch

import memguard as M

HIP_PY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torch-interpol_amd", "interpol", "_hip.py")
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int32, torch.uint8]


@pytest.mark.parametrize("dtype", DTYPES)
def test_interior_and_guards_start_poisoned(dtype):
    t = M.guarded([3, 5, 7], dtype, "cpu")
    g = t._memguard
    assert t.is_contiguous() and list(t.shape) == [3, 5, 7] and t.dtype == dtype
    assert g.guard_damage() == (0, 0)
    es = t.element_size()
    assert g.lo >= max(M.GUARD_BYTES, 35 * es) and g.raw.numel() - g.hi >= max(M.GUARD_BYTES, 35 * es)
    if dtype.is_floating_point:
        assert torch.isnan(t).all() and M.unwritten(t) == t.numel()
    elif dtype == torch.int32:
        assert (t == M.LABEL_POISON).all() and M.unwritten(t) == t.numel()
    else:
        assert (t == 0xFF).all()


def test_guard_holds_one_innermost_plane_of_a_wide_tensor():
    t = M.guarded([2, 40, 50], torch.float64, "cpu")
    g = t._memguard
    assert g.lo >= 40 * 50 * 8 and g.raw.numel() - g.hi >= 40 * 50 * 8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
def test_write_into_either_guard_is_detected(dtype):
    for where in ("front", "back"):
        t = M.guarded([4, 9], dtype, "cpu", fill=0)
        flat = t._memguard.raw
        es = t.element_size()
        M.assert_guard_intact(t)
        # one element just outside the tensor, written the way a kernel's overrun would write it
        byte = t._memguard.lo - es if where == "front" else t._memguard.hi
        flat[byte:byte + es].view(dtype).fill_(1)
        front, back = t._memguard.guard_damage()
        assert (front > 0, back > 0) == (where == "front", where == "back")
        with pytest.raises(AssertionError, match="guard bytes overwritten"):
            M.assert_guard_intact(t)


def test_far_end_of_the_guard_is_watched_too():
    t = M.guarded([5], torch.float32, "cpu", fill=0)
    t._memguard.raw[0] = 0
    assert t._memguard.guard_damage() == (1, 0)
    t._memguard.raw[0] = 0xFF
    t._memguard.raw[-1] = 0
    assert t._memguard.guard_damage() == (0, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32])
def test_unwritten_element_is_detected(dtype):
    t = M.guarded([3, 4, 5], dtype, "cpu")
    t.fill_(2)
    M.assert_fully_written(t)
    t.view(-1)[37:38].view(torch.uint8).fill_(M.poison_byte(dtype))       # one element left as the allocator handed it out
    assert M.unwritten(t) == 1
    with pytest.raises(AssertionError, match="1 of 60 output elements hold poison"):
        M.assert_fully_written(t, what="case")


def test_coverage_is_judged_against_the_references_own_nans():
    t = M.guarded([6], torch.float32, "cpu", fill=1.0)
    ref = torch.ones(6)
    t[2] = float("nan")
    ref[2] = float("nan")                  # (a non-finite source legitimately gives a NaN)
    M.assert_fully_written(t, ref)
    t[4] = float("nan")
    assert M.unwritten(t, ref) == 1 and M.unwritten(t) == 2
    assert M.unwritten(t, ref.numpy()) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int32])
@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_misalign_shifts_the_base_pointer(dtype, misalign):
    for shape in ([7], [3, 5], [2, 3, 5, 7]):
        t = M.guarded(shape, dtype, "cpu", misalign=misalign)
        assert t.data_ptr() % 16 == (misalign * t.element_size()) % 16
        assert t.data_ptr() % M.ALIGN == misalign * t.element_size()
        assert t.is_contiguous() and t._memguard.guard_damage() == (0, 0)
    with pytest.raises(ValueError):
        M.guarded([4], dtype, "cpu", misalign=4)


def test_workspaces_stay_256_aligned():
    for n in (1, 255, 256, 4097, 100000):
        t = M.guarded(n, torch.uint8, "cpu")
        assert t.data_ptr() % 256 == 0 and t.numel() == n
    with pytest.raises(ValueError):
        M.guarded(64, torch.uint8, "cpu", misalign=1)
    seam = M.Seam(misalign=3)
    ws = seam.empty(1000, dtype=torch.uint8, device="cpu")
    acc = seam.empty(33, dtype=torch.float32, device="cpu")               # a flat size: a scratch accumulator
    out = seam.empty([2, 3, 5], dtype=torch.bfloat16, device="cpu")
    assert ws.data_ptr() % 256 == 0 and acc.data_ptr() % 256 == 0
    assert out.data_ptr() % 16 == 6
    assert [g.workspace for g in seam.records] == [True, True, False]
    assert len(seam.workspaces()) == 2 and len(seam.outputs()) == 1


def test_place_copies_an_input_between_guards():
    src = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    t = M.place(src, "cpu", misalign=1)
    assert torch.equal(t, src) and t.data_ptr() % 16 == 4
    M.assert_guard_intact(t)
    assert torch.isnan(t._memguard.raw[:t._memguard.lo].view(-1)[-8:].view(torch.float32)).all()
    lab = M.place(torch.arange(12, dtype=torch.int32).reshape(3, 4), "cpu")
    assert M.unwritten(lab) == 0


def test_installed_seam_records_checks_and_restores():
    calls = []

    def release():
        calls.append("release")

    hip = types.SimpleNamespace(_empty=torch.empty, _WS_NOCACHE=False, release_workspaces=release)
    with M.installed(hip, misalign=1) as seam:
        assert hip._WS_NOCACHE is True and hip._empty == seam.empty
        out = hip._empty([2, 3, 4], dtype=torch.float32, device="cpu")
        ws = hip._empty(512, dtype=torch.uint8, device="cpu")
        assert out.data_ptr() % 16 == 4 and ws.data_ptr() % 256 == 0
        assert not seam.workspace_was_written()
        seam.assert_guards_intact()
        with pytest.raises(AssertionError):
            seam.assert_fully_written(out)
        out.zero_()
        seam.assert_fully_written(out)
        ws[100] = 7
        assert seam.workspace_was_written()
        # an overrun of one element behind the output
        g = out._memguard
        g.raw[g.hi:g.hi + 4] = 0
        with pytest.raises(AssertionError, match="allocation 0"):
            seam.assert_guards_intact("case")
    assert hip._empty is torch.empty and hip._WS_NOCACHE is False
    assert calls == ["release", "release"]


def test_installed_seam_through_monkeypatch(monkeypatch):
    hip = types.SimpleNamespace(_empty=torch.empty, _WS_NOCACHE=False)
    with M.installed(hip, monkeypatch=monkeypatch) as seam:
        assert hip._empty == seam.empty
    assert hip._empty is torch.empty and hip._WS_NOCACHE is False


def test_hip_module_allocates_through_the_seam_only():
    """interpol/_hip.py: no direct torch.empty( call outside the definition of the seam (comments and strings aside)."""
    with open(HIP_PY) as f:
        src = f.read()
    code = []
    for line in src.splitlines():
        code.append(line.split("#", 1)[0])
    direct = [i for i, l in enumerate(code) if re.search(r"\btorch\s*\.\s*empty\s*\(", l)]
    assert len(direct) == 1, [(i + 1, code[i]) for i in direct]
    assert code[direct[0]].strip() == "return torch.empty(*size, **kw)" and code[direct[0] - 1].startswith("def _empty(")
    assert not re.search(r"\btorch\s*\.\s*empty\b(?!\s*\()(?!_)", "\n".join(code)), "torch.empty bound to another name"
    assert len(re.findall(r"(?<![\w.])_empty\(", src)) >= 15
    # other spellings that would bypass it
    for other in ("torch.zeros(", "torch.empty_like(", "torch.zeros_like(", "torch.full(", "new_empty("):
        hits = [l for l in code if other in l]
        assert all("return torch.zeros([dim, dim + 1]" in l for l in hits), (other, hits)


def test_poison_switch_covers_every_workspace_site():
    """INTERPOL_POISON_SCRATCH: every workspace / scratch accumulator goes through `_scratch` (source inspection)."""
    with open(HIP_PY) as f:
        src = f.read()
    for fn, n in (("gather", 1), ("scatter", 1), ("pull_backward", 2), ("push_backward", 1), ("_affine_reduce", 1), ("push_bricks", 1)):
        body = re.search(r"^def %s\(.*?(?=^def |\Z)" % fn, src, re.S | re.M).group(0)
        assert body.count("_scratch(") >= n, fn
        # no workspace is handed to the library un-routed
        for m in re.finditer(r"=\s*(_optional_workspace\(|_empty\([^\n]*torch\.uint8)", body):
            line = body[body.rfind("\n", 0, m.start()) + 1:body.find("\n", m.end())]
            assert "_scratch(" in line or fn == "scatter", (fn, line)
