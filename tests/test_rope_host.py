"""CPU: RoPE2D's host side. The library's cos / sin table against numpy, tests/rope_cases.py's restatement (the
device test's bit reference) against the float64 truth, the binding of the reference's own cuRoPE2D to the package's
``curope`` module, the argument checks of ``curope.rope_2d``, and the exports."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import curope
import rope_cases as RC
from m3s.rope import RoPE2D, rope2d_torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightweight-mast3r-slam_amd")
TESTS = os.path.join(REPO, "tests")
CROCO = "/root/reference/thirdparty/mast3r/dust3r/croco"


def _numpy_table(base, fwd, Q, P):
    inv = np.float64(fwd) / np.power(np.float64(base), np.arange(Q, dtype=np.float64) / Q)
    ang = np.arange(P, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


@pytest.mark.parametrize("Q", [3, 16])
def test_table_is_float32_of_the_float64_cos_and_sin(Q):
    """Every entry within 1 fp32 ulp of float32(np.cos / np.sin(float64 angle)) (libm and numpy may round the float64
    value differently in the last place; for (100, 1, 16) they agreed on all 16,384 entries where this was written);
    the fwd = -1 table has the same cosines and the negated sines, bit for bit."""
    tabs = {}
    for fwd in (1.0, -1.0):
        cos, sin = RC.lib_table(RC.BASE, fwd, Q)
        assert cos.shape == sin.shape == (RC.TABLE_P, Q) and cos.dtype == sin.dtype == np.float32
        want_c, want_s = _numpy_table(RC.BASE, fwd, Q, RC.TABLE_P)
        n_diff = int((cos != want_c).sum() + (sin != want_s).sum())
        print(f"Q={Q} fwd={fwd:+.0f}: {n_diff} of {2 * cos.size} entries differ from numpy's")
        for got, want in ((cos, want_c), (sin, want_s)):
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
        tabs[fwd] = (cos, sin)
    assert np.array_equal(tabs[1.0][0].view(np.uint32), tabs[-1.0][0].view(np.uint32))
    assert np.array_equal(tabs[1.0][1].view(np.uint32), (-tabs[-1.0][1]).view(np.uint32))
    assert (tabs[1.0][0][0] == 1.0).all() and (tabs[1.0][1][0] == 0.0).all()  # position 0: the identity


def test_table_rejects_bad_arguments():
    from m3s import _lib

    for args in ((0.0, 1.0, 16), (100.0, 1.0, 0), (float("nan"), 1.0, 16), (100.0, float("inf"), 16)):
        with pytest.raises(RuntimeError):
            _lib.rope2d_table(*args)


def test_restatement_is_within_the_fp32_bound_of_the_truth():
    """With the library's table the restatement is within 3 * 2^-24 * (|u| + |v|) of the float64 truth in f32: the two
    table entries contribute <= 2^-25 each, the two products <= 2^-24 relative, the final sum <= 2^-24 (2.5 in all).
    Measured where this was written: 1.8 * 2^-24."""
    tok, pos = RC.make_case(11, **RC.HOST_SHAPE)
    worst = 0.0
    for fwd in RC.F0S:
        cos, sin = RC.lib_table(RC.BASE, fwd, RC.HOST_SHAPE["D"] // 4)
        got = RC.restate(tok, pos, cos, sin).to(torch.float64).numpy()
        want, mag = RC.truth(tok, pos, RC.BASE, fwd)
        assert not np.array_equal(got, tok.to(torch.float64).numpy())
        ratio = float((np.abs(got - want) / mag).max() * 2.0 ** 24)
        print(f"fwd={fwd:+.0f}: max |restatement - truth| / (|u| + |v|) = {ratio:.2f} * 2^-24")
        worst = max(worst, ratio)
    assert worst <= 3.0


def test_torch_statement_agrees_with_the_truth():
    """m3s.rope.rope2d_torch in float64 is the truth to rounding; in float32 it is inside the restatement's bound."""
    tok, pos = RC.make_case(11, **RC.HOST_SHAPE)
    want, mag = RC.truth(tok, pos, RC.BASE, 1.0)
    got64 = rope2d_torch(tok.to(torch.float64), pos, RC.BASE, 1.0)
    assert got64.dtype == torch.float64 and got64.shape == tok.shape
    # two float64 evaluations: the angle (below 48 < 2^6) carries a few roundings of 2^-53 relative, so c and s differ
    # by less than 2^-45; 2^-40 leaves room for the two libraries' pow, cos and sin
    assert (np.abs(got64.numpy() - want) <= 2.0 ** -40 * mag).all()
    got32 = rope2d_torch(tok, pos, RC.BASE, 1.0)
    assert got32.dtype == torch.float32
    assert (np.abs(got32.to(torch.float64).numpy() - want) <= 3.0 * 2.0 ** -24 * mag).all()
    half = rope2d_torch(tok.to(torch.float16), pos, RC.BASE, 1.0)
    assert half.dtype == torch.float16
    with pytest.raises(RuntimeError, match="multiple of 4"):
        rope2d_torch(torch.zeros(1, 2, 1, 6), torch.zeros(1, 2, 2, dtype=torch.int64), RC.BASE, 1.0)


# ---- the reference's own classes, each in a process of its own (``models`` must not leak into this one) ----

_BIND_SCRIPT = """
import json, os, sys
sys.path[:0] = [%(croco)r, %(pkg)r]
import models.pos_embed as PE
import models.curope as MC
import models.curope.curope2d as C2
import curope
print(json.dumps(dict(same_class=PE.RoPE2D is MC.cuRoPE2D, kernels_is_ours=C2._kernels is curope,
                      curope_file=os.path.abspath(curope.__file__))))
"""

_SLOW_SCRIPT = """
import json, sys
sys.path[:0] = [%(croco)r, %(tests)r]
import numpy as np
import torch
import models.pos_embed as PE
import rope_cases as RC
assert "curope" not in sys.modules and hasattr(PE.RoPE2D, "apply_rope1d")  # the slow torch class
tok, pos = RC.make_case(11, **RC.HOST_SHAPE)
got = PE.RoPE2D(freq=RC.BASE, F0=1.0)(tok.transpose(1, 2), pos).transpose(1, 2)  # the class takes (B,H,N,D)
want, mag = RC.truth(tok, pos, RC.BASE, 1.0)
ratio = float((np.abs(got.to(torch.float64).numpy() - want) / mag).max() * 2.0 ** 24)
print(json.dumps(dict(ratio=ratio, moved=float(np.abs(want - tok.to(torch.float64).numpy()).max()))))
"""


def _run(script):
    out = subprocess.run([sys.executable, "-B", "-c", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stdout


@pytest.mark.skipif(not os.path.isdir(CROCO), reason="the reference tree is not on this machine")
def test_reference_curope2d_binds_to_this_package():
    """With the package directory on the path, models/pos_embed.py takes its cuRoPE2D (no slow-class warning) and that
    class's kernels are this package's curope module."""
    res, stdout = _run(_BIND_SCRIPT % dict(croco=CROCO, pkg=PKG))
    assert res["same_class"] and res["kernels_is_ours"]
    assert res["curope_file"] == os.path.join(PKG, "curope", "__init__.py")
    assert "slow pytorch version" not in stdout


@pytest.mark.skipif(not os.path.isdir(CROCO), reason="the reference tree is not on this machine")
def test_reference_slow_class_has_this_layout():
    """The reference's slow torch class (what runs without the extension) is within 2^-16 * (|u| + |v|) of the float64
    truth of rope_cases: its fp32 angle carries <= 4 roundings of 2^-24 relative, scaled by an angle below 64. This
    pins the layout (y half then x half, u block then v block) to the reference's: a wrong one is off by O(1).
    Measured where this was written: 28 * 2^-24."""
    res, stdout = _run(_SLOW_SCRIPT % dict(croco=CROCO, tests=TESTS))
    print(f"reference slow class: max |got - truth| / (|u| + |v|) = {res['ratio']:.1f} * 2^-24")
    assert "slow pytorch version" in stdout
    assert res["moved"] > 1.0  # the rotation is no near-identity on this case
    assert res["ratio"] <= 2.0 ** 8


# ---- curope.rope_2d's checks, which precede the device check ----

def _good():
    return torch.ones(2, 5, 3, 8), torch.zeros(2, 5, 2, dtype=torch.int64)


@pytest.mark.parametrize("mutate, message", [
    (lambda t, p: (t[0], p), "tokens must have 4 dimensions"),
    (lambda t, p: (t, p[0]), "positions must have 3 dimensions"),
    (lambda t, p: (t[:1], p), "batch size differs between tokens & positions"),
    (lambda t, p: (t[:, :4], p), "seq_length differs between tokens & positions"),
    (lambda t, p: (t, torch.zeros(2, 5, 3, dtype=torch.int64)), r"positions.shape\[2\] must be equal to 2"),
    (lambda t, p: (t.transpose(1, 2).contiguous().transpose(1, 2), p), "tokens are not contiguous"),
    (lambda t, p: (torch.ones(2, 5, 3, 16)[..., ::2], p), "tokens are not contiguous"),
    (lambda t, p: (t, torch.zeros(2, 5, 4, dtype=torch.int64)[..., ::2]), "positions are not contiguous"),
    (lambda t, p: (torch.ones(2, 5, 3, 6), p), "token dim must be multiple of 4"),
    (lambda t, p: (t, p.to(torch.int32)), "positions must be int64"),
    (lambda t, p: (t.to(torch.float64), p), "must be float16, float32 or bfloat16"),
], ids=["tokens_dim", "positions_dim", "batch", "seq_length", "pos_last", "head_stride", "last_stride",
        "pos_strides", "dim_mod_4", "pos_dtype", "f64"])
def test_rope_2d_rejects_like_the_reference(mutate, message):
    tok, pos = mutate(*_good())
    before = tok.clone()
    with pytest.raises(RuntimeError, match=message):
        curope.rope_2d(tok, pos, RC.BASE, 1.0)
    assert torch.equal(tok, before)


def test_rope_2d_has_no_cpu_path():
    tok, pos = _good()
    for t in (tok, tok.to(torch.float16), tok.to(torch.bfloat16), torch.ones(2, 5, 3, 3, 8)[:, :, 0]):
        before = t.clone()
        with pytest.raises(RuntimeError, match="must be on the HIP device"):
            curope.rope_2d(t, pos, RC.BASE, 1.0)
        assert torch.equal(t, before)
    with pytest.raises(RuntimeError, match="must be on the HIP device"):
        RoPE2D()(tok.transpose(1, 2), pos)
    with pytest.raises(RuntimeError, match="forward only"):
        RoPE2D()(tok.transpose(1, 2).requires_grad_(), pos)
    assert torch.equal(tok, torch.ones_like(tok))


def test_rope_exports_and_abi_version():
    from m3s import _lib

    header = open(os.path.join(REPO, "include", "m3s.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("m3s_rope2d", "m3s_rope2d_prepare", "m3s_rope2d_table", "m3s_rope2d_release"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b%s\s*\(" % s, header), s
    lib.m3s_abi_version.restype = ctypes.c_int
    assert lib.m3s_abi_version() == _lib.ABI_VERSION == 10
    assert int(re.search(r"#define M3S_ABI_VERSION (\d+)", header).group(1)) == 10


def test_rope2d_abi_argument_checks_touch_no_device():
    """M3S_EINVAL before any HIP call: bad dtype, D % 4, negative sizes, null pointers with work; empty work is OK."""
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_float * 64)()
    pos = (ctypes.c_int64 * 8)()
    tp, pp = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(pos, ctypes.c_void_p)
    call = lambda dt, t, p, B, N, H, D: lib.m3s_rope2d(dt, t, 64, 16, p, B, N, H, D, 100.0, 1.0, None)  # noqa: E731
    assert call(3, tp, pp, 1, 4, 1, 16) == _lib.EINVAL
    assert call(-1, tp, pp, 1, 4, 1, 16) == _lib.EINVAL
    assert call(1, tp, pp, 1, 4, 1, 6) == _lib.EINVAL
    assert call(1, tp, pp, -1, 4, 1, 16) == _lib.EINVAL
    assert call(1, None, pp, 1, 4, 1, 16) == _lib.EINVAL
    assert call(1, tp, None, 1, 4, 1, 16) == _lib.EINVAL
    assert "null pointer" in lib.m3s_last_error().decode()
    for shape in ((0, 4, 1, 16), (1, 0, 1, 16), (1, 4, 0, 16)):
        assert call(1, None, None, *shape) == 0
    assert all(v == 0.0 for v in buf)
