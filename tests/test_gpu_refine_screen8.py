"""GPU parity of the int8 pre-screen at the refine levels d >= 2 (refine.hip ScreenI8).

match()'s idx and valid must be bit-identical with the path on (default), with M3S_REFINE_SCREEN8=0 (the f16 screen at
every level) and with M3S_REFINE_SCREEN=0 (the exact scan), and equal to the oracle. No tolerances. The cases
(tests/refine_screen8_cases.py) are the smallest shapes that reach each branch: the int8 levels on a smooth pair,
border tiles, window outliers beside int8 levels, the frame-wide and the lane-level fallbacks, all-ties, a 0.03 score
ladder (inside the int8 band, outside the f16 band), NaN / inf descriptors, and both int8 window layouts.
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O
import refine_screen8_cases as C

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def cases():
    built = dict(C.gpu_cases())
    assert sorted(built) == sorted(C.GPU_CASE_NAMES)
    return built


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(args):
    from m3s.matching import match

    idx, valid = match(*args)
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), valid.cpu().numpy().copy()


@pytest.mark.parametrize("name", C.GPU_CASE_NAMES)
def test_int8_screen_is_bit_identical(monkeypatch, cases, name):
    from m3s.config import config

    c = cases[name]
    config["matching"]["dilation_max"] = c["dilation_max"]
    args = [_dev(c[k]) for k in ("X11", "X21", "D11", "D21")]
    if c["idx_init"] is not None:
        args.append(_dev(c["idx_init"]))
    ref = O.match(c["X11"], c["X21"], c["D11"], c["D21"], idx_init=c["idx_init"], dilation_max=c["dilation_max"])
    monkeypatch.delenv("M3S_REFINE_SCREEN8", raising=False)
    monkeypatch.delenv("M3S_REFINE_SCREEN", raising=False)
    on = _run(args)
    monkeypatch.setenv("M3S_REFINE_SCREEN8", "0")
    f16 = _run(args)
    monkeypatch.delenv("M3S_REFINE_SCREEN8")
    monkeypatch.setenv("M3S_REFINE_SCREEN", "0")
    exact = _run(args)
    monkeypatch.delenv("M3S_REFINE_SCREEN")
    # the three-launch path's tile instance has the int8 levels too
    monkeypatch.setenv("M3S_MATCH_FUSE_PROJ", "0")
    unfused = _run(args)
    for what, got in (("int8 screen", on), ("f16 screen", f16), ("exact scan", exact), ("int8, unfused", unfused)):
        mism = int((got[0] != ref[0]).sum())
        print(f"{name}: {what}: {mism} idx mismatches against the oracle ({c['reaches']})")
    for got in (on, f16, exact, unfused):
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
