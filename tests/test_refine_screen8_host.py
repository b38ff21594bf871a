"""Host checks of the int8 pre-screen's arithmetic (refine.hip ScreenI8, matching.hip desc_planar), no GPU.

* the bound: |S_half_chain - S8 / 127^2| <= B8 = B + E8 over > 10^5 operand pairs (components at +-1, zeros, half
  subnormals, worst-case sign patterns), the half chain with the oracle's rounding;
* the quantiser's edge values: values that round to +-127, the RNE midpoints, -1;
* the census script's replay on a 48 x 64 pair (it asserts that both survivor rules keep the exact winner);
* the layout case's premise: its first level has tiles for the one-fill and for the two-fill int8 window.
"""
import importlib.util
import os

import numpy as np

import refine_screen8_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bound_covers_half_chain_minus_int8_dot():
    q, c = C.bound_pairs()
    assert len(q) >= 100000
    assert np.abs(q).max() <= 1.0 and np.abs(c).max() <= 1.0
    assert (np.abs(q) == 1.0).any() and (q == 0).any() and ((np.abs(c) < 2.0 ** -14) & (c != 0)).any()
    sh = C.half_chain(q, c).astype(np.float64)
    q8, c8 = C.quantise8(q), C.quantise8(c)
    s8 = C.s8(q8, c8) / (127.0 * 127.0)
    # the frame's maxima taken per pair (the tightest the kernel can see: one candidate pixel in the image)
    cmax = np.linalg.norm(c.astype(np.float64), axis=-1)
    c1max = np.abs(c.astype(np.float64)).sum(-1)
    B = C.bound_B(q, cmax)
    E8 = C.bound_E8(q8, c1max)
    # E8 alone bounds the quantisation error of the real dot of the half operands
    real = (q.astype(np.float64) * c.astype(np.float64)).sum(-1)
    slack_q = E8 - np.abs(real - s8)
    slack = (B + E8) - np.abs(sh - s8)
    print(f"{len(q)} pairs: min slack of E8 {slack_q.min():.3e}, of B8 {slack.min():.3e}; "
          f"max |S_half - S8/127^2| {np.abs(sh - s8).max():.4f}, max B8 {(B + E8).max():.4f}")
    assert (slack_q >= -1e-12).all()
    assert (slack >= 0).all()


def test_quantiser_edge_values():
    h = C.half
    h1 = lambda v: float(h(np.array([v], np.float32))[0])  # noqa: E731
    # RNE midpoints: 127 x = n + 0.5 needs x = (2 n + 1) / 254, a half value only when 127 divides 2 n + 1: x = +-0.5
    # (63.5 -> 64, the even neighbour) and +-1.5 (190.5, clamped to 127)
    assert C.quantise8(h(np.array([0.5, -0.5], np.float32))).tolist() == [64, -64]
    assert int(C.quantise8(np.float32(1.5))) == 127 and int(C.quantise8(np.float32(-1.5))) == -127
    # ordinary values against Python's round (half-even) of the product, which is exact in double
    for v in (0.25, 2.0 ** -8, 3 * 2.0 ** -9, 0.99951171875, 0.996, 0.9921875, 1.0 / 127.0, 0.5 / 127.0):
        xv = h1(v)
        want = int(np.clip(round(127.0 * xv), -127, 127))
        assert int(C.quantise8(np.float32(xv))) == want
        assert int(C.quantise8(np.float32(-xv))) == -want
    # rounds to +-127: the largest half below 1 (0.99951 * 127 = 126.94) and 1 itself; -1 -> -127 (never -128)
    assert int(C.quantise8(np.float32(h1(0.9995)))) == 127
    assert int(C.quantise8(np.float32(1.0))) == 127
    assert int(C.quantise8(np.float32(-1.0))) == -127
    assert int(C.quantise8(np.float32(-65504.0))) == -127
    # just below / above the midpoint 126.5 / 127 = 0.99606..: the neighbouring halves 0.99561 and 0.99609 (step 2^-11)
    lo, hi = np.float32(2039 / 2048.0), np.float32(2040 / 2048.0)
    assert 127.0 * float(lo) < 126.5 < 127.0 * float(hi)
    assert int(C.quantise8(lo)) == 126 and int(C.quantise8(hi)) == 127
    # zeros and half subnormals quantise to 0
    assert C.quantise8(np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -15], np.float32)).tolist() == [0, 0, 0, 0]


def test_census_replay_48x64():
    spec = importlib.util.spec_from_file_location("refine_screen8_census",
                                                  os.path.join(ROOT, "scripts", "refine_screen8_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.census(48, 64, seed=1)
    assert sorted(r) == [1, 2, 3, 4, 5]
    for d, res in r.items():
        (fp, fw), (ip, iw) = res["f16"], res["int8"]
        assert 0 <= fp <= ip <= 49 and 0 <= fw <= iw <= 49  # the int8 band is the wider one
    assert abs(r[5]["f16"][0] - 1.0) < 0.05  # the first level keeps the winner alone on a smooth pair


def test_layout_case_reaches_both():
    case = dict(C.gpu_cases())["layouts_d3"]
    rows, cols = C.first_level_covers(case)
    one = (rows <= C.ONE_FILL_ROWS) & (cols <= C.ONE_FILL_COLS)
    two = ~one & (rows <= C.WIN_ROWS) & (cols <= C.WIN_COLS)
    assert one.any() and two.any(), (rows.tolist(), cols.tolist())
