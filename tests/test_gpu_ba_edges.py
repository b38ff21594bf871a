"""GPU: the BA linearisation (csrc/ba.hip: ba_pack_kernel, ba_lin_kernel, ba_edge_kernel) against the oracle's fp64 build,
edge by edge, on densely weighted edges.

The cases, the fp64 truth, the metric rho and the reference's own rho_ref are in tests/ba_edge_cases.py;
tests/test_ba_edges_host.py checks on the CPU that every case reaches what it is named for. Which shape reaches which
path, and the measured figures: DESIGN.md, BA, "edge shapes".

Bound: the device's rho <= 4 rho_ref on every edge, rho_ref being the larger rho of the fp32 restatement of the
reference in its two summation orders against the same truth, computed here on the CPU at run time. Entries whose
error scale is 0 in the truth (an edge without weight, g of the zero-residual case) must be exactly 0.0.

Measured on an MI355X (every test prints rho_ref and the device's rho per edge): rho_ref 4.5e-7 to 4.9e-6 on the
shapes, the device's largest rho 4.8e-6 (n5123 calib, 1.7 rho_ref); the largest rho / rho_ref of one case 2.6 (C513
calib: 1.74e-6 against 6.74e-7); zero residual 7.8e-8 against 1.4e-7. Per family: DESIGN.md.

Mutation check (by hand, not committed; red tests of this file / which of the older tests/test_gpu_ba.py tests turn
red, the RCCL, two-process and forced-stall tests not run):
  1. RoundPts ``has1 = k + bd <= c.k_end``: 22 red (n256, n257, n511, n1300c5, C1300c5) / test_gauss_newton_vs_oracle
     and test_factor_graph_matches_reference red, the rest green.
  2. no final flush after an in-loop flush of run_step: 2 red (n33000 rays, calib) / all green.
  3. ``cj * si`` for ``cj * sj`` in ba_pack_kernel and pack_record: 6 red (zero-copy against stacked) / all green.
  4. rows_calib without ``(vv < vh)``: 2 red (calib4100, tum4100) / all green.
  5. ``k > k_end`` in ba_pack_kernel's store loop (it stores a record at index N, over the rays' |Xi| of points 0..3):
     run only where N is no multiple of 4, where that store and the |Xi| store behind it stay inside the edge's own
     slot (n7, n15, n257, n511, n513, n5123, C513, ids513, zero513): 7 red, all rays (n257, n511, n513, C513 three
     times, ids513) / the older tests not run under it.
  6. ba_edge_kernel adding its clamped loads past the last chunk: 60 red / test_pack_tiles_with_ragged_last_tile red
     (3), the rest green: Gauss-Newton's fixed point does not move when M and g are scaled alike.
"""
import ctypes

import numpy as np
import pytest
import torch

import ba_edge_cases as B

pytestmark = pytest.mark.gpu


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _env(c, monkeypatch, fused="0"):
    if c["chunk_points"] is None:
        monkeypatch.delenv("M3S_BA_CHUNK_POINTS", raising=False)
    else:
        monkeypatch.setenv("M3S_BA_CHUNK_POINTS", str(c["chunk_points"]))
    monkeypatch.setenv("M3S_BA_FUSED_PACK", fused)


def _shard(c, mode, e0=0, e1=None, X=None, Cs=None, keyframes=None, cfg_mode=None, **kw):
    """A HipShard of the case: stacked (X, Cs; default the case's) or zero-copy (keyframes)."""
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config

    cfg = ba_config(cfg_mode or mode, B.local_opt(c, mode, config["local_opt"]), torch.from_numpy(c["K"]), c["H"], c["W"])
    if keyframes is None:
        X = _cuda(B.mode_X(c, mode)) if X is None else X
        Cs = _cuda(c["Cs"]) if Cs is None else Cs
    else:
        X = Cs = None
    sh = HipShard(cfg, _cuda(c["Twc"]), X, Cs, _cuda(c["ii"]), _cuda(c["jj"]), _cuda(c["idx"]),
                  _cuda(c["valid"], torch.bool), _cuda(c["Q"]), 0.0, e0, c["E"] if e1 is None else e1,
                  keyframes=keyframes, **kw)
    info = (ctypes.c_int * 13)()
    from m3s import _lib

    _lib.check(sh.lib.m3s_ba_plan_info(ctypes.byref(sh.plan), info))
    assert info[0] == c["chunks"], f"{c['name']}: {info[0]} linearisation chunks, the case is built for {c['chunks']}"
    return sh


def _rows(sh):
    sh.linearize()
    torch.cuda.synchronize()
    return sh.edge_sums.view(-1, 36).cpu().numpy().copy()


def _check(c, mode, rows, what=""):
    t, ref = B.truth(c, mode), B.rho_ref(c, mode)
    r = B.rho(rows, t)
    print(f"{c['name']} {mode}{what}: rho_ref {ref:.2e}, device rho per edge {' '.join(f'{v:.2e}' for v in r)} "
          f"(bound {4 * ref:.2e})")
    assert np.isfinite(rows[:, :35]).all()
    assert (r <= 4 * ref).all()


def _same(a, b):
    return np.array_equal(a[:, :35], b[:, :35])


@pytest.mark.parametrize("name,mode", B.case_modes(B.SHAPE_CASES))
def test_shapes_vs_fp64(name, mode, monkeypatch):
    """Every shape of the table in every mode: one partial round; every lane live; one second point; a
    missing last second point; a full round; a second round with one live lane; chunk starts off any power of two;
    chunks shorter than the block; two pack tiles and a ragged pack trip; one chunk of 65 rounds (the in-loop flush)."""
    c = B.build(name)
    _env(c, monkeypatch)
    _check(c, mode, _rows(_shard(c, mode)))


@pytest.mark.parametrize("name,mode", B.case_modes(B.THRESH_CASES + ["ids513"]))
def test_thresholds_and_ids_vs_fp64(name, mode, monkeypatch):
    """C_thresh = 0.5 with planted low confidences on either side of the edge; pixel_border = 2, planted depths and
    points behind the camera; a TUM-like K; keyframe ids {9, 2, 5} that are neither ranks nor in order of appearance."""
    c = B.build(name)
    _env(c, monkeypatch)
    _check(c, mode, _rows(_shard(c, mode)))


@pytest.mark.parametrize("mode", ["points", "rays"])
def test_zero_residual_vs_fp64(mode, monkeypatch):
    """Two identical keyframes, every pixel matched to itself: D = 0 and t = 0, every residual is exactly 0, Huber's
    quotient is rcp(0) * 0 = NaN and min(1, NaN) = 1. g is exactly 0.0, M finite and within the bound."""
    c = B.build("zero513")
    _env(c, monkeypatch)
    rows = _rows(_shard(c, mode))
    assert not rows[:, 28:35].any()
    assert (rows[:, B.DIAG] > 0).all()
    _check(c, mode, rows)


@pytest.mark.parametrize("name,mode", B.case_modes(B.BIT_CASES))
def test_fused_pack_and_relinearisation_are_bit_identical(name, mode, monkeypatch):
    """The pack fused into the first linearisation (ba_lin_kernel<PACK>, in order) == the separate pack, and a second
    linearize() on the same plan without a solve between (stored records, the pipelined loop) == the first, after
    either pack. The separate pack's rows are also checked against fp64."""
    c = B.build(name)
    out = {}
    for fused in ("0", "1"):
        _env(c, monkeypatch, fused)
        sh = _shard(c, mode)
        out[fused] = (_rows(sh), _rows(sh))
    _check(c, mode, out["0"][0])
    assert _same(out["0"][0], out["1"][0])
    assert _same(out["0"][0], out["0"][1]) and _same(out["1"][0], out["1"][1])


@pytest.mark.parametrize("name", B.BIT_CASES)
def test_calib_raw_is_bit_identical_to_calib_on_constrained_points(name, monkeypatch):
    """calib_raw on keyframe points moved off their pixel rays == calib on constrain_points_to_ray of them."""
    from m3s.geometry import constrain_points_to_ray

    c = B.build(name)
    _env(c, monkeypatch)
    gen = torch.Generator().manual_seed(17)
    raw = torch.from_numpy(c["X"]).clone()
    raw[..., :2] *= 1.0 + 0.05 * torch.randn(raw[..., :2].shape, generator=gen)
    raw = raw.cuda().contiguous()
    cons = constrain_points_to_ray((c["H"], c["W"]), raw, torch.from_numpy(c["K"]).cuda()).contiguous()
    assert float((raw - cons).abs().max()) > 1e-3    # the points did leave their rays
    a = _rows(_shard(c, "calib", X=cons))
    b = _rows(_shard(c, "calib", X=raw, cfg_mode="calib_raw"))
    assert np.abs(a[:, :35]).max() > 0 and _same(a, b)


@pytest.mark.parametrize("name,mode", B.case_modes(B.BIT_CASES))
def test_zero_copy_keyframes_are_bit_identical_to_stacked_averages(name, mode, monkeypatch):
    """Keyframes' own buffers with confidence sums and fusion counts (1, 3, 2) == the stacked average confidences: the
    confidence scale of either side decides points here (host test)."""
    c = B.build(name)
    _env(c, monkeypatch)
    X = _cuda(B.mode_X(c, mode))
    C_sum = [(_cuda(c["Cs"][k]) * float(n)).contiguous() for k, n in enumerate(B.NFUSE)]
    Cs = torch.stack([s / n for s, n in zip(C_sum, B.NFUSE)]).contiguous()
    a = _rows(_shard(c, mode, X=X, Cs=Cs))
    b = _rows(_shard(c, mode, keyframes=([X[k].contiguous() for k in range(3)], C_sum, list(B.NFUSE))))
    _check(c, mode, a, " (stacked averages)")
    assert _same(a, b)


@pytest.mark.parametrize("name,mode", B.case_modes(B.BIT_CASES))
def test_shard_ranges_are_bit_identical_and_zero_outside(name, mode, monkeypatch):
    c = B.build(name)
    _env(c, monkeypatch)
    full = _rows(_shard(c, mode))
    E = c["E"]
    for e0, e1 in ((0, 1), (1, E - 1), (E - 1, E)):
        part = _rows(_shard(c, mode, e0, e1))
        assert np.array_equal(part[e0:e1, :35], full[e0:e1, :35]), (e0, e1)
        outside = np.delete(part, np.arange(e0, e1), axis=0)
        assert not outside.any(), (e0, e1)


@pytest.mark.parametrize("name,mode", B.case_modes(B.BIT_CASES))
def test_record_cache_second_plan_packs_nothing_and_is_bit_identical(name, mode, monkeypatch):
    from m3s.dist_ba import RecordCache

    c = B.build(name)
    _env(c, monkeypatch)
    cache = RecordCache()
    uids = (np.arange(c["E"], dtype=np.int64), np.arange(c["Kp"], dtype=np.int64))
    try:
        first = _shard(c, mode, reuse=uids, cache=cache)
        a = _rows(first)
        assert first.reuse_info()[0] == c["E"]
        second = _shard(c, mode, reuse=uids, cache=cache)
        assert second.reuse_info() == (0, 0)
        b = _rows(second)
        del first, second
    finally:
        cache.release()
    assert np.abs(a[:, :35]).max() > 0 and _same(a, b)
