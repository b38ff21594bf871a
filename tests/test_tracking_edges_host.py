"""The tracking edge cases themselves, on the fp64 reference alone (no device): the conditions that keep
tests/test_gpu_tracking_edges.py from passing vacuously. For every case of tests/track_edge_cases.py:

* the reference is finite and its Cholesky factorisation succeeds;
* at the starting pose every planted class (points with valid false; calib: behind the camera, outside the border,
  invalid keyframe measurement) and both Huber branches count at least max(2, N / 50) points / whitened rows;
* matched cases: duplicates among the valid matches, a mark in the last partial 16-byte map entry, and
  n_valid_opt < n_valid_kf < N (both confidence thresholds bite);
* conditioning: scaling the points elementwise by 1 +- 2^-24 moves the reference's pose by at most 1e-6, so the
  1e-5 pose contract is a statement about the kernels and not about the inputs' rounding;
* float32 normal equations: the first-order bound of one float32 rounding of H and g on a GN step
  (``solve_rounding``) stays below a third of the contract. The kernels form H and g from float32 products and solve
  the 7x7 system in float32 by design, so beyond that a case would measure its own conditioning;
* the cases run to convergence keep the margin of ``margin_ok`` at every step.
"""
import numpy as np
import pytest

import track_edge_cases as E
from track_chain import oracle_track_from_matches

DIRECT = [pytest.param(m, n, s, id=f"{m}-{n}") for m, n, s in E.direct_cases()]
MATCHED = [pytest.param(m, s, id=f"{m}-{s[0]}x{s[1]}") for m, s in E.MATCHED]


def _report(kind, mode, H, W, seed, converge):
    bad = E.case_problems(kind, mode, H, W, seed, converge)
    assert not bad, f"{kind} {mode} {H}x{W} seed {seed}: {bad}"


@pytest.mark.parametrize("mode,N,shape", DIRECT)
def test_direct_case_reaches_its_branches(mode, N, shape):
    c = E.build_direct(mode, *shape, E.seed_of("direct", mode, N))
    _, _, it, trace = E.ref_direct_cached(mode, *shape, E.seed_of("direct", mode, N), 3 if N in E.BIG else 4)
    print(f"direct {mode} N={N}: {E.populations(mode, trace)}, conditioning {E.conditioning('direct', c):.1e}")
    _report("direct", mode, *shape, E.seed_of("direct", mode, N), False)
    if N in E.CONVERGE_N:
        _report("direct", mode, *shape, E.seed_of("direct", mode, N), True)


@pytest.mark.parametrize("mode,shape", MATCHED)
def test_matched_case_reaches_its_branches(mode, shape):
    N = shape[0] * shape[1]
    seed = E.seed_of("matched", mode, N)
    c = E.build_matched(mode, *shape, seed)
    r, trace = E.ref_matched_cached(mode, *shape, seed, 3 if N in E.BIG else None)
    print(f"matched {mode} {shape}: {r['status']} in {r['iters']}, opt/kf/unique/matches {r['n_valid_opt']} "
          f"{r['n_valid_kf']} {r['n_unique']} {int(c['valid_match'].sum())}, {E.populations(mode, trace)}")
    _report("matched", mode, *shape, seed, N not in E.BIG)
    # every threshold quantity at least 1 % away from its threshold
    assert (np.abs(r["Qk"] / np.float32(1.5) - 1) >= 0.0099).all()
    for C, n in ((c["kf_C"], c["kf_N"]), (c["Cff"], 1)):
        assert (np.abs(C / np.float32(n) / np.float32(0.5) - 1) >= 0.0099).all()
    assert ((C / np.float32(n) > 0.5).any() and (C / np.float32(n) < 0.5).any())
    assert (r["Qk"] > 1.5).any() and (r["Qk"] < 1.5).any()
    for k in ("outlier", "behind", "invalid_meas", "last_entry", "dup"):
        assert c["planted"][k].size >= 2, k


def test_skip_boundary_case():
    """52 of 1025 valid-opt points (0.0507) are tracked and solve, 51 (0.0498) are skipped; the skipped frame still
    has hundreds of valid matches, which mark the unique-match map."""
    a, b = E.ref_matched(E.skip_case(52)), E.ref_matched(E.skip_case(51))
    assert a["n_valid_opt"] == 52 and a["status"] == "ok" and np.isfinite(a["T_WCf"]).all()
    assert b["n_valid_opt"] == 51 and b["status"] == "skipped" and b["T_WCf"] is None
    assert b["n_unique"] > 300 and np.array_equal(b["X"], E.skip_case(51)["kf_X"].astype(np.float64))


def test_trace_changes_nothing():
    """The trace argument only records: same pose and iterations with and without it, fixed or to convergence."""
    for mode, shape in (("rays", (1, 259)), ("calib", (7, 37))):
        c = E.build_direct(mode, *shape, 1)
        for kw in ({}, {"fixed_iters": 2}):
            tr = []
            a, b = E.ref_direct(c, **kw), E.ref_direct(c, trace=tr, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(tr) == b[2]
            assert set(tr[0]) >= {"cost", "tau_norm", "rel", "huber_active", "huber_inactive", "n_invalid"}
            if mode == "calib":
                assert set(tr[0]) >= {"n_behind", "n_border", "n_invalid_meas"}
            assert np.isnan(tr[0]["rel"]) and all(np.isfinite(t["rel"]) for t in tr[1:])


def test_from_matches_statuses():
    """oracle_track_from_matches: max_iters without convergence, and a Cholesky failure caught."""
    c = E.build_matched("rays", 15, 17, 1)
    r = E.ref_matched(c, fixed_iters=1, rel_error=0.0, delta_norm=0.0)
    assert r["status"] == "max_iters" and r["iters"] == 1
    args = [c[k] for k in ("idx", "valid_match", "Xff", "Cff", "Qff", "Xkf", "Ckf", "Qkf", "kf_X", "kf_C", "kf_N")]
    r = oracle_track_from_matches("rays", *args, c["T_WCf"], c["T_WCk"], c["K"], (15, 17), Q_conf=1e9,
                                  min_match_frac=0.0)
    assert r["status"] == "cholesky" and r["n_valid_opt"] == 0
