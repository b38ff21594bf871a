"""GPU: the two device solves of the BA pose system (csrc/ba_sparse.hip: assembly, launched wide steps, the
one-workgroup factor / back substitution / retraction kernel under the dataflow and the level-synchronous schedule;
csrc/ba_dense.hip: panel Cholesky with look-ahead and carried inverse rows) against LAPACK, on graphs chosen for the
shape of their factor: the kernels' control flow depends on that shape, not on the data.

The cases, the truth, the bound, the failure variants and the reach predicates are in tests/ba_solve_cases.py;
tests/test_ba_solve_host.py checks on the CPU that every case reaches what it is named for. A case needs no
linearisation: the test writes its own (E, 36) fp64 table into the shard's edge sums and solves. Which case reaches
which path, and the measured figures: DESIGN.md, BA, "solve edge shapes".

Bound (ba_solve_cases.bound): |dx_i - ref_i| <= 2^-24 |ref_i| + 4 cond(H) 2^-44 max|ref|, elementwise. Every test
prints the reached nL / nlev / wide_steps / dense and the worst error-to-bound ratio.

Mutation check (by hand, not committed; each run once, on the one test named):
  1. sp_rows_extra ``base + 64 < nrow`` for ``base < nrow``: test_sparse_schedules_vs_lapack[clique30] red.
  2. sp_back_column's dataflow branch ``b += 9`` for ``b += 18``: test_sparse_schedules_vs_lapack[clique30] red.
  3. m3s_launch_ba_solve_dense without the ``xr`` term of U: test_dense_solve_vs_lapack[dense65] red.
  4. ba_assemble_kernel without ``*a.bad = 0``: test_failure_is_a_silent_zero_step_and_does_not_stick[clique30-neg_leaf]
     red.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_solve_cases as C
import ba_solve_device as D
import oracle.oracle as O

pytestmark = pytest.mark.gpu

# M3S_BA_FLOW x M3S_BA_WIDE: dataflow flags / a barrier per level, crossed with the launch-cost split / every step a
# ba_sparse_step_kernel launch / every step inside the one-workgroup kernel
SCHEDULES = [(flow, wide) for flow in ("1", "0") for wide in (None, "0", "1000000")]


def _env(mp, solver, flow=None, wide=None):
    mp.setenv("M3S_BA_SOLVER", solver)
    for key, v in (("M3S_BA_FLOW", flow), ("M3S_BA_WIDE", wide)):
        if v is None:
            mp.delenv(key, raising=False)
        else:
            mp.setenv(key, v)


def _check_reach(name, solver, s):
    r = C.reach(name)
    want = {"nL": r["nL"], "nlev": r["nlev"], "dense": r["dense"][solver]}
    assert {k: s.info[k] for k in want} == want, f"{name} {solver}: plan {s.info}, the case is built for {want}"


def _check_solution(name, what, s, dx, variant=0):
    _, _, ref, cond = C.system(name, variant)
    assert dx.shape == ref.shape and np.isfinite(dx).all()
    ratio = C.error_ratio(dx, ref, cond)
    print(f"{name} {what}: nL {s.info['nL']} nlev {s.info['nlev']} wide_steps {s.info['wide_steps']} dense "
          f"{s.info['dense']}; cond {cond:.3g}, max|ref| {np.abs(ref).max():.3g}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def _check_retraction(s, dx, T, T_before=None):
    """Twc == pose_retr(Twc before, the device's dx) evaluated in fp64 and rounded to fp32, to the last place of fp32
    per component (the device retracts in fp64 from the fp32 dx it stored); the pinned pose bit-unchanged."""
    T_before = s.Twc0 if T_before is None else T_before
    ref = O.pose_retr_f64(T_before.astype(np.float64), dx.astype(np.float64).reshape(-1, 7)).astype(np.float32)
    assert np.array_equal(T[0], T_before[0])
    assert (np.abs(T.astype(np.float64) - ref.astype(np.float64)) <= C.ulp32(ref)).all()
    assert not np.array_equal(T[1:], T_before[1:])


@pytest.mark.parametrize("name", C.CASES)
def test_sparse_schedules_vs_lapack(name, monkeypatch):
    """The block-sparse solve of every case under every schedule: the plan reports the factor shape the case is built
    for, dx and Twc are bit-identical across the schedules, and (checked on the first) dx is LAPACK's within the bound
    and Twc the fp64 retraction of it."""
    out, wide = {}, {}
    for flow, w in SCHEDULES:
        _env(monkeypatch, "sparse", flow, w)
        s = D.Shard(*C.graph(name))
        _check_reach(name, "sparse", s)
        dx, T, it = s.solve(C.edge_sums(name))
        assert it == 1
        if not out:
            _check_solution(name, f"sparse flow {flow} wide {w}", s, dx)
            _check_retraction(s, dx, T)
        out[flow, w], wide[flow, w] = (dx, T), s.info["wide_steps"]
    dx0, T0 = out[SCHEDULES[0]]
    for key, (dx, T) in out.items():
        assert np.array_equal(dx, dx0) and np.array_equal(T, T0), key
    for flow in ("1", "0"):
        steps = [wide[flow, w] for w in (None, "0", "1000000")]
        same = [n for n, v in zip(("unset", "0", "1000000"), steps) if v == steps[0]]
        print(f"{name} flow {flow}: wide_steps {steps} for M3S_BA_WIDE unset, 0, 1000000"
              + (f"; {' and '.join(same)} gave the same split: one schedule, not two" if len(same) > 1 else ""))
    # every level launched / none: both ends of the split are run whatever the cost model picks
    for flow in ("1", "0"):
        assert wide[flow, "0"] == min(C.reach(name)["nlev"], 40) and wide[flow, "1000000"] == 0


@pytest.mark.parametrize("name", C.CASES)
def test_dense_solve_vs_lapack(name, monkeypatch):
    """The dense solve of every case (the structured ones too): panels of 64 columns with a ragged, a one-column, a
    63-column last panel, n a multiple of 64 (the update's tile row that holds only the rhs row), a single panel."""
    _env(monkeypatch, "dense")
    s = D.Shard(*C.graph(name))
    _check_reach(name, "dense", s)
    dx, T, it = s.solve(C.edge_sums(name))
    assert it == 1
    _check_solution(name, "dense", s, dx)
    _check_retraction(s, dx, T)


@pytest.mark.parametrize("variant", C.FAIL_VARIANTS)
@pytest.mark.parametrize("name", C.FAIL_CASES)
def test_failure_is_a_silent_zero_step_and_does_not_stick(name, variant, monkeypatch):
    """A non-positive (or NaN) pivot at the root column only, at a level-0 column, anywhere: dx = 0, the poses
    bit-unchanged, no stall reported (a wait abandoned because another wave failed is not one), the count advanced;
    and the next solve on the same plan, on the good table, is LAPACK's again. Sparse under the dataflow and the
    level-synchronous schedule, with every step launched (the failure is then reported through *a.bad), and dense."""
    bad, good = C.failing_table(name, variant), C.edge_sums(name)
    for solver, flow, w in (("sparse", "1", None), ("sparse", "0", None), ("sparse", "1", "0"), ("dense", None, None)):
        _env(monkeypatch, solver, flow, w)
        s = D.Shard(*C.graph(name))
        _check_reach(name, solver, s)
        dx, T, it = s.solve(bad)  # iterations() raises on M3S_ESTALL
        what = f"{variant} {solver} flow {flow} wide {w}"
        assert it == 1, what
        assert np.all(dx == 0.0), what
        assert np.array_equal(T, s.Twc0), what
        dx, T, it = s.solve(good)
        assert it == 2, what
        _check_solution(name, f"after {what}", s, dx)
        _check_retraction(s, dx, T)


@pytest.mark.parametrize("solver", C.SOLVERS)
def test_early_exit_freezes_the_plan(solver, monkeypatch):
    """|dx| below delta_thresh sets the plan's done flag: that step is still applied, and every kernel of a later solve
    returns at once, whatever its edge sums hold."""
    name = "dense11"
    _env(monkeypatch, solver)
    ref = C.system(name)[2]
    s = D.Shard(*C.graph(name), delta_thresh=2.0 * float(np.linalg.norm(ref)))
    dx1, T1, it = s.solve(C.edge_sums(name))
    assert it == 1
    _check_solution(name, f"{solver} early exit", s, dx1)
    _check_retraction(s, dx1, T1)
    other = C.edge_sums(name, 1)
    assert not np.allclose(C.system(name, 1)[2], ref, rtol=0.1)
    dx2, T2, it = s.solve(other)
    assert it == 1 and np.array_equal(dx2, dx1) and np.array_equal(T2, T1)


def test_keyframe_without_edges_is_a_zero_step(monkeypatch):
    """Five poses, edges on the ids {0, 1, 2, 4}. The rank remap (gn_kernels.cu:161-170: position among the sorted
    unique ids of ii and jj) knows four keyframes, so id 4 takes rank 3, the row of pose 3, and rank 4 has no edge:
    the system still has Kp - 1 = 4 block columns, one of them empty. The reference sizes its system by the unique ids
    and never meets this; its callers pass as many poses as ids. Pinned here as it is today: the empty diagonal block
    is a non-positive pivot, so the solve is the silent zero step and no pose moves, under either solver."""
    ii, jj = C._two_way([(0, 1), (1, 2), (2, 4)])
    es = C.random_table(len(ii), np.random.default_rng(3))
    for solver in C.SOLVERS:
        _env(monkeypatch, solver)
        s = D.Shard(ii, jj, 5)
        assert s.info["nL"] == 6 and s.info["nlev"] == 3  # an isolated column beside a chain of three
        dx, T, it = s.solve(es)
        assert it == 1 and dx.shape == (28,) and np.all(dx == 0.0) and np.array_equal(T, s.Twc0)


def test_xcd_affinity_off_is_bit_identical(tmp_path, monkeypatch):
    """M3S_BA_XCD0=0 (launched steps spread over every XCD instead of the blocks of XCD 0 alone): the library reads it
    once per process, so a child process (tests/ba_solve_device.py) solves every case with every step launched, and dx
    and Twc are bit-identical to this process's."""
    _env(monkeypatch, "sparse", "1", "0")
    env = dict(os.environ, M3S_BA_XCD0="0", OUT_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                           "ba_solve_device.py"), *C.CASES],
                       env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "BA_SOLVE_CHILD_OK" in r.stdout, r.stderr[-3000:]
    got = np.load(os.path.join(tmp_path, "solve.npz"))
    for name in C.CASES:
        s = D.Shard(*C.graph(name))
        dx, T, _ = s.solve(C.edge_sums(name))
        assert int(got[f"{name}_wide"]) == s.info["wide_steps"] > 0
        assert np.array_equal(got[f"{name}_dx"], dx) and np.array_equal(got[f"{name}_T"], T), name
