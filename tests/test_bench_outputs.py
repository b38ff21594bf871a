"""bench.py's plain run and --dump-outputs: a run without --full times only the tracking headline (every secondary
leg stays out of the line), --steps sets the number of timed steps, and --dump-outputs writes what the last timed step
returned as float32 / float64 .npy files within the 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_dump_outputs_budget_dtype_and_fixed_sample(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4000)  # 4000 B per array
    big = np.arange(3 * 5000, dtype=np.float32).reshape(5000, 3)  # 60000 B: cut to 333 rows
    arrays = {"big": big, "idx": np.arange(100, dtype=np.int64), "flag": np.array([True])}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in arrays) <= 3 * 4000 + 3 * 128  # + .npy headers
    assert got["big"].dtype == np.float32 and got["big"].shape == (333, 3)
    rows = (got["big"][:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(got["big"], big[rows])  # distinct rows of the input, in order
    assert got["idx"].dtype == np.float64 and np.array_equal(got["idx"], np.arange(100))
    assert got["flag"].dtype == np.float64 and got["flag"][0] == 1.0
    for n in arrays:  # the same sample in every run
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))


def test_zero_steps_is_refused(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
    assert not r.stdout.strip() and not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--ring", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["full"] is False
    assert rec["unit"] == "tracked frames/s" and rec["higher_is_better"] is True and rec["value"] > 0
    assert rec["ms_per_step"] == pytest.approx(1e3 / rec["value"], rel=1e-9)  # one rank: value = steps / elapsed
    # --steps really sets the timed loop's length: the model was asked for 3 pairs inside it (once per track()), and
    # the dumped frame is the last of warmup + steps frames (ids from 0)
    assert rec["config"]["timed_track_calls"] == 3
    assert np.load(out / "frame_id.npy").tolist() == [1 + 3 - 1]
    for leg in ("roofline", "peaks_measured", "cpu_baseline", "ba", "retrieval", "store", "configs"):
        assert rec[leg] is None, leg
    assert rec["kernels_us"] == {} and rec["kernels"] == {}
    N = 512 * 512
    shapes = {"T_WC": (1, 8), "new_kf": (1,), "frame_id": (1,), "kf_X_canon": (N, 3), "kf_C_avg": (N, 1), "frame_X_canon": (N, 3),
              "frame_C_avg": (N, 1), "Qkf": (N, 1), "Qff": (N, 1), "idx_f2k": (N,)}
    assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in shapes)
    total = 0
    for n, shape in shapes.items():
        a = np.load(out / f"{n}.npy")
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.shape == shape and np.isfinite(a).all(), n
    assert total <= 64 << 20
    idx = np.load(out / "idx_f2k.npy")
    assert idx.min() >= 0 and idx.max() < N and np.array_equal(idx, np.round(idx))
