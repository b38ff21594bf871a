"""Host-side checks of the map / trajectory export (m3s.evaluate, the m3s_map_* ABI): no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from m3s import _lib
from m3s.config import config
from m3s.frame import Frame, Keyframes
from m3s.sim3 import Sim3

PLY_BODY = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])


def read_ply(path):
    """Numpy reader of a binary little-endian PLY with the six vertex properties: (xyz (M,3) f32, rgb (M,3) u8)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert lines[2].startswith("element vertex ")
    m = int(lines[2].split()[2])
    assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar red",
                         "property uchar green", "property uchar blue", "end_header"]
    assert PLY_BODY.itemsize == 15 and len(raw) - end == 15 * m
    body = np.frombuffer(raw[end:], dtype=PLY_BODY)
    return np.stack([body["x"], body["y"], body["z"]], axis=1), np.stack([body["r"], body["g"], body["b"]], axis=1)


def two_keyframes():
    """Two 4x4 keyframes with integer points and poses whose action is exact in fp32:
    keyframe 0: scale 2, no rotation, t = (1, 2, 3); N = 1.
    keyframe 1: half turn about z (q = (0, 0, 1, 0): (x, y, z) -> (-x, -y, z)), scale 0.5, t = (0, 0, 1); N = 2."""
    n = torch.arange(16, dtype=torch.float32)
    X0 = torch.stack((n, 2 * n, n + 1), dim=1)
    X1 = torch.stack((4 * n, -2 * n, 8 + 2 * n), dim=1)
    C0 = torch.full((16, 1), 1.0)
    C0[[1, 5, 15]] = torch.tensor([[2.0], [1.75], [9.0]])  # avg = C: pixels 1, 5, 15 pass 1.5
    C0[7] = 1.5  # equal to the threshold: dropped
    C1 = torch.full((16, 1), 3.0)  # N = 2: avg 1.5, dropped
    C1[[0, 6]] = torch.tensor([[3.5], [8.0]])  # avg 1.75, 4: kept
    C1[9] = float("nan")
    f0 = Frame(0, (4, 4), T_WC=Sim3(torch.tensor([[1.0, 2, 3, 0, 0, 0, 1, 2]])))
    f0.X_canon, f0.C, f0.N = X0, C0, 1
    f1 = Frame(1, (4, 4), T_WC=Sim3(torch.tensor([[0.0, 0, 1, 0, 0, 1, 0, 0.5]])))
    f1.X_canon, f1.C, f1.N = X1, C1, 2
    u = torch.arange(16 * 3, dtype=torch.float32).reshape(4, 4, 3)
    f0.uimg = u / 255.0 + 0.002  # (uimg * 255) truncates back to 0..47
    f1.uimg = (u + 100) / 255.0 + 0.002
    kfs = Keyframes()
    kfs.append(f0)
    kfs.append(f1)
    return kfs


# by hand: keyframe 0 keeps n = 1, 5, 15 -> 2 (n, 2n, n+1) + (1, 2, 3); keyframe 1 keeps n = 0, 6 ->
# 0.5 (-4n, 2n, 8 + 2n) + (0, 0, 1)
EXPECT_XYZ = np.array([[3, 6, 7], [11, 22, 15], [31, 62, 35], [0, 0, 5], [-12, 6, 11]], dtype=np.float32)
EXPECT_RGB = np.array([[3, 4, 5], [15, 16, 17], [45, 46, 47], [100, 101, 102], [118, 119, 120]], dtype=np.uint8)


def test_world_points_torch_hand_case():
    from m3s.evaluate import world_points_torch

    kfs = two_keyframes()
    pts, cols, counts = world_points_torch(kfs, 1.5)
    assert pts.dtype == torch.float32 and cols.dtype == torch.uint8 and counts.dtype == torch.int64
    assert np.array_equal(pts.numpy(), EXPECT_XYZ)
    assert np.array_equal(cols.numpy(), EXPECT_RGB)
    assert counts.tolist() == [3, 2]
    # indices select and order; colors=False
    pts, cols, counts = world_points_torch(kfs, 1.5, indices=[1, 0], colors=False)
    assert cols is None and counts.tolist() == [2, 3]
    assert np.array_equal(pts.numpy(), np.concatenate([EXPECT_XYZ[3:], EXPECT_XYZ[:3]]))
    # the PLY layout is the same rows packed to 15-byte records
    rec, counts = world_points_torch(kfs, 1.5, layout="ply")
    assert rec.shape == (5, 15) and rec.dtype == torch.uint8
    body = np.frombuffer(rec.numpy().tobytes(), dtype=PLY_BODY)
    assert np.array_equal(np.stack([body["x"], body["y"], body["z"]], 1), EXPECT_XYZ)
    assert np.array_equal(np.stack([body["r"], body["g"], body["b"]], 1), EXPECT_RGB)


def test_world_points_torch_calib_hand_case():
    """use_calib: the point at its own depth on its pixel's ray. K = [[2,0,1],[0,2,1],[0,0,1]] keeps it exact:
    pixel (u, v) at depth z -> (z (u - 1) / 2, z (v - 1) / 2, z)."""
    from m3s.evaluate import world_points

    kfs = two_keyframes()
    config["use_calib"] = True
    K = torch.tensor([[2.0, 0, 1], [0, 2.0, 1], [0, 0, 1]])
    for i in range(2):
        kfs[i].K = K
    X_before = kfs[0].X_canon.clone()
    pts, _, counts = world_points(kfs, 1.5, indices=[0])  # CPU keyframes: the torch formulation
    assert counts.tolist() == [3]
    exp = []
    for n in (1, 5, 15):
        u, v, z = n % 4, n // 4, n + 1.0
        exp.append([2 * (z * (u - 1) / 2) + 1, 2 * (z * (v - 1) / 2) + 2, 2 * z + 3])
    assert np.array_equal(pts.numpy(), np.array(exp, dtype=np.float32))
    assert torch.equal(kfs[0].X_canon, X_before)  # the keyframes are not overwritten


def test_save_ply_and_reconstruction_roundtrip(tmp_path):
    from m3s.evaluate import save_ply, save_reconstruction, world_points

    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    save_ply(tmp_path / "a.ply", xyz, rgb)
    got_xyz, got_rgb = read_ply(tmp_path / "a.ply")
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_rgb, rgb)
    save_ply(tmp_path / "b.ply", torch.from_numpy(xyz), torch.from_numpy(rgb))
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()

    kfs = two_keyframes()
    save_reconstruction(tmp_path / "out", "map.ply", kfs, 1.5)
    got_xyz, got_rgb = read_ply(tmp_path / "out" / "map.ply")
    assert np.array_equal(got_xyz, EXPECT_XYZ) and np.array_equal(got_rgb, EXPECT_RGB)
    pts, cols, _ = world_points(kfs, 1.5)
    assert np.array_equal(pts.numpy(), got_xyz) and np.array_equal(cols.numpy(), got_rgb)
    # an empty cloud is still a valid file
    save_reconstruction(tmp_path / "out", "empty.ply", kfs, 100.0)
    got_xyz, got_rgb = read_ply(tmp_path / "out" / "empty.ply")
    assert got_xyz.shape == (0, 3) and got_rgb.shape == (0, 3)


def test_save_traj_line_format(tmp_path):
    from m3s.evaluate import save_traj

    kfs = two_keyframes()
    stamps = {0: 12.5, 1: "1305031102.175304"}
    save_traj(tmp_path / "logs", "traj.txt", stamps, kfs)
    lines = open(tmp_path / "logs" / "traj.txt").read().splitlines()
    assert lines == ["12.5 1.0 2.0 3.0 0.0 0.0 0.0 1.0", "1305031102.175304 0.0 0.0 1.0 0.0 0.0 1.0 0.0"]
    with pytest.raises(NotImplementedError):
        save_traj(tmp_path / "logs", "traj2.txt", stamps, kfs, intrinsics=object())


def _lib_host():
    return _lib.load(require_gpu=False)


def test_map_symbols_and_workspace_size():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("m3s_map_workspace_size", "m3s_map_count", "m3s_map_write"):
        assert hasattr(lib, name) and name in _lib.EXPORTED
    lib = _lib_host()
    size = lib.m3s_map_workspace_size
    assert size(0, 100) == 0 and size(4, 0) == 0
    prev = 0
    for Kp in (1, 2, 7, 64, 256):
        s = size(Kp, 3072)
        assert s >= prev and s > 0
        prev = s
    prev = 0
    for N in (1, 63, 384, 1024, 1025, 3072, 196608):
        s = size(3, N)
        assert s >= prev and s > 0
        prev = s
    # at least the validity bits, the block offsets and the pointer tables
    assert size(256, 196608) >= 256 * 196608 // 8 + 256 * 192 * 12


def _fake_table(Kp):
    fake = (ctypes.c_void_p * Kp)(*([0x1000] * Kp))
    return _lib.BaKeyframes(fake, fake, (ctypes.c_float * Kp)(*([1.0] * Kp)))


def _count(lib, mc, table, Kp, N, ws_bytes):
    total = ctypes.c_int64(-7)
    rc = lib.m3s_map_count(mc, None if table is None else ctypes.byref(table), Kp, N, None, ctypes.byref(total),
                           ctypes.c_void_p(0x1000), ws_bytes, None)
    assert total.value == -7
    return rc


def _write(lib, mc, table, Kp, N, ws_bytes):
    return lib.m3s_map_write(mc, None if table is None else ctypes.byref(table), ctypes.c_void_p(0x1000), None, Kp, N,
                             ctypes.c_void_p(0x1000), None, 1 << 20, ctypes.c_void_p(0x1000), ws_bytes, None)


def test_map_argument_errors_need_no_device():
    """Every one of these returns before the library touches HIP (the pointers are never dereferenced)."""
    lib = _lib_host()
    Kp, N = 3, 48 * 64
    table = _fake_table(Kp)
    big = lib.m3s_map_workspace_size(Kp, N)
    for call in (_count, _write):
        assert call(lib, None, table, Kp, N, big) == _lib.EINVAL  # null config
        assert b"config" in lib.m3s_last_error()
        mc = _lib.MapConfig(calib=0, c_conf_threshold=1.5, layout=2)
        assert call(lib, ctypes.byref(mc), table, Kp, N, big) == _lib.EINVAL  # bad layout
        assert b"layout" in lib.m3s_last_error()
        mc = _lib.MapConfig(calib=1, fx=1, fy=1, cx=0, cy=0, height=48, width=63, c_conf_threshold=1.5, layout=0)
        assert call(lib, ctypes.byref(mc), table, Kp, N, big) == _lib.EINVAL  # N != height * width
        mc = _lib.MapConfig(calib=1, fx=1, fy=1, cx=0, cy=0, height=1, width=65536, c_conf_threshold=1.5, layout=1)
        assert call(lib, ctypes.byref(mc), table, Kp, 65536, lib.m3s_map_workspace_size(Kp, 65536)) == _lib.EINVAL
        mc = _lib.MapConfig(calib=1, fx=1, fy=1, cx=0, cy=0, height=48, width=64, c_conf_threshold=1.5, layout=1)
        assert call(lib, ctypes.byref(mc), table, Kp, N, big - 1) == _lib.ESPACE  # short workspace
        assert call(lib, ctypes.byref(mc), table, 0, N, big) == _lib.EINVAL
        assert call(lib, ctypes.byref(mc), None, Kp, N, big) == _lib.EINVAL  # null keyframe table
