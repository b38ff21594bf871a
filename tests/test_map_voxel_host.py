"""Host-side checks of the voxel-grid thinning of the map export (m3s.evaluate.voxel_select, the voxel_size keyword
of world_points_torch, the m3s_map_voxel ABI's argument checks): no GPU needed."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from m3s import _lib
from m3s.frame import Frame, Keyframes
from m3s.sim3 import Sim3


def test_voxel_select_hand_case():
    """Voxel size 0.5 (r = 2, exact). Rows by voxel:
    (0,0,0):   rows 0 (conf 2), 3 (conf 3), 5 (conf 3): the tie at 3 goes to the smaller row, 3
    (-1,0,0):  row 1 at x = -0.2: floor puts it next to, not into, the cell of x = 0.2 (row 0)
    (-1,-1,-1): rows 2 (conf 1), 6 (conf 1): tie, row 2
    (2,0,-3):  row 4 alone (x = 1.0 is the lower edge of cell 2, z = -1.5 that of cell -3)
    row 7 has a NaN, row 8 an Inf, row 9 lies beyond 2^20 cells: left out."""
    from m3s.evaluate import voxel_select

    pts = torch.tensor([[0.2, 0.1, 0.3],
                        [-0.2, 0.1, 0.3],
                        [-0.4, -0.1, -0.25],
                        [0.49, 0.0, 0.45],
                        [1.0, 0.25, -1.5],
                        [0.3, 0.3, 0.3],
                        [-0.01, -0.49, -0.5],
                        [float("nan"), 0.0, 0.0],
                        [0.0, float("inf"), 0.0],
                        [0.0, 0.0, 0.5 * 2.0 ** 20]])
    conf = torch.tensor([2.0, 5.0, 1.0, 3.0, 1.5, 3.0, 1.0, 9.0, 9.0, 9.0])
    keep = voxel_select(pts, conf, 0.5)
    assert keep.dtype == torch.int64 and keep.tolist() == [1, 2, 3, 4]
    # the last cell inside the range is kept, the first one outside is not; both ends
    edge = torch.tensor([[0.5 * (2.0 ** 20 - 1), 0.0, 0.0], [-0.5 * 2.0 ** 20, 0.0, 0.0],
                         [-0.5 * (2.0 ** 20 + 1), 0.0, 0.0]])
    assert voxel_select(edge, torch.ones(3), 0.5).tolist() == [0, 1]
    # a huge voxel merges everything of one sign pattern; the winner is the most confident row
    assert voxel_select(pts[:7].abs(), conf[:7], 100.0).tolist() == [1]
    # a tiny voxel keeps every row that has a cell
    assert voxel_select(pts[:7], conf[:7], 1e-3).tolist() == list(range(7))
    assert voxel_select(torch.zeros((0, 3)), torch.zeros(0), 0.5).tolist() == []
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            voxel_select(pts, conf, bad)


def cpu_keyframes(K=3, H=12, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    kfs = Keyframes()
    for k in range(K):
        T = torch.cat((torch.randn(3, generator=g), torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0),
                       torch.tensor([1.0 + 0.25 * k])))
        f = Frame(k, (H, W), T_WC=Sim3(T.view(1, 8)))
        f.X_canon = torch.randn(H * W, 3, generator=g)
        f.C = (1.0 + 2.0 * torch.rand(H * W, 1, generator=g)) * (k + 1)
        f.N = k + 1
        f.uimg = torch.rand(H, W, 3, generator=g)
        kfs.append(f)
    return kfs


@pytest.mark.parametrize("voxel_size", [1e-3, 0.5, 100.0])
def test_world_points_torch_voxel_is_voxel_select_of_its_rows(voxel_size):
    from m3s.evaluate import voxel_select, world_points, world_points_torch

    kfs = cpu_keyframes()
    thr = 1.5
    pts, cols, counts = world_points_torch(kfs, thr)
    conf = torch.cat([kfs[k].get_average_conf().reshape(-1)[kfs[k].get_average_conf().reshape(-1) > thr]
                      for k in range(3)])
    assert conf.numel() == pts.shape[0] > 100
    keep = voxel_select(pts, conf, voxel_size)
    assert 0 < keep.numel() <= pts.shape[0]
    if voxel_size == 0.5:
        assert keep.numel() < pts.shape[0]  # some rows do share a cell
    owner = torch.repeat_interleave(torch.arange(3), counts)
    vp, vc, vn = world_points_torch(kfs, thr, voxel_size=voxel_size)
    assert torch.equal(vp, pts[keep]) and torch.equal(vc, cols[keep])
    assert vn.dtype == torch.int64 and vn.tolist() == torch.bincount(owner[keep], minlength=3).tolist()
    # CPU keyframes: world_points is the torch formulation; the other keywords still hold
    wp, wc, wn = world_points(kfs, thr, colors=False, voxel_size=voxel_size)
    assert wc is None and torch.equal(wp, vp) and torch.equal(wn, vn)
    rec, rn = world_points_torch(kfs, thr, layout="ply", voxel_size=voxel_size)
    assert rec.shape == (keep.numel(), 15) and torch.equal(rn, vn)
    assert torch.equal(rec[:, :12].contiguous().view(torch.float32).reshape(-1, 3), vp) and torch.equal(rec[:, 12:], vc)
    # None is the unthinned export
    p0, c0, n0 = world_points_torch(kfs, thr, voxel_size=None)
    assert torch.equal(p0, pts) and torch.equal(c0, cols) and torch.equal(n0, counts)


def test_world_points_torch_voxel_warns_once_about_dropped_rows(tmp_path):
    from m3s.evaluate import save_reconstruction, world_points_torch

    kfs = cpu_keyframes()
    valid = torch.nonzero(kfs[1].get_average_conf().reshape(-1) > 1.5).flatten()
    kfs[1].X_canon[valid[:3], 0] = float("nan")
    kfs[1].X_canon[valid[3], 2] = float("inf")
    base, _, _ = world_points_torch(kfs, 1.5)
    with pytest.warns(RuntimeWarning, match=r"\b4 rows") as rec:
        pts, _, counts = world_points_torch(kfs, 1.5, voxel_size=1e-3)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert pts.shape[0] == base.shape[0] - 4 == int(counts.sum()) and bool(torch.isfinite(pts).all())
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        world_points_torch(cpu_keyframes(), 1.5, voxel_size=0.5)  # nothing dropped: no warning
    with pytest.warns(RuntimeWarning):
        save_reconstruction(tmp_path, "thin.ply", kfs, 1.5, voxel_size=1e-3)
    raw = open(tmp_path / "thin.ply", "rb").read()
    assert f"element vertex {pts.shape[0]}\n".encode() in raw
    assert len(raw) - (raw.index(b"end_header\n") + 11) == 15 * pts.shape[0]


def _lib_host():
    return _lib.load(require_gpu=False)


def test_voxel_symbols_and_table_size():
    from m3s.evaluate import map_voxel, map_voxel_table_size  # noqa: F401  the thin wrappers exist

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("m3s_map_voxel", "m3s_map_voxel_table_size"):
        assert hasattr(raw, name) and name in _lib.EXPORTED
    size = _lib_host().m3s_map_voxel_table_size
    assert size(-1) == 0 and size(-2 ** 62) == 0 and size(2 ** 62) == 0  # negative, overflowing
    assert size(0) == size(1) == size(512) == 1024 * 16  # the minimum
    assert size(513) == 2048 * 16
    for total in (0, 1, 511, 512, 513, 3703, 65536, 65537, 44_400_000, 2 ** 31, 2 ** 32 - 1):
        b = size(total)
        slots = b // 16
        assert b % 16 == 0 and slots & (slots - 1) == 0 and slots >= max(1024, 2 * total) and slots < max(2048, 4 * total)
        assert map_voxel_table_size(total) == b
    assert size(44_400_000) == 2 ** 27 * 16  # the README's 256-keyframe cloud: 2 GiB


def _fake_table(Kp):
    fake = (ctypes.c_void_p * Kp)(*([0x1000] * Kp))
    return _lib.BaKeyframes(fake, fake, (ctypes.c_float * Kp)(*([1.0] * Kp)))


def _voxel(lib, mc, table, Kp, N, ws_bytes, voxel_size=0.5, vox_table=0x1000, Twc=0x1000):
    total, dropped = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = lib.m3s_map_voxel(mc, None if table is None else ctypes.byref(table), ctypes.c_void_p(Twc), Kp, N, voxel_size,
                           ctypes.c_void_p(vox_table), 1 << 20, None, ctypes.byref(total), ctypes.byref(dropped),
                           ctypes.c_void_p(0x1000), ws_bytes, None)
    assert total.value == -7 and dropped.value == -7
    return rc


def test_voxel_argument_errors_need_no_device():
    """Every one of these returns before the library touches HIP (the pointers are never dereferenced)."""
    lib = _lib_host()
    Kp, N = 3, 48 * 64
    table = _fake_table(Kp)
    big = lib.m3s_map_workspace_size(Kp, N)
    good = _lib.MapConfig(calib=1, fx=1, fy=1, cx=0, cy=0, height=48, width=64, c_conf_threshold=1.5, layout=1)
    ok = ctypes.byref(good)
    # the checks shared with the count and the write
    assert _voxel(lib, None, table, Kp, N, big) == _lib.EINVAL  # null config
    assert b"config" in lib.m3s_last_error()
    mc = _lib.MapConfig(calib=0, c_conf_threshold=1.5, layout=2)
    assert _voxel(lib, ctypes.byref(mc), table, Kp, N, big) == _lib.EINVAL  # bad layout
    mc = _lib.MapConfig(calib=1, fx=1, fy=1, cx=0, cy=0, height=48, width=63, c_conf_threshold=1.5, layout=0)
    assert _voxel(lib, ctypes.byref(mc), table, Kp, N, big) == _lib.EINVAL  # N != height * width
    assert _voxel(lib, ok, table, Kp, N, big - 1) == _lib.ESPACE  # short workspace
    assert _voxel(lib, ok, table, 0, N, big) == _lib.EINVAL
    assert _voxel(lib, ok, None, Kp, N, big) == _lib.EINVAL  # null keyframe table
    # its own
    for bad in (0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        assert _voxel(lib, ok, table, Kp, N, big, voxel_size=bad) == _lib.EINVAL
        assert b"voxel_size" in lib.m3s_last_error()
    assert _voxel(lib, ok, table, Kp, N, big, vox_table=0) == _lib.EINVAL  # null table
    assert b"table" in lib.m3s_last_error()
    assert _voxel(lib, ok, table, Kp, N, big, Twc=0) == _lib.EINVAL  # null poses
    # Kp N = 2^32: global row indices no longer fit 32 bits
    Kp2, N2 = 16, 1 << 28
    mc = _lib.MapConfig(calib=0, c_conf_threshold=1.5, layout=0)
    big2 = lib.m3s_map_workspace_size(Kp2, N2)
    assert big2 > 0
    assert _voxel(lib, ctypes.byref(mc), _fake_table(Kp2), Kp2, N2, big2) == _lib.EINVAL
    assert b"2^32" in lib.m3s_last_error()
    bad_n = _lib.BaKeyframes(table.X, table.C, (ctypes.c_float * Kp)(1.0, 0.0, 1.0))
    assert _voxel(lib, ok, bad_n, Kp, N, big) == _lib.EINVAL  # fusion count 0
