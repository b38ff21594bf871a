"""Map and trajectory export (the reference's ``mast3r_slam/evaluate.py:23-106``).

``world_points`` is the confidence-filtered world point cloud of the keyframes: the cloud the reference saves at
the end of a run (``evaluate.save_reconstruction``, ``main.py:370-376``) and its viewer shows live
(``visualization.py:38,351``). The reference loops over the keyframes on the host (a constrained copy in calib mode,
``T_WC.act``, three ``.cpu().numpy()`` copies, a boolean index and a final concatenate). Here the keyframes' own
device buffers are read in place by two HIP passes (csrc/map.hip: ``m3s_map_count`` stores one validity bit per point
and scans the block counts, ``m3s_map_write`` transforms and compacts in keyframe order and pixel order), so only the
poses (K x 8 floats) and the colours (3 B per pixel, the host ``uimg``) are gathered. ``voxel_size`` adds one stage
between the passes (``m3s_map_voxel``) that thins the cloud to one row per occupied voxel; ``voxel_select`` states its
rule in torch ops.

``world_points_torch`` is the same contract in plain torch ops, the reference's formulation on
``m3s.geometry.constrain_points_to_ray`` and ``Sim3.act``; it runs on any device and is what ``world_points`` falls
back to for keyframes whose buffers the kernels cannot read in place (not on a HIP device, not contiguous fp32,
differing sizes).
"""
import ctypes
import pathlib
import warnings

import numpy as np
import torch

from m3s import _lib
from m3s.config import config
from m3s.geometry import constrain_points_to_ray
from m3s.sim3 import as_SE3
from m3s.tracker import frame_img_size

_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_LAYOUTS = {"soa": _lib.MAP_SOA, "ply": _lib.MAP_PLY}


def _select(keyframes, indices):
    idx = range(len(keyframes)) if indices is None else [int(i) for i in indices]
    return [keyframes[i] for i in idx]


def _intrinsics(keyframes, frames):
    """(use_calib, K or None): K from the store (``SharedKeyframes.K``) or the first frame."""
    if not config["use_calib"]:
        return False, None
    K = getattr(keyframes, "K", None)
    if not torch.is_tensor(K):
        K = frames[0].K
    if K is None:
        raise ValueError("world_points: use_calib is set but neither the keyframe store nor the frame carries K")
    return True, K


def _colors_u8(frame):
    """evaluate.py:60: (uimg * 255) truncated to u8, (N,3)."""
    if frame.uimg is None:
        raise ValueError("world_points: colors=True needs uimg on every keyframe")
    return (frame.uimg * 255).to(torch.uint8).reshape(-1, 3)


def _pack_ply(points, colors):
    """(M,3) f32 + (M,3) u8 or None -> (M,15) u8 vertex records (x, y, z little-endian f32, r, g, b)."""
    xyz = points.contiguous().view(torch.uint8).reshape(-1, 12)
    rgb = colors if colors is not None else torch.zeros((xyz.shape[0], 3), dtype=torch.uint8, device=xyz.device)
    return torch.cat((xyz, rgb), dim=1)


_VOXEL_RANGE = float(1 << 20)  # voxel coordinates lie in [-2^20, 2^20): csrc/m3s_map.h MAP_VOX_RANGE


def _voxel_scale(voxel_size):
    """float32(1) / float32(voxel_size), the one factor both paths multiply by."""
    v = np.float32(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"voxel_size must be finite and positive, not {voxel_size!r}")
    return float(np.float32(1) / v)


def _voxel_pick(points, conf, voxel_size):
    """``voxel_select`` and the number of rows that reached no voxel."""
    points, conf = points.reshape(-1, 3), conf.reshape(-1)
    r = torch.tensor(_voxel_scale(voxel_size), dtype=torch.float32, device=points.device)
    q = torch.floor(points.to(torch.float32) * r)  # one fp32 multiply, one floor
    ok = torch.isfinite(points).all(dim=1) & ((q >= -_VOXEL_RANGE) & (q < _VOXEL_RANGE)).all(dim=1)
    rows = torch.nonzero(ok).flatten()
    b = q[rows].to(torch.int64) + (1 << 20)  # 21 biased bits per coordinate
    _, voxel = torch.unique((b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2], return_inverse=True)
    # lexicographic pick by stable sorts, last key first: voxel, then confidence descending, then row ascending
    by_conf = torch.sort(conf[rows], descending=True, stable=True).indices
    order = by_conf[torch.sort(voxel[by_conf], stable=True).indices]
    v = voxel[order]
    first = torch.ones_like(v, dtype=torch.bool)
    first[1:] = v[1:] != v[:-1]
    return torch.sort(rows[order[first]]).values, int(points.shape[0] - rows.numel())


def voxel_select(points, conf, voxel_size):
    """The voxel-grid thinning rule of the map export, in plain torch ops on any device: the reference for
    ``m3s_map_voxel``. ``points`` (M,3) f32 world points, ``conf`` (M) their average confidences. Returns the kept row
    indices (int64, ascending).

    With ``r = float32(1) / float32(voxel_size)`` the voxel of a row is ``floor(points * r)`` per coordinate (one fp32
    multiply, one floor). A row with a non-finite coordinate, or a voxel coordinate outside ``[-2^20, 2^20)``, is
    left out. Per occupied voxel one row is kept: the largest confidence, among equal confidences the smallest row
    index. The rows themselves are kept (no centroid), so the result is exact and reproducible."""
    return _voxel_pick(points, conf, voxel_size)[0]


def _warn_dropped(dropped):
    if dropped:
        warnings.warn(f"world_points: {int(dropped)} rows dropped by the voxel grid (not finite, or outside 2^20 "
                      "voxels of the origin)", RuntimeWarning, stacklevel=3)


def world_points_torch(keyframes, c_conf_threshold, indices=None, colors=True, layout="soa", voxel_size=None):
    """``world_points`` in plain torch ops on the keyframes' device (evaluate.py:50-68 per keyframe, concatenated
    there instead of on the host); with ``voxel_size`` its rows are thinned by ``voxel_select``."""
    if layout not in _LAYOUTS:
        raise ValueError(f"world_points: layout must be 'soa' or 'ply', not {layout!r}")
    if voxel_size is not None:
        _voxel_scale(voxel_size)
    frames = _select(keyframes, indices)
    dev = frames[0].X_canon.device if frames else torch.device("cpu")
    use_calib, K = _intrinsics(keyframes, frames) if frames else (False, None)
    pts, cols, counts = [torch.zeros((0, 3), dtype=torch.float32, device=dev)], [], []
    confs = [torch.zeros((0,), dtype=torch.float32, device=dev)]
    for kf in frames:
        X = kf.X_canon.reshape(-1, 3)
        if use_calib:
            X = constrain_points_to_ray(frame_img_size(kf), X[None], K.to(X.device))[0]
        pW = kf.T_WC.to(X.device).act(X).reshape(-1, 3)
        conf = kf.get_average_conf().reshape(-1)
        valid = conf > c_conf_threshold
        pts.append(pW[valid])
        confs.append(conf[valid].to(dev, torch.float32))
        counts.append(int(valid.sum()))
        if colors:
            cols.append(_colors_u8(kf).to(dev)[valid])
    points = torch.cat(pts, dim=0)
    cols_t = torch.cat([torch.zeros((0, 3), dtype=torch.uint8, device=dev)] + cols, dim=0) if colors else None
    counts_t = torch.tensor(counts, dtype=torch.int64, device=dev)
    if voxel_size is not None:
        keep, dropped = _voxel_pick(points, torch.cat(confs), voxel_size)
        owner = torch.repeat_interleave(torch.arange(len(frames), device=dev), counts_t)
        counts_t = torch.bincount(owner[keep], minlength=len(frames))
        points = points[keep]
        cols_t = cols_t[keep] if colors else None
        _warn_dropped(dropped)
    if layout == "ply":
        return _pack_ply(points, cols_t), counts_t
    return points, cols_t, counts_t


def _in_place_ok(frames):
    X0 = frames[0].X_canon
    for kf in frames:
        x, c = kf.X_canon, kf.C
        if not (torch.is_tensor(x) and torch.is_tensor(c) and x.is_cuda and c.is_cuda and x.device == X0.device and
                c.device == X0.device and x.dtype == torch.float32 and c.dtype == torch.float32 and
                x.is_contiguous() and c.is_contiguous() and x.numel() == X0.numel() and c.numel() * 3 == x.numel()):
            return False
        if kf.N <= 0:
            return False
    return True


def keyframe_table(X_list, C_list, N_list):
    """The ``m3s_ba_keyframes`` pointer table of device tensors X (N,3), C (N) and fusion counts N."""
    Kp = len(X_list)
    return _lib.BaKeyframes((ctypes.c_void_p * Kp)(*[x.data_ptr() for x in X_list]),
                            (ctypes.c_void_p * Kp)(*[c.data_ptr() for c in C_list]),
                            (ctypes.c_float * Kp)(*[float(n) for n in N_list]))


def map_config(c_conf_threshold, layout="soa", K=None, img_size=None):
    """``m3s_map_config``; calib mode iff K (3,3) is given, with the pointmap size ``img_size`` = (H, W)."""
    mc = _lib.MapConfig()
    mc.c_conf_threshold = float(c_conf_threshold)
    mc.layout = _LAYOUTS[layout]
    mc.calib = 0
    if K is not None:
        Kh = K.detach().to("cpu", torch.float32)
        mc.calib = 1
        mc.fx, mc.fy, mc.cx, mc.cy = float(Kh[0, 0]), float(Kh[1, 1]), float(Kh[0, 2]), float(Kh[1, 2])
        mc.height, mc.width = int(img_size[0]), int(img_size[1])
    return mc


def map_count(mc, table, Kp, N, ws, device):
    """``m3s_map_count`` on torch's current stream: (rows per keyframe (Kp,) int64 numpy, total)."""
    lib = _lib.load()
    counts = (ctypes.c_int64 * Kp)()
    total = ctypes.c_int64()
    _lib.check(lib.m3s_map_count(ctypes.byref(mc), ctypes.byref(table), Kp, N, counts, ctypes.byref(total),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(device)))
    return np.frombuffer(counts, dtype=np.int64).copy(), int(total.value)


def map_write(mc, table, Twc, rgb_list, Kp, N, out, out_rgb, capacity, ws, device):
    """``m3s_map_write`` on torch's current stream; ``rgb_list``: Kp device tensors (N,3) u8, or None."""
    lib = _lib.load()
    rgb = None if rgb_list is None else (ctypes.c_void_p * Kp)(*[r.data_ptr() for r in rgb_list])
    _lib.check(lib.m3s_map_write(ctypes.byref(mc), ctypes.byref(table), _lib.ptr(Twc), rgb, Kp, N, _lib.ptr(out),
                                 _lib.ptr(out_rgb), int(capacity), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(device)))


def map_voxel_table_size(total):
    """``m3s_map_voxel_table_size``: bytes of the voxel table for a counted total."""
    return int(_lib.load(require_gpu=False).m3s_map_voxel_table_size(int(total)))


def map_voxel(mc, table, Twc, Kp, N, voxel_size, vox_table, ws, device):
    """``m3s_map_voxel`` on torch's current stream, between ``map_count`` and ``map_write`` on ``ws``; ``vox_table``: a
    uint8 device tensor of ``map_voxel_table_size(total)`` bytes or more. Returns (thinned rows per keyframe (Kp,)
    int64 numpy, thinned total, rows dropped)."""
    lib = _lib.load()
    counts = (ctypes.c_int64 * Kp)()
    total, dropped = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.m3s_map_voxel(ctypes.byref(mc), ctypes.byref(table), _lib.ptr(Twc), Kp, N, float(voxel_size),
                                 _lib.ptr(vox_table), vox_table.numel(), counts, ctypes.byref(total),
                                 ctypes.byref(dropped), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(device)))
    return np.frombuffer(counts, dtype=np.int64).copy(), int(total.value), int(dropped.value)


def world_points(keyframes, c_conf_threshold, indices=None, colors=True, layout="soa", voxel_size=None):
    """The keyframes' points with average confidence above ``c_conf_threshold``, in the world frame.

    ``keyframes``: a ``Keyframes`` or ``SharedKeyframes`` store; ``indices`` selects and orders the keyframes
    (default: all; a viewer passes its dirty ones). Rows are in keyframe order, pixels ascending: the reference's order
    (evaluate.py:50-68). ``layout="soa"`` returns ``(points (M,3) f32, colors (M,3) u8 or None, counts (K,) int64)``,
    ``layout="ply"`` returns ``(records (M,15) u8, counts)``: packed binary-PLY vertex records (x, y, z little-endian
    f32, then r, g, b; colour bytes 0 with ``colors=False``). Everything is on the keyframes' device.

    With ``config["use_calib"]`` the points are constrained to their pixel rays (evaluate.py:54-58; K from the store or
    the frame, the size from ``frame_img_size``), in the kernel and bit-identically to ``constrain_points_to_ray``.
    The poses are stacked to (K,8) as ``FactorGraph.get_poses_keyframes`` does; points and confidences are read where
    they live. ``uimg`` is on the host: it is converted as the reference does, ``(uimg * 255)`` truncated to u8, and
    uploaded at 3 B per pixel. Keyframes whose buffers do not qualify (not on a HIP device, not contiguous fp32,
    differing N) go through ``world_points_torch``.

    ``voxel_size`` (default None: every row) thins the cloud to one row per occupied cell of that size in the world
    frame, by the rule of ``voxel_select``: the row with the largest average confidence, among equal ones the first in
    the order above (so ties go to the first listed keyframe); the rows are a subsequence of the unthinned ones and
    ``counts`` are the thinned counts. One stage between the two passes (``m3s_map_voxel``: a hash table of 16 B per
    slot, 2 to 4 slots per counted row, cached like the workspace). Rows that are not finite or lie beyond 2^20 cells
    of the origin are left out, with one ``RuntimeWarning`` naming their number."""
    if layout not in _LAYOUTS:
        raise ValueError(f"world_points: layout must be 'soa' or 'ply', not {layout!r}")
    if voxel_size is not None:
        _voxel_scale(voxel_size)
    frames = _select(keyframes, indices)
    if not frames or not _in_place_ok(frames):
        return world_points_torch(keyframes, c_conf_threshold, indices, colors, layout, voxel_size)
    dev = frames[0].X_canon.device
    Kp, N = len(frames), frames[0].C.numel()
    use_calib, K = _intrinsics(keyframes, frames)
    mc = map_config(c_conf_threshold, layout, K if use_calib else None, frame_img_size(frames[0]))
    table = keyframe_table([kf.X_canon for kf in frames], [kf.C for kf in frames], [kf.N for kf in frames])
    with torch.cuda.device(dev):
        lib = _lib.load()
        ws = _lib.workspace("map", lib.m3s_map_workspace_size(Kp, N), dev, _lib.stream_ptr(dev))
        counts, M = map_count(mc, table, Kp, N, ws, dev)
        Twc = None
        if M > 0:
            Twc = torch.stack([kf.T_WC.data.reshape(1, 8) for kf in frames])[:, 0, :]
            Twc = Twc.to(dev, torch.float32).contiguous()
        if voxel_size is not None and M > 0:
            vox = _lib.workspace("map_voxel", lib.m3s_map_voxel_table_size(M), dev, _lib.stream_ptr(dev))
            counts, M, dropped = map_voxel(mc, table, Twc, Kp, N, voxel_size, vox, ws, dev)
            _warn_dropped(dropped)
        if layout == "ply":
            out, out_rgb = torch.empty((M, 15), dtype=torch.uint8, device=dev), None
        else:
            out = torch.empty((M, 3), dtype=torch.float32, device=dev)
            out_rgb = torch.empty((M, 3), dtype=torch.uint8, device=dev) if colors else None
        if M > 0:
            rgb = None
            if colors:  # one upload for all keyframes
                rgb = torch.stack([_colors_u8(kf) for kf in frames]).to(dev).contiguous()
            map_write(mc, table, Twc, None if rgb is None else list(rgb), Kp, N, out, out_rgb, M, ws, dev)
    counts_t = torch.from_numpy(counts).to(dev)
    if layout == "ply":
        return out, counts_t
    return out, out_rgb, counts_t


def _ply_header(n):
    """The header plyfile writes for these six properties (evaluate.py:88-106, ``PlyData(text=False)``)."""
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").encode("ascii")


def _write_ply(filename, records):
    """records: (M,15) u8 host array, the vertex body."""
    with open(filename, "wb") as f:
        f.write(_ply_header(records.shape[0]))
        f.write(np.ascontiguousarray(records).tobytes())


def save_ply(filename, points, colors):
    """evaluate.py:88-106 without plyfile: (M,3) points and (M,3) colours (arrays or tensors) as a binary
    little-endian PLY."""
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    points, colors = to_np(points).reshape(-1, 3), to_np(colors).reshape(-1, 3).astype(np.uint8)
    pcd = np.empty(len(points), dtype=_PLY_DTYPE)
    pcd["x"], pcd["y"], pcd["z"] = points.T
    pcd["red"], pcd["green"], pcd["blue"] = colors.T
    _write_ply(filename, pcd.view(np.uint8).reshape(-1, 15))


def save_reconstruction(savedir, filename, keyframes, c_conf_threshold, voxel_size=None):
    """evaluate.py:47-70 through the PLY layout: the file is the header plus one device-to-host copy of the vertex
    records. Unlike the reference it does not overwrite ``keyframe.X_canon`` with the ray-constrained copy in calib
    mode (evaluate.py:55-58): the keyframes are left as they are. ``voxel_size`` thins the cloud as in
    ``world_points``."""
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    records, _ = world_points(keyframes, c_conf_threshold, layout="ply", voxel_size=voxel_size)
    _write_ply(savedir / filename, records.cpu().numpy())


def save_traj(logdir, logfile, timestamps, frames, intrinsics=None):
    """evaluate.py:23-44: one ``t x y z qx qy qz qw`` line per keyframe, the pose through ``as_SE3``.
    ``intrinsics`` (``refine_pose_with_calibration``) belongs to the dataloader, which stays the reference's."""
    if intrinsics is not None:
        raise NotImplementedError("save_traj: pose refinement with calibration belongs to the reference's dataloader")
    logdir = pathlib.Path(logdir)
    logdir.mkdir(exist_ok=True, parents=True)
    with open(logdir / logfile, "w") as f:
        for i in range(len(frames)):
            keyframe = frames[i]
            t = timestamps[keyframe.frame_id]
            x, y, z, qx, qy, qz, qw = as_SE3(keyframe.T_WC).data.numpy().reshape(-1)
            f.write(f"{t} {x} {y} {z} {qx} {qy} {qz} {qw}\n")
