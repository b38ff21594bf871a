"""Map and trajectory export (the reference's ``mast3r_slam/evaluate.py:23-106``).

``world_points`` is the confidence-filtered world point cloud of the keyframes: the cloud the reference saves at
the end of a run (``evaluate.save_reconstruction``, ``main.py:370-376``) and its viewer shows live
(``visualization.py:38,351``). The reference loops over the keyframes on the host (a constrained copy in calib mode,
``T_WC.act``, three ``.cpu().numpy()`` copies, a boolean index and a final concatenate). Here the keyframes' own
device buffers are read in place by two HIP passes (csrc/map.hip: ``m3s_map_count`` stores one validity bit per point
and scans the block counts, ``m3s_map_write`` transforms and compacts in keyframe order and pixel order), so only the
poses (K x 8 floats) and the colours (3 B per pixel, the host ``uimg``) are gathered.

``world_points_torch`` is the same contract in plain torch ops, the reference's formulation on
``m3s.geometry.constrain_points_to_ray`` and ``Sim3.act``; it runs on any device and is what ``world_points`` falls
back to for keyframes whose buffers the kernels cannot read in place (not on a HIP device, not contiguous fp32,
differing sizes).
"""
import ctypes
import pathlib

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


def world_points_torch(keyframes, c_conf_threshold, indices=None, colors=True, layout="soa"):
    """``world_points`` in plain torch ops on the keyframes' device (evaluate.py:50-68 per keyframe, concatenated
    there instead of on the host)."""
    if layout not in _LAYOUTS:
        raise ValueError(f"world_points: layout must be 'soa' or 'ply', not {layout!r}")
    frames = _select(keyframes, indices)
    dev = frames[0].X_canon.device if frames else torch.device("cpu")
    use_calib, K = _intrinsics(keyframes, frames) if frames else (False, None)
    pts, cols, counts = [torch.zeros((0, 3), dtype=torch.float32, device=dev)], [], []
    for kf in frames:
        X = kf.X_canon.reshape(-1, 3)
        if use_calib:
            X = constrain_points_to_ray(frame_img_size(kf), X[None], K.to(X.device))[0]
        pW = kf.T_WC.to(X.device).act(X).reshape(-1, 3)
        valid = kf.get_average_conf().reshape(-1) > c_conf_threshold
        pts.append(pW[valid])
        counts.append(int(valid.sum()))
        if colors:
            cols.append(_colors_u8(kf).to(dev)[valid])
    points = torch.cat(pts, dim=0)
    cols_t = torch.cat([torch.zeros((0, 3), dtype=torch.uint8, device=dev)] + cols, dim=0) if colors else None
    counts_t = torch.tensor(counts, dtype=torch.int64, device=dev)
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


def world_points(keyframes, c_conf_threshold, indices=None, colors=True, layout="soa"):
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
    differing N) go through ``world_points_torch``."""
    if layout not in _LAYOUTS:
        raise ValueError(f"world_points: layout must be 'soa' or 'ply', not {layout!r}")
    frames = _select(keyframes, indices)
    if not frames or not _in_place_ok(frames):
        return world_points_torch(keyframes, c_conf_threshold, indices, colors, layout)
    dev = frames[0].X_canon.device
    Kp, N = len(frames), frames[0].C.numel()
    use_calib, K = _intrinsics(keyframes, frames)
    mc = map_config(c_conf_threshold, layout, K if use_calib else None, frame_img_size(frames[0]))
    table = keyframe_table([kf.X_canon for kf in frames], [kf.C for kf in frames], [kf.N for kf in frames])
    with torch.cuda.device(dev):
        lib = _lib.load()
        ws = _lib.workspace("map", lib.m3s_map_workspace_size(Kp, N), dev, _lib.stream_ptr(dev))
        counts, M = map_count(mc, table, Kp, N, ws, dev)
        if layout == "ply":
            out, out_rgb = torch.empty((M, 15), dtype=torch.uint8, device=dev), None
        else:
            out = torch.empty((M, 3), dtype=torch.float32, device=dev)
            out_rgb = torch.empty((M, 3), dtype=torch.uint8, device=dev) if colors else None
        if M > 0:
            Twc = torch.stack([kf.T_WC.data.reshape(1, 8) for kf in frames])[:, 0, :]
            Twc = Twc.to(dev, torch.float32).contiguous()
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


def save_reconstruction(savedir, filename, keyframes, c_conf_threshold):
    """evaluate.py:47-70 through the PLY layout: the file is the header plus one device-to-host copy of the vertex
    records. Unlike the reference it does not overwrite ``keyframe.X_canon`` with the ray-constrained copy in calib
    mode (evaluate.py:55-58): the keyframes are left as they are."""
    savedir = pathlib.Path(savedir)
    savedir.mkdir(exist_ok=True, parents=True)
    records, _ = world_points(keyframes, c_conf_threshold, layout="ply")
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
