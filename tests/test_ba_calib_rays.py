"""Host-only: the pixel-ray tables of the raw-calib BA mode (m3s_ba_calib_rays, mode 3 of m3s_ba_config).

A mode-3 plan forms X_j = z_j * (x_of_u[u], y_of_v[v], 1) in its kernels and must give the poses of mode 2 on
constrain_points_to_ray(points) bit for bit, so its tables must be torch's (u - cx) / fx, (v - cy) / fy to the last
bit: one fp32 subtraction, then one correctly rounded fp32 division. A reciprocal-multiply table rounds differently
in a few entries at 48x66 (none at 24x32 or 384x512): that is the shape tested, and the test itself checks that each
K it uses can tell the two apart.
"""
import numpy as np
import pytest
import torch

H, W = 48, 66


def _tum_like(H, W):
    """TUM freiburg1 calibration (640x480) scaled per axis to H x W: fx != fy, cx and cy no representable halves."""
    sx, sy = 640.0 / W, 480.0 / H
    return torch.tensor([[517.3 / sx, 0.0, 318.6 / sx], [0.0, 516.5 / sy, 255.3 / sy], [0.0, 0.0, 1.0]],
                        dtype=torch.float32)


def _centred(H, W):
    from m3s.synthetic import intrinsics

    return intrinsics(H, W)


@pytest.mark.parametrize("make_K", [_centred, _tum_like], ids=["centred", "tum_like"])
def test_calib_ray_tables_are_torch_division_bit_for_bit(make_K):
    from m3s import _lib
    from m3s.config import config
    from m3s.dist_ba import BA_MODES, ba_config
    from m3s.geometry import backproject, get_pixel_coords

    K = make_K(H, W)
    assert K.dtype == torch.float32 and K.device.type == "cpu"
    assert BA_MODES["calib_raw"] == 3
    cfg = ba_config("calib_raw", config["local_opt"], K, H, W)
    assert cfg.mode == 3 and (cfg.height, cfg.width) == (H, W)
    x_of_u, y_of_v = _lib.ba_calib_rays(cfg)
    assert x_of_u.shape == (W,) and y_of_v.shape == (H,) and x_of_u.dtype == y_of_v.dtype == np.float32

    uv = get_pixel_coords(1, (H, W), "cpu", torch.float32)
    rays = backproject(uv, torch.ones(1, H, W, 1), K)[0, ..., :2].numpy()  # (H, W, 2)
    # the expected tables are separable: x depends on the column only, y on the row only
    assert (rays[..., 0] == rays[:1, :, 0]).all() and (rays[..., 1] == rays[:, :1, 1]).all()
    want_x, want_y = rays[0, :, 0], rays[:, 0, 1]

    # this K tells a division from a reciprocal-multiply (otherwise the equality below would prove nothing)
    fx, fy, cx, cy = (np.float32(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    rcp_x = (np.arange(W, dtype=np.float32) - cx) * (np.float32(1.0) / fx)
    rcp_y = (np.arange(H, dtype=np.float32) - cy) * (np.float32(1.0) / fy)
    n_diff = int((rcp_x != want_x).sum() + (rcp_y != want_y).sum())
    print(f"{make_K.__name__}: reciprocal-multiply differs from the division in {n_diff} of {W + H} entries")
    assert n_diff >= 1

    assert np.array_equal(x_of_u.view(np.uint32), want_x.view(np.uint32))
    assert np.array_equal(y_of_v.view(np.uint32), want_y.view(np.uint32))


def test_calib_ray_tables_reject_bad_sizes():
    from m3s import _lib
    from m3s.config import config
    from m3s.dist_ba import ba_config

    cfg = ba_config("calib_raw", config["local_opt"], _centred(H, W), H, W)
    cfg.width = 65536
    with pytest.raises(RuntimeError):
        _lib.ba_calib_rays(cfg)
    cfg.width, cfg.height = W, 0
    with pytest.raises(RuntimeError):
        _lib.ba_calib_rays(cfg)
