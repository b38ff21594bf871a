"""Cases, expectations and the error metric of the dense head tail's tests (test_head_host.py on the CPU,
test_gpu_head.py on the device; tests/golden/make_head_golden.py writes the fixture from the same generators).

A pixel's channels: 0..2 xyz, 3 the conf logit, 4..4+F-1 the descriptor, 4+F the desc_conf logit when two_confs.
Every generator returns the channel-first float32 array ``out (B, 4 + F + tc, H, W)`` that the reference's
``postprocess`` takes (layout CAT); ``to_tokens`` splits it into the ``pts`` / ``feat`` pair of layout TOKENS.

Measured on an MI355X against the fixture's float64 result, in units of 2^-24 (``err_units``), accuracy case 32 x 48,
seed 7; the bound is 2 e_ref + 1 with e_ref the same figure of the reference's own float32 CPU result:
    output      device (CAT = TOKENS)   e_ref   bound
    pts3d       2.35                    2.34    5.67
    conf        1.61                    1.43    3.86
    desc        2.64                    3.19    7.39
    desc_conf   1.19                    0.97    2.94
The special-value pixels' finite values: 0.29 / 0.11 / 0.61 / 0.11. The stand-in head of test_gpu_head.py (other inputs,
same bounds): at most 2.42 / 1.57 / 2.53 / 1.18.
"""
import numpy as np
import torch
import torch.nn.functional as F

INF = float("inf")
DEPTH_MODE = ("exp", -INF, INF)
CONF_MODE = ("exp", 1, INF)
DESC_CONF_MODE = ("exp", 0, INF)
F_ACC = 24
ACC_SEED, ACC_SHAPE = 7, (1, 32, 48)  # the fixture's accuracy case
LAYOUT_SHAPE = (2, 16, 32)            # the fixture's layout case (F = 24, two_confs)
PATCH = 16
KEYS = ("pts3d", "conf", "desc", "desc_conf")


def accuracy_inputs(seed, B, H, W, Fd=F_ACC, two_confs=True):
    """Standard normal values; xyz scaled per pixel by exp(clamp(N(0,1), -3, 2.2)), both logits by 4, the descriptor
    per pixel by exp(3 N(0,1))."""
    rng = np.random.default_rng(seed)
    tc = int(two_confs)
    out = rng.standard_normal((B, 4 + Fd + tc, H, W))
    out[:, 0:3] *= np.exp(np.clip(rng.standard_normal((B, 1, H, W)), -3.0, 2.2))
    out[:, 3] *= 4.0
    out[:, 4:4 + Fd] *= np.exp(3.0 * rng.standard_normal((B, 1, H, W)))
    if tc:
        out[:, 4 + Fd] *= 4.0
    return out.astype(np.float32)


def _grid(B, H, W):
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    return b, y, x


def layout_inputs(B, H, W, Fd=F_ACC, two_confs=True):
    """Per pixel one non-zero xyz component, at (5y + 2x + b) % 3, and one non-zero descriptor channel, at
    (7y + 3x + b) % Fd; their values are +-2^k, k in -2..2; the logits are 0 or -inf. Every output of a correct
    implementation is then exact (``layout_expected``), and a pixel read from the wrong place shows."""
    tc = int(two_confs)
    b, y, x = _grid(B, H, W)
    out = np.zeros((B, 4 + Fd + tc, H, W), dtype=np.float32)
    vx = np.where((x + y) % 2 == 0, 1.0, -1.0) * 2.0 ** ((y + 2 * x + b) % 5 - 2)
    vd = np.where((y + b) % 2 == 0, 1.0, -1.0) * 2.0 ** ((3 * y + x + b) % 5 - 2)
    np.put_along_axis(out, ((5 * y + 2 * x + b) % 3)[:, None], vx[:, None].astype(np.float32), axis=1)
    np.put_along_axis(out, (4 + (7 * y + 3 * x + b) % Fd)[:, None], vd[:, None].astype(np.float32), axis=1)
    out[:, 3] = np.where((x + y + b) % 2 == 0, 0.0, -INF)
    if tc:
        out[:, 4 + Fd] = np.where((x + 2 * y + b) % 3 == 0, 0.0, -INF)
    return out


def layout_expected(B, H, W, Fd=F_ACC, two_confs=True, conf_mode=CONF_MODE, desc_conf_mode=DESC_CONF_MODE, step=1):
    """From the generator's formulas, not from an implementation: dict of
    x_comp (B,H',W') the index of X's non-zero component, x_val (B,H',W') its float64 value sign * expm1(2^k),
    d (B,H',W') = 2^k, and the exact float32 conf (B,H',W'), desc (B,H',W',Fd), desc_conf (B,H',W')."""
    b, y, x = _grid(B, H, W)
    k = (y + 2 * x + b) % 5 - 2
    sign = np.where((x + y) % 2 == 0, 1.0, -1.0)
    desc = np.zeros((B, H, W, Fd), dtype=np.float32)
    np.put_along_axis(desc, ((7 * y + 3 * x + b) % Fd)[..., None],
                      np.where((y + b) % 2 == 0, 1.0, -1.0)[..., None].astype(np.float32), axis=-1)
    conf = (conf_mode[1] + np.where((x + y + b) % 2 == 0, 1.0, 0.0)).astype(np.float32)
    if two_confs:
        dconf = (desc_conf_mode[1] + np.where((x + 2 * y + b) % 3 == 0, 1.0, 0.0)).astype(np.float32)
    else:
        dconf = conf.copy()
    s = (slice(None), slice(None, None, step), slice(None, None, step))
    return dict(x_comp=((5 * y + 2 * x + b) % 3)[s], x_val=(sign * np.expm1(2.0 ** k))[s], d=(2.0 ** k)[s],
                conf=conf[s], desc=desc[s], desc_conf=dconf[s])


# the special-value pixels: (channels to overwrite -> values) on a benign pixel (xyz (1, 2, 2), logits 0, descriptor 1)
_NAN = float("nan")
SPECIAL_LOGITS = (0.0, 89.0, -200.0, _NAN, INF, -INF, 88.0)


def special_inputs(Fd=F_ACC, two_confs=True):
    """(1, 4 + Fd + tc, 1, P): one pixel per special value.
    xyz: 0 -> 0; d < 1e-8 -> x / 1e-8 * expm1(d); d = 100 -> +-inf, NaN where the component is 0; a NaN component ->
    three NaNs; (3e38, 3e38, 0) -> three NaNs. Logits 0, 89, -200, NaN, +inf, -inf, 88 (the desc_conf logit takes the
    same list rotated by three). Descriptor: zero -> NaN; all 1e-30 -> inf; all 1e20 -> 0; one NaN channel -> all NaN;
    one inf channel -> 0 and NaN."""
    tc = int(two_confs)
    xyz = [(0.0, 0.0, 0.0), (3e-9, 0.0, -4e-9), (-60.0, 0.0, 80.0), (_NAN, 1.0, 1.0), (3e38, 3e38, 0.0)]
    n_l = len(SPECIAL_LOGITS)
    P = len(xyz) + n_l + 5
    out = np.ones((1, 4 + Fd + tc, 1, P), dtype=np.float32)
    out[0, 1:3] = 2.0
    out[0, 3] = 0.0
    if tc:
        out[0, 4 + Fd] = 0.0
    for i, v in enumerate(xyz):
        out[0, 0:3, 0, i] = v
    p0 = len(xyz)
    for i, l in enumerate(SPECIAL_LOGITS):
        out[0, 3, 0, p0 + i] = l
        if tc:
            out[0, 4 + Fd, 0, p0 + i] = SPECIAL_LOGITS[(i + 3) % n_l]
    p1 = p0 + n_l
    d = slice(4, 4 + Fd)
    out[0, d, 0, p1] = 0.0
    out[0, d, 0, p1 + 1] = 1e-30
    out[0, d, 0, p1 + 2] = 1e20
    out[0, 4 + min(5, Fd - 1), 0, p1 + 3] = _NAN
    out[0, 4 + min(7, Fd - 1), 0, p1 + 4] = INF
    return out


def to_tokens(out):
    """out (B, 4 + C, H, W) torch -> pts (B, 4, H, W), feat (B, S, C 256): the inverse of the head's transpose / view /
    pixel_shuffle / cat."""
    B, _, H, W = out.shape
    pts = out[:, :4].contiguous()
    feat = F.pixel_unshuffle(out[:, 4:], PATCH)  # (B, C 256, H/16, W/16)
    return pts, feat.reshape(B, feat.shape[1], -1).transpose(1, 2).contiguous()


def norm64(out):
    """d (B,H,W) float64 of the xyz channels."""
    return np.sqrt((out[:, 0:3].astype(np.float64) ** 2).sum(axis=1))


def classes(a):
    """0 finite non-zero, 1 NaN, 2 +inf, 3 -inf, 4 zero."""
    a = np.asarray(a)
    return np.select([np.isnan(a), a == INF, a == -INF, a == 0], [1, 2, 3, 4], 0)


def err_units(got, truth, scale=None, where=None):
    """max |got - truth| / (|truth| s) in units of 2^-24 over the elements where truth is finite and non-zero (and
    ``where`` holds); s = ``scale`` broadcast, default 1. For X the scale is max(1, d): an error in d is amplified by d
    through expm1."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    s = np.ones_like(truth) if scale is None else np.broadcast_to(scale, truth.shape)
    m = np.isfinite(truth) & (truth != 0)
    if where is not None:
        m &= np.broadcast_to(where, truth.shape)
    if not m.any():
        return 0.0
    return float((np.abs(got[m] - truth[m]) / (np.abs(truth[m]) * s[m])).max() * 2.0 ** 24)


def scales(out):
    """The metric's scale per output key for the inputs ``out`` (numpy, channel-first)."""
    return dict(pts3d=np.maximum(1.0, norm64(out))[..., None], conf=None, desc=None, desc_conf=None)


def bounds(golden, prefix="acc"):
    """2 e_ref + 1 per output key, e_ref measured on the fixture: the reference's float32 CPU result against its
    float64 result."""
    sc = scales(golden[prefix + "_out"])
    e_ref = {k: err_units(golden[f"{prefix}_ref32_{k}"], golden[f"{prefix}_ref64_{k}"], sc[k]) for k in KEYS}
    return {k: 2.0 * e + 1.0 for k, e in e_ref.items()}, e_ref
