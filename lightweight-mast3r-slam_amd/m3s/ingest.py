"""Frame ingest: from a decoded camera image to the ViT's input, the reference's ``create_frame`` -> ``resize_img``
(``mast3r_slam/frame.py:111-122``, ``mast3r_utils.py:245-289``).

The reference turns the float image back into ``uint8``, lets Pillow resample it to a long edge of 512 (LANCZOS when
shrinking, BICUBIC otherwise), crops the centre to multiples of 16, normalises to the ``(1,3,H,W)`` tensor it uploads and
makes a second ``/ 255`` copy for ``uimg``, all on one host thread. ``m3s_ingest`` does the same on the device in two
launches, bit for bit: Pillow's 8-bit resampler is fixed point (``include/m3s.h``), so the bytes are equal, not close.

``resize_img(img, size, ..., device=None)`` is the host statement (Pillow, then ``ToTensor`` / ``Normalize`` as torch
ops); with a HIP device it runs the kernels. ``ingest`` is the device operator itself, ``create_frame`` the reference's
per-frame entry point, which takes the device path when ``M3S_INGEST_FUSED=1``.

A caller that holds the camera's ``uint8`` image should pass it as it is: the float image the reference's loaders
make of it (``/ 255``) gives the same bytes back (``uint8(float32(u) / 255 * 255) == u`` for all 256 levels) at four
times the upload.
"""
import collections
import ctypes
import sys

import numpy as np
import torch

from m3s import _lib
from m3s.config import config

Geometry = collections.namedtuple(
    "Geometry", "resized filter crop out_size transformation")  # (Wr, Hr), 0 / 1, (x0, y0, x1, y1), (Wc, Hc), 4 floats


def geometry(h, w, size=512, square_ok=False):
    """The geometry ``resize_img`` gives a (h, w) image: resized (W, H), the filter (``_lib.INGEST_BICUBIC`` /
    ``_lib.INGEST_LANCZOS``), the crop box in the resized image, the output (W, H) and the transformation tuple
    (scale_w, scale_h, half_crop_w, half_crop_h). RuntimeError where the crop is empty or an argument is bad."""
    g = _lib.ingest_geometry(h, w, size, square_ok)
    return Geometry((g.resized_w, g.resized_h), g.filter, (g.crop_x0, g.crop_y0, g.crop_x1, g.crop_y1),
                    (g.out_w, g.out_h), (g.scale_w, g.scale_h, g.half_crop_w, g.half_crop_h))


def _is_hip(device):
    return device is not None and torch.device(device).type == "cuda"


def _source(img, device):
    """img -> a (B, H, W, 3) uint8 or float32 device tensor whose pixels and rows the kernel can walk, and whether the
    caller's image had the batch dimension."""
    t = torch.from_numpy(img) if isinstance(img, np.ndarray) else img
    if not isinstance(t, torch.Tensor):
        raise TypeError("ingest: img must be a numpy array or a torch tensor")
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"ingest: img must be uint8 or float32 (got {t.dtype})")
    if t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise RuntimeError(f"ingest: img must be (H, W, 3) or (B, H, W, 3) (got {tuple(t.shape)})")
    batched = t.dim() == 4
    t = t.to(device)
    if not batched:
        t = t[None]
    B, H, W, _ = t.shape
    if t.stride(3) != 1 or t.stride(2) != 3 or t.stride(1) < 3 * W or (B > 1 and t.stride(0) != H * t.stride(1)):
        t = t.contiguous()
    return t, batched


def run(src, size=512, square_ok=False, downsample=1, img=None, uimg=None, rgb_u8=None):
    """The raw call of ``m3s_ingest`` on a (B, H, W, 3) device tensor ``src`` (uint8 or float32; a row stride of its own
    is fine, pixels are contiguous). ``img`` (B,3,Hc,Wc) f32, ``uimg`` (B,ceil(Hc/ds),ceil(Wc/ds),3) f32 and ``rgb_u8``
    (B,Hc,Wc,3) u8 are the caller's contiguous device tensors; None passes a null pointer and that output is skipped."""
    _lib.require_cuda("ingest", src, img, uimg, rgb_u8)
    B, H, W, _ = src.shape
    lib = _lib.load()
    es = src.element_size()
    a = _lib.IngestArgs(src.data_ptr(), _lib.INGEST_F32 if src.dtype == torch.float32 else _lib.INGEST_U8,
                        src.stride(1) * es, B, H, W, int(size), int(bool(square_ok)), int(downsample),
                        *(t.data_ptr() if t is not None else None for t in (img, uimg, rgb_u8)))
    with torch.cuda.device(src.device):
        stream = _lib.stream_ptr(src.device)
        nbytes = lib.m3s_ingest_workspace_size(H, W, int(size), int(bool(square_ok)), B)
        ws = _lib.workspace("ingest", nbytes, src.device, stream)
        _lib.check(lib.m3s_ingest(ctypes.byref(a), _lib.ptr(ws), ws.numel(), stream))


def ingest(img, size=512, downsample=None, device="cuda:0", square_ok=False):
    """img: numpy array or tensor, on the host or the device, ``uint8`` or ``float32`` in [0, 1], (H, W, 3) or
    (B, H, W, 3) -> (img (B,3,Hc,Wc) f32 normalised, uimg f32 in [0, 1] downsampled, rgb_u8, true_shape (B,2) int32
    rows of (Hc, Wc)), all on ``device``; uimg and rgb_u8 carry the batch dimension when the source does. ``downsample``
    defaults to ``config["dataset"]["img_downsample"]``."""
    if not _is_hip(device):
        raise RuntimeError(f"ingest: device must be a HIP device (got {device}); the host statement is resize_img")
    _lib.load()  # no HIP device, no library: an error, never the host path
    device = torch.device(device)
    ds = int(config["dataset"]["img_downsample"] if downsample is None else downsample)
    src, batched = _source(img, device)
    B, H, W, _ = src.shape
    Wc, Hc = geometry(H, W, size, square_ok).out_size
    out = torch.empty((B, 3, Hc, Wc), dtype=torch.float32, device=src.device)
    uimg = torch.empty((B, -(-Hc // max(ds, 1)), -(-Wc // max(ds, 1)), 3), dtype=torch.float32, device=src.device)
    rgb = torch.empty((B, Hc, Wc, 3), dtype=torch.uint8, device=src.device)
    run(src, size, square_ok, ds, out, uimg, rgb)
    true_shape = torch.tensor([[Hc, Wc]] * B, dtype=torch.int32, device=src.device)
    return (out, uimg, rgb, true_shape) if batched else (out, uimg[0], rgb[0], true_shape)


def _resize_host(img, size, square_ok):
    """Pillow's part of the host statement: the cropped PIL image and the transformation tuple."""
    import PIL.Image

    if size != 224 and size != 512:
        raise RuntimeError("resize_img: size must be 512 or 224")
    if isinstance(img, torch.Tensor):
        img = img.cpu().numpy()
    pil = PIL.Image.fromarray(img if img.dtype == np.uint8 else np.uint8(img * 255))
    W1, H1 = pil.size
    S = max(W1, H1)
    L = size if size == 512 else round(size * max(W1 / H1, H1 / W1))
    new_size = tuple(int(round(x * L / S)) for x in pil.size)
    pil = pil.resize(new_size, PIL.Image.LANCZOS if S > L else PIL.Image.BICUBIC)
    W, H = pil.size
    cx, cy = W // 2, H // 2
    if size == 224:
        half = min(cx, cy)
        box = (cx - half, cy - half, cx + half, cy + half)
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
        if not square_ok and W == H:
            halfh = 3 * halfw // 4  # halfw is a multiple of 8
        box = (cx - halfw, cy - halfh, cx + halfw, cy + halfh)
    if box[2] <= box[0] or box[3] <= box[1]:
        raise RuntimeError("resize_img: the crop is empty")
    pil = pil.crop(box)
    return pil, (W1 / W, H1 / H, (W - pil.size[0]) / 2, (H - pil.size[1]) / 2)


def resize_img(img, size, square_ok=False, return_transformation=False, device=None):
    """The reference's ``resize_img``: img (H, W, 3) float in [0, 1] (or the ``uint8`` image itself) -> dict(img
    (1,3,Hc,Wc) f32, true_shape np.int32 [[Hc, Wc]], unnormalized_img (Hc,Wc,3) uint8), and the transformation tuple on
    request. ``device=None``: the host statement, Pillow then ``ToTensor`` / ``Normalize(0.5, 0.5)`` as torch ops, host
    tensors out (unnormalized_img a numpy array, as the reference's). A HIP device: ``img`` and ``unnormalized_img`` are
    device tensors from ``m3s_ingest``."""
    if _is_hip(device):
        if isinstance(img, (np.ndarray, torch.Tensor)) and img.ndim != 3:
            raise RuntimeError("resize_img: img must be (H, W, 3)")
        _lib.load()
        src, _ = _source(img, torch.device(device))
        g = geometry(src.shape[1], src.shape[2], size, square_ok)
        Wc, Hc = g.out_size
        out = torch.empty((1, 3, Hc, Wc), dtype=torch.float32, device=src.device)
        rgb = torch.empty((1, Hc, Wc, 3), dtype=torch.uint8, device=src.device)
        run(src, size, square_ok, 1, out, None, rgb)
        res = dict(img=out, true_shape=np.int32([[Hc, Wc]]), unnormalized_img=rgb[0])
        tf = g.transformation
    else:
        if device is not None and torch.device(device).type != "cpu":
            raise RuntimeError(f"resize_img: device must be None, the CPU or a HIP device (got {device})")
        pil, tf = _resize_host(img, size, square_ok)
        u8 = np.array(pil)
        t = torch.from_numpy(u8).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)
        res = dict(img=t[None].contiguous(), true_shape=np.int32([pil.size[::-1]]), unnormalized_img=u8)
    return (res, tf) if return_transformation else res


def create_frame(i, img, T_WC, img_size=512, device="cuda:0"):
    """The reference's ``create_frame``: the frame of image ``img`` (H, W, 3; float in [0, 1] or uint8) with pose
    ``T_WC``. ``img`` (1,3,Hc,Wc) is on ``device``, ``img_shape`` (divided by the config's ``img_downsample``) and
    ``img_true_shape`` are int32 tensors on it, ``uimg`` is a host float32 tensor as the shared keyframe stores hold it.
    With ``M3S_INGEST_FUSED=1`` and a HIP ``device`` the image is uploaded as it is and ``m3s_ingest`` does the rest, with
    one device-to-host copy for ``uimg``; otherwise this is the host statement. The results are equal bit for bit.
    Builds ``mast3r_slam.frame.Frame`` when that module is imported (the hook's case), else ``m3s.frame.Frame``."""
    downsample = int(config["dataset"]["img_downsample"])
    if _lib.env_flag("M3S_INGEST_FUSED", False) and _is_hip(device):
        rgb, uimg_dev, _, img_true_shape = ingest(img, img_size, max(downsample, 1), device)
        uimg = uimg_dev.cpu()
        img_shape = img_true_shape // downsample if downsample > 1 else img_true_shape.clone()
    else:
        res = resize_img(img, img_size)
        rgb = res["img"].to(device=device)
        img_shape = torch.tensor(res["true_shape"], device=device)
        img_true_shape = img_shape.clone()
        uimg = torch.from_numpy(res["unnormalized_img"]) / 255.0
        if downsample > 1:
            uimg = uimg[::downsample, ::downsample]
            img_shape = img_shape // downsample
    ref = sys.modules.get("mast3r_slam.frame")
    if ref is not None and hasattr(ref, "Frame"):
        return ref.Frame(i, rgb, img_shape, img_true_shape, uimg, T_WC)
    from m3s.frame import Frame

    return Frame(i, tuple(int(v) for v in rgb.shape[-2:]), T_WC, img=rgb, uimg=uimg, img_shape=img_shape,
                 img_true_shape=img_true_shape)
