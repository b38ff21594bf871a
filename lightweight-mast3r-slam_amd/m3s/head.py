"""Dense head tail: from the ViT head's raw output to the matcher's X, C, D, Q in one HIP launch (``m3s_head_post``).

Replaces the tail of MASt3R's ``Cat_MLP_LocalFeatures_DPT_Pts3d.forward`` and its ``postprocess``
(``thirdparty/mast3r/mast3r/catmlp_dpt_head.py:25-39,82-95``), the regressions of
``dust3r/heads/postprocess.py:22-55`` and the stacking and ``downsample`` of
``mast3r_slam/mast3r_utils.py:69-78,210-216``. The DPT convolutions and the MLP stay stock PyTorch.

* ``postprocess`` has the reference's signature and returns its dict; the hook binds it in place of the reference's.
  ``cat_tail`` is its launch with the kernel's pixel step and preallocated outputs.
* ``head_tail`` takes the DPT output and the MLP output as they are, before ``transpose`` / ``view`` /
  ``pixel_shuffle`` / ``cat``, keeps only the pixels ``[::step, ::step]`` and can write into preallocated outputs.
* ``postprocess_torch`` and ``head_tail_torch`` state the same operators in torch ops. They are the CPU path, the
  timing baseline of ``scripts/head_post_time.py``, and the route of every call the kernel does not take: a depth mode
  other than ``('exp', -inf, inf)``, a conf mode other than ``('exp', finite vmin, vmax > vmin)``, a desc mode other
  than ``'norm'``, ``desc_dim=None`` or ``conf_mode=None``, a descriptor wider than 32 channels, channels beyond
  ``4 + desc_dim + two_confs``, a dtype other than float32, and a tensor that requires grad under grad mode (the kernel
  is forward only). A HIP float32 call with the device modes always runs the kernel: there is no fallback from it.
* ``FusedHeadMixin`` puts ``head_tail`` behind the head class's ``forward``; ``asymmetric_inference`` is
  ``mast3r_utils.py:190-217`` with both views written into one stacked allocation.
"""
import math

import torch
import torch.nn.functional as F

from m3s import _lib

PATCH = 16  # the ViT's patch edge, the only pixel_shuffle factor the kernel's TOKENS layout takes
MAX_F = 32
DEPTH_MODE = ("exp", -float("inf"), float("inf"))  # the one depth mode on the device


# ---------------------------------------------------------------------------------------------- torch statements
def _depth_torch(xyz, mode):
    kind, vmin, vmax = mode
    if not (vmin == -float("inf") and vmax == float("inf")):
        raise AssertionError("depth modes are unbounded")
    if kind == "linear":
        return xyz
    d = xyz.norm(dim=-1, keepdim=True)
    unit = xyz / d.clip(min=1e-8)
    if kind == "square":
        return unit * d.square()
    if kind == "exp":
        return unit * torch.expm1(d)
    raise ValueError(f"bad depth mode {kind!r}")


def _conf_torch(x, mode):
    kind, vmin, vmax = mode
    if kind == "exp":
        return vmin + x.exp().clip(max=vmax - vmin)
    if kind == "sigmoid":
        return (vmax - vmin) * torch.sigmoid(x) + vmin
    raise ValueError(f"bad conf mode {kind!r}")


def postprocess_torch(out, depth_mode, conf_mode, desc_dim=None, desc_mode="norm", two_confs=False,
                      desc_conf_mode=None):
    """The reference's ``postprocess`` in torch ops: out (B, C, H, W) -> dict of channel-last tensors."""
    if desc_conf_mode is None:
        desc_conf_mode = conf_mode
    fmap = out.permute(0, 2, 3, 1)
    res = {"pts3d": _depth_torch(fmap[..., 0:3], depth_mode)}
    if conf_mode is not None:
        res["conf"] = _conf_torch(fmap[..., 3], conf_mode)
    if desc_dim is not None:
        if "norm" not in desc_mode:
            raise ValueError(f"Unknown desc mode {desc_mode}")
        c0 = 4 if conf_mode is not None else 3
        desc = fmap[..., c0:c0 + desc_dim]
        res["desc"] = desc / desc.norm(dim=-1, keepdim=True)
        if two_confs:
            res["desc_conf"] = _conf_torch(fmap[..., c0 + desc_dim], desc_conf_mode)
        else:
            res["desc_conf"] = res["conf"].clone()
    return res


def _fill(out, vals):
    _check_out(out, [tuple(v.shape) for v in vals], vals[0].dtype, vals[0].device)
    for o, v in zip(out, vals):
        o.copy_(v)
    return tuple(out)


def head_tail_torch(pts, feat, H, W, *, two_confs, conf_mode, desc_conf_mode=None, step=1, out=None,
                    depth_mode=DEPTH_MODE, desc_mode="norm"):
    """The stock tail: ``transpose``, ``view``, ``pixel_shuffle``, ``cat``, ``postprocess_torch``, then the strided
    ``downsample`` with ``.contiguous()``. pts (B, 4, H, W), feat (B, S, (F + two_confs) 256) -> X, C, D, Q."""
    B = feat.shape[0]
    Fd = feat.shape[-1] // (PATCH * PATCH) - int(bool(two_confs))
    local = feat.transpose(-1, -2).view(B, -1, H // PATCH, W // PATCH)
    local = F.pixel_shuffle(local, PATCH)
    res = postprocess_torch(torch.cat([pts, local], dim=1), depth_mode, conf_mode, desc_dim=Fd, desc_mode=desc_mode,
                            two_confs=two_confs, desc_conf_mode=desc_conf_mode)
    X, C, D, Q = res["pts3d"], res["conf"], res["desc"], res["desc_conf"]
    if step > 1:
        X, D = X[:, ::step, ::step, :].contiguous(), D[:, ::step, ::step, :].contiguous()
        C, Q = C[:, ::step, ::step].contiguous(), Q[:, ::step, ::step].contiguous()
    if out is not None:
        return _fill(out, (X, C, D, Q))
    return X, C, D, Q


# ---------------------------------------------------------------------------------------------- the device path
def _exp_bounds(mode, unbounded=False):
    """(vmin, vmax) of an ``('exp', vmin, vmax)`` mode the kernel takes, else None."""
    try:
        kind, vmin, vmax = mode
        vmin, vmax = float(vmin), float(vmax)
    except (TypeError, ValueError):
        return None
    if kind != "exp":
        return None
    if unbounded:
        return (vmin, vmax) if (vmin == -float("inf") and vmax == float("inf")) else None
    return (vmin, vmax) if (math.isfinite(vmin) and vmax > vmin) else None


def device_modes(depth_mode, conf_mode, desc_mode, two_confs, desc_conf_mode):
    """The kernel's modes: depth ('exp', -inf, inf), conf and desc_conf ('exp', finite vmin, vmax > vmin), desc
    'norm'. Returns (conf bounds, desc_conf bounds) or None."""
    if _exp_bounds(depth_mode, unbounded=True) is None or desc_mode != "norm":
        return None
    cb = _exp_bounds(conf_mode)
    qb = _exp_bounds(conf_mode if desc_conf_mode is None else desc_conf_mode) if two_confs else cb
    return None if cb is None or qb is None else (cb, qb)


def _on_device(*tensors):
    """HIP float32 tensors, none of which needs a gradient."""
    grad = torch.is_grad_enabled()
    return all(t.is_cuda and t.dtype == torch.float32 and not (grad and t.requires_grad) for t in tensors)


def _check_out(out, shapes, dtype, device):
    if len(out) != 4:
        raise RuntimeError("head: out must be the four tensors (X, C, D, Q)")
    for name, t, shape in zip("XCDQ", out, shapes):
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"head: out {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        if t.dtype != dtype or t.device != device:
            raise RuntimeError(f"head: out {name} must be {dtype} on {device} (got {t.dtype} on {t.device})")
        if not t.is_contiguous():
            raise RuntimeError(f"head: out {name} must be contiguous")


def _launch(layout, a, feat, B, H, W, Fd, two_confs, step, bounds, out):
    step = int(step)
    if step < 1:
        raise RuntimeError("head: step must be at least 1")
    Ho, Wo = -(-H // step), -(-W // step)
    shapes = ((B, Ho, Wo, 3), (B, Ho, Wo), (B, Ho, Wo, Fd), (B, Ho, Wo))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=a.device) for s in shapes)
    else:
        _check_out(out, shapes, torch.float32, a.device)
    lib = _lib.load()
    (cmin, cmax), (qmin, qmax) = bounds
    with torch.cuda.device(a.device):
        _lib.check(lib.m3s_head_post(layout, _lib.ptr(a), _lib.ptr(feat), B, H, W, Fd, int(bool(two_confs)), step,
                                     cmin, cmax, qmin, qmax, *(_lib.ptr(t) for t in out), _lib.stream_ptr(a.device)))
    return tuple(out)


def postprocess(out, depth_mode, conf_mode, desc_dim=None, desc_mode="norm", two_confs=False, desc_conf_mode=None):
    """The reference's ``postprocess`` (catmlp_dpt_head.py:25-39): out (B, 4 + desc_dim + two_confs, H, W) ->
    dict(pts3d (B,H,W,3), conf (B,H,W), desc (B,H,W,desc_dim), desc_conf (B,H,W)). One launch of layout CAT for a HIP
    float32 tensor with the device modes; ``postprocess_torch`` for everything else (module docstring)."""
    bounds = device_modes(depth_mode, conf_mode, desc_mode, two_confs, desc_conf_mode)
    fused = (bounds is not None and desc_dim is not None and 1 <= int(desc_dim) <= MAX_F and out.dim() == 4
             and out.shape[1] == 4 + int(desc_dim) + int(bool(two_confs)) and _on_device(out))
    if not fused:
        return postprocess_torch(out, depth_mode, conf_mode, desc_dim, desc_mode, two_confs, desc_conf_mode)
    X, C, D, Q = cat_tail(out, int(desc_dim), two_confs=two_confs, conf_mode=conf_mode, desc_conf_mode=desc_conf_mode)
    return dict(pts3d=X, conf=C, desc=D, desc_conf=Q)


def cat_tail(out, desc_dim, *, two_confs, conf_mode, desc_conf_mode=None, step=1, out_tensors=None):
    """Layout CAT with the kernel's stride and preallocated outputs: out (B, 4 + desc_dim + two_confs, H, W), a HIP
    float32 tensor -> X, C, D, Q over the pixels ``[::step, ::step]``; the device path only (``postprocess`` is the
    entry with the torch route)."""
    tc = int(bool(two_confs))
    bounds = device_modes(DEPTH_MODE, conf_mode, "norm", two_confs, desc_conf_mode)
    if bounds is None:
        raise RuntimeError("cat_tail: conf modes must be ('exp', finite vmin, vmax > vmin)")
    if out.dim() != 4 or out.shape[1] != 4 + desc_dim + tc or not 1 <= desc_dim <= MAX_F:
        raise RuntimeError(f"cat_tail: out must be (B, 4 + desc_dim + two_confs, H, W) with desc_dim in 1..{MAX_F}, "
                           f"got {tuple(out.shape)} for desc_dim {desc_dim}")
    _lib.require_cuda("cat_tail", out)
    if out.dtype != torch.float32:
        raise RuntimeError("cat_tail: out must be float32")
    B, _, H, W = out.shape
    return _launch(_lib.HEAD_CAT, out.contiguous(), None, B, H, W, desc_dim, two_confs, step, bounds, out_tensors)


def head_tail(pts, feat, H, W, *, two_confs, conf_mode, desc_conf_mode=None, step=1, out=None):
    """pts (B, 4, H, W), the DPT output, and feat (B, S, (F + two_confs) 256), the MLP output, S = (H/16)(W/16) ->
    X (B,H',W',3), C (B,H',W'), D (B,H',W',F), Q (B,H',W') over the pixels ``[::step, ::step]``. One launch of layout
    TOKENS. ``out=(X, C, D, Q)``: preallocated contiguous tensors to write into (slices ``X[v:v+1]`` of a stacked
    allocation, say); they are returned."""
    H, W = int(H), int(W)
    tc = int(bool(two_confs))
    if H % PATCH or W % PATCH:
        raise RuntimeError(f"head_tail: H and W must be multiples of {PATCH} (got {H} x {W})")
    if feat.dim() != 3 or feat.shape[1] != (H // PATCH) * (W // PATCH) or feat.shape[2] % (PATCH * PATCH):
        raise RuntimeError(f"head_tail: feat must be (B, {(H // PATCH) * (W // PATCH)}, channels * {PATCH * PATCH}), "
                           f"got {tuple(feat.shape)}")
    B = feat.shape[0]
    Fd = feat.shape[2] // (PATCH * PATCH) - tc
    if tuple(pts.shape) != (B, 4, H, W):
        raise RuntimeError(f"head_tail: pts must be {(B, 4, H, W)}, got {tuple(pts.shape)}")
    if Fd < 1:
        raise RuntimeError("head_tail: feat holds no descriptor channel")
    bounds = device_modes(DEPTH_MODE, conf_mode, "norm", two_confs, desc_conf_mode)
    if bounds is None or Fd > MAX_F or not _on_device(pts, feat):
        return head_tail_torch(pts, feat, H, W, two_confs=two_confs, conf_mode=conf_mode,
                               desc_conf_mode=desc_conf_mode, step=step, out=out)
    return _launch(_lib.HEAD_TOKENS, pts.contiguous(), feat.contiguous(), B, H, W, Fd, two_confs, step, bounds, out)


# ---------------------------------------------------------------------------------------------- the head class
class FusedHeadMixin:
    """In front of ``Cat_MLP_LocalFeatures_DPT_Pts3d`` (m3s/hook.py SUBCLASSES): ``forward`` runs the DPT and the MLP
    as the reference does and hands their outputs to ``head_tail``. It defers to the reference's ``forward`` when the
    head has no ``postprocess`` or its modes are not the device's."""

    def fused_bounds(self):
        """The (conf, desc_conf) bounds when this head's tail is the device's operator, else None."""
        if not getattr(self, "postprocess", None) or getattr(self, "patch_size", None) != PATCH:
            return None
        if not 1 <= int(self.local_feat_dim) <= MAX_F:
            return None
        return device_modes(self.depth_mode, self.conf_mode, self.desc_mode, self.two_confs, self.desc_conf_mode)

    def forward_tail(self, decout, img_shape, step=1, out=None):
        """X, C, D, Q of ``forward`` over the pixels ``[::step, ::step]``, written into ``out`` when given."""
        H, W = int(img_shape[0]), int(img_shape[1])
        pts = self.dpt(decout, image_size=(H, W))
        feat = self.head_local_features(torch.cat([decout[0], decout[-1]], dim=-1))
        return head_tail(pts, feat, H, W, two_confs=self.two_confs, conf_mode=self.conf_mode,
                         desc_conf_mode=self.desc_conf_mode, step=step, out=out)

    def forward(self, decout, img_shape):
        if self.fused_bounds() is None:
            return super().forward(decout, img_shape)
        X, C, D, Q = self.forward_tail(decout, img_shape)
        return dict(pts3d=X, conf=C, desc=D, desc_conf=Q)


# ---------------------------------------------------------------------------------------------- the tracker's call
def _encode(model, frame):
    if frame.feat is None:
        frame.feat, frame.pos, _ = model._encode_image(frame.img, frame.img_true_shape)


@torch.inference_mode()
def asymmetric_inference(model, frame_i, frame_j):
    """``mast3r_asymmetric_inference`` (mast3r_utils.py:190-217) -> X (2,H',W',3), C (2,H',W'), D (2,H',W',F),
    Q (2,H',W'), with ``config["dataset"]["img_downsample"]`` as the kernel's step and both views written straight into
    one stacked allocation. A head without ``FusedHeadMixin`` (or with other modes, a batch above one, a portrait
    frame) goes through ``model._downstream_head`` and is copied into its slot."""
    from m3s.config import config

    _encode(model, frame_i)
    _encode(model, frame_j)
    shapes = (frame_i.img_true_shape, frame_j.img_true_shape)
    decs = model._decoder(frame_i.feat, frame_i.pos, frame_j.feat, frame_j.pos)
    step = int(config["dataset"]["img_downsample"])
    stacked = None
    with torch.amp.autocast(enabled=False, device_type="cuda"):
        for v, (dec, shape) in enumerate(zip(decs, shapes)):
            toks = [tok.float() for tok in dec]
            H, W = (int(s) for s in shape.reshape(-1, 2)[0].tolist())
            head = getattr(model, f"downstream_head{v + 1}", None)
            fused = (isinstance(head, FusedHeadMixin) and head.fused_bounds() is not None and H <= W
                     and toks[-1].shape[0] == 1)
            res = None if fused else model._downstream_head(v + 1, toks, shape)
            if stacked is None:
                if fused:
                    Fd = int(head.local_feat_dim)
                else:  # the sizes are the unfused result's
                    Fd, (H, W) = res["desc"].shape[-1], res["pts3d"].shape[1:3]
                Ho, Wo = -(-H // step), -(-W // step)
                dev = toks[-1].device
                stacked = tuple(torch.empty((2, Ho, Wo) + tail, dtype=torch.float32, device=dev)
                                for tail in ((3,), (), (Fd,), ()))
            slot = tuple(t[v:v + 1] for t in stacked)
            if fused:
                head.forward_tail(toks, (H, W), step=step, out=slot)
            else:
                for t, k in zip(slot, ("pts3d", "conf", "desc", "desc_conf")):
                    t[0].copy_(res[k][0][::step, ::step])
    return stacked
