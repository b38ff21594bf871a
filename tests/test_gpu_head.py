"""GPU: the dense head tail (m3s_head_post behind m3s.head) against tests/head_cases.py and the reference's CPU results
in tests/golden/head_post.npz.

Layout cases are exact on any correct implementation and are compared with ``assert_array_equal`` over every pixel.
Accuracy is measured against the fixture's float64 result in units of 2^-24 (``head_cases.err_units``); the bound per
output is 2 e_ref + 1 with e_ref the same figure of the reference's own float32 result, computed from the fixture.
Every case is at most a few thousand pixels."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import head_cases as HC
from m3s import head
from m3s.config import config

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
MODES = dict(conf_mode=HC.CONF_MODE, desc_conf_mode=HC.DESC_CONF_MODE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the head tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G(golden):
    return golden("head_post.npz")


def _np(ts):
    return dict(zip(HC.KEYS, (t.cpu().numpy() for t in ts)))


def _check_layout(got, B, H, W, Fd, tc, step, bound_x):
    exp = HC.layout_expected(B, H, W, Fd, bool(tc), step=step)
    Ho, Wo = -(-H // step), -(-W // step)
    assert got["pts3d"].shape == (B, Ho, Wo, 3) and got["desc"].shape == (B, Ho, Wo, Fd)
    for k in ("conf", "desc", "desc_conf"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    X = got["pts3d"]
    nz = np.zeros(X.shape, dtype=bool)
    np.put_along_axis(nz, exp["x_comp"][..., None], True, axis=-1)
    np.testing.assert_array_equal(X != 0, nz)
    val = np.take_along_axis(X, exp["x_comp"][..., None], axis=-1)[..., 0]
    e = HC.err_units(val, exp["x_val"], np.maximum(1.0, exp["d"]))
    assert e <= bound_x, f"X: {e:.2f} > {bound_x:.2f} (2^-24)"


@pytest.mark.parametrize("Fd, tc", [(24, 1), (24, 0), (5, 1), (1, 0), (32, 1), (8, 0)])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (2, 17, 65), (1, 16, 16), (2, 9, 68)])
def test_layout_cat(dev, G, shape, step, Fd, tc):
    """One block and less, and (2, 17, 65), (2, 9, 68): several blocks with a partial last one; F a multiple of four
    (16-byte D stores, every register group: 8, 24, 32) and not (scalar stores)."""
    B, H, W = shape
    out = torch.from_numpy(HC.layout_inputs(B, H, W, Fd, bool(tc))).to(dev)
    got = _np(head.cat_tail(out, Fd, two_confs=bool(tc), step=step, **MODES))
    _check_layout(got, B, H, W, Fd, tc, step, HC.bounds(G)[0]["pts3d"])
    if step == 1:  # the reference-signature entry is the same launch
        res = head.postprocess(out, HC.DEPTH_MODE, HC.CONF_MODE, desc_dim=Fd, two_confs=bool(tc),
                               desc_conf_mode=HC.DESC_CONF_MODE)
        assert list(res) == list(HC.KEYS)
        for k in HC.KEYS:
            np.testing.assert_array_equal(res[k].cpu().numpy(), got[k])


@pytest.mark.parametrize("tc", [1, 0])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 16, 16), (1, 16, 48), (2, 48, 32)])
def test_layout_tokens(dev, G, shape, step, tc):
    B, H, W = shape
    pts, feat = HC.to_tokens(torch.from_numpy(HC.layout_inputs(B, H, W, 24, bool(tc))))
    got = _np(head.head_tail(pts.to(dev), feat.to(dev), H, W, two_confs=bool(tc), step=step, **MODES))
    _check_layout(got, B, H, W, 24, tc, step, HC.bounds(G)[0]["pts3d"])


def _mixed_input(G):
    """(2, 29, 32, 48): accuracy inputs with the special-value pixels stamped into the first row of each image."""
    out = HC.accuracy_inputs(11, 2, 32, 48)
    spc = G["spc_out"]
    out[:, :, 0, :spc.shape[-1]] = spc[0, :, 0]
    return torch.from_numpy(out)


@pytest.mark.parametrize("step", [1, 2, 5])
def test_tokens_equal_cat_bit_for_bit(dev, G, step):
    out = _mixed_input(G)
    pts, feat = HC.to_tokens(out)
    a = head.cat_tail(out.to(dev), 24, two_confs=True, step=step, **MODES)
    b = head.head_tail(pts.to(dev), feat.to(dev), 32, 48, two_confs=True, step=step, **MODES)
    for x, y, k in zip(a, b, HC.KEYS):
        assert x.shape == y.shape
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    if step == 1:  # the special pixels are in
        assert torch.isnan(a[0]).any() and torch.isinf(a[2]).any() and torch.isnan(a[3]).any()


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("layout", ["cat", "tokens"])
def test_out_slots_of_a_stacked_allocation(dev, G, layout, step, misalign):
    """Results written through out= into slot 1 of (3, H', W', .) allocations equal the returned tensors of a plain
    call, and slots 0 and 2 keep their sentinel. misalign: the allocations start one float into a buffer, so D is not
    16-byte aligned and takes the scalar stores, against the plain call's 16-byte ones; same bits."""
    out = torch.from_numpy(G["acc_out"]).to(dev)
    _, _, H, W = out.shape
    Ho, Wo = H // step, W // step
    pts, feat = (t.to(dev) for t in HC.to_tokens(out.cpu()))

    def run(o):
        if layout == "cat":
            return head.cat_tail(out, 24, two_confs=True, step=step, out_tensors=o, **MODES)
        return head.head_tail(pts, feat, H, W, two_confs=True, step=step, out=o, **MODES)

    plain = run(None)
    stacked = []
    for tail in ((3,), (), (24,), ()):
        n = 3 * Ho * Wo * int(np.prod(tail, dtype=np.int64))
        flat = torch.full((n + misalign,), SENTINEL, device=dev)
        stacked.append(flat[misalign:].view((3, Ho, Wo) + tail))
    assert (stacked[2].data_ptr() % 16 != 0) == bool(misalign)
    ret = run(tuple(t[1:2] for t in stacked))
    for s, r, p in zip(stacked, ret, plain):
        assert r.data_ptr() == s[1:2].data_ptr()
        assert torch.equal(s[1:2].view(torch.int32), p.view(torch.int32))
        assert (s[0] == SENTINEL).all() and (s[2] == SENTINEL).all()
    bad = [t[1:2] for t in stacked]
    bad[2] = stacked[2][1:2, :, :, :23]
    with pytest.raises(RuntimeError, match="out D has shape"):
        run(tuple(bad))
    bad[2] = stacked[2][1:2].double()
    with pytest.raises(RuntimeError, match="out D must be"):
        run(tuple(bad))
    bad[2] = stacked[2][1:2].cpu()
    with pytest.raises(RuntimeError, match="out D must be"):
        run(tuple(bad))


def test_non_default_stream_and_finite_vmax(dev, G):
    out = torch.from_numpy(G["acc_out"]).to(dev)
    want = head.cat_tail(out, 24, two_confs=True, **MODES)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = head.cat_tail(out, 24, two_confs=True, **MODES)
    s.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # ('exp', 1, 5): C = 1 + min(exp(l), 4), so exactly 5 where exp(l) exceeds 4
    X, C, D, Q = head.cat_tail(out, 24, two_confs=True, conf_mode=("exp", 1, 5), desc_conf_mode=("exp", -2.5, 0.5))
    e_c, e_q = out[:, 3].double().exp(), out[:, 28].double().exp()
    tol = 1e-5  # the device's exp is within a few 2^-24 of the float64 one
    assert (C[e_c > 4.0 * (1 + tol)] == 5.0).all() and (C[e_c < 4.0 * (1 - tol)] < 5.0).all()
    assert (C <= 5.0).all() and (C >= 1.0).all() and (C == 5.0).any() and (C < 5.0).any()
    assert torch.equal(C[C < 5.0], want[1][C < 5.0])
    assert (Q[e_q > 3.0 * (1 + tol)] == 0.5).all() and (Q[e_q < 3.0 * (1 - tol)] < 0.5).all()
    assert (Q <= 0.5).all() and (Q >= -2.5).all() and (Q == 0.5).any() and (Q < 0.5).any()
    assert torch.equal(X, want[0]) and torch.equal(D, want[2])
    # without two_confs Q is C's bits and channel 28 is not there
    X1, C1, D1, Q1 = head.cat_tail(out[:, :28], 24, two_confs=False, conf_mode=HC.CONF_MODE)
    assert torch.equal(C1, want[1]) and torch.equal(Q1.view(torch.int32), C1.view(torch.int32))
    assert Q1.data_ptr() != C1.data_ptr() and torch.equal(D1, want[2])


def _check_accuracy(got, G, prefix, what):
    """Same NaN / +inf / -inf / zero positions as the reference's float32 result; its finite non-zero values within the
    bound of the float64 result."""
    bound, _ = HC.bounds(G)
    sc = HC.scales(G[prefix + "_out"])
    for k in HC.KEYS:
        ref32, ref64 = G[f"{prefix}_ref32_{k}"], G[f"{prefix}_ref64_{k}"]
        cls = HC.classes(ref32)
        np.testing.assert_array_equal(HC.classes(got[k]), cls, err_msg=f"{what} {k}")
        e = HC.err_units(got[k], ref64, sc[k], where=cls == 0)
        print(f"{what} {k}: {e:.2f} (bound {bound[k]:.2f}) * 2^-24")
        assert e <= bound[k], f"{what} {k}: {e:.2f} > {bound[k]:.2f} (2^-24)"


def test_accuracy_against_the_float64_result(dev, G):
    out = torch.from_numpy(G["acc_out"])
    _check_accuracy(_np(head.cat_tail(out.to(dev), 24, two_confs=True, **MODES)), G, "acc", "CAT")
    pts, feat = HC.to_tokens(out)
    _check_accuracy(_np(head.head_tail(pts.to(dev), feat.to(dev), 32, 48, two_confs=True, **MODES)), G, "acc", "TOKENS")


def test_special_values(dev, G):
    out = torch.from_numpy(G["spc_out"]).to(dev)
    _check_accuracy(_np(head.cat_tail(out, 24, two_confs=True, **MODES)), G, "spc", "special")


def test_gradients_and_other_dtypes_take_the_torch_route(dev, G):
    out = torch.from_numpy(G["lay_out"]).to(dev)
    kw = dict(desc_dim=24, two_confs=True, desc_conf_mode=HC.DESC_CONF_MODE)
    res = head.postprocess(out.clone().requires_grad_(), HC.DEPTH_MODE, HC.CONF_MODE, **kw)
    assert res["desc"].requires_grad
    with torch.no_grad():
        assert not head.postprocess(out.clone().requires_grad_(), HC.DEPTH_MODE, HC.CONF_MODE, **kw)["desc"].requires_grad
    assert head.postprocess(out.double(), HC.DEPTH_MODE, HC.CONF_MODE, **kw)["desc"].dtype == torch.float64
    with pytest.raises(RuntimeError, match="float32"):
        head.cat_tail(out.double(), 24, two_confs=True, **MODES)
    with pytest.raises(RuntimeError, match="HIP device"):
        head.cat_tail(out.cpu(), 24, two_confs=True, **MODES)


# ---- FusedHeadMixin and asymmetric_inference on a stand-in head and model ----

DIM = 8


class StandInHead(nn.Module):
    """The head's surface with the unfused tail: dpt = a fixed random 1 x 1 conv + upsample, head_local_features = a
    Linear, then head_tail_torch."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = nn.Conv2d(DIM, 4, 1)
        self.head_local_features = nn.Linear(2 * DIM, 25 * 256)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        self.patch_size, self.local_feat_dim, self.two_confs = 16, 24, True
        self.depth_mode, self.conf_mode, self.desc_mode, self.desc_conf_mode = (
            HC.DEPTH_MODE, HC.CONF_MODE, "norm", HC.DESC_CONF_MODE)
        self.postprocess = head.postprocess

    def dpt(self, decout, image_size):
        H, W = image_size
        B, S, D = decout[-1].shape
        x = decout[-1].transpose(1, 2).reshape(B, D, H // 16, W // 16)
        return F.interpolate(self.conv(x), size=(H, W), mode="bilinear", align_corners=False)

    def forward(self, decout, img_shape):
        H, W = img_shape
        pts = self.dpt(decout, image_size=(H, W))
        feat = self.head_local_features(torch.cat([decout[0], decout[-1]], dim=-1))
        X, C, D, Q = head.head_tail_torch(pts, feat, H, W, two_confs=True, **MODES)
        return dict(pts3d=X, conf=C, desc=D, desc_conf=Q)


class FusedStandInHead(head.FusedHeadMixin, StandInHead):
    pass


class StandInModel:
    def __init__(self, cls, dev):
        self.downstream_head1, self.downstream_head2 = cls(1).to(dev), cls(2).to(dev)
        self.proj = torch.randn(3, DIM, generator=torch.Generator().manual_seed(3)).to(dev)

    def _encode_image(self, img, true_shape):
        tok = F.avg_pool2d(img, 16).flatten(2).transpose(1, 2) @ self.proj  # (1, S, DIM)
        return tok, None, None

    def _decoder(self, f1, p1, f2, p2):
        return [f1, 0.5 * f1 + 0.5 * f2], [f2, 0.5 * f2 - 0.5 * f1]

    def _downstream_head(self, n, decout, shape):
        H, W = shape.reshape(-1, 2)[0].tolist()
        return getattr(self, f"downstream_head{n}")(decout, (H, W))


def _frames(dev):
    from m3s.frame import Frame

    g = torch.Generator().manual_seed(4)
    shape = torch.tensor([[32, 48]], dtype=torch.int32)
    return [Frame(i, (32, 48), img=(torch.randn(1, 3, 32, 48, generator=g) * 2).to(dev), img_true_shape=shape)
            for i in range(2)]


def _check_views(got, calls, G, step, what):
    """got: X, C, D, Q (2, H', W', .); calls: the (pts, feat) the tail received per view. Truth: the stock tail in
    float64 on the CPU from those very inputs."""
    bound, _ = HC.bounds(G)
    assert len(calls) == 2
    for v, (pts, feat) in enumerate(calls):
        truth = head.head_tail_torch(pts.double().cpu(), feat.double().cpu(), 32, 48, two_confs=True, step=step, **MODES)
        cat = torch.cat([pts.cpu(), F.pixel_shuffle(feat.cpu().transpose(-1, -2).reshape(1, -1, 2, 3), 16)], dim=1)
        sc = HC.scales(cat[:, :, ::step, ::step].numpy())
        for t, g, k in zip(truth, got, HC.KEYS):
            assert g.shape[0] == 2 and g[v].shape == t[0].shape and g.is_contiguous()
            e = HC.err_units(g[v].cpu().numpy(), t[0].numpy(), None if sc[k] is None else sc[k][0])
            print(f"{what} view {v} {k}: {e:.2f} (bound {bound[k]:.2f}) * 2^-24")
            assert e <= bound[k], f"{what} view {v} {k}: {e:.2f} > {bound[k]:.2f}"


@pytest.fixture
def tail_calls(monkeypatch):
    calls = []
    real = head.head_tail

    def recording(pts, feat, H, W, **kw):
        calls.append((pts.clone(), feat.clone()))
        return real(pts, feat, H, W, **kw)

    monkeypatch.setattr(head, "head_tail", recording)
    return calls


def test_fused_head_mixin_forward(dev, G, tail_calls):
    model = StandInModel(FusedStandInHead, dev)
    fi, fj = _frames(dev)
    with torch.no_grad():
        f1, _, _ = model._encode_image(fi.img, fi.img_true_shape)
        f2, _, _ = model._encode_image(fj.img, fj.img_true_shape)
        dec1, dec2 = model._decoder(f1, None, f2, None)
        res = [model.downstream_head1(dec1, (32, 48)), model.downstream_head2(dec2, (32, 48))]
        assert all(list(r) == list(HC.KEYS) for r in res)
        assert res[0]["pts3d"].shape == (1, 32, 48, 3) and res[0]["desc"].shape == (1, 32, 48, 24)
        got = tuple(torch.cat([r[k] for r in res]) for k in HC.KEYS)
        _check_views(got, tail_calls, G, 1, "forward")
        # other modes or no postprocess: the class behind the mixin answers
        h = model.downstream_head1
        h.conf_mode = ("sigmoid", 0, 1)
        assert h.fused_bounds() is None
        n = len(tail_calls)
        h.forward(dec1, (32, 48))
        h.conf_mode, h.postprocess = HC.CONF_MODE, None
        h.forward(dec1, (32, 48))
        assert len(tail_calls) == n


@pytest.mark.parametrize("step", [1, 2])
def test_asymmetric_inference_writes_both_views_into_one_allocation(dev, G, tail_calls, monkeypatch, step):
    """m3s.head.asymmetric_inference with img_downsample as the kernel's step, reached through the tracker's inference
    path with M3S_HEAD_FUSED=1; the same call on unfused heads (the copy route) agrees."""
    import m3s.tracker as T

    config["dataset"]["img_downsample"] = step
    monkeypatch.setenv("M3S_HEAD_FUSED", "1")
    got = T.asymmetric_inference(StandInModel(FusedStandInHead, dev), *_frames(dev))
    Ho, Wo = 32 // step, 48 // step
    assert [tuple(t.shape) for t in got] == [(2, Ho, Wo, 3), (2, Ho, Wo), (2, Ho, Wo, 24), (2, Ho, Wo)]
    _check_views(got, tail_calls, G, step, f"inference step {step}")
    n = len(tail_calls)
    unfused = T.asymmetric_inference(StandInModel(StandInHead, dev), *_frames(dev))
    assert len(tail_calls) == n  # no kernel on that route
    for g, u in zip(got, unfused):
        assert g.shape == u.shape
        torch.testing.assert_close(g, u, rtol=1e-4, atol=1e-6)
