"""CPU: the dense head tail's host side. The export and the argument checks of ``m3s_head_post``, the torch statements
(``postprocess_torch``, ``head_tail_torch``) against the reference's CPU results in tests/golden/head_post.npz
(written by tests/golden/make_head_golden.py), the generators' own expectations, the hook's binding of
``mast3r.catmlp_dpt_head`` and the tracker's ``M3S_HEAD_FUSED`` switch."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as HC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightweight-mast3r-slam_amd")
KW = dict(desc_dim=HC.F_ACC, desc_mode="norm", two_confs=True, desc_conf_mode=HC.DESC_CONF_MODE)


@pytest.fixture(scope="module")
def G(golden):
    return golden("head_post.npz")


def _torch_result(out):
    from m3s.head import postprocess_torch

    res = postprocess_torch(torch.from_numpy(out), HC.DEPTH_MODE, HC.CONF_MODE, **KW)
    assert list(res) == list(HC.KEYS)
    return {k: v.numpy() for k, v in res.items()}


def test_library_exports_head_post_and_the_abi_version_stays_10():
    from m3s import _lib

    header = open(os.path.join(REPO, "include", "m3s.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "m3s_head_post") and "m3s_head_post" in _lib.EXPORTED
    assert re.search(r"\bm3s_head_post\s*\(", header)
    lib.m3s_abi_version.restype = ctypes.c_int
    assert lib.m3s_abi_version() == _lib.ABI_VERSION == 10
    assert int(re.search(r"#define M3S_ABI_VERSION (\d+)", header).group(1)) == 10
    assert (_lib.HEAD_CAT, _lib.HEAD_TOKENS) == tuple(
        int(re.search(r"#define M3S_HEAD_%s (\d+)" % n, header).group(1)) for n in ("CAT", "TOKENS"))


def test_head_post_argument_checks_touch_no_device():
    """Every M3S_EINVAL case with null data pointers: the checks come before the pointers are looked at, so nothing
    can launch. Empty work is OK with null pointers; a good call with null pointers is rejected for them."""
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    inf = float("inf")

    def call(layout=0, B=1, H=16, W=32, Fd=24, tc=1, step=1, c=(1.0, inf), q=(0.0, inf), ptrs=(None,) * 6):
        a, feat, X, C, D, Q = ptrs
        return lib.m3s_head_post(layout, a, feat, B, H, W, Fd, tc, step, c[0], c[1], q[0], q[1], X, C, D, Q, None)

    bad = [dict(layout=2), dict(layout=-1), dict(Fd=0), dict(Fd=33), dict(step=0), dict(step=-2), dict(B=-1),
           dict(layout=1, H=24), dict(layout=1, W=40), dict(c=(1.0, 1.0)), dict(c=(2.0, 1.0)),
           dict(c=(-inf, inf)), dict(c=(float("nan"), inf)), dict(c=(0.0, float("nan"))), dict(q=(3.0, 2.0)),
           dict(B=4, H=4096, W=4608), dict(B=1 << 20, H=1 << 20, W=1 << 20)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert "head_post" in lib.m3s_last_error().decode()
    assert call(tc=0, q=(3.0, 2.0), B=0) == 0  # the desc_conf bounds are read only with two_confs
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(layout=1, B=0)):
        assert call(**kw) == 0, kw
    assert call() == _lib.EINVAL and "null pointer" in lib.m3s_last_error().decode()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert call(layout=1, ptrs=(p, None, p, p, p, p)) == _lib.EINVAL  # TOKENS needs feat
    assert "null pointer" in lib.m3s_last_error().decode()
    assert all(v == 0.0 for v in buf)


def test_fixture_accuracy_case_is_finite_and_spans_the_range(G):
    assert G["acc_out"].shape == (HC.ACC_SHAPE[0], 4 + HC.F_ACC + 1) + HC.ACC_SHAPE[1:]
    assert np.array_equal(G["acc_out"], HC.accuracy_inputs(HC.ACC_SEED, *HC.ACC_SHAPE))
    for k in HC.KEYS:
        assert np.isfinite(G[f"acc_ref32_{k}"]).all() and np.isfinite(G[f"acc_ref64_{k}"]).all()
        assert G[f"acc_ref32_{k}"].dtype == np.float32 and G[f"acc_ref64_{k}"].dtype == np.float64
    d = HC.norm64(G["acc_out"])
    assert d.min() < 0.05 and d.max() > 20.0
    bound, e_ref = HC.bounds(G)
    print("e_ref (2^-24):", e_ref)
    # the reference's own float32 error: a few units, far from the 1e5 of an indexing or formula error
    assert all(0.4 < e_ref[k] < 8.0 for k in HC.KEYS), e_ref


def test_postprocess_torch_matches_the_reference_on_the_accuracy_case(G):
    got = _torch_result(G["acc_out"])
    for k in HC.KEYS:
        assert got[k].shape == G[f"acc_ref32_{k}"].shape and got[k].dtype == np.float32
        np.testing.assert_allclose(got[k], G[f"acc_ref32_{k}"], rtol=1e-6, atol=0)


def test_postprocess_torch_special_values_fall_where_the_reference_puts_them(G):
    assert np.array_equal(G["spc_out"], HC.special_inputs(), equal_nan=True)
    got = _torch_result(G["spc_out"])
    for k in HC.KEYS:
        want = G[f"spc_ref32_{k}"]
        assert np.array_equal(HC.classes(got[k]), HC.classes(want)), k
        fin = HC.classes(want) == 0
        np.testing.assert_allclose(got[k][fin], want[fin], rtol=1e-6, atol=0)
    # what the issue lists, on the reference's result itself
    X, C, D = G["spc_ref32_pts3d"][0, 0], G["spc_ref32_conf"][0, 0], G["spc_ref32_desc"][0, 0]
    assert (X[0] == 0).all()
    np.testing.assert_allclose(X[1], np.array([3e-9, 0, -4e-9]) / 1e-8 * np.expm1(5e-9), rtol=1e-6)
    assert X[2][0] == -np.inf and np.isnan(X[2][1]) and X[2][2] == np.inf
    assert np.isnan(X[3]).all() and np.isnan(X[4]).all()
    assert C[5] == 2.0 and C[6] == np.inf and C[7] == 1.0 and np.isnan(C[8]) and C[9] == np.inf and C[10] == 1.0
    assert np.isfinite(C[11]) and C[11] > 1e38
    assert np.isnan(D[12]).all() and (D[13] == np.inf).all() and (D[14] == 0).all() and np.isnan(D[15]).all()
    assert np.isnan(D[16][7]) and (np.delete(D[16], 7) == 0).all()


def test_postprocess_torch_is_exact_on_the_layout_case(G):
    B, H, W = HC.LAYOUT_SHAPE
    assert np.array_equal(G["lay_out"], HC.layout_inputs(B, H, W))
    got = _torch_result(G["lay_out"])
    for k in HC.KEYS:
        np.testing.assert_array_equal(got[k], G[f"lay_ref32_{k}"])
    # the generator's own expectation agrees with the reference
    exp = HC.layout_expected(B, H, W)
    for k in ("conf", "desc", "desc_conf"):
        np.testing.assert_array_equal(exp[k], G[f"lay_ref32_{k}"])
    X = G["lay_ref32_pts3d"]
    nz = np.zeros(X.shape, dtype=bool)
    np.put_along_axis(nz, exp["x_comp"][..., None], True, axis=-1)
    np.testing.assert_array_equal(X != 0, nz)
    val = np.take_along_axis(X, exp["x_comp"][..., None], axis=-1)[..., 0]
    assert HC.err_units(val, exp["x_val"], np.maximum(1.0, exp["d"])) <= HC.bounds(G)[0]["pts3d"]


@pytest.mark.parametrize("step", [1, 2, 3])
def test_head_tail_torch_is_postprocess_torch_of_the_shuffled_input(G, step):
    from m3s.head import head_tail_torch, postprocess_torch

    out = torch.from_numpy(G["acc_out"])
    B, _, H, W = out.shape
    pts, feat = HC.to_tokens(out)
    assert feat.shape == (B, (H // 16) * (W // 16), 25 * 256)
    # to_tokens inverts the head's own composition
    local = F.pixel_shuffle(feat.transpose(-1, -2).view(B, -1, H // 16, W // 16), 16)
    assert torch.equal(torch.cat([pts, local], dim=1), out)
    want = postprocess_torch(out, HC.DEPTH_MODE, HC.CONF_MODE, **KW)
    got = head_tail_torch(pts, feat, H, W, two_confs=True, conf_mode=HC.CONF_MODE,
                          desc_conf_mode=HC.DESC_CONF_MODE, step=step)
    for g, k in zip(got, HC.KEYS):
        w = want[k][:, ::step, ::step]
        assert g.shape == w.shape and (step == 1 or g.is_contiguous())  # step 1: the reference's permuted views
        assert torch.equal(g.contiguous().view(torch.int32), w.contiguous().view(torch.int32)), k
    # out=: written into slots of a stacked allocation, the neighbours untouched
    stacked = [torch.full((3,) + tuple(g.shape[1:]), -7.0) for g in got]
    ret = head_tail_torch(pts, feat, H, W, two_confs=True, conf_mode=HC.CONF_MODE,
                          desc_conf_mode=HC.DESC_CONF_MODE, step=step, out=tuple(t[1:2] for t in stacked))
    for s, r, g in zip(stacked, ret, got):
        assert r.data_ptr() == s[1:2].data_ptr() and torch.equal(s[1:2], g)
        assert (s[0] == -7.0).all() and (s[2] == -7.0).all()


def test_cpu_calls_take_the_torch_statements_and_other_modes_stay_in_torch(G):
    from m3s import head

    out = torch.from_numpy(G["acc_out"])
    want = head.postprocess_torch(out, HC.DEPTH_MODE, HC.CONF_MODE, **KW)
    got = head.postprocess(out, HC.DEPTH_MODE, HC.CONF_MODE, **KW)
    assert all(torch.equal(got[k], want[k]) for k in HC.KEYS)
    pts, feat = HC.to_tokens(out)
    X, C, D, Q = head.head_tail(pts, feat, 32, 48, two_confs=True, conf_mode=HC.CONF_MODE,
                                desc_conf_mode=HC.DESC_CONF_MODE)
    assert torch.equal(X, want["pts3d"]) and torch.equal(D, want["desc"])
    inf = float("inf")
    assert head.device_modes(HC.DEPTH_MODE, ("exp", 1, 5), "norm", True, None) == ((1.0, 5.0), (1.0, 5.0))
    assert head.device_modes(HC.DEPTH_MODE, HC.CONF_MODE, "norm", False, ("sigmoid", 0, 1)) == ((1.0, inf), (1.0, inf))
    for modes in ((("linear", -inf, inf), HC.CONF_MODE, "norm", True, None),
                  (("square", -inf, inf), HC.CONF_MODE, "norm", True, None),
                  (HC.DEPTH_MODE, ("sigmoid", 0, 1), "norm", True, None),
                  (HC.DEPTH_MODE, ("exp", 1, 1), "norm", True, None),
                  (HC.DEPTH_MODE, ("exp", -inf, inf), "norm", True, None),
                  (HC.DEPTH_MODE, None, "norm", True, None),
                  (HC.DEPTH_MODE, HC.CONF_MODE, "norm", True, ("sigmoid", 0, 1)),
                  (HC.DEPTH_MODE, HC.CONF_MODE, "norm_l2", True, None)):
        assert head.device_modes(*modes) is None, modes
    res = head.postprocess(out, ("square", -inf, inf), ("sigmoid", 0, 2), desc_dim=24, two_confs=False)
    assert res["conf"].max() <= 2 and torch.equal(res["desc_conf"], res["conf"])
    assert list(head.postprocess(out, HC.DEPTH_MODE, HC.CONF_MODE)) == ["pts3d", "conf"]
    with pytest.raises(RuntimeError, match="multiples of 16"):
        head.head_tail(pts, feat, 24, 64, two_confs=True, conf_mode=HC.CONF_MODE)
    with pytest.raises(RuntimeError, match="out X has shape"):
        head.head_tail_torch(pts, feat, 32, 48, two_confs=True, conf_mode=HC.CONF_MODE,
                             out=(torch.empty(1, 3, 3, 3), C, D, Q))


def test_hook_binds_postprocess_and_the_head_class(tmp_path):
    """On a stand-in ``mast3r.catmlp_dpt_head``: the module's ``postprocess`` is m3s.head's and its head class a
    subclass of itself with FusedHeadMixin in front, as a model factory inside that module sees them; without the hook
    directory nothing changes."""
    ref = tmp_path / "ref" / "mast3r"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "catmlp_dpt_head.py").write_text(textwrap.dedent("""
        def postprocess(out, depth_mode, conf_mode, desc_dim=None, desc_mode='norm', two_confs=False,
                        desc_conf_mode=None):
            return "reference postprocess"
        class Cat_MLP_LocalFeatures_DPT_Pts3d:
            def __init__(self, post):
                self.postprocess = post
            def forward(self, decout, img_shape):
                return "reference forward"
        def mast3r_head_factory():
            return Cat_MLP_LocalFeatures_DPT_Pts3d(postprocess)
    """))
    main = tmp_path / "main.py"
    main.write_text(textwrap.dedent("""
        import mast3r.catmlp_dpt_head as M
        import m3s.head
        from m3s.head import FusedHeadMixin
        head = M.mast3r_head_factory()
        assert M.postprocess is m3s.head.postprocess and head.postprocess is m3s.head.postprocess
        assert type(head) is M.Cat_MLP_LocalFeatures_DPT_Pts3d
        assert type(head).__name__ == "Cat_MLP_LocalFeatures_DPT_Pts3d" and type(head).__mro__[1] is FusedHeadMixin
        assert type(head).forward is FusedHeadMixin.forward
        head.postprocess = None  # no postprocess: the reference's forward
        assert head.forward(None, (16, 16)) == "reference forward"
        print("HOOK_OK")
    """))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(PKG, "m3s_hook"), PKG, str(tmp_path / "ref")]))
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "HOOK_OK" in r.stdout
    env["PYTHONPATH"] = os.pathsep.join([PKG, str(tmp_path / "ref")])
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "AssertionError" in r.stderr


def test_tracker_inference_leaves_m3s_head_alone_unless_switched_on():
    """With M3S_HEAD_FUSED unset, m3s.tracker.asymmetric_inference goes to the reference's helper and never imports
    m3s.head; with M3S_HEAD_FUSED=1 it calls m3s.head.asymmetric_inference. A model with its own
    ``asymmetric_inference`` answers either way. (In a process of its own: sys.modules is the evidence.)"""
    script = textwrap.dedent("""
        import os, sys, types
        import m3s.tracker as T
        ref = types.ModuleType("mast3r_slam.mast3r_utils")
        ref.mast3r_asymmetric_inference = lambda model, fi, fj: "reference helper"
        sys.modules["mast3r_slam"] = types.ModuleType("mast3r_slam")
        sys.modules["mast3r_slam.mast3r_utils"] = ref
        class Own:
            def asymmetric_inference(self, fi, fj):
                return "own"
        os.environ.pop("M3S_HEAD_FUSED", None)
        assert T.asymmetric_inference(object(), None, None) == "reference helper"
        os.environ["M3S_HEAD_FUSED"] = "0"
        assert T.asymmetric_inference(object(), None, None) == "reference helper"
        assert "m3s.head" not in sys.modules
        os.environ["M3S_HEAD_FUSED"] = "1"
        assert T.asymmetric_inference(Own(), None, None) == "own"
        assert "m3s.head" not in sys.modules
        import m3s.head
        m3s.head.asymmetric_inference = lambda model, fi, fj: "fused"
        assert T.asymmetric_inference(object(), None, None) == "fused"
        print("SWITCH_OK")
    """)
    env = dict(os.environ, PYTHONPATH=PKG)
    env.pop("M3S_HEAD_FUSED", None)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SWITCH_OK" in r.stdout
