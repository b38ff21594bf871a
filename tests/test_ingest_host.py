"""CPU: the frame ingest's host side. tests/ingest_cases.py's restatement (the device test's bit reference) against
Pillow, live and from tests/golden/ingest.npz; the library's coefficient tables and geometry against the restatement's;
the package's host ``resize_img`` against a direct Pillow + torch statement; ``create_frame`` behind the start-up hook;
the exports and the argument checks. Every comparison is equality."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import ingest_cases as IC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightweight-mast3r-slam_amd")
ALL = IC.CASES + [IC.LEVELS]
IDS = [IC.case_id(c) for c in ALL]


@pytest.fixture(scope="module")
def G(golden):
    return golden("ingest.npz")


def _pillow(u8, g):
    import PIL.Image

    img = PIL.Image.fromarray(u8).resize(g["resized"], PIL.Image.LANCZOS if g["filter"] == IC.LANCZOS
                                         else PIL.Image.BICUBIC)
    return np.asarray(img.crop(g["crop"]))


def test_float_round_trip_is_the_identity_on_all_levels():
    """uint8(float32(u) / 255 * 255) == u: a uint8 source and the reference's float source give the same bytes."""
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(np.uint8(IC.to_float(u) * 255), u)


def test_numpy_tail_is_torchs():
    """The restatement's tail (numpy float32) and the host statement's torch ops agree on all 256 levels, bit for bit."""
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    img, uimg = IC.tail(u)
    t = torch.from_numpy(u).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)
    assert np.array_equal(t.numpy().view(np.uint32), img.view(np.uint32))
    assert np.array_equal((torch.from_numpy(u) / 255.0).numpy().view(np.uint32), uimg.view(np.uint32))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_restatement_equals_the_fixture(G, case):
    src, g, rgb = IC.restate(*case)
    cid = IC.case_id(case)
    assert tuple(G[cid + "/shape"]) == rgb.shape == (g["out"][1], g["out"][0], 3)
    assert tuple(G[cid + "/resized"]) == g["resized"] and tuple(G[cid + "/crop"]) == g["crop"]
    assert tuple(G[cid + "/transformation"]) == g["transformation"]
    assert hashlib.sha256(rgb.tobytes()).hexdigest() == str(G[cid + "/sha256"])
    if cid + "/rgb" in G:
        np.testing.assert_array_equal(rgb, G[cid + "/rgb"])
    else:
        assert rgb.nbytes > 32 * 1024
    assert rgb.min() < rgb.max() and not np.array_equal(rgb, rgb[::-1])


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_restatement_equals_pillow_live(case):
    pytest.importorskip("PIL")
    src, g, rgb = IC.restate(*case)
    got = _pillow(src, g)
    assert got.shape == rgb.shape
    n_diff = int((got != rgb).sum())
    print(f"{IC.case_id(case)}: {n_diff} of {rgb.size} bytes differ from Pillow's")
    assert n_diff == 0


@pytest.mark.parametrize("filt", [IC.BICUBIC, IC.LANCZOS], ids=["bicubic", "lanczos"])
def test_library_table_equals_the_restatement(filt):
    from m3s import _lib

    for n_in, n_out in IC.TABLE_PAIRS:
        xmin, n, k = _lib.ingest_table(n_in, n_out, filt)
        want = IC.table(n_in, n_out, filt)
        assert k.shape == want[2].shape == (n_out, IC.ksize_of(n_in, n_out, filt)), (n_in, n_out)
        for got, w, what in zip((xmin, n, k), want, ("xmin", "n", "k")):
            np.testing.assert_array_equal(got, w, err_msg=f"{what} of {n_in} -> {n_out}")
        assert (n >= 1).all() and (xmin >= 0).all() and (xmin + n <= n_in).all()
        # a row sums to 2^22 within its taps' roundings
        assert (np.abs(k.sum(axis=1, dtype=np.int64) - (1 << IC.PRECISION_BITS)) <= n).all()


def _assert_geometry(H1, W1, size, sq, lib, g, byref):
    from m3s import _lib

    want = IC.geometry(H1, W1, size, sq)
    rc = lib.m3s_ingest_geometry(H1, W1, size, int(sq), byref)
    if want is None:
        assert rc == _lib.EINVAL, (H1, W1, size, sq)
        return 0
    assert rc == 0, (H1, W1, size, sq)
    got = ((g.resized_w, g.resized_h), g.filter, (g.crop_x0, g.crop_y0, g.crop_x1, g.crop_y1), (g.out_w, g.out_h),
           (g.scale_w, g.scale_h, g.half_crop_w, g.half_crop_h))
    assert got == (want["resized"], want["filter"], want["crop"], want["out"], want["transformation"]), (H1, W1, size, sq)
    return 1


@pytest.mark.parametrize("size", [512, 224])
def test_library_geometry_equals_the_python_statement(size):
    """Every H1, W1 in 1..300 and the GPU cases' sizes, both square_ok values; an error exactly where the crop is
    empty (at size 224 the short side becomes 224, so no crop is)."""
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    g = _lib.IngestGeom()
    byref = ctypes.byref(g)
    shapes = [(h, w) for h in range(1, 301) for w in range(1, 301)] + [c[:2] for c in ALL] + [(1080, 1920), (16384, 1)]
    ok = empty = 0
    for H1, W1 in shapes:
        for sq in (False, True):
            r = _assert_geometry(H1, W1, size, sq, lib, g, byref)
            ok, empty = ok + r, empty + 1 - r
    print(f"size {size}: {ok} geometries equal, {empty} empty crops rejected")
    assert ok > 0 and (empty > 0) == (size == 512)
    if size == 512:
        assert "crop is empty" in lib.m3s_last_error().decode()  # (16384, 1) came last


def test_geometry_of_the_package():
    from m3s.ingest import geometry

    g = geometry(480, 640)
    assert g.resized == (512, 384) and g.filter == IC.LANCZOS and g.crop == (0, 0, 512, 384) and g.out_size == (512, 384)
    assert g.transformation == (1.25, 1.25, 0.0, 0.0)
    assert geometry(600, 600).out_size == (512, 384) and geometry(600, 600, square_ok=True).out_size == (512, 512)
    with pytest.raises(RuntimeError, match="crop is empty"):
        geometry(1, 300)
    with pytest.raises(RuntimeError, match="size must be 512 or 224"):
        geometry(480, 640, size=256)


@pytest.mark.parametrize("case", [(37, 53, 512, False), (600, 600, 512, False), (300, 400, 224, False),
                                  (480, 640, 512, False)], ids=IC.case_id)
def test_host_resize_img_equals_pillow_and_torch_ops(case):
    """The package's host statement against Pillow + torch ops written here, from the float image the reference's
    loaders make and from the uint8 image itself."""
    pytest.importorskip("PIL")
    from m3s.ingest import resize_img

    src, g, rgb = IC.restate(*case)
    want_u8 = _pillow(src, g)
    want_img = torch.from_numpy(want_u8.copy()).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)[None]
    for image in (IC.to_float(src), src, torch.from_numpy(IC.to_float(src))):
        res, tf = resize_img(image, case[2], square_ok=case[3], return_transformation=True)
        assert set(res) == {"img", "true_shape", "unnormalized_img"}
        assert res["img"].dtype == torch.float32 and res["img"].shape == (1, 3, g["out"][1], g["out"][0])
        assert torch.equal(res["img"].view(torch.int32), want_img.view(torch.int32))
        assert res["true_shape"].dtype == np.int32 and res["true_shape"].tolist() == [[g["out"][1], g["out"][0]]]
        assert res["unnormalized_img"].dtype == np.uint8
        np.testing.assert_array_equal(res["unnormalized_img"], rgb)
        assert tf == g["transformation"]
    assert isinstance(resize_img(src, case[2], square_ok=case[3]), dict)
    # and the restatement's tail is that tensor
    np.testing.assert_array_equal(IC.tail(rgb)[0].view(np.uint32), want_img[0].numpy().view(np.uint32))


def test_host_paths_reject_bad_arguments():
    from m3s.ingest import ingest, resize_img

    src = IC.make_image(37, 53)
    with pytest.raises(RuntimeError, match="size must be 512 or 224"):
        resize_img(src, 256)
    with pytest.raises(RuntimeError, match="must be a HIP device"):
        ingest(src, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            ingest(src, device="cuda:0")


_FRAME_STANDIN = """
import dataclasses
import torch

@dataclasses.dataclass
class Frame:
    frame_id: int
    img: torch.Tensor
    img_shape: torch.Tensor
    img_true_shape: torch.Tensor
    uimg: torch.Tensor
    T_WC: object = None

def create_frame(i, img, T_WC, img_size=512, device="cuda:0"):
    raise AssertionError("the stand-in's create_frame ran")
"""

_FRAME_MAIN = """
import sys
import numpy as np
import torch
from mast3r_slam.frame import Frame, create_frame
import m3s.ingest
from m3s.config import config
sys.path.insert(0, %(tests)r)
import ingest_cases as IC
assert create_frame is m3s.ingest.create_frame, create_frame
src, g, rgb = IC.restate(37, 53, 512, False)
want_img, _ = IC.tail(rgb)
for ds in (1, 3):
    config["dataset"]["img_downsample"] = ds
    for image in (IC.to_float(src), src):
        f = create_frame(7, image, "pose", img_size=512, device="cpu")
        assert type(f) is Frame and f.frame_id == 7 and f.T_WC == "pose"
        assert f.img.shape == (1, 3, 352, 512) and np.array_equal(f.img[0].numpy().view(np.uint32), want_img.view(np.uint32))
        assert f.img_true_shape.dtype == torch.int32 and f.img_true_shape.tolist() == [[352, 512]]
        assert f.img_shape.dtype == torch.int32 and f.img_shape.tolist() == [[352 // ds, 512 // ds]]
        want_uimg = (torch.from_numpy(rgb.copy()) / 255.0)[::ds, ::ds]
        assert f.uimg.dtype == torch.float32 and f.uimg.device.type == "cpu" and torch.equal(f.uimg, want_uimg)
        assert np.array_equal(f.uimg.numpy().view(np.uint32), IC.tail(rgb, ds)[1].view(np.uint32))
print("FRAME_OK")
"""


def test_hook_swaps_create_frame_and_builds_the_reference_frame(tmp_path):
    """On a stand-in ``mast3r_slam`` package (tests/test_hook.py's kind): ``from mast3r_slam.frame import create_frame``
    binds the package's, which builds the stand-in's ``Frame`` positionally; with M3S_INGEST_FUSED unset its fields are
    the host statement's."""
    pytest.importorskip("PIL")
    ref = tmp_path / "ref" / "mast3r_slam"
    ref.mkdir(parents=True)
    (ref / "__init__.py").write_text("")
    (ref / "frame.py").write_text(textwrap.dedent(_FRAME_STANDIN))
    main = tmp_path / "main.py"
    main.write_text(_FRAME_MAIN % dict(tests=os.path.join(REPO, "tests")))
    env = {k: v for k, v in os.environ.items() if k != "M3S_INGEST_FUSED"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(PKG, "m3s_hook"), PKG, str(tmp_path / "ref")])
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "FRAME_OK" in r.stdout
    env["PYTHONPATH"] = os.pathsep.join([PKG, str(tmp_path / "ref")])  # without the hook directory nothing changes
    r = subprocess.run([sys.executable, str(main)], env=env, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode != 0 and "AssertionError" in r.stderr


def test_create_frame_without_the_reference_builds_the_packages_frame(monkeypatch):
    pytest.importorskip("PIL")
    monkeypatch.delitem(sys.modules, "mast3r_slam.frame", raising=False)
    from m3s.frame import Frame
    from m3s.ingest import create_frame
    from m3s.sim3 import Sim3

    src, g, rgb = IC.restate(37, 53, 512, False)
    T = Sim3.Identity(1)
    f = create_frame(3, IC.to_float(src), T, device="cpu")
    assert type(f) is Frame and f.frame_id == 3 and f.img_size == (352, 512) and f.T_WC is T
    assert np.array_equal(f.img[0].numpy().view(np.uint32), IC.tail(rgb)[0].view(np.uint32))
    assert f.img_shape.tolist() == f.img_true_shape.tolist() == [[352, 512]]
    assert np.array_equal(f.uimg.numpy().view(np.uint32), IC.tail(rgb)[1].view(np.uint32))


def test_ingest_exports_and_abi_version():
    from m3s import _lib
    from m3s.hook import PATCHES

    header = open(os.path.join(REPO, "include", "m3s.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("m3s_ingest_geometry", "m3s_ingest_table", "m3s_ingest_prepare", "m3s_ingest_release",
              "m3s_ingest_workspace_size", "m3s_ingest"):
        assert hasattr(lib, s) and s in _lib.EXPORTED and re.search(r"\b%s\s*\(" % s, header), s
    lib.m3s_abi_version.restype = ctypes.c_int
    assert lib.m3s_abi_version() == _lib.ABI_VERSION == 10
    assert int(re.search(r"#define M3S_ABI_VERSION (\d+)", header).group(1)) == 10
    assert re.search(r"head_post, ingest\. query", header)  # the span's name is in the header's list
    assert PATCHES["mast3r_slam.frame"] == ("create_frame", "m3s.ingest")


def test_workspace_size_covers_the_mid_image():
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    size = lambda *a: lib.m3s_ingest_workspace_size(*a)  # noqa: E731
    assert size(480, 640, 512, 0, 1) >= 480 * 512 * 3 and size(480, 640, 512, 0, 1) % 256 == 0
    assert size(480, 640, 512, 0, 2) >= 2 * 480 * 512 * 3
    assert size(512, 384, 512, 0, 1) == 512 * 384 * 3  # no resize: the crop itself
    assert size(23, 512, 512, 0, 1) == 16 * 512 * 3    # only the rows the crop reads
    assert size(1, 300, 512, 0, 1) == 0 and size(480, 640, 100, 0, 1) == 0 and size(480, 640, 512, 0, -1) == 0
    assert size(1080, 1920, 512, 0, 1) <= 1080 * 512 * 3 + 256


def test_abi_argument_checks_touch_no_device():
    """M3S_EINVAL with a message before any HIP call; B == 0 is fine and launches nothing."""
    from m3s import _lib

    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def call(ws=p, ws_bytes=1 << 30, **kw):
        a = dict(src=p, src_dtype=0, row_stride=53 * 3, B=1, H1=37, W1=53, size=512, square_ok=0, downsample=1, img=p,
                 uimg=p, rgb_u8=p)
        a.update(kw)
        rc = lib.m3s_ingest(ctypes.byref(_lib.IngestArgs(**a)), ws, ws_bytes, None)
        return rc, lib.m3s_last_error().decode()

    for kw, msg in ((dict(size=256), "size must be 512 or 224"), (dict(H1=0), "must be in 1..16384"),
                    (dict(W1=16385, row_stride=16385 * 3), "must be in 1..16384"),
                    (dict(downsample=0), "downsample must be at least 1"), (dict(src_dtype=2), "src_dtype"),
                    (dict(B=-1), "B must be in"), (dict(H1=1, W1=300, row_stride=900), "crop is empty"),
                    (dict(row_stride=100), "row_stride below"), (dict(src=None), "null source"),
                    (dict(src_dtype=1, row_stride=53 * 12 + 2), "misaligned float source"),
                    (dict(src_dtype=1, row_stride=53 * 12, src=p + 1), "misaligned float source"),
                    (dict(img=p + 2), "misaligned float output"), (dict(uimg=p + 1), "misaligned float output"),
                    (dict(ws=None), "workspace")):
        rc, err = call(**kw)
        assert rc == _lib.EINVAL and msg in err, (kw, rc, err)
    rc, err = call(ws_bytes=16)
    assert rc == _lib.ESPACE and "workspace too small" in err
    assert call(B=0, src=None, ws=None, ws_bytes=0)[0] == 0
    assert lib.m3s_ingest(None, p, 1 << 30, None) == _lib.EINVAL
    for args in ((0, 5, 0), (5, 0, 0), (5, 5, 2)):
        x = (ctypes.c_int32 * 64)()
        xp = ctypes.cast(x, ctypes.c_void_p)
        assert lib.m3s_ingest_table(*args, xp, xp, xp, 64) == _lib.EINVAL
    x = (ctypes.c_int32 * 64)()
    xp = ctypes.cast(x, ctypes.c_void_p)
    assert lib.m3s_ingest_table(10, 5, 1, xp, xp, xp, 3) == _lib.EINVAL and "ksize" in lib.m3s_last_error().decode()
    assert all(v == 0.0 for v in buf)
