"""GPU: the frame ingest (m3s_ingest behind m3s.ingest) against tests/ingest_cases.py.

The two kernels compute in integers what ``ingest_cases.resample_crop`` computes in numpy from the same tables, and the
tail's three float operations one rounding each, so every output is compared bit for bit: ``rgb_u8`` as bytes, ``img``
and ``uimg`` viewed as uint32. Every output sits between guard runs holding a sentinel that no launch may touch. The
restatement of a case is computed once (``ingest_cases.restate``) and shared; the largest case is 480 x 640."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ingest_cases as IC
from m3s import _lib
from m3s import ingest as MI
from m3s.config import config

pytestmark = pytest.mark.gpu

GUARD = 1024  # elements in front of and behind every output that no launch may touch
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "ingest tests need a HIP device"
    return torch.device("cuda:0")


def _guarded(shape, dtype, dev):
    """(flat buffer of sentinels, its contiguous view of `shape` with GUARD elements on both sides)."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    else:
        flat = torch.full((n + 2 * GUARD,), SENTINEL & 255, dtype=torch.uint8, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _guards_hold(flat):
    raw = flat.view(torch.int32) if flat.dtype == torch.float32 else flat
    want = SENTINEL if flat.dtype == torch.float32 else SENTINEL & 255
    return bool((raw[:GUARD] == want).all()) and bool((raw[-GUARD:] == want).all())


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _want(rgbs, ds):
    """rgbs: list of (Hc, Wc, 3) uint8 -> the batch's (img, uimg, rgb) as numpy arrays."""
    tails = [IC.tail(r, ds) for r in rgbs]
    return np.stack([t[0] for t in tails]), np.stack([t[1] for t in tails]), np.stack(rgbs)


def _run_and_check(src, case, rgbs, dev, ds=1, outputs=(True, True, True)):
    """Run m3s_ingest on the (B, H, W, 3) device tensor src with the chosen outputs (others null) between guards and
    compare each with the restatement."""
    size, sq = case[2], case[3]
    B = src.shape[0]
    Hc, Wc = rgbs[0].shape[:2]
    Hd, Wd = -(-Hc // ds), -(-Wc // ds)
    shapes = ((B, 3, Hc, Wc), (B, Hd, Wd, 3), (B, Hc, Wc, 3))
    dtypes = (torch.float32, torch.float32, torch.uint8)
    bufs = [_guarded(s, d, dev) if on else (None, None) for s, d, on in zip(shapes, dtypes, outputs)]
    MI.run(src, size, sq, ds, *(b[1] for b in bufs))
    torch.cuda.synchronize()
    want = _want(rgbs, ds)
    # rgb_u8 first: a wrong byte explains a wrong float
    for i in (2, 0, 1):
        flat, view = bufs[i]
        if view is None:
            continue
        np.testing.assert_array_equal(_bits(view), want[i].view(np.uint32) if i < 2 else want[i],
                                      err_msg=("img", "uimg", "rgb_u8")[i])
        assert _guards_hold(flat), ("img", "uimg", "rgb_u8")[i] + ": a guard was written"


def _dev_src(u8, dev, f32=False):
    a = IC.to_float(u8) if f32 else u8
    return torch.from_numpy(np.array(a)).to(dev)[None]


@pytest.mark.parametrize("case", IC.CASES, ids=IC.case_id)
def test_bit_exact_and_guards_hold(dev, case):
    src, g, rgb = IC.restate(*case)
    _run_and_check(_dev_src(src, dev), case, [rgb], dev)


@pytest.mark.parametrize("case", IC.EXTRA, ids=IC.case_id)
@pytest.mark.parametrize("ds", [2, 3])
def test_downsample_with_odd_output_sizes(dev, case, ds):
    src, g, rgb = IC.restate(*case)
    if ds == 3:
        assert rgb.shape[0] % 3 and rgb.shape[1] % 3  # ceil sizes: the last kept pixel is not the last pixel
    _run_and_check(_dev_src(src, dev), case, [rgb], dev, ds=ds)


@pytest.mark.parametrize("case", IC.EXTRA, ids=IC.case_id)
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_batch_of_two_different_images(dev, case, f32):
    a, b = IC.restate(*case), IC.restate(*case, seed=1)
    assert not np.array_equal(a[2], b[2])
    src = torch.cat([_dev_src(a[0], dev, f32), _dev_src(b[0], dev, f32)])
    _run_and_check(src, case, [a[2], b[2]], dev, ds=2)


@pytest.mark.parametrize("case", IC.EXTRA, ids=IC.case_id)
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_padded_row_stride(dev, case, f32):
    """Rows 7 elements longer than their pixels: with bytes no row but the first starts on a dword."""
    src, g, rgb = IC.restate(*case)
    H, W = src.shape[:2]
    a = torch.from_numpy(IC.to_float(src) if f32 else src.copy()).reshape(H, W * 3)
    wide = torch.full((2, H, W * 3 + 7), 0.25 if f32 else 77, dtype=a.dtype)
    wide[:, :, :W * 3] = a
    wide = wide.to(dev)
    view = wide.as_strided((2, H, W, 3), (H * (W * 3 + 7), W * 3 + 7, 3, 1))
    assert view.stride(1) == W * 3 + 7
    _run_and_check(view, case, [rgb, rgb], dev)


@pytest.mark.parametrize("case", IC.EXTRA + [IC.LEVELS], ids=IC.case_id)
def test_float_source_gives_the_uint8_sources_bytes(dev, case):
    """The reference's float image (float32(u) / 255) through the kernel's x * 255 conversion: the same outputs. The
    levels case holds every level 0..255 in every channel."""
    src, g, rgb = IC.restate(*case)
    if case == IC.LEVELS:
        assert all(set(src[:, :, c].ravel()) == set(range(256)) for c in range(3))
    for f32 in (False, True):
        _run_and_check(_dev_src(src, dev, f32), case, [rgb], dev)
    # values outside [0, 1] clamp, NaN gives 0: the bytes of the clipped image
    f = IC.to_float(src).copy()
    f[0, 0], f[-1, -1], f[0, -1] = -3.0, 7.5, np.nan
    clipped = src.copy()
    clipped[0, 0], clipped[-1, -1], clipped[0, -1] = 0, 255, 0
    want = IC.resample_crop(clipped, g)
    _run_and_check(torch.from_numpy(f).to(dev)[None], case, [want], dev)


@pytest.mark.parametrize("outputs", [o for o in itertools.product((False, True), repeat=3)],
                         ids=lambda o: "".join("IUR"[i] if on else "-" for i, on in enumerate(o)))
def test_null_outputs_in_each_combination(dev, outputs):
    for case in IC.EXTRA:
        src, g, rgb = IC.restate(*case)
        _run_and_check(_dev_src(src, dev), case, [rgb], dev, ds=2, outputs=outputs)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rgb_u8_at_an_unaligned_address(dev, off):
    """rgb_u8 may start at any byte: no lane's four bytes then sit on a dword and every store goes byte by byte."""
    case = IC.EXTRA[0]
    src, g, rgb = IC.restate(*case)
    n = rgb.size
    flat = torch.full((n + 2 * GUARD + 4,), SENTINEL & 255, dtype=torch.uint8, device=dev)
    view = flat[GUARD + off:GUARD + off + n].view((1,) + rgb.shape)
    assert view.data_ptr() % 4 == off
    MI.run(_dev_src(src, dev), case[2], case[3], 1, None, None, view)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(view.cpu().numpy()[0], rgb)
    assert bool((flat[:GUARD + off] == SENTINEL & 255).all()) and bool((flat[GUARD + off + n:] == SENTINEL & 255).all())


def test_cached_tables_serve_later_calls_and_release_rebuilds(dev):
    lib = _lib.load()
    for case in IC.EXTRA:
        src, g, rgb = IC.restate(*case)
        d = _dev_src(src, dev)
        _run_and_check(d, case, [rgb], dev)
        _run_and_check(d, case, [rgb], dev)  # the cached tables
        with torch.cuda.device(dev):
            _lib.check(lib.m3s_ingest_release())
            _lib.check(lib.m3s_ingest_prepare(case[0], case[1], case[2], int(case[3]), _lib.stream_ptr(dev)))
        _run_and_check(d, case, [rgb], dev)


def test_ingest_operator_and_device_resize_img(dev):
    """m3s.ingest.ingest from host numpy, host tensor and device tensor sources, and resize_img(device=...)."""
    case = IC.EXTRA[0]
    src, g, rgb = IC.restate(*case)
    want_img, want_uimg, _ = _want([rgb], 3)
    for image in (src, IC.to_float(src), torch.from_numpy(src.copy()), torch.from_numpy(src.copy()).to(dev)):
        img, uimg, u8, true_shape = MI.ingest(image, 512, downsample=3, device=dev)
        assert img.device == uimg.device == u8.device == true_shape.device == dev
        np.testing.assert_array_equal(_bits(u8), rgb)
        np.testing.assert_array_equal(_bits(img), want_img.view(np.uint32))
        np.testing.assert_array_equal(_bits(uimg), want_uimg[0].view(np.uint32))
        assert true_shape.dtype == torch.int32 and true_shape.tolist() == [list(rgb.shape[:2])]
    config["dataset"]["img_downsample"] = 3  # the default of `downsample`
    assert MI.ingest(src, device=dev)[1].shape == want_uimg[0].shape
    batch = MI.ingest(np.stack([src, src]), downsample=1, device=dev)
    assert batch[0].shape[0] == 2 and batch[2].shape == (2,) + rgb.shape and batch[3].tolist() == [list(rgb.shape[:2])] * 2
    res, tf = MI.resize_img(IC.to_float(src), 512, return_transformation=True, device=dev)
    assert res["img"].device == dev and res["unnormalized_img"].device == dev and tf == g["transformation"]
    np.testing.assert_array_equal(_bits(res["img"]), IC.tail(rgb)[0][None].view(np.uint32))
    np.testing.assert_array_equal(_bits(res["unnormalized_img"]), rgb)
    assert res["true_shape"].dtype == np.int32 and res["true_shape"].tolist() == [list(rgb.shape[:2])]
    with pytest.raises(TypeError, match="uint8 or float32"):
        MI.ingest(src.astype(np.float64), device=dev)


@pytest.mark.parametrize("case", IC.EXTRA, ids=IC.case_id)
@pytest.mark.parametrize("ds", [1, 2])
def test_create_frame_fused_equals_the_host_statement(dev, case, ds, monkeypatch):
    pytest.importorskip("PIL")
    from m3s.sim3 import Sim3

    src, g, rgb = IC.restate(*case)
    config["dataset"]["img_downsample"] = ds
    T = Sim3.Identity(1, device=dev)
    monkeypatch.delenv("M3S_INGEST_FUSED", raising=False)
    host = MI.create_frame(5, IC.to_float(src), T, img_size=case[2], device=dev)
    monkeypatch.setenv("M3S_INGEST_FUSED", "1")
    for image in (IC.to_float(src), src):
        fused = MI.create_frame(5, image, T, img_size=case[2], device=dev)
        assert type(fused) is type(host) and fused.frame_id == host.frame_id == 5 and fused.T_WC is T
        assert fused.img_size == host.img_size
        for name in ("img", "img_shape", "img_true_shape", "uimg"):
            a, b = getattr(fused, name), getattr(host, name)
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, name
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=name)
        assert fused.uimg.device.type == "cpu" and fused.img.device == dev
    np.testing.assert_array_equal(_bits(host.img[0]), IC.tail(rgb)[0].view(np.uint32))


def test_timing_span_and_device_argument_errors(dev):
    lib = _lib.load()
    case = IC.EXTRA[0]
    src, g, rgb = IC.restate(*case)
    d = _dev_src(src, dev)
    _run_and_check(d, case, [rgb], dev)  # the tables are cached: the span holds the two launches alone
    lib.m3s_timing_reset()
    lib.m3s_timing_enable(1)
    try:
        _run_and_check(d, case, [rgb], dev)
    finally:
        lib.m3s_timing_enable(0)
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    _lib.check(lib.m3s_timing_query(b"ingest", ms, cnt))
    lib.m3s_timing_reset()
    assert cnt.value == 1 and ms.value >= 0.0
    with pytest.raises(RuntimeError, match="must be on the HIP device"):
        MI.run(torch.from_numpy(src.copy())[None], 512)
