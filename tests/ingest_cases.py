"""The frame ingest's cases and its numpy restatement: the bit reference of tests/test_ingest_host.py and
tests/test_gpu_ingest.py.

The restatement is the arithmetic of include/m3s.h written down a second time: geometry with Python's round, the
coefficient tables in Python floats (``math.sin``: the C library's, as the host code's), the two fixed-point passes in
integer numpy, the tail in float32 numpy. Pillow's 8-bit resampler computes the same, so ``restate`` equals Pillow byte
for byte (test_ingest_host.py checks that live and against tests/golden/ingest.npz).

Inputs come from a closed-form integer formula per pixel, not an RNG stream; one half of every image is pure 0 / 255
noise, so both clamps of both passes fire."""
import math

import numpy as np

BICUBIC, LANCZOS = 0, 1
PRECISION_BITS = 22

# (H1, W1, size, square_ok): the smallest shapes at which each branch exists
CASES = [
    (23, 512, 512, False),    # long edge already 512: both axes keep their length, crop 512 x 16
    (513, 100, 512, False),   # horizontal identity (100 -> round(99.8)), vertical lanczos 513 -> 512
    (100, 513, 512, False),   # vertical identity, horizontal lanczos
    (511, 100, 512, False),   # horizontal identity, vertical bicubic 511 -> 512
    (100, 511, 512, False),   # vertical identity, horizontal bicubic
    (24, 520, 512, False),    # lanczos at scale ~1.016
    (90, 2100, 512, False),   # lanczos at scale 4.1, 27 taps
    (37, 53, 512, False),     # bicubic upscale, edge clamps on every side
    (600, 600, 512, False),   # the square 3/4 rule
    (600, 600, 512, True),    # and the square kept
    (270, 1030, 512, False),  # scale ~2
    (512, 384, 512, False),   # no resize at all: crop and tail
    (300, 400, 224, False),   # the 224 branch
    (480, 640, 512, False),   # the one real shape
]
EXTRA = [(37, 53, 512, False), (270, 1030, 512, False)]  # the cases that also run the operator's other arguments
# every level 0..255 in every channel: (256, 3, 3). At size 512 its crop is empty (a 6-pixel side), so it runs at 224
LEVELS = (256, 3, 224, False)
TABLE_PAIRS = [(480, 384), (640, 512), (1080, 288), (1920, 512), (37, 357), (53, 512), (600, 512), (520, 512),
               (2100, 512), (3, 171), (9, 512), (300, 224), (400, 299)]


def case_id(c):
    return f"{c[0]}x{c[1]}-s{c[2]}" + ("-sq" if c[3] else "")


def make_image(H, W, seed=0):
    """(H, W, 3) uint8. Smooth-ish structure on one half; on the other (the right half, or the lower one of a narrow
    image) a multiplicative hash's top bit times 255."""
    y, x, c = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), np.arange(3, dtype=np.int64),
                          indexing="ij")
    s = np.int64(seed)
    smooth = (y * 131 + x * 71 + c * 57 + ((x * y) % 251) * 3 + ((x * x + y + s * 17) >> 2)) & 255
    h = ((x * 3 + 1) * (y * 5 + 7) + x * x + c * 11 + s * 101) * np.int64(2654435761) & np.int64(0xFFFFFFFF)
    noise = ((h >> 31) & 1) * 255
    half = x >= W // 2 if W >= 8 else y >= H // 2
    return np.where(half, noise, smooth).astype(np.uint8)


def levels_image():
    H, W = LEVELS[:2]
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return ((y + 85 * c + 31 * x) % 256).astype(np.uint8)


def to_float(u8):
    """The float image the reference's loaders hand to create_frame: float32(u) / 255."""
    return u8.astype(np.float32) / np.float32(255.0)


# ---- geometry ----

def geometry(H1, W1, size, square_ok):
    """dict(resized (Wr, Hr), filter, crop (x0, y0, x1, y1), out (Wc, Hc), transformation), or None where the crop is
    empty."""
    assert size in (512, 224)
    S = max(W1, H1)
    L = 512 if size == 512 else round(size * max(W1 / H1, H1 / W1))
    Wr, Hr = int(round(W1 * L / S)), int(round(H1 * L / S))
    cx, cy = Wr // 2, Hr // 2
    if size == 224:
        halfw = halfh = min(cx, cy)
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
        if not square_ok and Wr == Hr:
            halfh = 3 * halfw / 4
            assert halfh == int(halfh)
            halfh = int(halfh)
    Wc, Hc = 2 * halfw, 2 * halfh
    if Wc == 0 or Hc == 0:
        return None
    return dict(resized=(Wr, Hr), filter=LANCZOS if S > L else BICUBIC,
                crop=(cx - halfw, cy - halfh, cx + halfw, cy + halfh), out=(Wc, Hc),
                transformation=(W1 / Wr, H1 / Hr, (Wr - Wc) / 2, (Hr - Hc) / 2))


# ---- coefficients ----

def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _filter(f, x):
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_of(n_in, n_out, f):
    return int(math.ceil((3.0 if f == LANCZOS else 2.0) * max(n_in / n_out, 1.0))) * 2 + 1


def table(n_in, n_out, f, o0=0, o1=None):
    """xmin, n (o1 - o0) and k (o1 - o0, ksize) int32 of outputs [o0, o1) of the axis n_in -> n_out."""
    o1 = n_out if o1 is None else o1
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = (3.0 if f == LANCZOS else 2.0) * fs
    ss = 1.0 / fs
    ksize = ksize_of(n_in, n_out, f)
    xmin = np.zeros(o1 - o0, dtype=np.int32)
    n = np.zeros(o1 - o0, dtype=np.int32)
    k = np.zeros((o1 - o0, ksize), dtype=np.int32)
    for xx in range(o0, o1):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        m = min(int(center + support + 0.5), n_in) - lo
        w = [_filter(f, (x + lo - center + 0.5) * ss) for x in range(m)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx - o0], n[xx - o0] = lo, m
        for x, v in enumerate(w):
            k[xx - o0, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return xmin, n, k


# ---- the two passes and the tail ----

def _pass(img, axis, xmin, n, k):
    """img (H, W, 3) uint8; outputs along `axis` (0 rows, 1 columns), one per table entry. The sums stay below 2^31
    (Pillow's int32), so int64 numpy gives the same values."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + src.shape[1:], dtype=np.uint8)
    for i in range(len(xmin)):
        taps = k[i, :n[i]].astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin[i]:xmin[i] + n[i]] * taps).sum(axis=0)
        assert int(np.abs(acc).max()) < 2 ** 31
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resample_crop(u8, g):
    """The cropped uint8 image (Hc, Wc, 3) of source u8 (H1, W1, 3) under geometry g: horizontal pass, then vertical,
    an axis that keeps its length only cropped."""
    H1, W1, _ = u8.shape
    (Wr, Hr), f, (x0, y0, x1, y1) = g["resized"], g["filter"], g["crop"]
    mid = u8[:, x0:x1] if Wr == W1 else _pass(u8, 1, *table(W1, Wr, f, x0, x1))
    return np.ascontiguousarray(mid[y0:y1] if Hr == H1 else _pass(mid, 0, *table(H1, Hr, f, y0, y1)))


def tail(rgb, ds=1):
    """rgb (Hc, Wc, 3) uint8 -> img (3, Hc, Wc) and uimg (ceil(Hc/ds), ceil(Wc/ds), 3), float32, one rounding per
    operation."""
    f = rgb.astype(np.float32) / np.float32(255.0)
    img = (f - np.float32(0.5)) / np.float32(0.5)
    return np.ascontiguousarray(img.transpose(2, 0, 1)), np.ascontiguousarray(f[::ds, ::ds])


_RESTATED = {}


def restate(H1, W1, size, square_ok, seed=0):
    """(source uint8, geometry, rgb_u8) of a case, computed once and shared; treat the arrays as read-only."""
    key = (H1, W1, size, square_ok, seed)
    if key not in _RESTATED:
        src = levels_image() if (H1, W1, size, square_ok) == LEVELS else make_image(H1, W1, seed)
        g = geometry(H1, W1, size, square_ok)
        rgb = resample_crop(src, g)
        for a in (src, rgb):
            a.setflags(write=False)
        _RESTATED[key] = (src, g, rgb)
    return _RESTATED[key]
