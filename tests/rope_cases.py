"""Cases and references of the RoPE2D tests (test_rope_host.py on the CPU, test_gpu_rope.py on the device).

Layout (the reference's kernels.cu:40-41): a head row of D = 4 Q elements is [u_y | v_y | u_x | v_x], Q each; for
axis a (0 = y, 1 = x) and t < Q: u' = u c - v s, v' = v c + u s, c, s = cos, sin(fwd pos[a] / base^(t/Q)).

``restate`` is the operator as libm3s.so's kernel computes it, in numpy: c and s are looked up in GIVEN tables (the
library's own, from ``lib_table``), every product and sum is a separate float32 operation, and the result is rounded
once to the token dtype. The device must give its bits. ``truth`` is the formula in float64.
"""
import numpy as np
import torch

BASE = 100.0
TABLE_P = 1024  # rows of the library's table: positions [0, 1024)
B, N, H = 2, 5, 3
D_VEC, D_SCALAR = 64, 12  # 16-byte chunks per quarter / Q = 3: one element per lane
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
LAYOUTS = ("dense", "qkv")  # qkv: the q slice of a (B, N, 3, H, D) buffer, token stride 3 H D
F0S = (1.0, -1.0)
# the device grid: every combination
GRID = [(D, dt, layout, F0) for D in (D_VEC, D_SCALAR) for dt in DTYPES for layout in LAYOUTS for F0 in F0S]
# the host tests' case (the issue's measured figures are at this shape)
HOST_SHAPE = dict(B=2, H=3, N=37, D=64)

_TABLES = {}


def lib_table(base, fwd, Q):
    """The library's (TABLE_P, Q) float32 cos and sin tables (host-only ABI call), cached."""
    from m3s import _lib

    key = (float(base), float(fwd), int(Q))
    if key not in _TABLES:
        cos, sin = _lib.rope2d_table(base, fwd, Q, TABLE_P)
        cos.setflags(write=False)
        sin.setflags(write=False)
        _TABLES[key] = (cos, sin)
    return _TABLES[key]


def make_case(seed, B=B, N=N, H=H, D=D_VEC, dtype="f32"):
    """tokens (B,N,H,D): seeded standard_normal * 3, rounded to the dtype (a torch CPU tensor); positions (B,N,2) int64
    in [0, 48) with y != x in every token and different rows in every batch element."""
    rng = np.random.default_rng(seed)
    tok = torch.from_numpy((rng.standard_normal((B, N, H, D)) * 3).astype(np.float32)).to(DTYPES[dtype])
    y = rng.integers(0, 48, size=(B, N))
    x = (y + rng.integers(1, 48, size=(B, N))) % 48
    pos = np.stack([y, x], axis=-1).astype(np.int64)
    for b in range(1, B):  # no batch element repeats another's positions
        while any((pos[b] == pos[o]).all() for o in range(b)):
            pos[b, 0, 0] = (pos[b, 0, 0] + 1) % 48
            if pos[b, 0, 0] == pos[b, 0, 1]:
                pos[b, 0, 0] = (pos[b, 0, 0] + 1) % 48
    assert (pos[..., 0] != pos[..., 1]).all() and pos.min() >= 0 and pos.max() < 48
    return tok, torch.from_numpy(pos)


def _split(tok):
    """(B,N,H,D) -> u, v of shape (B,N,H,2,Q): axis, t"""
    b, n, h, d = tok.shape
    x = tok.reshape(b, n, h, 2, 2, d // 4)
    return x[:, :, :, :, 0], x[:, :, :, :, 1]


def restate(tok, pos, cos_tab, sin_tab):
    """tok: torch CPU tensor (B,N,H,D) of f32 / f16 / bf16; pos (B,N,2) int64 inside the tables. Returns the rotated
    tokens, a torch CPU tensor of the same dtype: float32 products and sums, one rounding to the dtype."""
    x = tok.to(torch.float32).numpy()
    p = pos.numpy()
    assert p.min() >= 0 and p.max() < cos_tab.shape[0]
    u, v = _split(x)
    c = cos_tab[p][:, :, None, :, :]  # (B,N,1,2,Q) float32
    s = sin_tab[p][:, :, None, :, :]
    assert u.dtype == v.dtype == c.dtype == s.dtype == np.float32
    uc, vs, vc, us = u * c, v * s, v * c, u * s  # four float32 roundings
    un, vn = uc - vs, vc + us
    assert un.dtype == vn.dtype == np.float32
    out = np.stack([un, vn], axis=4).reshape(x.shape)
    if tok.dtype == torch.float16:
        return torch.from_numpy(out.astype(np.float16))
    if tok.dtype == torch.bfloat16:
        return torch.from_numpy(out).to(torch.bfloat16)
    return torch.from_numpy(out)


def truth(tok, pos, base, fwd):
    """float64: (rotated tokens, |u| + |v| of every element's pair), both (B,N,H,D) numpy float64."""
    x = tok.to(torch.float64).numpy()
    p = pos.numpy().astype(np.float64)
    Q = x.shape[-1] // 4
    inv = float(fwd) / np.power(float(base), np.arange(Q, dtype=np.float64) / Q)
    ang = p[:, :, None, :, None] * inv  # (B,N,1,2,Q)
    c, s = np.cos(ang), np.sin(ang)
    u, v = _split(x)
    out = np.stack([u * c - v * s, v * c + u * s], axis=4).reshape(x.shape)
    mag = np.abs(u) + np.abs(v)
    return out, np.stack([mag, mag], axis=4).reshape(x.shape)


def bits(t):
    """A torch tensor's bit pattern, as an integer tensor on the CPU."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
