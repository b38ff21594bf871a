"""Drop-in replacement for the reference's second native extension ``curope``: RoPE2D of the MASt3R ViT.

Same module name and the one function ``rope_2d(tokens, positions, base, F0)`` that
``croco/models/curope/curope2d.py:6-9`` imports (``import curope as _kernels``), with the argument order, the
in-place semantics and the error messages of ``curope.cpp:49-65`` and ``kernels.cu:86-108``. With this package
directory on ``sys.path`` the reference's own ``cuRoPE2D`` (autograd wrapper included) binds to the HIP kernel of
``libm3s.so`` (``m3s_rope2d``, ``include/m3s.h``) and ``models/pos_embed.py`` no longer falls back to its slow
torch class. There is no CPU path: non-HIP tensors raise ``RuntimeError``.

Differences that a caller can observe:
  * float64 tokens are rejected (the reference's kernel computes them in float; the ViT has none); float16, float32
    and bfloat16 are taken (the reference dispatches no bfloat16);
  * positions must be int64 (the reference's ``data_ptr<int64_t>`` raises for any other dtype too);
  * the kernel runs on torch's *current* stream instead of the legacy default stream;
  * cos and sin come from a table computed in fp64 on the host and rounded once to fp32, not from per-thread fp32
    ``powf`` / ``cosf`` / ``sinf``; the products and sums are fp32 as the reference writes them, then one rounding to
    the token dtype. Results are reproducible bit for bit and closer to the exact rotation than the reference's;
  * the first call for a (device, base, F0, D) builds and uploads that table synchronously: call
    ``m3s_rope2d_prepare`` before capturing into a graph.
"""
import torch

from m3s import _lib

__all__ = ["rope_2d"]

_DTYPES = {torch.float16: 0, torch.float32: 1, torch.bfloat16: 2}


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def rope_2d(tokens, positions, base, F0):
    """curope.cpp:49-65. tokens (B,N,H,D) rotated in place by positions (B,N,2) int64 (y, x); returns None."""
    # curope.cpp:54-59
    _check(tokens.dim() == 4, "tokens must have 4 dimensions")
    _check(positions.dim() == 3, "positions must have 3 dimensions")
    _check(tokens.size(0) == positions.size(0), "batch size differs between tokens & positions")
    _check(tokens.size(1) == positions.size(1), "seq_length differs between tokens & positions")
    _check(positions.size(2) == 2, "positions.shape[2] must be equal to 2")
    _check(tokens.device == positions.device, "tokens and positions are not on the same device")
    # kernels.cu:91-94
    B, N, H, D = tokens.shape
    _check(D == 0 or (tokens.stride(3) == 1 and tokens.stride(2) == D), "tokens are not contiguous")
    _check(positions.is_contiguous(), "positions are not contiguous")
    _check(tuple(positions.shape) == (B, N, 2), "bad pos.shape")
    _check(D % 4 == 0, "token dim must be multiple of 4")
    _check(positions.dtype == torch.int64, f"positions must be int64, got {positions.dtype}")
    dt = _DTYPES.get(tokens.dtype)
    _check(dt is not None, f"rope_2d: tokens must be float16, float32 or bfloat16, got {tokens.dtype}")
    _lib.require_cuda("rope_2d", tokens, positions)
    lib = _lib.load()
    dev = tokens.device

    def launch():
        _lib.check(lib.m3s_rope2d(dt, _lib.ptr(tokens), tokens.stride(0), tokens.stride(1), _lib.ptr(positions),
                                  B, N, H, D, float(base), float(F0), _lib.stream_ptr(dev)))

    if dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):  # the table cache and the launch belong to the tokens' device
            launch()
    else:
        launch()
