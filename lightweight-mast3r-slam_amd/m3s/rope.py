"""RoPE2D of the MASt3R ViT: the module over the HIP kernel, and a plain-torch statement of the operator.

``RoPE2D`` has the constructor and the ``forward(tokens (B,H,N,D), positions (B,N,2))`` of the reference's
``cuRoPE2D`` (croco/models/curope/curope2d.py:32-40) without its autograd function: inference only. It rotates in
place through ``curope.rope_2d`` (``m3s_rope2d``) and returns ``tokens``.

``rope2d_torch`` states the same operator in torch ops, for CPU use and as the timing baseline of
``scripts/rope2d_time.py``. Layout (kernels.cu:40-41): a head row of D = 4 Q elements is [u_y | v_y | u_x | v_x]; per
axis a and t < Q, u' = u c - v s and v' = v c + u s with c, s = cos, sin(F0 pos[a] / base^(t/Q)).
"""
import torch

import curope


class RoPE2D(torch.nn.Module):
    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base = freq
        self.F0 = F0

    def forward(self, tokens, positions):
        """tokens (B,H,N,D), the transposed view of a (B,N,H,D) layout as attention holds q and k; in place."""
        if torch.is_grad_enabled() and tokens.requires_grad:
            raise RuntimeError("m3s.rope.RoPE2D is forward only: call it under torch.no_grad() or use the "
                               "reference's cuRoPE2D, which binds to the same kernel")
        curope.rope_2d(tokens.transpose(1, 2), positions, self.base, self.F0)
        return tokens


def rope2d_torch(tokens, positions, base, F0):
    """The operator on tokens (B,N,H,D), positions (B,N,2) integer (y, x), out of place: returns the rotated tokens.

    The angles are formed in float64; the rotation runs in float64 for float64 tokens and in float32 for every other
    dtype, and the result is cast back to the tokens' dtype."""
    B, N, H, D = tokens.shape
    if D % 4 != 0:
        raise RuntimeError("token dim must be multiple of 4")
    Q = D // 4
    work = torch.float64 if tokens.dtype == torch.float64 else torch.float32
    t = torch.arange(Q, device=tokens.device, dtype=torch.float64)
    inv = float(F0) / torch.pow(float(base), t / Q)  # (Q); scalar operands only: no host-to-device copy, no sync
    ang = positions.to(torch.float64)[:, :, None, :, None] * inv  # (B,N,1,2,Q)
    c, s = torch.cos(ang).to(work), torch.sin(ang).to(work)
    x = tokens.to(work).reshape(B, N, H, 2, 2, Q)  # axis, (u, v), t
    u, v = x[:, :, :, :, 0], x[:, :, :, :, 1]
    out = torch.stack((u * c - v * s, v * c + u * s), dim=4)
    return out.reshape(B, N, H, D).to(tokens.dtype)
