"""GPU: RoPE2D (m3s_rope2d behind curope.rope_2d and m3s.rope.RoPE2D) against tests/rope_cases.py.

The kernel computes in fp32 from the library's table exactly what ``rope_cases.restate`` computes in numpy from the
same table, so every in-table result is compared bit for bit. Every case is a few hundred elements."""
import ctypes

import numpy as np
import pytest
import torch

import curope
import rope_cases as RC
from m3s import _lib
from m3s.rope import RoPE2D, rope2d_torch

pytestmark = pytest.mark.gpu

GUARD = 64  # elements behind every buffer that no launch may touch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "RoPE2D tests need a HIP device"
    return torch.device("cuda:0")


def _place(tok, layout, dev, offset=0):
    """tok (B,N,H,D) on the CPU -> (flat device buffer with a guard tail, the (B,N,H,D) view of it to rotate, the flat
    buffer's expected-unchanged mask). layout "dense": the view is contiguous at `offset` elements; "qkv": the q slice
    of a (B,N,3,H,D) buffer whose k and v slices hold other values."""
    B, N, H, D = tok.shape
    g = torch.Generator().manual_seed(5)
    if layout == "dense":
        n = tok.numel()
        flat = torch.randn(offset + n + GUARD, generator=g).to(tok.dtype)
        flat[offset:offset + n] = tok.reshape(-1)
        flat = flat.to(dev)
        view = flat[offset:offset + n].view(B, N, H, D)
        keep = torch.ones(flat.numel(), dtype=torch.bool)
        keep[offset:offset + n] = False
    else:
        assert offset == 0
        n = 3 * tok.numel()
        flat = torch.randn(n + GUARD, generator=g).to(tok.dtype)
        flat[:n].view(B, N, 3, H, D)[:, :, 0] = tok
        flat = flat.to(dev)
        view = flat[:n].view(B, N, 3, H, D)[:, :, 0]
        keep = torch.ones(flat.numel(), dtype=torch.bool)
        keep[:n].view(B, N, 3, H, D)[:, :, 0] = False
        assert view.stride() == (N * 3 * H * D, 3 * H * D, D, 1)
    return flat, view, keep


def _assert_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape
    same = RC.bits(got) == RC.bits(want)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in bits"


@pytest.mark.parametrize("D, dtype, layout, F0", RC.GRID,
                         ids=[f"D{D}-{dt}-{layout}-F0{F0:+.0f}" for D, dt, layout, F0 in RC.GRID])
def test_bit_exact_and_neighbours_untouched(dev, D, dtype, layout, F0):
    tok, pos = RC.make_case(3, D=D, dtype=dtype)
    cos, sin = RC.lib_table(RC.BASE, F0, D // 4)
    want = RC.restate(tok, pos, cos, sin)
    assert not torch.equal(RC.bits(want), RC.bits(tok))
    flat, view, keep = _place(tok, layout, dev)
    before = flat.cpu().clone()
    assert curope.rope_2d(view, pos.to(dev), RC.BASE, F0) is None
    torch.cuda.synchronize()
    _assert_bits(view.cpu(), want, "rotated tokens")
    # the k and v slices (qkv) and the guard tail: bit-unchanged
    after = flat.cpu()
    assert torch.equal(RC.bits(after)[keep], RC.bits(before)[keep])
    assert int(keep.sum()) >= GUARD + (2 * tok.numel() if layout == "qkv" else 0)


def test_misaligned_base_takes_the_scalar_path(dev):
    """D = 64 f16 at a storage offset of 2 elements (4 bytes): no 16-byte access is legal there."""
    tok, pos = RC.make_case(4, D=RC.D_VEC, dtype="f16")
    cos, sin = RC.lib_table(RC.BASE, 1.0, RC.D_VEC // 4)
    flat, view, keep = _place(tok, "dense", dev, offset=2)
    assert view.data_ptr() % 16 == 4
    before = flat.cpu().clone()
    curope.rope_2d(view, pos.to(dev), RC.BASE, 1.0)
    torch.cuda.synchronize()
    _assert_bits(view.cpu(), RC.restate(tok, pos, cos, sin), "misaligned tokens")
    assert torch.equal(RC.bits(flat.cpu())[keep], RC.bits(before)[keep])


def test_out_of_table_positions(dev):
    """Positions -3, 1024 and 5000 take the in-kernel fp64 path; 1023 is the table's last row. In-table rows stay
    bit-exact; the others are within 2^-22 * (|u| + |v|) of the float64 truth: device fp64 trig rounded to fp32 is
    <= 1 ulp (2^-23) on c and s, plus the 2.5 * 2^-24 of the arithmetic."""
    tok, pos = RC.make_case(6, D=RC.D_VEC, dtype="f32")
    special = [-3, 1023, 1024, 5000]
    pos = pos.clone()
    flat_pos = pos.view(-1)
    for i, p in enumerate(special + special[::-1]):  # both axes, both batch elements
        flat_pos[(3 * i) % flat_pos.numel()] = p  # entries 0, 3, 6, ..., 18, 1: y and x slots alike
    inside = (pos >= 0) & (pos < RC.TABLE_P)  # (B,N,2)
    assert int((~inside).sum()) >= 5 and bool((pos == 1023).any()) and bool(inside.all(dim=-1).any())
    cos, sin = RC.lib_table(RC.BASE, 1.0, RC.D_VEC // 4)
    want_tab = RC.restate(tok, pos.clamp(0, RC.TABLE_P - 1), cos, sin)
    want, mag = RC.truth(tok, pos, RC.BASE, 1.0)
    flat, view, keep = _place(tok, "dense", dev)
    curope.rope_2d(view, pos.to(dev), RC.BASE, 1.0)
    torch.cuda.synchronize()
    got = view.cpu()
    B, N, H, D = tok.shape
    # element (b,n,h,d) belongs to axis d // (D / 2)
    in_elem = inside[:, :, None, :, None].expand(B, N, H, 2, D // 2).reshape(B, N, H, D)
    assert torch.equal(RC.bits(got)[in_elem], RC.bits(want_tab)[in_elem])
    err = np.abs(got.to(torch.float64).numpy() - want) / mag
    out_elem = ~in_elem.numpy()
    print(f"out-of-table rows: max |got - truth| / (|u| + |v|) = {err[out_elem].max() * 2.0 ** 24:.2f} * 2^-24")
    assert (err[out_elem] <= 2.0 ** -22).all()


def test_module_agrees_with_the_operator_and_the_torch_statement(dev):
    tok, pos = RC.make_case(7, D=RC.D_VEC, dtype="f32")  # (2,5,3,64)
    a = tok.to(dev)
    tokens = a.transpose(1, 2)  # (2,3,5,64): attention's (B,H,N,D) view
    assert tuple(tokens.shape) == (2, 3, 5, 64)
    with torch.no_grad():
        out = RoPE2D(freq=RC.BASE, F0=1.0)(tokens, pos.to(dev))
    assert out is tokens
    b = tok.to(dev)
    curope.rope_2d(b, pos.to(dev), RC.BASE, 1.0)
    torch.cuda.synchronize()
    assert not torch.equal(a.cpu(), tok)
    _assert_bits(a.cpu(), b.cpu(), "module against operator")
    want64 = rope2d_torch(tok.to(torch.float64), pos, RC.BASE, 1.0).numpy()
    _, mag = RC.truth(tok, pos, RC.BASE, 1.0)
    assert (np.abs(a.cpu().to(torch.float64).numpy() - want64) <= 3.0 * 2.0 ** -24 * mag).all()
    # the same statement on the device, in float32: the same bound
    got_dev = rope2d_torch(tok.to(dev), pos.to(dev), RC.BASE, 1.0).cpu()
    assert (np.abs(got_dev.to(torch.float64).numpy() - want64) <= 3.0 * 2.0 ** -24 * mag).all()
    with pytest.raises(RuntimeError, match="forward only"):
        RoPE2D()(tok.to(dev).transpose(1, 2).requires_grad_(), pos.to(dev))
    with pytest.raises(RuntimeError, match="not on the same device"):
        curope.rope_2d(tok.to(dev), pos, RC.BASE, 1.0)


def test_prepare_stream_and_release(dev):
    """m3s_rope2d_prepare, then a call on a non-default stream; m3s_rope2d_release, then a further call that builds the
    table again: the same bits every time. (base 50 so that no other test's table is the one prepared.)"""
    lib = _lib.load()
    base, Q = 50.0, RC.D_VEC // 4
    tok, pos = RC.make_case(8, D=RC.D_VEC, dtype="f16")
    cos, sin = _lib.rope2d_table(base, 1.0, Q)
    want = RC.restate(tok, pos, cos, sin)
    dpos = pos.to(dev)
    _lib.check(lib.m3s_rope2d_prepare(base, 1.0, Q, _lib.stream_ptr(dev)))
    side = torch.cuda.Stream(device=dev)
    a = tok.to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        curope.rope_2d(a, dpos, base, 1.0)
    side.synchronize()
    _assert_bits(a.cpu(), want, "non-default stream")
    _lib.check(lib.m3s_rope2d_release())
    _lib.check(lib.m3s_rope2d_release())  # nothing cached: still fine
    b = tok.to(dev)
    curope.rope_2d(b, dpos, base, 1.0)
    torch.cuda.synchronize()
    _assert_bits(b.cpu(), want, "after release")
    # the timing span of the launch
    lib.m3s_timing_reset()
    lib.m3s_timing_enable(1)
    curope.rope_2d(b, dpos, base, 1.0)
    torch.cuda.synchronize()
    lib.m3s_timing_enable(0)
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    _lib.check(lib.m3s_timing_query(b"rope2d", ms, cnt))
    lib.m3s_timing_reset()
    assert cnt.value == 1 and ms.value >= 0.0


def test_backward_pass_restores_the_tokens(dev):
    """fwd = -F0 after fwd = +F0 (the reference's autograd backward) restores f32 tokens to within
    6 * 2^-24 * (|u| + |v|): two applications of the 3 * 2^-24 bound of one."""
    tok, pos = RC.make_case(9, D=RC.D_VEC, dtype="f32")
    a = tok.to(dev)
    curope.rope_2d(a, pos.to(dev), RC.BASE, 1.0)
    mid = a.cpu()
    curope.rope_2d(a, pos.to(dev), RC.BASE, -1.0)
    torch.cuda.synchronize()
    _, mag = RC.truth(tok, pos, RC.BASE, 1.0)
    err = np.abs(a.cpu().to(torch.float64).numpy() - tok.to(torch.float64).numpy()) / mag
    print(f"forward then backward: max |got - tokens| / (|u| + |v|) = {err.max() * 2.0 ** 24:.2f} * 2^-24")
    assert not torch.equal(mid, tok)
    assert (err <= 6.0 * 2.0 ** -24).all()
