"""Map export on the GPU (csrc/map.hip through m3s_map_count / m3s_map_write and m3s.evaluate.world_points):
mask, order, transform accuracy, output alignment, the stored mask, the error paths and the Python surface."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from m3s import _lib
from m3s.config import config
from m3s.frame import Frame, Keyframes
from m3s.geometry import constrain_points_to_ray
from m3s.sim3 import Sim3

pytestmark = pytest.mark.gpu

THR = 1.5
TILE = 1024  # pixels per block of csrc/map.hip (MAP_TILE)
GUARD = 64
SHAPES = [(16, 24), (40, 56), (48, 64)]  # N = 384 (< one block, partial waves), 2240 (not a multiple of 256), 3072
PLY_BODY = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])


def dev():
    return torch.device("cuda:0")


def intrinsics(H, W):
    return torch.tensor([[0.9 * W, 0.0, 0.5 * W - 0.25], [0.0, 0.95 * W, 0.5 * H + 0.125], [0.0, 0.0, 1.0]])


def random_poses(K, g):
    q = torch.randn(K, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    s = torch.exp(0.5 * torch.randn(K, 1, generator=g))
    sign = torch.where(torch.rand(K, 3, generator=g) < 0.5, -1.0, 1.0)
    t = sign * 10.0 ** (torch.rand(K, 3, generator=g) * 4.0 - 2.0)  # 1e-2 .. 1e2
    return torch.cat((t, q, s), dim=1).float()


def identity_poses(K):
    return Sim3.Identity(K).data.clone()


@functools.lru_cache(maxsize=None)
def make_case(H, W, K, seed=0, valid_frac=0.4):
    """Host tensors of K keyframes: X (N,3), C sums (N), fusion counts in {1, 2, 4} (exact reciprocals), u8 colours.
    C * (1/N) stays 1e-3 or more away from THR, except planted pixels AT the threshold and NaN ones (both drop)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * H + K)
    N = H * W
    Xs, Cs, Ns, rgbs = [], [], [], []
    for k in range(K):
        X = torch.randn(N, 3, generator=g) * 2.0
        X[:, 2] = 1.0 + 9.0 * torch.rand(N, generator=g)
        n_avg = (1, 2, 4)[k % 3]
        keep = torch.rand(N, generator=g) < valid_frac
        avg = torch.where(keep, THR + 1e-3 + torch.rand(N, generator=g), THR - 1e-3 - torch.rand(N, generator=g))
        plant = torch.randperm(N, generator=g)[:12]
        avg[plant[:6]] = THR  # equal: the comparison is strict
        avg[plant[6:]] = float("nan")
        Xs.append(X)
        Cs.append(avg * n_avg)
        Ns.append(n_avg)
        rgbs.append(torch.randint(0, 256, (N, 3), generator=g, dtype=torch.uint8))
    return Xs, Cs, Ns, rgbs


def torch_mask(C, n):
    """Frame.get_average_conf() > THR on the device (C / N there is C * float32(1/N))."""
    return (C / n) > THR


def to_dev(ts):
    return [t.to(dev()).contiguous() for t in ts]


def dev_case(*args, **kw):
    """make_case with the tensors copied to the device (the cached host tensors stay unchanged)."""
    Xs, Cs, Ns, rgbs = make_case(*args, **kw)
    return to_dev(Xs), to_dev(Cs), Ns, to_dev(rgbs)


def guarded(nbytes):
    """A device byte buffer of nbytes with GUARD bytes of 0xA5 on both sides; (whole, payload view)."""
    whole = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + nbytes:] == 0xA5).all())


def run_map(Xs, Cs, Ns, Twc, rgbs, layout, K=None, size=None, between=None):
    """count + write through the C ABI on device tensors. Returns (xyz (M,3) f32, rgb (M,3) u8 or None, counts) for
    "soa", (records (M,15) u8, None, counts) for "ply"; asserts the guards around every output."""
    from m3s.evaluate import keyframe_table, map_config, map_count, map_write

    d = dev()
    Kp, N = len(Xs), Cs[0].numel()
    lib = _lib.load()
    ws = torch.zeros(lib.m3s_map_workspace_size(Kp, N), dtype=torch.uint8, device=d)
    mc = map_config(THR, layout, K, size)
    table = keyframe_table(Xs, Cs, Ns)
    counts, M = map_count(mc, table, Kp, N, ws, d)
    assert counts.sum() == M
    if between is not None:
        between()
    row = 15 if layout == "ply" else 12
    whole, out = guarded(M * row)
    whole_c = out_c = None
    if layout == "soa" and rgbs is not None:
        whole_c, out_c = guarded(M * 3)
    map_write(mc, table, Twc.to(d), rgbs, Kp, N, out, out_c, M, ws, d)
    torch.cuda.synchronize()
    assert guards_intact(whole, M * row)
    if whole_c is not None:
        assert guards_intact(whole_c, M * 3)
    if layout == "ply":
        return out.reshape(M, 15), None, counts
    return out.view(torch.float32).reshape(M, 3), None if out_c is None else out_c.reshape(M, 3), counts


def repack(xyz, rgb):
    """SOA rows -> the PLY records, on the host."""
    rec = np.zeros(xyz.shape[0], dtype=PLY_BODY)
    p = xyz.cpu().numpy()
    rec["x"], rec["y"], rec["z"] = p[:, 0], p[:, 1], p[:, 2]
    if rgb is not None:
        c = rgb.cpu().numpy()
        rec["r"], rec["g"], rec["b"] = c[:, 0], c[:, 1], c[:, 2]
    return rec.view(np.uint8).reshape(-1, 15)


def expected_rows(Xs, Cs, Ns, rgbs, K=None, size=None):
    """Torch on the device: per keyframe the (constrained) points, colours and mask."""
    P, R, Mk = [], [], []
    for X, C, n, c in zip(Xs, Cs, Ns, rgbs):
        m = torch_mask(C, n)
        p = X if K is None else constrain_points_to_ray(size, X[None], K.to(X.device))[0]
        P.append(p[m])
        R.append(c[m])
        Mk.append(m)
    return P, R, Mk


# ---- 1. mask and order are exact ----
@pytest.mark.parametrize("calib", [False, True])
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("H,W", SHAPES)
def test_mask_and_order_exact(H, W, K, calib):
    Xs, Cs, Ns, rgbs = dev_case(H, W, K)
    Kmat = intrinsics(H, W).to(dev()) if calib else None
    P, R, Mk = expected_rows(Xs, Cs, Ns, rgbs, Kmat, (H, W))
    exp_xyz, exp_rgb = torch.cat(P), torch.cat(R)
    exp_counts = [int(m.sum()) for m in Mk]
    assert 0 < sum(exp_counts) < K * H * W
    xyz, rgb, counts = run_map(Xs, Cs, Ns, identity_poses(K), rgbs, "soa", Kmat, (H, W))
    assert counts.tolist() == exp_counts
    assert xyz.shape == exp_xyz.shape and torch.equal(xyz, exp_xyz)  # no row missing, extra or reordered
    assert torch.equal(rgb, exp_rgb)
    rec, _, counts = run_map(Xs, Cs, Ns, identity_poses(K), rgbs, "ply", Kmat, (H, W))
    assert counts.tolist() == exp_counts
    assert np.array_equal(rec.cpu().numpy(), repack(exp_xyz, exp_rgb))
    # geometry only: no colour output in SOA, zero colour bytes in PLY
    xyz, rgb, _ = run_map(Xs, Cs, Ns, identity_poses(K), None, "soa", Kmat, (H, W))
    assert rgb is None and torch.equal(xyz, exp_xyz)
    rec, _, _ = run_map(Xs, Cs, Ns, identity_poses(K), None, "ply", Kmat, (H, W))
    assert np.array_equal(rec.cpu().numpy(), repack(exp_xyz, None))


# ---- 2. transform ----
def act_f64(T, p):
    """Sim3.act's formula (uv = 2 qv x p; r = p + w uv + qv x uv; s r + t) in fp64 from the fp32 inputs."""
    T, p = T.double(), p.double()
    t, qv, w, s = T[:3], T[3:6].expand_as(p), T[6], T[7]
    uv = 2.0 * torch.cross(qv, p, dim=-1)
    return s * (p + w * uv + torch.cross(qv, uv, dim=-1)) + t


def bound_ratio(got, p, T):
    """max over coordinates of |got - fp64| / (2^-18 (s |p|_2 + |t|_inf)); got, p (M,3) fp32 on the host."""
    ref = act_f64(T, p)
    bound = 2.0 ** -18 * (T[7].double() * p.double().norm(dim=1) + T[:3].double().abs().max())
    return float(((got.double() - ref).abs() / bound[:, None]).max()) if p.shape[0] else 0.0


@pytest.mark.parametrize("calib", [False, True])
def test_transform_within_derived_bound(calib):
    """About a dozen fp32 roundings on magnitudes of at most 3 |p| come to roughly 2^-19 (s |p| + |t|) per coordinate;
    the bound 2^-18 (s |p|_2 + |t|_inf) leaves a factor 2 over that."""
    H, W, K = 40, 56, 3
    Xs, Cs, Ns, rgbs = dev_case(H, W, K, seed=2)
    Kmat = intrinsics(H, W).to(dev()) if calib else None
    P, _, _ = expected_rows(Xs, Cs, Ns, rgbs, Kmat, (H, W))
    worst = 0.0
    for trial in range(4):
        T = random_poses(K, torch.Generator().manual_seed(trial))
        xyz, _, counts = run_map(Xs, Cs, Ns, T, None, "soa", Kmat, (H, W))
        got = torch.split(xyz.cpu(), counts.tolist())
        for k in range(K):
            worst = max(worst, bound_ratio(got[k], P[k].cpu(), T[k]))
    print(f"map transform: max |err| / bound = {worst:.3f} (calib={calib})")
    assert worst <= 1.0


# ---- 3. alignment ----
def counts_case(block_counts, N, seed):
    """C sums (N_avg = 1) of keyframes whose blocks of TILE pixels hold exactly the given numbers of valid pixels."""
    g = torch.Generator().manual_seed(seed)
    bpk = (N + TILE - 1) // TILE
    Cs = []
    for k in range(len(block_counts) // bpk):
        C = torch.full((N,), THR - 0.5)
        for b in range(bpk):
            lo, hi = b * TILE, min(N, (b + 1) * TILE)
            c = block_counts[k * bpk + b]
            C[lo + torch.randperm(hi - lo, generator=g)[:c]] = THR + 0.5
        Cs.append(C)
    return Cs


# valid pixels per block, 3 keyframes of 48 x 64 = three blocks each
ALIGNMENT_CASES = {
    # first rows 0, 1, 2, 3, 4, 6, 9, 14, 21: every residue of 15 off mod 4 and of 3 off mod 4
    "a_residues": [1, 1, 1, 1, 2, 3, 5, 7, 11],
    "b_empty_middle": [5, 300, 17, 0, 0, 0, 1024, 3, 77],
    "c_all_valid": [TILE] * 9,
    "d_last_pixel": [0] * 8 + [1],  # the one valid pixel is the last of the last keyframe
}


@pytest.mark.parametrize("name", sorted(ALIGNMENT_CASES))
def test_alignment_ply_equals_soa(name):
    bc, N, K = ALIGNMENT_CASES[name], 48 * 64, 3
    if name == "d_last_pixel":
        Cs = [torch.full((N,), THR - 0.5) for _ in range(K)]
        Cs[-1][N - 1] = THR + 0.5
    else:
        Cs = counts_case(bc, N, seed=7)
    if name == "a_residues":
        offs = np.concatenate([[0], np.cumsum(bc)[:-1]])
        assert {int(15 * o % 4) for o in offs} == {0, 1, 2, 3} and {int(3 * o % 4) for o in offs} == {0, 1, 2, 3}
    Xs, _, _, rgbs = make_case(48, 64, K, seed=3)
    Xs, Cs, rgbs = to_dev(Xs), to_dev(Cs), to_dev(rgbs)
    Ns = [1] * K
    T = random_poses(K, torch.Generator().manual_seed(5))
    xyz, rgb, counts = run_map(Xs, Cs, Ns, T, rgbs, "soa")
    assert counts.tolist() == [sum(bc[3 * k:3 * k + 3]) for k in range(K)]
    # content: the rows of the torch mask, in order (points within the bound of test 2, colours exact)
    P, R, _ = expected_rows(Xs, Cs, Ns, rgbs)
    assert torch.equal(rgb, torch.cat(R))
    got = torch.split(xyz.cpu(), counts.tolist())
    assert max(bound_ratio(got[k], P[k].cpu(), T[k]) for k in range(K)) <= 1.0
    rec, _, counts2 = run_map(Xs, Cs, Ns, T, rgbs, "ply")
    assert counts2.tolist() == counts.tolist()
    assert np.array_equal(rec.cpu().numpy(), repack(xyz, rgb))  # byte for byte


# ---- 4. stored mask ----
@pytest.mark.parametrize("layout", ["soa", "ply"])
def test_write_uses_the_mask_stored_at_count(layout):
    H, W, K = 40, 56, 3
    Xs, Cs, Ns, rgbs = dev_case(H, W, K, seed=4)
    Cs = [c.clone() for c in Cs]
    P, R, Mk = expected_rows(Xs, Cs, Ns, rgbs)
    exp_xyz, exp_rgb = torch.cat(P), torch.cat(R)

    def lower():  # C is only lowered: a kernel that re-evaluated it would under-write, never write out of range
        for c, m in zip(Cs, Mk):
            idx = torch.nonzero(m).flatten()[::3]
            c[idx] = 0.0

    a, b, counts = run_map(Xs, Cs, Ns, identity_poses(K), rgbs, layout, between=lower)
    assert counts.tolist() == [int(m.sum()) for m in Mk]
    assert any(int(torch_mask(c, n).sum()) < int(m.sum()) for c, n, m in zip(Cs, Ns, Mk))  # C did change
    if layout == "soa":
        assert torch.equal(a, exp_xyz) and torch.equal(b, exp_rgb)
    else:
        assert np.array_equal(a.cpu().numpy(), repack(exp_xyz, exp_rgb))


# ---- 5. error paths ----
def test_write_error_paths_leave_the_output_untouched():
    from m3s.evaluate import keyframe_table, map_config, map_count

    d = dev()
    H, W, K = 16, 24, 3
    N = H * W
    Xs, Cs, Ns, rgbs = dev_case(H, W, K)
    lib = _lib.load()
    ws = torch.zeros(lib.m3s_map_workspace_size(K, N), dtype=torch.uint8, device=d)
    mc = map_config(THR, "soa")
    table = keyframe_table(Xs, Cs, Ns)
    Twc = identity_poses(K).to(d)
    out = torch.full((K * N * 12,), 0xA5, dtype=torch.uint8, device=d)

    def write(Kp, capacity, cfg=mc):
        return lib.m3s_map_write(ctypes.byref(cfg), ctypes.byref(table), _lib.ptr(Twc), None, Kp, N, _lib.ptr(out),
                                 None, capacity, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(d))

    assert write(K, K * N) == _lib.EINVAL  # no count on this workspace
    assert b"count" in lib.m3s_last_error()
    _, M = map_count(mc, table, K, N, ws, d)
    assert M > 1
    assert write(K - 1, K * N) == _lib.EINVAL  # other shapes than the count's
    assert write(K, M - 1) == _lib.EINVAL  # capacity below the total
    assert write(K, K * N, map_config(THR + 0.25, "soa")) == _lib.EINVAL  # another threshold than the count's
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert write(K, M) == 0  # and the valid call goes through
    torch.cuda.synchronize()
    assert not bool((out[:M * 12] == 0xA5).all()) and bool((out[M * 12:] == 0xA5).all())


# ---- 6. Python surface ----
def make_store(use_calib, seed=6):
    H, W, K = 48, 64, 3
    Xs, Cs, Ns, rgbs = make_case(H, W, K, seed=seed)
    T = random_poses(K, torch.Generator().manual_seed(11))
    kfs = Keyframes()
    for k in range(K):
        f = Frame(k, (H, W), T_WC=Sim3(T[k:k + 1].to(dev())))
        f.X_canon, f.C, f.N = Xs[k].to(dev()), Cs[k].reshape(-1, 1).to(dev()), Ns[k]
        f.uimg = (rgbs[k].float().reshape(H, W, 3) + 0.5) / 255.0  # host; (uimg * 255) truncates back to rgbs[k]
        if use_calib:
            f.K = intrinsics(H, W).to(dev())
        kfs.append(f)
    return kfs, T, rgbs


def _no_torch_path(monkeypatch):
    """world_points must take the HIP passes for device keyframes: its torch formulation raises from here on."""
    from m3s import evaluate

    def boom(*a, **k):
        raise AssertionError("world_points fell back to world_points_torch")

    monkeypatch.setattr(evaluate, "world_points_torch", boom)


@pytest.mark.parametrize("use_calib", [False, True])
def test_world_points_matches_torch_formulation(use_calib, tmp_path, monkeypatch):
    from m3s.evaluate import save_reconstruction, world_points, world_points_torch

    config["use_calib"] = use_calib
    kfs, T, rgbs = make_store(use_calib)
    rpts, rcols, rcounts = world_points_torch(kfs, THR)
    _no_torch_path(monkeypatch)
    pts, cols, counts = world_points(kfs, THR)
    assert pts.device.type == "cuda" and pts.dtype == torch.float32 and cols.dtype == torch.uint8
    assert torch.equal(counts, rcounts) and counts.dtype == torch.int64 and int(counts.sum()) == pts.shape[0] > 0
    assert torch.equal(cols, rcols)
    # mask and order: the colours above, and per keyframe the points within the bound of the fp64 formula
    got = torch.split(pts.cpu(), counts.tolist())
    for k in range(3):
        kf = kfs[k]
        m = (kf.C / kf.N).reshape(-1) > THR
        p = kf.X_canon if not use_calib else constrain_points_to_ray((48, 64), kf.X_canon[None], kf.K)[0]
        assert bound_ratio(got[k], p[m].cpu(), T[k]) <= 1.0
        assert torch.equal(cols.cpu()[sum(counts.tolist()[:k]):sum(counts.tolist()[:k + 1])], rgbs[k][m.cpu()])
    assert float((pts - rpts).abs().max()) < 1e-3  # and next to the fp32 torch rows (both inside the bound)
    # indices reorder
    p20, c20, n20 = world_points(kfs, THR, indices=[2, 0])
    assert n20.tolist() == [int(counts[2]), int(counts[0])]
    g = torch.split(pts, counts.tolist())
    gc = torch.split(cols, counts.tolist())
    assert torch.equal(p20, torch.cat((g[2], g[0]))) and torch.equal(c20, torch.cat((gc[2], gc[0])))
    # colors=False
    p, c, n = world_points(kfs, THR, colors=False)
    assert c is None and torch.equal(p, pts) and torch.equal(n, counts)
    rec, n = world_points(kfs, THR, layout="ply")
    assert np.array_equal(rec.cpu().numpy(), repack(pts, cols))
    # save_reconstruction: the parsed rows are world_points'
    save_reconstruction(tmp_path, "map.ply", kfs, THR)
    raw = open(tmp_path / "map.ply", "rb").read()
    end = raw.index(b"end_header\n") + 11
    assert f"element vertex {pts.shape[0]}\n".encode() in raw[:end]
    body = np.frombuffer(raw[end:], dtype=PLY_BODY)
    assert np.array_equal(body.view(np.uint8).reshape(-1, 15), repack(pts, cols))


def test_world_points_on_shared_keyframes(monkeypatch):
    """The multi-process store: slot views of the (buffer, N, 3) / (buffer, N, 1) buffers, K from the store, uimg on
    the host; the slots are read in place."""
    import multiprocessing as mp

    from m3s.evaluate import world_points, world_points_torch
    from m3s.frame import SharedKeyframes

    config["use_calib"] = True
    src, _, _ = make_store(True, seed=8)
    manager = mp.get_context("spawn").Manager()
    try:
        kfs = SharedKeyframes(manager, 48, 64, buffer=4, device="cuda", feat_dim=8)
        for k in range(3):
            kfs.append(src[k])
        kfs.set_intrinsics(src[0].K)
        rpts, rcols, rcounts = world_points_torch(kfs, THR)
        _no_torch_path(monkeypatch)
        X_before = kfs.X.clone()
        pts, cols, counts = world_points(kfs, THR)
        assert torch.equal(counts, rcounts) and torch.equal(cols, rcols) and pts.shape == rpts.shape
        assert float((pts - rpts).abs().max()) < 1e-3
        assert torch.equal(kfs.X, X_before)  # not overwritten with the constrained copy
        p1, c1, n1 = world_points(kfs, THR, indices=torch.tensor([1]))  # a viewer's dirty index tensor
        lo = int(counts[0])
        assert n1.tolist() == [int(counts[1])] and torch.equal(p1, pts[lo:lo + int(counts[1])])
        assert torch.equal(c1, cols[lo:lo + int(counts[1])])
    finally:
        manager.shutdown()
