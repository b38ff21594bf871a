"""Voxel-grid thinning of the map export on the GPU (csrc/map.hip through m3s_map_voxel and the voxel_size keyword of
m3s.evaluate.world_points): exact against the rule (m3s.evaluate.voxel_select), ties, dropped rows, the error paths
and the Python surface. The inputs are those of tests/test_gpu_map_export.py (its small helpers are copied here)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from m3s import _lib
from m3s.config import config
from m3s.frame import Frame, Keyframes
from m3s.sim3 import Sim3

pytestmark = pytest.mark.gpu

THR = 1.5
GUARD = 64
H, W, K = 48, 64, 3  # three blocks of 1024 pixels per keyframe, rows in every one of them
VOXEL_SIZES = [1e-3, 0.5, 100.0]  # no collisions, mixed, maximal contention
# make_case(48, 64, 3) has about 3600 valid rows; under identity poses without calib a CPU run of voxel_select
# gives 3604 -> 3604 / 2378 / 4 distinct voxels at these sizes (x, y of both signs, z > 0: four cells of 100)
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


def row_conf(Cs, Ns):
    """The average confidence of every exported row, in export order: (C * float32(1/N))[mask] per keyframe."""
    out = []
    for C, n in zip(Cs, Ns):
        avg = C * torch.tensor(1.0 / n, dtype=torch.float32, device=C.device)
        out.append(avg[avg > THR])
    return torch.cat(out)


def run_map(Xs, Cs, Ns, Twc, rgbs, layout, Kmat=None, size=None, voxel_size=None, capacity=None):
    """count [+ voxel] + write through the C ABI on device tensors, every output between guard bytes. Returns
    (xyz (M,3) f32, rgb (M,3) u8 or None, counts, dropped) for "soa", (records (M,15) u8, None, counts, dropped) for
    "ply". ``capacity`` (rows, default the total): the outputs are that large and filled with 0xA5; everything beyond
    the written total must still be 0xA5 afterwards."""
    from m3s.evaluate import keyframe_table, map_config, map_count, map_voxel, map_voxel_table_size, map_write

    d = dev()
    Kp, N = len(Xs), Cs[0].numel()
    lib = _lib.load()
    ws = torch.zeros(lib.m3s_map_workspace_size(Kp, N), dtype=torch.uint8, device=d)
    mc = map_config(THR, layout, Kmat, size)
    table = keyframe_table(Xs, Cs, Ns)
    Twc = Twc.to(d).contiguous()
    counts, M = map_count(mc, table, Kp, N, ws, d)
    assert counts.sum() == M
    dropped = 0
    if voxel_size is not None:
        nbytes = map_voxel_table_size(M)
        whole_t, vox = guarded(nbytes)
        counts, M2, dropped = map_voxel(mc, table, Twc, Kp, N, voxel_size, vox, ws, d)
        assert counts.sum() == M2 <= M and 0 <= dropped <= M - M2
        assert guards_intact(whole_t, nbytes)
        M = M2
    cap = M if capacity is None else capacity
    row = 15 if layout == "ply" else 12
    whole, out = guarded(cap * row)
    whole_c = out_c = None
    if layout == "soa" and rgbs is not None:
        whole_c, out_c = guarded(cap * 3)
    map_write(mc, table, Twc, rgbs, Kp, N, out, out_c, cap, ws, d)
    torch.cuda.synchronize()
    assert guards_intact(whole, cap * row) and bool((out[M * row:] == 0xA5).all())
    if whole_c is not None:
        assert guards_intact(whole_c, cap * 3) and bool((out_c[M * 3:] == 0xA5).all())
    if layout == "ply":
        return out[:M * 15].reshape(M, 15), None, counts, dropped
    xyz = out[:M * 12].view(torch.float32).reshape(M, 3)
    return xyz, None if out_c is None else out_c[:M * 3].reshape(M, 3), counts, dropped


def pack_ply(xyz, rgb):
    return torch.cat((xyz.contiguous().view(torch.uint8).reshape(-1, 12), rgb), dim=1)


def thinned_counts(counts, keep):
    owner = torch.repeat_interleave(torch.arange(len(counts), device=keep.device),
                                    torch.as_tensor(counts, device=keep.device))
    return torch.bincount(owner[keep], minlength=len(counts)).tolist()


# ---- 1. exact against the rule ----
@pytest.mark.parametrize("poses", ["identity", "random"])
@pytest.mark.parametrize("calib", [False, True])
def test_voxel_exact_against_the_rule(calib, poses):
    from m3s.evaluate import _voxel_pick, voxel_select

    Xs, Cs, Ns, rgbs = dev_case(H, W, K)
    assert Ns == [1, 2, 4]
    Kmat = intrinsics(H, W).to(dev()) if calib else None
    T = identity_poses(K) if poses == "identity" else random_poses(K, torch.Generator().manual_seed(5))
    xyz, rgb, counts, _ = run_map(Xs, Cs, Ns, T, rgbs, "soa", Kmat, (H, W))
    conf = row_conf(Cs, Ns)
    rows = xyz.shape[0]
    assert conf.numel() == rows and 3400 < rows < 4000
    # rows in at least three blocks of 1024 pixels of a keyframe, and not a multiple of the wave
    assert all(c > 0 for c in counts) and xyz.shape[0] % 64 != 0
    for vs in VOXEL_SIZES:
        keep, exp_dropped = _voxel_pick(xyz, conf, vs)
        assert torch.equal(keep, voxel_select(xyz, conf, vs))
        print(f"voxel {vs}: calib={calib} poses={poses}: {xyz.shape[0]} rows -> {keep.numel()}, dropped {exp_dropped}")
        if not calib and poses == "identity":  # the three regimes: no collisions, mixed, maximal contention
            assert exp_dropped == 0
            assert {1e-3: keep.numel() == rows, 0.5: rows // 2 < keep.numel() < rows - 500, 100.0: keep.numel() == 4}[vs]
        exp_counts = thinned_counts(counts, keep)
        vx, vr, vcounts, dropped = run_map(Xs, Cs, Ns, T, rgbs, "soa", Kmat, (H, W), voxel_size=vs)
        assert vcounts.tolist() == exp_counts and dropped == exp_dropped
        assert vx.shape == (keep.numel(), 3) and torch.equal(vx, xyz[keep]) and torch.equal(vr, rgb[keep])
        rec, _, pcounts, dropped = run_map(Xs, Cs, Ns, T, rgbs, "ply", Kmat, (H, W), voxel_size=vs)
        assert pcounts.tolist() == exp_counts and dropped == exp_dropped
        assert torch.equal(rec, pack_ply(xyz[keep], rgb[keep]))
        if vs == 1e-3 and exp_dropped == 0:
            assert keep.numel() == xyz.shape[0]
        if vs == 1e-3 and keep.numel() == xyz.shape[0]:  # no two rows share a cell: the unfiltered output
            assert torch.equal(vx, xyz) and torch.equal(vr, rgb) and vcounts.tolist() == counts.tolist()


# ---- 2. ties and cross-keyframe winners ----
def test_ties_go_to_the_first_keyframe_and_higher_confidence_wins():
    from m3s.evaluate import voxel_select

    Xs, Cs, _, rgbs = dev_case(H, W, 1, seed=2)
    Xs, Ns = [Xs[0], Xs[0].clone()], [1, 1]
    rgbs = [rgbs[0], 255 - rgbs[0]]
    T = random_poses(1, torch.Generator().manual_seed(3)).repeat(2, 1)
    # equal confidences: every survivor is keyframe 0's
    C0 = Cs[0]
    xyz, rgb, counts, _ = run_map(Xs, [C0, C0.clone()], Ns, T, rgbs, "soa", voxel_size=0.5)
    one, one_rgb, one_counts, _ = run_map(Xs[:1], [C0], Ns[:1], T[:1], rgbs[:1], "soa", voxel_size=0.5)
    assert counts[1] == 0 and 0 < counts[0] == one_counts[0] < int((C0 > THR).sum())
    assert torch.equal(xyz, one) and torch.equal(rgb, one_rgb)
    # keyframe 1 higher on a planted subset of the valid pixels: exactly those voxels' survivors are keyframe 1's
    valid = torch.nonzero(C0 > THR).flatten()
    planted = valid[torch.randperm(valid.numel(), generator=torch.Generator().manual_seed(4))[:200].to(dev())]
    C1 = C0.clone()
    C1[planted] += 100.0  # above every other row of its voxel
    Cs2 = [C0, C1]
    full, full_rgb, full_counts, _ = run_map(Xs, Cs2, Ns, T, rgbs, "soa")
    keep = voxel_select(full, row_conf(Cs2, Ns), 0.5)
    xyz, rgb, counts, dropped = run_map(Xs, Cs2, Ns, T, rgbs, "soa", voxel_size=0.5)
    assert dropped == 0 and counts.tolist() == thinned_counts(full_counts, keep)
    assert torch.equal(xyz, full[keep]) and torch.equal(rgb, full_rgb[keep])
    # by hand: a voxel's survivor is keyframe 1's iff a planted pixel lies in it
    n0 = int(full_counts[0])
    pix1 = valid[keep[keep >= n0] - n0]  # pixels of keyframe 1's survivors (both keyframes have the same valid set)
    assert set(pix1.tolist()) <= set(planted.tolist())
    cell = lambda p: {tuple(v) for v in torch.floor(p * 2.0).to(torch.int64).tolist()}
    planted_rows = n0 + torch.searchsorted(valid, planted.sort().values)
    assert cell(xyz[int(counts[0]):]) == cell(full[planted_rows]) and counts[1] == len(cell(full[planted_rows]))
    assert not (cell(xyz[:int(counts[0])]) & cell(full[planted_rows]))


# ---- 3. dropped rows ----
def test_dropped_rows_are_counted_and_absent():
    from m3s.evaluate import _voxel_pick

    Xs, Cs, Ns, rgbs = dev_case(H, W, K, seed=5)
    Xs = [x.clone() for x in Xs]
    n_bad = 0
    for k, X in enumerate(Xs):  # NaN and Inf at valid pixels, in every keyframe
        valid = torch.nonzero(Cs[k] / Ns[k] > THR).flatten()
        X[valid[3:40:6], k % 3] = float("nan")
        X[valid[100:130:7], (k + 1) % 3] = float("inf")
        X[valid[-1], 2] = float("-inf")
        n_bad += len(range(3, 40, 6)) + len(range(100, 130, 7)) + 1
    T = identity_poses(K)
    full, full_rgb, full_counts, _ = run_map(Xs, Cs, Ns, T, rgbs, "soa")
    M = full.shape[0]
    assert int((~torch.isfinite(full).all(dim=1)).sum()) == n_bad
    conf = row_conf(Cs, Ns)
    keep, exp_dropped = _voxel_pick(full, conf, 0.5)
    assert exp_dropped == n_bad
    for layout in ("soa", "ply"):
        a, b, counts, dropped = run_map(Xs, Cs, Ns, T, rgbs, layout, voxel_size=0.5, capacity=M)
        assert dropped == n_bad and counts.tolist() == thinned_counts(full_counts, keep)
        if layout == "soa":
            assert bool(torch.isfinite(a).all()) and torch.equal(a, full[keep]) and torch.equal(b, full_rgb[keep])
        else:
            assert torch.equal(a, pack_ply(full[keep], full_rgb[keep]))
    # out of range: keyframe 1 translated by 100 at voxel size 1e-5 lies 1e7 cells out
    T = identity_poses(K)
    T[1, :3] = 100.0
    full, full_rgb, full_counts, _ = run_map(Xs, Cs, Ns, T, rgbs, "soa")
    keep, exp_dropped = _voxel_pick(full, conf, 1e-5)
    assert exp_dropped >= int(full_counts[1]) and keep.numel() > 0
    a, b, counts, dropped = run_map(Xs, Cs, Ns, T, rgbs, "soa", voxel_size=1e-5, capacity=M)
    print(f"out of range: {M} rows, {dropped} dropped, {a.shape[0]} kept")
    assert dropped == exp_dropped and counts[1] == 0 and counts.tolist() == thinned_counts(full_counts, keep)
    assert torch.equal(a, full[keep]) and torch.equal(b, full_rgb[keep])
    # everything out of range: an empty cloud, nothing written
    T[:, :3] = 100.0
    a, b, counts, dropped = run_map(Xs, Cs, Ns, T, rgbs, "ply", voxel_size=1e-5, capacity=M)
    assert a.shape[0] == 0 and counts.tolist() == [0, 0, 0] and dropped == M


# ---- 4. error paths on a live workspace ----
def test_voxel_error_paths_leave_the_mask_untouched():
    from m3s.evaluate import keyframe_table, map_config, map_count, map_voxel_table_size, map_write

    d = dev()
    N = H * W
    Xs, Cs, Ns, rgbs = dev_case(H, W, K)
    T = random_poses(K, torch.Generator().manual_seed(5)).to(d)
    exp_xyz, exp_rgb, exp_counts, _ = run_map(Xs, Cs, Ns, T, rgbs, "soa")
    lib = _lib.load()
    ws = torch.zeros(lib.m3s_map_workspace_size(K, N), dtype=torch.uint8, device=d)
    mc = map_config(THR, "soa")
    table = keyframe_table(Xs, Cs, Ns)
    vox = torch.full((map_voxel_table_size(K * N),), 0x5A, dtype=torch.uint8, device=d)

    def voxel(Kp=K, cfg=mc, table_bytes=None, size=0.5):
        total, dropped = ctypes.c_int64(-7), ctypes.c_int64(-7)
        rc = lib.m3s_map_voxel(ctypes.byref(cfg), ctypes.byref(table), _lib.ptr(T), Kp, N, size, _lib.ptr(vox),
                               vox.numel() if table_bytes is None else table_bytes, None, ctypes.byref(total),
                               ctypes.byref(dropped), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(d))
        assert rc != 0 and total.value == -7 and dropped.value == -7
        return rc

    assert voxel() == _lib.EINVAL  # no count on this workspace
    assert b"count" in lib.m3s_last_error()
    counts, M = map_count(mc, table, K, N, ws, d)
    assert M == exp_xyz.shape[0]
    before = ws.clone()
    assert voxel(Kp=K - 1) == _lib.EINVAL  # another Kp than the count's
    assert voxel(cfg=map_config(THR + 0.25, "soa")) == _lib.EINVAL  # another threshold
    assert voxel(table_bytes=map_voxel_table_size(M) - 16) == _lib.ESPACE  # a short table
    assert b"table" in lib.m3s_last_error()
    assert voxel(size=0.0) == _lib.EINVAL and voxel(size=float("nan")) == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(ws, before) and bool((vox == 0x5A).all())  # the mask, the offsets and the table: as they were
    out = torch.empty((M, 3), dtype=torch.float32, device=d)
    out_rgb = torch.empty((M, 3), dtype=torch.uint8, device=d)
    map_write(mc, table, T, rgbs, K, N, out, out_rgb, M, ws, d)  # a plain write still gives the unfiltered rows
    assert torch.equal(out, exp_xyz) and torch.equal(out_rgb, exp_rgb) and counts.tolist() == exp_counts.tolist()


# ---- 5. Python surface ----
def make_store(use_calib, seed=6):
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
    return kfs


def _no_torch_path(monkeypatch):
    """world_points must take the HIP passes for device keyframes: its torch formulation raises from here on."""
    from m3s import evaluate

    def boom(*a, **k):
        raise AssertionError("world_points fell back to world_points_torch")

    monkeypatch.setattr(evaluate, "world_points_torch", boom)


def store_conf(kfs, order):
    out = []
    for k in order:
        avg = (kfs[k].C / kfs[k].N).reshape(-1)
        out.append(avg[avg > THR])
    return torch.cat(out)


def check_surface(kfs, tmp_path):
    """world_points(voxel_size=0.5) against voxel_select over the unthinned world_points, on the HIP path."""
    from m3s.evaluate import save_reconstruction, voxel_select, world_points

    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # nothing is dropped here: no warning either
        pts, cols, counts = world_points(kfs, THR)
        keep = voxel_select(pts, store_conf(kfs, range(K)), 0.5)
        assert 0 < keep.numel() < pts.shape[0]
        vp, vc, vn = world_points(kfs, THR, voxel_size=0.5)
        assert vp.device.type == "cuda" and vn.dtype == torch.int64 and vn.device == vp.device
        assert torch.equal(vp, pts[keep]) and torch.equal(vc, cols[keep])
        assert vn.tolist() == thinned_counts(counts.tolist(), keep)
        # indices select and order the table: g follows it, so ties go to the first listed keyframe
        p20, c20, n20 = world_points(kfs, THR, indices=[2, 0])
        keep20 = voxel_select(p20, store_conf(kfs, [2, 0]), 0.5)
        vp20, vc20, vn20 = world_points(kfs, THR, indices=[2, 0], voxel_size=0.5)
        assert torch.equal(vp20, p20[keep20]) and torch.equal(vc20, c20[keep20])
        assert vn20.tolist() == thinned_counts(n20.tolist(), keep20)
        p, c, n = world_points(kfs, THR, colors=False, voxel_size=0.5)
        assert c is None and torch.equal(p, vp) and torch.equal(n, vn)
        rec, n = world_points(kfs, THR, layout="ply", voxel_size=0.5)
        assert torch.equal(rec, pack_ply(vp, vc)) and torch.equal(n, vn)
        save_reconstruction(tmp_path, "thin.ply", kfs, THR, voxel_size=0.5)
        raw = open(tmp_path / "thin.ply", "rb").read()
        end = raw.index(b"end_header\n") + 11
        assert f"element vertex {vp.shape[0]}\n".encode() in raw[:end]
        assert raw[end:] == pack_ply(vp, vc).cpu().numpy().tobytes()
        # None is the unthinned export, also right after a thinned one on the same cached workspace
        p, c, n = world_points(kfs, THR, voxel_size=None)
        assert torch.equal(p, pts) and torch.equal(c, cols) and torch.equal(n, counts)
    return pts, counts


@pytest.mark.parametrize("use_calib", [False, True])
def test_world_points_voxel_size_on_keyframes(use_calib, tmp_path, monkeypatch):
    from m3s.evaluate import world_points

    config["use_calib"] = use_calib
    kfs = make_store(use_calib)
    _no_torch_path(monkeypatch)
    pts, counts = check_surface(kfs, tmp_path)
    # identical keyframes listed twice: every survivor belongs to the first listed one
    vp, _, vn = world_points(kfs, THR, indices=[1, 1], voxel_size=0.5)
    assert vn[1] == 0 and 0 < vn[0] <= counts[1]
    # dropped rows: one RuntimeWarning that names their number
    valid = torch.nonzero((kfs[0].C / kfs[0].N).reshape(-1) > THR).flatten()
    kfs[0].X_canon[valid[:5], 2] = float("nan")
    with pytest.warns(RuntimeWarning, match=r"\b5 rows") as rec:
        vp, _, _ = world_points(kfs, THR, voxel_size=0.5)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1 and bool(torch.isfinite(vp).all())


def test_world_points_voxel_size_on_shared_keyframes(tmp_path, monkeypatch):
    import multiprocessing as mp

    from m3s.frame import SharedKeyframes

    config["use_calib"] = True
    src = make_store(True, seed=8)
    manager = mp.get_context("spawn").Manager()
    try:
        kfs = SharedKeyframes(manager, H, W, buffer=4, device="cuda", feat_dim=8)
        for k in range(K):
            kfs.append(src[k])
        kfs.set_intrinsics(src[0].K)
        _no_torch_path(monkeypatch)
        X_before = kfs.X.clone()
        check_surface(kfs, tmp_path)
        assert torch.equal(kfs.X, X_before)
    finally:
        manager.shutdown()
