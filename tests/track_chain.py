"""The tracker chain on the oracle (test infrastructure, CPU): tracker.py:28-114 with O.match, the fp64 opt_pose_*
restatement and the weighted_pointmap fusion. Shared by the CPU pin against the reference run
(tests/test_oracle.py) and the GPU config-size tests (tests/test_gpu_configs.py)."""
import numpy as np

import oracle.oracle as O

I8 = np.array([0, 0, 0, 0, 0, 0, 1, 1.0])


def oracle_track_from_matches(mode, idx, valid_match, Xff, Cff, Qff, Xkf, Ckf, Qkf, kf_X, kf_C, kf_N, T_WCf, T_WCk, K,
                              img_size, C_conf=0.0, Q_conf=1.5, min_match_frac=0.05, match_frac_thresh=0.333,
                              depth_eps=1e-6, fixed_iters=None, trace=None, **opt):
    """tracker.py:28-114 on given matches (what mast3r_match_asymmetric returned, without the batch dimension):
    idx (N,) frame pixel of every keyframe pixel, valid_match (N,), the frame's and the keyframe's view of the pair
    Xff/Cff/Qff and Xkf/Ckf/Qkf (float32), the keyframe record kf_X (its X_canon), kf_C (the confidence sum), kf_N,
    both poses, K, (H, W). The frame is a fresh one (its pointmap is Xff, Cff, N = 1). ``opt``: further
    track_rays / track_calib keywords (sigmas, huber_k, pixel_border, max_iters, rel_error, delta_norm).

    Returns a dict: status ("ok" | "max_iters" | "skipped" | "cholesky"), T_WCf, T_CkCf, iters, n_valid_opt,
    n_valid_kf, n_unique, new_kf, X (the fused keyframe points, fp64), C (the fused sum, float32), Ck_avg / Cf_avg
    (the float32 quotients C / N of frame.py:83-84 after the update). A skipped or failed frame leaves the keyframe
    alone: X, C are the inputs, the poses None and the averages None."""
    H, W = img_size
    f32 = np.float32
    i = np.asarray(idx).reshape(-1)
    vm = np.asarray(valid_match).reshape(-1).astype(bool)
    n = i.size
    Xff, Xkf, kf_X = (np.asarray(a, f32).reshape(-1, 3) for a in (Xff, Xkf, kf_X))
    Cff, Qff, Ckf, Qkf, kf_C = (np.asarray(a, f32).reshape(-1) for a in (Cff, Qff, Ckf, Qkf, kf_C))
    Qk = np.sqrt(Qff[i] * Qkf)  # float32, like the tensors of tracker.py:41
    Cf_avg = Cff / f32(1)  # frame.update_pointmap on a fresh frame: N = 1
    Ck_avg = kf_C / f32(kf_N)
    valid_kf = vm & (Qk > f32(Q_conf))
    v = valid_kf & (Cf_avg[i] > f32(C_conf)) & (Ck_avg > f32(C_conf))
    out = {"status": "skipped", "T_WCf": None, "T_CkCf": None, "iters": 0, "n_valid_opt": int(v.sum()),
           "n_valid_kf": int(valid_kf.sum()), "n_unique": int(np.unique(i[vm]).size), "new_kf": False,
           "X": kf_X.astype(np.float64), "C": kf_C.copy(), "Ck_avg": None, "Cf_avg": None, "Qk": Qk, "valid_opt": v}
    if f32(out["n_valid_opt"]) / f32(n) < f32(min_match_frac):  # tracker.py:67-70 (float32 tensors)
        return out
    trace = [] if trace is None else trace  # the status needs the last step's convergence test
    try:
        if mode == "rays":
            Tf, Tr, it = O.track_rays(Xff[i], kf_X, T_WCf, T_WCk, Qk, v, fixed_iters=fixed_iters, trace=trace, **opt)
        else:
            Xf = O.backproject_constrain(Xff[None], K, (H, W))[0][i]
            z = O.backproject_constrain(kf_X[None], K, (H, W))[0][:, 2]
            u, vv = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32), indexing="xy")
            vmk = z > depth_eps
            meas = np.stack((u.reshape(-1), vv.reshape(-1), np.log(np.where(vmk, z, 1.0))), -1) * vmk[:, None]
            Tf, Tr, it = O.track_calib(Xf, kf_X, T_WCf, T_WCk, Qk, v, meas, vmk, K, (H, W), depth_eps=depth_eps,
                                       fixed_iters=fixed_iters, trace=trace, **opt)
    except np.linalg.LinAlgError:
        out["status"] = "cholesky"
        return out
    max_iters = opt.get("max_iters", 50) if fixed_iters is None else fixed_iters
    out.update(T_WCf=Tf, T_CkCf=Tr, iters=it)
    # the step that reached max_iters may have converged too; the status then says ok (gn_step tests conv first)
    out["status"] = "max_iters" if it >= max_iters and not _last_step_converged(trace, opt) else "ok"
    Xkk = O.sim3_act(Tr, Xkf.astype(np.float64))
    kC, Cn = kf_C.astype(np.float64)[:, None], Ckf.astype(np.float64)[:, None]
    out["X"] = (kC * kf_X.astype(np.float64) + Cn * Xkk) / (kC + Cn)  # frame.py:74-77, weighted_pointmap
    out["C"] = kf_C + Ckf
    out["Ck_avg"] = out["C"] / f32(kf_N + 1)
    out["Cf_avg"] = Cf_avg
    out["new_kf"] = bool(min(out["n_valid_kf"] / n, out["n_unique"] / n) < match_frac_thresh)
    return out


def _last_step_converged(trace, opt):
    """Whether the last traced step passed the convergence test."""
    t = trace[-1]
    return bool(t["rel"] < opt.get("rel_error", 1e-3) or t["tau_norm"] < opt.get("delta_norm", 1e-3))


def oracle_track(P, mode, H, W):
    """tracker.py:28-114 on the oracle: match, Qk, valid_opt, opt_pose_* (fp64), keyframe fusion. The frame is
    never skipped (min_match_frac 0), as this helper always ran the solve."""
    X, C, D, Q = (P[k].numpy() for k in ("X", "C", "D", "Q"))
    idx, valid = O.match(X[:1], X[1:], D[:1], D[1:])
    r = oracle_track_from_matches(mode, idx[0], valid[0, :, 0], X[0], C[0], Q[0], X[1], C[1], Q[1], P["Xk"].numpy(),
                                  P["Ck"].numpy()[:, 0], 1, I8, I8, P["K"].numpy(), (H, W), min_match_frac=0.0)
    return idx, valid, r["T_WCf"], r["X"], r["iters"]


def oracle_track_seq(pairs, H, W, mode="calib"):
    """tracker.py:28-114 over a sequence of frames against one keyframe (calib or rays mode) on the oracle: each frame
    matched from the previous frame's idx_f2k (reset on new_kf), started at the previous frame's pose, the keyframe
    fused by weighted_pointmap after every frame (frame.py:74-77: X <- (C X + C' X') / (C + C'), C <- C + C',
    N <- N + 1; the tracker's Ck is the average C / N). Returns [(T_WCf, iters, new_kf)] per frame and the final
    keyframe (X, C, N)."""
    P0 = pairs[0]
    K = P0["K"].numpy()
    kX = P0["Xk"].numpy().astype(np.float64)
    kC = P0["Ck"].numpy()[:, 0].astype(np.float64)
    kN = 1
    T = I8.copy()
    idx_prev = None
    out = []
    u, vv = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    for P in pairs:
        X, C, D, Q = (P[k].numpy() for k in ("X", "C", "D", "Q"))
        idx, valid = O.match(X[:1], X[1:], D[:1], D[1:], idx_prev)
        i, vm = idx[0], valid[0, :, 0]
        Qk = np.sqrt(Q[0].reshape(-1)[i] * Q[1].reshape(-1))
        Ck = (kC / kN).astype(np.float32)
        v = vm & (C[0].reshape(-1)[i] > 0.0) & (Ck > 0.0) & (Qk > 1.5)
        Xk32 = kX.astype(np.float32)
        if mode == "rays":
            Tf, Tr, it = O.track_rays(X[0].reshape(-1, 3)[i], Xk32, T, I8, Qk, v)
        else:
            Xf = O.backproject_constrain(X[0].reshape(1, -1, 3), K, (H, W))[0][i]
            z = O.backproject_constrain(Xk32[None], K, (H, W))[0][:, 2]
            vmk = z > 1e-6
            meas = np.stack((u.reshape(-1), vv.reshape(-1), np.log(np.where(vmk, z, 1.0))), -1) * vmk[:, None]
            Tf, Tr, it = O.track_calib(Xf, Xk32, T, I8, Qk, v, meas, vmk, K, (H, W))
        valid_kf = vm & (Qk > 1.5)
        n_unique = np.unique(i[vm]).size
        new_kf = min(valid_kf.sum() / i.size, n_unique / i.size) < 0.333
        Xkk = O.sim3_act(Tr, X[1].reshape(-1, 3).astype(np.float64))
        Cf1 = C[1].reshape(-1).astype(np.float64)
        kX = (kC[:, None] * kX + Cf1[:, None] * Xkk) / (kC + Cf1)[:, None]
        kC = kC + Cf1
        kN += 1
        out.append((Tf, it, bool(new_kf)))
        T = Tf.astype(np.float32).astype(np.float64)  # the next frame starts at this frame's (fp32) pose
        idx_prev = None if new_kf else idx
    return out, kX, kC, kN
