/*
 * m3s.h — C ABI of the MI355X-native MASt3R-SLAM tracking hot path (libm3s.so).
 *
 * Plain pointers and sizes only (no torch types). All array pointers are DEVICE pointers on the
 * current HIP device unless the comment says "host"; `stream` is a hipStream_t passed as void*
 * (NULL = default stream). Every entry point returns 0 on success or a negative M3S_E* code; the
 * message of the last failure on the calling thread is available from m3s_last_error().
 *
 * Each entry point replaces one operator of the reference's native extension
 * `mast3r_slam_backends` (bindings /root/reference/mast3r_slam/backend/src/gn.cpp:116-123,
 * declarations backend/include/gn.h) or fuses a stretch of the reference's Python glue
 * (mast3r_slam/matching.py, tracker.py). The Python module `mast3r_slam_backends` in
 * lightweight-mast3r-slam_amd/ binds these through ctypes.
 */
#ifndef M3S_H
#define M3S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3S_ABI_VERSION 10

#define M3S_OK 0
#define M3S_EINVAL -1  /* bad shape / argument (reference: TORCH_CHECK -> RuntimeError) */
#define M3S_EHIP -2    /* HIP launch / runtime failure */
#define M3S_ESPACE -3  /* workspace too small */
#define M3S_ESTALL -4  /* global BA: a bounded dataflow hand-off wait of the factorisation timed out (a schedule
                        * fault, not a non-positive pivot): the GN loop stopped; reported by m3s_ba_iterations and
                        * m3s_gauss_newton. A non-positive pivot keeps the reference contract (dx = 0, no error). */

int m3s_abi_version(void);
const char* m3s_last_error(void);

/* Per-kernel HIP-event timing (no reference counterpart; the reference's profiler.py wraps regions
 * with torch.cuda.synchronize). When enabled, every launch group is bracketed by hipEvents on its
 * own stream under a name: prep_rays, proj_occlusion, refine_lin, track_setup, gn_iters,
 * ba_linearize, ba_solve, map_count, map_voxel, map_write, quantize_topk, asmk_update (the whole fused call, the
 * quantiser's span inside it), rope2d, head_post, ingest. query synchronises the recorded events. (m3s_match runs the
 * projection search inside the refine launch where the tile path is taken: refine_lin then covers both and
 * proj_occlusion has no spans, count 0; M3S_MATCH_FUSE_PROJ=0 separates them.) */
void m3s_timing_enable(int on);
void m3s_timing_reset(void);
int m3s_timing_query(const char* name, double* total_ms, int* count);

/* ---------------------------------------------------------------------------------------------
 * Reference operators (drop-in for mast3r_slam_backends.*)
 * ------------------------------------------------------------------------------------------- */

/* iter_proj(rays_img_with_grad, pts_3d_norm, p_init, max_iter, lambda_init, cost_thresh)
 *   -> [p_new, converged]                                   gn.cpp:84-99, gn.h:89-95,
 *                                                           matching_kernels.cu:119-316
 * rays (B,H,W,C=9) f32, pts (B,N,3) f32, p_init (B,N,2) f32 -> p_new (B,N,2) f32, converged (B,N) u8 */
int m3s_iter_proj(const float* rays, const float* pts, const float* p_init, float* p_new, uint8_t* converged,
                  int B, int H, int W, int C, int N, int max_iter, float lambda_init, float cost_thresh,
                  void* stream);

/* refine_matches(D11, D21, p1, radius, dilation_max) -> [p1_new]
 *                                                           gn.cpp:101-114, gn.h:112-117,
 *                                                           matching_kernels.cu:25-116
 * dtype 0 = f16 (c10::Half step rounding), 1 = f32. D11 (B,H,W,F), D21 (B,N,F), p1 (B,N,2) i64
 * -> p1_new (B,N,2) i64 */
int m3s_refine_matches(int dtype, const void* D11, const void* D21, const int64_t* p1, int64_t* p1_new, int B,
                       int H, int W, int F, int N, int radius, int dilation_max, void* stream);

/* gauss_newton_{points,rays,calib}(Twc, Xs, Cs, [K,] ii, jj, idx_ii2jj, valid_match, Q, ...) -> [dx]
 *                                                           gn.cpp:3-82, gn.h:22-87,
 *                                                           gn_kernels.cu:725-811, 1140-1228, 1546-1637
 * Twc (Kp,8) f32 is updated IN PLACE (as the reference). Xs (Kp,N,3), Cs (Kp,N) f32; ii, jj (E) i64
 * global keyframe ids (remapped to dense ranks internally, gn_kernels.cu:161-170); idx (E,N) i64;
 * valid (E,N) u8; Q (E,N) f32. dx_out ((Kp-1),7) f32 receives the last step. iters_out (host,
 * nullable) receives the iteration count. The workspace must hold m3s_ba_workspace_size() bytes.
 * mode 3 (M3S_BA_MODE_CALIB_RAW): the residuals and results of mode 2 on constrain_points_to_ray(points)
 * (geometry.py:37-42, global_opt.py:176), with the points in Xs / the keyframe table NOT constrained: the kernels
 * read only the depth z of a point and form the target point X_j = (z x_of_u[u], z y_of_v[v], z) of pixel (u, v)
 * from the plan's ray tables (m3s_ba_calib_rays), so a caller passes the keyframes' raw X_canon and makes no
 * constrained copy. Same checks as mode 2: N == height * width, height and width below 65536. */
#define M3S_BA_MODE_CALIB_RAW 3
typedef struct m3s_ba_config {
  int mode;          /* 0 points, 1 rays, 2 calib (points on their pixel rays), 3 M3S_BA_MODE_CALIB_RAW */
  float sigma_a;     /* sigma_point | sigma_ray | sigma_pixel */
  float sigma_b;     /* -           | sigma_dist | sigma_depth */
  float C_thresh, Q_thresh;
  float fx, fy, cx, cy; /* calib: K[0,0], K[1,1], K[0,2], K[1,2] (host values) */
  int height, width, pixel_border;
  float z_eps;
} m3s_ba_config;

/* Kp <= M3S_BA_MAX_POSES: the workspace is sized for the densest factor pattern of Kp poses (no edges are known
 * to the size query): nb (nb + 1) / 2 blocks of 512 B for nb = Kp - 1, 4.3 GB at the cap. */
#define M3S_BA_MAX_POSES 4096
size_t m3s_ba_workspace_size(int Kp, int N, int E);
int m3s_gauss_newton(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp, int N,
                     const int64_t* ii, const int64_t* jj, int E, const int64_t* idx, const uint8_t* valid,
                     const float* Q, int max_iter, float delta_thresh, float* dx_out, int* iters_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Split BA for edge-sharded multi-GPU runs (no reference counterpart).
 * plan: rank remap + block-sparse assembly pattern for ALL E edges, shard = edges [e0, e1).
 * Per iteration: m3s_ba_linearize (this shard's rows of the (E,36) f64 edge-sum table), then the
 * caller all-reduces that table (offset/size from m3s_ba_edge_sums), then m3s_ba_solve. */
typedef struct m3s_ba_plan { unsigned char opaque[768]; } m3s_ba_plan;
int m3s_ba_make_plan(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp, int N,
                     const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                     const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out, void* workspace,
                     size_t workspace_bytes, m3s_ba_plan* plan, void* stream);
/* Zero-copy keyframe source: instead of the stacked Xs / Cs that
 * FactorGraph.get_poses_points builds with torch.stack (global_opt.py:114-121), the keyframes' own buffers.
 * Host arrays of Kp entries: X[k] -> that keyframe's (N,3) X_canon, C[k] -> its (N) confidence sum (device
 * pointers), N_avg[k] = its fusion count N; the average confidence is C * float32(1/N), exactly
 * Frame.get_average_conf (frame.py:93-94) on a torch device. Same plan and results as m3s_ba_make_plan.
 * In every mode: rays (solve_GN_rays) and, with mode 3, calib (solve_GN_calib), whose stacked path otherwise
 * copies the points twice (torch.stack, then constrain_points_to_ray) before each solve. */
typedef struct m3s_ba_keyframes {
  const float* const* X;
  const float* const* C;
  const float* N_avg;
} m3s_ba_keyframes;
int m3s_ba_make_plan_kf(const m3s_ba_config* cfg, float* Twc, const m3s_ba_keyframes* kf, int Kp, int N,
                        const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                        const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out, void* workspace,
                        size_t workspace_bytes, m3s_ba_plan* plan, void* stream);
/* Record reuse across successive plans on ONE workspace (no reference counterpart; the reference backend calls
 * solve_GN once per new keyframe, main.py:150-155, and re-gathers every edge each time). Between two such calls
 * the edge set only grows and tracking changes only the keyframes it fuses into, so most edges' point records
 * (ba_pack: matched point or pixel + folded validity weight) are still valid in the workspace. With reuse ids a
 * plan packs only the edges that are new to the workspace or touch a keyframe whose points, confidences or
 * fusion count changed since the workspace's previous plan (an exact bit compare on the device against copies
 * the library keeps per keyframe); the other edges keep their records. Results are bit-identical to the plain
 * plan. edge_uid (E entries, host): a stable id per directed edge naming immutable match data (its idx / valid /
 * Q rows; FactorGraph uses 2u + direction for undirected edge u); kf_uid (Kp entries, host): a stable id per
 * pose rank (the keyframe's global index). Contract: between reuse plans the workspace holds nothing else (a
 * plain plan on it drops the cache); call m3s_ba_reuse_release(workspace) before freeing or repurposing it
 * (frees the keyframe copies, 16 B per keyframe point). */
typedef struct m3s_ba_reuse {
  const int64_t* edge_uid;
  const int64_t* kf_uid;
} m3s_ba_reuse;
int m3s_ba_make_plan_reuse(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp, int N,
                           const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                           const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out,
                           const m3s_ba_reuse* reuse, void* workspace, size_t workspace_bytes, m3s_ba_plan* plan,
                           void* stream);
int m3s_ba_make_plan_kf_reuse(const m3s_ba_config* cfg, float* Twc, const m3s_ba_keyframes* kf, int Kp, int N,
                              const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                              const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out,
                              const m3s_ba_reuse* reuse, void* workspace, size_t workspace_bytes, m3s_ba_plan* plan,
                              void* stream);
/* packed_edges: shard edges the plan's pack wrote; changed_keyframes: keyframes found changed (all without reuse) */
int m3s_ba_reuse_info(const m3s_ba_plan* plan, int* packed_edges, int* changed_keyframes);
int m3s_ba_reuse_release(const void* workspace);
/* The library keeps per-workspace host state for BA plans (the symbolic analysis a plan's solves use). Call
 * m3s_ba_plan_release(workspace) once no plan on `workspace` will be solved again and before freeing or repurposing
 * it (m3s_ba_reuse_release does it too); it joins a pending analysis and frees its tables. */
int m3s_ba_plan_release(const void* workspace);
/* Diagnostic: how many workspaces currently hold BA plan state (a leak check for callers that cache workspaces). */
int m3s_ba_plan_count(void);
int m3s_ba_edge_sums(const m3s_ba_plan* plan, size_t* byte_offset, size_t* byte_count);
int m3s_ba_linearize(const m3s_ba_plan* plan, void* stream);
int m3s_ba_solve(const m3s_ba_plan* plan, void* stream);
int m3s_ba_iterations(const m3s_ba_plan* plan, int* iters_out, void* stream); /* syncs the stream */
/* Host-only facts of a built plan (bench rooflines, tests): info[0] = linearisation chunks per edge,
 * [1] = factor blocks, [2] = elimination-tree levels, [3] = multi-workgroup factor steps, [4] = 1 if the dense
 * fallback factorisation is used, [5] = distinct target keyframes among the shard's edges, [6] = shard edges,
 * [7] = poses, [8..12] = 0 (round 5's opt-in solver phases, removed in round 6). info holds 13 ints. */
int m3s_ba_plan_info(const m3s_ba_plan* plan, int* info);
/* Host-only diagnostic of the symbolic factorisation the plan builds for these edges (host arrays):
 * stats[0] = factor blocks (7x7, diagonal included), [1] = elimination-tree levels, [2] = update groups
 * (source level, target column), [3] = update sources, [4] = source-map entries, [5] = groups run by
 * factor tasks. */
int m3s_ba_pattern_stats(const int64_t* ii, const int64_t* jj, int E, int Kp, int* stats);
/* Host-only: the pixel-ray tables a mode-3 plan builds for cfg (fx, fy, cx, cy, width, height; host arrays of width
 * and height floats): x_of_u[u] = (float(u) - cx) / fx, y_of_v[v] = (float(v) - cy) / fy, each one fp32 subtraction
 * then one correctly rounded fp32 division (geometry.backproject's operation order; not a reciprocal-multiply). */
int m3s_ba_calib_rays(const m3s_ba_config* cfg, float* x_of_u, float* y_of_v);

/* curope.rope_2d(tokens, positions, base, fwd)              the reference's second native extension, the ViT's
 *                                                           RoPE2D: croco/models/curope/curope.cpp:49-65 (binding
 *                                                           and checks), kernels.cu:17-108 (kernel and launcher),
 *                                                           curope2d.py:6-9 (`import curope`)
 * tokens (B,N,H,D) f16 / f32 / bf16 (dtype 0 / 1 / 2), D % 4 == 0, Q = D / 4, rotated IN PLACE (as the reference).
 * Element strides: stride_b and stride_n are arbitrary (the caller's q and k are views of the fused qkv buffer,
 * blocks.py:99-105, token stride 3 H D); the head stride is D and the last 1 (kernels.cu:91). pos (B,N,2) i64
 * contiguous, y then x. For axis a in {0, 1}, head h and t < Q, with u = tok[b,n,h, 2 a Q + t] and
 * v = tok[b,n,h, 2 a Q + Q + t]: u' = u c - v s, v' = v c + u s, c, s = cos, sin(fwd pos[b,n,a] / base^(t/Q));
 * fwd is F0, or -F0 in the backward pass of the reference's autograd function (curope2d.py:25-29).
 * Numerics (the reference evaluates powf, cosf and sinf in fp32 in every thread, kernels.cu:44,52-54): c and s come
 * from a table the library caches per (device, base, fwd, Q): for p in [0, 1024), host fp64
 * inv = double(fwd) / pow(double(base), double(t) / Q), a = p inv, c = float(cos(a)), s = float(sin(a)), uploaded
 * synchronously on first use. The kernel computes in fp32 exactly as written above, two products and one sum per
 * output with no contraction, and rounds once (nearest even) to the token dtype. A position outside [0, 1024),
 * negative ones included, takes the same formula in fp64 on the device (a = p inv[t], device cos / sin, rounded to
 * fp32): the operator is total without a host look at the positions. f64 tokens have no dtype code (the reference
 * computes them in float, and the ViT has none).
 * 16-byte accesses are used when Q * sizeof(dtype) % 16 == 0 and tokens, stride_b and stride_n are 16-byte aligned;
 * every other legal shape takes one element per lane. The launch is asynchronous on `stream`; B N H == 0 launches
 * nothing. M3S_EINVAL: bad dtype, D % 4 != 0, a negative size, a null pointer with non-empty work, base not finite
 * and positive.
 * m3s_rope2d_prepare builds and uploads the table of (base, fwd, Q) on the current device if it is not cached: call
 * it once before capturing m3s_rope2d into a graph (the first use of a table allocates and copies, which a capture
 * forbids). m3s_rope2d_table is host-only, like m3s_ba_calib_rays: the host code that fills the device table writes
 * its first P rows, P x Q floats each, to cos_out and sin_out (host). m3s_rope2d_release frees the current device's
 * cached tables (after the device's pending work); a later call builds them again. */
int m3s_rope2d(int dtype /* 0 f16, 1 f32, 2 bf16 */, void* tokens, int64_t stride_b, int64_t stride_n,
               const int64_t* pos, int B, int N, int H, int D, float base, float fwd, void* stream);
int m3s_rope2d_prepare(float base, float fwd, int Q, void* stream);
int m3s_rope2d_table(float base, float fwd, int Q, int P, float* cos_out, float* sin_out);
int m3s_rope2d_release(void);

/* postprocess(out, depth_mode, conf_mode, desc_dim, desc_mode, two_confs, desc_conf_mode)
 *   -> pts3d, conf, desc, desc_conf                         thirdparty/mast3r/mast3r/catmlp_dpt_head.py:25-39, with
 *                                                           the tail of Cat_MLP_LocalFeatures_DPT_Pts3d.forward in
 *                                                           front (:82-95: transpose, view, pixel_shuffle, cat),
 *                                                           dust3r/heads/postprocess.py:22-55 (reg_dense_depth,
 *                                                           reg_dense_conf) inside and the downsample of
 *                                                           mast3r_slam/mast3r_utils.py:69-78 behind it
 * One streaming launch, f32 only. Channels of a pixel: 0..2 xyz, 3 the conf logit, 4..4+F-1 the descriptor, 4+F the
 * desc_conf logit when two_confs (tc = 1, else 0). F in 1..32.
 * layout M3S_HEAD_CAT: a = out (B, 4+F+tc, H, W) contiguous, the argument of the reference's postprocess; feat unused;
 * any H, W. layout M3S_HEAD_TOKENS: a = pts (B, 4, H, W), the DPT output, and feat (B, S, (F+tc) 256), the MLP output
 * before transpose / view / pixel_shuffle, S = (H/16)(W/16): channel c of pixel (y, x) is
 * feat[b, (y/16)(W/16) + x/16, c 256 + (y%16) 16 + x%16]; H and W multiples of 16 (patch 16 only).
 * Outputs, contiguous, over the pixels [::step, ::step] (H' = ceil(H/step), W' = ceil(W/step); a stepped-over pixel is
 * not read): X (B,H',W',3), C (B,H',W'), D (B,H',W',F), Q (B,H',W').
 * Modes: depth ('exp', -inf, inf); conf and desc_conf ('exp', vmin, vmax), vmin finite and vmax > vmin (inf included;
 * the desc_conf bounds are read only when two_confs); desc 'norm'. Arithmetic, fp32 in this order without contraction:
 *   d = sqrt((x x + y y) + z z);  X = (xyz / (d < 1e-8 ? 1e-8 : d)) expm1(d)
 *   C = float(vmin) + min(exp(l), float(vmax - vmin)), the difference taken in double as Python takes it; Q likewise on
 *   its own logit and bounds, or C's bits without two_confs
 *   D = desc / sqrt((s0 + s1) + (s2 + s3)), s_j the squares of channels j, j+4, ... in order; no clamp: a zero
 *   descriptor gives NaN, as in the reference
 * NaN propagates as in torch (a NaN logit or coordinate gives NaN; clip there is not fmin / fmax). sqrt and division
 * are correctly rounded; exp and expm1 are the device library's.
 * D is written in 16-byte stores when F % 4 == 0 and D is 16-byte aligned, in scalar stores otherwise. The launch is
 * asynchronous on `stream`; B H W == 0 launches nothing. Everything is validated before the launch. M3S_EINVAL: a bad
 * layout, F outside 1..32, step < 1, a negative size, TOKENS with H or W not a multiple of 16, an array of 2^31
 * elements or more (B H W (4+F+tc)), vmax <= vmin or vmin not finite, a null or misaligned pointer with non-empty
 * work. */
#define M3S_HEAD_CAT 0
#define M3S_HEAD_TOKENS 1
int m3s_head_post(int layout, const float* a, const float* feat, int B, int H, int W, int F, int two_confs, int step,
                  double conf_vmin, double conf_vmax, double dconf_vmin, double dconf_vmax, float* X, float* C,
                  float* D, float* Q, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused operators (replace stretches of the reference's Python glue)
 * ------------------------------------------------------------------------------------------- */

/* create_frame -> resize_img: the frame ingest              mast3r_slam/frame.py:111-122,
 *                                                           mast3r_utils.py:245-289 (Pillow resize, centre crop,
 *                                                           ImgNorm) and the `/ 255` copy for uimg
 * From a decoded HWC image to the ViT's input, bit for bit what Pillow's 8-bit resampler and the float tail give.
 * Geometry (host doubles, S = max(W1, H1)): L = 512 for size 512, L = nearbyint(224 max(W1/H1, H1/W1)) for size 224;
 * resized (Wr, Hr) = nearbyint(W1 L / S), nearbyint(H1 L / S) (halves to even, as Python's round); filter LANCZOS
 * (support 3) when S > L, else BICUBIC (a = -0.5, support 2); crop with cx, cy = Wr / 2, Hr / 2 (integer): size 224:
 * half = min(cx, cy), box (cx-half, cy-half, cx+half, cy+half); size 512: halfw = ((2 cx) / 16) 8,
 * halfh = ((2 cy) / 16) 8, and halfh = 3 halfw / 4 when Wr == Hr and not square_ok. The transformation is
 * (W1/Wr, H1/Hr, (Wr-Wc)/2, (Hr-Hc)/2) with (Wc, Hc) the crop's size. An empty crop is M3S_EINVAL.
 * Coefficients per axis of length in -> out (host fp64): scale = in/out, fs = max(scale, 1), support = filter support
 * times fs; for output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
 * n = min(int(center + support + 0.5), in) - xmin, w[x] = filter((x + xmin - center + 0.5) / fs) (as a product with
 * 1 / fs), divided by their sum in index order when it is not 0, k[x] = int(w 2^22 -+ 0.5) truncated toward zero.
 * Passes: out = clamp((2^21 + sum k[x] pix[xmin + x]) >> 22, 0, 255) in int32, arithmetic shift; horizontal first into
 * a uint8 image, then vertical; an axis that keeps its length is copied, not filtered.
 * Tail per cropped byte u, fp32 with one rounding per operation: img[b, c, y, x] = ((float(u) / 255) - 0.5) / 0.5;
 * uimg[b, y/ds, x/ds, c] = float(u) / 255 for y % ds == 0 and x % ds == 0 ((B, ceil(Hc/ds), ceil(Wc/ds), 3));
 * rgb_u8[b, y, x, c] = u. Any of the three outputs may be NULL.
 * Source: (B, H1, W1, 3), pixels interleaved and contiguous in a row, rows row_stride bytes apart, images
 * H1 row_stride bytes apart; M3S_INGEST_U8 bytes (any alignment), or M3S_INGEST_F32 floats (4-byte aligned pointer and
 * row stride) which become bytes as numpy's uint8(x * 255) does on [0, 1]: one fp32 product, truncated, and clamped
 * to 0..255 outside that range (NaN gives 0).
 * m3s_ingest_geometry and m3s_ingest_table are host-only; the latter is the code that fills the device tables: xmin
 * and n of `out` entries, k of out x ksize entries (row xx at k + xx ksize, zero behind its n taps), ksize at least
 * 2 ceil(support) + 1. m3s_ingest_prepare builds and uploads the two tables of a geometry on the current device if
 * they are not cached (synchronous on first use: call it before capturing m3s_ingest into a graph);
 * m3s_ingest_release frees the current device's tables. m3s_ingest launches two kernels on `stream`: the horizontal
 * pass over the source rows and crop columns the output reads, into the workspace, and the vertical pass with the
 * tail. M3S_EINVAL: size not 512 or 224, H1 or W1 outside 1..16384, B outside 0..65535, downsample < 1, an empty crop,
 * a bad dtype, a null source or workspace with work to do, a misaligned float pointer or stride, img or uimg not
 * 4-byte aligned; M3S_ESPACE: short workspace. B == 0 launches nothing. */
#define M3S_INGEST_BICUBIC 0
#define M3S_INGEST_LANCZOS 1
#define M3S_INGEST_U8 0
#define M3S_INGEST_F32 1
typedef struct m3s_ingest_geom {
  int resized_w, resized_h;                   /* Wr, Hr */
  int filter;                                 /* M3S_INGEST_BICUBIC / M3S_INGEST_LANCZOS */
  int crop_x0, crop_y0, crop_x1, crop_y1;     /* the crop box in the resized image */
  int out_w, out_h;                           /* Wc, Hc */
  double scale_w, scale_h, half_crop_w, half_crop_h;
} m3s_ingest_geom;
typedef struct m3s_ingest_args {
  const void* src;    /* device */
  int src_dtype;      /* M3S_INGEST_U8 / M3S_INGEST_F32 */
  int64_t row_stride; /* bytes */
  int B, H1, W1;
  int size, square_ok, downsample;
  float* img;         /* (B, 3, Hc, Wc), nullable */
  float* uimg;        /* (B, ceil(Hc/ds), ceil(Wc/ds), 3), nullable */
  uint8_t* rgb_u8;    /* (B, Hc, Wc, 3), nullable */
} m3s_ingest_args;
int m3s_ingest_geometry(int H1, int W1, int size, int square_ok, m3s_ingest_geom* out /* host */);
int m3s_ingest_table(int in, int out, int filter, int32_t* xmin, int32_t* n, int32_t* k /* host arrays */, int ksize);
int m3s_ingest_prepare(int H1, int W1, int size, int square_ok, void* stream);
int m3s_ingest_release(void);
size_t m3s_ingest_workspace_size(int H1, int W1, int size, int square_ok, int B); /* 0 for a bad geometry */
int m3s_ingest(const m3s_ingest_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/* match(X11, X21, D11, D21, idx_init) -> (idx_1_to_2, valid_match2)     matching.py:8-90
 * X11, X21 (B,H,W,3) f32; D11, D21 (B,H,W,F) f32 (F % 8 == 0, F in {16,24,32}); idx_init (B,N) i64
 * or NULL (identity). idx_out (B,N) i64; valid_out (B,N) u8. Parameters = config `matching.*`. */
size_t m3s_match_workspace_size(int B, int H, int W, int F);
int m3s_match(const float* X11, const float* X21, const float* D11, const float* D21, const int64_t* idx_init,
              int64_t* idx_out, uint8_t* valid_out, int B, int H, int W, int F, int max_iter, float lambda_init,
              float cost_thresh, float dist_thresh, int radius, int dilation_max, void* workspace,
              size_t workspace_bytes, void* stream);

/* FrameTracker.track post-matching stretch (tracker.py:35-114): setup, Sim(3) GN to convergence
 * (rays: opt_pose_ray_dist_sim3 :173-214; calib: opt_pose_calib_sim3 :216-266), keyframe pointmap
 * fusion (frame.py:74-77) and the keyframe-selection statistics. */
#define M3S_TRACK_OK 1
#define M3S_TRACK_MAX_ITERS 2
#define M3S_TRACK_CHOLESKY_FAILED 3
#define M3S_TRACK_SKIPPED 4
/* The persistent GN launch's blocks did not all become resident within the bounded spin (e.g. the GPU
 * was shared with long-running persistent work): m3s_track then returns M3S_EHIP ("hand-off stalled")
 * instead of a result, never a silent relocalisation. */
#define M3S_TRACK_STALLED 5

typedef struct m3s_track_config {
  int mode;           /* 0 rays (use_calib False), 1 calib */
  int max_iters;      /* tracking.max_iters */
  float C_conf, Q_conf, min_match_frac;
  float sigma_a;      /* sigma_ray | sigma_pixel */
  float sigma_b;      /* sigma_dist | sigma_depth */
  float huber_k, rel_error, delta_norm;
  float pixel_border, depth_eps;
  float K[9];         /* calib intrinsics, row-major (host values) */
  int H, W;
} m3s_track_config;

typedef struct m3s_track_inputs {
  const int64_t* idx_f2k;      /* (N) */
  const uint8_t* valid_match;  /* (N) */
  const float* Xf;             /* (N,3) frame X_canon */
  const float* Cf;             /* (N)   frame C (sum) */
  float Nf;                    /* frame fusion count */
  const float* Qff;            /* (N) */
  const float* Xk;             /* (N,3) keyframe X_canon */
  const float* Ck;             /* (N)   keyframe C (sum) */
  float Nk;                    /* keyframe fusion count */
  const float* Qkf;            /* (N) */
  const float* T_WCf;          /* (8) device */
  const float* T_WCk;          /* (8) device */
  /* direct = 1: the opt_pose_* surface (tracker.py:173,216). idx_f2k is ignored (identity),
   * Qff holds Qk, valid_match holds valid_opt, Xf is already gathered (and constrained in calib
   * mode), meas_k (N,3) / valid_meas_k (N) are given; Cf, Ck, Qkf are unused. */
  int direct;
  const float* meas_k;
  const uint8_t* valid_meas_k;
} m3s_track_inputs;

typedef struct m3s_track_fuse_args {
  const float* Xk_canon; /* (N,3) keyframe X_canon; NULL = no fusion */
  const float* Ck_sum;   /* (N)   keyframe C */
  const float* Xkf;      /* (N,3) model output: keyframe points in the frame's camera */
  const float* Ckf;      /* (N) */
  float* Xk_out;         /* (N,3) fused X_canon (may alias Xk_canon: in place) */
  float* Ck_out;         /* (N)   fused C (may alias Ck_sum) */
  const float* Cf;       /* (N)   frame C (for Cf_avg_out; nullable) */
  float* Ck_avg_out;     /* (N)   fused C / Nk_new = keyframe.get_average_conf() (nullable) */
  float* Cf_avg_out;     /* (N)   Cf / Nf = frame.get_average_conf() (nullable) */
  float Nk_new, Nf;      /* keyframe N after this fusion, frame N (frame.py:83-84) */
  /* keyframe-store slot write-back (nullable; SharedKeyframes.__setitem__, frame.py:271-289, called at
   * tracker.py:101): with Xk_out / Ck_out pointing INTO the store's X[idx] / C[idx] rows, the fusion kernel also
   * stores the slot's fusion counters and dirty flag, on the device, when the frame tracked (the fusion's own
   * condition): slot_N = N_new, slot_N_updates = N_updates_new, slot_dirty = 1. Nothing else of the record changes
   * on a track (img, uimg, feat, pos, T_WC keep their values), so no full-record copy is needed. */
  int* slot_N;
  int* slot_N_updates;
  uint8_t* slot_dirty;
  int N_new, N_updates_new;
} m3s_track_fuse_args;

typedef struct m3s_track_result {
  float T_WCf[8];
  float T_CkCf[8];
  double cost;
  int iters, status, n_valid_opt, n_valid_kf, n_unique, N;
} m3s_track_result;

/* The track workspace's frame scratch (byte map, counters, tickets) persists across calls: each call's fusion launch
 * leaves it clean for the next frame, so only a fresh workspace is initialised. Call m3s_track_release(workspace)
 * before freeing or repurposing a workspace m3s_track used (a later workspace at the same address is then
 * initialised again); a workspace of another size at the same address is always initialised. */
size_t m3s_track_workspace_size(int N);
int m3s_track_release(const void* workspace);
int m3s_track(const m3s_track_inputs* in, const m3s_track_config* cfg, const m3s_track_fuse_args* fuse,
              int first_chunk /* ignored: one persistent launch runs every GN iteration */,
              float* T_out_dev /* (16) nullable: T_WCf | T_CkCf on device */,
              m3s_track_result* result /* host */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- retrieval codebook quantization ----
 * Replaces RetrievalDatabase.quantize_custom (mast3r_slam/retrieval_database.py:96-105):
 *   l2 = (|q|^2 + |c|^2) - 2 q c^T ; topk(l2, k, largest=False).indices, called from accumulate_scores (:119)
 *   and add_to_ivf_custom (:151-153) with the codebook `self.centroids` (:20-22).
 * m3s_codebook_prepare arranges the (C, D) fp32 centroids once (the reference moves them to the device once, in
 * __init__) into `codebook` (m3s_codebook_size bytes, device). m3s_quantize writes the (M, k) int64 indices of the
 * k nearest centroids of each of the M query rows (ascending distance; ties -> lower index), 1 <= k <= 8, k <= C.
 * Distances are computed with bf16 hi/lo split products on the matrix cores (fp32 accumulation): ~2^-16 relative
 * per product, tighter than the reference's TF32 GEMM (main.py:168). Everything is asynchronous on `stream`. */
size_t m3s_codebook_size(int C, int D);
int m3s_codebook_prepare(const float* centroids, int C, int D, void* codebook, size_t codebook_bytes, void* stream);
size_t m3s_quantize_workspace_size(int C, int D, int M, int k);
int m3s_quantize(const void* codebook, int C, int D, const float* qvecs, int M, int k, int64_t* topk_out,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- retrieval: the device-resident ASMK database (aggregate, score, top-k, append) ----
 * Replaces everything RetrievalDatabase.update does after prep_features (retrieval_database.py:43-72, 107-166) for the
 * configuration mast3r/retrieval/processor.py:91-96 fixes: binary kernel, use_idf False (other configurations are
 * rejected by the caller; nothing here falls back to the host).
 *   aggregate  asmk/kernel.py:26-39 + cython/hamming.pyx:24-30,79-109: for every unique word of the first `use_cols`
 *              columns of ids (M, k) int64, the fp32 sum over its rows (ascending, a row once) of
 *              fp32(des[row] - centroid[word]); bit = sum > 0, packed MSB-first (dim d -> word d / 32, bit 31 - d % 32).
 *              Codes are bit-exact with the reference. Words come out sorted; *count stays on the device.
 *   search     asmk/inverted_file.py:86-108, kernel.py:56-68, functional.py:11-15: for every query word and database
 *              entry of the same word h = popcount(q ^ e), sim = fp32(-2 fp32(h / D) + 1), kept if
 *              sim >= similarity_threshold, term = fp32(fp64(powf(sim, alpha)) / sqrt(fp64(norm[image]))), summed in
 *              fp64 per image and divided by sqrt(number of unique query words). norm[image] is the image's entry
 *              count. The sum's order is fixed (identical from run to run) but not the inverted file's.
 *   add        inverted_file.py:56-76, retrieval_database.py:138-166: append (code, word) under image id n_images.
 *   update     retrieval_database.py:43-72: quantise with k_query, aggregate, search, torch.topk(min(k, n_images)) with
 *              the `> min_thresh` filter (ties -> lower image index), then, with add_after_query, aggregate the first
 *              k_build columns again and append. On an empty database there is no query (count 0) and the add
 *              quantises with k_build (:149-154).
 * The database is a forward file in one device buffer: the (D + 1)-entry table of powf(sim, alpha), entries in
 * insertion order (codes (max_entries, D / 32) u32, words i32), img_ptr (max_images + 1) entry offsets, norm and the
 * fp64 scores of the last query. init fills the section pointers of the descriptor, uploads the table and empties the
 * database; n_images and entries_bound (an upper bound of the entries used: the host never reads a device count) are
 * host bookkeeping that add / update advance. M3S_ESPACE: the database cannot take another image of M * k_build
 * entries (nothing was launched; grow and repeat) or the workspace is short.
 * Limits: D % 32 == 0, M * k <= 4096, M <= 4096, C <= 2^20, 1 <= k_build <= k_query <= 8, k <= 64. Word ids must lie
 * in 0 .. C-1 (the quantiser's do). Everything is asynchronous on `stream`. */
#define M3S_ASMK_MAX_TOPK 64
typedef struct m3s_asmk_db {
  void* buf; /* device, m3s_asmk_db_size bytes */
  size_t bytes;
  int D, max_images;
  int64_t max_entries;
  int n_images;          /* host bookkeeping */
  int64_t entries_bound; /* host bookkeeping */
  /* sections of buf, set by init */
  float* table;
  uint32_t* codes;
  int32_t* words;
  int32_t* img_ptr;
  int32_t* norm;
  double* scores; /* (max_images): the last query's scores of images 0 .. n_images-1 */
} m3s_asmk_db;
typedef struct m3s_asmk_result { /* device; read back once by the caller */
  int32_t count;
  int32_t idx[M3S_ASMK_MAX_TOPK];
  double score[M3S_ASMK_MAX_TOPK];
} m3s_asmk_result;
size_t m3s_asmk_db_size(int D, int max_images, int64_t max_entries);
int m3s_asmk_db_init(m3s_asmk_db* db /* host; buf, bytes, D, max_images, max_entries set by the caller */, float alpha,
                     float similarity_threshold, void* stream);
size_t m3s_asmk_workspace_size(int C, int D, int M, int k);
/* codes (M * use_cols, D / 32) u32, words (M * use_cols) i32, count (1) i32: the first *count rows are valid */
int m3s_asmk_aggregate(const float* centroids, int C, int D, const float* features, int M, const int64_t* ids, int k,
                       int use_cols, uint32_t* codes, int32_t* words, int32_t* count, void* workspace,
                       size_t workspace_bytes, void* stream);
/* scores (n_images) f64; max_q: the rows the query arrays hold (<= 4096) */
int m3s_asmk_search(const m3s_asmk_db* db, const uint32_t* q_codes, const int32_t* q_words, const int32_t* q_count,
                    int max_q, double* scores, void* stream);
int m3s_asmk_add(m3s_asmk_db* db, const uint32_t* codes, const int32_t* words, const int32_t* count, int max_count,
                 void* stream);
int m3s_asmk_update(const void* codebook, const float* centroids, int C, m3s_asmk_db* db, const float* features, int M,
                    int k_query, int k_build, int k, double min_thresh, int add_after_query,
                    m3s_asmk_result* result /* device */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- map export: the confidence-filtered world point cloud of the keyframes ----
 * Replaces the per-keyframe host loop of evaluate.save_reconstruction (mast3r_slam/evaluate.py:47-70, called at
 * main.py:370-376; the viewer's live cloud, visualization.py:38,351, is the same filter): constrain_points_to_ray
 * (geometry.py:37-42) in calib mode, T_WC.act, get_average_conf() > c_conf_threshold, boolean indexing of points and
 * colours, np.concatenate. Rows come in the reference's order: keyframes in table order, pixels ascending.
 * Pixel n of keyframe k is kept iff C_k[n] * float32(1 / N_avg[k]) > c_conf_threshold (strict: NaN drops; the
 * keyframe table and its average are those of m3s_ba_keyframes). Its point is X_k[n], or with calib = 1 the point
 * (z x_of_u[u], z y_of_v[v], z) of its depth z = X_k[n].z on the ray of pixel u = n % width, v = n / width (the
 * tables of m3s_ba_calib_rays; bit-identical to constrain_points_to_ray; checks: N == height * width, both below
 * 65536), mapped to the world by Twc[k] in Sim3.act's fp32 operation order, one rounding per operation.
 * layout M3S_MAP_SOA: out (M,3) f32 and out_rgb (M,3) u8; M3S_MAP_PLY: out (M,15) bytes, the vertex records
 * (x, y, z little-endian f32, then r, g, b) of a binary little-endian PLY body (evaluate.save_ply, :88-106). */
#define M3S_MAP_SOA 0
#define M3S_MAP_PLY 1
typedef struct m3s_map_config {
  int calib;
  float fx, fy, cx, cy; /* calib: K[0,0], K[1,1], K[0,2], K[1,2] (host values) */
  int height, width;
  float c_conf_threshold;
  int layout;
} m3s_map_config;
size_t m3s_map_workspace_size(int Kp, int N);
/* Pass A + scan (evaluate.py:61-64, the mask): reads only C, stores 1 validity bit per point, the first output row of
 * every block of pixels and the counts in the workspace, whose header then records Kp, N, the threshold and the
 * total. Synchronises the stream. counts_out (host, Kp entries, nullable): rows per keyframe; total_out (host): M. */
int m3s_map_count(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, int Kp, int N, int64_t* counts_out,
                  int64_t* total_out, void* workspace, size_t workspace_bytes, void* stream);
/* Pass B (evaluate.py:54-60, 65-68): transform and compact the points that were valid AT THE COUNT (the stored bits;
 * C is not read again, so a keyframe that tracking fuses into between the two calls cannot move a row). Twc (Kp,8)
 * device. rgb: host array of Kp device pointers to (N,3) u8 colours, or NULL (geometry only: SOA out_rgb must then be
 * NULL, PLY colour bytes are 0). Rows at or beyond `capacity` are never written. The launch is asynchronous on
 * `stream`; before it the workspace header is read back (a 32-byte copy that waits for the stream's earlier work).
 * M3S_EINVAL: no count preceded the write on this workspace, Kp / N / threshold differ from that count's, capacity
 * below its total, a null table entry, a bad layout, a failed calib shape check; M3S_ESPACE: short workspace. */
int m3s_map_write(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, const float* Twc, const uint8_t* const* rgb,
                  int Kp, int N, void* out, uint8_t* out_rgb, int64_t capacity, void* workspace, size_t workspace_bytes,
                  void* stream);
/* Voxel-grid thinning, between m3s_map_count and m3s_map_write on the same workspace: of the counted rows, one per
 * occupied voxel stays in the stored mask. The world point y of a row is the write's (the same device code); with
 * r = float32(1) / float32(voxel_size) its voxel is q_c = floorf(y_c * r) per coordinate (one fp32 multiply, one floor).
 * A row whose y is not finite, or with a q_c outside [-2^20, 2^20), is dropped and counted. Per voxel the row with the
 * largest average confidence C_k[n] * float32(1 / N_avg[k]) survives, among equal confidences the smallest global
 * index g = k N + n (k the position in the keyframe table): its own point and colour, no centroid, so the result is
 * bit-reproducible. Survivors keep the export's order, so the thinned output is a subsequence of the unfiltered one;
 * m3s_map_write then runs unchanged (its header and capacity checks see the thinned total).
 * table: device memory of at least m3s_map_voxel_table_size(total of the count) bytes, 16-byte aligned; an
 * open-addressing hash table of 16-byte (key, best) slots, cleared here. m3s_map_voxel_table_size: 16 B times a power
 * of two of slots >= 2 total, at least 1024; 0 for a negative or overflowing total.
 * Uploads the keyframe pointer tables and the ray tables through the workspace, runs insert, thin and the count's scan,
 * and synchronises the stream. counts_out (host, Kp, nullable) / total_out (host): the thinned rows; dropped_out
 * (host, nullable): valid rows that reached no voxel (not finite, out of range, or a point that changed during the call).
 * M3S_EINVAL: voxel_size not finite or <= 0, a null table, Kp N >= 2^32, no count preceded on this workspace or its
 * Kp / N / threshold differ (the mask is then left as it was); M3S_ESPACE: short workspace, or table_bytes below the
 * size for the counted total. */
size_t m3s_map_voxel_table_size(int64_t total);
int m3s_map_voxel(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, const float* Twc, int Kp, int N,
                  float voxel_size, void* table, size_t table_bytes, int64_t* counts_out, int64_t* total_out,
                  int64_t* dropped_out, void* workspace, size_t workspace_bytes, void* stream);

/* Measured-peak probe (no reference counterpart; bench.py's roofline context):
 * blocks x 256 lanes x iters x 8 chains of v_fma_f32 (2 flops each) on `stream`. */
int m3s_peak_fma_f32(float* out_dev, int blocks, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_H */
