// LDS-tiled coarse-to-fine descriptor refine for MI355X (gfx950), F = 24, radius 3.
//
// Reference semantics: refine_matches_kernel<c10::Half>, mast3r_slam/backend/src/matching_kernels.cu:25-81 — per
// query pixel, dilation d = dmax..1, a 7x7 grid of stride d around the current centre (u outer, v inner), score =
// sequential c10::Half sum over 24 channels of half(q_k * c_k), strict '>' against a running max that starts at +0
// and is never reset, re-centre after each level.
//
// The kernel (refine_tile_kernel, at the end of the file): one 32x8 pixel tile per 256-lane block, four blocks per CU
// with 40 KiB of LDS each (they hide each other's fill latency), tiles dealt to XCDs in contiguous runs so each XCD's
// 4 MiB L2 holds its slab of D11. FUSE_PROJ instances first run the projection search for the tile's pixels
// (proj_prologue, m3s_proj.hpp): no launch and no p1 round trip between the LM search and the levels. Once per tile
// the block estimates the tile's flow (tile_flow); then the levels run as straight-line code, each specialised on d.
//
// One level (refine_level):
//   1. level_window: the bbox of the centres within 16 px of pixel + flow, +- 3d, is the level's cover; the window is
//      placed over it in one of four layouts of the block's 40 KiB (Layout, layout_rows / layout_cols):
//        GENERAL  40 x 64 cells of 16 B, one plane at a time    every level; three fills (f16 chunks), two (int8 planes)
//        PACKED   3 planes of 17 x 48                           f16 screen, d = 1: one fill, survivors rescored from LDS
//        DBUF     2 buffers of 26 x 48                          f16 screen, d = 2: chunk c + 1 streams in under chunk c
//        ONE8     30 x 56 cells of 16 B, then 30 x 56 of 8 B    int8 screen: both planes in one fill
//      a smaller layout is taken where the cover fits it. Fills are LDS DMA, one wave-instruction per window row, only
//      the cover's columns (fill_rows over a SrcPlane; fill_pairs8 for the int8 copy's 8 B cells).
//   2. level_outliers: a lane whose 49 candidates do not fit the window is scored in place by its wave, one outlier
//      at a time (wave_level: 49 lanes, 49 candidates from global memory, a first-maximum wave arg-max).
//   3. the lanes in the window, by instance and level:
//        exact_level     (!SCREEN)  all 49 candidates by the c10::Half chain from the window (score_chunk), the 49
//                        running half sums in registers across the three chunks; every read one ds_read_b128 with an
//                        immediate offset from a single per-lane base.
//        screened_level  (SCREEN: the fused path's instances) a cheap screen of the 49 candidates (screen_window ->
//                        screen_chunk), then screened_tail: threshold, mask (screen_mask), exact chains of the
//                        survivors (exact_survivors from L2, exact_survivors_lds in the PACKED window), re-centre.
//                        The screen is the int8 one (ScreenI8) at d >= RT_S8_DMIN = 2 when the frame has the int8 copy
//                        of D11 (24 B / px, written by prep_rays_kernel) and every component is within +-1, else the
//                        f16 one (ScreenF16): d = 1, M3S_REFINE_SCREEN8=0, and the frame fallback.
// Why the screened level returns the sequential scan's result bit for bit is written once, in front of ScreenF16; the
// int8 screen's part of it (the quantisation error, the integer threshold, the two fallbacks) in front of ScreenI8.
// Wave issue priorities follow the phase and the level (rt_prio below).
// Compiled with -ffp-contract=off and -fno-slp-vectorize: each candidate's half sum stays a scalar chain (VOP2
// v_add_f16 for the even channel, SDWA v_add_f16 for the odd one) instead of the SLP vectoriser pairing two
// candidates per v_pk_add_f16 behind v_perm / v_pack transposes. Measured issue costs on gfx950 at 4 waves/SIMD
// (scripts/micro/fma_rates, profiles/r03_valu_issue_rates.txt): VOP2 f16 add 1.18 ns, SDWA / VOP3P / v_perm
// 2.03-2.09 ns per wave-instruction, so 2.67 ns per channel-candidate against 3.1 ns paired: 125 -> 116 us.
#include "m3s_proj.hpp"
#include "m3s_match.h"

namespace m3s {

// Tile geometry: 32 x 8 pixel tiles, RT_WAVES waves per block, two pixel rows per wave
constexpr int RT_TW = 32, RT_TH = 8, RT_WAVES = 4, RT_THREADS = 64 * RT_WAVES;
constexpr int RT_MIN_BLOCKS = 16 / RT_WAVES;  // blocks per CU the register budget is sized for (16 waves: 128 VGPRs)
constexpr int RT_ROWS = 40, RT_COLS = 64;  // 40 x 64 x 16 B = 40 KiB per block: four blocks per CU (the LDS limit too)
// packed window (SCREEN, d = 1): all three chunk planes resident at once, 3 x 17 rows x 48 columns x 16 B = 38.25 KiB
// (the d = 1 cover is 16 x 39-40 on 97 % of the synthetic 512x512 tiles, scripts/refine_window_stats.py)
constexpr int RT_PROWS = 17, RT_PCOLS = 48, RT_PPLANE = RT_PROWS * RT_PCOLS;
// double-buffered window (SCREEN, d = 2): two 26-row x 48-column chunk buffers (2 x 19.5 KiB), chunk c + 1 streams in
// while chunk c is screened (the d = 2 cover is 23 x 45-47 on 97.6 % of the synthetic 512x512 tiles)
constexpr int RT_DROWS = 26, RT_DBUF = RT_DROWS * RT_PCOLS;
// int8 windows (SCREEN, d >= 2, the int8 screen_window): 24 B per cell as a 16-channel plane (16 B cells) and an 8-channel
// plane (8 B cells). The general 40 x 64 window holds one plane at a time (two fills); a cover within 30 x 56 holds
// both (30 x 56 x 24 B = 39.4 KiB, one fill): the d = 3 and d = 2 covers are 28 x 51 and 23 x 45 at the median
// (scripts/refine_window_stats.py)
constexpr int RT_8ROWS = 30, RT_8COLS = 56;
// the finest level that takes the int8 screen: 2 (its A/B against d >= 3 alone: profiles/refine_screen8_ab.json;
// -DRT_S8_DMIN=3 builds that variant). At d = 1 the int8 band would hold 5 more survivors per wave at the maximum
// (profiles/refine_screen8_census.txt): the packed f16 window stays.
#ifndef RT_S8_DMIN
#define RT_S8_DMIN 2
#endif
static_assert(RT_S8_DMIN >= 2, "d = 1 keeps the packed f16 window");
static_assert(RT_TH == 2 * RT_WAVES, "two pixel rows per wave");
static_assert(RT_8ROWS * RT_8COLS * 24 <= RT_ROWS * RT_COLS * 16, "the one-fill int8 window shares the block's window");
static_assert(RT_8COLS % 2 == 0 && RT_8COLS <= 64 && RT_COLS == 64, "8-byte cells are filled in pairs, two rows per DMA");
static_assert(3 * RT_PROWS * RT_PCOLS <= RT_ROWS * RT_COLS && 2 * RT_DROWS * RT_PCOLS <= RT_ROWS * RT_COLS,
              "the packed and double-buffered windows share the block's window");

typedef __attribute__((address_space(1))) const void* gvoid_t;
typedef __attribute__((address_space(3))) void* lvoid_t;

// Wave issue priority (s_setprio, user priority 0..3: the SIMD's arbiter takes the highest priority first, then the
// oldest wave). All 1024 blocks of a 512x512 launch are resident from the first microsecond, four per CU, so under
// oldest-first alone the blocks dispatched last lose every issue conflict and the launch ends on them (block 75 us at
// the median, launch 105 us). Two uses, both compile-time (DESIGN section 4 refine has the measurements):
//   * by phase: a block's chain alternates short issue phases that each start a long latency (the ~10 DMA rows of a
//     fill, a survivor trip's six loads, the LM gathers, the level-start exchange three other waves wait for) with long
//     dot2 bursts that start none. LM: the FUSE_PROJ instance's projection search and the D21 row loads behind it;
//     START: the level-start bbox reduction with its two barriers (and the window outliers' in-place levels); FILL: the
//     window fills through their vmcnt(0) and barrier arrival; SURV: the loads of an exact_survivors trip; SCORE:
//     screen_chunk / score_chunk, the mask and the exact chains.
//   * by level (LAG, "laggards first"): every value falls by one per level below d = 3, so a wave that is a level
//     behind the others on its SIMD outranks them in every phase and the blocks finish together.
// Doing both measured best: by level alone the same median with more spread, by phase alone a quarter of the gain
// (profiles/refine_prio_ab.json). The kernel has no spin-wait, so priorities change neither results nor liveness.
// Laggards first: 3 / 2 (latency phases / bursts) at d >= 3, 2 / 1 at d = 2, 1 / 0 at d = 1.
constexpr int RT_PRIO_LM = 3, RT_PRIO_START = 3, RT_PRIO_FILL = 3, RT_PRIO_SURV = 3, RT_PRIO_SCORE = 2,
              RT_PRIO_LAG = 1;
// the priority of phase value p at level d (d = 0: outside the levels)
constexpr int rt_prio_at(int p, int d) {
  const int q = (RT_PRIO_LAG && d > 0 && d < 3) ? p - (3 - d) : p;
  return q < 0 ? 0 : (q > 3 ? 3 : q);
}
template <int P, int D = 0>
__device__ __forceinline__ void rt_prio() {
  __builtin_amdgcn_s_setprio(rt_prio_at(P, D));
}
// ... where the wave is known to run at phase value FROM: nothing to do when the two are equal
template <int FROM, int P, int D>
__device__ __forceinline__ void rt_prio_from() {
  if constexpr (rt_prio_at(FROM, D) != rt_prio_at(P, D)) __builtin_amdgcn_s_setprio(rt_prio_at(P, D));
}

// Measurement builds. Each is a pair of helpers that compile to nothing without its macro.
// M3S_REFINE_STATS (the counts quoted in DESIGN section 4; m3s_debug_refine_stats reads them): per level d, window
// outlier lanes [2d] and waves [2d + 1]; survivors, the lanes' sum [32 + 2d] and the per-wave maximum summed [33 + 2d].
#ifdef M3S_REFINE_STATS
__device__ unsigned long long g_refine_stats[64];
#endif
template <int D>
__device__ __forceinline__ void stats_outliers(int lane, uint64_t om) {
#ifdef M3S_REFINE_STATS
  if (lane == 0 && om) {
    atomicAdd(&g_refine_stats[2 * D], (unsigned long long)__popcll(om));
    atomicAdd(&g_refine_stats[2 * D + 1], 1ull);
  }
#endif
}
template <int D>
__device__ __forceinline__ void stats_survivors(int lane, uint64_t m) {
#ifdef M3S_REFINE_STATS
  int mx = __popcll(m), sm = mx;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, __shfl_xor(mx, off, 64));
    sm += __shfl_xor(sm, off, 64);
  }
  if (lane == __ffsll((long long)__ballot(1)) - 1) {
    atomicAdd(&g_refine_stats[32 + 2 * D], (unsigned long long)sm);
    atomicAdd(&g_refine_stats[33 + 2 * D], (unsigned long long)mx);
  }
#endif
}
// M3S_REFINE_BSTAMPS (scripts/refine_blocks.py, scripts/refine_fuse_stamps.py): per block four words, [0] the levels'
// start (FUSE_PROJ: the kernel's first instruction), [1] the block's end, [2] its hardware id, [3] its active lanes
// (FUSE_PROJ: when the LM phase ended); s_memrealtime ticks.
#ifdef M3S_REFINE_BSTAMPS
__device__ unsigned long long g_refine_bstamps[8192 * 4];
#endif
__device__ __forceinline__ unsigned long long bstamp_clock() {
#ifdef M3S_REFINE_BSTAMPS
  return __builtin_amdgcn_s_memrealtime();
#else
  return 0ull;
#endif
}
__device__ __forceinline__ void bstamp_levels_start(bool fuse_proj, unsigned long long stamp_top) {
#ifdef M3S_REFINE_BSTAMPS
  if (threadIdx.x == 0 && blockIdx.x < 8192)
    g_refine_bstamps[blockIdx.x * 4 + 0] = fuse_proj ? stamp_top : __builtin_amdgcn_s_memrealtime();
#endif
}
__device__ __forceinline__ void bstamp_block_end(bool fuse_proj, unsigned long long stamp_lm, bool active,
                                                 uint4* lds) {
#ifdef M3S_REFINE_BSTAMPS
  const unsigned long long nact = __popcll(__ballot(active));
  // aliases the window (done with): a separate __shared__ array would push the block past 40 KiB of LDS and
  // change the occupancy being measured (4 -> 3 blocks per CU)
  unsigned long long* s_act = reinterpret_cast<unsigned long long*>(&lds[0]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_act[threadIdx.x >> 6] = nact;
  __syncthreads();
  if (threadIdx.x == 0 && blockIdx.x < 8192) {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    g_refine_bstamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime();
    g_refine_bstamps[blockIdx.x * 4 + 2] = hw;
    unsigned long long na = 0;
    for (int w = 0; w < RT_WAVES; w++) na += s_act[w];
    g_refine_bstamps[blockIdx.x * 4 + 3] = fuse_proj ? stamp_lm : na;
  }
#endif
}

// D11h layouts: PLANAR (fused path, written by prep_rays_kernel) = per image three chunk planes (H,W,8) f16, so a
// window row of one chunk is one contiguous 16 B-per-pixel run; otherwise the caller's (H,W,24) f16.
template <bool PLANAR>
__device__ __forceinline__ const h1* pix_ptr(const h1* img, size_t pix) {
  return img + pix * (PLANAR ? 8 : 24);
}
template <bool PLANAR>
__device__ __forceinline__ void load_chunks(const h1* p, size_t N, uint4& c0, uint4& c1, uint4& c2) {
  const size_t cs = PLANAR ? N * 8 : 8;  // chunk stride in halves
  c0 = *reinterpret_cast<const uint4*>(p);
  c1 = *reinterpret_cast<const uint4*>(p + cs);
  c2 = *reinterpret_cast<const uint4*>(p + 2 * cs);
}

// The exact score of one candidate: the c10::Half chain, from +0 sequentially over channels 0..23 (c0, c1, c2: the
// candidate's three 8-channel chunks)
__device__ __forceinline__ h1 exact_score(const h2* q, uint4 c0, uint4 c1, uint4 c2) {
  h1 sc = (h1)0.0f;
  add8(sc, &q[0], c0);
  add8(sc, &q[4], c1);
  add8(sc, &q[8], c2);
  return sc;
}
// ... and the scan's step for it: strict '>' against the running max
__device__ __forceinline__ void take_if_greater(h1 sc, int c, h1& max_score, int& bi) {
  if (sc > max_score) {
    max_score = sc;
    bi = c;
  }
}

// One level of one pixel by the whole wave (cu, cv, max_score, sq wave-uniform): lane c < 49 scores
// candidate (c / 7, c % 7) from global memory; the first candidate in scan order holding the wave
// maximum wins if it beats the running max — the sequential strict-'>' scan's result.
template <int D, bool PLANAR>
__device__ __forceinline__ void wave_level(const h1* __restrict__ img, int H, int W, const h2* sq, int& cu, int& cv,
                                           h1& max_score, int lane) {
  constexpr int R = 3, RD = R * D, G = 2 * R + 1;
  const int ci = lane / G, cj = lane % G;
  const int u = cu - RD + ci * D, v = cv - RD + cj * D;
  const bool ok = lane < G * G && u >= 0 && u < W && v >= 0 && v < H;
  uint4 c0, c1, c2;
  load_chunks<PLANAR>(pix_ptr<PLANAR>(img, (size_t)min(max(v, 0), H - 1) * W + min(max(u, 0), W - 1)),
                      (size_t)H * W, c0, c1, c2);
  const h1 sc = exact_score(sq, c0, c1, c2);
  const float sf = (ok && sc == sc) ? (float)sc : -INFINITY;  // NaN never wins a strict '>'
  float vmax = sf;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
  const int first = __ffsll((long long)__ballot(sf == vmax)) - 1;
  if (vmax > (float)max_score) {
    max_score = (h1)vmax;
    cu = cu - RD + (first / G) * D;
    cv = cv - RD + (first % G) * D;
  }
}

// 49 candidates x one 8-channel chunk from the LDS window; base = candidate (0,0) of this lane
template <int D>
__device__ __forceinline__ void score_chunk(const uint4* base, const h2* q4, h1* s) {
  constexpr int G = 7;
#pragma unroll
  for (int i = 0; i < G; i++) {
#pragma unroll
    for (int j = 0; j < G; j++) add8(s[i * G + j], q4, base[j * D * RT_COLS + i * D]);
    // bound the live candidate loads to one column (7 x 16 B) to keep the VGPR budget
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One window cell's part of a candidate's screen score (the screens and their proof: in front of screened_tail), the
// cell c against the query words q, accumulated into s. f16: an 8-channel chunk, four v_dot2c_f32_f16 of the same half
// operands as the exact chain; int8: the 16-channel plane A (uint4) or the 8-channel plane B (uint2), one
// v_dot4c_i32_i8 per word, exact in int32.
__device__ __forceinline__ float cell_dot(const h2* q4, const uint4& c, float s) {
  const h2* cv = reinterpret_cast<const h2*>(&c);
#pragma unroll
  for (int k = 0; k < 4; k++) s = __builtin_amdgcn_fdot2(q4[k], cv[k], s, false);
  return s;
}
template <class V>
__device__ __forceinline__ int cell_dot(const unsigned* q8, const V& c, int s) {
  const unsigned* cw = reinterpret_cast<const unsigned*>(&c);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(V) / 4); k++) s = __builtin_amdgcn_sdot4((int)q8[k], (int)cw[k], s, false);
  return s;
}

// 49 candidates x one chunk or plane of the screen from LDS (cell type V, accumulators A, cell_dot); base = candidate
// (0,0) of this lane in that plane, STRIDE cells a row.
// seed (the first chunk or plane, a constant at every call site): a[] is written, not accumulated into. The
// candidate's first product starts from +0 (0 + x: the same bits as accumulating into a zeroed register), so the 49
// accumulators are not live in front of it: zeroed ahead of the fill barrier they cost 98 moves per level (49 to zero
// them, 49 more where the screen's branch re-materialised them), now the one v_mov 0 the compiler puts in front of
// each candidate's first two-operand v_dot2c. (It selects v_dot2c for fdot2(q, c, 0) whatever the zero's source; the
// three-operand v_dot2_f32_f16 with an inline 0 would need inline asm and hand-kept dot -> VALU wait states.)
template <int D, int STRIDE = RT_COLS, class V, class Q, class A>
__device__ __forceinline__ void screen_chunk(const V* base, const Q* q, A* a, bool seed) {
  constexpr int G = 7;
#pragma unroll
  for (int i = 0; i < G; i++) {
    // the column's candidate reads in flight together (one LDS latency per column, not per candidate)
    V c[G];
#pragma unroll
    for (int j = 0; j < G; j++) c[j] = base[j * D * STRIDE + i * D];
#pragma unroll
    for (int j = 0; j < G; j++) a[i * G + j] = cell_dot(q, c[j], seed ? (A)0 : a[i * G + j]);
    // pin the column's dot products here: otherwise the last chunk's are sunk into the survivor code and all 49
    // candidate loads stay live across it (1000+ spilled VGPRs)
    A* ac = &a[i * G];
    asm volatile("" : "+v"(ac[0]), "+v"(ac[1]), "+v"(ac[2]), "+v"(ac[3]), "+v"(ac[4]), "+v"(ac[5]), "+v"(ac[6]));
    __builtin_amdgcn_sched_barrier(0);
  }
}

// bit c set where a[c] >= T (c < 49; a float NaN never), two VALU per candidate: the compare's lane mask (an SGPR pair)
// shifted into the mask word by an add-with-carry (m = m + m + carry), candidates in descending order so candidate c
// lands on bit c. The compiler's select / or / 64-bit shift form took about four per candidate. Each instruction is its
// own asm statement and the compares run two candidates ahead of the adds: gfx950 needs two wait states between a VALU
// write of an SGPR and a VALU read of it (the compiler pads v_cmp -> v_cndmask with s_nop 1), and the interleave
// provides them without nops; the compiler sees every operand, so it pads wherever the distance is short (the last two
// adds). A: float (the f16 screen's fp32 scores) or int (the int8 screen's): the compare's opcode is the difference.
template <class A>
__device__ __forceinline__ uint64_t screen_mask(const A* a, A T) {
  constexpr int C = 49;
  unsigned lo = 0u, hi = 0u;
  unsigned long long s[C];
#pragma unroll
  for (int k = 0; k < C + 2; k++) {
    if (k < C) {
      if constexpr (std::is_same<A, float>::value)
        asm volatile("v_cmp_ge_f32_e64 %0, %1, %2" : "=s"(s[k]) : "v"(a[C - 1 - k]), "v"(T));
      else
        asm volatile("v_cmp_ge_i32_e64 %0, %1, %2" : "=s"(s[k]) : "v"(a[C - 1 - k]), "v"(T));
    }
    if (k >= 2) {
      unsigned long long co;  // the carry-out (dead)
      if (C - 1 - (k - 2) >= 32)
        asm volatile("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(hi), "=s"(co) : "s"(s[k - 2]));
      else
        asm volatile("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(lo), "=s"(co) : "s"(s[k - 2]));
    }
  }
  return ((uint64_t)hi << 32) | lo;
}


// exact c10::Half chains of the survivor mask m in ascending scan order, read from D11h (L2); strict '>'. Two
// survivors per trip: both candidates' loads are in flight before the first chain (one L2 round trip per pair)
template <int D>
__device__ __forceinline__ void exact_survivors(const h1* __restrict__ img, int H, int W, const h2* q, int u_lo,
                                                int v_lo, uint64_t m, h1& max_score, int& bi) {
  while (__ballot(m != 0)) {  // wave-uniform trip count: the lane with the most survivors
    int c[2];
    uint4 x[2][3];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      c[k] = m != 0 ? __ffsll((long long)m) - 1 : -1;
      m &= m - 1;
    }
    rt_prio_from<RT_PRIO_SCORE, RT_PRIO_SURV, D>();  // the trip's loads start an L2 round trip
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (c[k] >= 0) {
        const int i = c[k] / 7, j = c[k] - 7 * i;
        load_chunks<true>(pix_ptr<true>(img, (size_t)(v_lo + j * D) * W + (u_lo + i * D)), (size_t)H * W, x[k][0],
                          x[k][1], x[k][2]);
      }
    }
    rt_prio_from<RT_PRIO_SURV, RT_PRIO_SCORE, D>();
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (c[k] >= 0) take_if_greater(exact_score(q, x[k][0], x[k][1], x[k][2]), c[k], max_score, bi);
  }
}

// LDS DMA of one window row (64 lanes x 16 B) by inline asm, for the double-buffered window: the compiler treats a
// global_load_lds as an LDS store of unknown extent and drains it (vmcnt(0)) before the next ds_read, which would
// serialise the fill of chunk c + 1 behind the screen of chunk c; the explicit vmcnt(0) + barrier order it instead.
// One wait state between the M0 write and the DMA (the compiler's own sequences keep one there too).
// lds_addr: the row's LDS byte address (wave-uniform)
__device__ __forceinline__ void lds_dma_row(const char* g, unsigned lds_addr) {
  const unsigned m0 = __builtin_amdgcn_readfirstlane(lds_addr);
  // M0 is an operand ({m0}): the compiler writes it itself right before the asm and knows its value (it also sets M0
  // for its own global_load_lds); the s_nop is the wait state between that M0 write and the DMA that reads it
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "{m0}"(m0) : "memory");
}

// the packed window's variant: the survivors' three chunks are read from the resident LDS planes (base = candidate
// (0,0) of this lane in plane 0), no L2 round trip; same ascending order, same strict '>'
template <int D>
__device__ __forceinline__ void exact_survivors_lds(const uint4* base, const h2* q, uint64_t m, h1& max_score,
                                                    int& bi) {
  while (m != 0) {
    const int c = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int i = c / 7, j = c - 7 * i;
    const uint4* p = base + j * D * RT_PCOLS + i * D;
    take_if_greater(exact_score(q, p[0], p[RT_PPLANE], p[2 * RT_PPLANE]), c, max_score, bi);
  }
}

// The int8 screen's state (set by screen_bound8; the derivation is in front of ScreenI8)
struct Int8Screen {
  const signed char* img = nullptr;  // this image's int8 planes: A (H,W,16) bytes, then B (H,W,8)
  bool on = false;   // block-uniform: the copy is there and every |c_h,k| <= 1 (the frame's partials finite)
  bool sok = false;  // this lane's int8 bound is usable (TileCtx::sok, and every |q_h,k| <= 1)
  float b = 0.0f;    // ... the bound B8 = B + E8
  unsigned q[6];     // ... and its query, four signed bytes per word, channels in order
};

struct TileCtx {
  const h1* img;
  int H, W, lane, wid, u_pix, v_pix;
  int fu, fv;   // tile flow estimate: mean initial centre displacement (fixed for all levels)
  int tcu, tcv; // tile centre + flow estimate: the window's centre when the centres' cover does not fit
  float bq = 0.0f;   // SCREEN: this lane's bound B (0.0125 |q| cmax + 2^-18)
  bool sok = false;  // SCREEN: the bound is usable (|q| cmax <= 16384 and finite)
  Int8Screen i8;     // SCREEN: the int8 screen of the levels d >= RT_S8_DMIN
};

// How a level lays its window out in the block's 40 KiB (the header comment has the table)
enum class Layout { GENERAL, PACKED, DBUF, ONE8 };
constexpr int layout_rows(Layout l) {
  return l == Layout::PACKED ? RT_PROWS : l == Layout::DBUF ? RT_DROWS : l == Layout::ONE8 ? RT_8ROWS : RT_ROWS;
}
constexpr int layout_cols(Layout l) {
  return l == Layout::PACKED || l == Layout::DBUF ? RT_PCOLS : l == Layout::ONE8 ? RT_8COLS : RT_COLS;
}

// One level's window over D11 (block-uniform) and this lane's column of it
struct LevelWin {
  int wx0, wy0;      // image coordinates of the window's corner
  int nrows, ncols;  // rows and columns actually filled
  Layout layout;
  bool col_in;       // this lane's column is filled
  int lane_off;      // ... and its offset in a row of a 16 B-per-pixel plane (D11h's: 48 B when not PLANAR), in bytes
};

// This lane's 7x7 candidate grid at one level
struct LaneGrid {
  int u_lo, v_lo;  // image coordinates of candidate (0, 0)
  int bx, by;      // ... and its window coordinates
  bool in;         // the lane is active and all 49 candidates lie in the filled window
};
// re-centre on the level's winner bi (scan index; -1: none beat the running max)
template <int D>
__device__ __forceinline__ void recentre(const LaneGrid& g, int bi, int& cu, int& cv) {
  if (bi >= 0) {
    cu = g.u_lo + (bi / 7) * D;
    cv = g.v_lo + (bi % 7) * D;
  }
}

// A plane of a level's source that holds 16 B of a pixel's channels, as a fill reads it: one of D11h's three
// 8-channel f16 chunks, or the int8 copy's 16-channel plane A
struct SrcPlane {
  const char* base;  // the image's row 0 in this plane (wave-uniform)
  size_t row_bytes;  // from one image row to the next
  int lane_bytes;    // this lane's window column in a row
};
template <bool PLANAR>
__device__ __forceinline__ SrcPlane chunk_plane(const TileCtx& t, const LevelWin& w, int chunk) {
  return {reinterpret_cast<const char*>(t.img + chunk * (PLANAR ? (size_t)t.H * t.W * 8 : 8)),
          (size_t)t.W * (PLANAR ? 16 : 48), w.lane_off};
}
__device__ __forceinline__ SrcPlane int8_plane_a(const TileCtx& t, const LevelWin& w) {
  return {reinterpret_cast<const char*>(t.i8.img), (size_t)t.W * 16, w.lane_off};
}

// Rows y0, y0 + RT_WAVES, .. < w.nrows of one source plane into LDS, dst + y * stride (uint4 units): one DMA (64 lanes
// x 16 B) per window row, only the cover's columns. The row base is wave-uniform (scalar), the column offset per
// lane. ASM_DMA: lds_dma_row instead of the builtin (the double-buffered window).
template <bool ASM_DMA>
__device__ __forceinline__ void fill_rows(const TileCtx& t, const LevelWin& w, const SrcPlane& p, uint4* dst,
                                          int stride, int y0) {
  for (int y = y0; y < w.nrows; y += RT_WAVES) {
    const int gy = min(max(w.wy0 + y, 0), t.H - 1);
    const char* rowp = p.base + (size_t)gy * p.row_bytes;
    if (w.col_in) {
      if constexpr (ASM_DMA)
        lds_dma_row(rowp + p.lane_bytes, (unsigned)(uintptr_t)(lvoid_t)&dst[y * stride]);
      else
        __builtin_amdgcn_global_load_lds((gvoid_t)(rowp + p.lane_bytes), (lvoid_t)&dst[y * stride], 16, 0, 0);
    }
  }
}

// The level's window: the bbox of the inlier centres, exchanged across the block's waves, and its placement
template <int D, bool SCREEN, bool PLANAR>
__device__ __forceinline__ LevelWin level_window(const TileCtx& t, bool active, int cu, int cv, int (*s_red)[4]) {
  constexpr int RD = 3 * D;
  const int lane = t.lane, wid = t.wid;
  // bbox of the inlier centres (within 16 px of pixel + the tile's flow estimate t.fu/t.fv)
  const bool inl = active && abs(cu - t.u_pix - t.fu) <= 16 && abs(cv - t.v_pix - t.fv) <= 16;
  // Both bounds as minima of signed 16-bit pairs, one packed instruction per step for two of them: lo = {mnu, mnv},
  // hi = {~mxu, ~mxv} (~x = -x - 1 reverses the order, and is one instruction for both fields). H, W < 32768
  // (m3s_refine_tile_ok), so a centre inside the image fits with room for the sentinel: a lane that is no inlier holds
  // 0x7fff in every field, neutral for the minimum, which reads back as mn = 32767 > mx = -32768 when no lane of the
  // block is one. The pack saturates (v_cvt_pk_i16_i32): a centre outside that range (a caller's p1 past the image)
  // gives a window that is not its cover, and the lane is then a window outlier like any other (refine_level's g.in
  // is tested in 32 bits against the window that was placed). Reduced by wave_reduce2 (DPP and permlane swaps, no
  // LDS round trip): lane 0 holds the wave's lo, lane 32 its hi.
  constexpr int NONE = 0x7fff7fff;
  const int pk = __builtin_bit_cast(int, __builtin_amdgcn_cvt_pk_i16(cu, cv));
  const int red = wave_reduce2(inl ? pk : NONE, inl ? ~pk : NONE, [](int a, int b) { return pk_min_i16(a, b); });
  __syncthreads();  // previous level's readers of s_red / lds are done
  if ((lane & 31) == 0) s_red[wid][lane >> 5] = red;
  __syncthreads();
  int lo = s_red[0][0], hi = s_red[0][1];
#pragma unroll
  for (int w = 1; w < RT_WAVES; w++) {
    lo = pk_min_i16(lo, s_red[w][0]);
    hi = pk_min_i16(hi, s_red[w][1]);
  }
  // unpacked here: the placement below is 32-bit arithmetic (mxu + 3d passes 32767 at W = 32767)
  hi = ~hi;
  int mnu = (int)(short)lo, mnv = lo >> 16, mxu = (int)(short)hi, mxv = hi >> 16;
  if (mnu > mxu) {  // no inlier: any window (every active lane is an outlier)
    mnu = mxu = 0;
    mnv = mxv = 0;
  }
  // window placement: exact bbox cover when it fits, else centred on the tile's centre displaced by its flow
  // estimate. A cover that does not fit is mostly a tight cluster plus a few far centres at one end: centring on the
  // bbox middle left the cluster itself outside (d = 4 on the synthetic 512x512 pair: 1502 outlier lanes against 54,
  // scripts/refine_window_stats.py)
  const int x_lo = mnu - RD, x_hi = mxu + RD, y_lo = mnv - RD, y_hi = mxv + RD;
  LevelWin w;
  // the level's smaller layout where the cover fits it, else the general window (block-uniform: every input is)
  const auto fits = [&](Layout l) { return x_hi - x_lo + 1 <= layout_cols(l) && y_hi - y_lo + 1 <= layout_rows(l); };
  w.layout = Layout::GENERAL;
  if constexpr (SCREEN) {
    if (D >= RT_S8_DMIN && t.i8.on)
      w.layout = fits(Layout::ONE8) ? Layout::ONE8 : Layout::GENERAL;
    else if (D == 1 && fits(Layout::PACKED))
      w.layout = Layout::PACKED;
    else if (D == 2 && fits(Layout::DBUF))
      w.layout = Layout::DBUF;
  }
  const int wc = layout_cols(w.layout), wr = layout_rows(w.layout);
  w.wx0 = (x_hi - x_lo + 1 <= wc) ? x_lo : t.tcu - wc / 2;
  w.wy0 = (y_hi - y_lo + 1 <= wr) ? y_lo : t.tcv - wr / 2;
  // rows and columns actually filled: the bbox cover, clipped to the window (a fine level's cover is ~40 of the 64
  // columns: the fill, bound by L2 -> LDS bandwidth, moves only those)
  w.nrows = min(wr, y_hi - w.wy0 + 1);
  w.ncols = min(wc, x_hi - w.wx0 + 1);
  w.col_in = lane < w.ncols;
  w.lane_off = min(max(w.wx0 + lane, 0), t.W - 1) * (PLANAR ? 16 : 48);
  return w;
}

// The wave's window outliers (outl: active lanes whose 49 candidates do not fit the window), scored in place: the
// wave takes them one at a time, one wave-level each, while the rest of the tile waits at the next barrier (a
// scattered warm start, every lane an outlier, costs its waves 64 pixels per level serially)
template <int D, bool PLANAR>
__device__ __forceinline__ void level_outliers(const TileCtx& t, bool outl, const h2* q, int& cu, int& cv,
                                               h1& max_score) {
  constexpr int F = 24;
  const int lane = t.lane;
  uint64_t m = __ballot(outl);
  stats_outliers<D>(lane, m);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    int scu = __shfl(cu, src, 64), scv = __shfl(cv, src, 64);
    const unsigned short mb0 = (unsigned short)__shfl((int)*reinterpret_cast<const unsigned short*>(&max_score),
                                                      src, 64);
    h1 smax = *reinterpret_cast<const h1*>(&mb0);
    h2 sq[F / 2];
#pragma unroll
    for (int k = 0; k < F / 2; k++) {
      const int v = __shfl(*reinterpret_cast<const int*>(&q[k]), src, 64);
      sq[k] = *reinterpret_cast<const h2*>(&v);
    }
    wave_level<D, PLANAR>(t.img, t.H, t.W, sq, scu, scv, smax, lane);
    if (lane == src) {
      cu = scu;
      cv = scv;
      max_score = smax;
    }
  }
}

// The general window, one 8-channel chunk at a time: fill, wait, barrier, then score(chunk) in the lanes whose grid
// lies in the window
template <int D, bool PLANAR, class Scorer>
__device__ __forceinline__ void general_window(const TileCtx& t, const LevelWin& w, uint4* lds, bool lane_in,
                                               Scorer score) {
#pragma unroll
  for (int chunk = 0; chunk < 3; chunk++) {
    if (chunk) {
      rt_prio_from<RT_PRIO_SCORE, RT_PRIO_FILL, D>();
      __syncthreads();  // previous chunk's readers are done
    }
    fill_rows<false>(t, w, chunk_plane<PLANAR>(t, w, chunk), lds, RT_COLS, t.wid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
    if (lane_in) score(chunk);
  }
}

// A lane's in-image candidates (bit c = i * 7 + j: candidate (i, j) of the grid at u_lo, v_lo), and whether any lane
// of the wave with its grid in the window has a candidate outside the image (wave-uniform)
template <int D>
__device__ __forceinline__ uint64_t in_image_mask(int u_lo, int v_lo, int H, int W) {
  constexpr int G = 7;
  uint64_t jm = 0, vm = 0;
#pragma unroll
  for (int j = 0; j < G; j++) jm |= (v_lo + j * D >= 0 && v_lo + j * D < H) ? (1ull << j) : 0ull;
#pragma unroll
  for (int i = 0; i < G; i++) vm |= (u_lo + i * D >= 0 && u_lo + i * D < W) ? (jm << (i * G)) : 0ull;
  return vm;
}
template <int D>
__device__ __forceinline__ bool wave_leaves_image(const LaneGrid& g, int H, int W) {
  return __ballot(g.in && !(g.u_lo >= 0 && g.u_lo + 6 * D < W && g.v_lo >= 0 && g.v_lo + 6 * D < H)) != 0;
}

// ---- the screened level (SCREEN) ----
// The level's 49 candidates are first scored by a cheap screen, then only candidates whose screen score lies within
// the rounding bound of the level's best are scored by the exact c10::Half chain, in scan order. Two screens share
// everything but the score: the f16 screen, an fp32 dot of the same half operands (v_dot2c_f32_f16: 12 per candidate
// instead of 24 half products + 24 half adds), and the int8 screen of the levels d >= RT_S8_DMIN (derived from this
// one in front of ScreenI8). The result is the sequential scan's, bit for bit:
//   * |S_half - S_real| <= 24 u P + 24 * 2^-25 for the c10::Half chain (u = 2^-11: 24 product roundings, 23 add
//     roundings, each <= u times a partial sum <= (1 + 0.013) P), where P = sum |q_k c_k| <= |q|_2 |c|_2, and
//     |S_dot2 - S_real| <= 12 (3 * 2^-24 P + 2^-36) (measured on gfx950, scripts/micro/dot2_exact.hip: at most
//     3 fp32 roundings of |a0 b0| + |a1 b1| + |acc| per instruction, 2^-36 absolute with subnormal halves);
//     so B = 0.0125 |q| cmax + 2^-18 bounds |S_half - S_dot2| (24 u = 0.01172), cmax = max |D11h[pixel]|_2
//     over the image (prep_rays_kernel).
//   * The winner w (first candidate in scan order with S_half[w] = M = max S_half, when M beats the running max)
//     has S_dot2[w] >= M - B >= Lmax - 2B, where Lmax = max over in-image candidates of S_dot2 (M >= S_half[c] >=
//     S_dot2[c] - B), and S_dot2[w] > max_score - B. A candidate failing either cannot win nor tie the winner,
//     so the scan over the survivors alone (ascending order, strict '>') returns the full scan's result.
//   * After the first level the centre candidate (3,3) is the last winner (its score IS the running max) or the
//     start pixel that did not beat +0: it never wins a strict '>' and is dropped from the survivors.
//   * |q| cmax > 16384 (overflow range) or non-finite: every in-image candidate survives (exact for all).
// A screen kind gives screened_tail the accumulator type with its "never wins" value, the lane's usable-bound flag, and
// the two terms of the threshold T = max(tms, tlm(Lmax)) in the accumulator's units.
struct ScreenF16 {
  typedef float acc_t;
  static __device__ __forceinline__ float never() { return -INFINITY; }
  static __device__ __forceinline__ bool usable(const TileCtx& t) { return t.sok; }
  static __device__ __forceinline__ float tms(const TileCtx& t, h1 max_score) { return (float)max_score - t.bq; }
  static __device__ __forceinline__ float tlm(const TileCtx& t, float lmax) { return lmax - 2.0f * t.bq; }
};

// the lane's bound B from its query's norm and the descriptor-norm bound cm (t.bq, t.sok)
__device__ __forceinline__ void screen_bound(TileCtx& t, const h2* q, float cm) {
  float qq = 0.0f;
#pragma unroll
  for (int k = 0; k < 12; k++) qq = __builtin_amdgcn_fdot2(q[k], q[k], qq, false);
  const float pq = sqrtf(qq) * cm * 1.001f;  // |q|_2 |c|_2 bound, rounded up
  t.sok = pq <= 16384.0f;                         // false for NaN / inf
  t.bq = t.sok ? 0.0125f * pq + 0x1p-18f : 0.0f;
}

// The int8 screen. The screen score is S8 = sum q8_k c8_k, exact in int32 (v_dot4c_i32_i8: 6 per candidate instead of
// 12 dot2), over q8 = clamp(rint(127 q_h)), c8 = clamp(rint(127 c_h)) (prep_rays_kernel's copy). With every
// |q_h,k| <= 1 and |c_h,k| <= 1 no clamp acts, so q_h = q8 / 127 + dq, c_h = c8 / 127 + dc with |dq|, |dc| <=
// 0.5 / 127, and
//   |sum q_h c_h - S8 / 127^2| = |sum dq c_h + (q8 / 127) dc| <= E8 = (0.5 / 127) (c1max + |q8|_1 / 127),
// c1max = max over the image of |c_h|_1 (prep's third partial). B8 = B + E8 bounds |S_half - S8 / 127^2|: B already
// covers |S_half - S_real|. The proof above carries over with S8 / 127^2 for S_dot2 and B8 for B: the winner w has
// S8[w] / 127^2 >= M - B8 >= Lmax - 2 B8 and > max_score - B8, so the survivors are the candidates with
// S8 >= 127^2 max(max_score - B8, Lmax - 2 B8). The comparison runs in integers against that threshold rounded down,
// less one for the fp32 arithmetic that forms it (|.| < 2^20: its error is far below 1): only ever more survivors.
// A lane with some |q_h,k| > 1 or not finite keeps every in-image candidate (!i8.sok); a frame with some |c_h,k| > 1
// or a non-finite partial takes the f16 screen at these levels (!i8.on, block-uniform).
constexpr float RT_K8 = 127.0f * 127.0f;
// floor to int32, saturating (a lane without a usable bound may hold anything here; its threshold is not used)
__device__ __forceinline__ int floor_i32(float x) { return (int)floorf(fminf(fmaxf(x, -2.0e9f), 2.0e9f)); }
struct ScreenI8 {
  typedef int acc_t;
  static __device__ __forceinline__ int never() { return INT_MIN; }
  static __device__ __forceinline__ bool usable(const TileCtx& t) { return t.i8.sok; }
  static __device__ __forceinline__ int tms(const TileCtx& t, h1 max_score) {
    return floor_i32(((float)max_score - t.i8.b) * RT_K8) - 1;
  }
  static __device__ __forceinline__ int tlm(const TileCtx& t, int lmax) {
    return floor_i32((float)lmax - 2.0f * t.i8.b * RT_K8) - 1;
  }
};

// the lane's int8 query and bound (after screen_bound); amax, c1max: the frame's max |c_h,k| and max |c_h|_1
__device__ __forceinline__ void screen_bound8(TileCtx& t, const h2* q, float amax, float c1max) {
  Int8Screen& s = t.i8;
  s.on = s.img != nullptr && amax <= 1.0f;  // false for NaN; a finite amax <= 1 makes c1max <= 24
  float qa = 0.0f;
  int qn1 = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) s.q[k] = 0u;
#pragma unroll
  for (int k = 0; k < 24; k++) {
    const float x = (k & 1) ? (float)q[k >> 1].y : (float)q[k >> 1].x;
    qa = fmaxf_nan(qa, fabsf(x));
    const int qi = (int)rintf(fminf(fmaxf(127.0f * x, -127.0f), 127.0f));
    qn1 += abs(qi);
    s.q[k >> 2] |= (unsigned)(qi & 0xff) << (8 * (k & 3));
  }
  s.sok = t.sok && qa <= 1.0f;
  // rounded up: c1max is a 24-term fp32 sum
  s.b = t.bq + (0.5f / 127.0f) * (c1max + (float)qn1 * (1.0f / 127.0f)) * 1.001f;
}

__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int max_of(int a, int b) { return max(a, b); }

// Everything of a screened level behind the screen, for the lanes whose grid lies in the window (a[]: their 49 screen
// scores): the in-image mask, the level's best, the threshold, the no-survivor skip, the mask word, the exact chains
// of the survivors and the re-centre. K: ScreenF16 or ScreenI8.
template <int D, class K>
__device__ __forceinline__ void screened_tail(const TileCtx& t, const LevelWin& w, const LaneGrid& g, const h2* q,
                                              typename K::acc_t* a, int& cu, int& cv, h1& max_score, const uint4* lds,
                                              bool first) {
  typedef typename K::acc_t A;
  constexpr int G = 7, CENTRE = G * G / 2;
  const int H = t.H, W = t.W;
  uint64_t vm = (1ull << (G * G)) - 1ull;  // in-image candidates
  if (wave_leaves_image<D>(g, H, W)) {
    vm = in_image_mask<D>(g.u_lo, g.v_lo, H, W);
    // out-of-image candidates scored clamped window pixels: they take no part in the level's best (nor survive)
#pragma unroll
    for (int c = 0; c < G * G; c++) a[c] = ((vm >> c) & 1ull) ? a[c] : K::never();
  }
  // the level's best over the candidates that can win: after the first level the centre is dropped from the
  // survivors (below), and it cannot raise T either: its exact score is the running max or a start pixel's <= +0,
  // so a[centre] - 2B <= max_score - B, the other term of T
  A lmax = a[0];
#pragma unroll
  for (int c = 1; c < G * G; c++)
    if (c != CENTRE) lmax = max_of(lmax, a[c]);
  lmax = max_of(lmax, first ? a[CENTRE] : K::never());
  // No lane of the wave can hold a survivor: the mask, the survivor loop and the re-centre are skipped as one
  // wave-uniform branch. A lane's mask is non-empty exactly when lmax >= max_score - B: lmax is one of its
  // candidates' a[c] and never below lmax - 2B, so it clears T = max(max_score - B, lmax - 2B) iff it clears the
  // first term, and no candidate clears a T that lmax does not (a NaN lmax fails both tests). A lane without a
  // usable bound (every candidate survives) keeps the wave out of the skip.
  const A tms = K::tms(t, max_score);
  if (__builtin_amdgcn_readfirstlane((int)(__ballot(!K::usable(t) || lmax >= tms) != 0ull)) == 0) return;
  const A T = max_of(tms, K::tlm(t, lmax));
  uint64_t m = screen_mask(a, T);
  if (!K::usable(t)) m = ~0ull;
  m &= vm;
  if (!first) m &= ~(1ull << CENTRE);
  stats_survivors<D>(t.lane, m);
  int bi = -1;
  if (D == 1 && w.layout == Layout::PACKED)  // the survivors' chunks are resident
    exact_survivors_lds<D>(&lds[g.by * RT_PCOLS + g.bx], q, m, max_score, bi);
  else
    exact_survivors<D>(t.img, H, W, q, g.u_lo, g.v_lo, m, max_score, bi);
  recentre<D>(g, bi, cu, cv);
}

// The f16 screen of one level: fill by layout, and the 49 screen scores a[] of the lanes whose grid lies in the window
template <int D>
__device__ __forceinline__ void screen_window(const TileCtx& t, const LevelWin& w, const LaneGrid& g, const h2* q,
                                              uint4* lds, float* a) {
  const int wid = t.wid;
  const int b0 = g.by * RT_PCOLS + g.bx;  // candidate (0, 0) in the 48-column layouts
  if (D == 1 && w.layout == Layout::PACKED) {  // the three chunk planes in one fill
    // row r = chunk * nrows + y of the 3 * nrows goes to wave r % RT_WAVES: an even deal whatever nrows is
    for (int chunk = 0; chunk < 3; chunk++)
      fill_rows<false>(t, w, chunk_plane<true>(t, w, chunk), &lds[chunk * RT_PPLANE], RT_PCOLS,
                       (wid - chunk * w.nrows) & (RT_WAVES - 1));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
    if (g.in) {
#pragma unroll
      for (int chunk = 0; chunk < 3; chunk++)
        screen_chunk<D, RT_PCOLS>(&lds[chunk * RT_PPLANE + b0], &q[chunk * 4], a, chunk == 0);
    }
  } else if (D == 2 && w.layout == Layout::DBUF) {  // chunk c + 1 lands in the other buffer while chunk c is screened
    fill_rows<true>(t, w, chunk_plane<true>(t, w, 0), lds, RT_PCOLS, wid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the same wait as a builtin: the compiler's wait model (blind to the asm) learns that none of its own loads
    // (a previous level's survivor loads, spill reloads) is still in flight, so it places no vmcnt(0) of its own
    // after the next fill, which would drain the DMA with them
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
    __syncthreads();
#pragma unroll
    for (int chunk = 0; chunk < 3; chunk++) {  // chunk is screened in buffer chunk & 1
      if (chunk < 2)
        fill_rows<true>(t, w, chunk_plane<true>(t, w, chunk + 1), &lds[((chunk + 1) & 1) * RT_DBUF], RT_PCOLS, wid);
      rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
      if (g.in) screen_chunk<D, RT_PCOLS>(&lds[(chunk & 1) * RT_DBUF + b0], &q[chunk * 4], a, chunk == 0);
      if (chunk < 2) {
        rt_prio_from<RT_PRIO_SCORE, RT_PRIO_FILL, D>();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // chunk + 1 landed; every wave is done with this chunk's buffer
      }
    }
  } else {
    general_window<D, true>(t, w, lds, g.in, [&](int chunk) {
      screen_chunk<D>(&lds[g.by * RT_COLS + g.bx], &q[chunk * 4], a, chunk == 0);
    });
  }
}

// Rows of the int8 copy's plane B (8 B cells) into LDS: row y at dst + y * STRIDE / 2 (uint4 units); a lane moves
// 16 B = two cells, STRIDE / 2 lanes a row, so one DMA (contiguous in LDS) takes two rows. A pair of cells that
// straddles the image's edge is read where it lies (one pixel before the row's start or behind its end: inside the
// copy, which has 16 B of slack at its end and plane A in front of plane B), so the cell inside the image holds its own
// pixel; a pair outside holds any. y0: this wave's first row (step 2 RT_WAVES rows)
template <int STRIDE>
__device__ __forceinline__ void fill_pairs8(const TileCtx& t, const LevelWin& w, uint4* dst, int y0) {
  constexpr int LPR = STRIDE / 2;  // lanes per row
  const int h = t.lane / LPR, l = t.lane - h * LPR;
  const int cc = min(max(w.wx0 + 2 * l, -1), t.W - 1);
  const bool on = h < 2 && 2 * l < w.ncols;
  const signed char* pB = t.i8.img + (size_t)t.H * t.W * 16;
  for (int y = y0; y < w.nrows; y += 2 * RT_WAVES) {
    const int gy = min(max(w.wy0 + y + h, 0), t.H - 1);
    const signed char* src = pB + ((ptrdiff_t)gy * t.W + cc) * 8;
    if (on && y + h < w.nrows) __builtin_amdgcn_global_load_lds((gvoid_t)src, (lvoid_t)&dst[y * LPR], 16, 0, 0);
  }
}

// The int8 screen of one level, likewise (a[]: int32 scores): plane A (16 channels) seeds a[], plane B adds the rest
template <int D>
__device__ __forceinline__ void screen_window(const TileCtx& t, const LevelWin& w, const LaneGrid& g, const h2*,
                                              uint4* lds, int* a) {
  const int wid = t.wid;
  const unsigned* q8 = t.i8.q;
  if (w.layout == Layout::ONE8) {  // both planes in one fill: plane A's 30 x 56 x 16 B, plane B behind it
    uint4* ldsB = &lds[RT_8ROWS * RT_8COLS];
    // plane A's rows wid, wid + 4, ..; plane B's row pairs dealt from the wave that follows A's last row
    fill_rows<false>(t, w, int8_plane_a(t, w), lds, RT_8COLS, wid);
    fill_pairs8<RT_8COLS>(t, w, ldsB, 2 * ((wid - w.nrows) & (RT_WAVES - 1)));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
    if (g.in) {
      const int b0 = g.by * RT_8COLS + g.bx;
      screen_chunk<D, RT_8COLS>(&lds[b0], &q8[0], a, true);
      screen_chunk<D, RT_8COLS>(reinterpret_cast<const uint2*>(ldsB) + b0, &q8[4], a, false);
    }
  } else {  // the general window, one plane at a time
    const int b0 = g.by * RT_COLS + g.bx;
    fill_rows<false>(t, w, int8_plane_a(t, w), lds, RT_COLS, wid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
    if (g.in) screen_chunk<D>(&lds[b0], &q8[0], a, true);
    rt_prio_from<RT_PRIO_SCORE, RT_PRIO_FILL, D>();
    __syncthreads();  // plane A's readers are done
    fill_pairs8<RT_COLS>(t, w, lds, 2 * wid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    rt_prio_from<RT_PRIO_FILL, RT_PRIO_SCORE, D>();
    if (g.in) screen_chunk<D>(reinterpret_cast<const uint2*>(lds) + b0, &q8[4], a, false);
  }
}

// The screened level: fill by layout and screen (screen_window of the kind's accumulator), then the tail
template <int D, class K>
__device__ __forceinline__ void screened_level(const TileCtx& t, const LevelWin& w, const LaneGrid& g, const h2* q,
                                               int& cu, int& cv, h1& max_score, uint4* lds, bool first) {
  typename K::acc_t a[49];  // written by the screen's first chunk or plane (seed): no zeroing
  __syncthreads();  // the reduction scratch aliases the window: its readers are done
  rt_prio_from<RT_PRIO_START, RT_PRIO_FILL, D>();
  screen_window<D>(t, w, g, q, lds, a);
  if (g.in) screened_tail<D, K>(t, w, g, q, a, cu, cv, max_score, lds, first);
}


// The exact scan's step over the 49 scores, in scan order (u outer, v inner), strict '>'. MASKED: only the candidates
// of vm take part
template <bool MASKED>
__device__ __forceinline__ void exact_scan(const h1* s, uint64_t vm, h1& max_score, int& bi) {
#pragma unroll
  for (int c = 0; c < 49; c++) {
    const bool gt = (!MASKED || ((vm >> c) & 1ull)) && s[c] > max_score;
    max_score = gt ? s[c] : max_score;
    bi = gt ? c : bi;
  }
}

// The exact level: all 49 candidates by the c10::Half chain, the running sums in registers across the three chunks
template <int D, bool PLANAR>
__device__ __forceinline__ void exact_level(const TileCtx& t, const LevelWin& w, const LaneGrid& g, const h2* q,
                                            int& cu, int& cv, h1& max_score, uint4* lds) {
  constexpr int G = 7;
  h1 s[G * G];
#pragma unroll
  for (int c = 0; c < G * G; c++) s[c] = (h1)0.0f;
  __syncthreads();  // the reduction scratch aliases the window: its readers are done
  rt_prio_from<RT_PRIO_START, RT_PRIO_FILL, D>();
  general_window<D, PLANAR>(t, w, lds, g.in, [&](int chunk) {
    score_chunk<D>(&lds[g.by * RT_COLS + g.bx], &q[chunk * 4], s);
  });
  if (g.in) {  // scan-order arg-max: u outer, v inner, strict '>' (matching_kernels.cu:54-71)
    int bi = -1;
    // every candidate grid of the wave lies inside the image (nearly every wave): index-only tracking, no mask test
    if (!wave_leaves_image<D>(g, t.H, t.W))
      exact_scan<false>(s, 0ull, max_score, bi);
    else
      exact_scan<true>(s, in_image_mask<D>(g.u_lo, g.v_lo, t.H, t.W), max_score, bi);
    recentre<D>(g, bi, cu, cv);
  }
}

// One level of the tile: window, outliers, then the screened or the exact scoring of the lanes in the window
template <int D, bool SCREEN, bool PLANAR>
__device__ __forceinline__ void refine_level(const TileCtx& t, bool active, const h2* q, int& cu, int& cv,
                                             h1& max_score, uint4* lds, int (*s_red)[4], bool first) {
  constexpr int RD = 3 * D;
  rt_prio<RT_PRIO_START, D>();  // three other waves wait at the exchange's barriers
  const LevelWin w = level_window<D, SCREEN, PLANAR>(t, active, cu, cv, s_red);
  LaneGrid g;
  g.u_lo = cu - RD;
  g.v_lo = cv - RD;
  g.bx = g.u_lo - w.wx0;
  g.by = g.v_lo - w.wy0;
  g.in = active && g.bx >= 0 && g.bx + 2 * RD < w.ncols && g.by >= 0 && g.by + 2 * RD < w.nrows;
  level_outliers<D, PLANAR>(t, active && !g.in, q, cu, cv, max_score);
  if constexpr (!SCREEN)
    exact_level<D, PLANAR>(t, w, g, q, cu, cv, max_score, lds);
  else if constexpr (D < RT_S8_DMIN)
    screened_level<D, ScreenF16>(t, w, g, q, cu, cv, max_score, lds, first);
  else if (t.i8.on)  // block-uniform
    screened_level<D, ScreenI8>(t, w, g, q, cu, cv, max_score, lds, first);
  else
    screened_level<D, ScreenF16>(t, w, g, q, cu, cv, max_score, lds, first);
}

template <bool P1_I64>
__device__ __forceinline__ void load_p1(const void* p1v, size_t bn, int& cu, int& cv) {
  if constexpr (P1_I64) {
    cu = (int)reinterpret_cast<const int64_t*>(p1v)[bn * 2];
    cv = (int)reinterpret_cast<const int64_t*>(p1v)[bn * 2 + 1];
  } else {
    cu = reinterpret_cast<const int*>(p1v)[bn * 2];
    cv = reinterpret_cast<const int*>(p1v)[bn * 2 + 1];
  }
}

template <bool LIN_OUT>
__device__ __forceinline__ void store_out(void* outv, size_t bn, int W, int cu, int cv) {
  if constexpr (LIN_OUT) {
    reinterpret_cast<int64_t*>(outv)[bn] = (int64_t)cu + (int64_t)W * cv;
  } else {
    reinterpret_cast<int64_t*>(outv)[bn * 2] = cu;
    reinterpret_cast<int64_t*>(outv)[bn * 2 + 1] = cv;
  }
}

// The projection search's arguments of the FUSE_PROJ instance (proj_occlusion_kernel's, matching.hip)
struct ProjArgs {
  const float* rays9;        // (B,H,W,9) prep_rays_kernel's ray image
  const float* X11;          // (B,H,W,3) raw points of image 1 (occlusion gather)
  const float* X21;          // (B,N,3) raw points of image 2
  const int64_t* idx_init;   // (B,N) warm start, nullable (identity)
  uint8_t* valid;            // (B,N) out
  const float* cnorm_part;   // SCREEN: prep's tile partials of the descriptor-norm bound
  int nparts, max_iter;
  float lambda_init, cost_thresh, dist_thresh;
};

// The FUSE_PROJ prologue: the lane projects its own pixel (centre -> cu, cv), writes valid and leaves the six loads
// of its raw D21 row (dv) in flight; SCREEN: wave 0 reduces prep's norm partials (cmax_w[0]; with the int8 copy also
// cmax_w[1], cmax_w[2]: max component, max 1-norm).
template <bool SCREEN>
__device__ __forceinline__ void proj_prologue(const TileCtx& t, const ProjArgs& pa, const void* D21, int b,
                                              bool active, size_t bn, int& cu, int& cv, float4* dv, float* cmax_w) {
  constexpr int F = 24;
  const int H = t.H, W = t.W, N = H * W;
  // the LM gathers and the D21 row loads behind them (until the first level's start sets its own)
  rt_prio_from<0, RT_PRIO_LM, 0>();
  // a lane past the image projects the nearest pixel inside it (every address stays in bounds, no branch join in
  // front of the loads) and writes nothing
  const int n = min(t.v_pix, H - 1) * W + min(t.u_pix, W - 1);
  const size_t bnc = (size_t)b * N + n;
  const float x = pa.X21[bnc * 3 + 0], y = pa.X21[bnc * 3 + 1], z = pa.X21[bnc * 3 + 2];
  const int64_t i0 = pa.idx_init != nullptr ? pa.idx_init[bnc] : (int64_t)n;
  if constexpr (SCREEN) {
    // reduce_cnorm's loads, in flight beside the pixel's own (4 KB from L2 at 512x512)
    // (with the int8 copy: the three runs norm, max component, max 1-norm)
    if (t.wid == 0) {
      if (t.i8.img != nullptr)
        reduce_cnorm_wave<3>(pa.cnorm_part, pa.nparts, cmax_w);
      else
        reduce_cnorm_wave<1>(pa.cnorm_part, pa.nparts, cmax_w);
    }
  }
  const float nrm = fmaxf(norm3_ref(x, y, z), 1e-12f);  // F.normalize (matching.py:44)
  const float p[3] = {x / nrm, y / nrm, z / nrm};
  float u, v;
  lin_to_pixel_f(i0, W, u, v);
  bool conv = false;
  float Xg[3];  // X11 at the final pixel, gathered during the last LM iteration
  iter_proj_point<true>(pa.rays9 + (size_t)b * N * 9, H, W, p, u, v, conv, pa.max_iter, pa.lambda_init,
                        pa.cost_thresh, pa.X11 + (size_t)b * N * 3, Xg);
  // The six loads of the D21 row are issued here, behind the LM loop (vmcnt retires in order: once they are issued,
  // the wave's next wait on an LM gather waits for them too); their latency runs under the tile-flow exchange. The
  // blocks leave the LM loop 16 to 31 us after the launch starts, which spreads the 1024 resident blocks' 25 MB by
  // itself. Measured (profiles/match_fuse_proj_ab.json, alternating bench runs on four boxes): the fastest and the
  // steadiest placement; staggered behind the LM iterations within 1 us of it with slow runs, at kernel start slowest.
  const float4* qsrc = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(D21) + bnc * F);
#pragma unroll
  for (int k = 0; k < F / 4; k++) dv[k] = qsrc[k];
  cu = (int)u;  // .long() truncation; u, v >= 1 after clamping
  cv = (int)v;
  // (every lane: a branch here would leave Xg's gather pending in the lanes past the image, and the next write of
  // its registers would drain the D21 loads with it)
  const float dx = Xg[0] - x, dy = Xg[1] - y, dz = Xg[2] - z;
  const float d = norm3_ref(dx, dy, dz);  // torch.linalg.norm (matching.py:71-73)
  const uint8_t vbyte = conv && (d < pa.dist_thresh);
  if (active) pa.valid[bn] = vbyte;
}

// Tile flow estimate, once per tile: the centres move by at most 3d per level, well inside the +-16 px inlier band, so
// the initial mean serves every level (saves a block reduction per level). Sets t.fu / t.fv and t.tcu / t.tcv.
// XCHG_CMAX: the same exchange hands wave 0's cmax_w[0..2] to every wave (cmax_b).
template <bool XCHG_CMAX>
__device__ __forceinline__ void tile_flow(TileCtx& t, bool active, int cu, int cv, int tx, int ty,
                                          const float* cmax_w, float* cmax_b, int (*s_red)[4]) {
  // the two displacement sums by wave_reduce2 (32-bit adds; lane 0 holds the wave's su, lane 32 its sv), the count
  // of active lanes from the ballot
  const int sum = wave_reduce2(active ? cu - t.u_pix : 0, active ? cv - t.v_pix : 0, [](int a, int b) { return a + b; });
  const int na = __popcll(__ballot(active));
  if ((t.lane & 31) == 0) s_red[t.wid][t.lane >> 5] = sum;
  if (t.lane == 0) {
    s_red[t.wid][2] = na;
    if constexpr (XCHG_CMAX) {
      if (t.wid == 0) {
#pragma unroll
        for (int r = 0; r < 3; r++) s_red[r][3] = __float_as_int(cmax_w[r]);
      }
    }
  }
  __syncthreads();
  if constexpr (XCHG_CMAX) {
#pragma unroll
    for (int r = 0; r < 3; r++) cmax_b[r] = __int_as_float(__builtin_amdgcn_readfirstlane(s_red[r][3]));
  }
  // block-uniform: SGPRs (readfirstlane), not VGPRs live across every level
  int tu = 0, tv = 0, tn = 0;
#pragma unroll
  for (int w = 0; w < RT_WAVES; w++) {
    tu += s_red[w][0];
    tv += s_red[w][1];
    tn += s_red[w][2];
  }
  const int nall = max(1, tn);
  t.fu = __builtin_amdgcn_readfirstlane(tu / nall);
  t.fv = __builtin_amdgcn_readfirstlane(tv / nall);
  t.tcu = tx * RT_TW + RT_TW / 2 + t.fu;
  t.tcv = ty * RT_TH + RT_TH / 2 + t.fv;
}

// P1_I64: p1 given as (B,N,2) int64 (reference op) else int32 (fused); LIN_OUT: write idx = u + W v.
// LIN_OUT (fused path) reads the PLANAR D11h of prep_rays_kernel.
// SCREEN (LIN_OUT instances only): bound-screened scoring (cmaxp = the descriptor-norm bound written by prep /
// proj_occlusion).
// FUSE_PROJ: the launch also runs the projection search (proj_occlusion_kernel's arithmetic in its order, from the
// shared m3s_proj.hpp, so the centres and valid are bit-identical): each lane projects its own pixel, keeps the
// centre in registers (no p1 traffic), writes valid and goes on into the levels; one wave per block reduces prep's
// norm partials itself (no launch sits between prep and this one; the max is order-independent, so every block gets
// the same bits).
template <bool D21_F32, bool P1_I64, bool LIN_OUT, bool SCREEN, bool FUSE_PROJ = false>
__global__ void __launch_bounds__(RT_THREADS, RT_MIN_BLOCKS)
    refine_tile_kernel(const h1* __restrict__ D11h, const void* __restrict__ D21, const void* __restrict__ p1v,
                       void* __restrict__ outv, int H, int W, int dilation_max, int tiles_x, int tiles_per_img,
                       int nblocks, const float* __restrict__ cmaxp, const signed char* __restrict__ D8,
                       const ProjArgs pa) {
  constexpr int F = 24;
  static_assert(!FUSE_PROJ || (D21_F32 && !P1_I64 && LIN_OUT), "the fused projection feeds the fused match path");
  static_assert(!SCREEN || LIN_OUT, "the screens read the fused path's PLANAR D11h (and its int8 copy)");
  const unsigned long long stamp_top = bstamp_clock();
  __shared__ uint4 lds[RT_ROWS * RT_COLS];
  int(*s_red)[4] = reinterpret_cast<int(*)[4]>(&lds[0]);  // level-start reductions alias the window
  const int lb = xcd_remap(blockIdx.x, nblocks);
  const int b = lb / tiles_per_img, tt = lb % tiles_per_img;
  const int tx = tt % tiles_x, ty = tt / tiles_x;
  TileCtx t;
  t.H = H;
  t.W = W;
  t.lane = threadIdx.x & 63;
  t.wid = threadIdx.x >> 6;
  {  // pixel of this lane: each ds_read_b128 lane group (16 lanes, one LDS cycle when conflict-free) takes 16
     // CONTIGUOUS pixels of one row, so lanes whose centres are displaced alike hit 16 distinct bank quads; the
     // row-major lane order put pixels 17 px apart into one group, which collide on a 1-px displacement change
    const int l = t.lane & 31;
    const int g = (l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28)) ? 0 : 1;
    const int r = g == 0 ? (l < 4 ? l : l < 16 ? l - 8 : l - 12) : (l < 12 ? l - 4 : l < 20 ? l - 8 : l - 16);
    t.u_pix = tx * RT_TW + g * 16 + r;
    t.v_pix = ty * RT_TH + 2 * t.wid + (t.lane >> 5);
  }
  const bool active = t.u_pix < W && t.v_pix < H;
  const int N = H * W;
  const size_t bn = (size_t)b * N + (size_t)t.v_pix * W + t.u_pix;
  t.img = D11h + (size_t)b * N * F;
  if constexpr (SCREEN) t.i8.img = D8 != nullptr ? D8 + (size_t)b * N * F : nullptr;
  h2 q[F / 2];
  int cu = 0, cv = 0;
  float4 dv[F / 4];   // FUSE_PROJ: the raw D21 row, converted where it is first needed
  // FUSE_PROJ && SCREEN: the descriptor-norm bound (and the int8 screen's two), held by wave 0 until the tile-flow
  // exchange
  float cmax_w[3] = {0.0f, 0.0f, 0.0f}, cmax_b[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (FUSE_PROJ) {
    proj_prologue<SCREEN>(t, pa, D21, b, active, bn, cu, cv, dv, cmax_w);
  } else if (active) {
    load_query<F, D21_F32>(D21, bn, q);
    load_p1<P1_I64>(p1v, bn, cu, cv);
  } else {
#pragma unroll
    for (int k = 0; k < F / 2; k++) q[k] = h2{(h1)0.0f, (h1)0.0f};
  }
  const unsigned long long stamp_lm = bstamp_clock();  // FUSE_PROJ: the LM phase's end
  // FUSE_PROJ && SCREEN: wave 0's cmax_w, for every wave
  tile_flow<FUSE_PROJ && SCREEN>(t, active, cu, cv, tx, ty, cmax_w, cmax_b, s_red);
  if constexpr (FUSE_PROJ) {
    // the D21 row, f32 -> f16 (RNE, == torch .half(): load_query's conversion) behind the tile-flow exchange: the
    // loads' latency runs under it
#pragma unroll
    for (int k = 0; k < F / 4; k++) {
      q[2 * k + 0] = h2{(h1)dv[k].x, (h1)dv[k].y};
      q[2 * k + 1] = h2{(h1)dv[k].z, (h1)dv[k].w};
    }
  }
  if constexpr (SCREEN) {
    screen_bound(t, q, FUSE_PROJ ? cmax_b[0] : cmaxp[0]);
    // (cmaxp holds three floats when the copy is there)
    if (t.i8.img != nullptr && dilation_max >= RT_S8_DMIN)
      screen_bound8(t, q, FUSE_PROJ ? cmax_b[1] : cmaxp[1], FUSE_PROJ ? cmax_b[2] : cmaxp[2]);
  }
  bstamp_levels_start(FUSE_PROJ, stamp_top);
  h1 max_score = (h1)0.0f;   // numeric_limits<c10::Half>::min() == +0, never reset between levels
  // the levels as straight-line code (d = dilation_max .. 1) instead of a loop over a switch of the eight inlined level
  // bodies: across that loop's back edge the register allocator made ~800 copies and spilled 19 VGPRs (80 B of scratch
  // per lane, ~18 MB of scratch writes per frame); straight-line, the screened kernel takes 118 VGPRs and spills none
  // (csrc/Makefile checks it: scripts/isa_check_spills.py)
#define RT_LEVEL(DD)                                                                                        \
  if (dilation_max >= DD)                                                                                   \
    refine_level<DD, SCREEN, LIN_OUT>(t, active, q, cu, cv, max_score, lds, s_red, dilation_max == DD);
  RT_LEVEL(8)
  RT_LEVEL(7)
  RT_LEVEL(6)
  RT_LEVEL(5)
  RT_LEVEL(4)
  RT_LEVEL(3)
  RT_LEVEL(2)
  RT_LEVEL(1)
#undef RT_LEVEL
  rt_prio<0>();
  if (active) store_out<LIN_OUT>(outv, bn, W, cu, cv);
  bstamp_block_end(FUSE_PROJ, stamp_lm, active, lds);
}

// One launch of a tile instance: one block per 32 x 8 tile of every image
template <bool D21_F32, bool P1_I64, bool LIN_OUT, bool SCREEN, bool FUSE_PROJ>
static void launch_tile(const void* D11h, const void* D21, const void* p1, void* out, int B, int H, int W,
                        int dilation_max, const float* cmax, const void* D8, const ProjArgs& pa, hipStream_t s) {
  const int tx = (W + RT_TW - 1) / RT_TW, ty = (H + RT_TH - 1) / RT_TH, nb = tx * ty * B;
  hipLaunchKernelGGL((refine_tile_kernel<D21_F32, P1_I64, LIN_OUT, SCREEN, FUSE_PROJ>), dim3(nb), dim3(RT_THREADS), 0,
                     s, reinterpret_cast<const h1*>(D11h), D21, p1, out, H, W, dilation_max, tx, tx * ty, nb, cmax,
                     reinterpret_cast<const signed char*>(D8), pa);
}

}  // namespace m3s

// shapes the tile kernel takes (else the per-pixel kernels of matching.hip); the fused path's prep writes the
// PLANAR D11h exactly when this holds
extern "C" int m3s_refine_tile_ok(int B, int H, int W, int F, int radius, int dilation_max) {
  if (F != 24 || radius != 3 || dilation_max < 1 || dilation_max > 8) return 0;
  if ((long long)B * H * W >= (1ll << 31) || H >= 32768 || W >= 32768) return 0;
  return 1;
}

// D21 f32 + p1 int32 -> idx (fused path) or D21 f16 + p1 int64 -> p1_new (reference op). Returns
// hipErrorNotSupported when the shape is not eligible (the caller falls back to the per-pixel kernels).
extern "C" hipError_t m3s_launch_refine_tile(const void* D11h, const void* D21, const void* p1, void* out, int B,
                                             int H, int W, int F, int radius, int dilation_max, int fused,
                                             const float* cmax, const void* D8, hipStream_t s) {
  if (!m3s_refine_tile_ok(B, H, W, F, radius, dilation_max)) return hipErrorNotSupported;
  const m3s::ProjArgs none{};
  if (fused && cmax != nullptr)
    m3s::launch_tile<true, false, true, true, false>(D11h, D21, p1, out, B, H, W, dilation_max, cmax, D8, none, s);
  else if (fused)
    m3s::launch_tile<true, false, true, false, false>(D11h, D21, p1, out, B, H, W, dilation_max, nullptr, nullptr, none,
                                                      s);
  else
    m3s::launch_tile<false, true, false, false, false>(D11h, D21, p1, out, B, H, W, dilation_max, nullptr, nullptr, none,
                                                       s);
  return hipGetLastError();
}

// The fused match path's tile launch with the projection search inside (refine_tile_kernel FUSE_PROJ): X21 /
// idx_init (nullable) -> valid and idx, no p1 buffer. cnorm_part (nullable: unscreened scoring):
// prep's nparts tile partials. hipErrorNotSupported when the shape is not eligible (the caller takes the
// proj_occlusion + refine launches).
extern "C" hipError_t m3s_launch_refine_tile_proj(const void* D11h, const float* D21, int64_t* idx_out, uint8_t* valid,
                                                  const float* rays9, const float* X11, const float* X21,
                                                  const int64_t* idx_init, int B, int H, int W, int F, int radius,
                                                  int dilation_max, int max_iter, float lambda_init, float cost_thresh,
                                                  float dist_thresh, const float* cnorm_part, int nparts,
                                                  const void* D8, hipStream_t s) {
  if (!m3s_refine_tile_ok(B, H, W, F, radius, dilation_max)) return hipErrorNotSupported;
  if ((size_t)9 * H * W >= ((size_t)1 << 31)) return hipErrorNotSupported;  // bilin_sample9's 32-bit offsets
  const m3s::ProjArgs pa{rays9, X11, X21, idx_init, valid, cnorm_part, nparts, max_iter, lambda_init, cost_thresh,
                         dist_thresh};
  if (cnorm_part != nullptr)
    m3s::launch_tile<true, false, true, true, true>(D11h, D21, nullptr, idx_out, B, H, W, dilation_max, nullptr, D8, pa,
                                                    s);
  else
    m3s::launch_tile<true, false, true, false, true>(D11h, D21, nullptr, idx_out, B, H, W, dilation_max, nullptr, nullptr,
                                                     pa, s);
  return hipGetLastError();
}

#ifdef M3S_REFINE_BSTAMPS
extern "C" int m3s_debug_refine_bstamps(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(m3s::g_refine_bstamps), sizeof(unsigned long long) * 8192 * 4) == hipSuccess
             ? 0 : -1;
}
#endif
#ifdef M3S_REFINE_STATS
extern "C" int m3s_debug_refine_stats(unsigned long long* out, int reset) {
  (void)hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(m3s::g_refine_stats), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[64] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(m3s::g_refine_stats), z, sizeof(z));
  }
  return 0;
}
#endif
