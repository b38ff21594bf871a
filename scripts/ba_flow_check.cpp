// Host check of the BA plan's host-built half (ba_pattern.cpp), a plain C++ program with no HIP:
//  * the dataflow schedule (ba_flow_schedule) against the device protocol of ba_sparse_factor_kernel's flow path
//    (ba_sparse.hip sp_flow_factor / sp_flow_back): interprets every wave's task list, decoded through BaFlowView, with
//    the kernel's wait conditions (update groups landed per column, source columns factored, x of struct(j) done) one
//    task at a time, and fails on a deadlock (no wave can proceed), on an update group applied out of step order, on a
//    factor task before all of its column's groups, or on a column left unfinished. Run for the `wide` given and for
//    the split each plan below chose;
//  * the plan (ba_build_plan) under the default options, the level-synchronous option and two forced wide splits:
//    every section of the packed image equals its source vector at its offset (the BA_SYM_SECTIONS list), the
//    LDS-staged range spans exactly the sections marked so, and every wide-step task record equals what the kernel's
//    sp_task_of_column / sp_task_of_group read from the tables (restated below): why the launched steps are
//    bit-identical to the in-kernel ones.
// Graph: a chain of K poses plus `loops` random earlier co-visibility edges per keyframe (both directions), or
// "i j" pairs from a file. build: g++ -O2 -I../lightweight-mast3r-slam_amd/csrc ba_flow_check.cpp
// ../lightweight-mast3r-slam_amd/csrc/ba_pattern.cpp -o /tmp/ba_flow_check
// usage: ba_flow_check K loops seed wide   |   ba_flow_check -f edges.txt wide
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ba_pattern.h"

static int fail(const char* m, int a = -1, int b = -1) {
  printf("FAIL %s (%d, %d)\n", m, a, b);
  return 1;
}

struct FlowStats {
  int nt = 0, busiest = 0, longest = 0, nowait = 0;
};

// the schedule S of pattern P with steps [0, wide) launched, interpreted with the kernel's wait conditions
static int check_schedule(const BaPattern& P, const std::vector<int>& S, int wide, FlowStats* st) {
  const int nb = P.nb, W = M3S_BA_SP_WAVES;
  const BaFlowView V{S.data(), W, nb};
  if (S.size() < BaFlowView::ints(W, nb, 0) || S.size() != BaFlowView::ints(W, nb, V.ntask()))
    return fail("schedule size");
  const int *wl_ptr = V.wl_ptr(), *bs_ptr = V.bs_ptr(), *fac_init = V.fac_init(), *wl = V.wl_task(),
            *bs_col = V.bs_col();
  const int nt = V.ntask();
  // level of each column; the expected group order per target = step order
  std::vector<int> lev(nb);
  for (int l = 0; l < P.nlev; l++)
    for (int c = P.lev_ptr[l]; c < P.lev_ptr[l + 1]; c++) lev[P.lev_col[c]] = l;
  int expect_tasks = 0;
  for (int l = wide; l <= P.nlev; l++) {
    expect_tasks += l < P.nlev ? P.lev_ptr[l + 1] - P.lev_ptr[l] : 0;
    expect_tasks += P.grp_ptr[l + 1] - P.grp_ptr[l];
  }
  if (nt != expect_tasks) return fail("task count", nt, expect_tasks);
  for (int j = 0; j < nb; j++)
    if (fac_init[j] != (lev[j] < wide ? 1 : 0)) return fail("fac_init", j);
  std::vector<int> app(nb, 0), fac(nb, 0), last_step(nb, -1), pos(W);
  for (int j = 0; j < nb; j++) fac[j] = fac_init[j] ? 1 : 0;  // the launched wide steps: done
  for (int w = 0; w < W; w++) pos[w] = wl_ptr[w];
  auto step_of_group = [&](int g) {
    int l = 0;
    while (!(P.grp_ptr[l] <= g && g < P.grp_ptr[l + 1])) l++;
    return l;
  };
  auto srcs_done = [&](int g) {
    if (g < 0) return true;
    for (int e = P.grp[4 * g + 1]; e < P.grp[4 * g + 2]; e++)
      if (!fac[P.src[4 * e + 1]]) return false;
    return true;
  };
  int done = 0;
  while (done < nt) {
    bool moved = false;
    for (int w = 0; w < W; w++) {
      if (pos[w] >= wl_ptr[w + 1]) continue;
      const int code = wl[2 * pos[w]], q = wl[2 * pos[w] + 1];
      if (code >= 0) {
        const int j = code, g = P.pull_grp[j];
        if (app[j] != q || !srcs_done(g)) continue;
        for (int t = P.grp_ptr[0]; t < P.grp_ptr[P.nlev + 1]; t++)  // every step group on j has landed
          if (P.grp[4 * t] == j && step_of_group(t) >= wide && last_step[j] < step_of_group(t))
            return fail("factor before its update groups", j, t);
        if (fac[j]) return fail("column factored twice", j);
        fac[j] = 1;
      } else {
        const int g = -1 - code, j = P.grp[4 * g];
        if (app[j] != q || !srcs_done(g)) continue;
        const int sg = step_of_group(g);
        if (sg <= last_step[j]) return fail("update groups out of step order", j, g);
        if (fac[j]) return fail("update after the target was factored", j, g);
        last_step[j] = sg;
        app[j]++;
      }
      pos[w]++;
      done++;
      moved = true;
    }
    if (!moved) return fail("factor deadlock", done, nt);
  }
  for (int j = 0; j < nb; j++)
    if (!fac[j]) return fail("column never factored", j);
  // back substitution
  std::vector<int> xd(nb, 0), seen(nb, 0);
  for (int w = 0; w < W; w++) pos[w] = bs_ptr[w];
  int bdone = 0;
  if (bs_ptr[W] != nb) return fail("back-substitution list size", bs_ptr[W], nb);
  while (bdone < nb) {
    bool moved = false;
    for (int w = 0; w < W; w++) {
      if (pos[w] >= bs_ptr[w + 1]) continue;
      const int j = bs_col[pos[w]] & BA_BS_COL;
      bool ok = true;
      for (int b = P.col_ptr[j] + 1; b < P.col_ptr[j + 1]; b++) ok = ok && xd[P.rowL[b]];
      if (bs_col[pos[w]] & BA_BS_NOWAIT) {
        if (!ok) return fail("no-wait column whose struct is not done", j);
      } else if (!ok) {
        continue;
      }
      if (seen[j]++) return fail("column solved twice", j);
      xd[j] = 1;
      pos[w]++;
      bdone++;
      moved = true;
    }
    if (!moved) return fail("back-substitution deadlock", bdone, nb);
  }
  st->nt = nt;
  for (int t = 0; t < nb; t++) st->nowait += (bs_col[t] & BA_BS_NOWAIT) ? 1 : 0;
  for (int w = 0; w < W; w++) {
    st->busiest = std::max(st->busiest, wl_ptr[w + 1] - wl_ptr[w]);
    st->longest = std::max(st->longest, bs_ptr[w + 1] - bs_ptr[w]);
  }
  return 0;
}

// ba_sparse.hip's SpTask and its two table readers, in host terms
struct Task {
  int j, b0, b1;
  bool has_g;
  int src0, src1;
  bool operator==(const Task& o) const {
    return j == o.j && b0 == o.b0 && b1 == o.b1 && has_g == o.has_g && src0 == o.src0 && src1 == o.src1;
  }
};
static Task task_of_column(const BaPattern& P, int j) {
  const int g = P.pull_grp[j];
  return Task{j, P.col_ptr[j], P.col_ptr[j + 1], g >= 0, g >= 0 ? P.grp[4 * g + 1] : 0, g >= 0 ? P.grp[4 * g + 2] : 0};
}
static Task task_of_group(const BaPattern& P, int g) {
  const int j = P.grp[4 * g];
  return Task{j, P.col_ptr[j], P.col_ptr[j + 1], true, P.grp[4 * g + 1], P.grp[4 * g + 2]};
}
static Task task_of_record(const BaStepRec& r) { return Task{r.j, r.b0, r.b1, r.g >= 0, r.src0, r.src1}; }

// one plan of the graph: its image against its sources, its task records against the tables, its own schedule
static int check_plan(const std::vector<int>& ri, const std::vector<int>& rj, int K, const BaPlanOptions& opt) {
  BaSymPlan Y;
  BaPlanSources Q;
  std::string err;
  if (!ba_build_plan(ri.data(), rj.data(), (int)ri.size(), K, opt, &Y, &err, &Q)) return fail(err.c_str());
  const BaPattern& S = Q.S;
  const std::vector<int>* secs[BA_SYM_NSEC] = {
#define SEC_SRC(name, src, lds, cap) &Q.src,
      BA_SYM_SECTIONS(SEC_SRC)
#undef SEC_SRC
  };
  const bool lds[BA_SYM_NSEC] = {
#define SEC_LDS(name, src, lds, cap) lds != 0,
      BA_SYM_SECTIONS(SEC_LDS)
#undef SEC_LDS
  };
  // the image: sections in list order, 16-B aligned, back to back, each equal to its source; padding zero
  size_t end = 0, lo = 0, hi = 0;
  bool in_lds = false, after_lds = false;
  for (int k = 0; k < BA_SYM_NSEC; k++) {
    const size_t bytes = sizeof(int) * secs[k]->size();
    if (Y.off[k] != end || Y.off[k] % 16) return fail("section offset", k);
    if (Y.off[k] + bytes > Y.image.size()) return fail("section past the image", k);
    if (bytes && memcmp(Y.image.data() + Y.off[k], secs[k]->data(), bytes)) return fail("section differs", k);
    end = (Y.off[k] + bytes + 15) & ~(size_t)15;
    for (size_t i = Y.off[k] + bytes; i < end; i++)
      if (Y.image[i]) return fail("padding not zero", k);
    if (lds[k] && after_lds) return fail("LDS-staged sections not contiguous", k);
    if (lds[k] && !in_lds) lo = Y.off[k];
    if (lds[k]) hi = Y.off[k] + bytes;
    after_lds = after_lds || (in_lds && !lds[k]);
    in_lds = lds[k];
  }
  if (end != Y.image.size()) return fail("image size");
  if ((size_t)Y.plan_lo_off != lo || (size_t)Y.plan_bytes != hi - lo) return fail("LDS-staged range");
  const size_t max_ints = ba_sym_capacity_ints(S.nb, (size_t)S.nb * (S.nb + 1) / 2, ri.size(), opt.max_pairs,
                                               M3S_BA_SP_WAVES);
  if (Y.image.size() > 4 * max_ints + 16 * BA_SYM_NSEC) return fail("image over its capacity bound");
  if (Y.nb != S.nb || Y.nlev != S.nlev || Y.nL != S.nL) return fail("plan sizes");
  if (Y.flow != (Q.sched.empty() ? 0 : 1) || (Y.flow && !opt.flow)) return fail("flow flag");
  if (Y.flow && m3s::ba_sp_lds_bytes(Y.plan_bytes, S.nb, true) > (size_t)m3s::SP_PLAN_BYTES)
    return fail("schedule kept past the LDS rule");
  // the wide steps' task records
  const int lmax = std::min(S.nlev + 1, BA_MAX_WIDE_STEPS);
  if (Y.wide_steps < 0 || Y.wide_steps > lmax) return fail("wide steps", Y.wide_steps, lmax);
  auto rec = [&](int i) {
    BaStepRec r;
    memcpy(&r, Y.image.data() + Y.off[BA_SEC_step_rec] + sizeof(r) * i, sizeof(r));
    return r;
  };
  int nrec = 0;
  for (int l = 0; l < lmax; l++) {
    const BaWideStep& w = Y.steps[l];
    const int c0 = l < S.nlev ? S.lev_ptr[l] : 0, na = l < S.nlev ? S.lev_ptr[l + 1] - c0 : 0;
    const int t0 = S.grp_ptr[l], nt = S.grp_ptr[l + 1] - t0;
    if (w.base != nrec || w.na != na || w.tasks != na + nt) return fail("wide step", l);
    for (int t = 0; t < na; t++)
      if (!(task_of_record(rec(nrec + t)) == task_of_column(S, S.lev_col[c0 + t]))) return fail("factor record", l, t);
    for (int t = 0; t < nt; t++)
      if (!(task_of_record(rec(nrec + na + t)) == task_of_group(S, t0 + t))) return fail("update record", l, t);
    nrec += na + nt;
  }
  if ((size_t)nrec * sizeof(BaStepRec) != sizeof(int) * Q.step_rec.size()) return fail("task record count", nrec);
  FlowStats st;
  return Y.flow ? check_schedule(S, Q.sched, Y.wide_steps, &st) : 0;
}

int main(int argc, char** argv) {
  std::vector<int> ri, rj;
  int K = 0, wide = 0;
  if (argc >= 3 && !strcmp(argv[1], "-f")) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return fail("cannot open edge file");
    int a, b;
    while (fscanf(f, "%d %d", &a, &b) == 2) {
      ri.push_back(a);
      rj.push_back(b);
      K = std::max(K, std::max(a, b) + 1);
    }
    fclose(f);
    wide = argc > 3 ? atoi(argv[3]) : 0;
  } else if (argc >= 5) {
    K = atoi(argv[1]);
    const int loops = atoi(argv[2]);
    std::mt19937 rng(atoi(argv[3]));
    wide = atoi(argv[4]);
    for (int k = 1; k < K; k++) {
      ri.push_back(k - 1), rj.push_back(k);
      ri.push_back(k), rj.push_back(k - 1);
      for (int l = 0; l < loops && k >= 3; l++) {
        const int o = (int)(rng() % (unsigned)(k - 1));
        ri.push_back(o), rj.push_back(k);
        ri.push_back(k), rj.push_back(o);
      }
    }
  } else {
    return fail("usage: ba_flow_check K loops seed wide | -f edges.txt wide");
  }
  // the plans: default, level-synchronous, everything launched, nothing launched
  BaPlanOptions opts[4];
  opts[1].flow = false;
  opts[2].wide_by_thr = opts[3].wide_by_thr = true;
  opts[2].wide_thr = 0;
  opts[3].wide_thr = 1000000;
  for (const BaPlanOptions& o : opts)
    if (int rc = check_plan(ri, rj, K, o)) return rc;
  BaPattern P;
  ba_build_pattern(ri.data(), rj.data(), (int)ri.size(), K, &P);
  wide = std::min(wide, P.nlev + 1);
  if (P.nb == 0) {
    printf("OK empty\n");
    return 0;
  }
  std::vector<int> S;
  ba_flow_schedule(P, wide, M3S_BA_SP_WAVES, &S);
  FlowStats st;
  if (int rc = check_schedule(P, S, wide, &st)) return rc;
  printf("OK K %d E %d nlev %d wide %d tasks %d (max %d per wave) back columns %d (max %d per wave, %d without a "
         "wait)\n",
         K, (int)ri.size(), P.nlev, wide, st.nt, st.busiest, P.nb, st.longest, st.nowait);
  return 0;
}
