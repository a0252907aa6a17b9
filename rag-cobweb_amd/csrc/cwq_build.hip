// libcwq index construction (host side): the filter operands and bound constants (build_filter), the
// group cut and its pruning tables (plan_groups, build_prune), cwq_index_create / _create_cv /
// index_create_device and cwq_index_destroy.  Kernels: cwq_kernels.hip, cwq_mfma.hip, cwq_group.hip,
// cwq_prune.hip.
//
// Index layout in HBM:
//   internal nodes (nodes with children), BFS order:     A = 1/sigma, B = mu/sigma  [DP][ld_int]
//   leaf-class rows (childless nodes + internal nodes that hold sentences),
//     isotropic rows first (var identical across d):    M = mu                      [DP][ld_iso]
//     then anisotropic rows:                            A = 1/sigma, B = mu/sigma   [DP][ld_an]
//   dim-major ("transposed") so a wave's 64 lanes = 64 consecutive rows read one
//   coalesced 256-B line per dimension.
#include "cwq_handle.h"

namespace {
float round_up_f(double v) {
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, INFINITY);
  return f;
}

// bf16 operands, fp32 rerank copy, per-row and per-tile bound constants, and the
// strided threshold sample of the isotropic rows.
// Group-centred rows and the pruning cut (cwq_group.hip, cwq_prune.hip).
// A cut is a set of internal nodes, the group centres, such that every internal node lies in
// exactly one centre's subtree (its group) or is an ancestor of centres (a top node; the root
// is always one).  A group's rows -- the isotropic rows whose parent is in the group -- are
// centred at the centre's mean when every one of them is at most twice as far from it as
// from the root mean (then the rounding terms stay within the bound's eps and beta margins)
// and all rows of each of its parents share the key coefficients (the group term is folded
// into the parent's prefix): the group is "ok".  The rows of the other groups, and the rows
// whose parent is a top node, stay root-centred; every group is still a pruning group.
//
// The cut is tree-adaptive: a DP over the internal tree (children before parents) minimises
// the rows' summed squared norms as stored -- an ok group's rows at their centre, the rest at
// the root -- plus a penalty lam per group and per top node:
//   best(c) = min( centre at c:  cost(c) + lam,
//                  split c:      (rows directly below c, at the root) + sum best(internal child) + lam )
// A broad root child spanning many clusters (a 500k x 768 ifit tree: 37 root children over
// 500 clusters) is split down to its cluster-level nodes; a tight one stays one group (in
// high dimension splitting a Gaussian cluster saves ~1/D of its norms, far below lam).
// Centres are at depth <= 8 (CWQ_GROUP_MAXDEP); lam = the mean squared root norm of a row
// (CWQ_GROUP_LAMBDA scales it), doubled while the cut has more than kCutMaxGroups groups or
// kCutMaxTop top nodes.  CWQ_GROUP_CUT=1 keeps the round-4 cut (every depth-1 node a centre).  The
// mode is on when the centred rows cut the summed squared norms at least 4x
// (CWQ_GROUP_CENTRE=0 / 1: off / on whenever they shrink).  rgrp[r] = the group a row is
// centred at, or -1.
constexpr int kCutMaxGroups = 4096, kCutMaxTop = kPruneMaxTop;
int plan_groups(cwq_index* ix, const float* mean, const int64_t* d_rows, const std::vector<RowMeta>& meta,
                const std::vector<int>& row_par, const std::vector<int64_t>& int_nodes, const std::vector<int>& par_int,
                std::vector<int>& rgrp, hipStream_t s) {
  int rc;
  const int NLi = ix->NL_iso, NI = ix->NI, D = ix->D;
  rgrp.assign(NLi, -1);
  const int force = env_int("CWQ_GROUP_CENTRE", -1);
  if (force == 0 || NI < 2 || NLi == 0) return CWQ_OK;
  std::vector<int> idep(NI, 0);
  int maxdep_all = 0;
  for (int i = 1; i < NI; ++i) {
    idep[i] = idep[par_int[i]] + 1;   // BFS internal ids: the parent first
    maxdep_all = std::max(maxdep_all, idep[i]);
  }
  const bool depth1 = env_int("CWQ_GROUP_CUT", 0) == 1;
  const char* em = getenv("CWQ_GROUP_MAXDEP");
  const int maxd = depth1 ? 1 : std::max(1, std::min(maxdep_all, em && *em && atoi(em) > 0 ? atoi(em) : 8));
  const int W = maxd + 1;
  // per row: the squared norm centred at the root ([0]) and at each ancestor of depth 1..maxd
  int *d_rpar = nullptr, *d_pint = nullptr, *d_idep = nullptr;
  int64_t* d_inodes = nullptr;
  double* d_dist = nullptr;
  if ((rc = ix->upload(&d_rpar, row_par, s)) || (rc = ix->upload(&d_pint, par_int, s)) ||
      (rc = ix->upload(&d_idep, idep, s)) || (rc = ix->upload(&d_inodes, int_nodes, s)) ||
      (rc = ix->alloc(&d_dist, (size_t)NLi * W)))
    return rc;
  HIPCHK(launch_group_anc_dist(mean, D, d_rows, NLi, ix->iso_c, d_rpar, d_pint, d_idep, d_inodes, maxd, d_dist, s));
  std::vector<double> dist((size_t)NLi * W);
  HIPCHK(hipMemcpyAsync(dist.data(), d_dist, dist.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // per internal node: the rows below it -- their squared norms centred at its mean (depth <=
  // maxd) and at the root, their count, and whether they qualify for centring at it; the
  // rows directly below it at the root
  std::vector<double> cost(NI, 0.0), rsub(NI, 0.0), rdir(NI, 0.0);
  std::vector<int64_t> nrow(NI, 0);
  std::vector<char> ok(NI, 1);
  std::vector<float> pcw(NI, NAN), piv(NI, NAN), pinvL(NI, NAN);
  std::vector<char> pbad(NI, 0);
  double sum_root = 0.0;
  for (int r = 0; r < NLi; ++r) {
    const double r0 = dist[(size_t)r * W];
    sum_root += r0;
    const int p = row_par[r];
    if (p < 0) continue;
    rdir[p] += r0;
    if (std::isnan(pcw[p])) {
      pcw[p] = meta[r].cw;
      piv[p] = meta[r].iv;
      pinvL[p] = meta[r].invL;
    } else if (pcw[p] != meta[r].cw || piv[p] != meta[r].iv || pinvL[p] != meta[r].invL) {
      pbad[p] = 1;
    }
    for (int a = p; a > 0; a = par_int[a]) {
      rsub[a] += r0;
      nrow[a]++;
      if (idep[a] <= maxd) {
        const double v = dist[(size_t)r * W + idep[a]];
        cost[a] += v;
        if (!(v <= 4.0 * r0)) ok[a] = 0;   // |M_g| <= 2 |M_0|: the rounding cross term stays in eps
      }
    }
  }
  for (int p = 1; p < NI; ++p)
    if (pbad[p])
      for (int a = p; a > 0; a = par_int[a]) ok[a] = 0;
  std::vector<int> kptr(NI + 1, 0), kids(NI > 0 ? NI - 1 : 0);
  for (int i = 1; i < NI; ++i) kptr[par_int[i] + 1]++;
  for (int i = 0; i < NI; ++i) kptr[i + 1] += kptr[i];
  {
    std::vector<int> fill(kptr.begin(), kptr.end() - 1);
    for (int i = 1; i < NI; ++i) kids[fill[par_int[i]]++] = i;
  }
  const char* el = getenv("CWQ_GROUP_LAMBDA");
  double lam = (el && *el ? atof(el) : 1.0) * sum_root / NLi;
  std::vector<double> best(NI);
  std::vector<char> centre(NI, 0);
  std::vector<int> gint(NI, -1);
  std::vector<int64_t> gnode;
  std::vector<int> gcent;
  int ntop = 0;
  for (int it = 0; it < 64; ++it, lam = lam > 0.0 ? 2.0 * lam : 1.0) {
    for (int c = NI - 1; c >= 1; --c) {
      double cc = INFINITY, sp = INFINITY;
      cc = (ok[c] ? cost[c] : rsub[c]) + lam;
      if (idep[c] < maxd && kptr[c + 1] > kptr[c]) {
        sp = rdir[c] + lam;
        for (int j = kptr[c]; j < kptr[c + 1]; ++j) sp += best[kids[j]];
      }
      centre[c] = cc <= sp ? 1 : 0;
      best[c] = std::min(cc, sp);
    }
    // top-down: group ids in BFS order of the centres
    gnode.clear();
    gcent.clear();
    ntop = 1;
    for (int i = 1; i < NI; ++i) {
      const int p = par_int[i];
      if (gint[p] >= 0) {   // inside p's group
        gint[i] = gint[p];
      } else if (centre[i]) {   // p is a top node (the root, or split): i a centre ...
        gint[i] = (int)gnode.size();
        gnode.push_back(int_nodes[i]);
        gcent.push_back(i);
      } else {   // ... or a top node itself
        gint[i] = -1;
        ++ntop;
      }
    }
    if ((int)gnode.size() <= kCutMaxGroups && ntop <= kCutMaxTop) break;
  }
  const int G = (int)gnode.size();
  if (G == 0 || G > kCutMaxGroups || ntop > kCutMaxTop) return CWQ_OK;
  std::vector<char> gok(G, 0);
  for (int g = 0; g < G; ++g) gok[g] = ok[gcent[g]];
  std::vector<int> cand(NLi, -1);
  double sum_sel = 0.0;
  for (int r = 0; r < NLi; ++r) {
    cand[r] = row_par[r] >= 0 ? gint[row_par[r]] : -1;
    const int g = cand[r];
    sum_sel += (g >= 0 && gok[g]) ? dist[(size_t)r * W + idep[gcent[g]]] : dist[(size_t)r * W];
  }
  ix->cut_gint = gint;
  ix->cut_centre = gcent;
  ix->cut_ok = gok;
  ix->cut_top = ntop;
  ix->cut_maxdep = 0;
  for (int c : gcent) ix->cut_maxdep = std::max(ix->cut_maxdep, idep[c]);
  const bool on = force == 1 ? sum_sel < sum_root : sum_sel * 4.0 <= sum_root;
  if (!on) return CWQ_OK;
  int64_t* d_gnode = nullptr;
  float* cent = nullptr;
  if ((rc = ix->upload(&d_gnode, gnode, s)) || (rc = ix->alloc(&cent, (size_t)G * D))) return rc;
  HIPCHK(launch_gather_rows_f32(mean, D, d_gnode, G, cent, s));
  for (int r = 0; r < NLi; ++r) {
    rgrp[r] = (cand[r] >= 0 && gok[cand[r]]) ? cand[r] : -1;
    ix->n_grp_rows += rgrp[r] >= 0;
  }
  std::vector<int> gpar(NI, -1);
  std::vector<double> F(NI, 0.0), Fc(NI, 0.0);
  for (int p = 1; p < NI; ++p) {
    const int g = gint[p];
    if (g < 0 || !gok[g] || std::isnan(pcw[p])) continue;
    gpar[p] = g;
    const double hs = (double)(float)(-0.5 * (double)pcw[p] * (double)piv[p]);   // RowF.hs (fp32)
    const double hsc = (double)(float)(-0.5 * (double)piv[p]);                    // categorize RowF.hs
    F[p] = hs / (double)pinvL[p];
    Fc[p] = hsc;
  }
  ix->grp_mode = true;
  ix->G = G;
  ix->grp_c = cent;
  if ((rc = ix->upload(&ix->grp_par, gpar, s)) || (rc = ix->upload(&ix->grp_F, F, s)) ||
      (rc = ix->upload(&ix->grp_Fc, Fc, s)))
    return rc;
  HIPCHK(hipStreamSynchronize(s));
  return CWQ_OK;
}

int build_filter(cwq_index* ix, const float* mean, const int64_t* d_rows, const std::vector<RowMeta>& meta,
                 const std::vector<int>& row_par, const std::vector<int>& row_flags,
                 const std::vector<int64_t>& int_nodes, const std::vector<int>& par_int, hipStream_t s) {
  int rc;
  const int DP = ix->DP, D = ix->D, NLi = ix->NL_iso;
  ix->DPB = fgemm_dpb(D);   // whole fgemm stages (cwq_mfma.hip)
  const int DPB = ix->DPB;
  ix->ld_f = round_up(NLi, kFgTile);
  const int64_t ld = ix->ld_f;
  float *n2 = nullptr, *nlo = nullptr, *nhi = nullptr, *nm = nullptr;
  if ((rc = ix->alloc(&ix->iso_Mf, (size_t)DP * ld))) return rc;
  if ((rc = ix->alloc(&ix->iso_Mb, (size_t)DPB * ld))) return rc;
  if ((rc = ix->alloc(&n2, ld))) return rc;
  if ((rc = ix->alloc(&nlo, ld))) return rc;
  if ((rc = ix->alloc(&nhi, ld))) return rc;
  if ((rc = ix->alloc(&nm, ld))) return rc;
  if ((rc = ix->alloc(&ix->iso_c, D))) return rc;
  HIPCHK(hipMemcpyAsync(ix->iso_c, mean, (size_t)D * 4, hipMemcpyDeviceToDevice, s));   // root mean
  std::vector<int> rgrp;
  if ((rc = plan_groups(ix, mean, d_rows, meta, row_par, int_nodes, par_int, rgrp, s))) return rc;
  int* d_rgrp = nullptr;
  if (ix->grp_mode && (rc = ix->upload(&d_rgrp, rgrp, s))) return rc;
  HIPCHK(launch_rows_prep(mean, D, d_rows, NLi, ix->iso_c, DP, DPB, ld, ix->iso_Mf, ix->iso_Mb, n2, nlo, nhi, s,
                          ix->grp_c, d_rgrp, nm));
  std::vector<float> hn2(ld), hlo(ld), hhi(ld), hnm(ld);
  HIPCHK(hipMemcpyAsync(hn2.data(), n2, ld * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hlo.data(), nlo, ld * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hhi.data(), nhi, ld * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(hnm.data(), nm, ld * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const FiltConsts fc = filt_consts(DPB);
  // per-row and per-tile constants.  Fast key (cat = false): pi + hs*S + hl with
  // hs = -cw*iv/2, hl = -cw*logdet/2, pi = P[parent]/L.  Categorize (cat = true): the
  // full lp = -(logdet + D log 2pi)/2 - iv*S/2 (cw = 1, no prefix term: invL = 0, tiles
  // parent-free), min'ed with BF[parent] in the kernels; usable = not an internal copy.
  const float dfull = (float)((double)ix->D * (double)logf(2.0f * (float)M_PI));
  ix->cat_dconst = dfull;
  // multi-parent tiles keep the pretest up to this many parents (deep trees: ~4 leaves
  // per parent puts ~64 parents in a 256-row tile); CWQ_FG_MAX_PARENTS overrides
  const int max_parents = [] {
    const char* e = getenv("CWQ_FG_MAX_PARENTS");
    return e && *e ? std::max(1, atoi(e)) : kFgMaxTileParents;
  }();
  // Fast key row terms R0 of the rows a uniform tile may hold (-inf: none), for the hub rows
  // of the threshold sample below
  std::vector<float> hub_key(NLi, -INFINITY);
  auto tables = [&](bool cat, std::vector<RowF>& rf, std::vector<TileF>& tf) {
    rf.assign(ld, RowF{});
    std::vector<double> gr(ld, 0.0);
    for (int64_t r = 0; r < ld; ++r) {
      RowF& f = rf[r];
      const bool usable = r < NLi && (cat ? !(row_flags[r] & FLAG_INT_COPY) : (row_flags[r] & FLAG_HAS_SENT) != 0);
      if (!usable) {
        f = RowF{-INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -2};
        continue;
      }
      const RowMeta& m = meta[r];
      const double cw = cat ? 1.0 : (double)m.cw;
      const double ldet = cat ? (double)(m.logdet + dfull) : (double)m.logdet;   // fp32 add, as the scan
      const double hs = -0.5 * cw * (double)m.iv, hl = -0.5 * cw * ldet;
      const double g = cw * (double)m.iv;
      const bool grow = ix->grp_mode && rgrp[r] >= 0;
      // group-centred rows: the fp32 rounding of M = fl(mu - c_g) enters the dot through
      // |x'| |M| -- 2^-23 |M| on both split norms covers it (cwq_group.hip)
      const double ge = grow ? std::ldexp((double)hnm[r], -23) * (1.0 + std::ldexp(1.0, -20)) : 0.0;
      f.beta = round_up_f((double)hlo[r] + fc.gamma * (double)hhi[r] + ge);
      f.delta = round_up_f((double)hhi[r] + (double)hlo[r] + ge);
      f.rn2 = hn2[r];
      f.hs = (float)hs;
      f.hl = (float)hl;
      // categorize reads a prefix term only for group-centred rows: their group term
      f.invL = cat ? (grow ? 1.f : 0.f) : m.invL;
      f.par = row_par[r];
      gr[r] = g;
      if (g > 0.0 && std::isfinite(g) && std::isfinite(hl)) {
        const double rn2 = hn2[r];
        double R = hl / g - 0.5 * rn2 + 0.5 * fc.eps_n * rn2 + fc.slack * (std::fabs(hl) / g + 1.5 * rn2);
        R += 4.0 * fc.gamma * (std::fabs(R) + std::fabs(hl) / g + rn2);
        f.R0 = round_up_f(R);
        if (!cat && f.par >= -1 && std::isfinite(f.R0)) hub_key[r] = f.R0;
      } else {
        f.R0 = 0.f;   // only ever on non-uniform tiles
      }
    }
    const int n_rt = (int)(ld / kFgTile);
    tf.assign(n_rt, TileF{});
    for (int t = 0; t < n_rt; ++t) {
      TileF& T = tf[t];
      T = TileF{1, -1, 1.f, 1.f, 0.f, 0.f, -1, 0.f};
      bool first = true, same_par = true;
      int plo = INT32_MAX, phi = -1, tgrp = -1;
      for (int64_t r = (int64_t)t * kFgTile; r < (int64_t)(t + 1) * kFgTile; ++r) {
        if (rf[r].par < -1) continue;
        const double g = gr[r];
        if (!(g > 0.0) || !std::isfinite(g) || !std::isfinite(rf[r].R0)) T.uniform = 0;
        // categorize tiles: parent-free, or (group-centred rows) all rows of one group,
        // whose term any of their parents carries
        const int cg = ix->grp_mode && r < NLi ? rgrp[r] : -1;
        if (first) {
          T.par = cat ? (cg >= 0 ? rf[r].par : -1) : rf[r].par;
          T.invL = rf[r].invL;
          T.g = (float)g;
          tgrp = cg;
          first = false;
        } else if (rf[r].invL != T.invL || (float)g != T.g || (cat && cg != tgrp)) {
          T.uniform = 0;
        }
        if (!cat && rf[r].par != T.par) same_par = false;
        plo = std::min(plo, rf[r].par);
        phi = std::max(phi, rf[r].par);
        T.beta_max = std::max(T.beta_max, rf[r].beta);
        T.delta_max = std::max(T.delta_max, rf[r].delta);
      }
      T.par_hi = T.par;
      if (T.uniform && !same_par) {
        if (plo >= 0 && phi - plo < max_parents && !env_set("CWQ_FG_NO_MULTI")) {
          T.uniform = 2;
          T.par = plo;
          T.par_hi = phi;
        } else {
          T.uniform = 0;
        }
      }
    }
  };
  std::vector<RowF> rf;
  std::vector<TileF> tf;
  tables(false, rf, tf);
  const int n_rt = (int)(ld / kFgTile);
  if ((rc = ix->upload(&ix->iso_rf, rf, s))) return rc;
  if ((rc = ix->upload(&ix->iso_tf, tf, s))) return rc;
  ix->tile_uni_prefix.assign(n_rt + 1, 0);
  // all_uniform launches (fgemm_kernel<0, true>) need single-parent tiles
  for (int t = 0; t < n_rt; ++t) ix->tile_uni_prefix[t + 1] = ix->tile_uni_prefix[t] + (tf[t].uniform == 1 ? 1 : 0);
  ix->n_multi_tiles = 0;
  for (int t = 0; t < n_rt; ++t) ix->n_multi_tiles += tf[t].uniform == 2 ? 1 : 0;
  HIPCHK(hipStreamSynchronize(s));   // the uploads read rf / tf, rebuilt below
  tables(true, rf, tf);
  if ((rc = ix->upload(&ix->cat_rf, rf, s))) return rc;
  if ((rc = ix->upload(&ix->cat_tf, tf, s))) return rc;
  ix->cat_uni_prefix.assign(n_rt + 1, 0);
  for (int t = 0; t < n_rt; ++t) ix->cat_uni_prefix[t + 1] = ix->cat_uni_prefix[t] + (tf[t].uniform == 1 ? 1 : 0);
  HIPCHK(hipStreamSynchronize(s));   // the host vectors above are freed on return
  // threshold sample: ~NL_iso/128 rows at a fixed stride, 256 <= S <= 32768 (the filter
  // phases tighten T afterwards, so a small sample only costs the first phase)
  const char* sd = getenv("CWQ_FG_SAMPLE_DIV");
  const int sdiv = sd && atoi(sd) > 0 ? atoi(sd) : 128;
  int S = (int)std::min<int64_t>(32768, std::max<int64_t>(kFgTile, NLi / sdiv / kFgTile * kFgTile));
  const int stride = std::max(1, NLi / S);
  std::vector<int> srow;
  srow.reserve(S);
  for (int j = 0; j < S; ++j) {
    const int64_t r = (int64_t)j * stride;
    if (r < NLi) srow.push_back((int)r);
  }
  if (ix->grp_mode) {
    // clustered trees: the query's own cluster decides its top-k, and a strided sample
    // holds only ~1/sdiv of it, so T stayed at other clusters' keys and most of the
    // cluster passed the filter (C2 ifit tree: ~1,100 candidates per query, overflowing
    // the record buffers).  Add kPerGroup rows of every group, spread over its rows
    // (distinct rows only: T must bound the K-th best key over distinct rows).
    // (fewer per group on a deep cut: the sample stays within 32,768 rows)
    const int kPerGroup = std::max(8, std::min(64, (32768 - (int)srow.size()) / std::max(1, ix->G)));
    std::vector<std::vector<int>> gr(ix->G);
    for (int64_t r = 0; r < NLi; ++r)
      if (rgrp[r] >= 0) gr[rgrp[r]].push_back((int)r);
    std::vector<char> in(NLi, 0);
    for (int r : srow) in[r] = 1;
    for (int g = 0; g < ix->G && (int64_t)srow.size() + kPerGroup <= 32768; ++g) {
      const int n = (int)gr[g].size();
      const int m = std::min(n, kPerGroup);
      for (int j = 0; j < m; ++j) {
        const int r = gr[g][(int64_t)j * n / m];
        if (!in[r]) {
          in[r] = 1;
          srow.push_back(r);
        }
      }
    }
  }
  // hub rows: the rows with the largest query-independent term R0 of the Fast key (small
  // |mu'|^2) are the likely top-k of any query, so with them in the sample the first launch
  // already runs near the threshold the call ends with (C3: the K-th best key of the
  // lowest-norm 1/128 of the rows has median rank 25 of 1M, of a strided 1/128 rank ~1,100).
  // H = S/2 rows by default (CWQ_FG_HUB_DIV = n: NL_iso/n; 0: none), appended after the
  // strided rows -- S is a multiple of 256, so the sample pass's 4-row groups keep their
  // members -- ties by smaller row index, rows of the strided sample skipped (T bounds the
  // K-th best key over DISTINCT rows).  The sample pass keeps one maximum per 4 consecutive
  // sample rows, so hub j of H goes to group j mod H/4: the best H/4 hubs each lead a group.
  ix->n_hub = 0;
  if (!ix->grp_mode && NLi >= 4 * S) {
    const char* hd = getenv("CWQ_FG_HUB_DIV");
    const int64_t want = hd && *hd ? (atoi(hd) > 0 ? NLi / atoi(hd) / kFgTile * kFgTile : 0) : S / 2;
    const int H = (int)std::min<int64_t>(want, (32768 - (int64_t)srow.size()) / 4 * 4);
    if (H > 0) {
      std::vector<int> cand;
      cand.reserve(NLi);
      for (int r = 0; r < NLi; ++r)
        if (hub_key[r] > -INFINITY) cand.push_back(r);
      // the best H rows outside the strided sample are among the best H + |strided| rows
      const size_t top = std::min(cand.size(), (size_t)H + srow.size());
      std::partial_sort(cand.begin(), cand.begin() + top, cand.end(), [&](int a, int b) {
        return hub_key[a] > hub_key[b] || (hub_key[a] == hub_key[b] && a < b);
      });
      std::vector<char> in(NLi, 0);
      for (int r : srow) in[r] = 1;
      std::vector<int> hub;
      hub.reserve(H);
      for (size_t i = 0; i < top && (int)hub.size() < H; ++i)
        if (!in[cand[i]]) hub.push_back(cand[i]);
      const int nh = (int)hub.size(), ng = (nh + 3) / 4;
      for (int g = 0; g < ng; ++g)
        for (int j = g; j < nh; j += ng) srow.push_back(hub[j]);
      ix->n_hub = nh;
    }
  }
  const int ns = (int)srow.size();
  srow.resize(round_up(ns, kFgTile), -1);
  ix->n_samp = ns;
  ix->ld_s = (int)srow.size();
  if ((rc = ix->upload(&ix->samp_rows, srow, s))) return rc;
  if ((rc = ix->alloc(&ix->iso_Sb, (size_t)DPB * ix->ld_s))) return rc;
  HIPCHK(launch_gather_bf16_rows(ix->iso_Mb, DPB, ix->samp_rows, ix->ld_s, ix->iso_Sb, s));
  HIPCHK(hipStreamSynchronize(s));
  return CWQ_OK;
}

// Group pruning constants (cwq_prune.hip).  Groups are plan_groups' cut:
// a group's members are the internal nodes of its centre's subtree and the leaf-class rows
// below them (a row that is itself an internal node belongs to that node's group); the top
// nodes (the root and the centres' ancestors) belong to no group and every query computes
// them exactly (prune_head_kernel).  Needs the group-centred mode (group centres), the
// row-major A/B copies (exact pass of a group), and every level weight and row weight >= 0
// (the key bound adds upper bounds of lp' with non-negative coefficients).
// CWQ_GROUP_PRUNE=0 at index creation leaves it off.
int build_prune(cwq_index* ix, const float* mean, const VarSrc& var, const std::vector<int64_t>& int_nodes,
                const std::vector<int>& par_int, const std::vector<float>& w_int, const std::vector<int64_t>& rows,
                const std::vector<int>& int_id, const std::vector<RowMeta>& meta, const std::vector<int>& row_par,
                const std::vector<int>& row_flags, hipStream_t s) {
  if (env_off("CWQ_GROUP_PRUNE") || !ix->grp_mode || ix->G <= 0 || !ix->int_Ar || ix->NI < 2 || ix->DP > 2048)
    return CWQ_OK;
  const int NI = ix->NI, NL = ix->NL, G = ix->G;
  for (float w : w_int)
    if (!(w >= 0.f)) return CWQ_OK;
  for (int r = 0; r < NL; ++r)
    if (!(meta[r].cw >= 0.f) || !(meta[r].invL >= 0.f)) return CWQ_OK;
  // pruning group of every internal node (plan_groups' cut; -1: a top node)
  const std::vector<int>& gint = ix->cut_gint;
  if ((int)gint.size() != NI || (int)ix->cut_centre.size() != G) return CWQ_OK;
  // top nodes, BFS order: their parents are top nodes too (a cut)
  std::vector<int> tnodes, tpos(NI, -1), tpp, tdep;
  std::vector<int> idep(NI, 0);
  for (int i = 1; i < NI; ++i) idep[i] = idep[par_int[i]] + 1;
  for (int i = 0; i < NI; ++i) {
    if (gint[i] >= 0) continue;
    const int p = i == 0 ? -1 : par_int[i];
    if (p >= 0 && tpos[p] < 0) return CWQ_OK;   // never: the parent of a top node is a top node
    tpos[i] = (int)tnodes.size();
    tnodes.push_back(i);
    tpp.push_back(p >= 0 ? tpos[p] : -1);
    tdep.push_back(idep[i]);
  }
  std::vector<int> gtpos(G);
  for (int g = 0; g < G; ++g) {
    const int c = ix->cut_centre[g];
    if (gint[c] != g || tpos[par_int[c]] < 0) return CWQ_OK;   // never: a centre's parent is a top node
    gtpos[g] = tpos[par_int[c]];
  }
  // members: internal nodes 1.. (top nodes: no group), then rows
  std::vector<int64_t> mnode;
  std::vector<float> miv;
  std::vector<int> mgrp;
  for (int i = 1; i < NI; ++i) {
    mnode.push_back(int_nodes[i]);
    miv.push_back(0.f);
    mgrp.push_back(gint[i]);
  }
  std::vector<int> rgrp(NL, -1);
  for (int r = 0; r < NL; ++r) {
    const int own = int_id[rows[r]];
    rgrp[r] = own >= 0 ? gint[own] : (row_par[r] >= 0 ? gint[row_par[r]] : -1);
    mnode.push_back(rows[r]);
    miv.push_back(r < ix->NL_iso ? meta[r].iv : 0.f);
    mgrp.push_back(rgrp[r]);
  }
  const int64_t nm = (int64_t)mnode.size();
  int64_t* d_mnode = nullptr;
  float* d_miv = nullptr;
  int* d_mgrp = nullptr;
  double4* d_out = nullptr;
  int rc;
  if ((rc = ix->upload(&d_mnode, mnode, s)) || (rc = ix->upload(&d_miv, miv, s)) || (rc = ix->upload(&d_mgrp, mgrp, s)) ||
      (rc = ix->alloc(&d_out, nm)))
    return rc;
  HIPCHK(launch_prune_members(mean, var, ix->D, d_mnode, d_miv, d_mgrp, ix->grp_c, nm, d_out, s));
  std::vector<double4> mo(nm);
  std::vector<float> ldi(NI);
  HIPCHK(hipMemcpyAsync(mo.data(), d_out, nm * sizeof(double4), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ldi.data(), ix->logdet_int, NI * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<GroupBound> gb(G);
  std::vector<double> d2max(G, 0.0), m2max(G, 0.0);
  for (auto& b : gb) {
    b = GroupBound{};
    b.wmin = INFINITY;
    b.wmax = 0.0;
    b.ldmin = INFINITY;
    b.ldabs = 0.0;
    b.iLmin = b.Cmin = INFINITY;
    b.iLmax = b.Cmax = -INFINITY;
    b.valid = 0;
  }
  for (int64_t m = 0; m < nm; ++m) {
    const int g = mgrp[m];
    if (g < 0) continue;
    GroupBound& b = gb[g];
    b.wmin = std::min(b.wmin, mo[m].x);
    b.wmax = std::max(b.wmax, mo[m].y);
    d2max[g] = std::max(d2max[g], mo[m].z);
    m2max[g] = std::max(m2max[g], mo[m].w);
    const double ld = m < NI - 1 ? (double)ldi[m + 1] : (double)meta[m - (NI - 1)].logdet;
    b.ldmin = std::min(b.ldmin, ld);
    b.ldabs = std::max(b.ldabs, std::fabs(ld));
  }
  // the key coefficients of the usable rows: 1/L and C = invL * sum_{a in path, a in g} w_a + cw
  // (the path's top nodes -- the root down to the centre's parent t_g -- are P(t_g), exact)
  std::vector<double> wsum(NI, 0.0);   // sum of w over the path of internal node i within its group
  for (int i = 1; i < NI; ++i)
    if (gint[i] >= 0) wsum[i] = (gint[par_int[i]] == gint[i] ? wsum[par_int[i]] : 0.0) + (double)w_int[i];
  for (int r = 0; r < NL; ++r) {
    const int g = rgrp[r];
    if (g < 0 || !(row_flags[r] & FLAG_HAS_SENT)) continue;
    GroupBound& b = gb[g];
    const int rp = row_par[r];
    const double iL = meta[r].invL, C = iL * (rp >= 0 && gint[rp] == g ? wsum[rp] : 0.0) + (double)meta[r].cw;
    b.iLmin = std::min(b.iLmin, iL);
    b.iLmax = std::max(b.iLmax, iL);
    b.Cmin = std::min(b.Cmin, C * (1.0 - 0x1p-40));
    b.Cmax = std::max(b.Cmax, C * (1.0 + 0x1p-40));
    b.valid = 1;
  }
  for (int g = 0; g < G; ++g) {
    GroupBound& b = gb[g];
    b.r = std::sqrt(d2max[g]) * (1.0 + 0x1p-40) + 1e-30;
    b.mmax = std::sqrt(m2max[g]) * (1.0 + 0x1p-40);
    b.wmin *= 1.0 - 0x1p-40;
    b.wmax *= 1.0 + 0x1p-40;
    if (!(b.wmin > 0.0) || !std::isfinite(b.wmax) || !std::isfinite(b.ldmin)) b.valid = b.valid ? -1 : 0;
  }
  for (auto& b : gb)
    if (b.valid < 0) return CWQ_OK;   // a member without a finite positive weight: no bound
  // group-major internal node lists (ascending internal id)
  std::vector<int> gptr(G + 1, 0), gnodes;
  for (int i = 1; i < NI; ++i)
    if (gint[i] >= 0) gptr[gint[i] + 1]++;
  for (int g = 0; g < G; ++g) gptr[g + 1] += gptr[g];
  gnodes.assign(gptr[G], 0);
  std::vector<int> fillp(gptr.begin(), gptr.end() - 1);
  for (int i = 1; i < NI; ++i)
    if (gint[i] >= 0) gnodes[fillp[gint[i]]++] = i;
  ix->prn_gmax = 1;
  for (int g = 0; g < G; ++g) ix->prn_gmax = std::max(ix->prn_gmax, gptr[g + 1] - gptr[g]);
  // LDS of the seed and stage-B kernels (their group-prefix arrays grow with the largest group)
  if (prune_lds_max(ix->DP, ix->prn_gmax) > kPruneLdsCap) return CWQ_OK;
  // per list entry: depth (root 0) and the parent's position in the same list (-1: the
  // centre, whose parent is a top node; the lists are BFS-ordered, so a level is finished
  // before the next starts)
  std::vector<int> lpos(NI, -1), gdep(gnodes.size()), gpp(gnodes.size());
  for (size_t j = 0; j < gnodes.size(); ++j) lpos[gnodes[j]] = (int)j;
  ix->prn_maxdep = 0;
  ix->prn_mindep = INT32_MAX;
  for (size_t j = 0; j < gnodes.size(); ++j) {
    const int i = gnodes[j], p = par_int[i];
    gdep[j] = idep[i];
    const bool inner = gint[p] == gint[i];
    gpp[j] = inner ? lpos[p] : -1;
    ix->prn_maxdep = std::max(ix->prn_maxdep, idep[i]);
    ix->prn_mindep = std::min(ix->prn_mindep, idep[i]);
    if (inner ? lpos[p] >= (int)j : i != ix->cut_centre[gint[i]]) return CWQ_OK;   // never: a group is a subtree in BFS order
  }
  if (ix->prn_mindep == INT32_MAX) ix->prn_mindep = 1;
  if (gdep.empty()) {
    gdep.push_back(0);
    gpp.push_back(-1);
  }
  // the seed threshold's rows: up to 64 usable isotropic rows of each group, spread over it
  std::vector<std::vector<int>> grows(G);
  for (int r = 0; r < ix->NL_iso; ++r)
    if (rgrp[r] >= 0 && (row_flags[r] & FLAG_HAS_SENT)) grows[rgrp[r]].push_back(r);
  std::vector<int> sptr2(G + 1, 0), srows2;
  for (int g = 0; g < G; ++g) {
    const int n = (int)grows[g].size(), m = std::min(n, 64);
    for (int j = 0; j < m; ++j) srows2.push_back(grows[g][(int64_t)j * n / m]);
    sptr2[g + 1] = (int)srows2.size();
  }
  if (srows2.empty()) srows2.push_back(0);
  if ((rc = ix->upload(&ix->gs_ptr, sptr2, s)) || (rc = ix->upload(&ix->gs_rows, srows2, s))) return rc;
  // the per-call filter's blocks: a block is left out when its rows' one group is pruned
  std::vector<int> bg((size_t)std::max<int64_t>(1, ((int64_t)ix->NL_iso + 15) / 16), -1);
  for (int64_t b = 0; b * 16 < ix->NL_iso; ++b) {
    const int r0 = (int)(b * 16), r1 = (int)std::min<int64_t>(ix->NL_iso, b * 16 + 16);
    int g = rgrp[r0];
    for (int r = r0 + 1; r < r1 && g >= 0; ++r)
      if (rgrp[r] != g) g = -1;
    bg[b] = g;
  }
  if ((rc = ix->upload(&ix->blk_grp, bg, s))) return rc;
  if ((rc = ix->upload(&ix->gi_dep, gdep, s)) || (rc = ix->upload(&ix->gi_ppos, gpp, s))) return rc;
  ix->n_top = (int)tnodes.size();
  ix->top_maxdep = 0;
  for (int d : tdep) ix->top_maxdep = std::max(ix->top_maxdep, d);
  if ((rc = ix->upload(&ix->top_nodes, tnodes, s)) || (rc = ix->upload(&ix->top_ppos, tpp, s)) ||
      (rc = ix->upload(&ix->top_dep, tdep, s)) || (rc = ix->upload(&ix->grp_tpos, gtpos, s)))
    return rc;
  if ((rc = ix->upload(&ix->prn_gint, gint, s)) || (rc = ix->upload(&ix->gi_ptr, gptr, s)) ||
      (rc = ix->upload(&ix->gi_nodes, gnodes, s)) || (rc = ix->upload(&ix->gbound, gb, s)) ||
      (rc = ix->alloc(&ix->prune_ctr, 8)))
    return rc;
  HIPCHK(hipMemsetAsync(ix->prune_ctr, 0, 8 * sizeof(int), s));
  HIPCHK(hipStreamSynchronize(s));
  ix->prune_ok = true;
  return CWQ_OK;
}

// cwq_index_create / cwq_index_create_cv: `var` is either the full [n_nodes][D] array or
// the compact per-node form (VarSrc); both give the same index.
int index_create_impl(int device, int64_t n_nodes, int32_t dim, const float* mean, const VarSrc& var,
                      const int64_t* parent, const int64_t* node_of_sentence, int64_t n_sent, const double* level_w,
                      int32_t n_w, hipStream_t s, cwq_index** out) {

  // ---- structure (host) ----
  if (parent[0] != -1) return fail(CWQ_ERR_ARG, "parent[0] must be -1 (root first, BFS order)");
  std::vector<int> depth(n_nodes, 0), nchild(n_nodes, 0);
  for (int64_t i = 1; i < n_nodes; ++i) {
    const int64_t p = parent[i];
    if (p < 0 || p >= i) return fail(CWQ_ERR_ARG, "parent[i] must be in [0, i) (BFS order)");
    if (p < parent[i - 1]) return fail(CWQ_ERR_ARG, "parent array must be non-decreasing (BFS order)");
    depth[i] = depth[p] + 1;
    nchild[p]++;
  }
  std::vector<std::vector<int64_t>> sents(n_nodes);
  for (int64_t sidx = 0; sidx < n_sent; ++sidx) {
    const int64_t nd = node_of_sentence[sidx];
    if (nd < -1 || nd >= n_nodes) return fail(CWQ_ERR_ARG, "node_of_sentence out of range");
    if (nd >= 0) sents[nd].push_back(sidx);
  }
  std::unique_ptr<cwq_index> ix(new cwq_index());
  ix->device = device;
  ix->n_nodes = n_nodes;
  ix->n_sent = n_sent;
  ix->D = dim;
  ix->DP = (int)round_up(dim, kDChunk);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ix->cus = prop.multiProcessorCount;

  std::vector<int64_t> int_nodes, leaf_nodes;
  std::vector<int> int_id(n_nodes, -1);
  for (int64_t i = 0; i < n_nodes; ++i) {
    if (nchild[i] > 0) {
      int_id[i] = (int)int_nodes.size();
      int_nodes.push_back(i);
    }
    if (nchild[i] == 0 || !sents[i].empty()) leaf_nodes.push_back(i);
    ix->max_depth = std::max(ix->max_depth, depth[i]);
  }
  ix->NI = (int)int_nodes.size();
  const int64_t nleaf = (int64_t)leaf_nodes.size();

  // isotropy of leaf-class rows (device)
  int64_t* d_leaf_nodes = nullptr;
  int* d_iso = nullptr;
  int rc = ix->upload(&d_leaf_nodes, leaf_nodes, s);
  if (rc) return rc;
  if ((rc = ix->alloc(&d_iso, nleaf))) return rc;
  HIPCHK(launch_iso_flags(var, dim, d_leaf_nodes, nleaf, d_iso, s));
  std::vector<int> iso(nleaf);
  HIPCHK(hipMemcpyAsync(iso.data(), d_iso, nleaf * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));

  std::vector<int64_t> rows_iso, rows_an;
  for (int64_t r = 0; r < nleaf; ++r) (iso[r] ? rows_iso : rows_an).push_back(leaf_nodes[r]);
  ix->NL_iso = (int)rows_iso.size();
  ix->NL_an = (int)rows_an.size();
  ix->NL = ix->NL_iso + ix->NL_an;
  std::vector<int64_t> rows(rows_iso);
  rows.insert(rows.end(), rows_an.begin(), rows_an.end());
  std::vector<int> row_of_node(n_nodes, -1);
  for (int r = 0; r < ix->NL; ++r) row_of_node[rows[r]] = r;

  auto wdepth = [&](int d) -> double { return d < n_w ? level_w[d] : 1.0; };

  // leaf-row metadata
  std::vector<RowMeta> meta(ix->NL);
  std::vector<int> row_par(ix->NL), row_flags(ix->NL), row_bfs(ix->NL);
  std::vector<int64_t> sptr(ix->NL + 1, 0), sids;
  std::vector<int> row_of_sent(n_sent, -1);
  for (int r = 0; r < ix->NL; ++r) {
    const int64_t nd = rows[r];
    const int L = depth[nd] + 1;
    meta[r].cw = (float)(wdepth(depth[nd]) / L);
    meta[r].invL = (float)(1.0 / L);
    row_par[r] = parent[nd] >= 0 ? int_id[parent[nd]] : -1;
    row_flags[r] = (sents[nd].empty() ? 0 : FLAG_HAS_SENT) | (nchild[nd] > 0 ? FLAG_INT_COPY : 0);
    row_bfs[r] = (int)nd;
    for (int64_t sidx : sents[nd]) {
      sids.push_back(sidx);
      row_of_sent[sidx] = r;
    }
    sptr[r + 1] = (int64_t)sids.size();
  }
  // internal-node metadata
  std::vector<int> par_int(ix->NI), cb(ix->NI, 0), ce(ix->NI, 0), ibfs(ix->NI), ihs(ix->NI), inch(ix->NI);
  std::vector<int> la0(ix->NI, 0), la1(ix->NI, 0), lb0(ix->NI, 0), lb1(ix->NI, 0);
  std::vector<float> w_int(ix->NI);
  for (int i = 0; i < ix->NI; ++i) {
    const int64_t nd = int_nodes[i];
    par_int[i] = parent[nd] >= 0 ? int_id[parent[nd]] : -1;
    ibfs[i] = (int)nd;
    ihs[i] = sents[nd].empty() ? 0 : 1;
    inch[i] = nchild[nd];
    ix->max_fanout = std::max(ix->max_fanout, (int)nchild[nd]);
    w_int[i] = (float)wdepth(depth[nd]);
    cb[i] = ce[i] = -1;
    la0[i] = la1[i] = lb0[i] = lb1[i] = -1;
  }
  for (int64_t nd = 1; nd < n_nodes; ++nd) {   // children ranges (contiguous in each ordering)
    const int pi = int_id[parent[nd]];
    if (int_id[nd] >= 0) {
      if (cb[pi] < 0) cb[pi] = int_id[nd];
      ce[pi] = int_id[nd] + 1;
    }
    const int r = row_of_node[nd];
    if (r >= 0) {
      if (r < ix->NL_iso) {
        if (la0[pi] < 0) la0[pi] = r;
        la1[pi] = r + 1;
      } else {
        if (lb0[pi] < 0) lb0[pi] = r;
        lb1[pi] = r + 1;
      }
    }
  }
  for (int i = 0; i < ix->NI; ++i) {
    if (cb[i] < 0) cb[i] = ce[i] = 0;
    if (la0[i] < 0) la0[i] = la1[i] = 0;
    if (lb0[i] < 0) lb0[i] = lb1[i] = 0;
  }
  for (int i = 0; i < ix->NI;) {   // levels (BFS -> depth non-decreasing)
    int j = i;
    const int d0 = depth[int_nodes[i]];
    while (j < ix->NI && depth[int_nodes[j]] == d0) ++j;
    ix->levels.push_back({i, j});
    i = j;
  }
  std::vector<int> node_src(n_nodes);
  for (int64_t nd = 0; nd < n_nodes; ++nd) node_src[nd] = int_id[nd] >= 0 ? int_id[nd] : -(row_of_node[nd] + 1);
  std::vector<int> lv_starts;
  for (auto& lv : ix->levels) lv_starts.push_back(lv.first);
  lv_starts.push_back(ix->NI);

  // ---- device arrays ----
  const int DP = ix->DP;
  ix->ld_int = round_up(std::max(ix->NI, 1), kWave);
  ix->ld_iso = round_up(std::max(ix->NL_iso, 1), kWave);
  ix->ld_an = round_up(std::max(ix->NL_an, 1), kWave);
  int64_t *d_int_nodes = nullptr, *d_rows = nullptr;
  if ((rc = ix->upload(&d_int_nodes, int_nodes, s))) return rc;
  if ((rc = ix->upload(&d_rows, rows, s))) return rc;
  if ((rc = ix->alloc(&ix->int_A, (size_t)DP * ix->ld_int))) return rc;
  if ((rc = ix->alloc(&ix->int_B, (size_t)DP * ix->ld_int))) return rc;
  if ((rc = ix->alloc(&ix->iso_M, (size_t)DP * ix->ld_iso))) return rc;
  if ((rc = ix->alloc(&ix->an_A, (size_t)DP * ix->ld_an))) return rc;
  if ((rc = ix->alloc(&ix->an_B, (size_t)DP * ix->ld_an))) return rc;
  HIPCHK(launch_gather_T(mean, var, dim, d_int_nodes, ix->NI, 1, ix->int_A, ix->ld_int, DP, s));
  HIPCHK(launch_gather_T(mean, var, dim, d_int_nodes, ix->NI, 2, ix->int_B, ix->ld_int, DP, s));
  HIPCHK(launch_gather_T(mean, var, dim, d_rows, ix->NL_iso, 0, ix->iso_M, ix->ld_iso, DP, s));
  HIPCHK(launch_gather_T(mean, var, dim, d_rows + ix->NL_iso, ix->NL_an, 1, ix->an_A, ix->ld_an, DP, s));
  HIPCHK(launch_gather_T(mean, var, dim, d_rows + ix->NL_iso, ix->NL_an, 2, ix->an_B, ix->ld_an, DP, s));
  if ((rc = ix->alloc(&ix->logdet_int, ix->NI))) return rc;
  if ((rc = ix->alloc(&ix->logdet_row, ix->NL))) return rc;
  HIPCHK(launch_logdet(var, dim, d_int_nodes, ix->NI, ix->logdet_int, s));
  HIPCHK(launch_logdet(var, dim, d_rows, ix->NL, ix->logdet_row, s));
  float* d_iv = nullptr;
  if ((rc = ix->alloc(&d_iv, ix->NL))) return rc;
  HIPCHK(hipMemsetAsync(d_iv, 0, std::max(ix->NL, 1) * sizeof(float), s));
  HIPCHK(launch_inv_var0(var, dim, d_rows, ix->NL_iso, d_iv, s));
  std::vector<float> ldr(ix->NL), ivh(ix->NL);
  if (ix->NL) {
    HIPCHK(hipMemcpyAsync(ldr.data(), ix->logdet_row, ix->NL * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ivh.data(), d_iv, ix->NL * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  for (int r = 0; r < ix->NL; ++r) {
    meta[r].logdet = ldr[r];
    meta[r].iv = ivh[r];
  }
  if ((rc = ix->upload(&ix->row_meta, meta, s))) return rc;
  if (ix->NL_iso > 0 && (rc = build_filter(ix.get(), mean, d_rows, meta, row_par, row_flags, int_nodes, par_int, s)))
    return rc;
  if ((rc = ix->upload(&ix->row_par, row_par, s))) return rc;
  if ((rc = ix->upload(&ix->row_flags, row_flags, s))) return rc;
  if ((rc = ix->upload(&ix->row_bfs, row_bfs, s))) return rc;
  {
    std::vector<int> rdep(ix->NL), idep(ix->NI);
    for (int r = 0; r < ix->NL; ++r) rdep[r] = depth[rows[r]];
    for (int i = 0; i < ix->NI; ++i) idep[i] = depth[int_nodes[i]];
    if ((rc = ix->upload(&ix->row_depth, rdep, s)) || (rc = ix->upload(&ix->int_depth, idep, s))) return rc;
  }
  if ((rc = ix->upload(&ix->par_int, par_int, s))) return rc;
  if ((rc = ix->upload(&ix->w_int, w_int, s))) return rc;
  if ((rc = ix->upload(&ix->int_child_begin, cb, s))) return rc;
  if ((rc = ix->upload(&ix->int_child_end, ce, s))) return rc;
  if ((rc = ix->upload(&ix->int_nchild, inch, s))) return rc;
  if ((rc = ix->upload(&ix->int_bfs, ibfs, s))) return rc;
  if ((rc = ix->upload(&ix->int_has_sent, ihs, s))) return rc;
  for (int v : ihs) ix->any_int_sent = ix->any_int_sent || v != 0;
  if ((rc = ix->upload(&ix->int_leaf_a0, la0, s))) return rc;
  if ((rc = ix->upload(&ix->int_leaf_a1, la1, s))) return rc;
  if ((rc = ix->upload(&ix->int_leaf_b0, lb0, s))) return rc;
  if ((rc = ix->upload(&ix->int_leaf_b1, lb1, s))) return rc;
  if ((rc = ix->upload(&ix->sent_ptr, sptr, s))) return rc;
  if ((rc = ix->upload(&ix->sent_ids, sids, s))) return rc;
  if ((rc = ix->upload(&ix->row_of_sent, row_of_sent, s))) return rc;
  if ((rc = ix->upload(&ix->node_src, node_src, s))) return rc;
  if ((rc = ix->upload(&ix->d_lv, lv_starts, s))) return rc;
  if (ix->NI > 0) {   // the root's terms (the per-call probe's fused prep forms its prefix)
    ix->root_w0 = w_int[0];
    HIPCHK(hipMemcpyAsync(&ix->root_logdet0, ix->logdet_int, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (ix->NL_iso > 0 && ix->NI >= 2 && ix->max_depth <= kMaxChain) {
    // internal-node bound operands: K = [x'^2, x'] -> DPB2 = fgemm width of 2*DP
    ix->DPB2 = fgemm_dpb(2 * ix->DP);
    ix->int_path = !env_off("CWQ_INT_PATH");
    const float gamma2 = (float)((ix->DPB2 + 64) * std::ldexp(1.0, -23));
    ix->root_w = w_int[0];
    HIPCHK(hipMemcpyAsync(&ix->root_ld, ix->logdet_int, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = ix->alloc(&ix->int_Ar, (size_t)ix->NI * DP))) return rc;
    if ((rc = ix->alloc(&ix->int_Br, (size_t)ix->NI * DP))) return rc;
    std::vector<int> rowid;
    if (ix->int_path) {
      // rows: the root (its exact prefix: final_kernel's chain starts from P[q][0]) and
      // every internal node with isotropic leaf rows below it, in id order
      for (int i = 0; i < ix->NI; ++i)
        if (i == 0 || la1[i] > la0[i]) rowid.push_back(i);
      ix->ld_i2 = round_up((int64_t)rowid.size(), kFgTile);
      const int64_t n = (int64_t)rowid.size();
      rowid.resize(ix->ld_i2, -1);
      if ((rc = ix->alloc(&ix->int_Mb2, (size_t)ix->DPB2 * ix->ld_i2))) return rc;
      if ((rc = ix->alloc(&ix->int_rf2, (size_t)ix->ld_i2))) return rc;
      if ((rc = ix->upload(&ix->int_rowid, rowid, s))) return rc;
      HIPCHK(launch_int_prep(mean, var, dim, d_int_nodes, ix->NI, ix->iso_c, ix->logdet_int, ix->par_int, ix->w_int, DP,
                             ix->DPB2, ix->NI, nullptr, nullptr, ix->int_Ar, ix->int_Br, gamma2, s));
      HIPCHK(launch_int_path_prep(mean, var, dim, d_int_nodes, ix->int_rowid, n, ix->iso_c, ix->logdet_int,
                                  ix->par_int, ix->w_int, DP, ix->DPB2, ix->ld_i2, ix->int_Mb2, ix->int_rf2, gamma2, s));
      // the same RowF by internal id, for the readers of the path-sum dots (PathB)
      std::vector<RowF> rf2h((size_t)n), nrf((size_t)ix->NI, RowF{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -2});
      HIPCHK(hipMemcpyAsync(rf2h.data(), ix->int_rf2, (size_t)n * sizeof(RowF), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (int64_t r = 0; r < n; ++r) nrf[rowid[r]] = rf2h[r];
      if ((rc = ix->upload(&ix->int_nrf, nrf, s))) return rc;
    } else {
      // level-aligned operand layout: segments [levels 0 and 1], [level 2], [level 3], ...,
      // each padded to whole 256-row tiles
      std::vector<std::pair<int, int>> segs;   // internal id ranges
      for (size_t lv = 0; lv < ix->levels.size(); ++lv) {
        if (lv == 1) segs.back().second = ix->levels[1].second;
        else segs.push_back(ix->levels[lv]);
      }
      std::vector<int64_t> seg_row(segs.size());
      int64_t rows = 0;
      for (size_t g = 0; g < segs.size(); ++g) {
        seg_row[g] = rows;
        rows += round_up(segs[g].second - segs[g].first, kFgTile);
      }
      ix->ld_i2 = rows;
      rowid.assign(rows, -1);
      for (size_t g = 0; g < segs.size(); ++g)
        for (int i = segs[g].first; i < segs[g].second; ++i) rowid[seg_row[g] + (i - segs[g].first)] = i;
      if ((rc = ix->alloc(&ix->int_Mb2, (size_t)ix->DPB2 * ix->ld_i2))) return rc;
      if ((rc = ix->alloc(&ix->int_rf2, (size_t)ix->ld_i2))) return rc;
      if ((rc = ix->upload(&ix->int_rowid, rowid, s))) return rc;
      for (size_t g = 0; g < segs.size(); ++g) {
        const int i0 = segs[g].first, n = segs[g].second - segs[g].first;
        HIPCHK(launch_int_prep(mean, var, dim, d_int_nodes + i0, n, ix->iso_c, ix->logdet_int + i0, ix->par_int + i0,
                               ix->w_int + i0, DP, ix->DPB2, round_up(n, kFgTile),
                               ix->int_Mb2 + (size_t)seg_row[g] * ix->DPB2, ix->int_rf2 + seg_row[g],
                               ix->int_Ar + (size_t)i0 * DP, ix->int_Br + (size_t)i0 * DP, gamma2, s));
      }
    }
    HIPCHK(hipStreamSynchronize(s));   // the rowid host vector is freed on return
    ix->int_bounds = true;
  }
  if ((rc = build_prune(ix.get(), mean, var, int_nodes, par_int, w_int, rows, int_id, meta, row_par, row_flags, s)))
    return rc;
  if ((rc = ix->alloc(&ix->dummy, 64))) return rc;
  // the per-call path's int8 row panel is built here, with the index, when its policy
  // holds (flat trees, >= kI8MinBytes of int8 rows, room on the device): no allocation or
  // first-call latency inside a query
  if (ix->NL_iso > 0 && !use_int_bounds(ix.get()))
    ix->i8_by_size = ensure_i8(ix.get(), s) && i8_size_rule(ix.get());
  HIPCHK(hipStreamSynchronize(s));
  *out = ix.release();
  return CWQ_OK;
}

int create_args_ok(int64_t n_nodes, int32_t dim, const float* mean, const int64_t* parent,
                   const int64_t* node_of_sentence, int64_t n_sent, cwq_index** out) {
  if (!out) return fail(CWQ_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (n_nodes <= 0 || dim <= 0 || !mean || !parent) return fail(CWQ_ERR_ARG, "empty tree or NULL inputs");
  if (n_nodes >= (int64_t)INT32_MAX / 2) return fail(CWQ_ERR_ARG, "too many nodes");
  if (n_sent < 0 || (n_sent > 0 && !node_of_sentence)) return fail(CWQ_ERR_ARG, "bad sentence map");
  return CWQ_OK;
}
}  // namespace

extern "C" int cwq_index_create(int device, int64_t n_nodes, int32_t dim, const float* mean, const float* var,
                                const int64_t* parent, const int64_t* node_of_sentence, int64_t n_sent,
                                const double* level_w, int32_t n_w, void* stream, cwq_index** out) {
  int rc = create_args_ok(n_nodes, dim, mean, parent, node_of_sentence, n_sent, out);
  if (rc) return rc;
  if (!var) return fail(CWQ_ERR_ARG, "var is NULL");
  DevGuard dg(device);
  const VarSrc vs{var, nullptr, nullptr, nullptr};
  return index_create_impl(device, n_nodes, dim, mean, vs, parent, node_of_sentence, n_sent, level_w, n_w,
                           (hipStream_t)stream, out);
}

extern "C" int cwq_index_create_cv(int device, int64_t n_nodes, int32_t dim, const float* mean, const float* var_row,
                                   const int64_t* an_nodes, int64_t n_an, const float* an_var, const int64_t* parent,
                                   const int64_t* node_of_sentence, int64_t n_sent, const double* level_w, int32_t n_w,
                                   void* stream, cwq_index** out) {
  int rc = create_args_ok(n_nodes, dim, mean, parent, node_of_sentence, n_sent, out);
  if (rc) return rc;
  if (!var_row || n_an < 0 || (n_an > 0 && (!an_nodes || !an_var))) return fail(CWQ_ERR_ARG, "bad compact var");
  std::vector<int> an_map(n_nodes, -1);
  for (int64_t j = 0; j < n_an; ++j) {
    const int64_t nd = an_nodes[j];
    if (nd < 0 || nd >= n_nodes) return fail(CWQ_ERR_ARG, "an_nodes out of range");
    if (an_map[nd] >= 0) return fail(CWQ_ERR_ARG, "an_nodes lists a node twice");
    an_map[nd] = (int)j;
  }
  DevGuard dg(device);
  hipStream_t s = (hipStream_t)stream;
  int* d_map = nullptr;
  if (hipMalloc(&d_map, (size_t)n_nodes * sizeof(int)) != hipSuccess)
    return fail(CWQ_ERR_OOM, "hipMalloc failed (compact var map)");
  if (hipMemcpyAsync(d_map, an_map.data(), (size_t)n_nodes * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipFree(d_map);
    return fail(CWQ_ERR_HIP, "compact var map upload failed");
  }
  const VarSrc vs{nullptr, var_row, d_map, an_var};
  rc = index_create_impl(device, n_nodes, dim, mean, vs, parent, node_of_sentence, n_sent, level_w, n_w, s, out);
  (void)hipStreamSynchronize(s);   // the build kernels read the map (an error path may return early)
  (void)hipFree(d_map);
  return rc;
}

// cwq_index_create_from_fit (cwq_fitindex.hip): mean and the compact variances (VarSrc with
// its an_map) already on the device; parent / node_of_sentence on the host.  Errors go to
// cwq_last_error (msg_out: the message, for the caller's own error slot).

namespace cwq {
int index_create_device(int device, int64_t n_nodes, int32_t dim, const float* mean, const VarSrc& var,
                        const int64_t* parent, const int64_t* node_of_sentence, int64_t n_sent,
                        const double* level_w, int32_t n_w, hipStream_t s, cwq_index** out, const char** msg_out) {
  int rc = create_args_ok(n_nodes, dim, mean, parent, node_of_sentence, n_sent, out);
  if (!rc) {
    DevGuard dg(device);
    rc = index_create_impl(device, n_nodes, dim, mean, var, parent, node_of_sentence, n_sent, level_w, n_w, s, out);
  }
  if (msg_out) *msg_out = cwq_last_error();
  return rc;
}
int index_fail(int code, const char* msg) { return fail(code, msg); }
}  // namespace cwq

extern "C" int cwq_index_destroy(cwq_index* idx) {
  if (!idx) return CWQ_OK;
  DevGuard dg(idx->device);
  delete idx;
  return CWQ_OK;
}
