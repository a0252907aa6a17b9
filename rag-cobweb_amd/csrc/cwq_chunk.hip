// The per-chunk exact passes of a query call (host side): the internal-node pass and its prefixes
// (exact, group-pruned or by bounds), the leaf scan, and the chunk's workspace sizing and carving.
// Shared by every query entry point behind cwq_handle.h.
#include "cwq_handle.h"

namespace cwq {
// ---------------------------------------------------------------------------
// Query orchestration
// ---------------------------------------------------------------------------

// The group-centred rows' prefix tables of a chunk (after the exact internal pass wrote
// c.P): q = the chunk's [nq][D] queries.  No-op without grp_mode.
int group_tables(cwq_index* ix, Chunk& c, const float* q, bool cat, hipStream_t s) {
  if (!ix->grp_mode || ix->NI == 0) return CWQ_OK;
  if (c.grp_done >= (cat ? 1 : 0)) return CWQ_OK;   // written by run_internal's fused pass
  HIPCHK(launch_group_prefixes(q, c.nq, ix->D, ix->iso_c, ix->grp_c, ix->G, c.P, c.ldP, ix->NI, ix->grp_par, ix->grp_F,
                               ix->grp_Fc, c.gsh, c.Pg_lo, c.Pg_hi, cat ? c.Pc_lo : nullptr, cat ? c.Pc_hi : nullptr,
                               s));
  return CWQ_OK;
}

// Group pruning (cwq_prune.hip) of a Fast chunk: on by default where the index built its
// constants (build_prune); CWQ_GROUP_PRUNE=0 turns it off per call (in-process A/Bs).
bool use_prune(const cwq_index* ix) {
  return ix->prune_ok && !env_off("CWQ_GROUP_PRUNE");
}
}  // namespace cwq

namespace {
size_t prune_bytes_per_query(const cwq_index* ix) { return ix->prune_ok ? (size_t)ix->G * 36 + 16 : 0; }
}  // namespace

namespace cwq {
// The pruned Fast chunk's internal pass, in place of run_internal + group_tables (four
// launches, cwq_prune.hip): the group shifts, the bound terms, the root, KUB and g* (head);
// g*'s exact pass over many workgroups; g*'s tables, the seed threshold from its sample rows,
// the stage-B pairs and the sentinel fill; stage B.  K: the call's top-K.  T0 (optional): the seed is
// also written there (the per-call filter's threshold: no probe pass).
int prune_internal(cwq_index* ix, Chunk& c, const float* q, int K, Bump& b, hipStream_t s, float* T0,
                   int64_t ldT0, int* live) {
  const int nq = c.nq, G = ix->G;
  PruneArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.nq = nq;
  pa.G = G;
  pa.NI = ix->NI;
  pa.DP = ix->DP;
  pa.D = ix->D;
  pa.K = K;
  pa.ldS = ix->NI;
  pa.q = q;
  pa.X = c.X;
  pa.c0 = ix->iso_c;
  pa.cent = ix->grp_c;
  pa.Ar = ix->int_Ar;
  pa.Br = ix->int_Br;
  pa.par_int = ix->par_int;
  pa.w_int = ix->w_int;
  pa.logdet_int = ix->logdet_int;
  pa.gint = ix->prn_gint;
  pa.gi_ptr = ix->gi_ptr;
  pa.gi_nodes = ix->gi_nodes;
  pa.gb = ix->gbound;
  pa.kpart = b.take<double>((size_t)3 * c.nq_pad * G);
  pa.S = c.S_int;
  pa.P = c.P;
  pa.Plo = c.Pg_lo;
  pa.Phi = c.Pg_hi;
  pa.grp = ix->grp_par;
  pa.F = ix->grp_F;
  pa.sh = c.gsh;
  pa.fillP = ix->NL_an > 0 ? 1 : 0;
  pa.kub = b.take<float>((size_t)c.nq_pad * G);
  pa.gstar = b.take<int>((size_t)c.nq_pad);
  pa.pairs = b.take<int2>((size_t)c.nq_pad * G);
  pa.ctr = ix->prune_ctr;   // the handle's (calls on it are serialised): [4] survives a fallback re-run
  pa.gs_ptr = ix->gs_ptr;
  pa.gs_rows = ix->gs_rows;
  pa.Mf = ix->iso_Mf;
  pa.meta = ix->row_meta;
  pa.row_par = ix->row_par;
  c.Tseed = b.take<float>((size_t)c.nq_pad);
  pa.Tseed = c.Tseed;
  pa.T0 = T0;
  pa.ldT0 = ldT0;
  pa.gnodes_max = ix->prn_gmax;
  pa.gi_dep = ix->gi_dep;
  pa.gi_ppos = ix->gi_ppos;
  pa.gmaxdep = ix->prn_maxdep;
  pa.gmindep = ix->prn_mindep;
  pa.top_nodes = ix->top_nodes;
  pa.top_ppos = ix->top_ppos;
  pa.top_dep = ix->top_dep;
  pa.n_top = ix->n_top;
  pa.top_maxdep = ix->top_maxdep;
  pa.grp_tpos = ix->grp_tpos;
  if (live) {   // the per-call filter's live block list (count in ctr[5])
    pa.blk_grp = ix->blk_grp;
    pa.nblk = ((int64_t)ix->NL_iso + 15) / 16;
    pa.live = live;
  }
  HIPCHK(launch_prune(pa, ix->cus, ix->prune_nq == 0, s));   // the call's first pruned chunk resets the total
  if (env_set("CWQ_PRUNE_DEBUG")) {   // diagnostics: the first queries' bounds and thresholds
    const int n = std::min(nq, 3);
    std::vector<float> kub((size_t)n * G), th(n);
    std::vector<int> gs(n), ctr(8);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(kub.data(), pa.kub, kub.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gs.data(), pa.gstar, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctr.data(), pa.ctr, 32, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(th.data(), pa.Tseed, n * 4, hipMemcpyDeviceToHost));
    fprintf(stderr, "[prune] nq %d G %d pairs %d total %d\n", nq, G, ctr[0], ctr[4]);
    for (int i = 0; i < n; ++i) {
      float mx = -INFINITY;
      for (int g = 0; g < G; ++g)
        if (g != gs[i]) mx = std::max(mx, kub[(size_t)i * G + g]);
      fprintf(stderr, "[prune] q %d T %g g* %d kub* %g others max %g\n", i, th[i], gs[i],
              gs[i] >= 0 ? kub[(size_t)i * G + gs[i]] : NAN, mx);
    }
  }
  c.grp_done = 0;   // the Fast tables are written (group_tables is a no-op)
  ix->prune_nq += nq;
  return CWQ_OK;
}

// The path-sum dots of a chunk after run_internal_bounds (int_path), or none.
PathB path_b(const cwq_index* ix, const Chunk& c) {
  if (c.pT && ix->int_path && c.qi2 && ix->int_nrf) return PathB{c.P, c.ldP, c.qi2, ix->int_nrf};
  return PathB{nullptr, 0, nullptr, nullptr};
}

// Query blocks of a launch; a multiple of 8 under the XCD-aware mapping (the
// extra blocks exit at once).
int n_qblocks_for(int64_t nq, int kl) {
  const int qpb = scan_queries_per_block(kl);
  const int n = (int)((nq + qpb - 1) / qpb);
  // XCD-aware mapping needs a multiple of 8 blocks; below 8 the padding blocks would be
  // 7/8 of the grid and of the slab count chosen for it, so small calls map plainly
  return scan_xcd_map() && n >= 8 ? (int)round_up(n, 8) : n;
}

// Choose the slab split of a segment: enough workgroups for >= ~5 waves of the
// resident grid, with the last wave as full as possible (tail balance).
int pick_nslab(const cwq_index* ix, int nrows, int n_qblocks, int kl) {
  if (nrows <= 0) return 0;
  const int max_slab = (int)std::max<int64_t>(1, round_up(nrows, kWave) / 256);
  const int64_t slots = (int64_t)ix->cus * scan_wgs_per_cu(kl);
  int best = 1;
  double best_fill = -1.0;
  for (int r = 5; r <= 10; ++r) {
    const int n = (int)std::max<int64_t>(1, std::min<int64_t>(max_slab, r * slots / std::max(1, n_qblocks)));
    const int64_t wgs = (int64_t)n * n_qblocks;
    const int64_t rounds = (wgs + slots - 1) / slots;
    const double fill = (double)wgs / (double)(rounds * slots);
    if (fill >= best_fill - 1e-9) {
      best_fill = fill;
      best = n;
    }
  }
  return best;
}
}  // namespace cwq

namespace {
ScanArgs base_args(const cwq_index* ix, const Chunk& c) {
  ScanArgs a;
  memset(&a, 0, sizeof(a));
  a.DP = ix->DP;
  a.nq = c.nq;
  a.meta = c.meta ? c.meta : ix->row_meta;
  a.par = ix->row_par;
  a.flags = ix->row_flags;
  a.P = c.P ? c.P : ix->dummy;   // query-major: the scans run with the exact pass's P (never after pT bounds)
  a.ldP = std::max(ix->NI, 1);
  a.xcd_map = scan_xcd_map();
  return a;
}

// Internal nodes: raw sums -> P (path prefix), BF (bottleneck), LPF (full lp).
// bf_lpf: also the path bottleneck BF and full lp LPF (categorize / log_prob); the fast
// keys need only P.
// The raw sums -> prefixes step of run_internal: one prefix_level_kernel launch per level,
// or (several levels, a few queries, shallow trees) internal_chain_kernel -- one thread per
// (query, node) down its path, same values -- which also writes the group-centred rows'
// prefix tables when q (the caller's queries) is given: grp_cat 0 Fast, 1 + categorize.
constexpr int kChainMaxQ = 64, kChainMaxDepth = 16;
int internal_prefixes(cwq_index* ix, Chunk& c, hipStream_t s, float* BF, float* LPF, float dfull, const float* q,
                      int grp_cat) {
  const float* w_int = c.w_int ? c.w_int : ix->w_int;
  const bool fin = ix->levels.size() > 1 && c.nq <= kChainMaxQ && ix->max_depth <= kChainMaxDepth &&
                   !env_off("CWQ_INT_FINISH");
  if (!fin) {
    for (auto& lv : ix->levels)
      HIPCHK(launch_prefix_level(c.S_int, ix->NI, c.nq, lv.first, lv.second, ix->par_int, w_int, ix->logdet_int,
                                 dfull, c.P, BF, LPF, s));
    return CWQ_OK;
  }
  IntFinishArgs f;
  memset(&f, 0, sizeof(f));
  f.S = c.S_int;
  f.ldS = ix->NI;
  f.nq = c.nq;
  f.NI = ix->NI;
  f.lv0 = ix->d_lv;
  f.nlev = (int)ix->levels.size();
  f.par_int = ix->par_int;
  f.w_int = w_int;
  f.logdet_int = ix->logdet_int;
  f.dfull = dfull;
  f.P = c.P;
  f.BF = BF;
  f.LPF = LPF;
  const bool grp = q && grp_cat >= 0 && ix->grp_mode && c.Pg_lo && ix->G > 0;
  if (grp) {
    f.q = q;
    f.D = ix->D;
    f.c0 = ix->iso_c;
    f.cent = ix->grp_c;
    f.G = ix->G;
    f.grp = ix->grp_par;
    f.F = ix->grp_F;
    f.Fc = ix->grp_Fc;
    f.sh = c.gsh;
    f.Plo = c.Pg_lo;
    f.Phi = c.Pg_hi;
    f.Pclo = grp_cat ? c.Pc_lo : nullptr;
    f.Pchi = grp_cat ? c.Pc_hi : nullptr;
  }
  HIPCHK(launch_internal_finish(f, s));
  if (grp) c.grp_done = grp_cat;
  return CWQ_OK;
}
}  // namespace

namespace cwq {
int run_internal(cwq_index* ix, Chunk& c, hipStream_t s, bool bf_lpf, const float* q,
                 int grp_cat) {
  float* BF = bf_lpf ? c.BF : nullptr;
  float* LPF = bf_lpf ? c.LPF : nullptr;
  if (ix->NI == 0) return CWQ_OK;
  const float dfull = (float)((double)ix->D * (double)logf(2.0f * (float)M_PI));
  if (ix->NI <= kWave && (size_t)ix->DP * 8 <= 65536) {   // a few internal nodes: lane = query, same arithmetic
    HIPCHK(launch_int_small(c.X, ix->int_A, ix->int_B, ix->ld_int, ix->NI, ix->DP, c.nq, c.S_int, ix->NI, s));
    return internal_prefixes(ix, c, s, BF, LPF, dfull, q, grp_cat);
  }
  ScanArgs a = base_args(ix, c);
  // raw sums need no top-k list: the hot (list width 16, two rows per lane) configuration
  const int kl = 16, tq = scan_tq(kl);
  a.ld = ix->ld_int;
  a.nrows = ix->NI;
  a.nrows_pad = (int)round_up(ix->NI, kWave);
  a.n_qblocks = n_qblocks_for(c.nq, kl);
  const int nslab = pick_nslab(ix, ix->NI, a.n_qblocks, kl);
  a.rows_per_slab = (int)round_up((a.nrows_pad + nslab - 1) / nslab, scan_rows_per_tile(kl));
  const int nslab2 = (a.nrows_pad + a.rows_per_slab - 1) / a.rows_per_slab;
  a.out = c.S_int;
  a.ldo = ix->NI;
  // CWQ_RAW_SPLIT=0: the scan kernel for one query too (A/B)
  if (c.nq == 1 && (size_t)(ix->DP / 16) * kWave * 4 <= 65536 && !env_off("CWQ_RAW_SPLIT"))
    HIPCHK(launch_raw_split(c.X, ix->int_A, ix->int_B, a, s));
  else
    HIPCHK(launch_scan(false, EPI_RAW, false, kl, c.X, ix->int_A, ix->int_B, a, nslab2, s));
  return internal_prefixes(ix, c, s, BF, LPF, dfull, q, grp_cat);
}

// Filter paths on hierarchical trees: bounded internal prefixes instead of the exact
// internal pass (CWQ_INT_BOUND=0 disables).  Anisotropic leaf rows need exact prefixes
// (the exact scan reads them), so such trees keep the exact pass.
bool use_int_bounds(const cwq_index* ix) {
  // group-centred rows need the exact prefixes (their group terms are folded into them)
  if (!ix->int_bounds || ix->NL_an > 0 || ix->grp_mode) return false;
  return !env_off("CWQ_INT_BOUND");
}

size_t int_bounds_bytes(const cwq_index* ix, int64_t nqf) {
  return ix->int_bounds ? (size_t)nqf * ix->DPB2 * 2 + (size_t)nqf * 16 + (size_t)nqf * 4 + 5 * 256 : 0;
}

// Internal nodes by bounds: c.P <- lower, c.S_int <- upper bounds of the path prefix of
// the internal nodes the Fast filter reads (int_path: the leaf parents and the root;
// otherwise every internal node), the root exact in both.  q: the caller's [nq][D] queries.
int run_internal_bounds(cwq_index* ix, Chunk& c, const float* q, int64_t nqf, Bump& b, hipStream_t s) {
  uint16_t* Xb2 = b.take<uint16_t>((size_t)nqf * ix->DPB2);
  float4* qinfo2 = b.take<float4>(nqf);
  float* Sroot = b.take<float>(nqf);
  int* tctr = b.take<int>(64);
  HIPCHK(launch_query_prep2(q, c.nq, ix->D, ix->iso_c, ix->DP, ix->DPB2, nqf, Xb2, qinfo2, s));
  HIPCHK(launch_int_small(c.X, ix->int_A, ix->int_B, ix->ld_int, 1, ix->DP, c.nq, Sroot, 1, s));   // root, exact
  FgArgs g;
  memset(&g, 0, sizeof(g));
  g.DPB = ix->DPB2;
  g.nq = c.nq;
  g.n_qt = (int)(nqf / kFgTile);
  fg_groups(g.n_qt, g.qgroups, g.rgroups);
  g.qinfo = qinfo2;
  g.order = fg_order();
  g.tctr = tctr;
  g.rf = ix->int_rf2;
  g.tf = ix->iso_tf;
  g.P = ix->dummy;
  g.ldP = 1;
  g.ldq = nqf;
  g.mode = 2;
  g.path_sum = ix->int_path ? 1 : 0;
  g.n_rt = (int)(ix->ld_i2 / kFgTile);
  g.lb = c.P;
  g.lb_hi = c.S_int;
  g.ldlb = std::max(ix->NI, 1);
  if (ix->int_path) {   // node-major lines of nq_pad queries (the chunk's [nq_pad][NI] space): dots
    g.pT = 1;
    g.lb_hi = nullptr;
    g.ldlb = c.nq_pad;
    c.pT = 1;
    c.ldP = c.nq_pad;
    c.qi2 = qinfo2;
  }
  g.Sroot = Sroot;
  g.root_w = ix->root_w;
  g.root_ld = ix->root_ld;
  g.row_id = ix->int_rowid;
  g.nrows = (int)ix->ld_i2;
  const int nqb = (c.nq + 15) / 16;
  if (ix->int_path && c.nq <= kStreamMaxQ && stream_lds_bytes(nqb, ix->DPB2) <= (size_t)kStreamMaxLds &&
      !env_set("CWQ_INT_STREAM_OFF")) {
    // a few queries (the per-call path): the path-sum rows streamed once against <= 64
    // queries (stream_kernel<2>) instead of 256-query MFMA tiles that are mostly padding;
    // the same dots and root lines
    StreamArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.DPB = ix->DPB2;
    sa.nq = c.nq;
    sa.nqb = nqb;
    sa.nrows = ix->ld_i2;
    sa.K = 1;
    sa.Xb = Xb2;
    sa.qinfo = qinfo2;
    sa.Mb = ix->int_Mb2;
    sa.rf = ix->int_rf2;
    sa.row_id = ix->int_rowid;
    sa.Sroot = Sroot;
    sa.root_w = ix->root_w;
    sa.root_ld = ix->root_ld;
    sa.pout = c.P;
    sa.ldpout = g.ldlb;
    const char* iwe = getenv("CWQ_INT_STREAM_WGS");   // workgroups per CU (A/B; read per call)
    HIPCHK(launch_stream(sa, 2, ix->cus * (iwe && atoi(iwe) > 0 ? std::min(4, atoi(iwe)) : 1), s));
  } else {
    HIPCHK(hipMemsetAsync(tctr, 0, 64 * 4, s));   // the tile claim counters (the stream pass has none)
    HIPCHK(launch_fgemm(Xb2, ix->int_Mb2, g, ix->cus, s));
  }
  if (!ix->int_path)
    for (size_t lv = 2; lv < ix->levels.size(); ++lv)
      HIPCHK(launch_prefix_bounds(c.P, c.S_int, std::max(ix->NI, 1), c.nq, ix->levels[lv].first,
                                  ix->levels[lv].second, ix->par_int, ix->w_int, ix->logdet_int, Sroot, s));
  return CWQ_OK;
}

IntChain int_chain(const cwq_index* ix) { return IntChain{ix->int_Ar, ix->int_Br, ix->par_int, ix->w_int, ix->logdet_int}; }

// Fast top-K over a small isotropic segment with many queries: the lane-per-query scan
// (scan_small_kernel).
bool small_scan_fits(const cwq_index* ix, int K) {   // size limits only (workspace sizing)
  return ix->NL_iso > 0 && ix->NL_iso <= kSmallScanMaxRows && K <= kSmallScanMaxK;
}
}  // namespace cwq

namespace {
bool use_small_scan(const cwq_index* ix, int64_t nq, int K) {
  if (!small_scan_fits(ix, K) || nq < kSmallScanMinQ) return false;
  const char* e = getenv("CWQ_SCAN_SMALL");   // 0: never, 1: whenever it applies
  if (e && *e) return atoi(e) != 0;
  // by wave counts: the row-sliced scan's slabs are >= 256 rows, so on a small corpus it
  // has few waves, each waiting on its scalar query loads; the lane-per-query scan wins
  // with ~0.9x as many waves, or with half as many once it fills the SIMDs
  // (measured crossover, profiles/r02_small_scan.log)
  const int nqb = n_qblocks_for(nq, 16);
  const int64_t nqb_real = (nq + scan_queries_per_block(16) - 1) / scan_queries_per_block(16);
  const int64_t rs_waves = (int64_t)pick_nslab(ix, ix->NL_iso, nqb) * nqb_real * kWavesPerWG;
  const int64_t small_waves = (nq + kWave - 1) / kWave * small_scan_slabs(nq, ix->NL_iso);
  return small_waves * 10 >= rs_waves * 9 || (small_waves * 2 >= rs_waves && small_waves >= 4 * (int64_t)ix->cus);
}
}  // namespace

namespace cwq {
// One scan over both leaf-row segments.
// seg_mask: bit 0 = isotropic segment, bit 1 = anisotropic; TOPK lists start at
// slab_off0 (slots before it are filled by the caller).
int run_leaf_scan(cwq_index* ix, const Chunk& c, int epi, bool cat, int kl, float dconst, float* out, int64_t ldo,
                  float* pkey, float* paux, int* prow, int K, int* nslab_total_out, hipStream_t s,
                  int seg_mask, int slab_off0, int max_lists) {
  if (c.pT && ((seg_mask & 1) ? ix->NL : ix->NL_an) > 0)   // the scans read query-major exact prefixes
    return fail(CWQ_ERR_ARG, "leaf scan after node-major prefix bounds (internal error)");
  const int tq = scan_tq(kl);
  const int nqb = n_qblocks_for(c.nq, kl);
  const bool small = epi == EPI_TOPK && !cat && (seg_mask & 1) && use_small_scan(ix, c.nq, K);
  struct Seg {
    bool iso;
    int n;
    int base;
    const float *A, *B;
    int64_t ld;
  } segs[2] = {{true, ix->NL_iso, 0, ix->iso_M, ix->iso_M, ix->ld_iso},
               {false, ix->NL_an, ix->NL_iso, ix->an_A, ix->an_B, ix->ld_an}};
  int ns[2], rps[2];
  for (int i = 0; i < 2; ++i) {
    ns[i] = 0;
    rps[i] = 0;
    if (!((seg_mask >> i) & 1)) segs[i].n = 0;
    if (segs[i].n == 0) continue;
    const int tile = scan_rows_per_tile(kl);
    const int npad = (int)round_up(segs[i].n, kWave);
    if (i == 0 && small) {
      ns[0] = small_scan_slabs(c.nq, segs[0].n);
      continue;
    }
    const int n = pick_nslab(ix, segs[i].n, nqb);
    rps[i] = (int)round_up((npad + n - 1) / n, tile);   // slabs hold whole tiles: no row scanned twice
    ns[i] = (npad + rps[i] - 1) / rps[i];
  }
  const int lps = scan_lists_per_slab(kl);
  const int nslab_total = slab_off0 + (small ? ns[0] : ns[0] * lps) + ns[1] * lps;
  if (nslab_total > max_lists)
    return fail(CWQ_ERR_ARG, "internal: partial-list buffer too small (" + std::to_string(nslab_total) +
                                 " lists needed, " + std::to_string(max_lists) + " allocated)");
  if (nslab_total_out) *nslab_total_out = nslab_total;
  int slab_off = slab_off0;
  for (int i = 0; i < 2; ++i) {
    if (segs[i].n == 0) continue;
    ScanArgs a = base_args(ix, c);
    // categorize keys min(BF[parent], lp) read the path BOTTLENECK (the Fast keys read the
    // path prefix P); with P here the key was min(prefix, lp), equal to the bottleneck
    // key only while the leaf's lp stays below its ancestors' (a near-duplicate query
    // broke the top-R list's order)
    if (cat) a.P = c.BF ? c.BF : ix->dummy;
    a.ld = segs[i].ld;
    a.nrows = segs[i].n;
    a.nrows_pad = (int)round_up(segs[i].n, kWave);
    a.rows_per_slab = rps[i];
    a.n_qblocks = nqb;
    a.seg_base = segs[i].base;
    a.meta = (c.meta ? c.meta : ix->row_meta) + segs[i].base;
    a.par = ix->row_par + segs[i].base;
    a.flags = ix->row_flags + segs[i].base;
    a.dconst = dconst;
    a.out = out;
    a.ldo = ldo;
    a.out_base = segs[i].base;
    a.pkey = pkey;
    a.paux = paux;
    a.prow = prow;
    a.nslab_total = nslab_total;
    a.slab_off = slab_off;
    a.K = K;
    if (i == 0 && small) {
      HIPCHK(launch_scan_small(c.X, segs[0].A, a, ns[0], s));
      slab_off += ns[0];
      continue;
    }
    HIPCHK(launch_scan(segs[i].iso, epi, cat, kl, c.X, segs[i].A, segs[i].B, a, ns[i], s));
    slab_off += ns[i] * lps;
  }
  return CWQ_OK;
}
}  // namespace cwq

namespace {
// Workspace for one chunk: X + internal arrays.
// Workspace of one chunk: X + the [nq][NI] internal arrays -- S_int and P always; BF and
// LPF (path bottleneck, full log_prob) only for categorize / log_prob (`full`).
size_t group_bytes_per_query(const cwq_index* ix) {
  return ix->grp_mode ? (size_t)ix->G * 16 + (size_t)4 * std::max(ix->NI, 1) * 4 + 5 * 256 + prune_bytes_per_query(ix) : 0;
}
}  // namespace

namespace cwq {
size_t chunk_bytes(const cwq_index* ix, int64_t nq_pad, bool full) {
  return (size_t)nq_pad * ix->DP * 4 + (full ? 4 : 2) * (size_t)nq_pad * std::max(ix->NI, 1) * 4 + 8 * 256 +
         (size_t)nq_pad * group_bytes_per_query(ix);
}

void carve_chunk(cwq_index* ix, Bump& b, Chunk& c, int nq, bool full) {
  c.nq = nq;
  c.nq_pad = round_up(nq, kQPad);
  c.X = b.take<float>((size_t)c.nq_pad * ix->DP);
  c.ldP = std::max(ix->NI, 1);
  c.pT = 0;
  if (ix->NI > 0) {
    const size_t n = (size_t)c.nq_pad * ix->NI;
    c.S_int = b.take<float>(n);
    c.P = b.take<float>(n);
    if (full) {
      c.BF = b.take<float>(n);
      c.LPF = b.take<float>(n);
    }
    if (ix->grp_mode) {
      c.gsh = b.take<double>((size_t)2 * c.nq_pad * ix->G);   // the shifts, then their error bounds
      c.Pg_lo = b.take<float>(n);
      c.Pg_hi = b.take<float>(n);
      c.Pc_lo = b.take<float>(n);
      c.Pc_hi = b.take<float>(n);
    }
  }
}

// Query-chunk size that keeps the per-chunk workspace within the budget (16 GiB by
// default -- 288 GB of HBM hold it beside the largest indexes; CWQ_WS_BUDGET_MB; at
// least 128 queries).
int64_t chunk_queries(const cwq_index* ix, int64_t nq, size_t per_query_extra, bool full) {
  const size_t per_q = (size_t)ix->DP * 4 + (full ? 4 : 2) * (size_t)std::max(ix->NI, 1) * 4 + per_query_extra +
                       group_bytes_per_query(ix);
  // budget: CWQ_WS_BUDGET_MB, else 40% of what the device has free (plus the workspace
  // already held), between 2 and 48 GiB -- one chunk for 10k queries over trees with
  // ~350k internal nodes (whose [lo, hi] prefix matrices alone are 28 GB), which beats two
  // chunks by 11% (balanced 4/9 tree, 1M x 768)
  // (hipMemGetInfo is a driver query of ~0.3 ms: once per handle, not per call)
  const char* e = getenv("CWQ_WS_BUDGET_MB");
  size_t budget = (size_t)16 << 30;
  if (e && atoll(e) > 0) {
    budget = (size_t)atoll(e) << 20;
  } else if (ix->ws_budget) {
    budget = ix->ws_budget;
  } else {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess)
      budget = std::min<size_t>((size_t)48 << 30, std::max<size_t>((size_t)2 << 30, (fr + ix->ws.size) / 5 * 2));
    const_cast<cwq_index*>(ix)->ws_budget = budget;
  }
  int64_t c = (int64_t)std::max<size_t>(kQPad, budget / std::max<size_t>(per_q, 1));
  c = std::max<int64_t>(kQPad, c / kQPad * kQPad);
  return std::min(nq, c);
}
}  // namespace cwq
