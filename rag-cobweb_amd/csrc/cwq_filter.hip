// The batch filter shared by Fast and Basic (host side): when it runs (use_filter, note_filter), its
// launch geometry and phases, the int8 panel and its schedules, and run_iso_filter -- sample pass,
// select, the filter launches over the row-tile phases.  Kernels: cwq_mfma.hip.
#include "cwq_handle.h"

namespace {
// Clustered (group-centred) trees: a query's whole cluster can pass -- categorize keys tie at
// the cluster node's lp for every row of the cluster (~1,000 rows at C2) -- so the record
// buffers hold 4x as many per query (48 KB instead of 12 KB per query).
inline int rec_per_q(const cwq_index* ix) { return ix->grp_mode ? 4 * kFgRecPerQ : kFgRecPerQ; }
inline int dir_per_q(const cwq_index* ix) { return ix->grp_mode ? 4 * kFgDirPerQ : kFgDirPerQ; }
}  // namespace

namespace cwq {
// min_rows: the automatic mode's threshold (the batch filter: kFiltMinRows; the per-call
// stream path pays no batch pipeline and wins from a few hundred rows on -- the exact
// scan's per-call cost on a 1.5k-row tree is its scalar query-slice latency chain, 0.3 ms)
// fast: a Fast call (score_topk), which the auto-mode record can turn off; categorize keeps
// its own rule (its per-call lists still pay on a tree whose Fast filter fails: 500k x 768
// Basic one query per call 4.0 ms with the filter, 8.3 ms without,
// profiles/r05_c500k_probe_v1.log / _v2.log)
bool use_filter(const cwq_index* ix, int k, int min_rows, bool fast) {
  if (k > kFiltMaxK || ix->NL_iso == 0 || !ix->iso_Mb) return false;
  int mode = ix->filter;
  if (mode < 0) {
    const char* e = getenv("CWQ_FILTER");
    if (e && *e) mode = atoi(e) ? 1 : 0;
  }
  if (mode < 0) return ix->NL_iso >= min_rows && !(fast && ix->filt_auto_off);
  return mode == 1;
}

// After a Fast call (cwq_last_stats' record): the auto-mode filter record of the index.  The
// exact-scan choice is not for good: after kFiltRetryCalls auto-mode Fast calls on the exact
// scan the record starts afresh and the filter is tried again (an early query mix that
// defeated the bounds costs speed for a while, never for the index's life).
constexpr int kFiltRetryCalls = 64;
void note_filter(cwq_index* ix) {
  if (ix->filter >= 0) return;
  if (ix->stats[2] == 0) {
    if (ix->filt_auto_off && ++ix->filt_off_calls >= kFiltRetryCalls) {
      ix->filt_auto_off = false;
      ix->filt_q = ix->filt_fb = 0;
      ix->filt_off_calls = 0;
    }
    return;
  }
  if (ix->stats[0] <= 0) return;
  ix->filt_q += ix->stats[0];
  ix->filt_fb += ix->stats[1];
  if (ix->filt_q >= 256 && ix->filt_fb * 10 >= ix->filt_q * 9) {
    ix->filt_auto_off = true;
    ix->filt_off_calls = 0;
  }
}
}  // namespace cwq

namespace {
// fgemm launch geometry: query groups over the 8 XCDs (each keeps its query panel in
// L2), row groups for the remaining factor.
int fg_phases() { return env_int("CWQ_FG_PHASES", 1); }

// filter phases over the row tiles: cut points at n_rt * f / 1024 for the fractions f in
// CWQ_FG_CUTS (comma separated, increasing, at most 4; default 32,96,256,512: five
// launches, the first over 1/32 of the tiles; in-process A/B vs 1/16,1/4: x1.02 per call)
int fg_phase_cuts(int n_rt, int* cuts) {
  if (n_rt < 16 || !fg_phases()) return 1;
  int f[4] = {32, 96, 256, 512}, nf = 4;
  if (const char* e = getenv("CWQ_FG_CUTS")) {
    nf = 0;
    for (const char* p = e; *p && nf < 4;) {
      const int v = atoi(p);
      if (v > 0 && v < 1024) f[nf++] = v;
      while (*p && *p != ',') ++p;
      if (*p == ',') ++p;
    }
  }
  int n = 1;
  for (int i = 0; i < nf; ++i) {
    const int c = std::max(cuts[n - 1] + 1, (int)((int64_t)n_rt * f[i] / 1024));
    if (c >= n_rt) break;
    cuts[n++] = c;
  }
  cuts[n] = n_rt;
  return n;
}
}  // namespace

namespace cwq {
int fg_order() { return env_int("CWQ_FG_ORDER", 2); }   // default: dynamic per-XCD tile claims (measured fastest)

// XCD split of the tiles: qg query groups x rg row groups (qg * rg = 8).  Default: all 8
// XCDs split the queries (each keeps its query panels in its L2 and streams every row
// panel); CWQ_FG_QG = 4 / 2 / 1 caps qg (row panels fetched by fewer XCDs, more query
// panels per XCD).
void fg_groups(int n_qt, int& qg, int& rg) {
  qg = n_qt >= 8 ? 8 : n_qt >= 4 ? 4 : n_qt >= 2 ? 2 : 1;
  if (const char* e = getenv("CWQ_FG_QG")) {
    const int v = atoi(e);
    if ((v == 1 || v == 2 || v == 4) && v < qg) qg = v;
  }
  rg = 8 / qg;
}
}  // namespace cwq

namespace {
// The stream filter's int8 row panel (half the bf16 panel's bytes per row; the per-call pass
// is HBM-bound).  Built once, from the fp32 rerank copy, when the device has room for it.
// Used when it pays: the pass saves ~half its HBM time, the wider int8 bounds cost the
// exact rerank ~9x the reranks per query (one workgroup per query).  Measured at D = 768
// (profiles/r03_i8_*): 1M rows nq = 1 341 -> 271 us, nq = 64 385 -> 347 us; 100k rows
// nq = 1 110 -> 126 us (a loss); so by default for an int8 panel of >= kI8MinBytes.
// CWQ_STREAM_I8=0 / 1: off / forced on (read per call, for in-process A/Bs).  The panel
// is built by cwq_index_create when the policy holds there; a call that forces it on an
// index created without it builds it then (A/B and test use only).
constexpr int64_t kI8MinBytes = (int64_t)384 << 20;
// The panel with its row and tile constants, whatever its size (the policies are the
// callers'): built once per index; false when it cannot be (no room, group-centred rows).
bool build_i8(cwq_index* ix, hipStream_t s) {
  if (ix->grp_mode) return false;   // the int8 rows are root-centred
  if (ix->i8_state) return ix->i8_state > 0;
  ix->i8_state = -1;
  if (ix->DPB % 64 || !ix->iso_Mf || !ix->iso_rf || !ix->iso_tf) return false;
  const size_t n_rt = (size_t)(ix->ld_f / kFgTile);
  const size_t need = (size_t)ix->ld_f * ix->DPB + (size_t)ix->ld_f * sizeof(RowF) + n_rt * sizeof(TileF);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < need + std::max<size_t>((size_t)4 << 30, tot / 20)) return false;
  if (ix->alloc(&ix->iso_Mq, (size_t)ix->ld_f * ix->DPB) || ix->alloc(&ix->iso_rf8, (size_t)ix->ld_f) ||
      ix->alloc(&ix->iso_tf8, n_rt))
    return false;
  if (launch_rows_i8(ix->iso_Mf, ix->DP, ix->D, ix->iso_c, ix->DPB, ix->ld_f, ix->iso_rf, ix->iso_Mq, ix->iso_rf8, s) !=
          hipSuccess ||
      launch_tiles_i8(ix->iso_tf, ix->iso_rf8, (int)n_rt, ix->iso_tf8, s) != hipSuccess)
    return false;
  // the direct schedule's sample panel: the sample rows of the int8 panel, gathered once (an
  // index without hub rows never runs that schedule; without room for it the index keeps the
  // bf16 sample pass)
  if (ix->n_hub > 0 && ix->samp_rows && ix->ld_s > 0 && !ix->iso_Sq) {
    int8_t* Sq = nullptr;
    float4* St = nullptr;
    if (!ix->alloc(&Sq, (size_t)ix->ld_s * ix->DPB) && !ix->alloc(&St, (size_t)ix->ld_s) &&
        launch_gather_i8_rows(ix->iso_Mq, ix->DPB, ix->samp_rows, ix->ld_s, ix->iso_rf, ix->iso_rf8, Sq, St, s) ==
            hipSuccess) {
      ix->iso_Sq = Sq;
      ix->iso_St = St;
    }
  }
  ix->i8_state = 1;
  return true;
}
}  // namespace

namespace cwq {
bool i8_size_rule(const cwq_index* ix) { return (int64_t)ix->NL_iso * ix->DPB >= kI8MinBytes; }
bool ensure_i8(cwq_index* ix, hipStream_t s) {
  const int e = env_int("CWQ_STREAM_I8", -1);
  if (e == 0 || ix->grp_mode) return false;
  if (e != 1 && !i8_size_rule(ix)) return false;
  return build_i8(ix, s);
}
}  // namespace cwq

namespace {
// The batch filter's int8 launches (fgemm_kernel<0, true, true, true>): the
// first filter phase that takes the int8 operands, nph for none.  By default the phases that
// start at or past a quarter of the row tiles, on an index that has its int8 panel: the bf16
// launches before them have raised T, so the wider int8 bounds pass few candidates
// (profiles/fgi8_model_c3.log).  The early schedule: an index that got its panel by the size
// rule when it was built and whose sample holds hub rows (build_filter) runs every launch on
// the int8 operands -- the hub rows put the sample threshold near the final one, so the first
// launch passes what the late ones do (profiles/hub_model_c3.log).  Row terms that say nothing
// about the keys (unit-norm rows around a zero mean) leave it at the strided sample's
// threshold: a call on the early schedule that ends above kFgCapQ / 4 candidates per query or
// re-runs a query sends the index back to the quarter rule (note_i8_early; until
// cwq_set_filter).  CWQ_FG_I8_EARLY (read per call; tests and A/Bs): 1: the early schedule on
// an index of any size (building the panel), 2: the direct schedule (below) likewise, 0: the
// quarter rule.
// CWQ_FG_I8 (read per call; tests and in-process A/Bs):
// negative: off; n >= 0: from phase n on, building the panel at any size.
// A launch then takes them only when it is raw (all-uniform, Fast key).
// The direct schedule (*direct): where the early schedule runs by the size rule --
// or on an index of any size under CWQ_FG_I8_EARLY=2 -- on a flat index (every row tile
// uniform) with its int8 sample panel, the sample pass ranks the sample rows on the int8
// operands, the thresholds are exact keys of the rows it picks, and no bf16 query panel is
// prepared (run_iso_filter).  CWQ_FG_I8_EARLY=1 keeps the early schedule as it was: bf16
// sample pass with certified-bound thresholds.  The same guard covers both.
int fg_i8_from(cwq_index* ix, const int* cuts, int nph, bool cat, bool ib, hipStream_t s, bool* direct) {
  *direct = false;
  if (cat || ib || ix->grp_mode || ix->DPB % 64) return nph;
  const char* e = getenv("CWQ_FG_I8");
  if (e && *e) {
    const int v = atoi(e);
    return v >= 0 && build_i8(ix, s) ? std::min(v, nph) : nph;
  }
  const int ev = env_int("CWQ_FG_I8_EARLY", -1);
  if ((ev < 0 ? ix->i8_by_size : ev > 0) && ix->n_hub > 0 && !ix->i8_early_off && build_i8(ix, s)) {
    ix->i8_early_ran = true;
    *direct = ev != 1 && ix->iso_Sq && ix->iso_St && fg_flat_tiles(ix);
    return 0;
  }
  if (ix->i8_state <= 0) return nph;
  for (int ph = 1; ph < nph; ++ph)   // (the first launch would run on the strided sample's threshold)
    if (cuts[ph] >= cuts[nph] / 4) return ph;
  return nph;
}
}  // namespace

namespace cwq {
// After a Fast call on the early schedule: its guard (fg_i8_from).
void note_i8_early(cwq_index* ix, int64_t nq, int64_t cand_sum, int64_t n_fallback) {
  if (ix->i8_early_ran && (n_fallback > 0 || cand_sum > nq * (kFgCapQ / 4))) ix->i8_early_off = true;
}

// Isotropic leaf rows through the batch bf16-MFMA filter (cwq_mfma.hip): sample pass ->
// select -> filter launches over row-tile phases (bucket / tighten between them).  The
// caller then runs final_kernel on the returned candidate lists (exact keys -> list
// slot 0).  cat: the categorize key min(BF[parent], lp) (cwq_categorize) instead of the
// Fast key; ib: bounded internal prefixes (c.P lower, c.S_int upper).
size_t iso_filter_bytes_per_query(const cwq_index* ix, int n_rt) {
  return (size_t)ix->DPB * 2 + 16 + (size_t)ix->DPB + 16 +   // (the int8 query and its info)
         (size_t)ix->ld_s * 4 + 64 * 8 + (size_t)kFgCapQ * 12 + 32 +
         (size_t)(rec_per_q(ix) + dir_per_q(ix)) * 16 + 64 + ((size_t)2 * ix->cus * kFgChunk * 16) / 256 +
         (ix->n_multi_tiles ? (size_t)n_rt * 8 : 0) + 4 + 64 * 4;
}

int run_iso_filter(cwq_index* ix, Chunk& c, const float* qsrc, int64_t nqf, int K, bool cat, bool ib, Bump& b,
                   IsoFilter& o, hipStream_t s) {
  const int nqc = c.nq;
  const int n_rt = (int)(ix->ld_f / kFgTile);
  const int n_rts = ix->ld_s / kFgTile;
  const FiltConsts fc = filt_consts(ix->DPB);
  const int n_qt = (int)(nqf / kFgTile);
  uint16_t* Xb = b.take<uint16_t>((size_t)nqf * ix->DPB);
  float4* qinfo = b.take<float4>(nqf);
  int8_t* Xq = b.take<int8_t>((size_t)nqf * ix->DPB);   // the int8 launches' query side
  float4* qinfo8 = b.take<float4>(nqf);
  float* lb = b.take<float>((size_t)nqf * ix->ld_s + 4096);
  float* tl = b.take<float>((size_t)nqf * 64);
  int* tr = b.take<int>((size_t)nqf * 64);
  // [qcnt | ok | n_exact | qover | tdone | gctr]: the host reads the first three with one
  // copy; one memset clears the block before the filter launches (tighten_kernel
  // clears gctr between them)
  int* qcnt = b.take<int>((size_t)5 * nqf + 64);
  int* okf = qcnt + nqf;
  int* nex = qcnt + 2 * nqf;
  int* qover = qcnt + 3 * nqf;
  int* tdone = qcnt + 4 * nqf;                       // tighten/final incremental state
  int* gctr = qcnt + 5 * nqf;
  float* tlk = b.take<float>((size_t)nqf * 64);
  int* crow = b.take<int>((size_t)nqf * kFgCapQ);
  float* cu = b.take<float>((size_t)nqf * kFgCapQ);
  float* cl = b.take<float>((size_t)nqf * kFgCapQ);
  // every workgroup holds one partly filled chunk at a time: keep room for two per workgroup
  const int64_t rec_cap = round_up(std::max<int64_t>((int64_t)nqf * rec_per_q(ix), (int64_t)2 * ix->cus * kFgChunk),
                                   kFgChunk);
  int4* rec = b.take<int4>((size_t)rec_cap);
  int* chunk_fill = b.take<int>((size_t)(rec_cap / kFgChunk));
  const int dir_cap = (int)std::min<int64_t>((int64_t)nqf * dir_per_q(ix), INT32_MAX / 2);
  int4* rec_dir = b.take<int4>((size_t)dir_cap);
  float2* pmm = (!cat && ix->n_multi_tiles) ? b.take<float2>((size_t)n_rt * nqf) : nullptr;
  const PathB pb = (!cat && ib) ? path_b(ix, c) : PathB{nullptr, 0, nullptr, nullptr};
  const bool grp = ix->grp_mode && c.Pg_lo;   // group-centred rows: the shifted prefix tables
  // the launch schedule (fg_phase_cuts, fg_i8_from), chosen before the query prep: nothing on
  // the direct schedule reads the bf16 query panel.  It keeps the phase cuts: one launch over
  // every row tile (CWQ_FG_PHASES=0) passes as few candidates at C3 but its fgemm time measured
  // 0.25 ms above the five launches' sum (DESIGN Appendix C.1)
  int cuts[6] = {0, n_rt, n_rt, n_rt, n_rt, n_rt};
  const int nph = fg_phase_cuts(n_rt, cuts);
  bool direct = false;
  const int i8_from = fg_i8_from(ix, cuts, nph, cat, ib, s, &direct);
  direct = direct && !cat && !ib && !grp && !pb.dot && !pmm;
  ix->direct_ran = direct;
  if (!direct) HIPCHK(launch_query_prep(qsrc, nqc, ix->D, ix->iso_c, ix->DPB, nqf, Xb, qinfo, s));
  if (pmm)   // multi-parent tiles: parent-prefix range per (tile, query) for the pretest
    HIPCHK(launch_tile_prange(grp ? c.Pg_lo : c.P, grp ? c.Pg_hi : ib ? c.S_int : nullptr, c.ldP, c.pT, nqc, ix->iso_tf,
                              n_rt, pmm, nqf, s, &pb));
  FgArgs g;
  memset(&g, 0, sizeof(g));
  g.DPB = ix->DPB;
  g.nq = nqc;
  g.n_qt = n_qt;
  fg_groups(n_qt, g.qgroups, g.rgroups);
  g.qinfo = qinfo;
  g.order = fg_order();
  g.dbg = env_int("CWQ_FG_DBG", 0);
  g.tctr = gctr + 8;
  g.rf = cat ? ix->cat_rf : ix->iso_rf;
  g.tf = cat ? ix->cat_tf : ix->iso_tf;
  g.cat = cat ? 1 : 0;
  g.pmm = pmm;
  g.ldq = nqf;
  g.P = cat ? (c.BF ? c.BF : ix->dummy) : (c.P ? c.P : ix->dummy);
  g.pb = pb;
  g.Phi = (!cat && ib && !pb.dot) ? c.S_int : nullptr;
  if (grp) {
    g.P = cat ? c.Pc_lo : c.Pg_lo;
    g.Phi = cat ? c.Pc_hi : c.Pg_hi;
    g.BFt = cat ? (c.BF ? c.BF : ix->dummy) : nullptr;
  }
  g.ldP = cat ? std::max(ix->NI, 1) : c.ldP;
  g.pT = cat ? 0 : c.pT;
  g.gamma = (float)fc.gamma;
  g.eps_n = (float)fc.eps_n;
  g.slack = (float)fc.slack;
  // 1. sample pass -> T[q] = K-th largest lower bound over the sample rows
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[4], s));
  g.mode = 1;
  if (g.order == 2) HIPCHK(hipMemsetAsync(g.tctr, 0, 32, s));
  g.n_rt = n_rts;
  g.nrows = ix->ld_s;
  g.rowmap = ix->samp_rows;
  // large samples: lower bounds reduced to maxima over groups of 4 rows in the
  // kernel (fgemm_kernel<1>); small ones keep one value per row so that K groups exist
  g.lb = lb;
  g.lbg = direct || (ix->n_samp >= 64 * K && !pb.dot) ? 4 : 1;   // path-sum bounds: per-row values (fgemm_kernel<1>)
  g.ldlb = ix->ld_s / g.lbg;
  bool i8_prepped = false;   // the int8 query side: once per chunk, before the first launch that reads it
  if (direct) {
    // approximate pass on the int8 operands (one ranking value and the row's place per group
    // of 4 sample rows), the K best groups, T[q] = the K-th largest exact key of their rows
    HIPCHK(launch_query_prep_i8(qsrc, nqc, ix->D, ix->iso_c, ix->DPB, nqf, Xq, qinfo8, s));
    i8_prepped = true;
    g.i8 = 1;
    g.qinfo8 = qinfo8;
    g.samp8 = ix->iso_St;
    HIPCHK(launch_fgemm(Xq, ix->iso_Sq, g, ix->cus, s));
    g.i8 = 0;
    HIPCHK(launch_select(lb, g.ldlb, nqc, (int)g.ldlb, K, tl, tr, s, true));
    HIPCHK(launch_sample_threshold(c.X, ix->iso_Mf, ix->DP, nqc, K, tl, tr, ix->samp_rows, ix->ld_s, ix->row_meta,
                                   ix->row_par, c.P ? c.P : ix->dummy, c.pT ? 1 : c.ldP, tl + (K - 1), 64, s));
  } else {
    HIPCHK(launch_fgemm(Xb, ix->iso_Sb, g, ix->cus, s));
    HIPCHK(launch_select(lb, g.ldlb, nqc, (int)g.ldlb, K, tl, tr, s));
  }
  // group pruning: the sample saw only the groups kept; its seed threshold is a floor
  if (!cat && c.Tseed) HIPCHK(launch_raise_threshold(tl + (K - 1), 64, c.Tseed, nqc, s));

  // 2. filter launches over row-tile phases (fg_phase_cuts: 1/32, 2/32, 5/32, 8/32,
  // 16/32 of the tiles); after each the candidates go to per-query lists and T[q] is
  // raised to the K-th largest candidate lower bound, so later phases emit fewer
  g.mode = 0;
  g.nrows = ix->NL_iso;
  g.rowmap = nullptr;
  g.T = tl + (K - 1);
  g.ldT = 64;
  g.rec = rec;
  g.rec_cap = rec_cap;
  g.gctr = gctr;
  g.chunk_fill = chunk_fill;
  g.qover = qover;
  g.rec_dir = rec_dir;
  g.dir_cap = dir_cap;
  HIPCHK(hipMemsetAsync(qcnt, 0, ((size_t)5 * nqf + 64) * 4, s));
  ix->n_fg_launch = nph;
  g.qinfo8 = qinfo8;
  g.rf8 = ix->iso_rf8;
  g.tf8 = ix->iso_tf8;
  for (int ph = 0; ph < nph; ++ph) {
    g.rt_off = cuts[ph];
    g.n_rt = cuts[ph + 1] - cuts[ph];
    const std::vector<int>& up = cat ? ix->cat_uni_prefix : ix->tile_uni_prefix;
    g.all_uniform = up[cuts[ph + 1]] - up[cuts[ph]] == g.n_rt && !env_set("CWQ_FG_NO_ALLUNI");
    // all-uniform Fast-key launches append raw records; the bucket pass evaluates their
    // bounds (the categorize tables keep the in-kernel bounds: their key is min'ed with
    // the bottleneck table per survivor)
    g.raw = g.all_uniform && !cat;
    g.i8 = g.raw && ph >= i8_from;   // (fg_i8_from)
    if (g.i8 && !i8_prepped) {
      HIPCHK(launch_query_prep_i8(qsrc, nqc, ix->D, ix->iso_c, ix->DPB, nqf, Xq, qinfo8, s));
      i8_prepped = true;
    }
    ix->n_fg_i8 += g.i8;
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[5], s));
    unsigned long long* stamp_d = nullptr;
    const char* stamp_f = ph == nph - 1 ? getenv("CWQ_FG_STAMP") : nullptr;   // diagnostic builds
    if (stamp_f) {
      HIPCHK(hipMalloc(&stamp_d, 1 << 20));
      HIPCHK(hipMemsetAsync(stamp_d, 0, 1 << 20, s));
    }
    g.stamp = stamp_d;
    if (g.i8) HIPCHK(launch_fgemm(Xq, ix->iso_Mq, g, ix->cus, s));
    else HIPCHK(launch_fgemm(Xb, ix->iso_Mb, g, ix->cus, s));
    if (stamp_f) {
      std::vector<unsigned long long> hs(1 << 17);
      HIPCHK(hipMemcpyAsync(hs.data(), stamp_d, 1 << 20, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipFree(stamp_d));
      g.stamp = nullptr;
      if (FILE* fo = fopen(stamp_f, "wb")) {
        fwrite(hs.data(), 8, hs.size(), fo);
        fclose(fo);
      }
    }
    if (ix->timing) {   // per-launch fgemm time (timing mode synchronises)
      float e = 0, e0 = 0;
      HIPCHK(hipEventRecord(ix->ev[6], s));
      HIPCHK(hipEventSynchronize(ix->ev[6]));
      HIPCHK(hipEventElapsedTime(&e, ix->ev[5], ix->ev[6]));
      ix->t_ms[6] += e;
      if (ph == 0) {
        HIPCHK(hipEventElapsedTime(&e0, ix->ev[4], ix->ev[5]));
        ix->t_ms[5] += e0;
      }
    }
    if (g.raw)   // before launch_tighten: the records are tested against this launch's T
      HIPCHK(launch_bucket_raw(g, kFgCapQ, qcnt, crow, cu, cl, s));
    else
      HIPCHK(launch_bucket(rec, gctr, chunk_fill, rec_cap, rec_dir, dir_cap, kFgCapQ, qcnt, qover, crow, cu, cl,
                           s));
    if (ph + 1 < nph)
      HIPCHK(launch_tighten(nqc, K, kFgCapQ, qcnt, qover, cl, tl + (K - 1), 64, tlk, tr, tdone, gctr, s));
  }
  o = IsoFilter{qcnt, okf, nex, qover, tdone, crow, tr, cu, cl, tl, tlk};
  return CWQ_OK;
}
}  // namespace cwq
