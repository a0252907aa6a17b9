// Basic (categorize), host side: the list paths, the two-level and lazy replays, the measured path
// choice, cwq_categorize and cwq_categorize_host.  Calls the chunk passes (cwq_chunk.hip), the batch
// filter (cwq_filter.hip) and the per-call path's helpers (cwq_topk.hip).
#include "cwq_handle.h"

namespace {
// Categorize's top-R row list for a few queries (nq <= kStreamMaxQ) through the per-call
// stream filter instead of the batch pipeline (sample pass, select, five fgemm launches with
// bucket / tighten): query prep, probe + fused select, one pass, final_wide_kernel with the
// categorize key -- the key min(BFk[parent], lp_full) bounded by the categorize RowF and
// min'ed with BFk in the kernels (cwq_stream.hip), exact keys and the list order of
// list_before<true> in final_wide.  BFk: the chunk's BF (list 1) or the second-level T2
// (the two-level replay's list 2).  The list goes to slot 0 of pkey/paux/prow (stride lstride),
// the per-query certified flags to okf (a query whose candidates overflow: 0).
// the probe's 16-row groups for a list of R and the per-row bound lines they fill
int64_t cat_n_probe(const cwq_index* ix, int R) {
  const int64_t ngroups = (ix->NL_iso + 15) / 16;
  return std::min<int64_t>(std::max<int64_t>((int64_t)3 * R * ngroups / 1024, (int64_t)8 * R), ngroups);
}
int64_t cat_ldlb(const cwq_index* ix, int R) { return round_up(cat_n_probe(ix, R) * 16 + 1, 1024) + 1024; }
size_t stream_cat_bytes(const cwq_index* ix, int nqc) {
  const int nq16 = (nqc + 15) / 16 * 16;
  const int64_t ldlb = cat_ldlb(ix, 64);
  return (size_t)nq16 * ix->DPB * 2 + (size_t)nq16 * 16 + (size_t)nqc * 4 + (size_t)(5 * nqc + 1) * 4 +
         (size_t)nqc * kFgCapQ * 12 + (size_t)nqc * 64 * 16 + (size_t)nqc * ldlb * 4 + 16 * 256 +
         (size_t)nqc * kFwSplitMax * 64 * 12 + 3 * 256;
}
bool stream_cat_ok(const cwq_index* ix, int nqc, int R) {
  return ix->iso_Mb && ix->NL_iso >= kStreamMinRows && nqc <= kStreamMaxQ && R <= kFiltMaxK &&
         stream_lds_bytes((nqc + 15) / 16, ix->DPB) <= (size_t)kStreamMaxLds && final_wide_rows(ix->DP, kFgCapQ) > 0 &&
         !env_set("CWQ_CAT_STREAM_OFF");
}
int stream_cat_list(cwq_index* ix, Chunk& c, const float* q, int nqc, int R, const float* BFk, float dfull, float* pkey,
                    float* paux, int* prow, int64_t lstride, int* okf, Bump& b, hipStream_t s) {
  const int nqb = (nqc + 15) / 16, nq16 = nqb * 16;
  const int capq = kFgCapQ;
  uint16_t* Xb = b.take<uint16_t>((size_t)nq16 * ix->DPB);
  float4* qinfo = b.take<float4>(nq16);
  float* T = b.take<float>(nqc);
  int* qcnt = b.take<int>((size_t)5 * nqc + 1);   // [qcnt | ok | n_exact | qover | done | select counter]
  int* nex = qcnt + 2 * nqc;
  int* qover = qcnt + 3 * nqc;
  int* done = qcnt + 4 * nqc;
  int* sel_ctr = qcnt + 5 * nqc;
  int* crow = b.take<int>((size_t)nqc * capq);
  float* cu = b.take<float>((size_t)nqc * capq);
  float* cl = b.take<float>((size_t)nqc * capq);
  float* lkb = b.take<float>((size_t)nqc * 64);
  int* lrb = b.take<int>((size_t)nqc * 64);
  const int64_t ldlb = cat_ldlb(ix, R);   // every probed row's bound (probe_rows)
  float* lb = b.take<float>((size_t)nqc * ldlb);
  float* tl = b.take<float>((size_t)nqc * 64);
  int* tr = b.take<int>((size_t)nqc * 64);
  // the rerank split over workgroups (categorize lists: ~1k candidates, most reranked --
  // their keys tie at the parents' bottlenecks); arrivals counted in the zeroed ok slot
  // (at most 8: the last workgroup's merge inserts the others' tie-heavy lists serially --
  // C2 list 2: 8 workgroups end at 33 us, 32 at 61 us, profiles/r05_basic_percall_stamps_radix_s{8,32}.log)
  const int fws = std::min(8, fw_split(ix, nqc, true));
  FwExpand fx{nullptr, nullptr, nullptr, nullptr, 0, nullptr, fws, b.take<float>((size_t)nqc * fws * 64),
              b.take<float>((size_t)nqc * fws * 64), b.take<int>((size_t)nqc * fws * 64), qcnt + nqc};
  // the counters (qcnt, qover, done, the fused select's) zeroed by the prep's block 0
  HIPCHK(launch_query_prep(q, nqc, ix->D, ix->iso_c, ix->DPB, nq16, Xb, qinfo, s, qcnt, (int)(5 * nqc + 1)));
  const FiltConsts fc = filt_consts(ix->DPB);
  StreamArgs a;
  memset(&a, 0, sizeof(a));
  a.DPB = ix->DPB;
  a.nq = nqc;
  a.nqb = nqb;
  a.nrows = ix->NL_iso;
  a.K = R;
  a.Xb = Xb;
  a.qinfo = qinfo;
  a.Mb = ix->iso_Mb;
  a.rf = ix->cat_rf;
  const bool grp = ix->grp_mode && c.Pc_lo;
  a.P = grp ? c.Pc_lo : (c.BF ? c.BF : ix->dummy);   // non-group rows: invL 0 (no prefix term)
  a.Phi = grp ? c.Pc_hi : nullptr;
  a.ldP = std::max(ix->NI, 1);
  a.pT = 0;
  a.BFk = BFk;
  a.ldBF = std::max(ix->NI, 1);
  a.eps_n = (float)fc.eps_n;
  a.slack = (float)fc.slack;
  a.T = T;
  a.qcnt = qcnt;
  a.qover = qover;
  a.capq = capq;
  a.crow = crow;
  a.cu = cu;
  a.cl = cl;
  const int64_t ngroups = (ix->NL_iso + 15) / 16;
  const int64_t n_probe = cat_n_probe(ix, R);
  a.probe_stride = std::max<int64_t>(1, ngroups / std::max<int64_t>(n_probe, 1));
  a.n_probe = std::min<int64_t>(n_probe, (ngroups + a.probe_stride - 1) / a.probe_stride);
  a.probe_rows = env_set("CWQ_CAT_PROBE_MAX") ? 0 : 1;   // 1: group maxima (A/B)
  a.lb = lb;
  a.ldlb = ldlb;
  a.T0 = tl;
  a.ldT0 = 64;
  a.sel_ctr = sel_ctr;
  a.sel_lk = tl;
  a.sel_lr = tr;
  HIPCHK(launch_stream(a, 1, (int)std::max<int64_t>(1, std::min<int64_t>(ix->cus, (a.n_probe + 7) / 8)), s));
  a.sel_ctr = nullptr;
  a.probe_rows = 0;
  HIPCHK(launch_stream(a, 0, stream_wgs(ix), s));
  HIPCHK(launch_final(c.X, ix->iso_Mf, ix->DP, nqc, R, capq, qcnt, qover, crow, cu, cl, T, 1, ix->row_meta, ix->row_par,
                      BFk ? BFk : ix->dummy, std::max(ix->NI, 1), 0, pkey, paux, prow, lstride, okf, nex, lkb, lrb,
                      done, nullptr, 1, dfull, s, fws > 1 ? &fx : nullptr));
  if (env_set("CWQ_CAT_DEBUG")) {   // diagnostics: per query candidates, overflow, threshold, certified
    std::vector<int> hc(nqc), ho(nqc), hk(nqc), hx(nqc);
    std::vector<float> ht(nqc), hl(64);
    HIPCHK(hipMemcpyAsync(hc.data(), qcnt, nqc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ho.data(), qover, nqc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hk.data(), okf, nqc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hx.data(), nex, nqc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ht.data(), T, nqc * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hl.data(), tl, 64 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < std::min(nqc, 4); ++i)
      fprintf(stderr, "[cat stream] q %d R %d cand %d over %d T %.6g ok %d exact %d probe T0 %.6g | tl[R-2..R] %.6g %.6g\n",
              i, R, hc[i], ho[i], ht[i], hk[i], hx[i], i == 0 ? hl[R - 1] : 0.f, i == 0 ? hl[R - 2] : 0.f,
              i == 0 && R < 64 ? hl[R] : 0.f);
  }
  return CWQ_OK;
}

constexpr int kCatCountRetry = 16;   // (cwq_index::cat_count_idle)
constexpr int kCatExplore = 32, kCatDenseMemory = 64;   // (cwq_index::cat_ema_*)
constexpr int kLzFanout = 1024;   // batches try the lazy path when no node has more children
constexpr int kl = 64;            // the scan's list width

// What a categorize_impl call fixes before its chunk loop, and what its chunks add up.
struct CatCall {
  cwq_index* ix;
  const float* q;
  int64_t nq;
  int k;
  int64_t max_nodes;
  int64_t* nodes;
  int32_t* n_found;
  int64_t* n_calls;
  hipStream_t s;
  float dfull;
  int R;           // list length
  bool complete;   // the list holds every leaf row
  int64_t cap_list, cap2, cap_dense;   // heap entries per query: list replay, two-level replay, DENSE
  bool filt;       // list 1 through the filter
  size_t filt_q;   // (its workspace bytes per query)
  int64_t cq;      // queries per chunk
  bool scat, small2;   // the two-level replay in place on the chunk: stream lists / exact-scan lists
  int pk;          // the policy slot: small call / batch
  bool measure, direct;
  std::vector<int64_t> fredo;   // queries the filter could not certify
  int64_t n_dense = 0;          // queries the list paths left to the DENSE re-run

  int n_slabs(int nqb) const {
    return filt ? 1 + (pick_nslab(ix, ix->NL_an, nqb) + 1) * scan_lists_per_slab(kl)
                : (pick_nslab(ix, ix->NL_iso, nqb) + pick_nslab(ix, ix->NL_an, nqb) + 2) * scan_lists_per_slab(kl);
  }
};

// The path of a call: the list paths, or straight to the exact lazy replay (a call of <= 64
// queries, or a batch; CWQ_CAT_DIRECT=0 / 1: never / always where it applies); the choice is
// measured (cwq_index::cat_ema_*).  top: not the filter-overflow re-run of a call.
void cat_policy_begin(CatCall& cc, bool top) {
  cwq_index* ix = cc.ix;
  const int cdv = env_int("CWQ_CAT_DIRECT", -1);
  const int pk = cc.pk = cc.nq <= 64 ? 0 : 1;
  const bool direct_ok = (pk == 1 || cc.nq <= cc.cq) && ix->NI > 0 && ix->DP <= 2048;
  cc.measure = direct_ok && cdv < 0 && top;
  cc.direct = false;
  if (!direct_ok) return;
  if (cdv >= 0) {
    cc.direct = cdv == 1;
  } else if (!top) {
    cc.direct = ix->cat_pref_direct[pk];
  } else {
    ++ix->cat_pol_calls[pk];
    const bool may = ix->cat_dense_seen > 0 || (pk == 1 && ix->max_fanout <= kLzFanout);
    if (!may) cc.direct = false;                                     // the lists resolve this tree
    else if (ix->cat_ema_list[pk] < 0.0) cc.direct = false;          // the lists first
    else if (ix->cat_ema_direct[pk] < 0.0) cc.direct = true;         // then one trial
    else cc.direct = (ix->cat_ema_direct[pk] < ix->cat_ema_list[pk]) != (ix->cat_pol_calls[pk] % kCatExplore == 0);
  }
}

// After the chunks (and the filter-overflow re-run): the path's per-query wall time, completed
// (the caller syncs after a small call anyway).  (cat_dense_seen is noted before that re-run;
// cat_count_idle and cat_two_spec chunk by chunk, where the next chunk reads them.)
int cat_policy_end(CatCall& cc, std::chrono::steady_clock::time_point t_call) {
  cwq_index* ix = cc.ix;
  if (!cc.measure) return CWQ_OK;
  HIPCHK(hipStreamSynchronize(cc.s));
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count() /
                    (double)cc.nq;
  const int pk = cc.pk;
  double& ema = cc.direct ? ix->cat_ema_direct[pk] : ix->cat_ema_list[pk];
  ema = ema < 0.0 ? us : 0.75 * ema + 0.25 * us;
  ix->cat_pref_direct[pk] = ix->cat_ema_direct[pk] >= 0.0 && ix->cat_ema_list[pk] >= 0.0 &&
                            ix->cat_ema_direct[pk] < ix->cat_ema_list[pk];
  return CWQ_OK;
}

// The replay arguments every path starts from: the call, the tree, the internal-node tables of
// the chunk c and the outputs of its nq queries.  The caller sets what differs: the lists (R),
// the heap, the status and its gates, the queries X (lazy replay) or the dense keys.
// DP, Mf, NL_iso, anA, anB, ld_an, meta and dconst are the lazy replay's operands: only
// launch_simulate_lazy / launch_simulate_lazy_runs and their kernels read or check them.
// launch_simulate, launch_cat_count and launch_simulate_two (whose sites left them zero before
// this builder) ignore them; a check on one of them added to those launchers would change that.
SimArgs sim_args(const CatCall& cc, const Chunk& c, int nq, int64_t* nodes, int* n_found, int64_t* n_calls) {
  const cwq_index* ix = cc.ix;
  SimArgs a;
  memset(&a, 0, sizeof(a));
  a.nq = nq;
  a.k = cc.k;
  a.max_nodes = cc.max_nodes;
  a.NI = ix->NI;
  a.NL = ix->NL;
  a.LPF = c.LPF ? c.LPF : ix->dummy;
  a.BF = c.BF ? c.BF : ix->dummy;
  a.ldI = std::max(ix->NI, 1);
  a.complete = cc.complete ? 1 : 0;
  a.int_child_begin = ix->int_child_begin;
  a.int_child_end = ix->int_child_end;
  a.int_nchild = ix->int_nchild;
  a.int_bfs = ix->int_bfs;
  a.int_has_sent = ix->int_has_sent;
  a.int_leaf_a0 = ix->int_leaf_a0;
  a.int_leaf_a1 = ix->int_leaf_a1;
  a.int_leaf_b0 = ix->int_leaf_b0;
  a.int_leaf_b1 = ix->int_leaf_b1;
  a.row_par = ix->row_par;
  a.row_bfs = ix->row_bfs;
  a.row_flags = ix->row_flags;
  a.par_int = ix->par_int;
  a.out_nodes = nodes;
  a.n_found = n_found;
  a.n_calls = n_calls;
  a.DP = ix->DP;
  a.Mf = ix->iso_Mf;
  a.NL_iso = ix->NL_iso;
  a.anA = ix->an_A;
  a.anB = ix->an_B;
  a.ld_an = ix->ld_an;
  a.meta = ix->row_meta;
  a.dconst = cc.dfull;
  return a;
}

// The three result arrays of a gathered sub-call back to the call's outputs
int scatter_results(const CatCall& cc, SubCall& g, const int64_t* nodes2, const int* found2, const int64_t* calls2) {
  int rc;
  if ((rc = g.scatter(nodes2, 2 * (int64_t)cc.k, cc.nodes)) || (rc = g.scatter(found2, 1, cc.n_found))) return rc;
  return cc.n_calls ? g.scatter(calls2, 2, cc.n_calls) : CWQ_OK;
}

// DENSE re-run of the queries `redo` (indices in the chunk at q0): the exact heap replay
// (exact by construction), results scattered into the outputs.  By default lazily
// (simulate_lazy_kernel: a popped node's leaf rows scored when their parent is popped);
// CWQ_CAT_LAZY=0: every leaf row materialised first by the exact scan.
int dense_rerun(CatCall& cc, int64_t q0, const std::vector<int>& redo) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int k = cc.k;
  int rc;
  ix->cat_tail_done = false;   // the re-run writes after the last flag gather
  const bool lazy = !env_off("CWQ_CAT_LAZY") && ix->DP <= 2048;
  const int64_t ldL = lazy ? 1 : std::max(ix->NL, 1);
  const int64_t cap_dense = cc.cap_dense;
  const size_t per_q = (size_t)ix->DP * 4 + 4 * (size_t)std::max(ix->NI, 1) * 4 + (size_t)ldL * 4 +
                       (size_t)cap_dense * 16 + 64 + (size_t)k * 8 + (size_t)ix->D * 4;
  const int64_t sub = std::max<int64_t>(1, std::min<int64_t>((int64_t)redo.size(), ((size_t)2 << 30) / per_q));
  for (size_t r0 = 0; r0 < redo.size(); r0 += sub) {
    const int ns = (int)std::min<int64_t>(sub, (int64_t)redo.size() - (int64_t)r0);
    const int64_t ns_pad = round_up(ns, kQPad);
    // per hard query: dense keys, heap, then status / nodes[k] / found / calls
    if ((rc = ix->reserve(chunk_bytes(ix, ns_pad) +
                          (size_t)ns_pad * ((size_t)ldL * 4 + cap_dense * 16 + 64 + (size_t)k * 8) + 16 * 256 +
                          (size_t)ns_pad * ix->D * 4)))
      return rc;
    Bump b2(ix->ws.p, ix->ws.size);
    Chunk c2;
    carve_chunk(ix, b2, c2, ns);
    float* qsub = b2.take<float>((size_t)ns * ix->D);
    float* dense = b2.take<float>((size_t)ns_pad * ldL);
    HeapEnt* heap2 = b2.take<HeapEnt>((size_t)ns_pad * cap_dense);
    int* status2 = b2.take<int>(ns_pad);
    int64_t* nodes2 = b2.take<int64_t>((size_t)ns_pad * k);
    int* found2 = b2.take<int>(ns_pad);
    int64_t* calls2 = b2.take<int64_t>(ns_pad);
    std::vector<int64_t> gq(ns);   // the hard queries' indices in the call
    for (int i = 0; i < ns; ++i) gq[i] = q0 + redo[r0 + i];
    SubCall g;
    if ((rc = ix->fb.reserve((size_t)ns * 8, ix->busy())) || (rc = g.open(gq, ix->fb.as<int64_t>(), s)) ||
        (rc = g.gather(cc.q, ix->D, qsub)))
      return rc;
    HIPCHK(launch_pad_queries(qsub, ns, ix->D, c2.X, c2.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c2, s))) return rc;
    if (!lazy && (rc = run_leaf_scan(ix, c2, EPI_KEY, true, 16, cc.dfull, dense, ix->NL, nullptr, nullptr, nullptr, 1,
                                     nullptr, s)))
      return rc;
    SimArgs sd = sim_args(cc, c2, ns, nodes2, found2, calls2);   // R 0; every hard query replays (status2 is fresh scratch)
    sd.dense_lpf = dense;
    sd.ldL = ldL;
    sd.heap = heap2;
    sd.heap_cap = cap_dense;
    sd.status = status2;
    if (lazy) {
      sd.X = c2.X;
      // the run-merge replay in LDS; a query that overflows its arena is re-run on the
      // global heap (status 1 gates it; the second kernel writes status 0)
      if (!env_off("CWQ_CAT_LAZY_RUNS")) {
        HIPCHK(launch_simulate_lazy_runs(sd, s));
        sd.pre_status = 1;
      }
      HIPCHK(launch_simulate_lazy(sd, s));
      ix->lazy_stats[1] += ns;
    } else {
      HIPCHK(launch_simulate(sd, s));
    }
    if ((rc = scatter_results(cc, g, nodes2, found2, calls2)) || (rc = g.close())) return rc;
  }
  return CWQ_OK;
}

// One chunk of a call in the workspace.
struct CatChunk {
  Bump b;
  int64_t q0 = 0;
  int nqc = 0;
  int64_t nq_pad = 0;
  int slabs = 0;
  Chunk c;
  const float* qc = nullptr;                                 // its queries
  float *pkey = nullptr, *paux = nullptr, *okey = nullptr, *oaux = nullptr;   // partial lists [slabs], list 1
  int *prow = nullptr, *orow = nullptr;
  int* status = nullptr;
  int64_t* nodes = nullptr;                                  // its outputs
  int* n_found = nullptr;
  int64_t* n_calls = nullptr;
};

// The chunk's queries straight through the exact lazy replay: every pushed entry scored when
// its parent is popped.
int direct_chunk(CatCall& cc, CatChunk& ch) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int nqc = ch.nqc;
  int rc;
  SimArgs sd = sim_args(cc, ch.c, nqc, ch.nodes, ch.n_found, ch.n_calls);
  sd.status = ch.status;
  sd.X = ch.c.X;
  ix->cat_tail_done = false;
  if (cc.pk == 0) {   // a few queries: the global-heap form queued behind for arena overflows
    sd.heap = ch.b.take<HeapEnt>((size_t)ch.nq_pad * cc.cap_dense);
    sd.heap_cap = cc.cap_dense;
    HIPCHK(launch_simulate_lazy_runs(sd, s));
    sd.pre_status = 1;
    HIPCHK(launch_simulate_lazy(sd, s));
    ix->stats[4] += nqc;
    ix->lazy_stats[0] += nqc;
    return CWQ_OK;
  }
  // a batch: the run-merge replays side by side; a query that overflows its arena goes
  // to the DENSE re-run (its heap memory only for those)
  HIPCHK(launch_simulate_lazy_runs(sd, s));
  std::vector<int> hst(nqc);
  HIPCHK(hipMemcpyAsync(hst.data(), ch.status, (size_t)nqc * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int> redo;
  for (int i = 0; i < nqc; ++i)
    if (hst[i]) redo.push_back(i);
  ix->stats[4] += nqc - (int64_t)redo.size();
  ix->lazy_stats[0] += nqc - (int64_t)redo.size();
  ix->stats[1] += (int64_t)redo.size();
  if (!redo.empty() && (rc = dense_rerun(cc, ch.q0, redo))) return rc;
  return CWQ_OK;
}

// List 1 of the chunk, the top-R leaf rows by the categorize key min(BF[parent], lp), into
// okey / oaux / orow.  okf_d: the filter's per-query list-certified flags (none: exact scan).
int first_list(CatCall& cc, CatChunk& ch, int** okf_d) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int R = cc.R, nqc = ch.nqc, slabs = ch.slabs;
  Chunk& c = ch.c;
  Bump& b = ch.b;
  int rc, nst = 0;
  *okf_d = nullptr;
  if (cc.filt && cc.scat) {
    // anisotropic rows: the exact scan into slots 1..; isotropic rows: the stream filter
    // with the categorize key -> exact keys in list slot 0
    if ((rc = run_leaf_scan(ix, c, EPI_TOPK, true, kl, cc.dfull, nullptr, 0, ch.pkey, ch.paux, ch.prow, R, &nst, s, 2, 1,
                            slabs)))
      return rc;
    *okf_d = b.take<int>((size_t)ch.nq_pad);
    // no anisotropic rows (nst == 1): the rerank writes list 1 itself, no merge launch
    if ((rc = nst == 1 ? stream_cat_list(ix, c, ch.qc, nqc, R, c.BF, cc.dfull, ch.okey, ch.oaux, ch.orow, R, *okf_d, b, s)
                       : stream_cat_list(ix, c, ch.qc, nqc, R, c.BF, cc.dfull, ch.pkey, ch.paux, ch.prow,
                                         (int64_t)nst * R, *okf_d, b, s)))
      return rc;
  } else if (cc.filt) {
    // isotropic rows: the filter with the categorize key -> exact keys in list slot 0;
    // anisotropic rows: the exact scan into slots 1..
    IsoFilter fo;
    if ((rc = run_iso_filter(ix, c, ch.qc, round_up(nqc, kFgTile), R, true, false, b, fo, s))) return rc;
    if ((rc = run_leaf_scan(ix, c, EPI_TOPK, true, kl, cc.dfull, nullptr, 0, ch.pkey, ch.paux, ch.prow, R, &nst, s, 2, 1,
                            slabs)))
      return rc;
    HIPCHK(launch_final(c.X, ix->iso_Mf, ix->DP, nqc, R, kFgCapQ, fo.qcnt, fo.qover, fo.crow, fo.cu, fo.cl,
                        fo.tl + (R - 1), 64, ix->row_meta, ix->row_par, c.BF ? c.BF : ix->dummy, std::max(ix->NI, 1), 0,
                        ch.pkey, ch.paux, ch.prow, (int64_t)nst * R, fo.okf, fo.nex, fo.tlk, fo.tr, fo.tdone, nullptr, 1,
                        cc.dfull, s));
    *okf_d = fo.okf;
  } else if ((rc = run_leaf_scan(ix, c, EPI_TOPK, true, kl, cc.dfull, nullptr, 0, ch.pkey, ch.paux, ch.prow, R, &nst, s, 3,
                                 0, slabs))) {
    return rc;
  }
  if (!(cc.filt && cc.scat && nst == 1))
    HIPCHK(launch_merge(ch.pkey, ch.paux, ch.prow, nqc, nst * R, R, ch.okey, ch.oaux, ch.orow, s, true));
  return CWQ_OK;
}

// Two-level replay (simulate_two_kernel, §4.7) of the queries of chunk c (qc) whose top-R list
// ended inside a tie: the second-level table T2 from list 1 (st.lkey), a second leaf scan keyed
// by it -- by the stream filter (stream: plus the anisotropic rows' exact scan) or the exact
// scan of every row -- the merge, and the replay on both lists.  st: the replay arguments with
// list 1 and the outputs; gate: queries with gate[q] == 0 are skipped (none: null).  Scratch
// from b; status2 / okf2: the replay's status and (stream) list 2's certified flags.
int two_level(const CatCall& cc, const Chunk& c, const float* qc, int slabs, bool stream, SimArgs st, const int* gate,
              Bump& b, int** status2, int** okf2) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int R = cc.R, nq = st.nq;
  const int64_t nq_pad = c.nq_pad;
  const size_t ldI = (size_t)std::max(ix->NI, 1);
  float* T2 = b.take<float>((size_t)nq_pad * ldI);
  float* pk2 = b.take<float>((size_t)nq_pad * slabs * R);
  float* pa2 = b.take<float>((size_t)nq_pad * slabs * R);
  int* pr2 = b.take<int>((size_t)nq_pad * slabs * R);
  float* l2k = b.take<float>((size_t)nq_pad * R);
  float* l2a = b.take<float>((size_t)nq_pad * R);
  int* l2r = b.take<int>((size_t)nq_pad * R);
  HeapEnt* heap2 = b.take<HeapEnt>((size_t)nq_pad * cc.cap2);
  *status2 = b.take<int>((size_t)nq_pad);
  *okf2 = stream ? b.take<int>((size_t)nq_pad) : nullptr;   // (the exact scan's lists are certified)
  HIPCHK(launch_cat_t2(c.BF, c.LPF, (int64_t)ldI, ix->NI, nq, ix->par_int, st.lkey, R, T2, s));
  Chunk c2t = c;
  c2t.BF = T2;   // the categorize key reads min(T2[parent], lp)
  int nst2 = 0;
  int rc;
  if (!stream) {   // both segments by the exact scan
    if ((rc = run_leaf_scan(ix, c2t, EPI_TOPK, true, kl, cc.dfull, nullptr, 0, pk2, pa2, pr2, R, &nst2, s, 3, 0, slabs)))
      return rc;
  } else {
    if ((rc = run_leaf_scan(ix, c2t, EPI_TOPK, true, kl, cc.dfull, nullptr, 0, pk2, pa2, pr2, R, &nst2, s, 2, 1, slabs)))
      return rc;
    if ((rc = nst2 == 1 ? stream_cat_list(ix, c2t, qc, nq, R, T2, cc.dfull, l2k, l2a, l2r, R, *okf2, b, s)
                        : stream_cat_list(ix, c2t, qc, nq, R, T2, cc.dfull, pk2, pa2, pr2, (int64_t)nst2 * R, *okf2, b,
                                          s)))
      return rc;
  }
  if (!(stream && nst2 == 1)) HIPCHK(launch_merge(pk2, pa2, pr2, nq, nst2 * R, R, l2k, l2a, l2r, s, true));
  st.pre_status = 0;
  st.lkey2 = l2k;
  st.laux2 = l2a;
  st.lrow2 = l2r;
  st.T2 = T2;
  st.heap = heap2;
  st.heap_cap = cc.cap2;
  st.status = *status2;
  st.gate = gate;
  HIPCHK(launch_simulate_two(st, s));
  return CWQ_OK;
}

// The two-level replay of the chunk's queries `redo` gathered into chunks of their own (list 1
// through the host, the internal pass recomputed); left: those it could not certify.
int two_level_gathered(CatCall& cc, CatChunk& ch, const std::vector<int>& redo, std::vector<int>& left) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int R = cc.R, k = cc.k, nqc = ch.nqc;
  const int64_t cap2 = cc.cap2;
  int rc;
  ix->cat_tail_done = false;   // the gathered replay writes after the flag gather
  std::vector<float> h1k((size_t)nqc * R), h1a((size_t)nqc * R);
  std::vector<int> h1r((size_t)nqc * R);
  HIPCHK(hipMemcpyAsync(h1k.data(), ch.okey, h1k.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h1a.data(), ch.oaux, h1a.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h1r.data(), ch.orow, h1r.size() * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const size_t per_q2 = chunk_bytes(ix, kQPad) / kQPad + (size_t)std::max(ix->NI, 1) * 4 + (size_t)cap2 * 16 +
                        (size_t)R * 12 * 2 + 64 + (size_t)k * 8 + (size_t)ix->D * 4 +
                        (size_t)R * 12 * (pick_nslab(ix, ix->NL_iso, 1) + pick_nslab(ix, ix->NL_an, 1) + 2) *
                            scan_lists_per_slab(kl);
  const int64_t sub2 = std::max<int64_t>(1, std::min<int64_t>((int64_t)redo.size(), ((size_t)2 << 30) / per_q2));
  for (size_t r0 = 0; r0 < redo.size(); r0 += sub2) {
    const int ns = (int)std::min<int64_t>(sub2, (int64_t)redo.size() - (int64_t)r0);
    const int64_t ns_pad = round_up(ns, kQPad);
    const int nqb2 = n_qblocks_for(ns, kl);
    const int slabs2 = (pick_nslab(ix, ix->NL_iso, nqb2) + pick_nslab(ix, ix->NL_an, nqb2) + 2) *
                       scan_lists_per_slab(kl);
    const size_t ldI = (size_t)std::max(ix->NI, 1);
    if ((rc = ix->reserve(chunk_bytes(ix, ns_pad) +
                          (size_t)ns_pad * (ldI * 4 + (size_t)slabs2 * R * 12 + (size_t)R * 24 + cap2 * 16 + 64 +
                                            (size_t)k * 8) +
                          (size_t)ns * ix->D * 4 + 24 * 256)))
      return rc;
    Bump b2(ix->ws.p, ix->ws.size);
    Chunk c2;
    carve_chunk(ix, b2, c2, ns);
    float* qsub = b2.take<float>((size_t)ns * ix->D);
    float* l1k = b2.take<float>((size_t)ns_pad * R);
    float* l1a = b2.take<float>((size_t)ns_pad * R);
    int* l1r = b2.take<int>((size_t)ns_pad * R);
    int64_t* nodes2 = b2.take<int64_t>((size_t)ns_pad * k);
    int* found2 = b2.take<int>(ns_pad);
    int64_t* calls2 = b2.take<int64_t>(ns_pad);
    std::vector<int64_t> gq(ns);
    std::vector<float> s1k((size_t)ns * R), s1a((size_t)ns * R);
    std::vector<int> s1r((size_t)ns * R);
    for (int i = 0; i < ns; ++i) {
      const int li = redo[r0 + i];
      gq[i] = ch.q0 + li;
      std::copy(h1k.begin() + (size_t)li * R, h1k.begin() + (size_t)(li + 1) * R, s1k.begin() + (size_t)i * R);
      std::copy(h1a.begin() + (size_t)li * R, h1a.begin() + (size_t)(li + 1) * R, s1a.begin() + (size_t)i * R);
      std::copy(h1r.begin() + (size_t)li * R, h1r.begin() + (size_t)(li + 1) * R, s1r.begin() + (size_t)i * R);
    }
    SubCall g;
    if ((rc = ix->fb.reserve((size_t)ns * 8, ix->busy())) || (rc = g.open(gq, ix->fb.as<int64_t>(), s))) return rc;
    HIPCHK(hipMemcpyAsync(l1k, s1k.data(), s1k.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(l1a, s1a.data(), s1a.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(l1r, s1r.data(), s1r.size() * 4, hipMemcpyHostToDevice, s));
    if ((rc = g.gather(cc.q, ix->D, qsub))) return rc;
    HIPCHK(launch_pad_queries(qsub, ns, ix->D, c2.X, c2.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c2, s))) return rc;
    SimArgs st = sim_args(cc, c2, ns, nodes2, found2, calls2);
    st.R = R;
    st.lkey = l1k;
    st.laux = l1a;
    st.lrow = l1r;
    int *status2 = nullptr, *okf2 = nullptr;
    if ((rc = two_level(cc, c2, qsub, slabs2, false, st, nullptr, b2, &status2, &okf2))) return rc;
    // every result goes back; the uncertified ones are overwritten by the DENSE re-run
    if ((rc = scatter_results(cc, g, nodes2, found2, calls2))) return rc;
    std::vector<int> hs(ns);
    HIPCHK(hipMemcpyAsync(hs.data(), status2, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
    if ((rc = g.close())) return rc;   // (the list sources are pageable host memory too)
    for (int i = 0; i < ns; ++i) {
      if (hs[i]) left.push_back(redo[r0 + i]);
      else ++ix->stats[5];
    }
  }
  return CWQ_OK;
}

// One chunk of the call: the queries [q0, q0 + cq).
int cat_chunk(CatCall& cc, int64_t q0) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int R = cc.R, k = cc.k;
  const bool filt = cc.filt, scat = cc.scat, small2 = cc.small2, direct = cc.direct;
  int rc;
  const int nqc = (int)std::min(cc.cq, cc.nq - q0);
  const int64_t nq_pad = round_up(nqc, kQPad);
  const int slabs = cc.n_slabs(n_qblocks_for(nqc, kl));
  const int64_t nqf = round_up(nqc, kFgTile);
  size_t need = chunk_bytes(ix, nq_pad) + (size_t)nq_pad * ((size_t)slabs * R * 12 + (size_t)R * 12 +
                                                            (size_t)cc.cap_list * 16 + 12) + 17 * 256 +
                (filt ? (size_t)nqf * cc.filt_q + 4096 * 8 : 0);
  if (direct && cc.pk == 0) need += (size_t)nq_pad * ((size_t)cc.cap_dense * 16 + 16) + 2 * 256;
  if (scat || small2)   // + the second list's stream pass, T2, lists and heap (the two-level replay in place)
    need += (scat ? 2 * stream_cat_bytes(ix, nqc) : 0) + (size_t)nq_pad * ((size_t)std::max(ix->NI, 1) * 4 + (size_t)slabs * R * 12 +
                                                               (size_t)R * 12 + (size_t)cc.cap2 * 16 + 16) + 32 * 256;
  if ((rc = ix->reserve(need))) return rc;
  CatChunk ch{Bump(ix->ws.p, ix->ws.size)};
  Bump& b = ch.b;
  Chunk& c = ch.c;
  ch.q0 = q0;
  ch.nqc = nqc;
  ch.nq_pad = nq_pad;
  ch.slabs = slabs;
  ch.qc = cc.q + q0 * ix->D;
  ch.nodes = cc.nodes + q0 * k;
  ch.n_found = cc.n_found + q0;
  ch.n_calls = cc.n_calls ? cc.n_calls + q0 : nullptr;
  carve_chunk(ix, b, c, nqc);
  ch.pkey = b.take<float>((size_t)nq_pad * slabs * R);
  ch.paux = b.take<float>((size_t)nq_pad * slabs * R);
  ch.prow = b.take<int>((size_t)nq_pad * slabs * R);
  ch.okey = b.take<float>((size_t)nq_pad * R);
  ch.oaux = b.take<float>((size_t)nq_pad * R);
  ch.orow = b.take<int>((size_t)nq_pad * R);
  HeapEnt* heap = b.take<HeapEnt>((size_t)nq_pad * cc.cap_list);
  int* status = ch.status = b.take<int>((size_t)nq_pad);
  HIPCHK(launch_pad_queries(ch.qc, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
  if ((rc = run_internal(ix, c, s, true, ch.qc, direct ? -1 : (filt ? 1 : -1)))) return rc;
  if (direct) return direct_chunk(cc, ch);
  if (filt && (rc = group_tables(ix, c, ch.qc, true, s))) return rc;
  int* okf_d = nullptr;   // filter: per-query list-certified flags
  if ((rc = first_list(cc, ch, &okf_d))) return rc;
  SimArgs sa = sim_args(cc, c, nqc, ch.nodes, ch.n_found, ch.n_calls);
  sa.R = R;
  sa.lkey = ch.okey;
  sa.laux = ch.oaux;
  sa.lrow = ch.orow;
  sa.heap = heap;
  sa.heap_cap = cc.cap_list;
  sa.status = status;
  // the pop sequence by counting over the bottleneck order (cat_count_kernel); the
  // queries it cannot certify go through the heap replay (CWQ_CAT_COUNT=0: replay all;
  // 2: always -- tests)
  const int ccv = env_int("CWQ_CAT_COUNT", 1);
  const bool by_count = ix->NI > 0 && !ix->any_int_sent && ccv != 0 &&
                        (ccv == 2 || ix->cat_count_idle < 8 || ix->cat_count_idle % kCatCountRetry == 0);
  if (by_count) {
    HIPCHK(launch_cat_count(sa, s));
    sa.pre_status = 1;
  }
  // the count pass's status, kept on the device for the one read-back below
  int* cst_d = by_count ? b.take<int>((size_t)nq_pad) : nullptr;
  if (by_count) HIPCHK(hipMemcpyAsync(cst_d, status, nqc * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (okf_d) {
    // queries whose filter lists overflowed have no list (every entry -inf, which the
    // replay would read as "every leaf listed" and search the whole tree for: 117 ms of a
    // 142 ms C2 batch for 4 such queries); they are re-run whole below, so skip them
    HIPCHK(launch_skip_failed(status, okf_d, nqc, by_count ? 0 : 1, s));
    sa.pre_status = 1;
  }
  HIPCHK(launch_simulate(sa, s));
  // The two-level replay (two_level) of the queries whose list ended inside a tie; what it
  // cannot certify goes to the DENSE re-run below.  On the chunk itself (scat / small2) its BF /
  // LPF, the group term tables and list 1 stay on the device and the results go straight into
  // the outputs, gated by the first replay's status (queries it resolved are skipped).
  const bool two = ix->NI > 0 && !ix->any_int_sent && !cc.complete && R == 64 && !env_off("CWQ_CAT_TWO");
  int *status2 = nullptr, *okf2 = nullptr;
  // speculative: the second list goes out with the first replay, one status read-back for
  // both (the last call needed it for every query; CWQ_CAT_SPEC=0 turns it off, =2 forces
  // it -- tests)
  const int spv = env_int("CWQ_CAT_SPEC", 1);
  const bool spec = two && (scat || small2) && spv != 0 && (ix->cat_two_spec || spv == 2);
  if (spec && (rc = two_level(cc, c, ch.qc, slabs, scat, sa, status, b, &status2, &okf2))) return rc;
  // the count status, the replay status, the filter's certified flags (and the second
  // list's) written by one kernel into host-mapped memory: one sync, no pageable copies
  if ((rc = ix->hflags.reserve((size_t)5 * nqc * sizeof(int)))) return rc;
  int* hf = ix->hflags.as<int>();
  HIPCHK(launch_gather_flags(hf, nqc, cst_d, status, okf_d, spec ? status2 : nullptr, spec ? okf2 : nullptr, s, ch.nodes,
                             ch.n_found, k));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int> cst(hf, hf + (by_count ? nqc : 0)), st(hf + nqc, hf + 2 * (size_t)nqc);
  std::vector<int> hs(spec ? hf + 3 * (size_t)nqc : hf, spec ? hf + 4 * (size_t)nqc : hf);
  std::vector<int> ho(spec ? hf + 4 * (size_t)nqc : hf, spec ? hf + 5 * (size_t)nqc : hf);
  std::vector<char> fbad(nqc, 0);
  if (okf_d)
    for (int i = 0; i < nqc; ++i)
      if (!hf[2 * (size_t)nqc + i]) {
        fbad[i] = 1;
        cc.fredo.push_back(q0 + i);
      }
  std::vector<int> redo;
  for (int i = 0; i < nqc; ++i)
    if (st[i] && !fbad[i]) redo.push_back(i);   // filter failures are re-run whole after the chunks
  int n_counted = 0;
  for (int i = 0; i < nqc; ++i) {
    if (by_count && cst[i] == 0 && !fbad[i]) ++ix->stats[3], ++n_counted;
    else if (!fbad[i]) ++ix->stats[4];
  }
  if (ccv != 0) ix->cat_count_idle = by_count && n_counted > 0 ? 0 : std::min(ix->cat_count_idle + 1, 1 << 30);
  if ((scat || small2) && two) ix->cat_two_spec = (int)redo.size() == nqc;
  if (redo.empty()) return CWQ_OK;

  if (spec || (two && ((scat && (int)redo.size() == nqc) || small2))) {
    if (!spec) {   // after the status read-back (gated: the first replay's resolved queries keep their results)
      if ((rc = two_level(cc, c, ch.qc, slabs, scat, sa, status, b, &status2, &okf2))) return rc;
      HIPCHK(launch_gather_flags(hf, nqc, status2, okf2, nullptr, nullptr, nullptr, s, ch.nodes, ch.n_found, k));
      HIPCHK(hipStreamSynchronize(s));
      hs.assign(hf, hf + nqc);
      ho.assign(hf + nqc, hf + 2 * (size_t)nqc);
    }
    std::vector<int> left;
    for (const int i : redo) {
      if (hs[i] || (okf2 && !ho[i])) left.push_back(i);   // uncertified, or list 2 overflowed: DENSE
      else ++ix->stats[5];
    }
    redo.swap(left);
  } else if (two) {
    std::vector<int> left;
    if ((rc = two_level_gathered(cc, ch, redo, left))) return rc;
    redo.swap(left);
  }
  ix->stats[1] += (int64_t)redo.size();
  cc.n_dense += (int64_t)redo.size();
  if (redo.empty()) return CWQ_OK;
  return dense_rerun(cc, q0, redo);
}

// Filter overflow: the queries cc.fredo through the exact path, results scattered back.
// again(queries, n, nodes, found, calls): categorize_impl on them without the filter.
template <class F>
int rerun_unfiltered(CatCall& cc, F again) {
  cwq_index* ix = cc.ix;
  hipStream_t s = cc.s;
  const int k = cc.k;
  const int64_t n = (int64_t)cc.fredo.size();
  const size_t D = (size_t)ix->D;
  const size_t o_q = round_up(n * 8, 256), o_nd = o_q + round_up(n * D * 4, 256),
               o_f = o_nd + round_up((int64_t)n * k * 8, 256), o_c = o_f + round_up(n * 4, 256),
               tot = o_c + round_up(n * 8, 256);
  int rc;
  if ((rc = ix->fb2.reserve(tot, ix->busy()))) return rc;
  char* f = ix->fb2.as<char>();
  float* qs = (float*)(f + o_q);
  int64_t* nd = (int64_t*)(f + o_nd);
  int* fd = (int*)(f + o_f);
  int64_t* cl = (int64_t*)(f + o_c);
  SubCall g;
  if ((rc = g.open(cc.fredo, (int64_t*)f, s)) || (rc = g.gather(cc.q, (int64_t)D, qs))) return rc;
  if ((rc = again(qs, n, nd, fd, cl))) return rc;
  if ((rc = scatter_results(cc, g, nd, fd, cl)) || (rc = g.close())) return rc;
  ix->cat_tail_done = false;
  return CWQ_OK;
}

// cwq_categorize body.  allow_filter: the isotropic leaf rows go through the bf16-MFMA
// filter with the categorize key (run_iso_filter, cat); queries whose candidate lists
// overflow are re-run with allow_filter = false (the exact scan of every leaf row).
int categorize_impl(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t max_nodes, int64_t* nodes,
                    int32_t* n_found, int64_t* n_calls, hipStream_t s, bool allow_filter) {
  CatCall cc{ix, q, nq, k, max_nodes, nodes, n_found, n_calls, s};
  cc.dfull = (float)((double)ix->D * (double)logf(2.0f * (float)M_PI));
  const int R = cc.R = std::max(1, std::min(64, ix->NL));
  cc.complete = ix->NL <= R;
  cc.cap_list = 1 + (int64_t)ix->NI + R;
  cc.cap2 = 1 + (int64_t)ix->NI + 2 * R;
  cc.cap_dense = 1 + (int64_t)ix->NI + ix->NL;
  // a call of a few queries takes the per-call stream lists from kStreamMinRows rows on (as
  // Fast does): the exact 64-wide list scan of a small tree is its latency chain -- qqp1k
  // (1,000 rows x 1,024): 285 us a list, profiles/r05_published_shapes_v4.log
  cc.filt = allow_filter && use_filter(ix, R, nq <= 64 ? kStreamMinRows : kFiltMinRows, false) &&
            !env_off("CWQ_CAT_FILTER");
  cc.filt_q = cc.filt ? iso_filter_bytes_per_query(ix, (int)(ix->ld_f / kFgTile)) : 0;
  const int max_slabs = cc.n_slabs(n_qblocks_for(nq, kl));
  cc.cq = chunk_queries(ix, nq, (size_t)cc.cap_list * 16 + (size_t)max_slabs * R * 12 + R * 12 + cc.filt_q);
  if (cc.filt && cc.cq < nq) cc.cq = std::max<int64_t>(kFgTile, cc.cq / kFgTile * kFgTile);   // whole query tiles
  // a few queries (the reference's one cobweb_predict per query): the lists through the
  // per-call stream filter (stream_cat_list), and a two-level replay of every query of the
  // call reuses the chunk's internal pass instead of gathering and recomputing it
  cc.scat = cc.filt && nq <= cc.cq && stream_cat_ok(ix, (int)nq, R);
  // a few queries without the filter (small trees): the two-level replay on the chunk too,
  // list 2 by the exact scan (instead of gathering the queries and re-running the internal
  // pass: qqp1k's Basic call 1.02 ms, profiles/r05_published_shapes_v3.log)
  cc.small2 = !cc.filt && nq <= std::min<int64_t>(cc.cq, 64);
  // every query resolved in the first chunk by the list paths: the flag gathers cleared the
  // node tails after the last results, so the caller needs no clear_tail launch / sync
  ix->cat_tail_done = nq <= cc.cq;
  cat_policy_begin(cc, allow_filter);
  const auto t_call = std::chrono::steady_clock::now();
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cc.cq)
    if ((rc = cat_chunk(cc, q0))) return rc;
  if (cc.measure && !cc.direct)
    ix->cat_dense_seen = cc.n_dense > 0 ? kCatDenseMemory : std::max(0, ix->cat_dense_seen - 1);
  ix->stats[2] += (int64_t)cc.fredo.size();
  auto again = [&](const float* qs, int64_t n, int64_t* nd, int* fd, int64_t* cl) {
    return categorize_impl(ix, qs, n, k, max_nodes, nd, fd, cl, s, false);
  };
  if (!cc.fredo.empty() && (rc = rerun_unfiltered(cc, again))) return rc;
  return cat_policy_end(cc, t_call);
}
}  // namespace

static int cat_args(const cwq_index* ix, const float* q, int64_t nq, int32_t k, const int64_t* nodes,
                    const int32_t* n_found) {
  if (!ix || (!q && nq > 0) || (nq > 0 && (!nodes || !n_found))) return fail(CWQ_ERR_ARG, "NULL argument");
  if (k <= 0) return fail(CWQ_ERR_ARG, "k must be >= 1");
  return CWQ_OK;
}
static void cat_reset(cwq_index* ix) {
  for (int64_t& t : ix->stats) t = 0;
  ix->lazy_stats[0] = ix->lazy_stats[1] = 0;
}

extern "C" int cwq_categorize(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t max_nodes, int64_t* nodes,
                              int32_t* n_found, int64_t* n_calls, void* stream) {
  if (int rc = cat_args(ix, q, nq, k, nodes, n_found)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  cat_reset(ix);
  if (call.rc) return call.rc;
  const int rc = categorize_impl(ix, q, nq, k, max_nodes, nodes, n_found, n_calls, s, true);
  ix->stats[0] = nq;
  if (rc) return rc;
  if (!ix->cat_tail_done) HIPCHK(launch_clear_tail(nodes, n_found, nq, k, s));
  return CWQ_OK;
}

// Basic in the harness's shape (benchmark_utils.py:580-581: cobweb_predict(numpy_query, k)):
// the query through pinned staging, the pop-order node ids / found counts / call counts
// written by the kernels straight into mapped host memory, the call returning synchronized.
extern "C" int cwq_categorize_host(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t max_nodes,
                                   int64_t* nodes, int32_t* n_found, int64_t* n_calls, void* stream) {
  if (int rc = cat_args(ix, q, nq, k, nodes, n_found)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  cat_reset(ix);
  if (call.rc) return call.rc;
  const size_t qb = (size_t)nq * ix->D * 4, nb = (size_t)round_up(nq * k * 8, 256), cb = (size_t)round_up(nq * 8, 256),
               fb = (size_t)nq * 4;
  int rc;
  if ((rc = stage_host(ix, q, qb, nb + cb + fb, s))) return rc;
  int64_t* hn = ix->hout.as<int64_t>();
  int64_t* hc = (int64_t*)(ix->hout.as<char>() + nb);
  int32_t* hf = (int32_t*)(ix->hout.as<char>() + nb + cb);
  rc = categorize_impl(ix, ix->dq.as<float>(), nq, k, max_nodes, hn, hf, hc, s, true);
  ix->stats[0] = nq;
  if (rc) return rc;
  if (!ix->cat_tail_done) {   // (otherwise categorize_impl's last sync already covers every write)
    HIPCHK(launch_clear_tail(hn, hf, nq, k, s));
    HIPCHK(sync_spin(s));
  }
  ix->ws_idle = true;   // synchronized
  memcpy(nodes, hn, (size_t)nq * k * 8);
  memcpy(n_found, hf, fb);
  if (n_calls) memcpy(n_calls, hc, (size_t)nq * 8);
  return CWQ_OK;
}
