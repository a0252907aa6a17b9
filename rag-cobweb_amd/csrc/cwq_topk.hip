// The Fast top-k calls (host side): the per-call stream path (stream_topk_impl), the batch path with
// its exact re-run (score_topk_impl, rerun_exact), cwq_score_topk and cwq_score_topk_host.
// Calls the chunk passes (cwq_chunk.hip) and the batch filter (cwq_filter.hip).
#include "cwq_handle.h"

namespace {
int score_topk_impl(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                    hipStream_t s, bool allow_filter);
}  // namespace

namespace cwq {
// Wait for a one-query call's kernels by polling the stream: a blocking
// hipStreamSynchronize issued ~0.3 ms before the work ends falls back to an interrupt
// wait, whose wake-up is a large share of the per-call path's fixed cost.  Polls for at
// most ~20 ms, then blocks.
hipError_t sync_spin(hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) return hipStreamSynchronize(s);
  }
}
}  // namespace cwq

namespace {
// Queries whose certificate failed: exact scan, results scattered back in place.
int rerun_exact(cwq_index* ix, const float* q, const std::vector<int64_t>& qi, int32_t k, int64_t* ids, float* scores,
                hipStream_t s) {
  // buffers from the handle's fallback region; one gather launch in, one scatter out
  const int64_t n = (int64_t)qi.size();
  const size_t D = (size_t)ix->D;
  const size_t o_tq = round_up(n * 8, 256), o_tid = o_tq + round_up(n * D * 4, 256),
               o_ts = o_tid + round_up((int64_t)n * k * 8, 256), tot = o_ts + round_up((int64_t)n * k * 4, 256);
  int rc = ix->fb.reserve(tot, ix->busy());
  if (rc) return rc;
  char* fb = ix->fb.as<char>();
  float* tq = (float*)(fb + o_tq);
  int64_t* tid = (int64_t*)(fb + o_tid);
  float* ts = scores ? (float*)(fb + o_ts) : nullptr;
  SubCall g;
  if ((rc = g.open(qi, (int64_t*)fb, s)) || (rc = g.gather(q, (int64_t)D, tq))) return rc;
  if ((rc = score_topk_impl(ix, tq, n, k, tid, ts, s, false))) return rc;
  if ((rc = g.scatter(tid, 2 * (int64_t)k, ids)) || (scores && (rc = g.scatter(ts, k, scores)))) return rc;
  return g.close();
}

// Small-batch path (cwq_stream.hip): nq <= kStreamMaxQ queries, isotropic rows through
// the stream filter (probe -> filter -> exact rerank), anisotropic rows through the exact
// scan; the reference harness's one-query-per-call mode.  false: not applicable.
bool use_stream(const cwq_index* ix, int64_t nq, int k) {
  if (nq > kStreamMaxQ || k > kFiltMaxK || !ix->iso_Mb) return false;
  if (stream_lds_bytes((int)((nq + 15) / 16), ix->DPB) > (size_t)kStreamMaxLds) return false;
  return !env_off("CWQ_STREAM");
}

// CWQ_SELECT_UNFUSED=1: the per-call path keeps select_kernel (and sb_prep) -- A/B only
bool sel_unfused() { return env_int("CWQ_SELECT_UNFUSED", 0) != 0; }
}  // namespace

namespace cwq {
// Workgroups of the per-call filter pass: one per CU (8 waves); CWQ_STREAM_WGS = m runs m
// per CU (more loads in flight on short passes -- an A/B knob).
int stream_wgs(const cwq_index* ix) {
  const char* e = getenv("CWQ_STREAM_WGS");   // read per call: in-process A/Bs switch it
  const int m = e && atoi(e) > 0 ? std::min(4, atoi(e)) : 1;
  return ix->cus * m;
}

// Workgroups per query of the per-call path's rerank tail (FwExpand::split): after the int8
// pass a query's ~1k-row candidate list reranked by one workgroup leaves the chip idle, so
// up to kFwSplitMax per query, about one per CU in total (C3 one query per call 267 -> 262
// us); the bf16 pass's lists are short and the split's merge costs more than it saves (C2:
// 142 -> 154 us, profiles/r05_c2_probe_envab_v1.log), so one there.  CWQ_FW_SPLIT = n caps it.
int fw_split(const cwq_index* ix, int nq, bool i8) {
  int S = i8 ? std::max(1, std::min(kFwSplitMax, ix->cus / std::max(nq, 1))) : 1;
  if (const char* e = getenv("CWQ_FW_SPLIT"))
    if (atoi(e) > 0) S = std::min(S, atoi(e));
  return S;
}
}  // namespace cwq

namespace {
int stream_topk_impl(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                     hipStream_t s) {
  const int K = k, kl = k <= 16 ? 16 : 64;
  const int nqc = (int)nq;
  const int nqb = (nqc + 15) / 16, nq16 = nqb * 16;
  const int64_t nq_pad = round_up(nqc, kQPad);
  const int nqb_scan = n_qblocks_for(nqc, kl);
  const int slabs = 1 + (pick_nslab(ix, ix->NL_an, nqb_scan) + 1) * scan_lists_per_slab(kl);
  const int capq = kFgCapQ;
  size_t need = chunk_bytes(ix, nq_pad, false) + 64 * 256 + (size_t)nq_pad * ((size_t)slabs * K * 12 + (size_t)K * 12) +
                (size_t)nq16 * ix->DPB * 2 + (size_t)nq16 * 16 + (size_t)64 * nqc * 4 + (size_t)nqc * 4 +
                (size_t)5 * nqc * 4 + (size_t)nqc * capq * 12 + (size_t)nqc * 64 * 16 +
                (size_t)nqc * 4 * (round_up((ix->NL_iso + 15) / 16 + 1, 1024) + 1024) + 32 * 256 +
                int_bounds_bytes(ix, kFgTile) + (size_t)nq16 * ix->DPB + (size_t)nq16 * 16 + 512 +
                (size_t)nqc * kFwSplitMax * 64 * 12 + 3 * 256 + (size_t)((ix->NL_iso + 15) / 16) * 4 + 256;
  const bool ib = use_int_bounds(ix);
  // int8 pass: flat trees, and hierarchical ones for calls of <= 8 queries.  With bounded
  // internal prefixes the ~9x exact reranks pay the exact parent chains too: round 3, b4/L9
  // one query per call 692 -> 1166 us (profiles/r03_i8_ab_hier_*.log); with the split rerank
  // tail and its radix T2 it pays at a few queries (nq 1 / 8: 670 -> 601 / 722 -> 664 us) and
  // not at 64 (1373 -> 3161 us), profiles/r05_percall_b4d9_i8_ab.log.  CWQ_STREAM_I8=1 / 0
  // forces it on / off.
  const int e8v = env_int("CWQ_STREAM_I8", -1);
  const bool i8 = e8v != 0 && (!ib || nqc <= 8 || e8v == 1) && ensure_i8(ix, s);
  int rc;
  if ((rc = ix->reserve(need))) return rc;
  Bump b(ix->ws.p, ix->ws.size);
  Chunk c;
  carve_chunk(ix, b, c, nqc, false);
  float* pkey = b.take<float>((size_t)nq_pad * slabs * K);
  float* paux = b.take<float>((size_t)nq_pad * slabs * K);
  int* prow = b.take<int>((size_t)nq_pad * slabs * K);
  uint16_t* Xb = b.take<uint16_t>((size_t)nq16 * ix->DPB);
  float4* qinfo = b.take<float4>(nq16);
  int8_t* Xq = i8 ? b.take<int8_t>((size_t)nq16 * ix->DPB) : nullptr;
  float4* qinfo8 = i8 ? b.take<float4>(nq16) : nullptr;
  int* Tb = b.take<int>((size_t)(K + 1) * nqc);   // [K][nq] blocks + [nq] live threshold
  float* T = b.take<float>(nqc);
  int* qcnt = b.take<int>((size_t)5 * nqc + 1);   // [qcnt | ok | n_exact | qover | done | select counter]
  int* okf = qcnt + nqc;
  int* nex = qcnt + 2 * nqc;
  int* qover = qcnt + 3 * nqc;
  int* done = qcnt + 4 * nqc;
  int* sel_ctr = qcnt + 5 * nqc;
  int* crow = b.take<int>((size_t)nqc * capq);
  float* cu = b.take<float>((size_t)nqc * capq);
  float* cl = b.take<float>((size_t)nqc * capq);
  float* lkb = b.take<float>((size_t)nqc * 64);
  int* lrb = b.take<int>((size_t)nqc * 64);
  const int64_t ldlb = round_up((ix->NL_iso + 15) / 16 + 1, 1024) + 1024;   // select reads whole 1024 steps
  float* lb = b.take<float>((size_t)nqc * ldlb);
  float* tl = b.take<float>((size_t)nqc * 64);
  int* tr = b.take<int>((size_t)nqc * 64);
  const int fws = fw_split(ix, nqc, i8);
  float* fsk = b.take<float>((size_t)nqc * fws * 64);
  float* fsa = b.take<float>((size_t)nqc * fws * 64);
  int* fsr = b.take<int>((size_t)nqc * fws * 64);
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[0], s));
  // one fused prep launch when the exact internal pass is small (flat trees: the root)
  bool fused = !ib && ix->NI <= kSbMaxNI && (int)ix->levels.size() <= kSbMaxNI &&
               ((size_t)2 * std::max(ix->DP, ix->DPB) + (size_t)ix->NI * (ix->DP / 16) + ix->NI) * 4 <= 65536 &&
               !env_set("CWQ_SB_UNFUSED");
  SbPrepArgs sp;
  const bool prn = !ib && use_prune(ix);
  int* live = nullptr;   // group pruning: the filter's 16-row blocks
  if (prn) fused = false;
  if (fused) {
    memset(&sp, 0, sizeof(sp));
    sp.q = q;
    sp.nq = nqc;
    sp.D = ix->D;
    sp.DP = ix->DP;
    sp.DPB = ix->DPB;
    sp.nq_pad = c.nq_pad;
    sp.nq16 = nq16;
    sp.X = c.X;
    sp.Xb = Xb;
    sp.qinfo = qinfo;
    sp.Xq = Xq;
    sp.qinfo8 = qinfo8;
    sp.c = ix->iso_c;
    sp.A = ix->int_A;
    sp.B = ix->int_B;
    sp.ld = ix->ld_int;
    sp.NI = ix->NI;
    sp.par_int = ix->par_int;
    sp.w_int = ix->w_int;
    sp.logdet_int = ix->logdet_int;
    sp.P = c.P;
    sp.ldP = std::max(ix->NI, 1);
    sp.qcnt = qcnt;
    sp.nlev = (int)ix->levels.size();
    for (int l = 0; l < sp.nlev && fused; ++l) {
      sp.lv0[l] = ix->levels[l].first;
      if (l > 0 && ix->levels[l].first != ix->levels[l - 1].second) fused = false;   // BFS: contiguous levels
    }
    if (sp.nlev > 0) sp.lv0[sp.nlev] = ix->levels.back().second;
    if (ix->NI > 0 && (!c.P || sp.nlev == 0 || sp.lv0[0] != 0 || sp.lv0[sp.nlev] != ix->NI)) fused = false;
  }
  // flat trees, up to 16 queries, bf16 pass: the prep inside the probe launch (stream_kernel<1>
  // with fprep) -- one launch less, but measured slower (C2 one query per call 101.5 ->
  // 104.9 us: the probe's workgroups all wait for the prep, profiles/r04_percall_ab_c2_v1.log),
  // so opt-in: CWQ_PROBE_PREP=1
  const bool fprep = fused && ix->NI == 1 && nqb == 1 && !i8 && ix->DP <= 1024 && !sel_unfused() &&
                     env_int("CWQ_PROBE_PREP", 0) == 1;
  if (fprep && !ix->sel_ctr)   // the fused select's counter (lives across calls)
    if ((rc = ix->alloc(&ix->sel_ctr, 1))) return rc;
  if (fprep) {
    // re-zeroed on every such call: its last workgroup resets it too, but an aborted launch
    // or one with another grid size would leave it nonzero and later calls would read stale
    // thresholds (this opt-in path only; the default path's counter is zeroed by the prep)
    HIPCHK(hipMemsetAsync(ix->sel_ctr, 0, 4, s));
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[1], s));
  } else if (fused) {
    HIPCHK(launch_sb_prep(sp, s));
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[1], s));
  } else {
    HIPCHK(launch_pad_queries(q, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if (ib) {
      if ((rc = run_internal_bounds(ix, c, q, kFgTile, b, s))) return rc;
    } else if (prn) {
      // the seed threshold goes straight to the filter's T0: no probe pass; the filter pass
      // covers the live blocks only
      live = b.take<int>((size_t)std::max<int64_t>(1, (ix->NL_iso + 15) / 16));
      if ((rc = prune_internal(ix, c, q, K, b, s, tl + (K - 1), 64, live))) return rc;
    } else if ((rc = run_internal(ix, c, s, false, q, 0))) {
      return rc;
    }
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[1], s));
    // the counters (qcnt, qover, done, ..., the fused select's) zeroed by the prep's block 0
    HIPCHK(launch_query_prep(q, nqc, ix->D, ix->iso_c, ix->DPB, nq16, Xb, qinfo, s, qcnt, (int)(5 * nqc + 1)));
    if (i8) HIPCHK(launch_query_prep_i8(q, nqc, ix->D, ix->iso_c, ix->DPB, nq16, Xq, qinfo8, s));
  }
  if ((rc = group_tables(ix, c, q, false, s))) return rc;
  const FiltConsts fc = filt_consts(ix->DPB);
  StreamArgs a;
  memset(&a, 0, sizeof(a));
  a.DPB = ix->DPB;
  a.nq = nqc;
  a.nqb = nqb;
  a.nrows = ix->NL_iso;
  a.K = K;
  a.Xb = Xb;
  a.qinfo = qinfo;
  a.Mb = ix->iso_Mb;
  a.rf = ix->iso_rf;
  a.P = c.P ? c.P : ix->dummy;
  a.pb = ib ? path_b(ix, c) : PathB{nullptr, 0, nullptr, nullptr};
  a.Phi = ib && !a.pb.dot ? c.S_int : nullptr;
  if (ix->grp_mode && c.Pg_lo) {   // group-centred rows: the shifted prefix tables
    a.P = c.Pg_lo;
    a.Phi = c.Pg_hi;
  }
  a.ldP = c.ldP;
  a.pT = c.pT;
  a.eps_n = (float)fc.eps_n;
  a.slack = (float)fc.slack;
  a.Tb = Tb;
  a.Tlive = Tb + (size_t)K * nqc;
  // live threshold (CWQ_STREAM_LIVE=n: refresh every n groups): measured slower at C3 --
  // the publishing atomics cost more than the ~3x fewer candidates save -- so off
  a.live_every = 0;
  if (const char* e = getenv("CWQ_STREAM_LIVE")) a.live_every = std::max(0, atoi(e));
  if (a.live_every > 0) HIPCHK(launch_stream_init(Tb, (K + 1) * nqc, s));   // only the live threshold reads Tb
  a.T = T;
  a.qcnt = qcnt;
  a.qover = qover;
  a.capq = capq;
  a.crow = crow;
  a.cu = cu;
  a.cl = cl;
  // probe: ~3*K*rows/1024 rows (a 16-row group per probe_stride groups), so that the
  // K-th largest probe bound leaves ~1k candidates per query before the live threshold
  // takes over; CWQ_STREAM_PROBE_DIV overrides (groups / div)
  const int64_t ngroups = (ix->NL_iso + 15) / 16;
  int64_t n_probe = std::max<int64_t>((int64_t)3 * K * ngroups / 1024, (int64_t)8 * K);
  if (const char* e = getenv("CWQ_STREAM_PROBE_DIV"))
    if (atoi(e) > 0) n_probe = std::max<int64_t>(ngroups / atoi(e), (int64_t)K);
  n_probe = std::min(n_probe, ngroups);
  a.probe_stride = std::max<int64_t>(1, ngroups / std::max<int64_t>(n_probe, 1));
  a.n_probe = std::min<int64_t>(n_probe, (ngroups + a.probe_stride - 1) / a.probe_stride);
  a.lb = lb;
  a.ldlb = ldlb;
  a.T0 = tl;
  a.ldT0 = 64;
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[4], s));
  const bool use_live = live && !env_off("CWQ_PRUNE_LIVE");   // 0: the pass over every block (A/B)
  // the select runs in the probe launch's last workgroup (one launch less per call);
  // CWQ_SELECT_UNFUSED=1 keeps select_kernel (same thresholds: both run select_wave)
  const bool fsel = !sel_unfused();
  if (fsel) {
    a.sel_ctr = fprep ? ix->sel_ctr : sel_ctr;
    a.sel_lk = tl;
    a.sel_lr = tr;
    a.sel_floor = c.Tseed;   // group pruning: the probe saw only the groups kept
  }
  if (fprep) {
    a.fprep = 1;
    a.fq = q;
    a.fc = ix->iso_c;
    a.fD = ix->D;
    a.fDP = ix->DP;
    a.f_nq_pad = c.nq_pad;
    a.fX = c.X;
    a.fA = ix->int_A;
    a.fB = ix->int_B;
    a.fld = ix->ld_int;
    a.fw0 = ix->root_w0;
    a.flogdet0 = ix->root_logdet0;
    a.fP = c.P;
    a.fldP = std::max(ix->NI, 1);
    a.fqcnt = qcnt;
  }
  // group pruning: the seed threshold (exact keys of the best group's sample rows) is T0 --
  // the probe would only see the groups kept, so it is skipped
  if (!prn) HIPCHK(launch_stream(a, 1, (int)std::max<int64_t>(1, std::min<int64_t>(ix->cus, (a.n_probe + 7) / 8)), s));
  a.sel_ctr = nullptr;
  a.sel_floor = nullptr;
  a.fprep = 0;
  if (!fsel && !prn) {
    HIPCHK(launch_select(lb, ldlb, nqc, (int)a.n_probe, K, tl, tr, s));
    if (c.Tseed) HIPCHK(launch_raise_threshold(tl + (K - 1), 64, c.Tseed, nqc, s));
  }
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[5], s));
  if (i8) {   // the filter pass over the int8 panel (the probe above: bf16, a tighter T0)
    StreamArgs a8 = a;
    a8.i8 = 1;
    a8.Xb = reinterpret_cast<const uint16_t*>(Xq);
    a8.qinfo = qinfo8;
    a8.Mb = reinterpret_cast<const uint16_t*>(ix->iso_Mq);
    a8.rf = ix->iso_rf8;
    HIPCHK(launch_stream(a8, 0, stream_wgs(ix), s));
  } else {
    StreamArgs a0 = a;
    if (use_live) {
      a0.live = live;
      a0.live_n = ix->prune_ctr + 5;
    }
    HIPCHK(launch_stream(a0, 0, stream_wgs(ix), s));
  }
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[6], s));
  int nst = 0;
  if ((rc = run_leaf_scan(ix, c, EPI_TOPK, false, kl, 0.f, nullptr, 0, pkey, paux, prow, K, &nst, s, 2, 1, slabs)))
    return rc;
  const IntChain chain = int_chain(ix);
  if ((rc = ix->hflags.reserve((size_t)3 * nqc * sizeof(int)))) return rc;
  int* hflags = ix->hflags.as<int>();
  // one candidate list per query (no anisotropic rows): final_wide expands the top-K to
  // sentence ids and writes the host flags itself (no merge launch, no flag copy)
  const bool ftail = nst == 1 && final_wide_rows(ix->DP, capq) > 0 && !env_set("CWQ_FW_UNFUSED");
  // okf / nex: the split tail's arrival count and exact-rerank sum (zeroed with the counters;
  // the fused tail reports through hflags, not these)
  const FwExpand fx{ix->sent_ptr, ix->sent_ids, ids, scores, k, hflags, fws, fsk, fsa, fsr};
  HIPCHK(launch_final(c.X, ix->iso_Mf, ix->DP, nqc, K, capq, qcnt, qover, crow, cu, cl, T, 1, ix->row_meta,
                      ix->row_par, c.P ? c.P : ix->dummy, c.pT ? 1 : c.ldP, 0, pkey, paux, prow, (int64_t)nst * K, okf,
                      nex, lkb, lrb, done, ib ? &chain : nullptr, 0, 0.f, s, ftail ? &fx : nullptr));
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[7], s));
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[2], s));
  if (!ftail) {
    HIPCHK(launch_merge_expand(pkey, paux, prow, nqc, nst * K, K, k, ix->sent_ptr, ix->sent_ids, ids, scores, s));
    HIPCHK(hipMemcpyAsync(hflags, qcnt, (size_t)3 * nqc * 4, hipMemcpyDeviceToHost, s));
  }
  if (ix->timing) HIPCHK(hipEventRecord(ix->ev[3], s));
  HIPCHK(sync_spin(s));
  std::vector<int64_t> redo;
  int64_t cand_sum = 0, exact_sum = 0;
  for (int i = 0; i < nqc; ++i) {
    if (!hflags[nqc + i]) redo.push_back(i);
    cand_sum += hflags[i];
    exact_sum += hflags[2 * nqc + i];
  }
  if (ix->timing) {
    float e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipEventElapsedTime(&e[0], ix->ev[1], ix->ev[2]));
    HIPCHK(hipEventElapsedTime(&e[1], ix->ev[0], ix->ev[1]));
    HIPCHK(hipEventElapsedTime(&e[2], ix->ev[2], ix->ev[3]));
    HIPCHK(hipEventElapsedTime(&e[3], ix->ev[0], ix->ev[3]));
    HIPCHK(hipEventElapsedTime(&e[5], ix->ev[4], ix->ev[5]));
    HIPCHK(hipEventElapsedTime(&e[6], ix->ev[5], ix->ev[6]));
    HIPCHK(hipEventElapsedTime(&e[7], ix->ev[6], ix->ev[7]));
    for (int i = 0; i < 8; ++i) ix->t_ms[i] += e[i];
    ix->t_ms[4] += 1;   // one filter launch
  }
  if (!redo.empty() && (rc = rerun_exact(ix, q, redo, k, ids, scores, s))) return rc;
  ix->ws_idle = true;   // synchronized above (rerun_exact synchronizes too): no end event
  ix->stats[0] = nq;
  ix->stats[1] = (int64_t)redo.size();
  ix->stats[2] = 2 + (i8 ? 256 : 0);   // the stream filter (+256: its int8 pass)
  ix->stats[3] = (cand_sum + nq / 2) / nq;
  ix->stats[4] = (exact_sum + nq / 2) / nq;
  ix->stats[5] = a.n_probe * 16;
  return CWQ_OK;
}

int score_topk_impl(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                    hipStream_t s, bool allow_filter) {
  const bool general = k > 64;
  const bool filt = !general && allow_filter && use_filter(ix, k);
  if (allow_filter) {
    ix->n_fg_i8 = 0;
    ix->i8_early_ran = false;
    ix->direct_ran = false;
  }
  if (!general && allow_filter && use_filter(ix, k, kStreamMinRows) && use_stream(ix, nq, k))
    return stream_topk_impl(ix, q, nq, k, ids, scores, s);
  const int kl = k <= 16 ? 16 : 64;
  const int K = std::min<int>(k, 64);
  const int n_pow2 = (int)std::max<int64_t>(2, 1LL << (int)ceil(log2((double)std::max(ix->NL, 2))));
  // partial-list entries per query (upper bound over both segments; one list for the filter)
  const int nqb_est = n_qblocks_for(nq, kl);
  auto n_slabs = [&](int nqb) {
    // a chunk may take either scan (use_small_scan on its own query count): room for both
    // (small_scan_slabs(1, n) is its largest slab count)
    const int n_iso = std::max(pick_nslab(ix, ix->NL_iso, nqb), small_scan_fits(ix, K) ? small_scan_slabs(1, ix->NL_iso) : 0);
    return filt ? 1 + (pick_nslab(ix, ix->NL_an, nqb) + 1) * scan_lists_per_slab(kl)
                : (n_iso + pick_nslab(ix, ix->NL_an, nqb) + 2) * scan_lists_per_slab(kl);
  };
  const int n_rt = filt ? (int)(ix->ld_f / kFgTile) : 0;
  const int n_rts = filt ? ix->ld_s / kFgTile : 0;
  // per query: bf16 query, info, sample bounds, threshold list, candidate lists, flags, records
  const size_t filt_q = filt ? iso_filter_bytes_per_query(ix, n_rt) : 0;
  const size_t extra = general ? (size_t)ix->NL * 4 + (size_t)n_pow2 * 8
                               : (size_t)n_slabs(nqb_est) * K * 12 + K * 12 + filt_q;
  int64_t cq = chunk_queries(ix, nq, extra, false);
  if (filt && cq < nq) cq = std::max<int64_t>(kFgTile, cq / kFgTile * kFgTile);   // whole query tiles
  int64_t n_fallback = 0, cand_sum = 0, exact_sum = 0;
  std::vector<int64_t> redo;
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    const int nqb = n_qblocks_for(nqc, kl);
    const int slabs = n_slabs(nqb);
    const int64_t nqf = round_up(nqc, kFgTile);
    size_t need = chunk_bytes(ix, nq_pad, false) + 64 * 256;
    need += general ? (size_t)nq_pad * ((size_t)ix->NL * 4 + (size_t)n_pow2 * 8)
                    : (size_t)nq_pad * ((size_t)slabs * K * 12 + (size_t)K * 12) + (size_t)nqf * filt_q + 4096 * 8;
    const bool ib = filt && use_int_bounds(ix);
    if (ib) need += int_bounds_bytes(ix, nqf);
    const bool prn = filt && !ib && !general && use_prune(ix);
    if ((rc = ix->reserve(need))) return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[0], s));
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if (ib) {
      if ((rc = run_internal_bounds(ix, c, q + q0 * ix->D, nqf, b, s))) return rc;
    } else if (prn) {
      if ((rc = prune_internal(ix, c, q + q0 * ix->D, K, b, s))) return rc;
    } else if ((rc = run_internal(ix, c, s, false, q + q0 * ix->D, filt ? 0 : -1))) {
      return rc;
    }
    if (filt && (rc = group_tables(ix, c, q + q0 * ix->D, false, s))) return rc;
    if (ix->timing) HIPCHK(hipEventRecord(ix->ev[1], s));
    if (!general) {
      float* pkey = b.take<float>((size_t)nq_pad * slabs * K);
      float* paux = b.take<float>((size_t)nq_pad * slabs * K);
      int* prow = b.take<int>((size_t)nq_pad * slabs * K);
      int nst = 0;
      int* okf = nullptr;
      int *qcnt_d = nullptr, *nex_d = nullptr;
      if (filt) {
        // isotropic rows: sample bounds -> thresholds -> MFMA filter -> candidates ->
        // exact rerank into list slot 0; anisotropic rows: exact scan into slots 1..
        IsoFilter fo;
        if ((rc = run_iso_filter(ix, c, q + q0 * ix->D, nqf, K, false, ib, b, fo, s))) return rc;
        int* qcnt = fo.qcnt;
        int* nex = fo.nex;
        okf = fo.okf;
        float* tl = fo.tl;
        float* tlk = fo.tlk;
        int* tr = fo.tr;
        int* tdone = fo.tdone;
        int* qover = fo.qover;
        int* crow = fo.crow;
        float* cu = fo.cu;
        float* cl = fo.cl;
        if ((rc = run_leaf_scan(ix, c, EPI_TOPK, false, kl, 0.f, nullptr, 0, pkey, paux, prow, K, &nst, s, 2, 1, slabs)))
          return rc;
        const IntChain chain = int_chain(ix);
        HIPCHK(launch_final(c.X, ix->iso_Mf, ix->DP, nqc, K, kFgCapQ, qcnt, qover, crow, cu, cl, tl + (K - 1), 64,
                            ix->row_meta, ix->row_par, c.P ? c.P : ix->dummy, c.pT ? 1 : c.ldP, 0, pkey, paux,
                            prow, (int64_t)nst * K, okf, nex, tlk, tr, tdone, ib ? &chain : nullptr, 0, 0.f, s));
        qcnt_d = qcnt;
        nex_d = nex;
        if (ix->timing) HIPCHK(hipEventRecord(ix->ev[7], s));
      } else {
        if ((rc = run_leaf_scan(ix, c, EPI_TOPK, false, kl, 0.f, nullptr, 0, pkey, paux, prow, K, &nst, s, 3, 0, slabs)))
          return rc;
      }
      if (ix->timing) HIPCHK(hipEventRecord(ix->ev[2], s));
      HIPCHK(launch_merge_expand(pkey, paux, prow, nqc, nst * K, K, k, ix->sent_ptr, ix->sent_ids, ids + q0 * k,
                                 scores ? scores + q0 * k : nullptr, s));
      if (filt) {
        if ((rc = ix->hflags.reserve((size_t)3 * nqf * sizeof(int)))) return rc;
        HIPCHK(hipMemcpyAsync(ix->hflags.p, qcnt_d, (size_t)3 * nqf * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int* cnth = ix->hflags.as<int>();
        const int* okh = cnth + nqf;
        const int* nexh = cnth + 2 * nqf;
        for (int i = 0; i < nqc; ++i) {
          if (!okh[i]) redo.push_back(q0 + i);
          cand_sum += cnth[i];
          exact_sum += nexh[i];
        }
      }
    } else {
      float* rowkey = b.take<float>((size_t)nq_pad * std::max(ix->NL, 1));
      float* skey = b.take<float>((size_t)nq_pad * n_pow2);
      int* srow = b.take<int>((size_t)nq_pad * n_pow2);
      if ((rc = run_leaf_scan(ix, c, EPI_KEY, false, 16, 0.f, rowkey, ix->NL, nullptr, nullptr, nullptr, 1, nullptr, s)))
        return rc;
      if (ix->timing) HIPCHK(hipEventRecord(ix->ev[2], s));
      HIPCHK(launch_init_rows(rowkey, ix->NL, nqc, ix->NL, n_pow2, skey, srow, s));
      HIPCHK(launch_sort_rows(skey, srow, nqc, ix->NL, n_pow2, s));
      HIPCHK(launch_expand(skey, srow, nqc, n_pow2, k, ix->sent_ptr, ix->sent_ids, ids + q0 * k,
                           scores ? scores + q0 * k : nullptr, s));
    }
    if (ix->timing) {
      HIPCHK(hipEventRecord(ix->ev[3], s));
      HIPCHK(hipEventSynchronize(ix->ev[3]));
      float a = 0, b2 = 0, c2 = 0, d = 0;
      HIPCHK(hipEventElapsedTime(&a, ix->ev[1], ix->ev[2]));
      HIPCHK(hipEventElapsedTime(&b2, ix->ev[0], ix->ev[1]));
      HIPCHK(hipEventElapsedTime(&c2, ix->ev[2], ix->ev[3]));
      HIPCHK(hipEventElapsedTime(&d, ix->ev[0], ix->ev[3]));
      ix->t_ms[0] += a;
      ix->t_ms[1] += b2;
      ix->t_ms[2] += c2;
      ix->t_ms[3] += d;
      ix->t_ms[4] += filt ? ix->n_fg_launch : (ix->NL_iso > 0) + (ix->NL_an > 0);   // filter: fgemm launches
      if (filt) {
        float e3 = 0;
        HIPCHK(hipEventElapsedTime(&e3, ix->ev[6], ix->ev[7]));
        ix->t_ms[7] += e3;
      }
    }
  }
  if (!redo.empty()) {
    n_fallback = (int64_t)redo.size();
    if ((rc = rerun_exact(ix, q, redo, k, ids, scores, s))) return rc;
  }
  if (allow_filter) {
    if (filt) note_i8_early(ix, nq, cand_sum, n_fallback);
    ix->stats[0] = filt ? nq : 0;
    ix->stats[1] = n_fallback;
    ix->stats[2] = filt ? 1 + ((int64_t)std::min(ix->n_fg_i8, 32767) << 16) : 0;   // (<< 16: its int8 launches)
    ix->stats[3] = filt && nq > 0 ? (cand_sum + nq / 2) / nq : 0;
    ix->stats[4] = filt && nq > 0 ? (exact_sum + nq / 2) / nq : 0;
    ix->stats[5] = filt ? ix->n_samp : 0;
  }
  return CWQ_OK;
}
}  // namespace

// The paired entry points (device / host memory) open alike: the argument checks; then, under the
// call's hold on the handle (QueryCall), the last call's record cleared.
static int topk_args(const cwq_index* ix, const float* q, int64_t nq, int32_t k, const int64_t* ids) {
  if (!ix || (!q && nq > 0) || (!ids && nq > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  if (k <= 0) return fail(CWQ_ERR_ARG, "k must be >= 1");
  return CWQ_OK;
}
static void topk_reset(cwq_index* ix) {
  for (float& t : ix->t_ms) t = 0.f;
  for (int64_t& t : ix->stats) t = 0;
  ix->prune_nq = 0;
}

namespace cwq {
// The host entry points' staging: the queries through pinned memory into ix->dq, room for
// obytes of results in the mapped host memory ix->hout
int stage_host(cwq_index* ix, const float* q, size_t qbytes, size_t obytes, hipStream_t s) {
  int rc;
  if ((rc = ix->hq.reserve(qbytes)) || (rc = ix->dq.reserve(qbytes)) || (rc = ix->hout.reserve(obytes))) return rc;
  memcpy(ix->hq.p, q, qbytes);
  HIPCHK(hipMemcpyAsync(ix->dq.p, ix->hq.p, qbytes, hipMemcpyHostToDevice, s));
  return CWQ_OK;
}

// for cwq_score_topk_masked (cwq_maskcalls.hip), which holds the handle itself: the last call's
// record cleared, and cwq_score_topk's work
void topk_begin(cwq_index* ix) { topk_reset(ix); }
int score_topk_unmasked(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                        hipStream_t s) {
  const int rc = score_topk_impl(ix, q, nq, k, ids, scores, s, true);
  if (!rc) note_filter(ix);
  return rc;
}
}  // namespace cwq

extern "C" int cwq_score_topk(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                              void* stream) {
  if (int rc = topk_args(ix, q, nq, k, ids)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  topk_reset(ix);
  if (call.rc) return call.rc;
  const int rc = score_topk_impl(ix, q, nq, k, ids, scores, s, true);
  if (!rc) note_filter(ix);
  return rc;
}

// The reference harness's call with host memory on both sides (benchmark_utils.py:801-805:
// a numpy query in, sentence ids out): the query is copied into pinned staging and sent with
// one async copy, the kernels write the ids / scores straight into mapped host memory, and
// the call returns synchronized -- no torch tensors, no device allocations, no separate
// device-to-host copy per call.
extern "C" int cwq_score_topk_host(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                                   void* stream) {
  if (int rc = topk_args(ix, q, nq, k, ids)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  topk_reset(ix);
  if (call.rc) return call.rc;
  const size_t qb = (size_t)nq * ix->D * 4, ib = (size_t)round_up(nq * k * 8, 256), sb = (size_t)nq * k * 4;
  int rc;
  if ((rc = stage_host(ix, q, qb, ib + sb, s))) return rc;
  int64_t* hid = ix->hout.as<int64_t>();
  float* hsc = (float*)(ix->hout.as<char>() + ib);
  if ((rc = score_topk_impl(ix, ix->dq.as<float>(), nq, k, hid, hsc, s, true))) return rc;
  note_filter(ix);
  HIPCHK(sync_spin(s));
  ix->ws_idle = true;   // synchronized
  memcpy(ids, hid, (size_t)nq * k * 8);
  if (scores) memcpy(scores, hsc, sb);
  return CWQ_OK;
}
