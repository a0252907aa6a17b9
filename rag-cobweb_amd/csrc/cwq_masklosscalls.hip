// Masked ranking loss (no reference counterpart): cwq_rank_ce_masked, the
// cross-entropy loss, its gradient, the target's score and rank over a mask's allowed sentences,
// and cwq_rank_ce_topk_masked, the truncated loss over the masked retrieval's top-K.
// Calls the exact per-chunk passes (cwq_chunk.hip), the CE kernels (cwq_loss.hip), the key-writing
// gathered scan (cwq_mask.hip), the backward's kernels (cwq_grad.hip) and, for the top-K form,
// the masked Fast call (cwq_maskcalls.hip) and the pair kernels' host passes (cwq_sparsecalls.hip).
#include "cwq_handle.h"

namespace {

// ---- the path rule ----
// Full: rank_ce_impl's pipeline (the exact scan over every row, the backward stream over every
// row) with the rows' allowed counts.  Gathered: both streams over the mask's live rows only.
// Fitted on flat 1M x 768 and 100k x 768 (profiles/maskloss_probe_c3.log, _100k.log; DESIGN
// §4.19): the gathered path's time is linear in the live fraction and meets the full path's at
// 0.93 / 0.50 / 0.79 of the rows for 1 / 16 / 256 queries at 1M rows (100k: near 1, 0.9, 0.73).
// The rule may not read nq, so it follows the lowest crossing, the 16-query call's; 0.55 puts a
// random half mask (0.499 - 0.501 of the rows live) on the gathered side, where it ties at 16
// queries and is 33 - 40% faster at 1 and 256.
constexpr double kMaskCeGatherFrac = 0.55;

int mask_ce_path_env() {
  const char* e = getenv("CWQ_MASK_CE_PATH");
  const int v = e && *e ? atoi(e) : 0;
  return v == 1 || v == 2 ? v : 0;
}

bool mask_of_index(const cwq_index* ix, const cwq_mask* m) {
  return m->serial == ix->serial && m->n_sent == ix->n_sent && m->NL_iso == ix->NL_iso && m->NL_an == ix->NL_an;
}

// slabs of a segment's row list for the key-writing scan: ~4 workgroups per CU, whole tiles
void key_slabs(const cwq_index* ix, int n_live, int n_qblocks, bool shq, int& nslab, int& rps) {
  nslab = rps = 0;
  if (n_live <= 0) return;
  const int tile = mask_scan_tile(shq);
  const int tiles = (n_live + tile - 1) / tile;
  const int n = (int)std::min<int64_t>(tiles, std::max<int64_t>(1, (int64_t)4 * ix->cus / std::max(1, n_qblocks)));
  rps = (tiles + n - 1) / n * tile;
  nslab = (n_live + rps - 1) / rps;
}

// The gathered backward's plan: the dense plan with the two leaf-class streams cut by list
// position -- a function of the index and the mask alone.
GradPlan gathered_plan(const cwq_index* ix, const cwq_mask* m) {
  GradPlan g = grad_plan(ix);
  g.rps = grad_rows_per_slab((int64_t)m->n_iso + 2 * ((int64_t)m->n_an + ix->NI), ix->cus);
  g.ns_iso = (m->n_iso + g.rps - 1) / g.rps;
  g.ns_an = (m->n_an + g.rps - 1) / g.rps;
  g.ns_int = (ix->NI + g.rps - 1) / g.rps;
  g.nslab = g.ns_iso + g.ns_an + g.ns_int;
  g.per_q = ((size_t)2 * std::max(ix->NL, 1) + (size_t)(2 + g.nsplit) * std::max(ix->NI, 1) + (size_t)g.nslab * ix->DP) * 4;
  return g;
}

// The three streams of the backward and the slab sum.  m: the gathered path walks the mask's
// row lists (dead rows' coefficients are zero, so the full path's sum has the same terms).
int loss_streams(const cwq_index* ix, const cwq_mask* m, const GradPlan& gp, const GradCoefArgs& ca, float* part,
                 const float* q, int nqc, int qtiles, float* grad_q, hipStream_t s) {
  GradStreamArgs g;
  memset(&g, 0, sizeof(g));
  g.q = q;
  g.nq = nqc;
  g.qtiles = qtiles;
  g.D = ix->D;
  g.DP = ix->DP;
  g.rows_per_slab = gp.rps;
  g.part = part;
  g.coef = ca.coefL;
  g.ncoef = ix->NL;
  const int n_iso = m ? m->n_iso : ix->NL_iso, n_an = m ? m->n_an : ix->NL_an;
  if (n_iso > 0) {
    g.M = ix->iso_Mf;
    g.nrows = n_iso;
    g.list = m ? m->rows_iso : nullptr;
    g.coef_base = 0;
    g.slab_off = 0;
    HIPCHK(launch_grad_stream(g, s));
  }
  g.M = nullptr;
  if (n_an > 0) {
    g.A = ix->an_A;
    g.B = ix->an_B;
    g.ld = ix->ld_an;
    g.nrows = n_an;
    g.list = m ? m->rows_an : nullptr;
    g.coef_base = ix->NL_iso;
    g.slab_off = gp.ns_iso;
    HIPCHK(launch_grad_stream(g, s));
  }
  g.list = nullptr;
  if (ix->NI > 0) {   // the internal nodes: as the unmasked backward streams them
    g.A = ix->int_A;
    g.B = ix->int_B;
    g.ld = ix->ld_int;
    g.nrows = ix->NI;
    g.coef = ca.coefI;
    g.ncoef = ix->NI;
    g.coef_base = 0;
    g.slab_off = gp.ns_iso + gp.ns_an;
    HIPCHK(launch_grad_stream(g, s));
  }
  HIPCHK(launch_grad_reduce(part, gp.nslab, qtiles, nqc, ix->DP, ix->D, grad_q, s));
  return CWQ_OK;
}

// The gathered forward: -inf into the chunk's key lines, then the exact keys of the live rows.
int gathered_keys(cwq_index* ix, const cwq_mask* m, const Chunk& c, int nqc, float* rowkey, hipStream_t s) {
  const int NL = ix->NL;
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)rowkey, (int)0xff800000u, (size_t)nqc * NL, s));
  const bool shq = nqc <= kXQ * 2;   // small chunks: the shared-query form (the keys are the same bits)
  const int qpb = shq ? kXQ : kXQ * kWavesPerWG;
  MaskScanArgs a;
  memset(&a, 0, sizeof(a));
  a.DP = ix->DP;
  a.nq = nqc;
  a.n_qblocks = (nqc + qpb - 1) / qpb;
  a.P = c.P ? c.P : ix->dummy;
  a.ldP = std::max(ix->NI, 1);
  a.dconst = 0.f;
  a.rowkey = rowkey;
  a.ldr = NL;
  int ns, rps;
  if (m->n_iso > 0) {
    key_slabs(ix, m->n_iso, a.n_qblocks, shq, ns, rps);
    a.n_live = m->n_iso;
    a.rows_per_slab = rps;
    a.seg_base = 0;
    a.list = m->rows_iso;
    a.meta = ix->row_meta;
    a.par = ix->row_par;
    HIPCHK(launch_mask_scan_keys(true, shq, c.X, ix->iso_Mf, nullptr, a, ns, s));
  }
  if (m->n_an > 0) {
    key_slabs(ix, m->n_an, a.n_qblocks, shq, ns, rps);
    a.n_live = m->n_an;
    a.rows_per_slab = rps;
    a.seg_base = ix->NL_iso;
    a.list = m->rows_an;
    a.ld = ix->ld_an;
    a.meta = ix->row_meta + ix->NL_iso;
    a.par = ix->row_par + ix->NL_iso;
    HIPCHK(launch_mask_scan_keys(false, shq, c.X, ix->an_A, ix->an_B, a, ns, s));
  }
  return CWQ_OK;
}

// rank_ce_impl (cwq_rank.hip) with the mask: the rows' allowed counts, computed per call, in
// place of their sentence counts; the key and coefficient arrays stay dense and [row]-indexed on
// both paths, so loss, target_score and rank are the same bits on both.
int rank_ce_masked_impl(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, const int64_t* target,
                        float temperature, float* loss, float* grad_q, float* target_score, int64_t* rank,
                        hipStream_t s) {
  const int NL = ix->NL;
  const int64_t live = (int64_t)m->n_iso + m->n_an;
  const int forced = mask_ce_path_env();
  const bool gathered = forced ? forced == 2 : (double)live < kMaskCeGatherFrac * (double)NL;
  for (int64_t& t : ix->mask_stats) t = 0;
  ix->mask_stats[0] = gathered ? 6 : 5;
  ix->mask_stats[3] = live;
  if (live == 0)   // nothing is allowed: every target is invalid, no scan
    return launch_ce_invalid(nq, ix->D, loss, grad_q, target_score, rank, s) == hipSuccess
               ? CWQ_OK
               : fail(CWQ_ERR_HIP, "launch_ce_invalid failed");
  const int npart = (NL + kCePart - 1) / kCePart;
  const GradPlan gp = gathered ? gathered_plan(ix, m) : grad_plan(ix);
  const bool grad = grad_q != nullptr;
  const size_t ce_q = (size_t)std::max(npart, 1) * 12 + 12;
  const size_t per_q = (size_t)std::max(NL, 1) * 4 + ce_q + (grad ? gp.per_q : 0);
  const int64_t cq = std::min<int64_t>(chunk_queries(ix, nq, per_q, false), 4096);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    const int qtiles = (nqc + kXQ - 1) / kXQ;
    const size_t nq16 = (size_t)qtiles * kXQ;
    if ((rc = ix->reserve(chunk_bytes(ix, nq_pad, false) + (size_t)nq_pad * std::max(NL, 1) * 4 + nq16 * ce_q +
                          (grad ? nq16 * gp.per_q : 0) + (size_t)std::max(NL, 1) * 4 + 32 * 256)))
      return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    float* rowkey = b.take<float>((size_t)nq_pad * std::max(NL, 1));
    int* cnt = b.take<int>(std::max(NL, 1));
    CeArgs a;
    memset(&a, 0, sizeof(a));
    a.rowkey = rowkey;
    a.ldr = NL;
    a.NL = NL;
    a.nq = nqc;
    a.qtiles = qtiles;
    a.npart = npart;
    a.invT = 1.f / temperature;
    a.sent_ptr = ix->sent_ptr;
    a.sent_ids = ix->sent_ids;
    a.row_bfs = ix->row_bfs;
    a.row_of_sent = ix->row_of_sent;
    a.n_sent = ix->n_sent;
    a.target = target + q0;
    a.pm = b.take<float>(nq16 * std::max(npart, 1));
    a.pz = b.take<float>(nq16 * std::max(npart, 1));
    a.pc = b.take<int>(nq16 * std::max(npart, 1));
    a.mz = b.take<float2>(nq16);
    a.rtq = b.take<int>(nq16);
    a.loss = loss + q0;
    a.tscore = target_score ? target_score + q0 : nullptr;
    a.rank = rank ? rank + q0 : nullptr;
    a.cnt = cnt;
    a.bits = m->bits;
    HIPCHK(launch_mask_counts(m->live, ix->sent_ptr, ix->sent_ids, m->bits, NL, cnt, s));
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false))) return rc;
    if (gathered) {
      if ((rc = gathered_keys(ix, m, c, nqc, rowkey, s))) return rc;
    } else if ((rc = run_leaf_scan(ix, c, EPI_KEY, false, 16, 0.f, rowkey, NL, nullptr, nullptr, nullptr, 1, nullptr,
                                   s))) {
      return rc;
    }
    HIPCHK(launch_ce_reduce(a, s));
    if (!grad) continue;
    GradCoefArgs ca;
    float* part = grad_carve(ix, gp, b, nqc, qtiles, ca);
    HIPCHK(launch_ce_coef(a, ca.meta, ix->NL_iso, ca.coefL, ca.hL, s));
    HIPCHK(launch_grad_tree(ca, s));
    if ((rc = loss_streams(ix, gathered ? m : nullptr, gp, ca, part, q + q0 * ix->D, nqc, qtiles, grad_q + q0 * ix->D,
                           s)))
      return rc;
  }
  return CWQ_OK;
}

int check_temperature(float temperature) {
  if (!std::isfinite(temperature) || !(temperature > 0.f))
    return fail(CWQ_ERR_ARG, "temperature must be finite and > 0");
  return CWQ_OK;
}

}  // namespace

extern "C" int cwq_rank_ce_masked(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, const int64_t* target,
                                  float temperature, float* loss, float* grad_q, float* target_score, int64_t* rank,
                                  void* stream) {
  if (!ix || !m || !q || !target || !loss) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  if (int rc = check_temperature(temperature)) return rc;
  if (!mask_of_index(ix, m)) return fail(CWQ_ERR_ARG, "the mask was built for another index");
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  return rank_ce_masked_impl(ix, m, q, nq, target, temperature, loss, grad_q, target_score, rank, s);
}

extern "C" int cwq_rank_ce_topk_masked(cwq_index* ix, const cwq_mask* const* masks, int32_t n_masks,
                                       const int32_t* mask_of_query, const float* q, int64_t nq,
                                       const int64_t* target, float temperature, int32_t K, float* loss, float* grad_q,
                                       float* target_score, int64_t* rank, float* tail_bound, int64_t* cand_ids,
                                       void* stream) {
  if (!ix || !masks || !q || !target || !loss) return fail(CWQ_ERR_ARG, "NULL argument");
  if (n_masks < 1) return fail(CWQ_ERR_ARG, "n_masks must be >= 1");
  if (!mask_of_query && n_masks != 1) return fail(CWQ_ERR_ARG, "mask_of_query may be NULL only when n_masks == 1");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  if (K < 1) return fail(CWQ_ERR_ARG, "K must be >= 1");
  if (int rc = check_temperature(temperature)) return rc;
  if (grad_q && (int64_t)K + 1 > kSparseMaxM)
    return fail(CWQ_ERR_ARG, "the sparse backward takes at most 4096 entries per query: K + 1 <= 4096 with grad_q");
  if (mask_of_query)
    for (int64_t i = 0; i < nq; ++i)
      if (mask_of_query[i] < 0 || mask_of_query[i] >= n_masks)
        return fail(CWQ_ERR_ARG, "mask_of_query[" + std::to_string(i) + "] = " + std::to_string(mask_of_query[i]) +
                                     " is outside [0, " + std::to_string(n_masks) + ")");
  for (int32_t i = 0; i < n_masks; ++i) {   // the first checks that read a handle
    if (!masks[i]) return fail(CWQ_ERR_ARG, "masks[" + std::to_string(i) + "] is NULL");
    if (!mask_of_index(ix, masks[i])) return fail(CWQ_ERR_ARG, "the mask was built for another index");
  }
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  // the handle's masked-loss buffer (the masked Fast call uses mk, fb and mg itself): the slot
  // table, the queries' slots, the top-K result, the target's key, the backward's list
  const int64_t K1 = (int64_t)K + 1;
  std::vector<MaskSlot> slots((size_t)n_masks);
  for (int32_t i = 0; i < n_masks; ++i) slots[i] = MaskSlot{masks[i]->bits, masks[i]->n_allowed};
  const size_t o_qs = round_up((int64_t)(slots.size() * sizeof(MaskSlot)), 256), o_tid = o_qs + round_up(nq * 4, 256),
               o_ts = o_tid + round_up(nq * (int64_t)K * 8, 256), o_tk = o_ts + round_up(nq * (int64_t)K * 4, 256),
               o_bid = o_tk + round_up(nq * 4, 256), o_bg = o_bid + (grad_q ? round_up(nq * K1 * 8, 256) : 0),
               tot = o_bg + (grad_q ? round_up(nq * K1 * 4, 256) : 0);
  int rc;
  if ((rc = ix->ml.reserve(tot, ix->busy()))) return rc;
  char* ml = ix->ml.as<char>();
  int* qslot = mask_of_query ? (int*)(ml + o_qs) : nullptr;
  int64_t* tid = (int64_t*)(ml + o_tid);
  float* ts = (float*)(ml + o_ts);
  float* tk = (float*)(ml + o_tk);
  HIPCHK(hipMemcpyAsync(ml, slots.data(), slots.size() * sizeof(MaskSlot), hipMemcpyHostToDevice, s));
  if (qslot) HIPCHK(hipMemcpyAsync(qslot, mask_of_query, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // pageable host tables: uploaded before this frame and the caller's array go
  if ((rc = masked_topk_locked(ix, masks, n_masks, mask_of_query, q, nq, K, tid, ts, s))) return rc;
  ix->ws_idle = false;   // a path of the Fast call may end synchronized, but this call goes on using the workspace
  if ((rc = pairs_forward(ix, q, nq, target, 1, 1, tk, 1, s))) return rc;
  SparseCeArgs a;
  memset(&a, 0, sizeof(a));
  a.nq = (int)nq;
  a.K = K;
  a.NL = ix->NL;
  a.invT = 1.f / temperature;
  a.top_ids = tid;
  a.top_scores = ts;
  a.target = target;
  a.tscore = tk;
  a.n_sent = ix->n_sent;
  a.row_of_sent = ix->row_of_sent;
  a.sent_ptr = ix->sent_ptr;
  a.loss = loss;
  a.tscore_out = target_score;
  a.rank = rank;
  a.tail_bound = tail_bound;
  a.cand_ids = cand_ids;
  a.bid = grad_q ? (int64_t*)(ml + o_bid) : nullptr;
  a.bg = grad_q ? (float*)(ml + o_bg) : nullptr;
  a.slots = (const MaskSlot*)ml;
  a.qslot = qslot;
  HIPCHK(launch_ce_topk(a, s));
  if (!grad_q) return CWQ_OK;
  return pairs_backward(ix, q, nq, a.bid, (int)K1, a.bg, grad_q, s);
}
