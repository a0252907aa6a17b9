// Sparse differentiable scores: cwq_score_pairs, cwq_score_pairs_backward and
// cwq_rank_ce_topk over the kernels of cwq_sparse.hip, the exact internal pass and the backward's
// stream kernel for the internal nodes (cwq_grad.hip).
#include "cwq_handle.h"

namespace cwq {

// scores[q][j] for the call's queries, chunk by chunk: pad, the exact internal pass (the parents'
// prefixes, bit for bit the scan's), the gathered keys.
int pairs_forward(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int m, int64_t ld_ids, float* out,
                  int64_t ld_out, hipStream_t s) {
  const int64_t cq = chunk_queries(ix, nq, 0, false);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    if ((rc = ix->reserve(chunk_bytes(ix, nq_pad, false) + 8 * 256))) return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false))) return rc;
    SparsePairArgs a;
    memset(&a, 0, sizeof(a));
    a.X = c.X;
    a.DP = ix->DP;
    a.nq = nqc;
    a.m = m;
    a.ids = ids + q0 * ld_ids;
    a.ld_ids = ld_ids;
    a.n_sent = ix->n_sent;
    a.row_of_sent = ix->row_of_sent;
    a.NL_iso = ix->NL_iso;
    a.Mf = ix->iso_Mf;
    a.anA = ix->an_A;
    a.anB = ix->an_B;
    a.ld_an = ix->ld_an;
    a.meta = ix->row_meta;
    a.par = ix->row_par;
    a.P = c.P ? c.P : ix->dummy;
    a.ldP = std::max(ix->NI, 1);
    a.dconst = 0.f;
    a.out = out + q0 * ld_out;
    a.ld_out = ld_out;
    HIPCHK(launch_sparse_pairs(a, s));
  }
  return CWQ_OK;
}

// grad_q for the call's queries: the listed rows gathered per query (slab 0), the internal nodes
// through grad_stream_kernel from the scattered coefficients (slabs 1..), the slab sum.  The slab
// size is a function of the index alone, so a query's gradient does not depend on the batch.
int pairs_backward(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int m, const float* g, float* grad_q,
                   hipStream_t s) {
  const int NI = ix->NI, DP = ix->DP;
  // the internal class alone is streamed here: slabs of at least 64 nodes (not the dense backward's
  // 256) so that a tree of ~10k internal nodes still fills the CUs at one query tile
  const int64_t per = ((int64_t)NI + 3 * (int64_t)ix->cus - 1) / (3 * (int64_t)ix->cus);
  const int rps = (int)((std::max<int64_t>(per, 64) + 7) / 8 * 8);
  const int ns_int = (NI + rps - 1) / rps;
  const size_t per_q = ((size_t)2 * std::max(NI, 1) + (size_t)(1 + ns_int) * DP) * 4;
  const int64_t cq = std::min<int64_t>(chunk_queries(ix, nq, per_q, false), 4096);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int qtiles = (nqc + kXQ - 1) / kXQ;
    const size_t nq16 = (size_t)qtiles * kXQ;
    if ((rc = ix->reserve(nq16 * per_q + 8 * 256))) return rc;
    Bump b(ix->ws.p, ix->ws.size);
    float* cI = b.take<float>(nq16 * std::max(NI, 1));
    float* coefI = b.take<float>(nq16 * std::max(NI, 1));
    float* part = b.take<float>(nq16 * (size_t)(1 + ns_int) * DP);
    SparseGradArgs a;
    memset(&a, 0, sizeof(a));
    a.q = q + q0 * ix->D;
    a.nq = nqc;
    a.qtiles = qtiles;
    a.D = ix->D;
    a.DP = DP;
    a.m = m;
    a.ids = ids + q0 * m;
    a.g = g + q0 * m;
    a.n_sent = ix->n_sent;
    a.row_of_sent = ix->row_of_sent;
    a.NL_iso = ix->NL_iso;
    a.NI = NI;
    a.Mf = ix->iso_Mf;
    a.anA = ix->an_A;
    a.anB = ix->an_B;
    a.ld_an = ix->ld_an;
    a.meta = ix->row_meta;
    a.par = ix->row_par;
    a.par_int = ix->par_int;
    a.w_int = ix->w_int;
    a.part = part;
    a.cI = cI;
    a.coefI = coefI;
    HIPCHK(launch_sparse_grad(a, s));
    if (NI > 0) {
      GradStreamArgs gs;
      memset(&gs, 0, sizeof(gs));
      gs.q = a.q;
      gs.nq = nqc;
      gs.qtiles = qtiles;
      gs.D = ix->D;
      gs.DP = DP;
      gs.A = ix->int_A;
      gs.B = ix->int_B;
      gs.ld = ix->ld_int;
      gs.nrows = NI;
      gs.rows_per_slab = rps;
      gs.coef = coefI;
      gs.ncoef = NI;
      gs.coef_base = 0;
      gs.part = part;
      gs.slab_off = 1;
      HIPCHK(launch_grad_stream(gs, s));
    }
    HIPCHK(launch_grad_reduce(part, 1 + ns_int, qtiles, nqc, DP, ix->D, grad_q + q0 * ix->D, s));
  }
  return CWQ_OK;
}

}  // namespace cwq

namespace {

int backward_m_check(int64_t m) {
  if (m > kSparseMaxM)
    return fail(CWQ_ERR_ARG, "the sparse backward takes at most 4096 entries per query: scatter the gradient into "
                             "[nq, n_sent] and call cwq_rank_scores_backward");
  return CWQ_OK;
}

}  // namespace

extern "C" int cwq_score_pairs(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int32_t m, float* scores,
                               void* stream) {
  if (!ix || !q || !ids || !scores) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  if (m < 1) return fail(CWQ_ERR_ARG, "m must be >= 1");
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  return pairs_forward(ix, q, nq, ids, m, m, scores, m, s);
}

extern "C" int cwq_score_pairs_backward(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int32_t m,
                                        const float* grad_scores, float* grad_q, void* stream) {
  if (!ix || !q || !ids || !grad_scores || !grad_q) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  if (m < 1) return fail(CWQ_ERR_ARG, "m must be >= 1");
  if (int rc = backward_m_check(m)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  return pairs_backward(ix, q, nq, ids, m, grad_scores, grad_q, s);
}

extern "C" int cwq_rank_ce_topk(cwq_index* ix, const float* q, int64_t nq, const int64_t* target, float temperature,
                                int32_t K, float* loss, float* grad_q, float* target_score, int64_t* rank,
                                float* tail_bound, int64_t* cand_ids, void* stream) {
  if (!ix || !q || !target || !loss) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  if (K < 1) return fail(CWQ_ERR_ARG, "K must be >= 1");
  if (!std::isfinite(temperature) || !(temperature > 0.f))
    return fail(CWQ_ERR_ARG, "temperature must be finite and > 0");
  if (grad_q)
    if (int rc = backward_m_check((int64_t)K + 1)) return rc;
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  topk_begin(ix);
  if (call.rc) return call.rc;
  // the handle's buffers (not `ws`: score_topk_impl carves that anew per chunk): the top-K
  // result, the target's key, the backward's list
  const int64_t K1 = (int64_t)K + 1;
  const size_t o_ts = round_up(nq * (int64_t)K * 8, 256), o_tk = o_ts + round_up(nq * (int64_t)K * 4, 256),
               o_bid = o_tk + round_up(nq * 4, 256), o_bg = o_bid + (grad_q ? round_up(nq * K1 * 8, 256) : 0),
               tot = o_bg + (grad_q ? round_up(nq * K1 * 4, 256) : 0);
  int rc;
  if ((rc = ix->mk.reserve(tot, ix->busy()))) return rc;
  char* mk = ix->mk.as<char>();
  int64_t* tid = (int64_t*)mk;
  float* ts = (float*)(mk + o_ts);
  float* tk = (float*)(mk + o_tk);
  if ((rc = score_topk_unmasked(ix, q, nq, K, tid, ts, s))) return rc;
  ix->ws_idle = false;   // the per-call path ends synchronized, but this call goes on using the workspace
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
  a.bid = grad_q ? (int64_t*)(mk + o_bid) : nullptr;
  a.bg = grad_q ? (float*)(mk + o_bg) : nullptr;
  HIPCHK(launch_ce_topk(a, s));
  if (!grad_q) return CWQ_OK;
  return pairs_backward(ix, q, nq, a.bid, (int)K1, a.bg, grad_q, s);
}
