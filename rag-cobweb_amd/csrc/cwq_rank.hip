// Scores over all leaves: call-time level weights, rank scores, their backward, the cross-entropy
// loss, cwq_node_logprob and cwq_prefix_bounds.  Calls the chunk passes (cwq_chunk.hip).
#include "cwq_handle.h"

namespace {
// Call-time level weights (cwq_lweight.hip): the chunk's RowMeta' / w_int' in the workspace,
// read by the exact passes and the backward's coefficient kernels instead of the index's.
size_t lw_operand_bytes(const cwq_index* ix, const float* level_w) {
  return level_w ? (size_t)std::max(ix->NL, 1) * sizeof(RowMeta) + (size_t)std::max(ix->NI, 1) * 4 + 2 * 256 : 0;
}
int lw_operands(const cwq_index* ix, Bump& b, const float* level_w, int n_w, const RowMeta** meta, const float** w_int,
                hipStream_t s) {
  *meta = ix->row_meta;
  *w_int = ix->w_int;
  if (!level_w) return CWQ_OK;
  RowMeta* m = b.take<RowMeta>(std::max(ix->NL, 1));
  float* w = b.take<float>(std::max(ix->NI, 1));
  HIPCHK(launch_lw_operands(level_w, n_w, ix->row_meta, ix->row_depth, ix->NL, ix->int_depth, ix->NI, m, w, s));
  *meta = m;
  *w_int = w;
  return CWQ_OK;
}
int lw_check(const float* level_w, int32_t n_w) {
  (void)level_w;
  if (n_w < 0 || n_w > kLwMaxLevels) return fail(CWQ_ERR_ARG, "n_w must be in [0, 64]");
  return CWQ_OK;
}

int rank_scores_impl(cwq_index* ix, const float* q, int64_t nq, const float* level_w, int n_w, float* out,
                     void* stream) {
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  const int64_t cq = chunk_queries(ix, nq, (size_t)ix->NL * 4, false);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    if ((rc = ix->reserve(chunk_bytes(ix, nq_pad, false) + (size_t)nq_pad * std::max(ix->NL, 1) * 4 + 8 * 256 +
                          lw_operand_bytes(ix, level_w))))
      return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    float* rowkey = b.take<float>((size_t)nq_pad * std::max(ix->NL, 1));
    if ((rc = lw_operands(ix, b, level_w, n_w, &c.meta, &c.w_int, s))) return rc;
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false))) return rc;
    if ((rc = run_leaf_scan(ix, c, EPI_KEY, false, 16, 0.f, rowkey, ix->NL, nullptr, nullptr, nullptr, 1, nullptr, s)))
      return rc;
    HIPCHK(launch_gather_sentences(rowkey, ix->NL, nqc, ix->row_of_sent, ix->n_sent, out + q0 * ix->n_sent, s));
  }
  return CWQ_OK;
}
}  // namespace

extern "C" int cwq_rank_scores(cwq_index* ix, const float* q, int64_t nq, float* out, void* stream) {
  if (!ix || (!q && nq > 0) || (!out && nq > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  return rank_scores_impl(ix, q, nq, nullptr, 0, out, stream);
}

extern "C" int cwq_rank_scores_w(cwq_index* ix, const float* q, int64_t nq, const float* level_w, int32_t n_w,
                                 float* out, void* stream) {
  if (!ix || !q || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  if (int rc = lw_check(level_w, n_w)) return rc;
  return rank_scores_impl(ix, q, nq, level_w, n_w, out, stream);
}

namespace cwq {
// The backward's launch plan (GradPlan, cwq_handle.h; shared with cwq_masklosscalls.hip)
GradPlan grad_plan(const cwq_index* ix) {
  GradPlan g;
  const int NL = ix->NL, NI = ix->NI;
  g.rps = grad_rows_per_slab((int64_t)ix->NL_iso + 2 * ((int64_t)ix->NL_an + NI), ix->cus);
  g.ns_iso = (ix->NL_iso + g.rps - 1) / g.rps;
  g.ns_an = (ix->NL_an + g.rps - 1) / g.rps;
  g.ns_int = (NI + g.rps - 1) / g.rps;
  g.nslab = g.ns_iso + g.ns_an + g.ns_int;
  g.nsplit = (int)std::min<int64_t>(64, std::max<int64_t>(1, ((int64_t)ix->max_fanout + 4095) / 4096));
  g.P = ix->max_fanout > 64 ? 16 : 1;
  for (auto& l : ix->levels) {
    g.lv.push_back(l.first);
    g.lv.push_back(l.second);
  }
  g.per_q = ((size_t)2 * std::max(NL, 1) + (size_t)(2 + g.nsplit) * std::max(NI, 1) + (size_t)g.nslab * ix->DP) * 4;
  return g;
}

// The coefficient arrays and the partial tiles of one chunk (nq16 * per_q bytes + 8 * 256).
float* grad_carve(const cwq_index* ix, const GradPlan& gp, Bump& b, int nqc, int qtiles, GradCoefArgs& ca) {
  const int NL = ix->NL, NI = ix->NI;
  const size_t nq16 = (size_t)qtiles * kXQ;
  memset(&ca, 0, sizeof(ca));
  ca.n_sent = ix->n_sent;
  ca.nq = nqc;
  ca.qtiles = qtiles;
  ca.NL = NL;
  ca.NL_iso = ix->NL_iso;
  ca.NI = NI;
  ca.sent_ptr = ix->sent_ptr;
  ca.sent_ids = ix->sent_ids;
  ca.meta = ix->row_meta;
  ca.leaf_a0 = ix->int_leaf_a0;
  ca.leaf_a1 = ix->int_leaf_a1;
  ca.leaf_b0 = ix->int_leaf_b0;
  ca.leaf_b1 = ix->int_leaf_b1;
  ca.child_begin = ix->int_child_begin;
  ca.child_end = ix->int_child_end;
  ca.w_int = ix->w_int;
  ca.lv = gp.lv.data();
  ca.nlev = (int)ix->levels.size();
  ca.P = gp.P;
  ca.nsplit = gp.nsplit;
  ca.coefL = b.take<float>(nq16 * std::max(NL, 1));
  ca.hL = b.take<float>(nq16 * std::max(NL, 1));
  ca.cz = b.take<float>(nq16 * std::max(NI, 1) * gp.nsplit);
  ca.cI = b.take<float>(nq16 * std::max(NI, 1));
  ca.coefI = b.take<float>(nq16 * std::max(NI, 1));
  return b.take<float>(nq16 * (size_t)gp.nslab * ix->DP);
}
}  // namespace cwq

namespace {

// The streaming reduction over the three row classes and the slab sum, from the coefficients.
int grad_streams(const cwq_index* ix, const GradPlan& gp, const GradCoefArgs& ca, float* part, const float* q, int nqc,
                 int qtiles, float* grad_q, hipStream_t s) {
  const int NL = ix->NL, NI = ix->NI, DP = ix->DP;
  GradStreamArgs g;
  memset(&g, 0, sizeof(g));
  g.q = q;
  g.nq = nqc;
  g.qtiles = qtiles;
  g.D = ix->D;
  g.DP = DP;
  g.rows_per_slab = gp.rps;
  g.part = part;
  if (ix->NL_iso > 0) {   // isotropic rows: row-major fp32 means, 1/v folded into the coefficient
    g.M = ix->iso_Mf;
    g.nrows = ix->NL_iso;
    g.coef = ca.coefL;
    g.ncoef = NL;
    g.coef_base = 0;
    g.slab_off = 0;
    HIPCHK(launch_grad_stream(g, s));
  }
  g.M = nullptr;
  if (ix->NL_an > 0) {
    g.A = ix->an_A;
    g.B = ix->an_B;
    g.ld = ix->ld_an;
    g.nrows = ix->NL_an;
    g.coef = ca.coefL;
    g.ncoef = NL;
    g.coef_base = ix->NL_iso;
    g.slab_off = gp.ns_iso;
    HIPCHK(launch_grad_stream(g, s));
  }
  if (NI > 0) {
    g.A = ix->int_A;
    g.B = ix->int_B;
    g.ld = ix->ld_int;
    g.nrows = NI;
    g.coef = ca.coefI;
    g.ncoef = NI;
    g.coef_base = 0;
    g.slab_off = gp.ns_iso + gp.ns_an;
    HIPCHK(launch_grad_stream(g, s));
  }
  HIPCHK(launch_grad_reduce(part, gp.nslab, qtiles, nqc, DP, ix->D, grad_q, s));
  return CWQ_OK;
}

// The weight gradient of one chunk (cwq_lweight.hip) from the coefficient pass's hL / cI and
// the raw sums the exact passes left: the chunk's S_int and sraw (EPI_RAW over the leaf rows).
size_t lw_grad_bytes_per_q(const cwq_index* ix) {   // sraw is counted by the caller (nq_pad lines)
  return (size_t)lw_parts(ix->NL, ix->NI) * (ix->max_depth + 1) * 8;
}
int lw_grad(const cwq_index* ix, const Chunk& c, const GradCoefArgs& ca, const float* sraw, bool is_lp, double* part,
            int n_w, float* grad_w, hipStream_t s) {
  LwGradArgs g;
  memset(&g, 0, sizeof(g));
  g.nq = ca.nq;
  g.qtiles = ca.qtiles;
  g.NL = ix->NL;
  g.NI = ix->NI;
  g.nlev = ix->max_depth + 1;
  g.n_w = n_w;
  g.hL = ca.hL;
  g.cI = ca.cI;
  g.S_row = sraw;
  g.ldS_row = std::max(ix->NL, 1);
  g.S_int = c.S_int;
  g.ldS_int = std::max(ix->NI, 1);
  g.logdet_row = is_lp ? nullptr : ix->logdet_row;
  g.logdet_int = ix->logdet_int;
  g.row_depth = ix->row_depth;
  g.int_depth = ix->int_depth;
  g.part = part;
  g.grad_w = grad_w;
  HIPCHK(launch_lw_grad(g, s));
  return CWQ_OK;
}

// Backward of cwq_rank_scores (cwq_grad.hip): the coefficient pass, the streaming reduction
// over the three row classes, the slab sum.  Needs q, grad_out and the index only; the weight
// gradient also needs the forward's raw sums, which it recomputes (internal pass + EPI_RAW).
int rank_scores_backward_impl(cwq_index* ix, const float* q, int64_t nq, const float* grad_out, const float* level_w,
                              int n_w, float* grad_q, float* grad_w, void* stream) {
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  if (grad_w && ix->max_depth + 1 > kLwMaxLevels) return fail(CWQ_ERR_ARG, "weight gradient: tree deeper than 64 levels");
  const GradPlan gp = grad_plan(ix);
  const int NL = ix->NL;
  const size_t lw_q = grad_w ? (size_t)std::max(NL, 1) * 4 + lw_grad_bytes_per_q(ix) : 0;
  const int64_t cq = std::min<int64_t>(chunk_queries(ix, nq, gp.per_q + lw_q, false), 4096);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    const int qtiles = (nqc + kXQ - 1) / kXQ;
    const size_t nq16 = (size_t)qtiles * kXQ;
    if ((rc = ix->reserve(nq16 * gp.per_q + 8 * 256 + lw_operand_bytes(ix, level_w) +
                          (grad_w ? chunk_bytes(ix, nq_pad, false) + (size_t)nq_pad * std::max(NL, 1) * 4 +
                                        nq16 * lw_grad_bytes_per_q(ix) + 8 * 256
                                  : 0))))
      return rc;
    Bump b(ix->ws.p, ix->ws.size);
    GradCoefArgs ca;
    float* part = grad_carve(ix, gp, b, nqc, qtiles, ca);
    if ((rc = lw_operands(ix, b, level_w, n_w, &ca.meta, &ca.w_int, s))) return rc;
    ca.G = grad_out + q0 * ix->n_sent;
    HIPCHK(launch_grad_coef(ca, s));
    if (grad_q && (rc = grad_streams(ix, gp, ca, part, q + q0 * ix->D, nqc, qtiles, grad_q + q0 * ix->D, s))) return rc;
    if (!grad_w) continue;
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    float* sraw = b.take<float>((size_t)nq_pad * std::max(NL, 1));
    double* lwp = b.take<double>(nq16 * lw_grad_bytes_per_q(ix) / 8);
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false))) return rc;
    if ((rc = run_leaf_scan(ix, c, EPI_RAW, false, 16, 0.f, sraw, NL, nullptr, nullptr, nullptr, 1, nullptr, s)))
      return rc;
    if ((rc = lw_grad(ix, c, ca, sraw, false, lwp, n_w, grad_w + q0 * n_w, s))) return rc;
  }
  return CWQ_OK;
}

// Cross-entropy ranking loss over all sentence scores with its gradient, the target's score
// and rank (cwq_loss.hip): the exact scan's row keys stay in the workspace,
// the softmax goes straight into the backward's coefficient layout.
int rank_ce_impl(cwq_index* ix, const float* q, int64_t nq, const int64_t* target, float temperature,
                 const float* level_w, int n_w, float* loss, float* grad_q, float* grad_w, float* target_score,
                 int64_t* rank, void* stream) {
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  if (grad_w && ix->max_depth + 1 > kLwMaxLevels) return fail(CWQ_ERR_ARG, "weight gradient: tree deeper than 64 levels");
  const int NL = ix->NL;
  const int npart = (NL + kCePart - 1) / kCePart;
  const GradPlan gp = grad_plan(ix);
  const bool grad = grad_q || grad_w;
  // per query: its row keys, the partials and (m, 1/z, row); the backward's arrays when wanted;
  // the rows' raw sums and the fp64 partial lines of the weight gradient
  const size_t ce_q = (size_t)std::max(npart, 1) * 12 + 12;
  const size_t lw_q = grad_w ? (size_t)std::max(NL, 1) * 4 + lw_grad_bytes_per_q(ix) : 0;
  const size_t per_q = (size_t)std::max(NL, 1) * 4 + ce_q + (grad ? gp.per_q : 0) + lw_q;
  const int64_t cq = std::min<int64_t>(chunk_queries(ix, nq, per_q, false), 4096);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    const int qtiles = (nqc + kXQ - 1) / kXQ;
    const size_t nq16 = (size_t)qtiles * kXQ;
    if ((rc = ix->reserve(chunk_bytes(ix, nq_pad, false) + (size_t)nq_pad * std::max(NL, 1) * 4 + nq16 * ce_q +
                          (grad ? nq16 * gp.per_q : 0) + 24 * 256 + lw_operand_bytes(ix, level_w) +
                          (grad_w ? (size_t)nq_pad * std::max(NL, 1) * 4 + nq16 * lw_grad_bytes_per_q(ix) + 4 * 256
                                  : 0))))
      return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    float* rowkey = b.take<float>((size_t)nq_pad * std::max(NL, 1));
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
    if ((rc = lw_operands(ix, b, level_w, n_w, &c.meta, &c.w_int, s))) return rc;
    // the weight gradient reads every row's lp': the scan writes it beside the key (EPI_KEYLP)
    float* rowlp = grad_w ? b.take<float>((size_t)nq_pad * std::max(NL, 1)) : nullptr;
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false))) return rc;
    if ((rc = run_leaf_scan(ix, c, grad_w ? EPI_KEYLP : EPI_KEY, false, 16, 0.f, rowkey, NL, rowlp, nullptr, nullptr, 1,
                            nullptr, s)))
      return rc;
    HIPCHK(launch_ce_reduce(a, s));
    if (!grad) continue;
    GradCoefArgs ca;
    float* part = grad_carve(ix, gp, b, nqc, qtiles, ca);
    ca.meta = c.meta;
    ca.w_int = c.w_int;
    HIPCHK(launch_ce_coef(a, ca.meta, ix->NL_iso, ca.coefL, ca.hL, s));
    HIPCHK(launch_grad_tree(ca, s));
    if (grad_q && (rc = grad_streams(ix, gp, ca, part, q + q0 * ix->D, nqc, qtiles, grad_q + q0 * ix->D, s))) return rc;
    if (!grad_w) continue;
    double* lwp = b.take<double>(nq16 * lw_grad_bytes_per_q(ix) / 8);
    if ((rc = lw_grad(ix, c, ca, rowlp, true, lwp, n_w, grad_w + q0 * n_w, s))) return rc;
  }
  return CWQ_OK;
}
}  // namespace

extern "C" int cwq_rank_scores_backward(cwq_index* ix, const float* q, int64_t nq, const float* grad_out,
                                        float* grad_q, void* stream) {
  if (!ix || !q || !grad_out || !grad_q) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  return rank_scores_backward_impl(ix, q, nq, grad_out, nullptr, 0, grad_q, nullptr, stream);
}

extern "C" int cwq_rank_scores_backward_w(cwq_index* ix, const float* q, int64_t nq, const float* grad_out,
                                          const float* level_w, int32_t n_w, float* grad_q, float* grad_w,
                                          void* stream) {
  if (!ix || !q || !grad_out || (!grad_q && !grad_w)) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  if (int rc = lw_check(level_w, n_w)) return rc;
  return rank_scores_backward_impl(ix, q, nq, grad_out, level_w, n_w, grad_q, n_w > 0 ? grad_w : nullptr, stream);
}

extern "C" int cwq_rank_ce(cwq_index* ix, const float* q, int64_t nq, const int64_t* target, float temperature,
                           float* loss, float* grad_q, float* target_score, int64_t* rank, void* stream) {
  if (!ix || !q || !target || !loss) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  if (!std::isfinite(temperature) || !(temperature > 0.f))
    return fail(CWQ_ERR_ARG, "temperature must be finite and > 0");
  return rank_ce_impl(ix, q, nq, target, temperature, nullptr, 0, loss, grad_q, nullptr, target_score, rank, stream);
}

extern "C" int cwq_rank_ce_w(cwq_index* ix, const float* q, int64_t nq, const int64_t* target, float temperature,
                             const float* level_w, int32_t n_w, float* loss, float* grad_q, float* grad_w,
                             float* target_score, int64_t* rank, void* stream) {
  if (!ix || !q || !target || !loss) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq < 0) return fail(CWQ_ERR_ARG, "nq < 0");
  if (int rc = lw_check(level_w, n_w)) return rc;
  if (!std::isfinite(temperature) || !(temperature > 0.f))
    return fail(CWQ_ERR_ARG, "temperature must be finite and > 0");
  return rank_ce_impl(ix, q, nq, target, temperature, level_w, n_w, loss, grad_q, n_w > 0 ? grad_w : nullptr,
                      target_score, rank, stream);
}

extern "C" int cwq_node_logprob(cwq_index* ix, const float* q, int64_t nq, int32_t full, float* out, void* stream) {
  if (!ix || (!q && nq > 0) || (!out && nq > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  const float dconst = full ? (float)((double)ix->D * (double)logf(2.0f * (float)M_PI)) : 0.f;
  const int64_t cq = chunk_queries(ix, nq, (size_t)ix->NL * 4);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    if ((rc = ix->reserve(chunk_bytes(ix, nq_pad) + (size_t)nq_pad * std::max(ix->NL, 1) * 4 + 8 * 256))) return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc);
    float* sleaf = b.take<float>((size_t)nq_pad * std::max(ix->NL, 1));
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s))) return rc;
    if ((rc = run_leaf_scan(ix, c, EPI_RAW, false, 16, 0.f, sleaf, ix->NL, nullptr, nullptr, nullptr, 1, nullptr, s)))
      return rc;
    HIPCHK(launch_node_lp(c.S_int ? c.S_int : ix->dummy, std::max(ix->NI, 1), sleaf, std::max(ix->NL, 1), nqc,
                          ix->node_src, ix->logdet_int, ix->logdet_row, dconst, ix->n_nodes, out + q0 * ix->n_nodes, s));
  }
  return CWQ_OK;
}

extern "C" int cwq_prefix_bounds(cwq_index* ix, const float* q, int64_t nq, float* lo, float* hi, float* exact,
                                 void* stream) {
  if (!ix || !q || !lo || !hi || !exact) return fail(CWQ_ERR_ARG, "NULL argument");
  if (nq <= 0 || nq > 4096) return fail(CWQ_ERR_ARG, "nq must be in [1, 4096]");
  if (!ix->int_bounds)
    return fail(CWQ_ERR_ARG, "no internal-node bounds on this index (flat tree, no isotropic leaf rows or too deep)");
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  if (call.rc) return call.rc;
  const int64_t nq_pad = round_up(nq, kQPad), nqf = round_up(nq, kFgTile);
  int rc;
  if ((rc = ix->reserve(chunk_bytes(ix, nq_pad, false) + int_bounds_bytes(ix, nqf) + 64 * 256))) return rc;
  Bump b(ix->ws.p, ix->ws.size);
  Chunk c;
  carve_chunk(ix, b, c, (int)nq, false);
  const size_t n = (size_t)nq * ix->NI * 4;
  HIPCHK(launch_pad_queries(q, nq, ix->D, c.X, c.nq_pad, ix->DP, s));
  if ((rc = run_internal(ix, c, s, false))) return rc;
  HIPCHK(hipMemcpyAsync(exact, c.P, n, hipMemcpyDeviceToDevice, s));
  const size_t nall = (size_t)c.nq_pad * ix->NI * 4;
  HIPCHK(hipMemsetAsync(c.P, 0xff, nall, s));   // NaN where the bound pass writes nothing
  HIPCHK(hipMemsetAsync(c.S_int, 0xff, nall, s));
  if ((rc = run_internal_bounds(ix, c, q, nqf, b, s))) return rc;
  const PathB pb = path_b(ix, c);
  if (pb.dot) {   // path-sum dots, node-major [NI][nq_pad] -> bounds [nq][NI]
    HIPCHK(launch_pathb_expand(pb, (int)nq, ix->NI, lo, hi, s));
  } else if (c.pT) {   // node-major [NI][nq_pad] -> [nq][NI]
    HIPCHK(launch_transpose(c.P, ix->NI, nq, c.ldP, lo, ix->NI, s));
    HIPCHK(launch_transpose(c.S_int, ix->NI, nq, c.ldP, hi, ix->NI, s));
  } else {
    HIPCHK(hipMemcpyAsync(lo, c.P, n, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(hi, c.S_int, n, hipMemcpyDeviceToDevice, s));
  }
  return CWQ_OK;
}
