// Masked Fast top-k (no reference counterpart): the cwq_mask handle and
// cwq_score_topk_masked.  Calls the launch_mask_* kernels (cwq_mask.hip), the exact per-chunk
// passes and the unmasked Fast call of cwq_api.hip.
#include <atomic>

#include "cwq_handle.h"

namespace cwq {
uint64_t next_index_serial() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}
}  // namespace cwq

namespace {

// ---- the path rule ----
// Over-fetch serves a call when the unmasked top-k' at some k' <= the cap is expected to hold
// kMaskSlack * k allowed sentences (allowed fraction f: k' = ceil(kMaskSlack * k / f)); below
// that fraction most queries would come up short and be redone, so the call goes straight to
// the gathered scan.  kMaskSlack: the queries' allowed counts among the top-k' spread around
// f * k' (binomially for a mask that is independent of the ranking), and 2x keeps the short
// queries rare (at k = 10: 4 to 7 of 10,000 queries redone at f = 0.5).
// The cap is what the unmasked call costs by k', measured on C3 (flat 1M x 768, top-10;
// profiles/mask_probe_c3.log): calls of <= 64 queries (the stream filter) grow smoothly, 0.23 ms
// at k' = 10 to 0.33 ms at 64 for one query, so any k' <= 64 is worth trying; the batch filter
// costs 11.1 ms at k' = 10, 12.9 ms at 32, 77 ms at 40 and 628 ms from 48 on for 10,000 queries
// (its candidate lists overflow and the queries are re-run exactly), against 70 ms per 0.1 of
// allowed fraction for the gathered scan -- so a batch over-fetches up to k' = 40 and no further.
constexpr int kMaskMaxKp = 64;        // kFiltMaxK: the unmasked filter paths serve k <= 64
constexpr int kMaskMaxKpBatch = 40;   // calls of more than kMaskSmallQ queries
constexpr int kMaskSmallQ = kStreamMaxQ;   // up to here the unmasked call is the stream filter's
constexpr double kMaskSlack = 2.0;
// the gathered scan's partial lists per query, at most (per segment)
constexpr int kMaskMaxSlabs = 2048;

int mask_path_env() {
  const char* e = getenv("CWQ_MASK_PATH");
  const int v = e && *e ? atoi(e) : 0;
  return v == 1 || v == 2 ? v : 0;
}

// k' of the over-fetch path for this mask, k and call size; 0: the rule sends the call to the gathered scan
int overfetch_kp(const cwq_index* ix, const cwq_mask* m, int k, int64_t nq) {
  if (k > kMaskMaxKp || m->n_allowed <= 0 || ix->n_sent <= 0) return 0;
  if (m->n_allowed == ix->n_sent) return k;   // nothing masked: the unmasked call is the answer
  const double f = (double)m->n_allowed / (double)ix->n_sent;
  const double want = std::ceil(kMaskSlack * k / f);
  const int cap = std::max(k, nq <= kMaskSmallQ ? kMaskMaxKp : kMaskMaxKpBatch);
  return want <= cap ? std::max(k, (int)want) : 0;
}

// small calls take the gathered scan's shared-query form (the waves of a workgroup split the rows)
constexpr int kMaskShqMaxQ = 32;

// slabs of a segment's row list: enough workgroups for ~4 per CU, whole tiles
void slab_split(const cwq_index* ix, int n_live, int n_qblocks, bool shq, int& nslab, int& rps) {
  nslab = rps = 0;
  if (n_live <= 0) return;
  const int tile = mask_scan_tile(shq);
  const int tiles = (n_live + tile - 1) / tile;
  const int want = (int)std::min<int64_t>(kMaskMaxSlabs / mask_scan_lists(shq),
                                          std::max<int64_t>(1, (int64_t)4 * ix->cus / std::max(1, n_qblocks)));
  const int n = std::min(tiles, want);
  rps = (tiles + n - 1) / n * tile;
  nslab = (n_live + rps - 1) / rps;
}

// The gathered path: exact keys of the mask's live rows only (k <= 64: partial top-K lists,
// merged and expanded under the bitset; k > 64: every row's key, the rows that are not live
// set to -inf, full sort, masked expansion).
int masked_exact_impl(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, int32_t k, int64_t* ids,
                      float* scores, hipStream_t s) {
  const bool general = k > 64;
  const int K = std::min<int>(k, 64);
  const int kl = K <= 16 ? 16 : 64;
  const int n_pow2 = (int)std::max<int64_t>(2, 1LL << (int)ceil(log2((double)std::max(ix->NL, 2))));
  // the slab split is fixed from the call's query count, so every chunk's lists fit the estimate
  const bool shq = nq <= kMaskShqMaxQ;
  const int qpb = shq ? kXQ : kXQ * kWavesPerWG, lps = mask_scan_lists(shq);
  const int nqb_call = (int)std::min<int64_t>((nq + qpb - 1) / qpb, INT_MAX);
  int ns_iso, rps_iso, ns_an, rps_an;
  slab_split(ix, m->n_iso, nqb_call, shq, ns_iso, rps_iso);
  slab_split(ix, m->n_an, nqb_call, shq, ns_an, rps_an);
  const int nst = std::max(1, (ns_iso + ns_an) * lps);
  const size_t extra = general ? (size_t)ix->NL * 4 + (size_t)n_pow2 * 8 : (size_t)nst * K * 12;
  const int64_t cq = chunk_queries(ix, nq, extra, false);
  int rc;
  for (int64_t q0 = 0; q0 < nq; q0 += cq) {
    const int nqc = (int)std::min(cq, nq - q0);
    const int64_t nq_pad = round_up(nqc, kQPad);
    const size_t need = chunk_bytes(ix, nq_pad, false) + 64 * 256 + (size_t)nq_pad * extra;
    if ((rc = ix->reserve(need))) return rc;
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, nqc, false);
    HIPCHK(launch_pad_queries(q + q0 * ix->D, nqc, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false, q + q0 * ix->D, -1))) return rc;   // exact prefixes, as the unfiltered path
    int64_t* oid = ids + q0 * k;
    float* osc = scores ? scores + q0 * k : nullptr;
    if (general) {
      float* rowkey = b.take<float>((size_t)nq_pad * std::max(ix->NL, 1));
      float* skey = b.take<float>((size_t)nq_pad * n_pow2);
      int* srow = b.take<int>((size_t)nq_pad * n_pow2);
      if ((rc = run_leaf_scan(ix, c, EPI_KEY, false, 16, 0.f, rowkey, ix->NL, nullptr, nullptr, nullptr, 1, nullptr, s)))
        return rc;
      HIPCHK(launch_mask_kill(rowkey, ix->NL, nqc, ix->NL, m->live, s));
      HIPCHK(launch_init_rows(rowkey, ix->NL, nqc, ix->NL, n_pow2, skey, srow, s));
      HIPCHK(launch_sort_rows(skey, srow, nqc, ix->NL, n_pow2, s));
      HIPCHK(launch_mask_expand(skey, srow, nqc, n_pow2, k, ix->sent_ptr, ix->sent_ids, m->bits, oid, osc, s));
      continue;
    }
    float* pkey = b.take<float>((size_t)nq_pad * nst * K);
    float* paux = b.take<float>((size_t)nq_pad * nst * K);
    int* prow = b.take<int>((size_t)nq_pad * nst * K);
    MaskScanArgs a;
    memset(&a, 0, sizeof(a));
    a.DP = ix->DP;
    a.nq = nqc;
    a.n_qblocks = (nqc + qpb - 1) / qpb;
    a.P = c.P ? c.P : ix->dummy;
    a.ldP = std::max(ix->NI, 1);
    a.dconst = 0.f;
    a.pkey = pkey;
    a.paux = paux;
    a.prow = prow;
    a.nslab_total = nst;
    a.K = K;
    if (m->n_iso > 0) {
      a.n_live = m->n_iso;
      a.rows_per_slab = rps_iso;
      a.seg_base = 0;
      a.list = m->rows_iso;
      a.meta = ix->row_meta;
      a.par = ix->row_par;
      a.slab_off = 0;
      HIPCHK(launch_mask_scan(true, kl, shq, c.X, ix->iso_Mf, nullptr, a, ns_iso, s));
    }
    if (m->n_an > 0) {
      a.n_live = m->n_an;
      a.rows_per_slab = rps_an;
      a.seg_base = ix->NL_iso;
      a.list = m->rows_an;
      a.ld = ix->ld_an;
      a.meta = ix->row_meta + ix->NL_iso;
      a.par = ix->row_par + ix->NL_iso;
      a.slab_off = ns_iso * lps;
      HIPCHK(launch_mask_scan(false, kl, shq, c.X, ix->an_A, ix->an_B, a, ns_an, s));
    }
    HIPCHK(launch_mask_merge_expand(pkey, paux, prow, nqc, nst * K, K, k, ix->sent_ptr, ix->sent_ids, m->bits, oid, osc,
                                    s));
  }
  return CWQ_OK;
}

// The queries the over-fetch left short: gathered, through the gathered scan, scattered back
// (rerun_exact's shape; the buffers are the handle's fallback region).
int redo_short(cwq_index* ix, const cwq_mask* m, const float* q, const std::vector<int64_t>& qi, int32_t k,
               int64_t* ids, float* scores, hipStream_t s) {
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
  if ((rc = masked_exact_impl(ix, m, tq, n, k, tid, ts, s))) return rc;
  if ((rc = g.scatter(tid, 2 * (int64_t)k, ids)) || (scores && (rc = g.scatter(ts, k, scores)))) return rc;
  return g.close();
}

}  // namespace

extern "C" int cwq_mask_create(cwq_index* ix, const uint32_t* bits, int64_t n_sent, void* stream, cwq_mask** out) {
  if (!ix || !out || (!bits && n_sent > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  *out = nullptr;
  if (n_sent != ix->n_sent)
    return fail(CWQ_ERR_ARG, "mask length " + std::to_string(n_sent) + " != the index's " + std::to_string(ix->n_sent) +
                                 " sentences");
  hipStream_t s = (hipStream_t)stream;
  DevGuard dg(ix->device);
  std::unique_ptr<cwq_mask> m(new cwq_mask());
  m->serial = ix->serial;
  m->device = ix->device;
  m->n_sent = n_sent;
  m->NL_iso = ix->NL_iso;
  m->NL_an = ix->NL_an;
  const size_t words = (size_t)std::max<int64_t>(1, (n_sent + 31) / 32);
  const int nb = (std::max(ix->NL_iso, ix->NL_an) + 1023) / 1024 + 1;
  const size_t o_bits = 0, o_live = o_bits + round_up(words * 4, 256), o_ri = o_live + round_up(std::max(ix->NL, 1), 256),
               o_ra = o_ri + round_up((int64_t)std::max(ix->NL_iso, 1) * 4, 256),
               o_bc = o_ra + round_up((int64_t)std::max(ix->NL_an, 1) * 4, 256), o_cnt = o_bc + round_up((int64_t)nb * 4, 256),
               tot = o_cnt + 256;
  if (hipMalloc(&m->mem, tot) != hipSuccess)
    return fail(CWQ_ERR_OOM, "mask hipMalloc failed (" + std::to_string(tot) + " B)");
  m->bytes = tot;
  char* base = (char*)m->mem;
  m->bits = (uint32_t*)(base + o_bits);
  m->live = (uint8_t*)(base + o_live);
  m->rows_iso = (int*)(base + o_ri);
  m->rows_an = (int*)(base + o_ra);
  int* bc = (int*)(base + o_bc);
  unsigned long long* d_allowed = (unsigned long long*)(base + o_cnt);
  int* d_counts = (int*)(base + o_cnt + 8);
  HIPCHK(hipMemsetAsync(m->bits, 0, words * 4, s));
  if (n_sent > 0) HIPCHK(hipMemcpyAsync(m->bits, bits, (size_t)((n_sent + 31) / 32) * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(launch_mask_build(m->bits, ix->sent_ptr, ix->sent_ids, ix->row_flags, ix->NL_iso, ix->NL_an, m->live,
                           m->rows_iso, m->rows_an, bc, d_allowed, d_counts, s));
  unsigned long long h_allowed = 0;
  int h_counts[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&h_allowed, d_allowed, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_counts, d_counts, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  m->n_allowed = (int64_t)h_allowed;
  m->n_iso = h_counts[0];
  m->n_an = h_counts[1];
  if (m->n_iso < 0 || m->n_iso > ix->NL_iso || m->n_an < 0 || m->n_an > ix->NL_an)
    return fail(CWQ_ERR_HIP, "mask build: row counts out of range (internal error)");
  *out = m.release();
  return CWQ_OK;
}

extern "C" int cwq_mask_destroy(cwq_mask* m) {
  delete m;
  return CWQ_OK;
}

extern "C" int cwq_mask_info(const cwq_mask* m, int64_t* o) {
  if (!m || !o) return fail(CWQ_ERR_ARG, "NULL argument");
  o[0] = m->n_allowed;
  o[1] = m->n_iso;
  o[2] = m->n_an;
  o[3] = (int64_t)m->bytes;
  return CWQ_OK;
}

extern "C" int cwq_score_topk_masked(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, int32_t k,
                                     int64_t* ids, float* scores, void* stream) {
  if (!ix || !m || (!q && nq > 0) || (!ids && nq > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  if (k <= 0) return fail(CWQ_ERR_ARG, "k must be >= 1");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  if (m->serial != ix->serial || m->n_sent != ix->n_sent || m->NL_iso != ix->NL_iso || m->NL_an != ix->NL_an)
    return fail(CWQ_ERR_ARG, "the mask was built for another index");
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  topk_begin(ix);
  for (int64_t& t : ix->mask_stats) t = 0;
  if (call.rc) return call.rc;
  // the path: k > 64 always sorts; else CWQ_MASK_PATH (read per call) or the rule
  const int forced = mask_path_env();
  int kp = overfetch_kp(ix, m, k, nq);
  int path = k > 64 ? 3 : forced ? forced : kp > 0 ? 1 : 2;
  if (path == 1 && kp == 0) kp = kMaskMaxKp;   // forced over-fetch below the rule's fraction: the widest k'
  ix->mask_stats[0] = path;
  ix->mask_stats[1] = path == 1 ? kp : 0;
  ix->mask_stats[3] = (int64_t)m->n_iso + m->n_an;
  if (m->n_iso + m->n_an == 0) {   // nothing is allowed: no scan
    HIPCHK(launch_mask_fill(ids, scores, nq * (int64_t)k, s));
    return CWQ_OK;
  }
  if (path != 1) return masked_exact_impl(ix, m, q, nq, k, ids, scores, s);

  // over-fetch: the unmasked Fast call at k' into the handle's buffers, compaction, the short
  // queries through the gathered scan
  const size_t o_ts = round_up(nq * (int64_t)kp * 8, 256), o_fl = o_ts + round_up(nq * (int64_t)kp * 4, 256),
               tot = o_fl + round_up(nq * 4, 256);
  int rc;
  if ((rc = ix->mk.reserve(tot, ix->busy()))) return rc;
  int64_t* tid = ix->mk.as<int64_t>();
  float* ts = (float*)(ix->mk.as<char>() + o_ts);
  int* flag = (int*)(ix->mk.as<char>() + o_fl);
  if ((rc = score_topk_unmasked(ix, q, nq, kp, tid, ts, s))) return rc;
  HIPCHK(launch_mask_overfetch(tid, ts, (int)nq, kp, k, m->bits, m->n_allowed, ids, scores, flag, s));
  // the flags come back through the handle's mapped host buffer, like the filter's own
  // (the unmasked call is done with it)
  if ((rc = ix->hflags.reserve((size_t)nq * sizeof(int)))) return rc;
  HIPCHK(hipMemcpyAsync(ix->hflags.p, flag, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int* hflag = ix->hflags.as<int>();
  std::vector<int64_t> redo;
  for (int64_t i = 0; i < nq; ++i)
    if (hflag[i]) redo.push_back(i);
  ix->mask_stats[2] = (int64_t)redo.size();
  if (!redo.empty() && (rc = redo_short(ix, m, q, redo, k, ids, scores, s))) return rc;
  return CWQ_OK;
}

extern "C" int cwq_last_mask_stats(const cwq_index* ix, int64_t* out) {
  if (!ix || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  for (int i = 0; i < 4; ++i) out[i] = ix->mask_stats[i];
  return CWQ_OK;
}
