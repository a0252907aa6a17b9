// Masked Fast top-k (no reference counterpart): the cwq_mask handle,
// cwq_score_topk_masked and cwq_score_topk_masked_multi.
// Calls the launch_mask_* kernels (cwq_mask.hip), the exact per-chunk passes and the unmasked
// Fast call (cwq_chunk.hip, cwq_topk.hip).
#include <atomic>
#include <map>

#include "cwq_handle.h"
#include "cwq_maskplan.h"

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
// the single-mask gathered scan's partial lists per query and segment, at most (the grouped
// scan's planner caps both segments together at kMpMaxSlabs, the same number)
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
constexpr int kMaskShqMaxQ = kMpShqMaxQ;

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

static int masked_single_locked(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, int32_t k, int64_t* ids,
                                float* scores, hipStream_t s);

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
  return masked_single_locked(ix, m, q, nq, k, ids, scores, s);
}

// cwq_score_topk_masked under the handle's lock (the multi call runs it per mask where a mask is
// better served as a call of its own; it starts the last call's stats anew each time)
static int masked_single_locked(cwq_index* ix, const cwq_mask* m, const float* q, int64_t nq, int32_t k, int64_t* ids,
                                float* scores, hipStream_t s) {
  for (int64_t& t : ix->mask_stats) t = 0;
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

// ---------------------------------------------------------------------------
// Per-query masks (cwq_score_topk_masked_multi)
// ---------------------------------------------------------------------------
namespace {

// Over-fetch widths of the multi call: a mask's k' is rounded up to the next of these, and each
// width runs one unmasked call over the queries of all its masks.  They follow the unmasked
// filter's cost steps (the comment at kMaskMaxKp): up to 32 a batch costs about the same, 40 is
// the batch cap, 64 the cap of calls of <= kMaskSmallQ queries.
constexpr int kMultiWidths[4] = {16, 32, 40, 64};
int multi_width(int kp) {
  for (int w : kMultiWidths)
    if (kp <= w) return w;
  return kMaskMaxKp;
}

struct MultiGroup {        // one distinct mask of the call
  const cwq_mask* m;
  std::vector<int> qi;     // its queries (positions in the call), ascending
  int width = 0;           // its over-fetch width; 0: none
  int kp = 0;              // the k' the rule gave it
  std::vector<int> scan;   // its queries for the gathered scan (planned there, or left short)
  bool own = false;        // it runs as a single-mask call of its own (masked_multi_impl)
};

// The device tables of one phase, packed on the host and sent with one copy: add() returns a
// table's offset (256-byte aligned) in the device region the blob is sent to.
struct Blob {
  std::vector<char> h;
  template <class T>
  size_t add(const std::vector<T>& v) {
    const size_t o = (h.size() + 255) & ~size_t(255);
    h.resize(o + v.size() * sizeof(T));
    if (!v.empty()) memcpy(h.data() + o, v.data(), v.size() * sizeof(T));
    return o;
  }
};
// The blobs of a call (pageable host memory): alive until the call has synchronised its stream.
struct Uploads {
  hipStream_t s;
  std::vector<std::unique_ptr<Blob>> keep;
  Blob& blob() {
    keep.emplace_back(new Blob());
    return *keep.back();
  }
  hipError_t send(const Blob& b, void* dst) {
    return b.h.empty() ? hipSuccess : hipMemcpyAsync(dst, b.h.data(), b.h.size(), hipMemcpyHostToDevice, s);
  }
};

bool mask_of_index(const cwq_index* ix, const cwq_mask* m) {
  return m->serial == ix->serial && m->n_sent == ix->n_sent && m->NL_iso == ix->NL_iso && m->NL_an == ix->NL_an;
}

// The grouped gathered scan of every group's `scan` queries (k <= 64): the plan of
// cwq_maskplan.h, then per chunk the staged queries, one exact internal pass, one scan launch
// per (segment, form) and one grouped merge.  tq: room for max_slots staged queries (the
// handle's mk buffer).
int multi_gathered(cwq_index* ix, const std::vector<MultiGroup>& gs, const float* q, int32_t k, int64_t* ids,
                   float* scores, float* tq, int64_t max_slots, Uploads& up, hipStream_t s) {
  const int K = std::min<int>(k, 64);
  const int kl = K <= 16 ? 16 : 64;
  std::vector<int> gidx;   // planner group -> gs
  std::vector<MpGroup> pg;
  for (size_t g = 0; g < gs.size(); ++g) {
    if (gs[g].scan.empty()) continue;
    gidx.push_back((int)g);
    pg.push_back(MpGroup{(int)gs[g].scan.size(), {gs[g].m->n_iso, gs[g].m->n_an}});
  }
  if (pg.empty()) return CWQ_OK;
  MpParams p;
  p.cus = ix->cus;
  p.K = K;
  p.entry_bytes = 12;
  p.slot_bytes = (chunk_bytes(ix, 2 * kQPad, false) - chunk_bytes(ix, kQPad, false)) / kQPad;
  p.budget = (size_t)chunk_queries(ix, INT_MAX, 0, false) * p.slot_bytes;
  MaskPlan plan;
  mask_plan(pg, p, plan);
  auto table_bytes = [](const MpChunk& ch) {
    size_t b = round_up((int64_t)(ch.queries.size() * sizeof(MaskMergeQ)), 256) + round_up((int64_t)ch.n_slots * 8, 256);
    for (int sg = 0; sg < 2; ++sg)
      for (int f = 0; f < 2; ++f) b += round_up((int64_t)(ch.work[sg][f].size() * sizeof(MaskWork)), 256);
    return b + 8 * 256;
  };
  size_t need = 0;
  for (const MpChunk& ch : plan.chunks) {
    if (ch.n_slots > max_slots) return fail(CWQ_ERR_HIP, "masked multi: staged queries past the buffer (internal error)");
    need = std::max(need, chunk_bytes(ix, round_up(ch.n_slots, kQPad), false) + 64 * 256 +
                              (size_t)ch.n_lists * K * 12 + table_bytes(ch));
  }
  int rc;
  if ((rc = ix->reserve(need))) return rc;
  for (MpChunk& ch : plan.chunks) {
    // the chunk's tables: the staged queries' positions in the call -- sorted by group, each piece
    // from a kXQ boundary; a gap repeats the piece's last query (no workgroup computes it: nvq
    // stops at the piece's end) -- the work items with their row lists, the merge's queries
    std::vector<int64_t> src((size_t)ch.n_slots);
    for (const MpPiece& pc : ch.pieces) {
      const std::vector<int>& sq = gs[gidx[pc.group]].scan;
      const int n = pc.qb - pc.qa, slots = (int)round_up(n, kMpXQ);
      for (int j = 0; j < slots; ++j) src[pc.slot + j] = sq[pc.qa + std::min(j, n - 1)];
    }
    Blob& tb = up.blob();
    const size_t o_src = tb.add(src);
    size_t o_w[2][2];
    for (int sg = 0; sg < 2; ++sg)
      for (int f = 0; f < 2; ++f) {
        for (MaskWork& it : ch.work[sg][f])
          it.list = sg ? gs[gidx[it.group]].m->rows_an : gs[gidx[it.group]].m->rows_iso;
        o_w[sg][f] = tb.add(ch.work[sg][f]);
      }
    for (MaskMergeQ& mq : ch.queries) {
      const MultiGroup& g = gs[gidx[mq.group]];
      mq.bits = g.m->bits;
      mq.orig = g.scan[mq.gidx];
    }
    const size_t o_mq = tb.add(ch.queries);
    // the whole carve, checked against the reservation before anything is launched
    Bump b(ix->ws.p, ix->ws.size);
    Chunk c;
    carve_chunk(ix, b, c, ch.n_slots, false);
    const size_t nent = (size_t)std::max<int64_t>(1, ch.n_lists) * K;
    float* pkey = b.take<float>(nent);
    float* paux = b.take<float>(nent);
    int* prow = b.take<int>(nent);
    char* dtab = b.take<char>(tb.h.size());
    if (b.off > ix->ws.size) return fail(CWQ_ERR_HIP, "masked multi: workspace estimate too small (internal error)");
    HIPCHK(up.send(tb, dtab));
    HIPCHK(launch_copy_rows(q, ix->D, (const int64_t*)(dtab + o_src), tq, ix->D, nullptr, ch.n_slots, ix->D, s));
    HIPCHK(launch_pad_queries(tq, ch.n_slots, ix->D, c.X, c.nq_pad, ix->DP, s));
    if ((rc = run_internal(ix, c, s, false, tq, -1))) return rc;   // exact prefixes, once for every group
    MaskScanArgs a;
    memset(&a, 0, sizeof(a));
    a.DP = ix->DP;
    a.nq = ch.n_slots;
    a.P = c.P ? c.P : ix->dummy;
    a.ldP = std::max(ix->NI, 1);
    a.dconst = 0.f;
    a.pkey = pkey;
    a.paux = paux;
    a.prow = prow;
    a.K = K;
    for (int sg = 0; sg < 2; ++sg) {
      a.seg_base = sg ? ix->NL_iso : 0;
      a.ld = sg ? ix->ld_an : 0;
      a.meta = ix->row_meta + a.seg_base;
      a.par = ix->row_par + a.seg_base;
      for (int f = 0; f < 2; ++f) {
        const std::vector<MaskWork>& w = ch.work[sg][f];
        if (w.empty()) continue;
        HIPCHK(launch_mask_scan_grouped(sg == 0, kl, f == 1, c.X, sg ? ix->an_A : ix->iso_Mf, sg ? ix->an_B : nullptr, a,
                                        (const MaskWork*)(dtab + o_w[sg][f]), (int)w.size(), s));
        ix->mask_multi_stats[4] += 1;
        ix->mask_multi_stats[5] += (int64_t)w.size();
      }
    }
    HIPCHK(launch_mask_merge_expand_multi(pkey, paux, prow, (const MaskMergeQ*)(dtab + o_mq), (int)ch.queries.size(), K, k, ix->sent_ptr,
                                          ix->sent_ids, ids, scores, s));
  }
  return CWQ_OK;
}

// The loop form: where the gathered scan's own work dwarfs what one call over all masks saves --
// the fixed cost of a single-mask call, kLoopCallMs each -- the masks run one after another
// through the single-mask call, each with the slab split and path of a call of its own.
// Work: the row-queries planned to the gathered scan over its rate.  The constants are fitted
// to one shape, C3 (flat 1M x 768 on MI355X, profiles/maskmulti_probe_c3.log): 0.28 - 0.4 ms per
// call in a loop over 1,000 masks; 14.4 G row-queries/s at DP = 768, taken as inversely
// proportional to DP (the scan's arithmetic and bytes per row-query are); the grouped form lost
// 2 - 50% from a work / saving ratio of 4.2 up (16 and 128 masks x 10,000 queries at allowed
// fraction 0.1 - 0.5) and won from 2.7 down.  Other devices and shapes have not been measured.
constexpr double kLoopCallMs = 0.3, kLoopScanRqPerMs768 = 14.4e6, kLoopRatio = 4.0;
// CWQ_MASK_MULTI_FORM, read per call: 1 grouped only (no loop form, no masks as calls of their
// own), 2 loop form, else the rules
int multi_form_env() {
  const char* e = getenv("CWQ_MASK_MULTI_FORM");
  const int v = e && *e ? atoi(e) : 0;
  return v == 1 || v == 2 ? v : 0;
}
bool multi_loop_form(const cwq_index* ix, const std::vector<MultiGroup>& gs) {
  if (multi_form_env()) return multi_form_env() == 2;
  if (mask_path_env()) return false;   // a forced path is a test of that path, grouped
  double rq = 0;
  for (const MultiGroup& g : gs)
    if (!g.width && !g.own) rq += (double)g.qi.size() * ((double)g.m->n_iso + g.m->n_an);
  const double rq_per_ms = kLoopScanRqPerMs768 * 768.0 / (double)std::max(ix->DP, 1);
  return rq / rq_per_ms > kLoopRatio * kLoopCallMs * (double)gs.size();
}

// Masks as single-mask calls of their own, one after another (every mask with a live row: the
// loop form; else those marked `own`): the mask's queries gathered into the handle's mg buffer,
// masked_single_locked, the rows scattered back.  Counts what each sub-call did into the multi
// stats [0], [2], [3]; acc: the widest k' and the short queries, for cwq_last_mask_stats.
int multi_own_calls(cwq_index* ix, const std::vector<MultiGroup>& gs, bool all, const float* q, int64_t nq, int32_t k,
                    int64_t* ids, float* scores, int64_t acc[2], Uploads& up, hipStream_t s) {
  int64_t* st = ix->mask_multi_stats;
  int64_t nmax = 0;
  std::vector<int64_t> idx;   // the sub-calls' queries (positions in the call), mask after mask: one upload
  for (const MultiGroup& g : gs)
    if ((all || g.own) && g.m->n_iso + g.m->n_an > 0) {
      nmax = std::max<int64_t>(nmax, (int64_t)g.qi.size());
      idx.insert(idx.end(), g.qi.begin(), g.qi.end());
    }
  if (nmax == 0) return CWQ_OK;
  const int64_t D = ix->D;
  const size_t o_idx = 0, o_tq = o_idx + round_up((int64_t)idx.size() * 8, 256), o_tid = o_tq + round_up(nmax * D * 4, 256),
               o_ts = o_tid + round_up(nmax * k * 8, 256), tot = o_ts + round_up(nmax * k * 4, 256);
  int rc;
  if ((rc = ix->mg.reserve(tot, ix->busy()))) return rc;
  char* mg = ix->mg.as<char>();
  Blob& tb = up.blob();
  tb.add(idx);
  HIPCHK(up.send(tb, mg + o_idx));
  const int64_t* didx = (const int64_t*)(mg + o_idx);
  float* tq = (float*)(mg + o_tq);
  int64_t* tid = (int64_t*)(mg + o_tid);
  float* ts = (float*)(mg + o_ts);
  // the buffers are reused from mask to mask in stream order: no synchronisation in between
  for (const MultiGroup& g : gs) {
    if (!(all || g.own) || g.m->n_iso + g.m->n_an == 0) continue;
    const int64_t n = (int64_t)g.qi.size();
    HIPCHK(launch_copy_rows(q, D, didx, tq, D, nullptr, n, D, s));
    scan_cfg_begin(n);   // the sub-call's own scan configuration
    rc = masked_single_locked(ix, g.m, tq, n, k, tid, ts, s);
    scan_cfg_begin(nq);
    if (rc) return rc;
    HIPCHK(launch_copy_rows(tid, 2 * (int64_t)k, nullptr, ids, 2 * (int64_t)k, didx, n, 2 * (int64_t)k, s));
    if (scores) HIPCHK(launch_copy_rows(ts, k, nullptr, scores, k, didx, n, k, s));
    // as between two calls: the next sub-call waits for this one's work only if it has to free
    // and grow one of the handle's buffers (cwq_index::busy)
    if ((rc = ix->ws_end(s))) return rc;
    didx += n;
    if (ix->mask_stats[0] == 1) {
      st[0] += n - ix->mask_stats[2];
      st[2] += ix->mask_stats[2];
      acc[0] = std::max(acc[0], ix->mask_stats[1]);
      acc[1] += ix->mask_stats[2];
    } else {
      st[3] += n;
    }
  }
  return CWQ_OK;
}

// The multi call under the handle's lock.  order: the queries counting-sorted by distinct mask;
// gs: the distinct masks that queries name.
int masked_multi_impl(cwq_index* ix, std::vector<MultiGroup>& gs, const float* q, int64_t nq, int32_t k, int64_t* ids,
                      float* scores, hipStream_t s) {
  int64_t* st = ix->mask_multi_stats;
  Uploads up{s, {}};
  int rc;
  // ---- masks without a live row: -1 / -inf, never scanned ----
  std::vector<int> fill;
  int64_t live = 0;
  for (MultiGroup& g : gs) {
    live += (int64_t)g.m->n_iso + g.m->n_an;
    if (g.m->n_iso + g.m->n_an == 0) fill.insert(fill.end(), g.qi.begin(), g.qi.end());
  }
  ix->mask_stats[0] = 4;
  ix->mask_stats[3] = live;
  const int64_t D = ix->D;
  Blob& tb = up.blob();   // the tables of this phase, sent with one copy
  const size_t o_fill = tb.add(fill);
  if (k > 64) {
    // the sort path per mask on its gathered sub-batch (rare, and a full sort per query anyway)
    if ((rc = ix->mk.reserve(tb.h.size() + 256, ix->busy()))) return rc;
    HIPCHK(up.send(tb, ix->mk.p));
    HIPCHK(launch_mask_fill_rows(ids, scores, k, (const int*)(ix->mk.as<char>() + o_fill), (int)fill.size(), s));
    for (MultiGroup& g : gs) {
      if (g.m->n_iso + g.m->n_an == 0) continue;
      std::vector<int64_t> qi(g.qi.begin(), g.qi.end());
      if ((rc = redo_short(ix, g.m, q, qi, k, ids, scores, s))) return rc;
      st[7] += (int64_t)qi.size();
    }
    HIPCHK(hipStreamSynchronize(s));
    return CWQ_OK;
  }
  // ---- the class of every mask, by the single-mask rule at the call's whole nq ----
  const int forced = mask_path_env();
  int widths[4] = {kMultiWidths[0], kMultiWidths[1], kMultiWidths[2], kMultiWidths[3]};
  int64_t n_w[4] = {0, 0, 0, 0}, n_ov = 0, n_ovw = 0, n_scan_max = 0;
  int n_groups_scan = 0, w_max = 0;
  for (MultiGroup& g : gs) {
    if (g.m->n_iso + g.m->n_an == 0) continue;
    int kp = overfetch_kp(ix, g.m, k, nq);
    const int path = forced ? forced : kp > 0 ? 1 : 2;
    if (path == 1 && kp == 0) kp = kMaskMaxKp;
    g.width = path == 1 ? multi_width(kp) : 0;
    g.kp = path == 1 ? kp : 0;
    w_max = std::max(w_max, g.kp);
    // The rule at the whole nq caps a batch's k' at kMaskMaxKpBatch; a mask with <= kMaskSmallQ
    // queries of its own that the rule over-fetches as a call of that size (cap kMaskMaxKp)
    // would go to the gathered scan over most of the corpus here.  It runs as a call of its own
    // (measured on C3, 1,000 masks x 10,000 queries at allowed fraction 0.5: 567 ms grouped,
    // 423 ms as 1,000 calls; the rows are the same either way).
    g.own = !g.width && !forced && multi_form_env() != 1 && overfetch_kp(ix, g.m, k, (int64_t)g.qi.size()) > 0;
    if (g.own) continue;
    if (!g.width) {
      g.scan = g.qi;
      st[3] += (int64_t)g.qi.size();
    }
    n_scan_max += (int64_t)g.qi.size();   // every query may end in the gathered scan
    ++n_groups_scan;
  }
  const bool loop = multi_loop_form(ix, gs);
  if (loop) st[3] = 0;   // counted per sub-call
  int64_t acc[2] = {0, 0};
  if ((rc = multi_own_calls(ix, gs, loop, q, nq, k, ids, scores, acc, up, s))) return rc;
  ix->mask_stats[0] = 4;   // the sub-calls wrote their own
  ix->mask_stats[1] = acc[0];
  ix->mask_stats[2] = acc[1];
  ix->mask_stats[3] = live;
  if (loop)   // no shared widths, no grouped launches: [1], [4] and [5] stay 0
    for (MultiGroup& g : gs) g.width = 0, g.scan.clear();
  for (MultiGroup& g : gs) {
    if (!g.width) continue;
    // a small call's unmasked filter grows smoothly with k' (the comment at kMaskMaxKp): one
    // call at the widest k' of its masks, unrounded, costs less than one per width
    if (nq <= kMaskSmallQ) g.width = widths[3] = w_max, widths[0] = widths[1] = widths[2] = 0;
    for (int i = 0; i < 4; ++i)
      if (widths[i] == g.width) {
        n_w[i] += (int64_t)g.qi.size();
        break;
      }
  }
  // the over-fetch queries width by width: their positions in the call (gather and result row)
  // and their mask slots
  std::vector<int64_t> src;
  std::vector<int> qs, qo;
  for (int i = 0; i < 4; ++i) {
    if (!n_w[i]) continue;
    for (size_t g = 0; g < gs.size(); ++g) {
      if (gs[g].width != widths[i]) continue;
      for (int o : gs[g].qi) {
        src.push_back(o);
        qs.push_back((int)g);
        qo.push_back(o);
      }
    }
    n_ov += n_w[i];
    n_ovw = std::max(n_ovw, n_w[i] * widths[i]);
    st[1] += 1;
    ix->mask_stats[1] = std::max<int64_t>(ix->mask_stats[1], widths[i]);
  }
  st[0] += n_ov;
  std::vector<MaskSlot> slots(n_ov ? gs.size() : 0);
  for (size_t g = 0; g < slots.size(); ++g) slots[g] = MaskSlot{gs[g].m->bits, gs[g].m->n_allowed};
  const size_t o_src = tb.add(src), o_qs = tb.add(qs), o_qo = tb.add(qo), o_sl = tb.add(slots);
  // ---- the handle's mk buffer: tables, flags, the unmasked results, the gathered queries ----
  const int64_t max_slots = n_scan_max + (int64_t)(kMpXQ - 1) * n_groups_scan;
  const int64_t n_stage = std::max<int64_t>(1, std::max(n_ov, max_slots));
  const size_t o_fl = round_up((int64_t)tb.h.size() + 1, 256), o_tid = o_fl + round_up(nq * 4, 256),
               o_ts = o_tid + round_up(n_ovw * 8 + 8, 256), o_tq = o_ts + round_up(n_ovw * 4 + 4, 256),
               tot = o_tq + round_up(n_stage * D * 4, 256);
  if ((rc = ix->mk.reserve(tot, ix->busy()))) return rc;
  char* mk = ix->mk.as<char>();
  int* flag = (int*)(mk + o_fl);
  int64_t* tid = (int64_t*)(mk + o_tid);
  float* ts = (float*)(mk + o_ts);
  float* tq = (float*)(mk + o_tq);
  HIPCHK(up.send(tb, mk));
  HIPCHK(launch_mask_fill_rows(ids, scores, k, (const int*)(mk + o_fill), (int)fill.size(), s));
  // ---- over-fetch: one unmasked call per width over the queries of all its masks ----
  if (n_ov > 0) {
    HIPCHK(hipMemsetAsync(flag, 0, (size_t)nq * 4, s));
    HIPCHK(launch_copy_rows(q, D, (const int64_t*)(mk + o_src), tq, D, nullptr, n_ov, D, s));
    int64_t q0 = 0;
    for (int i = 0; i < 4; ++i) {
      if (!n_w[i]) continue;
      const int W = widths[i];
      const int64_t n = n_w[i];
      scan_cfg_begin(n);   // the sub-call's own scan configuration
      rc = score_topk_unmasked(ix, tq + q0 * D, n, W, tid, ts, s);
      scan_cfg_begin(nq);
      if (rc) return rc;
      HIPCHK(launch_mask_overfetch_multi(tid, ts, (int)n, W, k, (const MaskSlot*)(mk + o_sl), (const int*)(mk + o_qs) + q0,
                                         (const int*)(mk + o_qo) + q0, ids, scores, flag, s));
      q0 += n;
    }
    // the short flags of every width, read back once
    if ((rc = ix->hflags.reserve((size_t)nq * sizeof(int)))) return rc;
    HIPCHK(hipMemcpyAsync(ix->hflags.p, flag, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int* hflag = ix->hflags.as<int>();
    int64_t n_short = 0;
    for (MultiGroup& g : gs) {
      if (!g.width) continue;
      for (int o : g.qi)
        if (hflag[o]) g.scan.push_back(o);
      n_short += (int64_t)g.scan.size();
    }
    st[0] -= n_short;   // answered by the over-fetch leg: not the short ones
    st[2] += n_short;
    ix->mask_stats[2] = st[2];
  }
  // ---- the gathered scan, grouped ----
  if ((rc = multi_gathered(ix, gs, q, k, ids, scores, tq, n_stage, up, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));   // the uploads' host tables go with this frame
  ix->ws_idle = true;
  return CWQ_OK;
}

}  // namespace

namespace cwq {
// The masked Fast call under the handle's lock (cwq_handle.h); rc0: the caller's ws_begin result,
// returned once the stats are reset, as the entry points did.
int masked_topk_locked(cwq_index* ix, const cwq_mask* const* masks, int32_t n_masks, const int32_t* mask_of_query,
                       const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores, hipStream_t s, int rc0) {
  // counting sort by distinct mask (a mask named by two slots is one group)
  std::vector<int> group_of_slot((size_t)n_masks, -1);
  std::vector<MultiGroup> gs;
  {
    std::map<const cwq_mask*, int> seen;
    std::vector<char> used((size_t)n_masks, 0);
    if (!mask_of_query) used[0] = 1;
    for (int64_t i = 0; mask_of_query && i < nq; ++i) used[mask_of_query[i]] = 1;
    for (int32_t i = 0; i < n_masks; ++i) {
      if (!used[i]) continue;
      auto it = seen.find(masks[i]);
      if (it == seen.end()) {
        it = seen.emplace(masks[i], (int)gs.size()).first;
        gs.push_back(MultiGroup());
        gs.back().m = masks[i];
      }
      group_of_slot[i] = it->second;
    }
    if (gs.size() > 1)
      for (int64_t i = 0; i < nq; ++i) gs[group_of_slot[mask_of_query[i]]].qi.push_back((int)i);
  }
  topk_begin(ix);
  for (int64_t& t : ix->mask_stats) t = 0;
  for (int64_t& t : ix->mask_multi_stats) t = 0;
  ix->mask_multi_stats[6] = (int64_t)gs.size();
  if (rc0) return rc0;
  // one mask for every query: the single-mask call, its path and its stats
  if (gs.size() == 1) return masked_single_locked(ix, gs[0].m, q, nq, k, ids, scores, s);
  return masked_multi_impl(ix, gs, q, nq, k, ids, scores, s);
}
}  // namespace cwq

extern "C" int cwq_score_topk_masked_multi(cwq_index* ix, const cwq_mask* const* masks, int32_t n_masks,
                                           const int32_t* mask_of_query, const float* q, int64_t nq, int32_t k,
                                           int64_t* ids, float* scores, void* stream) {
  if (!ix || !masks || !mask_of_query || (!q && nq > 0) || (!ids && nq > 0)) return fail(CWQ_ERR_ARG, "NULL argument");
  if (n_masks < 1) return fail(CWQ_ERR_ARG, "n_masks must be >= 1");
  if (k <= 0) return fail(CWQ_ERR_ARG, "k must be >= 1");
  if (nq < 0 || nq > INT_MAX) return fail(CWQ_ERR_ARG, "nq must be in [0, 2^31)");
  for (int32_t i = 0; i < n_masks; ++i) {
    if (!masks[i]) return fail(CWQ_ERR_ARG, "masks[" + std::to_string(i) + "] is NULL");
    if (!mask_of_index(ix, masks[i])) return fail(CWQ_ERR_ARG, "the mask was built for another index");
  }
  for (int64_t i = 0; i < nq; ++i)
    if (mask_of_query[i] < 0 || mask_of_query[i] >= n_masks)
      return fail(CWQ_ERR_ARG, "mask_of_query[" + std::to_string(i) + "] = " + std::to_string(mask_of_query[i]) +
                                   " is outside [0, " + std::to_string(n_masks) + ")");
  if (nq == 0) return CWQ_OK;
  hipStream_t s = (hipStream_t)stream;
  QueryCall call(ix, nq, s);
  return masked_topk_locked(ix, masks, n_masks, mask_of_query, q, nq, k, ids, scores, s, call.rc);
}

extern "C" int cwq_last_mask_multi_stats(const cwq_index* ix, int64_t* out) {
  if (!ix || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  for (int i = 0; i < 8; ++i) out[i] = ix->mask_multi_stats[i];
  return CWQ_OK;
}
