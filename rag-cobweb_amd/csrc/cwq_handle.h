// The query library's host layer behind the C ABI: the handle (struct cwq_index), the per-call
// scopes, the query chunk, and the declarations of the host functions that cross a file.
// Host only: included by cwq_api.hip, cwq_build.hip, cwq_chunk.hip, cwq_filter.hip, cwq_topk.hip,
// cwq_categorize.hip, cwq_rank.hip, cwq_fitcalls.hip, cwq_maskcalls.hip, cwq_sparsecalls.hip and
// cwq_masklosscalls.hip and by nothing else; the kernel sources share cwq_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cobweb_query.h"
#include "cwq_internal.h"

using namespace cwq;

namespace cwq {
int fail(int code, const std::string& msg);   // cwq_api.hip: sets cwq_last_error's message; returns code
}  // namespace cwq

#define HIPCHK(expr)                                                                                \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) return fail(CWQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace cwq {

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Bump allocator over the handle's workspace.
struct Bump {
  char* base;
  size_t off = 0, cap;
  Bump(void* b, size_t c) : base((char*)b), cap(c) {}
  template <class T>
  T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = (T*)(base + off);
    off += n * sizeof(T);
    return p;
  }
};

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// A grow-on-demand buffer of the handle: kept between calls, freed and allocated anew (rounded up
// to `round` bytes) when a call needs more than it holds.  busy: an event to wait for before the
// free -- earlier calls' kernels may still read a device buffer (cwq_index::busy).
struct GrowBuf {
  enum Kind { kDevice, kPinned, kMapped };   // hipMalloc / pinned host / mapped coherent host memory
  Kind kind;
  size_t round;
  const char* what;   // the error message; one that ends in '(' gets the size appended
  void* p = nullptr;
  size_t size = 0;
  template <class T>
  T* as() const {
    return (T*)p;
  }
  void release() {
    if (p) (void)(kind == kDevice ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    size = 0;
  }
  int reserve(size_t b, hipEvent_t busy = nullptr) {
    if (b <= size) return CWQ_OK;
    if (busy) (void)hipEventSynchronize(busy);
    release();
    b = (size_t)round_up((int64_t)b, (int64_t)round);
    const hipError_t e = kind == kDevice   ? hipMalloc(&p, b)
                         : kind == kPinned ? hipHostMalloc(&p, b, hipHostMallocDefault)
                                           : hipHostMalloc(&p, b, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) {
      std::string msg = what;
      if (msg.back() == '(') msg += std::to_string(b) + " B)";
      return fail(CWQ_ERR_OOM, msg);
    }
    size = b;
    return CWQ_OK;
  }
};

// A number no other index of this process has had: what a cwq_mask remembers of its index (an
// index pointer can come back for a new index once the old one is destroyed).
uint64_t next_index_serial();   // cwq_maskcalls.hip

}  // namespace cwq

struct cwq_index {
  uint64_t serial = cwq::next_index_serial();
  int device = 0;
  int64_t n_nodes = 0, n_sent = 0;
  int D = 0, DP = 0;
  int NI = 0, NL = 0, NL_iso = 0, NL_an = 0;
  int64_t ld_int = 0, ld_iso = 0, ld_an = 0;
  int max_depth = 0;
  int cus = 256;
  std::vector<std::pair<int, int>> levels;   // internal-node ranges, one per depth
  int* d_lv = nullptr;                       // device copy: level starts + end [levels + 1]
  int* sel_ctr = nullptr;                    // per-call path: fused select counter (probe with fused prep)
  float root_w0 = 0.f, root_logdet0 = 0.f;   // the root's w and logdet (host copies)
  std::vector<void*> allocs;
  size_t bytes = 0;
  // row data
  float *int_A = nullptr, *int_B = nullptr, *iso_M = nullptr, *an_A = nullptr, *an_B = nullptr;
  RowMeta* row_meta = nullptr;
  int *row_par = nullptr, *row_flags = nullptr, *row_bfs = nullptr;
  int *row_depth = nullptr, *int_depth = nullptr;   // depth of each leaf-class row / internal node (call-time level weights)
  float* logdet_row = nullptr;
  float *logdet_int = nullptr, *w_int = nullptr;
  int *par_int = nullptr, *int_child_begin = nullptr, *int_child_end = nullptr, *int_nchild = nullptr;
  int *int_bfs = nullptr, *int_has_sent = nullptr;
  bool any_int_sent = false;   // an internal node holds sentences (categorize: heap replay only)
  int *int_leaf_a0 = nullptr, *int_leaf_a1 = nullptr, *int_leaf_b0 = nullptr, *int_leaf_b1 = nullptr;
  int64_t *sent_ptr = nullptr, *sent_ids = nullptr;
  int* row_of_sent = nullptr;
  int* node_src = nullptr;
  float* dummy = nullptr;
  // bf16-MFMA filter operands for the isotropic rows (cwq_mfma.hip): row-major
  // fp32 (exact rerank, DP wide) and bf16 hi-part (GEMM, DPB wide) copies padded to
  // whole 256-row tiles, per-row / per-tile bound constants, the threshold sample
  int64_t ld_f = 0;
  int DPB = 0;
  float *iso_Mf = nullptr, *iso_c = nullptr;   // iso_c: centre [D] (root mean)
  uint16_t* iso_Mb = nullptr;
  RowF* iso_rf = nullptr;
  TileF* iso_tf = nullptr;
  // int8 operands of the stream filter pass (launch_rows_i8), built on the first small-batch
  // call: 0 not yet, 1 built, -1 off (CWQ_STREAM_I8=0, DPB % 64, or too little free memory)
  int8_t* iso_Mq = nullptr;
  RowF* iso_rf8 = nullptr;
  TileF* iso_tf8 = nullptr;   // iso_tf with the int8 tile maxima (the batch filter's int8 launches)
  int i8_state = 0;
  bool i8_by_size = false;   // the panel was built with the index by the size rule (ensure_i8), not by a knob
  // the batch filter's early int8 schedule (fg_i8_from) went back to the quarter rule: a call
  // on it passed too many candidates or re-ran a query (until cwq_set_filter)
  bool i8_early_off = false;
  bool i8_early_ran = false;   // the current call ran the early schedule
  std::vector<int> tile_uni_prefix;   // prefix counts of uniform row tiles (all_uniform per launch range)
  int n_multi_tiles = 0;              // tiles with several parents (TileF uniform 2)
  // the same tables for the categorize key min(BF[parent], lp) (cwq_categorize through the
  // filter): lp with the 2*pi constant, no prefix term (invL 0), the categorize usable rule
  RowF* cat_rf = nullptr;
  TileF* cat_tf = nullptr;
  std::vector<int> cat_uni_prefix;
  float cat_dconst = 0.f;
  int n_samp = 0, ld_s = 0;                    // sample rows, padded to 256
  int n_hub = 0;                               // of n_samp: the hub rows (largest row terms R0)
  // group-centred filter rows (cwq_group.hip; clustered trees): the isotropic rows below a
  // depth-1 internal node g are centred at its mean grp_c[g]; grp_par[p] = the group of
  // internal node p's rows (-1: root-centred), grp_F[p] = hs / invL of p's rows (Fast),
  // grp_Fc[p] = their categorize hs.  grp_mode: the filters read the shifted prefix tables.
  bool grp_mode = false;
  int G = 0;
  int64_t n_grp_rows = 0;
  // the cut plan_groups chose (host copies, build_prune reads them): the group of every
  // internal node (-1: a top node -- the root and the ancestors of the group centres, which
  // every query computes exactly), each group's centre (internal id) and whether its rows are
  // centred there (grp_ok; a group that fails the centring rule is still a pruning group)
  std::vector<int> cut_gint, cut_centre;
  std::vector<char> cut_ok;
  int cut_maxdep = 0, cut_top = 0;   // deepest centre, number of top nodes (filter_info)
  float* grp_c = nullptr;
  int* grp_par = nullptr;
  double *grp_F = nullptr, *grp_Fc = nullptr;
  // group pruning of the Fast query (cwq_prune.hip; group-centred trees with every level
  // weight >= 0): the pruning group of each internal node, group-major internal node lists,
  // per-group bound constants.  prune_ctr: the last call's stage-B pair count (diagnostics).
  bool prune_ok = false;
  int *prn_gint = nullptr, *gi_ptr = nullptr, *gi_nodes = nullptr;
  // top nodes in BFS order (root first) with their parents' list positions and depths; per
  // group the list position of its centre's parent (a top node)
  int *top_nodes = nullptr, *top_ppos = nullptr, *top_dep = nullptr, *grp_tpos = nullptr;
  int n_top = 0, top_maxdep = 0;
  // auto mode's record of the filter on this index: queries filtered / re-run exactly; when
  // at least 9 in 10 of >= 256 queries had to be re-run (the bounds too loose for this
  // tree's rows), auto mode takes the exact scan from then on (same results, less work)
  int64_t filt_q = 0, filt_fb = 0;
  bool filt_auto_off = false;
  int filt_off_calls = 0;   // auto-mode Fast calls on the exact scan since the filter went off
  // categorize: the last call's queries all went to the two-level replay, so the next call
  // launches the second list with the first replay (gated on its status) instead of after
  // reading that status back (categorize_impl)
  bool cat_two_spec = false;
  bool cat_tail_done = false;   // categorize_impl: the node tails are cleared, nothing runs after its last sync
  // categorize, calls of <= 64 queries: the list paths, or straight to the exact lazy replay
  // (simulate_lazy_runs_kernel; categorize_impl's path choice).  The choice is measured: per-query
  // wall time of each path (EMA), the faster one taken, the other tried every kCatExplore calls
  // -- but the lazy path is only ever tried while the list paths recently left queries to the
  // DENSE re-run (cat_dense_seen: ties nested deeper than the two-level replay certifies; a
  // tree the lists resolve, C2's or a flat one, never pays for the trial).  lazy_stats: the last
  // call's queries replayed lazily straight away / after the list paths (cwq_last_lazy_stats)
  // [0]: calls of <= 64 queries, [1]: batches (tried on any tree whose widest node fits the
  // replay's arena, max_fanout <= kLzFanout: the lazy replays of a batch run side by side)
  double cat_ema_list[2] = {-1.0, -1.0}, cat_ema_direct[2] = {-1.0, -1.0};
  int cat_dense_seen = 0, cat_pol_calls[2] = {0, 0};
  bool cat_pref_direct[2] = {false, false};
  int max_fanout = 0;   // the most children (internal + leaf rows) of one internal node
  int64_t lazy_stats[2] = {0, 0};
  // categorize: calls since the counting pass last resolved a query (after 8 such calls
  // cat_count_kernel is skipped -- every query then goes to the replay anyway -- and tried
  // again every kCatCountRetry calls)
  int cat_count_idle = 0;
  int prn_gmax = 1;   // the most internal nodes of one pruning group
  int prn_maxdep = 0, prn_mindep = 1;   // deepest / shallowest internal node of any group
  int *gi_dep = nullptr, *gi_ppos = nullptr;   // per group-list entry: depth, the parent's list position
  int* blk_grp = nullptr;   // per 16-row block of isotropic rows: the pruning group of all its rows (-1: mixed)
  int *gs_ptr = nullptr, *gs_rows = nullptr;   // per group: up to 64 usable isotropic rows (the seed threshold)
  GroupBound* gbound = nullptr;
  int* prune_ctr = nullptr;     // device [8]: per chunk pair count + claim counters, [4] the call's pair total
  int64_t prune_nq = 0;         // queries the last Fast call pruned (0: none)
  // internal-node bounds (hierarchical trees): bf16 operand rows, their RowF constants,
  // row-major fp32 A/B copies for the exact chain in final_kernel.  int_path (default):
  // the Fast filter reads the path prefix P of leaf parents only, so there is one row per
  // leaf parent (and the root), its b' vectors summed along the path (cwq_mfma.hip
  // int_path_prep) -- one GEMM, no prefix passes.  Otherwise (CWQ_INT_PATH=0 at index
  // creation) one row per internal node, levels 0-1 together and each deeper level from
  // a new 256-row tile, then prefix_bounds_kernel level by level.
  bool int_bounds = false;
  bool int_path = true;
  int DPB2 = 0;
  int64_t ld_i2 = 0;                  // operand rows (padded to 256)
  uint16_t* int_Mb2 = nullptr;
  RowF* int_rf2 = nullptr;
  int* int_rowid = nullptr;           // operand row -> internal id (-1: padding)
  RowF* int_nrf = nullptr;            // int_path: int_rf2 by internal id (par -2: no operand row), PathB
  float *int_Ar = nullptr, *int_Br = nullptr;
  float root_w = 1.f, root_ld = 0.f;   // the root's level weight and logdet (host copies)
  int* samp_rows = nullptr;
  uint16_t* iso_Sb = nullptr;
  // the direct schedule's sample operand (build_i8, on an index whose sample holds hub rows):
  // the sample rows of iso_Mq in iso_Sb's row order, and their terms {pa, pb, s_r, -}
  int8_t* iso_Sq = nullptr;
  float4* iso_St = nullptr;
  bool direct_ran = false;   // the current call ran the direct schedule (last_stats, filter_info)
  int64_t stats[6] = {0, 0, 0, 0, 0, 0};   // cwq_last_stats
  // timing (cwq_set_timing)
  bool timing = false;
  int filter = -1;   // cwq_set_filter
  int n_fg_launch = 0;   // filter launches of the last chunk (timing report)
  int n_fg_i8 = 0;       // of the call's filter launches (all chunks), those on the int8 operands
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float t_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // workspace.  Every query call carves its buffers from `ws`; the call's kernels may
  // still be running when it returns, so the end of each call records `ws_ev` on its
  // stream and the next call makes its own stream wait for it (ws_begin / ws_end):
  // calls on different streams reuse the workspace in order.
  std::mutex mu;
  GrowBuf ws{GrowBuf::kDevice, 1 << 20, "workspace hipMalloc failed ("};
  size_t ws_budget = 0;   // query-chunk workspace budget, from the free memory at the first call
  hipEvent_t ws_ev = nullptr;
  bool ws_ev_live = false;
  bool ws_idle = false;   // set by a call that ends with its stream synchronized: no event needed
  // the per-query filter flags on the host (int): coherent (fine-grained) memory --
  // final_wide_kernel writes the flags of the per-call path straight into it; the batch paths
  // copy into it (one D2H per chunk)
  GrowBuf hflags{GrowBuf::kMapped, 1, "hipHostMalloc failed"};
  // cwq_score_topk_host: pinned staging of the host queries, their device copy, and mapped
  // (coherent) host memory the kernels write the results into
  GrowBuf hq{GrowBuf::kPinned, 1 << 16, "host query staging allocation failed"};
  GrowBuf dq{GrowBuf::kDevice, 1 << 16, "host query staging allocation failed"};
  GrowBuf hout{GrowBuf::kMapped, 1 << 16, "host result buffer allocation failed"};
  // fallback re-runs (cwq_score_topk / cwq_categorize): gathered queries, their results
  // and the device index lists, kept between calls
  GrowBuf fb{GrowBuf::kDevice, 1 << 20, "fallback hipMalloc failed ("};
  GrowBuf fb2{GrowBuf::kDevice, 1, "categorize fallback buffers"};   // categorize's filter fallback (its exact re-run uses fb itself)
  // cwq_score_topk_masked, over-fetch path: the unmasked top-k' ids / scores and the per-query
  // short flags (not from `ws`: score_topk_impl carves that anew per chunk)
  // (cwq_score_topk_masked_multi: the same per width, the gathered queries and the device tables)
  GrowBuf mk{GrowBuf::kDevice, 1 << 16, "masked top-k buffers hipMalloc failed ("};
  // cwq_score_topk_masked_multi, masks run as calls of their own: one mask's gathered queries
  // and results (the single-mask call uses mk and fb itself)
  GrowBuf mg{GrowBuf::kDevice, 1 << 16, "per-query masks: sub-call buffers hipMalloc failed ("};
  // cwq_rank_ce_topk_masked: the slot table, the masked top-K result, the target's key and the
  // backward's list (the masked Fast call it runs uses mk, fb and mg itself)
  GrowBuf ml{GrowBuf::kDevice, 1 << 16, "masked loss buffers hipMalloc failed ("};
  int64_t mask_stats[4] = {0, 0, 0, 0};   // cwq_last_mask_stats
  int64_t mask_multi_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // cwq_last_mask_multi_stats

  template <class T>
  int alloc(T** p, size_t n) {
    void* q = nullptr;
    const size_t b = std::max<size_t>(n, 1) * sizeof(T);
    if (hipMalloc(&q, b) != hipSuccess) return fail(CWQ_ERR_OOM, "hipMalloc failed (" + std::to_string(b) + " B)");
    allocs.push_back(q);
    bytes += b;
    *p = (T*)q;
    return CWQ_OK;
  }
  template <class T>
  int upload(T** p, const std::vector<T>& v, hipStream_t s) {
    int rc = alloc(p, v.size());
    if (rc) return rc;
    if (!v.empty()) HIPCHK(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return CWQ_OK;
  }
  // earlier calls' kernels may still read the device buffers: the event to wait for before a free
  hipEvent_t busy() const { return ws_ev_live ? ws_ev : nullptr; }
  int reserve(size_t b) { return ws.reserve(b, busy()); }
  // start of a query call on stream s: wait for the previous call's use of the workspace
  int ws_begin(hipStream_t s) {
    if (!ws_ev && hipEventCreateWithFlags(&ws_ev, hipEventDisableTiming) != hipSuccess)
      return fail(CWQ_ERR_HIP, "hipEventCreate failed");
    // always wait, also on the previous call's stream handle: a destroyed stream's handle
    // can come back as a new stream.  The per-call path ends synchronized (ws_idle), so
    // it leaves no live event and queues no barrier packet here.
    if (ws_ev_live && hipStreamWaitEvent(s, ws_ev, 0) != hipSuccess)
      return fail(CWQ_ERR_HIP, "hipStreamWaitEvent failed");
    return CWQ_OK;
  }
  // end of a query call: the workspace is busy until the work queued on s so far is done
  int ws_end(hipStream_t s) {
    if (!ws_ev) return fail(CWQ_ERR_HIP, "workspace event missing");
    if (ws_idle) {   // every kernel of the call has finished: the workspace is free now
      ws_idle = false;
      ws_ev_live = false;
      return CWQ_OK;
    }
    if (hipEventRecord(ws_ev, s) != hipSuccess) {
      // the event no longer marks this call's work: wait for it here instead
      ws_ev_live = false;
      (void)hipStreamSynchronize(s);
      return fail(CWQ_ERR_HIP, "hipEventRecord failed");
    }
    ws_ev_live = true;
    return CWQ_OK;
  }
  ~cwq_index() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (ws_ev_live) (void)hipEventSynchronize(ws_ev);
    if (ws_ev) (void)hipEventDestroy(ws_ev);
    for (void* p : allocs) (void)hipFree(p);
    for (GrowBuf* b : {&ws, &fb, &fb2, &mk, &mg, &ml, &hflags, &hq, &dq, &hout}) b->release();
  }
};

// An allowed-sentence set for cwq_score_topk_masked (cwq_maskcalls.hip builds it): immutable after
// cwq_mask_create, so calls on any stream may share it; it holds no pointer into its index.
struct cwq_mask {
  uint64_t serial = 0;   // of the index it was built for
  int device = 0;
  int64_t n_sent = 0;
  int NL_iso = 0, NL_an = 0;
  void* mem = nullptr;   // one allocation: the arrays below
  size_t bytes = 0;
  uint32_t* bits = nullptr;   // the caller's bitset (private copy)
  uint8_t* live = nullptr;    // [NL] the row holds an allowed sentence
  int *rows_iso = nullptr, *rows_an = nullptr;   // live rows of each segment (segment row ids), ascending
  int n_iso = 0, n_an = 0;
  int64_t n_allowed = 0;   // allowed sentences that are in the tree
  ~cwq_mask() {
    if (mem) {
      DevGuard dg(device);
      (void)hipFree(mem);
    }
  }
};

namespace cwq {

// RAII: a query entry point's use of the handle workspace on stream s (cwq_index::ws_begin)
struct WsUse {
  cwq_index* ix;
  hipStream_t s;
  int rc;
  WsUse(cwq_index* i, hipStream_t st) : ix(i), s(st) {
    rc = ix->ws_begin(s);
  }
  ~WsUse() {
    if (rc == CWQ_OK) (void)ix->ws_end(s);   // ws_begin failed: nothing was queued on s
  }
};

// Scan configuration of one query call (cwq_kernels.hip scan_cfg_begin): fixed from the
// call's total query count, so every chunk and workspace estimate of the call agrees.
struct ScanCfgScope {
  explicit ScanCfgScope(int64_t nq) { scan_cfg_begin(nq); }
  ~ScanCfgScope() { scan_cfg_end(); }
};

// A query entry point's hold on the handle, in this order: its lock, its device, its use of the
// workspace on stream s (rc: ws_begin's result) and the call's scan configuration.
struct QueryCall {
  std::lock_guard<std::mutex> lk;
  DevGuard dg;
  WsUse wu;
  ScanCfgScope scs;
  int rc;
  QueryCall(cwq_index* ix, int64_t nq, hipStream_t s) : lk(ix->mu), dg(ix->device), wu(ix, s), scs(nq), rc(wu.rc) {}
};

// Gather some queries of a call, run a sub-call on them, scatter its results back: idx holds the
// queries' indices in the call (pageable host memory, so close() synchronises the stream: idx
// must outlive its upload to d_idx).
struct SubCall {
  hipStream_t s;
  int64_t n;
  int64_t* d_idx;
  int open(const std::vector<int64_t>& idx, int64_t* d, hipStream_t st) {
    s = st;
    n = (int64_t)idx.size();
    d_idx = d;
    HIPCHK(hipMemcpyAsync(d_idx, idx.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    return CWQ_OK;
  }
  int gather(const float* q, int64_t D, float* qsub) {   // qsub[i] = q[idx[i]]
    HIPCHK(launch_copy_rows(q, D, d_idx, qsub, D, nullptr, n, D, s));
    return CWQ_OK;
  }
  int scatter(const void* src, int64_t words, void* dst) {   // dst[idx[i]] = src[i], rows of 4-byte words
    HIPCHK(launch_copy_rows(src, words, nullptr, dst, words, d_idx, n, words, s));
    return CWQ_OK;
  }
  int close() {
    HIPCHK(hipStreamSynchronize(s));
    return CWQ_OK;
  }
};

constexpr int kQPad = 128;   // queries are padded to a multiple of the largest query block

struct Chunk {
  int nq = 0;           // valid queries
  int64_t nq_pad = 0;
  float* X = nullptr;   // [nq_pad][DP]
  float *S_int = nullptr, *P = nullptr, *BF = nullptr, *LPF = nullptr;   // [nq_pad][NI]
  // P / S_int layout (pidx): query-major [q][ldP] (the exact pass); node-major [node][nq_pad]
  // after the path-sum bounds (run_internal_bounds)
  int64_t ldP = 1;
  int pT = 0;
  const float4* qi2 = nullptr;   // path-sum bounds: the queries' [x'^2, x'] norms (PathB)
  // group-centred rows (grp_mode): the filters' prefix tables [nq_pad][NI] -- Fast
  // [Pg_lo, Pg_hi] and categorize [Pc_lo, Pc_hi] -- and the per-(query, group) shifts
  float *Pg_lo = nullptr, *Pg_hi = nullptr, *Pc_lo = nullptr, *Pc_hi = nullptr;
  double* gsh = nullptr;
  float* Tseed = nullptr;   // group pruning's seed threshold [nq] (a lower bound of tau_K), or none
  int grp_done = -1;   // the group tables run_internal's fused pass wrote: -1 none, 0 Fast, 1 + categorize
  // call-time level weights (cwq_lweight.hip): the exact passes read these instead of the index's
  const float* w_int = nullptr;    // [NI]
  const RowMeta* meta = nullptr;   // [NL]
};

// Run-time knobs (environment variables, read where they are used: tests switch them in-process)
inline int env_int(const char* name, int dflt) {   // the value of a non-empty setting, else dflt
  const char* e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
inline bool env_off(const char* name) {   // a non-empty setting that parses to 0
  const char* e = getenv(name);
  return e && *e && atoi(e) == 0;
}
inline bool env_set(const char* name) { return getenv(name) != nullptr; }

// Error-bound constants of the filter (cwq_mfma.hip header): fp32 accumulation of the
// MFMA products (2x the textbook (n-1)u, n = DPB + 64), norm/centring rounding, and the
// relative slack that covers the fp32 evaluation of both the bounds and the exact keys.
struct FiltConsts {
  double gamma, eps_n, slack;
};
inline FiltConsts filt_consts(int DPB) {
  return {(DPB + 64) * std::ldexp(1.0, -23), std::ldexp(1.0, -20), std::ldexp(1.0, -16)};
}

constexpr int kFiltMinRows = 16384;   // automatic mode: below this the exact scan is as fast
constexpr int kFiltMaxK = 64;         // the filter serves the list-based top-k path (k <= 64)
constexpr int kFgRecPerQ = 512;       // candidate-record slots per query (append buffer)
constexpr int kFgDirPerQ = 256;       // direct-record slots per query (tiles past kFgCap)
// use_filter's min_rows on the per-call stream path (cwq_filter.hip)
constexpr int kStreamMinRows = 512;
// the most workgroups per query of the per-call path's rerank tail (fw_split, cwq_topk.hip)
constexpr int kFwSplitMax = 32;

// The buffers run_iso_filter (cwq_filter.hip) leaves for the caller's final pass.
struct IsoFilter {
  int *qcnt, *okf, *nex, *qover, *tdone, *crow, *tr;
  float *cu, *cl, *tl, *tlk;
};

// ---- functions that cross a file, under the file that defines them ----

// cwq_api.hip
bool fg_flat_tiles(const cwq_index* ix);

// cwq_chunk.hip (the per-chunk exact passes, chunk sizing and carving)
int group_tables(cwq_index* ix, Chunk& c, const float* q, bool cat, hipStream_t s);
bool use_prune(const cwq_index* ix);
int prune_internal(cwq_index* ix, Chunk& c, const float* q, int K, Bump& b, hipStream_t s, float* T0 = nullptr,
                   int64_t ldT0 = 0, int* live = nullptr);
int n_qblocks_for(int64_t nq, int kl);
int pick_nslab(const cwq_index* ix, int nrows, int n_qblocks, int kl = 16);
bool use_int_bounds(const cwq_index* ix);
IntChain int_chain(const cwq_index* ix);
bool small_scan_fits(const cwq_index* ix, int K);
PathB path_b(const cwq_index* ix, const Chunk& c);
int run_internal(cwq_index* ix, Chunk& c, hipStream_t s, bool bf_lpf = true, const float* q = nullptr,
                 int grp_cat = -1);
size_t int_bounds_bytes(const cwq_index* ix, int64_t nqf);
int run_internal_bounds(cwq_index* ix, Chunk& c, const float* q, int64_t nqf, Bump& b, hipStream_t s);
int run_leaf_scan(cwq_index* ix, const Chunk& c, int epi, bool cat, int kl, float dconst, float* out, int64_t ldo,
                  float* pkey, float* paux, int* prow, int K, int* nslab_total_out, hipStream_t s,
                  int seg_mask = 3, int slab_off0 = 0, int max_lists = INT_MAX);
size_t chunk_bytes(const cwq_index* ix, int64_t nq_pad, bool full = true);
void carve_chunk(cwq_index* ix, Bump& b, Chunk& c, int nq, bool full = true);
int64_t chunk_queries(const cwq_index* ix, int64_t nq, size_t per_query_extra, bool full = true);

// cwq_filter.hip (the batch filter shared by Fast and Basic, its policy and its int8 panel)
bool use_filter(const cwq_index* ix, int k, int min_rows = kFiltMinRows, bool fast = true);
void note_filter(cwq_index* ix);
int fg_order();
void fg_groups(int n_qt, int& qg, int& rg);
bool i8_size_rule(const cwq_index* ix);
bool ensure_i8(cwq_index* ix, hipStream_t s);
void note_i8_early(cwq_index* ix, int64_t nq, int64_t cand_sum, int64_t n_fallback);
size_t iso_filter_bytes_per_query(const cwq_index* ix, int n_rt);
int run_iso_filter(cwq_index* ix, Chunk& c, const float* qsrc, int64_t nqf, int K, bool cat, bool ib, Bump& b,
                   IsoFilter& o, hipStream_t s);

// cwq_topk.hip (the per-call path's helpers that categorize shares; the host entry points' staging)
hipError_t sync_spin(hipStream_t s);
int stream_wgs(const cwq_index* ix);
int fw_split(const cwq_index* ix, int nq, bool i8);
int stage_host(cwq_index* ix, const float* q, size_t qbytes, size_t obytes, hipStream_t s);
// (the unmasked Fast call for a caller that holds the handle: topk_reset, score_topk_impl + note_filter)
void topk_begin(cwq_index* ix);
int score_topk_unmasked(cwq_index* ix, const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores,
                        hipStream_t s);

// cwq_maskcalls.hip: the masked Fast call for a caller that holds the handle (QueryCall): query i
// restricted to masks[mask_of_query[i]] (host array; null: masks[0] for every query), the path
// rules and stats of cwq_score_topk_masked / cwq_score_topk_masked_multi.  Arguments are checked
// by the caller.
int masked_topk_locked(cwq_index* ix, const cwq_mask* const* masks, int32_t n_masks, const int32_t* mask_of_query,
                       const float* q, int64_t nq, int32_t k, int64_t* ids, float* scores, hipStream_t s, int rc0 = 0);

// cwq_sparsecalls.hip: scores[q][j] of given sentences and the gradient of their weighted sum,
// chunk by chunk, for a caller that holds the handle
int pairs_forward(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int m, int64_t ld_ids, float* out,
                  int64_t ld_out, hipStream_t s);
int pairs_backward(cwq_index* ix, const float* q, int64_t nq, const int64_t* ids, int m, const float* g, float* grad_q,
                   hipStream_t s);

// cwq_rank.hip (the dense backward's plan and carve, shared with the masked loss)
// The backward's launch plan: slabs, leaf-sum pieces, threads per node and workspace bytes per
// query -- functions of the index alone (a query's gradient is the same in any batch).
struct GradPlan {
  int rps, ns_iso, ns_an, ns_int, nslab, nsplit, P;
  std::vector<int> lv;
  size_t per_q;
};
GradPlan grad_plan(const cwq_index* ix);
// The coefficient arrays and the partial tiles of one chunk (nq16 * per_q bytes + 8 * 256).
float* grad_carve(const cwq_index* ix, const GradPlan& gp, Bump& b, int nqc, int qtiles, GradCoefArgs& ca);

}  // namespace cwq
