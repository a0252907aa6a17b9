// libcwq C ABI (host side), the small parts: the error slot (fail / cwq_last_error), the version and
// build id, and the handle's getters and setters.  Public contract: include/cobweb_query.h.
// The jobs behind the other entry points: cwq_build.hip (index build), cwq_chunk.hip (the per-chunk
// exact passes), cwq_filter.hip (the batch filter), cwq_topk.hip (Fast top-k), cwq_categorize.hip (Basic).
#include "cwq_handle.h"

static thread_local std::string g_err;

namespace cwq {
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace cwq

#ifndef CWQ_BUILD_ID
#define CWQ_BUILD_ID "unversioned"
#endif
extern "C" int cwq_version(void) { return 310; }
// "CWQ_BUILD_ID=<id>" is also searched for in the file by build.py (no dlopen needed)
static const char kBuildId[] = "CWQ_BUILD_ID=" CWQ_BUILD_ID;
extern "C" const char* cwq_build_id(void) { return kBuildId + 13; }
extern "C" const char* cwq_last_error(void) { return g_err.c_str(); }

extern "C" int cwq_index_info(const cwq_index* idx, int64_t* o) {
  if (!idx || !o) return fail(CWQ_ERR_ARG, "NULL argument");
  o[0] = idx->n_nodes;
  o[1] = idx->D;
  o[2] = idx->n_sent;
  o[3] = idx->NI;
  o[4] = idx->NL;
  o[5] = idx->NL_iso;
  o[6] = idx->max_depth;
  o[7] = (int64_t)idx->bytes;
  return CWQ_OK;
}

namespace cwq {
// every row tile uniform (one parent: a flat tree's tiles), so one raw launch can cover them all
bool fg_flat_tiles(const cwq_index* ix) {
  const size_t n = ix->tile_uni_prefix.size();
  return n > 1 && (size_t)ix->tile_uni_prefix[n - 1] == n - 1 && !env_set("CWQ_FG_NO_ALLUNI");
}
}  // namespace cwq

extern "C" int cwq_index_filter_info(const cwq_index* idx, int64_t* o) {
  if (!idx || !o) return fail(CWQ_ERR_ARG, "NULL argument");
  o[0] = idx->grp_mode ? 1 : 0;
  o[1] = idx->G;
  o[2] = idx->n_grp_rows;
  o[3] = idx->i8_state > 0 ? 1 : 0;
  o[4] = idx->n_hub;
  // the batch filter's schedule on this index by the default rules (fg_i8_from; the per-call
  // knobs aside): 0 bf16 launches only, 1 the quarter rule, 2 the early schedule, 3 the direct one
  const bool early = idx->i8_state > 0 && idx->i8_by_size && idx->n_hub > 0 && !idx->i8_early_off && !idx->grp_mode;
  o[5] = idx->i8_state <= 0 ? 0 : !early ? 1 : (idx->iso_Sq && idx->iso_St && fg_flat_tiles(idx)) ? 3 : 2;
  o[6] = idx->direct_ran ? 1 : 0;   // the last Fast batch call ran the direct schedule
  return CWQ_OK;
}

extern "C" int cwq_last_lazy_stats(const cwq_index* idx, int64_t* o) {
  if (!idx || !o) return fail(CWQ_ERR_ARG, "NULL argument");
  o[0] = idx->lazy_stats[0];
  o[1] = idx->lazy_stats[1];
  return CWQ_OK;
}

extern "C" int cwq_index_cut_info(const cwq_index* idx, int64_t* o) {
  if (!idx || !o) return fail(CWQ_ERR_ARG, "NULL argument");
  o[0] = (int64_t)idx->cut_centre.size();
  o[1] = idx->cut_centre.empty() ? 0 : idx->cut_top;
  o[2] = idx->cut_maxdep;
  int64_t n_ok = 0;
  for (char c : idx->cut_ok) n_ok += c ? 1 : 0;
  o[3] = n_ok;
  return CWQ_OK;
}

extern "C" int cwq_set_filter(cwq_index* ix, int mode) {
  if (!ix) return fail(CWQ_ERR_ARG, "NULL index");
  if (mode < -1 || mode > 1) return fail(CWQ_ERR_ARG, "mode must be -1, 0 or 1");
  ix->filter = mode;
  ix->filt_q = ix->filt_fb = 0;   // a fresh auto-mode record
  ix->filt_auto_off = false;
  ix->filt_off_calls = 0;
  ix->i8_early_off = false;
  return CWQ_OK;
}

extern "C" int cwq_last_stats(cwq_index* ix, int64_t* out) {
  if (!ix || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  for (int i = 0; i < 6; ++i) out[i] = ix->stats[i];
  return CWQ_OK;
}

extern "C" int cwq_last_prune_stats(cwq_index* ix, int64_t* out) {
  if (!ix || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DevGuard dg(ix->device);
  out[0] = ix->prune_ok ? 1 : 0;
  out[1] = ix->prune_nq;
  out[2] = 0;
  out[3] = ix->G;
  if (ix->prune_ctr && ix->prune_nq > 0) {
    int v = 0;
    if (ix->ws_ev_live) HIPCHK(hipEventSynchronize(ix->ws_ev));
    HIPCHK(hipMemcpy(&v, ix->prune_ctr + 4, sizeof(int), hipMemcpyDeviceToHost));
    out[2] = v;
  }
  return CWQ_OK;
}

extern "C" int cwq_set_timing(cwq_index* ix, int enable) {
  if (!ix) return fail(CWQ_ERR_ARG, "NULL index");
  DevGuard dg(ix->device);
  for (int i = 0; i < 8; ++i)
    if (!ix->ev[i]) HIPCHK(hipEventCreate(&ix->ev[i]));
  ix->timing = enable != 0;
  return CWQ_OK;
}

extern "C" int cwq_last_timing(cwq_index* ix, float* out) {
  if (!ix || !out) return fail(CWQ_ERR_ARG, "NULL argument");
  for (int i = 0; i < 8; ++i) out[i] = ix->t_ms[i];
  return CWQ_OK;
}
