// Entry points that take no handle: cwq_welford_groups, cwq_whiten and the whitening-fit wrappers.
// Calls the launch_* functions (cwq_internal.h) and fail (cwq_api.hip).
#include "cwq_handle.h"

extern "C" int cwq_welford_groups(const float* X, int64_t n_rows, int32_t dim, const int64_t* order,
                                  const int64_t* group_ptr, int64_t n_groups, float* count, float* mean,
                                  float* meanSq, void* stream) {
  if (!X || !order || !group_ptr || !count || !mean || !meanSq || dim <= 0 || n_rows < 0)
    return fail(CWQ_ERR_ARG, "bad arguments");
  if (n_groups > 65535) return fail(CWQ_ERR_ARG, "at most 65535 groups per call");
  HIPCHK(launch_welford_groups(X, dim, order, group_ptr, n_groups, count, mean, meanSq, (hipStream_t)stream));
  return CWQ_OK;
}

// PCA + ICA whitening transform (F4) -- PCAICAWhiteningModel.transform, src/whitening/pca_ica.py:30-51.
extern "C" int cwq_whiten(const float* X, int64_t n, int32_t d_in, const float* mean, const float* comps,
                          int32_t d_pca, const float* denom, const float* unmix, int32_t d_out, float* out,
                          float* work, void* stream) {
  if (n < 0 || d_in <= 0 || d_pca <= 0 || (unmix && d_out <= 0)) return fail(CWQ_ERR_ARG, "bad whitening shape");
  if (n == 0) return CWQ_OK;
  if (!X || !mean || !comps || !denom || !out || (unmix && !work)) return fail(CWQ_ERR_ARG, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  float* pca = unmix ? work : out;
  HIPCHK(launch_gemm_nt_f32(X, n, d_in, mean, comps, d_pca, denom, pca, s));
  if (unmix) HIPCHK(launch_gemm_nt_f32(pca, n, d_pca, nullptr, unmix, d_out, nullptr, out, s));
  return CWQ_OK;
}

// ---- whitening fit: column sums, TN Gram, FastICA's G pass (cwq_whitenfit.hip) ----
static bool wf_dim_ok(int32_t d) { return d >= 1 && d <= 1024; }

extern "C" int cwq_whitenfit_slab(void) { return kWfSlab; }

extern "C" int64_t cwq_col_sums_work_bytes(int64_t n, int32_t d) {
  if (n < 0 || !wf_dim_ok(d)) return -1;
  return ((n + kWfSlab - 1) / kWfSlab) * d * (int64_t)sizeof(double);
}

extern "C" int64_t cwq_gram_acc_work_bytes(int64_t n, int32_t da, int32_t db) {
  if (n < 0 || !wf_dim_ok(da) || !wf_dim_ok(db)) return -1;
  return ((n + kWfSlab - 1) / kWfSlab) * da * db * (int64_t)sizeof(float);
}

extern "C" int64_t cwq_ica_g_work_bytes(int64_t n, int32_t p) {
  if (n < 0 || !wf_dim_ok(p)) return -1;
  return ((n + 127) / 128) * p * (int64_t)sizeof(double);
}

extern "C" int cwq_col_sums(const float* X, int64_t n, int32_t d, double* acc, void* work, void* stream) {
  if (n < 0 || !wf_dim_ok(d)) return fail(CWQ_ERR_ARG, "bad column-sum shape (n >= 0, d in [1, 1024])");
  if (!X || !acc || !work) return fail(CWQ_ERR_ARG, "NULL argument");
  if (n == 0) return CWQ_OK;
  HIPCHK(launch_col_sums(X, n, d, acc, (double*)work, (hipStream_t)stream));
  return CWQ_OK;
}

extern "C" int cwq_gram_acc(const float* A, const float* B, int64_t n, int32_t da, int32_t db, const float* ctr_a,
                            const float* ctr_b, double* acc, void* work, void* stream) {
  if (n < 0 || !wf_dim_ok(da) || !wf_dim_ok(db))
    return fail(CWQ_ERR_ARG, "bad Gram shape (n >= 0, da and db in [1, 1024])");
  if (!A || !B || !acc || !work) return fail(CWQ_ERR_ARG, "NULL argument");
  if (n == 0) return CWQ_OK;
  HIPCHK(launch_gram_acc(A, B, n, da, db, ctr_a, ctr_b, acc, (float*)work, (hipStream_t)stream));
  return CWQ_OK;
}

extern "C" int cwq_ica_g(const float* X1, int64_t n, int32_t p, const float* W, float* G, double* gsum, void* work,
                         void* stream) {
  if (n < 0 || !wf_dim_ok(p)) return fail(CWQ_ERR_ARG, "bad ICA shape (n >= 0, p in [1, 1024])");
  if (!X1 || !W || !G || !gsum || !work) return fail(CWQ_ERR_ARG, "NULL argument");
  if (n == 0) return CWQ_OK;
  HIPCHK(launch_ica_g(X1, n, p, W, G, gsum, (double*)work, (hipStream_t)stream));
  return CWQ_OK;
}
