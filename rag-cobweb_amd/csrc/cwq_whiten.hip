// libcwq: PCA + ICA whitening transform (F4) on fp32 MFMA.
//
// Replaces PCAICAWhiteningModel.transform (src/whitening/pca_ica.py:30-51):
//   x_c   = x - mean                         (:40)
//   x_pca = (x_c @ components^T) / sqrt(explained_var + eps)   (:43-44)
//   x_ica = x_pca @ unmixing^T               (:48)
// as two GEMMs C[m][n] = sum_k (A[m][k] - ctr[k]) * B[n][k] with the centring fused
// into the A-tile load and the per-column division into the epilogue.  fp32 in, fp32
// accumulate on v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain in k order, at the fp32
// vector rate): the path keeps the reference's fp32 numerics instead of dropping to
// bf16 -- its output feeds the tree statistics.  The divisor sqrt(var + eps) is passed
// in, computed by the caller exactly as numpy does (fp32 add, fp32 sqrt), so only the
// order of the dot-product accumulation differs from the reference's sgemm.
//
// The main loop (128 x 128 tiles, K staged through LDS) is cwq_gemm_nt_f32.h; this file
// holds the transform's epilogue: the per-column division and the store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cwq_gemm_nt_f32.h"
#include "cwq_internal.h"

namespace cwq {

// C[m][n] = acc / denom[n] (plain store when denom is NULL)
struct EpiDenom {
  const float* __restrict__ denom;
  float* __restrict__ C;
  __device__ void operator()(const f32x16w (&acc)[2][2], int64_t m0, int n0, int wm, int wn, int fi, int fk, int64_t M,
                             int N, float*) const {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + fi;
      if (n >= N) continue;
      const float dv = denom ? denom[n] : 1.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fk;
          if (m < M) C[m * N + n] = denom ? acc[i][j][e] / dv : acc[i][j][e];
        }
    }
  }
};

hipError_t launch_gemm_nt_f32(const float* A, int64_t M, int K, const float* ctr, const float* B, int N,
                              const float* denom, float* C, hipStream_t s) {
  if (M <= 0 || N <= 0) return hipSuccess;
  dim3 grid((unsigned)((M + WT - 1) / WT), (unsigned)((N + WT - 1) / WT));
  hipLaunchKernelGGL(gemm_nt_f32_kernel<EpiDenom>, grid, dim3(256), 0, s, A, M, K, ctr, B, N, EpiDenom{denom, C});
  return hipGetLastError();
}

}  // namespace cwq
