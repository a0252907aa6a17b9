// libcwq: the dense passes of the whitening fits (PCA + ICA, ZCA, PCA-ZCA) on the GPU.
//
// The reference fits on the host (src/whitening/pca_ica.py:55-76, zca.py:32-51,
// pca_zca.py:47-60): a mean, a covariance / PCA of [n, d], and FastICA's iteration
//   Y = X1 W^T,  G = tanh(Y),  M = G^T X1,  gsum = sum_r (1 - G^2)
// over [n, p].  Three passes carry all of the n-proportional work:
//
//   colsum  : column sums of X, fp64 accumulation                     (bandwidth bound)
//   gram    : acc[i][j] += sum_r (A[r][i] - ca[i]) (B[r][j] - cb[j])  (TN GEMM, k = rows)
//   ica_g   : G = tanh(X1 W^T) and gsum                               (NT GEMM + epilogue)
//
// Both GEMMs are exact fp32 on v_mfma_f32_32x32x2_f32 (an fp32 fma chain in k order),
// like cwq_whiten; the TN product, whose k runs over a whole slab, folds its chain into a
// second fp32 accumulator every 512 rows.  Every reduction over rows goes through a FIXED
// decomposition: rows are cut into slabs of kWfSlab rows (128-row tiles for gsum), each
// slab's partial depends on its own rows alone, and a reduce kernel adds the partials in
// slab order in fp64.  No atomics: results are bit-identical from run to run and do not depend on the
// number of CUs.
//
// TN tile: the 128 x 128 output tile of gemm_nt_f32_kernel with the same MFMA loop.  Its
// operands must be k-major in LDS ([k][i]); for a TN product k is the row index, so a
// [16 rows][128 columns] block of A goes to LDS as it lies in memory (two float4 per
// thread), with the centring applied on the way.  Rows past n are stored as 0, not -ctr.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cwq_gemm_nt_f32.h"
#include "cwq_internal.h"

namespace cwq {

// ---------------------------------------------------------------- column sums
// grid (slab, 64-column group); 4 row lanes x 64 columns; part[slab][d] fp64
__global__ __launch_bounds__(256) void wf_colsum_part_kernel(const float* __restrict__ X, int64_t n, int d,
                                                             double* __restrict__ part) {
  __shared__ double red[4][64];
  const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
  const int c = blockIdx.y * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.x * kWfSlab;
  const int64_t r1 = (r0 + kWfSlab < n) ? r0 + kWfSlab : n;
  double s = 0.0;
  if (c < d) {
#pragma unroll 8
    for (int64_t r = r0 + rl; r < r1; r += 4) s += (double)X[r * d + c];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < d) part[(int64_t)blockIdx.x * d + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// acc[c] += sum_s part[s][c] in a fixed order: 16 interleaved chains, then the chains in order.
// grid (64-column group), 1024 threads
__global__ __launch_bounds__(1024) void wf_colpart_reduce_kernel(const double* __restrict__ part, int64_t nparts,
                                                                 int ncols, double* __restrict__ acc) {
  __shared__ double red[16][64];
  const int tid = threadIdx.x, cl = tid & 63, g = tid >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < ncols) {
#pragma unroll 8
    for (int64_t p = g; p < nparts; p += 16) s += part[p * ncols + c];
  }
  red[g][cl] = s;
  __syncthreads();
  if (g == 0 && c < ncols) {
    double t = red[0][cl];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][cl];
    acc[c] += t;
  }
}

hipError_t launch_col_sums(const float* X, int64_t n, int d, double* acc, double* work, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t nslab = (n + kWfSlab - 1) / kWfSlab;
  const unsigned cg = (unsigned)((d + 63) / 64);
  hipLaunchKernelGGL(wf_colsum_part_kernel, dim3((unsigned)nslab, cg), dim3(256), 0, s, X, n, d, work);
  hipLaunchKernelGGL(wf_colpart_reduce_kernel, dim3(cg), dim3(1024), 0, s, work, nslab, d, acc);
  return hipGetLastError();
}

// ---------------------------------------------------------------- TN Gram
// grid (slab, tile pair); part[slab][da][db] fp32.  sym: only tile pairs tj >= ti.
__global__ __launch_bounds__(256) void wf_gram_tn_f32_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                             int64_t n, int da, int db,
                                                             const float* __restrict__ ca, const float* __restrict__ cb,
                                                             int sym, int tiles_j, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[2][WK][WLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][WK][WLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int ti, tj;
  if (sym) {
    int rem = blockIdx.y;
    ti = 0;
    while (rem >= tiles_j - ti) {
      rem -= tiles_j - ti;
      ++ti;
    }
    tj = ti + rem;
  } else {
    ti = blockIdx.y / tiles_j;
    tj = blockIdx.y % tiles_j;
  }
  const int i0 = ti * WT, j0 = tj * WT;
  const int64_t r0 = (int64_t)blockIdx.x * kWfSlab;
  const int64_t r1 = (r0 + kWfSlab < n) ? r0 + kWfSlab : n;
  // staging: thread owns row lk of the stage and 8 consecutive columns of each operand
  const int lk = tid >> 4, seg = (tid & 15) * 8;
  const int acol = i0 + seg, bcol = j0 + seg;
  const bool avec = (da & 3) == 0 && acol + 8 <= da;
  const bool bvec = (db & 3) == 0 && bcol + 8 <= db;
  float cav[8], cbv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cav[j] = (ca && acol + j < da) ? ca[acol + j] : 0.f;
    cbv[j] = (cb && bcol + j < db) ? cb[bcol + j] : 0.f;
  }
  float ra[8], rb[8];
  auto gload = [&](int kt) {
    const int64_t r = r0 + (int64_t)kt * WK + lk;
    const bool rowok = r < r1;
    const float* ap = A + r * da + acol;
    const float* bp = B + r * db + bcol;
    if (avec) {
      float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
      if (rowok) {
        x0 = *reinterpret_cast<const float4*>(ap);
        x1 = *reinterpret_cast<const float4*>(ap + 4);
      }
      ra[0] = x0.x; ra[1] = x0.y; ra[2] = x0.z; ra[3] = x0.w;
      ra[4] = x1.x; ra[5] = x1.y; ra[6] = x1.z; ra[7] = x1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) ra[j] = (rowok && acol + j < da) ? ap[j] : 0.f;
    }
    if (bvec) {
      float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
      if (rowok) {
        x0 = *reinterpret_cast<const float4*>(bp);
        x1 = *reinterpret_cast<const float4*>(bp + 4);
      }
      rb[0] = x0.x; rb[1] = x0.y; rb[2] = x0.z; rb[3] = x0.w;
      rb[4] = x1.x; rb[5] = x1.y; rb[6] = x1.z; rb[7] = x1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) rb[j] = (rowok && bcol + j < db) ? bp[j] : 0.f;
    }
  };
  auto swrite = [&](int b, int kt) {
    // padding (rows past the slab / n, columns past da / db) stays exactly 0, not -ctr
    const bool rowok = r0 + (int64_t)kt * WK + lk < r1;
    float va[8], vb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      va[j] = (rowok && acol + j < da) ? ra[j] - cav[j] : 0.f;
      vb[j] = (rowok && bcol + j < db) ? rb[j] - cbv[j] : 0.f;
    }
    *reinterpret_cast<float4*>(&As[b][lk][seg]) = make_float4(va[0], va[1], va[2], va[3]);
    *reinterpret_cast<float4*>(&As[b][lk][seg + 4]) = make_float4(va[4], va[5], va[6], va[7]);
    *reinterpret_cast<float4*>(&Bs[b][lk][seg]) = make_float4(vb[0], vb[1], vb[2], vb[3]);
    *reinterpret_cast<float4*>(&Bs[b][lk][seg + 4]) = make_float4(vb[4], vb[5], vb[6], vb[7]);
  };
  // acc: the running fma chain, folded into tot every kWfFold stages (512 rows) so that no
  // fp32 chain is longer than a blocked sgemm's: 512 products, then at most 8 partial sums
  f32x16w acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = tot[i][j][e] = 0.f;
  const int nk = (int)((r1 - r0 + WK - 1) / WK);
  gload(0);
  swrite(0, 0);
  __syncthreads();
  const int fi = lane & 31, fk = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int b = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int kk = 0; kk < WK; kk += 2) {
      float af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = As[b][kk + fk][wm * 64 + t * 32 + fi];
        bf[t] = Bs[b][kk + fk][wn * 64 + t * 32 + fi];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if ((kt & (kWfFold - 1)) == kWfFold - 1 || kt + 1 == nk) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
    }
    if (kt + 1 < nk) swrite(b ^ 1, kt + 1);
    __syncthreads();
  }
  // C[i][j]: lane: j = lane&31, i = (e&3) + 8(e>>2) + 4(lane>>5)
  float* P = part + (int64_t)blockIdx.x * da * db;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cj = j0 + wn * 64 + j * 32 + fi;
    if (cj >= db) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ci = i0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fk;
        if (ci < da) P[(int64_t)ci * db + cj] = tot[i][j][e];
      }
  }
}

// acc[i][j] += sum_s part[s][i][j], slab order, fp64.  sym: tiles below the diagonal were
// not computed; their elements are read from the mirrored tile.
__global__ __launch_bounds__(256) void wf_gram_reduce_kernel(const float* __restrict__ part, int64_t nslab, int da,
                                                             int db, int sym, double* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t sz = (int64_t)da * db;
  if (idx >= sz) return;
  const int i = (int)(idx / db), j = (int)(idx % db);
  const int64_t src = (sym && i / WT > j / WT) ? (int64_t)j * db + i : idx;
  double s = 0.0;
#pragma unroll 8
  for (int64_t k = 0; k < nslab; ++k) s += (double)part[k * sz + src];
  acc[idx] += s;
}

hipError_t launch_gram_acc(const float* A, const float* B, int64_t n, int da, int db, const float* ca, const float* cb,
                           double* acc, float* work, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t nslab = (n + kWfSlab - 1) / kWfSlab;
  const int sym = (A == B && ca == cb && da == db) ? 1 : 0;
  const int ti = (da + WT - 1) / WT, tj = (db + WT - 1) / WT;
  const int pairs = sym ? ti * (ti + 1) / 2 : ti * tj;
  hipLaunchKernelGGL(wf_gram_tn_f32_kernel, dim3((unsigned)nslab, (unsigned)pairs), dim3(256), 0, s, A, B, n, da, db,
                     ca, cb, sym, tj, work);
  const int64_t sz = (int64_t)da * db;
  hipLaunchKernelGGL(wf_gram_reduce_kernel, dim3((unsigned)((sz + 255) / 256)), dim3(256), 0, s, work, nslab, da, db,
                     sym, acc);
  return hipGetLastError();
}

// ---------------------------------------------------------------- G = tanh(X1 W^T), gsum
// Epilogue of gemm_nt_f32_kernel: stores G and writes this 128-row tile's column sums of
// 1 - G^2 to part[row tile][N] in fp64.  Rows past M and columns past N are masked out
// (a zero padding row would add 1 - tanh(0)^2 = 1).
struct EpiTanh {
  float* __restrict__ G;
  double* __restrict__ part;
  __device__ void operator()(const f32x16w (&acc)[2][2], int64_t m0, int n0, int wm, int wn, int fi, int fk, int64_t M,
                             int N, float* smem) const {
    double* red = reinterpret_cast<double*>(smem);   // [wm][fk][128 columns]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + fi;
      double s = 0.0;
      if (n < N) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fk;
            if (m < M) {
              const float g = tanhf(acc[i][j][e]);
              G[m * N + n] = g;
              s += (double)(1.f - g * g);
            }
          }
      }
      red[(wm * 2 + fk) * WT + wn * 64 + j * 32 + fi] = s;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < WT && n0 + c < N)
      part[(m0 / WT) * N + n0 + c] = ((red[c] + red[WT + c]) + red[2 * WT + c]) + red[3 * WT + c];
  }
};

hipError_t launch_ica_g(const float* X1, int64_t n, int p, const float* W, float* G, double* gsum, double* work,
                        hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t mt = (n + WT - 1) / WT;
  dim3 grid((unsigned)mt, (unsigned)((p + WT - 1) / WT));
  hipLaunchKernelGGL(gemm_nt_f32_kernel<EpiTanh>, grid, dim3(256), 0, s, X1, n, p, (const float*)nullptr, W, p,
                     EpiTanh{G, work});
  hipLaunchKernelGGL(wf_colpart_reduce_kernel, dim3((unsigned)((p + 63) / 64)), dim3(1024), 0, s, work, mt, p, gsum);
  return hipGetLastError();
}

}  // namespace cwq
