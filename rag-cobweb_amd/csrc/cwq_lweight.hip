// Call-time level weights and their gradient (cwq_rank_scores_w, cwq_rank_scores_backward_w,
// cwq_rank_ce_w).
//
// The Fast score is linear in the level weights w:
//   key_r = cw_r lp'_r + invL_r P[par_r],   P[p] = w_p lp'_p + P[par_p],   cw_r = w[depth_r] / L_r,
// and only three operands of the exact kernels carry them: RowMeta::cw (the exact leaf scan and
// the backward's row coefficients) and w_int (the exact internal pass and the backward's level
// pass).  lw_operands_kernel writes both for a device array of weights into the call's
// workspace -- the bits index_create_impl would have baked -- and the call's kernels read those
// instead of the index's.  The index is not modified.
//
// With g[q][r] = dloss/dkey_r, hL = invL_r g (grad_rows_kernel / ce_coef_kernel) and
// cI[q][p] = c[q][p] (grad_level_kernel):
//   dloss_q/dw[d] = sum_{rows r at depth d} hL[q][r] lp'_r(q) + sum_{internal p at depth d} cI[q][p] lp'_p(q)
// lp' = -(logdet + S)/2 from the raw sums S the exact internal pass leaves in the workspace, and
// for the rows the lp' the scan's EPI_KEYLP epilogue writes beside the key (cwq_rank_ce_w) or the
// raw sums of an EPI_RAW pass (cwq_rank_scores_backward_w, which has no forward of its own) --
// never from a key: w[d] = 0 is a legal weight.
//
// lw_grad_part_kernel: one workgroup per (part of kLwPart rows or nodes, query tile).  The
// part's lp' are transposed through LDS (the raw sums are query-major, the coefficients
// [query tile][row][16]); thread (sub, q) adds the fp64 products of rows sub, sub + 16, ... of
// one depth in index order, the 16 subs are summed in order, and the part writes one fp64 line
// [level][16] (zeros for the levels it does not hold).  lw_grad_reduce_kernel sums the parts in
// index order: 16 contiguous ranges, then the 16 range sums.  The cut is by the row index
// alone, there is no atomic: the same bits from run to run, for a query alone or in any batch
// or chunk.  fp64 because the depth-0 term of a cross-entropy gradient is a sum of ~n_sent
// products that cancels to near zero.
#include "cwq_internal.h"

namespace cwq {

namespace {

constexpr int kLQ = kXQ;   // queries per tile

__global__ __launch_bounds__(256) void lw_operands_kernel(const float* __restrict__ level_w, int n_w,
                                                          const RowMeta* __restrict__ meta,
                                                          const int* __restrict__ row_depth, int NL,
                                                          const int* __restrict__ int_depth, int NI,
                                                          RowMeta* __restrict__ meta_out,
                                                          float* __restrict__ w_int_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < NL) {
    RowMeta md = meta[i];
    const int d = row_depth[i];
    const double w = d < n_w ? (double)level_w[d] : 1.0;
    md.cw = (float)(w / (double)(d + 1));
    meta_out[i] = md;
  } else if (i - NL < NI) {
    const int d = int_depth[i - NL];
    w_int_out[i - NL] = d < n_w ? level_w[d] : 1.f;
  }
}

// One class (leaf-class rows or internal nodes) of n entries; parts [part0, part0 + ceil(n / kLwPart)).
struct LwClass {
  const float* coef;      // [qtiles][n][16]
  const float* S;         // [nq][ldS] raw sums, or lp' itself when logdet is null
  int64_t ldS;
  const float* logdet;    // [n] or null
  const int* depth;       // [n]
  int n, part0;
};

__global__ __launch_bounds__(256) void lw_grad_part_kernel(const LwClass c, int nq, int nlev, int npart,
                                                           double* __restrict__ part) {
  __shared__ float s_lp[kLwPart][kLQ + 1];
  __shared__ int s_dep[kLwPart];
  __shared__ int s_lo[4], s_hi[4];
  __shared__ double red[16][kLQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.y;
  const int r0 = blockIdx.x * kLwPart;
  const int r = r0 + tid;
  const int nqt = min(kLQ, nq - qt * kLQ);
  int dep = -1;
  float ld = 0.f;
  if (r < c.n) {
    dep = c.depth[r];
    if (c.logdet) ld = c.logdet[r];
  }
  s_dep[tid] = dep;
  for (int q = 0; q < kLQ; ++q) {
    float lp = 0.f;
    if (r < c.n && q < nqt) {
      const float sv = c.S[((int64_t)qt * kLQ + q) * c.ldS + r];
      lp = c.logdet ? -0.5f * (ld + sv) : sv;
    }
    s_lp[tid][q] = lp;
  }
  int lo = dep < 0 ? nlev : dep, hi = dep;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    lo = min(lo, __shfl_xor(lo, s, 64));
    hi = max(hi, __shfl_xor(hi, s, 64));
  }
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  const int dmin = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
  const int dmax = min(nlev - 1, max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3])));
  const int q = tid & 15, sub = tid >> 4;
  const float* __restrict__ cf = c.coef + ((size_t)qt * c.n + r0) * kLQ;
  double* __restrict__ out = part + ((size_t)qt * npart + c.part0 + blockIdx.x) * nlev * kLQ;
  for (int d = tid >> 4; d < nlev; d += 16)   // the levels this part does not hold
    if (d < dmin || d > dmax) out[(size_t)d * kLQ + q] = 0.0;
  for (int d = dmin; d <= dmax; ++d) {
    double acc = 0.0;
#pragma unroll 4
    for (int i = 0; i < kLwPart / 16; ++i) {
      const int rr = i * 16 + sub;
      if (s_dep[rr] == d) acc += (double)cf[(size_t)rr * kLQ + q] * (double)s_lp[rr][q];
    }
    red[sub][q] = acc;
    __syncthreads();
    if (sub == 0) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += red[k][q];
      out[(size_t)d * kLQ + q] = t;
    }
    __syncthreads();
  }
}

// grad_w[q][d] = sum over the parts in index order (16 contiguous ranges, then the 16 range
// sums), d < n_w; a level deeper than the tree is zero.
__global__ __launch_bounds__(256) void lw_grad_reduce_kernel(const double* __restrict__ part, int npart, int nlev,
                                                             int nq, int n_w, float* __restrict__ grad_w) {
  __shared__ double red[16][kLQ];
  const int q = threadIdx.x & 15, sub = threadIdx.x >> 4;
  const int qt = blockIdx.x, d = blockIdx.y;
  const int64_t gq = (int64_t)qt * kLQ + q;
  double s = 0.0;
  if (d < nlev) {
    const int per = (npart + 15) / 16;
    const int lo = sub * per, hi = min(npart, lo + per);
    const double* __restrict__ p = part + ((size_t)qt * npart * nlev + d) * kLQ + q;
    for (int i = lo; i < hi; ++i) s += p[(size_t)i * nlev * kLQ];
  }
  red[sub][q] = s;
  __syncthreads();
  if (sub == 0 && gq < nq) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][q];
    grad_w[gq * n_w + d] = (float)t;
  }
}

}  // namespace

hipError_t launch_lw_operands(const float* level_w, int n_w, const RowMeta* meta, const int* row_depth, int NL,
                              const int* int_depth, int NI, RowMeta* meta_out, float* w_int_out, hipStream_t s) {
  const int n = NL + NI;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(lw_operands_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, level_w, n_w, meta,
                     row_depth, NL, int_depth, NI, meta_out, w_int_out);
  return hipGetLastError();
}

int lw_parts(int NL, int NI) { return (NL + kLwPart - 1) / kLwPart + (NI + kLwPart - 1) / kLwPart; }

hipError_t launch_lw_grad(const LwGradArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.n_w <= 0) return hipSuccess;
  const int np_rows = (a.NL + kLwPart - 1) / kLwPart, np_int = (a.NI + kLwPart - 1) / kLwPart;
  const int npart = np_rows + np_int;
  if (np_rows > 0) {
    const LwClass c{a.hL, a.S_row, a.ldS_row, a.logdet_row, a.row_depth, a.NL, 0};
    hipLaunchKernelGGL(lw_grad_part_kernel, dim3((unsigned)np_rows, (unsigned)a.qtiles), dim3(256), 0, s, c, a.nq,
                       a.nlev, npart, a.part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (np_int > 0) {
    const LwClass c{a.cI, a.S_int, a.ldS_int, a.logdet_int, a.int_depth, a.NI, np_rows};
    hipLaunchKernelGGL(lw_grad_part_kernel, dim3((unsigned)np_int, (unsigned)a.qtiles), dim3(256), 0, s, c, a.nq,
                       a.nlev, npart, a.part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(lw_grad_reduce_kernel, dim3((unsigned)a.qtiles, (unsigned)a.n_w), dim3(256), 0, s, a.part, npart,
                     a.nlev, a.nq, a.n_w, a.grad_w);
  return hipGetLastError();
}

}  // namespace cwq
