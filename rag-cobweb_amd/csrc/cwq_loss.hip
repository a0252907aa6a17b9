// Cross-entropy ranking loss over all sentence scores, fused with its backward's coefficient
// pass (cwq_rank_ce): FixedDocsRankingLoss of the reference's query-encoder
// training (src/training/cobweb_query_train.py:104-126) and the two per-query numbers of its
// evaluate() (:213-304: the true document's score and rank), from the row keys the exact scan
// writes into the workspace.  No [nq][n_sent] array exists.
//
// A row r holds n_r sentences that all score key_r, so with T the temperature
//   lse[q]  = m/T + log z,  m = max_{n_r > 0} key_r,  z = sum_r n_r exp((key_r - m)/T)  (z >= 1)
//   loss[q] = lse - key_t/T = (m - key_t)/T + log z          (t the target's row)
//   dloss/dkey_r = g[q][r] = (n_r exp((key_r - m)/T)/z - [r == t]) / T
// and g is what grad_rows_kernel (cwq_grad.hip) would gather from a dense softmax - one-hot:
// ce_coef_kernel writes coefL = sc_r g, hL = invL_r g straight into the backward's layout.
// rank[q] = 1 + the sentences before the target under cwq_score_topk's documented order
// (higher key, then lower BFS node index, then lower sentence id): an integer count.
//
// Every reduction is cut by the row index alone (parts of kCePart rows; inside a part the
// thread, wave and part order are fixed) and combined in index order: no atomics, the same
// bits from run to run, for a query alone or in any batch or chunk.
#include <algorithm>

#include "cwq_internal.h"

namespace cwq {

namespace {

constexpr int kCQ = kXQ;                  // queries per tile
constexpr int kCeRows = kCePart / 256;    // rows per thread of a part

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}
// butterfly sums: the same pairing on every run (all lanes end with the same bits)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__device__ __forceinline__ bool ce_bit(const uint32_t* __restrict__ bits, int64_t s) {
  return (bits[s >> 5] >> (s & 31)) & 1u;
}
// The target's row, -1 for an invalid target.  MASKED (cwq_rank_ce_masked): the
// target must also be allowed and its row live.
template <bool MASKED>
__device__ __forceinline__ int ce_target_row(int64_t t, int64_t n_sent, const int* __restrict__ row_of_sent,
                                             const int* __restrict__ cnt, const uint32_t* __restrict__ bits) {
  int rt = -1;
  if (t >= 0 && t < n_sent) rt = row_of_sent[t];
  if constexpr (MASKED)
    if (rt >= 0 && !(ce_bit(bits, t) && cnt[rt] > 0)) rt = -1;
  return rt;
}

// MASKED, in the three kernels below: a row's sentence count is its allowed count cnt[r], the
// target is valid only when allowed; everything else is the same code.
// (m, z) of one part of rows per query, and the sentences of the part that precede the target.
// One workgroup per (part, query tile): a thread owns kCeRows rows (stride 256: a wave reads
// 64 consecutive keys of a query), whose sentence counts and BFS ids it loads once for the 16
// queries.  Per query: the wave's exact maximum, then the lane sums of n exp((key - max)/T),
// a butterfly sum; the four waves' pairs merged in wave order by thread q.
template <bool MASKED>
__global__ __launch_bounds__(256) void ce_part_kernel(const float* __restrict__ rowkey, int64_t ldr, int NL, int nq,
                                                      float invT, const int64_t* __restrict__ sent_ptr,
                                                      const int* __restrict__ row_bfs,
                                                      const int64_t* __restrict__ target, int64_t n_sent,
                                                      const int* __restrict__ row_of_sent, int want_rank, int npart,
                                                      float* __restrict__ pm, float* __restrict__ pz,
                                                      int* __restrict__ pc, const int* __restrict__ cnt,
                                                      const uint32_t* __restrict__ bits) {
  __shared__ float s_kt[kCQ], s_m[4][kCQ], s_z[4][kCQ];
  __shared__ int s_rt[kCQ], s_bt[kCQ], s_c[4][kCQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.y, part = blockIdx.x;
  const int r0 = part * kCePart;
  const float ninf = -__builtin_inff();
  if (tid < kCQ) {   // the target's row, key and BFS id, once
    const int64_t gq = (int64_t)qt * kCQ + tid;
    int rt = -1, bt = 0;
    float kt = 0.f;
    if (want_rank && gq < nq) {
      rt = ce_target_row<MASKED>(target[gq], n_sent, row_of_sent, cnt, bits);
      if (rt >= 0) {
        kt = rowkey[gq * ldr + rt];
        bt = row_bfs[rt];
      }
    }
    s_rt[tid] = rt;
    s_kt[tid] = kt;
    s_bt[tid] = bt;
  }
  int n[kCeRows], bfs[kCeRows];
#pragma unroll
  for (int j = 0; j < kCeRows; ++j) {
    const int r = r0 + j * 256 + tid;
    if constexpr (MASKED)
      n[j] = r < NL ? cnt[r] : 0;
    else
      n[j] = r < NL ? (int)(sent_ptr[r + 1] - sent_ptr[r]) : 0;
    bfs[j] = (want_rank && n[j] > 0) ? row_bfs[r] : 0;
  }
  __syncthreads();
  const int nqt = min(kCQ, nq - qt * kCQ);
  for (int q = 0; q < nqt; ++q) {
    const float* __restrict__ kp = rowkey + ((int64_t)qt * kCQ + q) * ldr + r0 + tid;
    float k[kCeRows];
#pragma unroll
    for (int j = 0; j < kCeRows; ++j) k[j] = n[j] > 0 ? kp[j * 256] : ninf;   // rows without sentences: skipped
    float m = k[0];
#pragma unroll
    for (int j = 1; j < kCeRows; ++j) m = fmaxf(m, k[j]);
    m = wave_max(m);
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < kCeRows; ++j)
      if (k[j] != ninf) z += (float)n[j] * expf((k[j] - m) * invT);
    z = wave_sum(z);
    int c = 0;
    const int rt = s_rt[q];
    if (rt >= 0) {
      const float kt = s_kt[q];
      const int bt = s_bt[q];
#pragma unroll
      for (int j = 0; j < kCeRows; ++j) {
        const bool before = k[j] > kt || (k[j] == kt && bfs[j] < bt);
        c += (n[j] > 0 && before && r0 + j * 256 + tid != rt) ? n[j] : 0;
      }
      c = wave_sum(c);
    }
    if (lane == 0) {
      s_m[wave][q] = m;
      s_z[wave][q] = z;
      s_c[wave][q] = c;
    }
  }
  __syncthreads();
  if (tid < nqt) {
    float m = s_m[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = fmaxf(m, s_m[w][tid]);
    float z = 0.f;
    int c = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (s_z[w][tid] != 0.f) z += s_z[w][tid] * expf((s_m[w][tid] - m) * invT);
      c += s_c[w][tid];
    }
    const size_t o = ((size_t)qt * kCQ + tid) * npart + part;
    pm[o] = m;
    pz[o] = z;
    pc[o] = c;
  }
}

// One wave per query: the parts merged (lane l takes parts l, l + 64, ... in order, then the
// butterfly), the target's place among its own row's sentences, and the four outputs;
// (m, 1/z) and the target's row (-1: invalid target) for ce_coef_kernel.
template <bool MASKED>
__global__ __launch_bounds__(64) void ce_final_kernel(const float* __restrict__ pm, const float* __restrict__ pz,
                                                      const int* __restrict__ pc, int npart,
                                                      const float* __restrict__ rowkey, int64_t ldr, float invT,
                                                      const int64_t* __restrict__ target, int64_t n_sent,
                                                      const int* __restrict__ row_of_sent,
                                                      const int64_t* __restrict__ sent_ptr,
                                                      const int64_t* __restrict__ sent_ids, float* __restrict__ loss,
                                                      float* __restrict__ tscore, int64_t* __restrict__ rank,
                                                      float2* __restrict__ mz, int* __restrict__ rtq,
                                                      const int* __restrict__ cnt,
                                                      const uint32_t* __restrict__ bits) {
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const float inf = __builtin_inff();
  const size_t o = (size_t)q * npart;
  float m = -inf;
  for (int p = lane; p < npart; p += 64) m = fmaxf(m, pm[o + p]);
  m = wave_max(m);
  float z = 0.f;
  int64_t c = 0;
  for (int p = lane; p < npart; p += 64) {
    const float zp = pz[o + p];
    if (zp != 0.f) z += zp * expf((pm[o + p] - m) * invT);
    if (rank) c += pc[o + p];
  }
  z = wave_sum(z);
  const int64_t t = target[q];
  const int rt = ce_target_row<MASKED>(t, n_sent, row_of_sent, cnt, bits);
  if (rank) {
    if (rt >= 0)   // the row's earlier (MASKED: allowed) sentence ids
      for (int64_t s = sent_ptr[rt] + lane; s < sent_ptr[rt + 1]; s += 64) {
        if constexpr (MASKED)
          c += (sent_ids[s] < t && ce_bit(bits, sent_ids[s])) ? 1 : 0;
        else
          c += sent_ids[s] < t ? 1 : 0;
      }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor((long long)c, s, 64);
  }
  if (lane == 0) {
    const float kt = rt >= 0 ? rowkey[q * ldr + rt] : -inf;
    loss[q] = rt >= 0 ? (m - kt) * invT + logf(z) : inf;
    if (tscore) tscore[q] = kt;
    if (rank) rank[q] = rt >= 0 ? 1 + c : -1;
    mz[q] = float2{m, 1.f / z};
    rtq[q] = rt;
  }
}

// grad_rows_kernel's grid, LDS transpose and output layout (cwq_grad.hip), with the gather of
// a dense upstream gradient replaced by the softmax itself: 64 rows x 16 queries per workgroup.
template <bool MASKED>
__global__ __launch_bounds__(256) void ce_coef_kernel(const float* __restrict__ rowkey, int64_t ldr, int nq,
                                                      float invT, const int64_t* __restrict__ sent_ptr,
                                                      const RowMeta* __restrict__ meta, int NL, int NL_iso,
                                                      const float2* __restrict__ mz, const int* __restrict__ rtq,
                                                      float* __restrict__ coefL, float* __restrict__ hL,
                                                      const int* __restrict__ cnt) {
  __shared__ float tc[64][kCQ + 1], th[64][kCQ + 1];
  const int qt = blockIdx.y;
  const int r0 = blockIdx.x * 64;
  const int rl = threadIdx.x & 63, qg = threadIdx.x >> 6;
  const int r = r0 + rl;
  int n = 0;
  float sc = 0.f, il = 0.f;
  if (r < NL) {
    if constexpr (MASKED)
      n = cnt[r];
    else
      n = (int)(sent_ptr[r + 1] - sent_ptr[r]);
    const RowMeta md = meta[r];
    sc = r < NL_iso ? md.cw * md.iv : md.cw;
    il = md.invL;
  }
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    const int q = qg * 4 + qi;
    const int64_t gq = (int64_t)qt * kCQ + q;
    float g = 0.f;
    if (gq < nq && n > 0) {
      const int rt = rtq[gq];
      if (rt >= 0) {   // an invalid target: a zero gradient row
        const float2 a = mz[gq];
        const float p = (float)n * expf((rowkey[gq * ldr + r] - a.x) * invT) * a.y;
        g = (p - (r == rt ? 1.f : 0.f)) * invT;   // the indicator once per row, whatever n is
      }
    }
    tc[rl][q] = n > 0 ? sc * g : 0.f;
    th[rl][q] = n > 0 ? il * g : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * kCQ; i += 256) {
    const int rr = i >> 4, q = i & 15;
    if (r0 + rr < NL) {
      const size_t o = ((size_t)qt * NL + r0 + rr) * kCQ + q;
      coefL[o] = tc[rr][q];
      hL[o] = th[rr][q];
    }
  }
}

}  // namespace

hipError_t launch_ce_reduce(const CeArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  hipError_t e;
  if ((a.cnt == nullptr) != (a.bits == nullptr)) return hipErrorInvalidValue;
  const bool masked = a.cnt != nullptr;
  if (a.npart > 0) {
    const auto part = masked ? ce_part_kernel<true> : ce_part_kernel<false>;
    hipLaunchKernelGGL(part, dim3((unsigned)a.npart, (unsigned)a.qtiles), dim3(256), 0, s, a.rowkey, a.ldr, a.NL, a.nq,
                       a.invT, a.sent_ptr, a.row_bfs, a.target, a.n_sent, a.row_of_sent, a.rank ? 1 : 0, a.npart, a.pm,
                       a.pz, a.pc, a.cnt, a.bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const auto fin = masked ? ce_final_kernel<true> : ce_final_kernel<false>;
  hipLaunchKernelGGL(fin, dim3((unsigned)a.nq), dim3(64), 0, s, a.pm, a.pz, a.pc, a.npart, a.rowkey, a.ldr, a.invT,
                     a.target, a.n_sent, a.row_of_sent, a.sent_ptr, a.sent_ids, a.loss, a.tscore, a.rank, a.mz, a.rtq,
                     a.cnt, a.bits);
  return hipGetLastError();
}

hipError_t launch_ce_coef(const CeArgs& a, const RowMeta* meta, int NL_iso, float* coefL, float* hL, hipStream_t s) {
  if (a.nq <= 0 || a.NL <= 0) return hipSuccess;
  const auto coef = a.cnt ? ce_coef_kernel<true> : ce_coef_kernel<false>;
  hipLaunchKernelGGL(coef, dim3((unsigned)((a.NL + 63) / 64), (unsigned)a.qtiles), dim3(256), 0, s, a.rowkey, a.ldr,
                     a.nq, a.invT, a.sent_ptr, meta, a.NL, NL_iso, a.mz, a.rtq, coefL, hL, a.cnt);
  return hipGetLastError();
}

namespace {
__global__ __launch_bounds__(256) void mask_counts_kernel(const uint8_t* __restrict__ live,
                                                          const int64_t* __restrict__ sent_ptr,
                                                          const int64_t* __restrict__ sent_ids,
                                                          const uint32_t* __restrict__ bits, int NL,
                                                          int* __restrict__ cnt) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= NL) return;
  int c = 0;
  if (live[r])   // a dead row holds no allowed sentence: its list is never read
    for (int64_t s = sent_ptr[r]; s < sent_ptr[r + 1]; ++s) c += ce_bit(bits, sent_ids[s]) ? 1 : 0;
  cnt[r] = c;
}

__global__ __launch_bounds__(256) void ce_invalid_kernel(int64_t nq, int D, float* __restrict__ loss,
                                                         float* __restrict__ grad_q, float* __restrict__ tscore,
                                                         int64_t* __restrict__ rank) {
  const int64_t n = grad_q ? nq * D : nq;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (grad_q) grad_q[i] = 0.f;
    if (i < nq) {
      loss[i] = __builtin_inff();
      if (tscore) tscore[i] = -__builtin_inff();
      if (rank) rank[i] = -1;
    }
  }
}
}  // namespace

hipError_t launch_mask_counts(const uint8_t* live, const int64_t* sent_ptr, const int64_t* sent_ids,
                              const uint32_t* bits, int NL, int* cnt, hipStream_t s) {
  if (NL <= 0) return hipSuccess;
  hipLaunchKernelGGL(mask_counts_kernel, dim3((unsigned)((NL + 255) / 256)), dim3(256), 0, s, live, sent_ptr, sent_ids,
                     bits, NL, cnt);
  return hipGetLastError();
}

hipError_t launch_ce_invalid(int64_t nq, int D, float* loss, float* grad_q, float* tscore, int64_t* rank,
                             hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  const int64_t n = grad_q ? nq * std::max(D, 1) : nq;
  hipLaunchKernelGGL(ce_invalid_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, nq, D,
                     loss, grad_q, tscore, rank);
  return hipGetLastError();
}

}  // namespace cwq
