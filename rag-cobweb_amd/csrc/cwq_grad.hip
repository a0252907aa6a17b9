// Backward pass of cwq_rank_scores: grad_x of the sentence scores (CobwebWrapper.py:267-294
// "Differentiable: return raw scores for all leaves").  DESIGN.md §4.11.
//
// A sentence's score is the key of its leaf-class row r,
//   key_r = cw_r lp'_r + invL_r P[par_r],   P[p] = w_p lp'_p + P[par_p],
//   lp'(n) = -(sum_d log v_nd + sum_d (x_d - mu_nd)^2 / v_nd) / 2,
// so with upstream gradients G[q][s]
//   grad_x[q][d] = - sum_n coef[q][n] (x_qd - mu_nd) / v_nd
// over every leaf-class row and internal node n, where
//   g[q][r]    = sum of G[q][s] over the sentences of row r      (grad_rows_kernel, CSR gather)
//   coef[q][r] = cw_r g[q][r]                                    (leaf-class rows)
//   c[q][p]    = sum_{leaf rows r under p} invL_r g[q][r] + sum_{internal children k} c[q][k]
//   coef[q][p] = w_p c[q][p]                                     (internal nodes, deepest level first)
// Every sum is a gather in a fixed order: no float atomics, results reproducible bit for bit,
// and a query's gradient does not depend on the other queries of the call.
//
// The hot kernel (grad_stream_kernel) is a split-K streaming reduction over the rows: a
// workgroup owns a slab of rows and a [16 queries x DP] fp32 accumulator tile in registers,
// reads every mean row once, and writes its partial tile [slab][query][DP]; grad_reduce_kernel
// sums the slabs in index order.  Coefficients are stored [query tile][row][16]: the 16
// coefficients of a row are one 64-B line, uniform over the wave that handles the row.
#include "cwq_internal.h"

namespace cwq {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kGQ = kXQ;          // queries per tile
constexpr int kGradDimChunk = 1024;   // dims per workgroup (blockIdx.z chunks beyond)

// ---------------------------------------------------------------------------
// Coefficient pass
// ---------------------------------------------------------------------------
// g[q][r] through the row -> sentences CSR; coefL = sc_r g (sc_r = cw_r iv_r for isotropic
// rows, whose stream term is (x - mu); cw_r otherwise) and hL = invL_r g (the parent's share).
// Sentences outside the CSR (row_of_sent < 0) are never read.
__global__ __launch_bounds__(256) void grad_rows_kernel(const float* __restrict__ G, int64_t n_sent, int nq,
                                                        const int64_t* __restrict__ sent_ptr,
                                                        const int64_t* __restrict__ sent_ids,
                                                        const RowMeta* __restrict__ meta, int NL, int NL_iso,
                                                        float* __restrict__ coefL, float* __restrict__ hL) {
  __shared__ float tc[64][kGQ + 1], th[64][kGQ + 1];
  const int qt = blockIdx.y;
  const int r0 = blockIdx.x * 64;
  const int rl = threadIdx.x & 63, qg = threadIdx.x >> 6;
  const int r = r0 + rl;
  int64_t s0 = 0, s1 = 0;
  float sc = 0.f, il = 0.f;
  if (r < NL) {
    s0 = sent_ptr[r];
    s1 = sent_ptr[r + 1];
    const RowMeta md = meta[r];
    sc = r < NL_iso ? md.cw * md.iv : md.cw;
    il = md.invL;
  }
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    const int q = qg * 4 + qi;
    const int64_t gq = (int64_t)qt * kGQ + q;
    float g = 0.f;
    if (gq < nq)
      for (int64_t s = s0; s < s1; ++s) g += G[gq * n_sent + sent_ids[s]];
    tc[rl][q] = s1 > s0 ? sc * g : 0.f;
    th[rl][q] = s1 > s0 ? il * g : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * kGQ; i += 256) {
    const int rr = i >> 4, q = i & 15;
    if (r0 + rr < NL) {
      const size_t o = ((size_t)qt * NL + r0 + rr) * kGQ + q;
      coefL[o] = tc[rr][q];
      hL[o] = th[rr][q];
    }
  }
}

// Sum of src[qt][r][q] over r in [lo, hi) by this thread's part (stride P), in index order.
__device__ __forceinline__ float part_sum(const float* __restrict__ src, int lo, int hi, int part, int P, int q) {
  float s = 0.f;
  int r = lo + part;
  for (; r + 7 * P < hi; r += 8 * P) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(r + u * P) * kGQ + q];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; r < hi; r += P) s += src[(size_t)r * kGQ + q];
  return s;
}

// The P parts of a node summed in part order (P == 16: one node per workgroup).
__device__ __forceinline__ float parts_total(float s, int P, int sub, int q, float (*red)[kGQ]) {
  if (P == 1) return s;
  red[sub][q] = s;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) t += red[k][q];
  return t;
}

// cz[z][qt][p][q] = the z-th split of sum_{leaf rows r under p} hL[qt][r][q]: a node's
// isotropic and anisotropic child rows are two contiguous ranges (int_leaf_a0..b1), each cut
// into nsplit pieces (a flat tree's root has every row as a child).  P = 16: one node per
// workgroup, 16 strided parts per query; P = 1: 16 nodes per workgroup.
__global__ __launch_bounds__(256) void grad_leafsum_kernel(const float* __restrict__ hL, int NL, int NI, int P,
                                                           int nsplit, const int* __restrict__ a0,
                                                           const int* __restrict__ a1, const int* __restrict__ b0,
                                                           const int* __restrict__ b1, float* __restrict__ cz) {
  __shared__ float red[16][kGQ];
  const int q = threadIdx.x & 15, sub = threadIdx.x >> 4;
  const int qt = blockIdx.y, z = blockIdx.z;
  const int p = P == 16 ? (int)blockIdx.x : (int)blockIdx.x * 16 + sub;
  const int part = P == 16 ? sub : 0;
  const float* src = hL + (size_t)qt * NL * kGQ;
  float s = 0.f;
  if (p < NI) {
    const int lo[2] = {a0[p], b0[p]}, hi[2] = {a1[p], b1[p]};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int n = hi[c] - lo[c];
      if (n <= 0) continue;
      const int ch = (n + nsplit - 1) / nsplit;
      const int l = lo[c] + z * ch;
      const int h = min(hi[c], l + ch);
      s += part_sum(src, l, h, part, P, q);
    }
  }
  const float t = parts_total(s, P, sub, q, red);
  if (p < NI && part == 0) cz[(((size_t)z * gridDim.y + qt) * NI + p) * kGQ + q] = t;
}

// One level [i0, i1) of internal nodes, after every deeper level:
// c[p] = sum_z cz[z][p] + sum_{internal children k} c[k] (contiguous, index order), coefI = w_p c[p].
__global__ __launch_bounds__(256) void grad_level_kernel(int i0, int i1, int NI, int P, int nsplit,
                                                         const float* __restrict__ cz,
                                                         const int* __restrict__ cb, const int* __restrict__ ce,
                                                         const float* __restrict__ w_int, float* cI,
                                                         float* __restrict__ coefI) {
  __shared__ float red[16][kGQ];
  const int q = threadIdx.x & 15, sub = threadIdx.x >> 4;
  const int qt = blockIdx.y;
  const int p = i0 + (P == 16 ? (int)blockIdx.x : (int)blockIdx.x * 16 + sub);
  const int part = P == 16 ? sub : 0;
  float s = 0.f;
  if (p < i1) s = part_sum(cI + (size_t)qt * NI * kGQ, cb[p], ce[p], part, P, q);
  float t = parts_total(s, P, sub, q, red);
  if (p < i1 && part == 0) {
    float l = 0.f;
    for (int z = 0; z < nsplit; ++z) l += cz[(((size_t)z * gridDim.y + qt) * NI + p) * kGQ + q];
    t += l;
    const size_t o = ((size_t)qt * NI + p) * kGQ + q;
    cI[o] = t;
    coefI[o] = w_int[p] * t;
  }
}

// ---------------------------------------------------------------------------
// Streaming reduction
// ---------------------------------------------------------------------------
struct StreamK {
  const float* q;        // [nq][D] caller queries
  int nq, D, DP;
  const float* M;        // row-major rows [nrows][DP] (isotropic), or
  const float* A;        // dim-major A, B [DP][ld]
  const float* B;
  int64_t ld;
  int nrows, rows_per_slab;
  const float* coef;     // [qtiles][ncoef][16]; this class's rows start at coef_base
  int ncoef, coef_base;
  float* part;           // [nslab_total][nq16][DP]
  int slab_off, nq16;
  int rt;                // dim-major: rows per LDS tile (4 or 8)
  const int* list;       // LIST: the class's rows to walk, list[0, nrows) (slabs by list position)
};

// the 16 coefficients of a row: a wave-uniform address (scalar loads)
__device__ __forceinline__ void load_coef(const float* __restrict__ cf, f2 (&c)[kGQ / 2]) {
#pragma unroll
  for (int k = 0; k < kGQ / 2; ++k) {
    c[k].x = cf[2 * k];
    c[k].y = cf[2 * k + 1];
  }
}

// TPR threads share a row (a multiple of 64: the row is wave-uniform), J dims per thread;
// 256 / TPR row groups take the slab's rows in turn and are summed in group order at the end.
// DM: dim-major operands, staged through LDS in tiles of a.rt rows (coalesced along rows).
// LIST (the masked loss's gathered backward): positions r_begin .. r_end walk
// a.list, whose entries are the class rows to read (means and coefficients by row id); a
// group's row is still wave-uniform.  !LIST is the code without the indirection.
template <int TPR, int J, bool DM, bool LIST>
__global__ __launch_bounds__(256) void grad_stream_kernel(const StreamK a) {
  extern __shared__ float lds[];
  constexpr int RG = 256 / TPR;
  const int tid = threadIdx.x;
  const int grp = __builtin_amdgcn_readfirstlane(tid / TPR);
  const int tl = tid % TPR;
  const int qt = blockIdx.y;
  const int d0 = blockIdx.z * kGradDimChunk;
  const int DPc = min(a.DP - d0, kGradDimChunk);
  const int r_begin = blockIdx.x * a.rows_per_slab;
  const int r_end = min(a.nrows, r_begin + a.rows_per_slab);
  const float* __restrict__ coef = a.coef + ((size_t)qt * a.ncoef + a.coef_base) * kGQ;

  f2 x[J][kGQ / 2], acc[J][kGQ / 2];
  bool dok[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int dl = tl + TPR * j;
    dok[j] = dl < DPc;
    const int d = d0 + dl;
#pragma unroll
    for (int k = 0; k < kGQ / 2; ++k) {
      const int64_t g0 = (int64_t)qt * kGQ + 2 * k;
      x[j][k].x = (dok[j] && d < a.D && g0 < a.nq) ? a.q[g0 * a.D + d] : 0.f;
      x[j][k].y = (dok[j] && d < a.D && g0 + 1 < a.nq) ? a.q[(g0 + 1) * a.D + d] : 0.f;
      acc[j][k] = f2{0.f, 0.f};
    }
  }

  if (!DM) {
    constexpr int U = 4;   // rows in flight per group
    for (int r = r_begin + grp; r < r_end; r += RG * U) {
      float m[U][J];
      int row[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rr = r + u * RG;
        row[u] = LIST ? (rr < r_end ? a.list[rr] : 0) : rr;
#pragma unroll
        for (int j = 0; j < J; ++j)
          m[u][j] = (rr < r_end && dok[j]) ? a.M[(size_t)row[u] * a.DP + d0 + tl + TPR * j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rr = r + u * RG;
        if (rr < r_end) {
          f2 c[kGQ / 2];
          load_coef(coef + (size_t)row[u] * kGQ, c);
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const f2 mm = f2{m[u][j], m[u][j]};
#pragma unroll
            for (int k = 0; k < kGQ / 2; ++k) acc[j][k] = c[k] * (x[j][k] - mm) + acc[j][k];
          }
        }
      }
    }
  } else {
    const int RT = a.rt;
    const int st = DPc + 1;
    float* sA = lds;
    float* sB = lds + RT * st;
    const int lr = tid & (RT - 1), ld0 = tid / RT, lstep = 256 / RT;
    for (int R0 = r_begin; R0 < r_end; R0 += RT) {
      __syncthreads();   // the previous tile's readers (and nothing before the first)
      const int srow = LIST ? (R0 + lr < r_end ? a.list[R0 + lr] : 0) : R0 + lr;
      for (int d = ld0; d < DPc; d += lstep) {
        const int rr = R0 + lr;
        const size_t o = (size_t)(d0 + d) * a.ld + srow;
        sA[lr * st + d] = rr < r_end ? a.A[o] : 0.f;
        sB[lr * st + d] = rr < r_end ? a.B[o] : 0.f;
      }
      __syncthreads();
      for (int t = grp; t < RT; t += RG) {
        const int rr = R0 + t;
        if (rr >= r_end) break;
        f2 c[kGQ / 2];
        load_coef(coef + (size_t)(LIST ? a.list[rr] : rr) * kGQ, c);
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (!dok[j]) continue;
          const float av = sA[t * st + tl + TPR * j], bv = sB[t * st + tl + TPR * j];
          const f2 aa = f2{av, av}, bb = f2{bv, bv};
#pragma unroll
          for (int k = 0; k < kGQ / 2; ++k) acc[j][k] = (c[k] * aa) * (x[j][k] * aa - bb) + acc[j][k];
        }
      }
    }
    __syncthreads();   // the tile buffer becomes the group reduction's
  }

  if (RG > 1) {   // groups summed into group 0 in the order RG-1, ..., 1
    constexpr int W = TPR * J;
    for (int g = RG - 1; g >= 1; --g) {
      if (grp == g) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
          for (int k = 0; k < kGQ / 2; ++k) {
            lds[(2 * k) * W + j * TPR + tl] = acc[j][k].x;
            lds[(2 * k + 1) * W + j * TPR + tl] = acc[j][k].y;
          }
      }
      __syncthreads();
      if (grp == g - 1) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
          for (int k = 0; k < kGQ / 2; ++k) {
            acc[j][k].x += lds[(2 * k) * W + j * TPR + tl];
            acc[j][k].y += lds[(2 * k + 1) * W + j * TPR + tl];
          }
      }
      __syncthreads();
    }
  }
  if (grp == 0) {
    const size_t slab = (size_t)a.slab_off + blockIdx.x;
#pragma unroll
    for (int k = 0; k < kGQ / 2; ++k) {
      const int64_t g0 = (int64_t)qt * kGQ + 2 * k;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        if (!dok[j]) continue;
        const int d = d0 + tl + TPR * j;
        if (g0 < a.nq) a.part[(slab * a.nq16 + g0) * a.DP + d] = acc[j][k].x;
        if (g0 + 1 < a.nq) a.part[(slab * a.nq16 + g0 + 1) * a.DP + d] = acc[j][k].y;
      }
    }
  }
}

// grad_q[q][d] = -sum_slab part[slab][q][d], d < D: 16 contiguous slab ranges per (q, d)
// summed in index order, then the 16 range sums in order.
__global__ __launch_bounds__(1024) void grad_reduce_kernel(const float* __restrict__ part, int nslab, int nq16,
                                                           int DP, int D, float* __restrict__ out) {
  __shared__ float red[16][64];
  const int tx = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + tx;
  const int64_t q = blockIdx.y;
  const int per = (nslab + 15) / 16;
  const int lo = sg * per, hi = min(nslab, lo + per);
  float s = 0.f;
  if (d < D) {
    const size_t st = (size_t)nq16 * DP;
    const float* p = part + (size_t)q * DP + d;
    int i = lo;
    for (; i + 8 <= hi; i += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(i + u) * st];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < hi; ++i) s += p[(size_t)i * st];
  }
  red[sg][tx] = s;
  __syncthreads();
  if (sg == 0 && d < D) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][tx];
    out[q * D + d] = -t;
  }
}

template <int TPR, int J, bool DM, bool LIST>
hipError_t launch_stream_tj(const StreamK& k, dim3 grid, size_t ldsb, hipStream_t s) {
  hipLaunchKernelGGL((grad_stream_kernel<TPR, J, DM, LIST>), grid, dim3(256), ldsb, s, k);
  return hipGetLastError();
}

template <bool DM, bool LIST>
hipError_t launch_stream_class(const StreamK& k, int tpr, int j, dim3 grid, size_t ldsb, hipStream_t s) {
#define CWQ_GRAD_CASE(T, JJ) \
  if (tpr == T && j == JJ) return launch_stream_tj<T, JJ, DM, LIST>(k, grid, ldsb, s);
  CWQ_GRAD_CASE(64, 1) CWQ_GRAD_CASE(64, 2) CWQ_GRAD_CASE(64, 3) CWQ_GRAD_CASE(64, 4)
  CWQ_GRAD_CASE(128, 1) CWQ_GRAD_CASE(128, 2) CWQ_GRAD_CASE(128, 3) CWQ_GRAD_CASE(128, 4)
  CWQ_GRAD_CASE(256, 1) CWQ_GRAD_CASE(256, 2) CWQ_GRAD_CASE(256, 3) CWQ_GRAD_CASE(256, 4)
#undef CWQ_GRAD_CASE
  return hipErrorInvalidValue;
}

}  // namespace

void grad_shape(int DP, int& tpr, int& j) {
  const int dpc = DP < kGradDimChunk ? DP : kGradDimChunk;
  int best_w = 1 << 30;
  tpr = 256;
  j = 4;
  for (int jj = 1; jj <= 4; ++jj)   // least idle lanes, then the fewest dims per thread
    for (int t = 64; t <= 256; t *= 2) {
      const int w = t * jj - dpc;
      if (w >= 0 && w < best_w) {
        best_w = w;
        tpr = t;
        j = jj;
      }
    }
}

int grad_rows_per_slab(int64_t weighted_rows, int cus) {
  // three workgroups per CU are resident (132 VGPRs at DP = 768): one round, 36 KiB of loads
  // in flight per CU; at least 256 rows, so the partial tiles stay a few percent of the stream
  const int64_t per = (weighted_rows + 3 * (int64_t)cus - 1) / (3 * (int64_t)cus);
  const int64_t s = per < 256 ? 256 : per;
  return (int)((s + 7) / 8 * 8);
}

hipError_t launch_grad_rows(const GradCoefArgs& a, hipStream_t s) {
  if (a.NL <= 0) return hipSuccess;
  hipLaunchKernelGGL(grad_rows_kernel, dim3((unsigned)((a.NL + 63) / 64), (unsigned)a.qtiles), dim3(256), 0, s, a.G,
                     a.n_sent, a.nq, a.sent_ptr, a.sent_ids, a.meta, a.NL, a.NL_iso, a.coefL, a.hL);
  return hipGetLastError();
}

hipError_t launch_grad_coef(const GradCoefArgs& a, hipStream_t s) {
  const hipError_t e = launch_grad_rows(a, s);
  return e != hipSuccess ? e : launch_grad_tree(a, s);
}

hipError_t launch_grad_tree(const GradCoefArgs& a, hipStream_t s) {
  const dim3 blk(256);
  if (a.NI <= 0) return hipSuccess;
  const int P = a.P;
  const unsigned nb = (unsigned)(P == 16 ? a.NI : (a.NI + 15) / 16);
  hipLaunchKernelGGL(grad_leafsum_kernel, dim3(nb, (unsigned)a.qtiles, (unsigned)a.nsplit), blk, 0, s, a.hL, a.NL, a.NI,
                     P, a.nsplit, a.leaf_a0, a.leaf_a1, a.leaf_b0, a.leaf_b1, a.cz);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int l = a.nlev - 1; l >= 0; --l) {
    const int i0 = a.lv[2 * l], i1 = a.lv[2 * l + 1];
    const unsigned n = (unsigned)(P == 16 ? i1 - i0 : (i1 - i0 + 15) / 16);
    hipLaunchKernelGGL(grad_level_kernel, dim3(n, (unsigned)a.qtiles), blk, 0, s, i0, i1, a.NI, P, a.nsplit, a.cz,
                       a.child_begin, a.child_end, a.w_int, a.cI, a.coefI);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_grad_stream(const GradStreamArgs& g, hipStream_t s) {
  if (g.nrows <= 0) return hipSuccess;
  StreamK k;
  k.q = g.q;
  k.nq = g.nq;
  k.D = g.D;
  k.DP = g.DP;
  k.M = g.M;
  k.A = g.A;
  k.B = g.B;
  k.ld = g.ld;
  k.nrows = g.nrows;
  k.rows_per_slab = g.rows_per_slab;
  k.coef = g.coef;
  k.ncoef = g.ncoef;
  k.coef_base = g.coef_base;
  k.part = g.part;
  k.slab_off = g.slab_off;
  k.nq16 = g.qtiles * kGQ;
  int tpr, j;
  grad_shape(g.DP, tpr, j);
  const int dpc = g.DP < kGradDimChunk ? g.DP : kGradDimChunk;
  k.rt = dpc > 512 ? 4 : 8;
  const int nslab = (g.nrows + g.rows_per_slab - 1) / g.rows_per_slab;
  const dim3 grid((unsigned)nslab, (unsigned)g.qtiles, (unsigned)((g.DP + kGradDimChunk - 1) / kGradDimChunk));
  const size_t red = tpr < 256 ? (size_t)kGQ * tpr * j * 4 : 0;
  k.list = g.list;
  if (g.M)
    return g.list ? launch_stream_class<false, true>(k, tpr, j, grid, red, s)
                  : launch_stream_class<false, false>(k, tpr, j, grid, red, s);
  const size_t tile = (size_t)2 * k.rt * (dpc + 1) * 4;
  const size_t ldsb = tile > red ? tile : red;
  return g.list ? launch_stream_class<true, true>(k, tpr, j, grid, ldsb, s)
                : launch_stream_class<true, false>(k, tpr, j, grid, ldsb, s);
}

hipError_t launch_grad_reduce(const float* part, int nslab, int qtiles, int nq, int DP, int D, float* out,
                              hipStream_t s) {
  hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)nq), dim3(1024), 0, s, part, nslab,
                     qtiles * kGQ, DP, D, out);
  return hipGetLastError();
}

}  // namespace cwq
