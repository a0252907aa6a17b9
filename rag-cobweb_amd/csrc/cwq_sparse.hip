// Sparse differentiable scores (no reference counterpart): forward and backward
// over a short per-query list of sentences instead of every leaf-class row.
//
//   pair_key_kernel     the exact Fast key of sentence ids[q][j]'s row.  The arithmetic is the
//                       exact scan's (16-dim fma partials in dim order, acc += part in slice
//                       order, iso_key_tail / the scan epilogue's anisotropic expression), so a
//                       score is the bits cwq_rank_scores writes in that column
//   sparse_grad_kernel  per query: the entries' rows, the upstream gradient summed over the
//                       entries of one row in entry order, then (role 0) the leaf-class rows'
//                       term of grad_q gathered row by row, (role 1) the ancestors' coefficients
//                       c[p] = sum invL_r g_r over the listed rows below p in entry order, written
//                       in cwq_grad.hip's [query tile][node][16] layout
//   sparse_scale_kernel coefI = w_int c; the internal nodes then go through grad_stream_kernel
//   ce_topk_kernel      one wave per query over its top-K list and the target's entry: max, z,
//                       loss, rank among the candidates, the bound on the truncated mass, g_j
// No float atomics: every sum has one fixed order, a query's outputs depend on nothing but the
// query and its own list.
#include "cwq_internal.h"
#include "cwq_exact.h"   // f32x16, CWQ_INF

namespace cwq {

namespace {

constexpr int kSpDC = 32;               // dims per staged chunk (DP is a multiple of 32)
constexpr int kSpStride = kSpDC + 1;    // LDS floats per staged row
constexpr int kSpQ = kXQ;               // queries per coefficient tile (cwq_grad.hip's)

__device__ __forceinline__ int row_of_id(int64_t id, int64_t n_sent, const int* __restrict__ row_of_sent) {
  return (id >= 0 && id < n_sent) ? row_of_sent[id] : -1;
}

// One wave per (query, 64 entries): lane = entry.  Isotropic rows are staged from the row-major
// copy Mf through LDS (8 lanes read one row's 128 B piece, every fetched line used whole; 33
// floats a row, so the lanes' reads of their own rows hit different banks); anisotropic rows
// exist only dim-major and each lane loads its own.  The query's 16-dim slices arrive by scalar
// loads from the scan's interleaved X layout.
__global__ __launch_bounds__(64) void pair_key_kernel(const SparsePairArgs a) {
  __shared__ float tile[64 * kSpStride];
  __shared__ int srow[64];
  const int lane = threadIdx.x;
  const int q = blockIdx.x;
  const int NV16 = a.DP / 16;
  const int NCH = a.DP / kSpDC;
  const f32x16* __restrict__ xg =
      reinterpret_cast<const f32x16*>(a.X) + (size_t)(q / kXQ) * NV16 * kXQ + (q % kXQ);
  for (int j0 = blockIdx.y * 64; j0 < a.m; j0 += gridDim.y * 64) {
    const int j = j0 + lane;
    int row = -1;
    if (j < a.m) row = row_of_id(a.ids[(size_t)q * a.ld_ids + j], a.n_sent, a.row_of_sent);
    const bool iso = row >= 0 && row < a.NL_iso;
    const bool an = row >= a.NL_iso;
    float acc = 0.f;
    if (__ballot(iso)) {   // NL_iso > 0 here: row 0 stands in for the other lanes
      __syncthreads();     // the previous round's reads
      srow[lane] = iso ? row : 0;
      __syncthreads();
      float4 g[8];
      size_t goff[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = lane + 64 * u;   // 64 rows x 8 float4
        goff[u] = (size_t)srow[idx >> 3] * a.DP + (idx & 7) * 4;
        g[u] = *reinterpret_cast<const float4*>(a.Mf + goff[u]);
      }
      for (int c = 0; c < NCH; ++c) {
        if (c > 0) __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = lane + 64 * u;
          float* t = tile + (idx >> 3) * kSpStride + (idx & 7) * 4;
          t[0] = g[u].x;
          t[1] = g[u].y;
          t[2] = g[u].z;
          t[3] = g[u].w;
        }
        __syncthreads();
        if (c + 1 < NCH) {
#pragma unroll
          for (int u = 0; u < 8; ++u) g[u] = *reinterpret_cast<const float4*>(a.Mf + goff[u] + (size_t)(c + 1) * kSpDC);
        }
        float m[kSpDC];
#pragma unroll
        for (int d = 0; d < kSpDC; ++d) m[d] = tile[lane * kSpStride + d];
#pragma unroll
        for (int h = 0; h < kSpDC / 16; ++h) {
          const f32x16 xa = xg[(size_t)(c * (kSpDC / 16) + h) * kXQ];
          float part;
#pragma unroll
          for (int d = 0; d < 16; ++d) {
            const float t = xa[d] - m[h * 16 + d];
            part = (d == 0) ? t * t : fmaf(t, t, part);
          }
          acc += part;
        }
      }
    }
    if (an) {
      acc = 0.f;   // the isotropic pass ran on a stand-in row for this lane
      const int r2 = row - a.NL_iso;
      for (int c = 0; c < NV16; ++c) {
        const f32x16 xa = xg[(size_t)c * kXQ];
        float av[16], bv[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) {
          av[d] = a.anA[(size_t)(c * 16 + d) * a.ld_an + r2];
          bv[d] = a.anB[(size_t)(c * 16 + d) * a.ld_an + r2];
        }
        float part;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
          const float t = fmaf(xa[d], av[d], -bv[d]);
          part = (d == 0) ? t * t : fmaf(t, t, part);
        }
        acc += part;
      }
    }
    if (j < a.m) {
      float key = -CWQ_INF;
      if (row >= 0) {
        const RowMeta md = a.meta[row];
        const int p = a.par[row];
        const float pp = p >= 0 ? a.P[(size_t)q * a.ldP + p] : 0.f;
        float lp;
        if (iso) {
          key = iso_key_tail(acc, md, pp, lp, 0, a.dconst);
        } else {
          lp = -0.5f * (md.logdet + a.dconst + acc);
          key = fmaf(pp, md.invL, md.cw * lp);
        }
      }
      a.out[(size_t)q * a.ld_out + j] = key;
    }
  }
}

// blockIdx.y: 0 the leaf-class rows' term into part[0][q][DP], 1 the ancestors' coefficients.
// Dynamic LDS: srow[m], keep[m] (int), sg[m] (float), then (role 1, a.c_lds) c[NI].
__global__ __launch_bounds__(256) void sparse_grad_kernel(const SparseGradArgs a) {
  extern __shared__ int sp_lds[];
  __shared__ int s_n;
  int* srow = sp_lds;
  int* keep = sp_lds + a.m;
  float* sg = reinterpret_cast<float*>(sp_lds + 2 * a.m);
  const int tid = threadIdx.x;
  const int q = blockIdx.x;
  const int role = blockIdx.y;
  const int m = a.m;
  for (int j = tid; j < m; j += 256) srow[j] = row_of_id(a.ids[(size_t)q * m + j], a.n_sent, a.row_of_sent);
  __syncthreads();
  // an entry is kept when no earlier entry names its row; it takes the later ones' gradients in
  // entry order.  Entries without a row (score -inf) are never read.
  for (int j = tid; j < m; j += 256) {
    const int r = srow[j];
    int first = r >= 0 ? 1 : 0;
    for (int i = 0; i < j && first; ++i) first = srow[i] != r;
    float g = 0.f;
    if (first)
      for (int i = j; i < m; ++i)
        if (srow[i] == r) g += a.g[(size_t)q * m + i];
    keep[j] = first;
    sg[j] = g;
  }
  __syncthreads();
  if (tid == 0) {   // compaction in entry order
    int n = 0;
    for (int j = 0; j < m; ++j)
      if (keep[j]) {
        srow[n] = srow[j];
        sg[n] = sg[j];
        ++n;
      }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n;

  if (role == 0) {
    // sg -> the stream coefficient sc_r g (grad_rows_kernel's: cw iv for isotropic rows)
    for (int j = tid; j < n; j += 256) {
      const int r = srow[j];
      const RowMeta md = a.meta[r];
      sg[j] = (r < a.NL_iso ? md.cw * md.iv : md.cw) * sg[j];
    }
    __syncthreads();
    for (int d = tid; d < a.DP; d += 256) {
      const float x = d < a.D ? a.q[(size_t)q * a.D + d] : 0.f;
      float acc = 0.f;
      for (int j = 0; j < n; ++j) {
        const int r = srow[j];
        const float c = sg[j];
        if (r < a.NL_iso) {
          acc = c * (x - a.Mf[(size_t)r * a.DP + d]) + acc;
        } else {
          const size_t o = (size_t)d * a.ld_an + (r - a.NL_iso);
          const float av = a.anA[o], bv = a.anB[o];
          acc = (c * av) * (x * av - bv) + acc;
        }
      }
      a.part[(size_t)q * a.DP + d] = acc;
    }
    return;
  }

  if (a.NI <= 0) return;
  const size_t tile_base = ((size_t)(q / kSpQ) * a.NI) * kSpQ + (q % kSpQ);   // + p * 16
  float* cl = reinterpret_cast<float*>(sp_lds + 3 * m);
  if (a.c_lds) {
    for (int p = tid; p < a.NI; p += 256) cl[p] = 0.f;
    __syncthreads();
  }
  if (tid == 0) {   // one thread, entry order, leaf's parent first: the order is the list's alone
    for (int j = 0; j < n; ++j) {
      const int r = srow[j];
      const float h = a.meta[r].invL * sg[j];
      for (int p = a.par[r]; p >= 0; p = a.par_int[p]) {
        if (a.c_lds)
          cl[p] += h;
        else
          a.cI[tile_base + (size_t)p * kSpQ] += h;   // zeroed before the launch
      }
    }
  }
  if (a.c_lds) {
    __syncthreads();
    for (int p = tid; p < a.NI; p += 256) a.cI[tile_base + (size_t)p * kSpQ] = cl[p];
  }
}

__global__ void sparse_scale_kernel(const float* __restrict__ cI, const float* __restrict__ w_int, int NI, size_t n,
                                    float* __restrict__ coefI) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    coefI[i] = w_int[(i / kSpQ) % NI] * cI[i];
}

__device__ __forceinline__ float sp_wave_max(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ float sp_wave_sum(float v) {   // butterfly: the same pairing on every run
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ int sp_wave_min(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ int sp_wave_sum(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// Lane l takes entries l, l + 64, ... of the query's top-K list in order, then the butterfly.
__global__ __launch_bounds__(64) void ce_topk_kernel(const SparseCeArgs a) {
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const int K = a.K;
  const float inf = CWQ_INF;
  const int64_t* __restrict__ tid = a.top_ids + q * K;
  const float* __restrict__ ts = a.top_scores + q * K;
  const int64_t t = a.target[q];
  bool tvalid = row_of_id(t, a.n_sent, a.row_of_sent) >= 0;
  int64_t n_in = 0;   // the sentences the full loss sums over: the tree's, or the mask's allowed ones
  if (a.slots) {
    const MaskSlot ms = a.slots[a.qslot ? a.qslot[q] : 0];
    tvalid = tvalid && ((ms.bits[t >> 5] >> (t & 31)) & 1u);
    n_in = ms.n_allowed;
  } else {
    n_in = a.sent_ptr[a.NL];
  }
  const float st = tvalid ? a.tscore[q] : -inf;
  float m = st;
  int pos = 0x7fffffff, nv = 0;
  for (int j = lane; j < K; j += 64) {
    const int64_t id = tid[j];
    if (id >= 0) {
      ++nv;
      m = fmaxf(m, ts[j]);
      if (tvalid && id == t) pos = min(pos, j);
    }
  }
  m = sp_wave_max(m);
  pos = sp_wave_min(pos);
  nv = sp_wave_sum(nv);
  const bool inside = pos != 0x7fffffff;
  float z = 0.f;
  for (int j = lane; j < K; j += 64)
    if (tid[j] >= 0) z += expf((ts[j] - m) * a.invT);
  z = sp_wave_sum(z);
  if (tvalid && !inside) z += expf((st - m) * a.invT);
  const float rz = 1.f / z;
  if (a.cand_ids)
    for (int j = lane; j < K; j += 64) a.cand_ids[q * K + j] = tid[j];
  if (a.bid) {   // the backward's list: the K entries, then the target when it is outside them
    int64_t* bid = a.bid + q * (K + 1);
    float* bg = a.bg + q * (K + 1);
    for (int j = lane; j < K; j += 64) {
      const int64_t id = tid[j];
      const bool on = tvalid && id >= 0;
      bid[j] = on ? id : -1;
      bg[j] = on ? (expf((ts[j] - m) * a.invT) * rz - (j == pos ? 1.f : 0.f)) * a.invT : 0.f;
    }
    if (lane == 0) {
      const bool on = tvalid && !inside;
      bid[K] = on ? t : -1;
      bg[K] = on ? (expf((st - m) * a.invT) * rz - 1.f) * a.invT : 0.f;
    }
  }
  if (lane == 0) {
    a.loss[q] = tvalid ? (m - st) * a.invT + logf(z) : inf;
    if (a.tscore_out) a.tscore_out[q] = st;
    if (a.rank) a.rank[q] = !tvalid ? -1 : inside ? pos + 1 : K + 1;
    if (a.tail_bound) {
      float b = 0.f;
      const int64_t rest = n_in - nv - (inside ? 0 : 1);   // sentences of the tree (the mask) outside C
      if (tvalid && nv == K && rest > 0) b = log1pf((float)rest * expf((ts[K - 1] - m) * a.invT) * rz);
      a.tail_bound[q] = b;
    }
  }
}

}  // namespace

hipError_t launch_sparse_pairs(const SparsePairArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.m <= 0) return hipSuccess;
  if (a.DP % kSpDC) return hipErrorInvalidValue;
  const unsigned gy = (unsigned)((a.m + 63) / 64 < 1024 ? (a.m + 63) / 64 : 1024);
  hipLaunchKernelGGL(pair_key_kernel, dim3((unsigned)a.nq, gy), dim3(64), 0, s, a);
  return hipGetLastError();
}

static size_t sparse_grad_lds(int m, int NI, bool* c_lds) {
  *c_lds = NI > 0 && (size_t)m * 12 + (size_t)NI * 4 <= (size_t)kSparseLdsBytes;
  return (size_t)m * 12 + (*c_lds ? (size_t)NI * 4 : 0);
}

hipError_t launch_sparse_grad(SparseGradArgs a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  if (a.m < 1 || a.m > kSparseMaxM) return hipErrorInvalidValue;
  bool c_lds;
  const size_t lds = sparse_grad_lds(a.m, a.NI, &c_lds);
  a.c_lds = c_lds ? 1 : 0;
  hipError_t e;
  if (a.NI > 0) {
    const size_t n = (size_t)a.qtiles * a.NI * kSpQ;
    if ((e = hipMemsetAsync(a.cI, 0, n * 4, s)) != hipSuccess) return e;   // also the tile's unused query slots
  }
  hipLaunchKernelGGL(sparse_grad_kernel, dim3((unsigned)a.nq, a.NI > 0 ? 2u : 1u), dim3(256), lds, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (a.NI > 0) {
    const size_t n = (size_t)a.qtiles * a.NI * kSpQ;
    hipLaunchKernelGGL(sparse_scale_kernel, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256),
                       0, s, a.cI, a.w_int, a.NI, n, a.coefI);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_ce_topk(const SparseCeArgs& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(ce_topk_kernel, dim3((unsigned)a.nq), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cwq
