// Masked Fast top-k (cwq_score_topk_masked; no reference counterpart): the kernels
// that restrict a query to an allowed sentence set.
//
//   mask build     sentence bitset -> one live flag per leaf-class row (a row is live when one of
//                  its sentences is allowed) -> two ascending row lists (isotropic / anisotropic
//                  segment) by a block count, a scan of the block counts and a compaction
//   gathered scan  the exact fp32 keys of the listed rows only, into per-slab sorted top-K lists
//                  like scan_kernel's EPI_TOPK.  The arithmetic is the exact scan's: 16-dim fma
//                  partials in dim order, acc += part in slice order, iso_key_tail -- so the keys
//                  are the exact scan's bit for bit
//   merge-expand   merge_expand_kernel's merge, then the rows' ALLOWED sentences only
//   compaction     the allowed entries of an unmasked top-k' result, in order (over-fetch path)
//   k > 64         the keys of the rows that are not live set to -inf before the full sort, and
//                  a masked expansion of the sorted rows
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cwq_internal.h"
#include "cwq_exact.h"

namespace cwq {

__device__ __forceinline__ bool bit_set(const uint32_t* __restrict__ bits, int64_t s) {
  return (bits[s >> 5] >> (s & 31)) & 1u;
}

// ---------------------------------------------------------------------------
// Mask build
// ---------------------------------------------------------------------------
// live[r] = row r holds an allowed sentence; *n_allowed += the allowed sentences in the tree
__global__ __launch_bounds__(256) void mask_rows_kernel(const uint32_t* __restrict__ bits,
                                                        const int64_t* __restrict__ sent_ptr,
                                                        const int64_t* __restrict__ sent_ids,
                                                        const int* __restrict__ flags, int NL, uint8_t* live,
                                                        unsigned long long* n_allowed) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  int c = 0;
  if (r < NL) {
    for (int64_t s = sent_ptr[r]; s < sent_ptr[r + 1]; ++s) c += bit_set(bits, sent_ids[s]) ? 1 : 0;
    live[r] = (c > 0 && (flags[r] & FLAG_HAS_SENT)) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c > 0) atomicAdd(n_allowed, (unsigned long long)c);
}

constexpr int kMaskBlk = 1024;   // rows per block of the list build (4 per thread)

__global__ __launch_bounds__(256) void mask_block_count_kernel(const uint8_t* __restrict__ live, int n, int* bc) {
  __shared__ int sw[4];
  const int r0 = blockIdx.x * kMaskBlk + threadIdx.x * 4;
  int c = 0;
  for (int j = 0; j < 4; ++j)
    if (r0 + j < n) c += live[r0 + j];
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) bc[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// exclusive scan of bc[0..nb) in place (one workgroup, 1024 counts a round), total to *out
__global__ __launch_bounds__(1024) void mask_block_scan_kernel(int* bc, int nb, int* out) {
  __shared__ int sh[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int i = b0 + (int)threadIdx.x;
    const int v = i < nb ? bc[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int t = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    const int incl = sh[threadIdx.x], base = carry;
    if (i < nb) bc[i] = base + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = carry;
}

// rows[bc[block] + rank within the block] = r for the live rows r of the block, ascending
__global__ __launch_bounds__(256) void mask_compact_kernel(const uint8_t* __restrict__ live, int n,
                                                           const int* __restrict__ bc, int* rows) {
  __shared__ int sh[256];
  const int r0 = blockIdx.x * kMaskBlk + threadIdx.x * 4;
  int c = 0;
  for (int j = 0; j < 4; ++j)
    if (r0 + j < n) c += live[r0 + j];
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int t = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  int o = bc[blockIdx.x] + sh[threadIdx.x] - c;
  for (int j = 0; j < 4; ++j)
    if (r0 + j < n && live[r0 + j]) rows[o++] = r0 + j;
}

hipError_t launch_mask_build(const uint32_t* bits, const int64_t* sent_ptr, const int64_t* sent_ids, const int* flags,
                             int NL_iso, int NL_an, uint8_t* live, int* rows_iso, int* rows_an, int* bc,
                             unsigned long long* n_allowed, int* counts2, hipStream_t s) {
  const int NL = NL_iso + NL_an;
  hipError_t e = hipMemsetAsync(n_allowed, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(counts2, 0, 2 * sizeof(int), s)) != hipSuccess) return e;
  if (NL == 0) return hipSuccess;
  hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)((NL + 255) / 256)), dim3(256), 0, s, bits, sent_ptr, sent_ids,
                     flags, NL, live, n_allowed);
  const int seg_n[2] = {NL_iso, NL_an}, seg_base[2] = {0, NL_iso};
  int* seg_rows[2] = {rows_iso, rows_an};
  for (int i = 0; i < 2; ++i) {
    const int n = seg_n[i];
    if (n == 0) continue;
    const int nb = (n + kMaskBlk - 1) / kMaskBlk;
    hipLaunchKernelGGL(mask_block_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, live + seg_base[i], n, bc);
    hipLaunchKernelGGL(mask_block_scan_kernel, dim3(1), dim3(1024), 0, s, bc, nb, counts2 + i);
    hipLaunchKernelGGL(mask_compact_kernel, dim3((unsigned)nb), dim3(256), 0, s, live + seg_base[i], n, bc,
                       seg_rows[i]);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The gathered exact scan.
// A workgroup owns one tile of the row list at a time (of its slab of the list) and a block of
// queries; lane = row, the queries arrive by scalar loads from the scan's interleaved X layout
// (a query's 16-dim slice feeds every row a lane owns).  Two forms, like scan_kernel's:
//   !SHQ  a 64-row tile; the 4 waves share the tile and own kXQ queries each (64 queries a
//         workgroup)
//    SHQ  small calls: a 256-row tile, the 4 waves share kXQ queries and own 64 rows each, one
//         list per wave (4 lists a slab)
// One row a lane in both: two rows a lane (scan_kernel's hot form) halve the scalar query loads
// per row but measured slower here (12.6 against 14.4 G row-queries/s at C3, 10k queries): at
// 178+ VGPRs too few waves are resident to hide the loads.
// Isotropic rows come from the row-major fp32 copy Mf[row][DP]: the workgroup gathers 32 dims
// of the tile's rows into LDS (128 B a row: 8 neighbouring threads read one row's piece, so
// every fetched cache line is used whole), padded to 33 floats a row so that the lanes' reads
// of their own rows hit 64 different banks; the next chunk's global loads fly during the
// current chunk's arithmetic.  Anisotropic rows exist only dim-major (A, B [DP][ld]): each lane
// loads its rows' values itself (a sparse list wastes most of each cache line there; such rows
// are few).  Grid: slab * n_qblocks + query block (queries fastest, so a tile is read from
// HBM once and then from L2).
// ---------------------------------------------------------------------------
// the planner (cwq_maskplan.h, host only) restates these; scripts/maskplan_check.cpp's bounds
// proof holds for the kernel only while they agree
static_assert(kMpXQ == kXQ && kMpWaves == kWavesPerWG, "cwq_maskplan.h: query group / waves per workgroup");
static_assert(mp_tile(false) == mask_scan_tile(false) && mp_tile(true) == mask_scan_tile(true), "cwq_maskplan.h: tile");
static_assert(mp_lists(false) == mask_scan_lists(false) && mp_lists(true) == mask_scan_lists(true),
              "cwq_maskplan.h: lists per slab");
static_assert(mp_qblock(false) == kXQ * kWavesPerWG && mp_qblock(true) == kXQ, "cwq_maskplan.h: queries per block");
constexpr int kMsDC = 32;              // dims per staged chunk (DP is a multiple of 32)
constexpr int kMsStride = kMsDC + 1;   // LDS floats per row

// GRP (the grouped form): the slab, the row list, the queries and the lists come
// from the workgroup's work item work[blockIdx.x] instead of blockIdx.x and `a` (one launch per
// segment and form serves every mask of a call); everything else is the same code.
// KEYS (the masked loss's gathered forward): the keys of the listed rows go to
// a.rowkey[q][global row] instead of into top-K lists -- the same arithmetic, the same bits.
template <bool ISO, int KL, bool SHQ, bool GRP, bool KEYS = false>
__global__ __launch_bounds__(256) void mask_scan_kernel(const float* __restrict__ X, const float* __restrict__ A,
                                                        const float* __restrict__ B, const MaskScanArgs a,
                                                        const MaskWork* __restrict__ work) {
  const MaskWork* __restrict__ w = GRP ? work + blockIdx.x : nullptr;
  constexpr int TQ = kXQ;
  constexpr int QPR = 64 / KL;
  constexpr int NLR = (TQ + QPR - 1) / QPR;
  constexpr int TILE = SHQ ? 256 : 64;   // rows per workgroup step
  constexpr int LPL = 1;                 // rows per lane
  constexpr int NG = TILE * (kMsDC / 4) / 256;   // staged float4 per thread and chunk
  __shared__ float tile[ISO ? TILE * kMsStride : 1];
  __shared__ int srow[ISO ? TILE : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int qb = GRP ? 0 : blockIdx.x % a.n_qblocks;
  const int slab = GRP ? 0 : blockIdx.x / a.n_qblocks;
  const int q0 = GRP ? w->q0 + (SHQ ? 0 : wave * TQ) : SHQ ? qb * TQ : (qb * kWavesPerWG + wave) * TQ;
  const int q_end = GRP ? w->q_end : a.nq;   // the end of the queries that share this row list
  // a wave past the call's queries still helps to stage the tile
  const int nvq = __builtin_amdgcn_readfirstlane(max(0, min(TQ, q_end - q0)));
  const int i_begin = GRP ? w->i_begin : slab * a.rows_per_slab;
  const int i_end = GRP ? w->i_end : min(i_begin + a.rows_per_slab, a.n_live);
  const int* list = GRP ? w->list : a.list;
  const int NV16 = a.DP / 16;
  const int NCH = a.DP / kMsDC;
  const f32x16* __restrict__ xg = reinterpret_cast<const f32x16*>(X) + (size_t)(q0 / kXQ) * NV16 * kXQ;

  float lk[NLR], la[NLR];
  int lr[NLR];
#pragma unroll
  for (int r = 0; r < NLR; ++r) {
    lk[r] = -CWQ_INF;
    la[r] = 0.f;
    lr[r] = 0x7fffffff;
  }

  for (int it = i_begin; it < i_end; it += TILE) {
    int trow[LPL], row[LPL];   // the lane's rows: position in the tile, segment row
    bool vrow[LPL];
#pragma unroll
    for (int l = 0; l < LPL; ++l) {
      trow[l] = SHQ ? wave * kWave + lane : lane + kWave * l;
      vrow[l] = it + trow[l] < i_end;
      row[l] = list[vrow[l] ? it + trow[l] : i_end - 1];   // < the segment's row count
    }
    float acc[LPL][TQ];
#pragma unroll
    for (int l = 0; l < LPL; ++l)
#pragma unroll
      for (int i = 0; i < TQ; ++i) acc[l][i] = 0.f;
    float4 g[NG];
    size_t goff[NG];
    if constexpr (ISO) {
      __syncthreads();   // the previous tile's srow / tile reads are done
      if (SHQ || wave == 0) {
#pragma unroll
        for (int l = 0; l < LPL; ++l) srow[trow[l]] = row[l];
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < NG; ++u) {
        const int idx = (int)threadIdx.x + 256 * u;   // TILE rows x 8 float4
        goff[u] = (size_t)srow[idx >> 3] * a.DP + (idx & 7) * 4;
        g[u] = *reinterpret_cast<const float4*>(A + goff[u]);
      }
    }
    for (int c = 0; c < NCH; ++c) {
      float m[LPL][kMsDC], sb[LPL][ISO ? 1 : kMsDC];
      if constexpr (ISO) {
        if (c > 0) __syncthreads();   // the previous chunk's tile reads are done
#pragma unroll
        for (int u = 0; u < NG; ++u) {
          const int idx = (int)threadIdx.x + 256 * u;
          float* t = tile + (idx >> 3) * kMsStride + (idx & 7) * 4;
          t[0] = g[u].x;
          t[1] = g[u].y;
          t[2] = g[u].z;
          t[3] = g[u].w;
        }
        __syncthreads();
        if (c + 1 < NCH) {
#pragma unroll
          for (int u = 0; u < NG; ++u) g[u] = *reinterpret_cast<const float4*>(A + goff[u] + (size_t)(c + 1) * kMsDC);
        }
#pragma unroll
        for (int l = 0; l < LPL; ++l)
#pragma unroll
          for (int j = 0; j < kMsDC; ++j) m[l][j] = tile[trow[l] * kMsStride + j];
      } else {
#pragma unroll
        for (int l = 0; l < LPL; ++l)
#pragma unroll
          for (int j = 0; j < kMsDC; ++j) {
            m[l][j] = A[(size_t)(c * kMsDC + j) * a.ld + row[l]];
            sb[l][j] = B[(size_t)(c * kMsDC + j) * a.ld + row[l]];
          }
      }
#pragma unroll
      for (int qi = 0; qi < TQ; ++qi) {
        if (qi >= nvq) continue;
#pragma unroll
        for (int h = 0; h < kMsDC / 16; ++h) {
          const f32x16 xa = xg[(size_t)(c * (kMsDC / 16) + h) * kXQ + qi];
#pragma unroll
          for (int l = 0; l < LPL; ++l) {
            float part;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
              float t;
              if constexpr (ISO)
                t = xa[j] - m[l][h * 16 + j];
              else
                t = fmaf(xa[j], m[l][h * 16 + j], -sb[l][h * 16 + j]);
              part = (j == 0) ? t * t : fmaf(t, t, part);
            }
            acc[l][qi] += part;
          }
        }
      }
    }

    // ---- epilogue: scan_kernel's, for the Fast key ----
#pragma unroll
    for (int l = 0; l < LPL; ++l) {
      const RowMeta md = a.meta[row[l]];
      const int p = a.par[row[l]];
      const int rid = a.seg_base + row[l];
#pragma unroll
      for (int qi = 0; qi < TQ; ++qi) {
        if (qi >= nvq) continue;
        const int q = q0 + qi;
        const float pp = p >= 0 ? a.P[(size_t)q * a.ldP + p] : 0.f;
        float lp, key;
        if constexpr (ISO) {
          key = iso_key_tail(acc[l][qi], md, pp, lp, 0, a.dconst);
        } else {
          lp = -0.5f * (md.logdet + a.dconst + acc[l][qi]);
          key = fmaf(pp, md.invL, md.cw * lp);
        }
        if constexpr (KEYS) {
          if (vrow[l]) a.rowkey[(size_t)q * a.ldr + rid] = key;
          continue;
        }
        if (!vrow[l]) key = -CWQ_INF;
        const int r = qi / QPR;
        const int gq = qi % QPR;
        const int tl = gq * KL + a.K - 1;
        const float tk = rl_f(lk[r], tl);
        const float ta = rl_f(la[r], tl);
        const int tr = rl_i(lr[r], tl);
        const bool cnd = key != -CWQ_INF && list_before<false>(key, lp, rid, tk, ta, tr);
        uint64_t mask = __ballot(cnd);
        while (mask) {
          const int j = __builtin_ctzll(mask);
          mask &= mask - 1;
          list_insert<KL, false>(lk[r], la[r], lr[r], gq, lane, rl_f(key, j), rl_f(lp, j), rl_i(rid, j), a.K);
        }
      }
    }
  }

  if constexpr (KEYS) return;
  const int slot = lane & (KL - 1);
  const int lst = SHQ ? slab * kWavesPerWG + wave : slab;   // shared queries: every wave holds its own list
#pragma unroll
  for (int qi = 0; qi < TQ; ++qi) {
    const int r = qi / QPR;
    const int gq = qi % QPR;
    const int q = q0 + qi;
    const bool ing = (KL == 64) || ((lane >> 4) == gq);
    if (q < q_end && ing && slot < a.K) {
      size_t o;
      if constexpr (GRP)
        o = ((size_t)w->lbase + (size_t)(q - w->gq0) * w->lpq + w->lslot + (SHQ ? wave : 0)) * a.K + slot;
      else
        o = ((size_t)q * a.nslab_total + a.slab_off + lst) * a.K + slot;
      a.pkey[o] = lk[r];
      a.paux[o] = la[r];
      a.prow[o] = lr[r];
    }
  }
}

// a.n_qblocks: blocks of 64 queries, or (shq) of 16; a.rows_per_slab: a multiple of the tile
// (64 rows, shq 256); a slab writes one list per query (shq: 4, see mask_scan_lists)
hipError_t launch_mask_scan(bool iso, int kl, bool shq, const float* X, const float* A, const float* B,
                            const MaskScanArgs& a, int nslab, hipStream_t s) {
  if (a.n_live <= 0 || nslab <= 0) return hipSuccess;
  if (a.K < 1 || a.K > kl || a.DP % kMsDC || a.rows_per_slab % mask_scan_tile(shq) ||
      (int64_t)nslab * a.rows_per_slab < a.n_live ||
      (int64_t)a.n_qblocks * (shq ? kXQ : kXQ * kWavesPerWG) < a.nq ||
      a.slab_off + nslab * mask_scan_lists(shq) > a.nslab_total)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((int64_t)nslab * a.n_qblocks)), block(256);
#define CWQ_MS(ISO_, KL_, SHQ_) hipLaunchKernelGGL((mask_scan_kernel<ISO_, KL_, SHQ_, false>), grid, block, 0, s, X, A, B, a, (const MaskWork*)nullptr)
  if (iso) {
    if (kl == 16) { if (shq) CWQ_MS(true, 16, true); else CWQ_MS(true, 16, false); }
    else { if (shq) CWQ_MS(true, 64, true); else CWQ_MS(true, 64, false); }
  } else {
    if (kl == 16) { if (shq) CWQ_MS(false, 16, true); else CWQ_MS(false, 16, false); }
    else { if (shq) CWQ_MS(false, 64, true); else CWQ_MS(false, 64, false); }
  }
#undef CWQ_MS
  return hipGetLastError();
}

hipError_t launch_mask_scan_keys(bool iso, bool shq, const float* X, const float* A, const float* B,
                                 const MaskScanArgs& a, int nslab, hipStream_t s) {
  if (a.n_live <= 0 || nslab <= 0) return hipSuccess;
  if (a.DP % kMsDC || a.rows_per_slab % mask_scan_tile(shq) || (int64_t)nslab * a.rows_per_slab < a.n_live ||
      (int64_t)a.n_qblocks * (shq ? kXQ : kXQ * kWavesPerWG) < a.nq || !a.rowkey || !a.list)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((int64_t)nslab * a.n_qblocks)), block(256);
#define CWQ_MSK(ISO_, SHQ_) hipLaunchKernelGGL((mask_scan_kernel<ISO_, 16, SHQ_, false, true>), grid, block, 0, s, X, A, B, a, (const MaskWork*)nullptr)
  if (iso) { if (shq) CWQ_MSK(true, true); else CWQ_MSK(true, false); }
  else { if (shq) CWQ_MSK(false, true); else CWQ_MSK(false, false); }
#undef CWQ_MSK
  return hipGetLastError();
}

hipError_t launch_mask_scan_grouped(bool iso, int kl, bool shq, const float* X, const float* A, const float* B,
                                    const MaskScanArgs& a, const MaskWork* work, int n_work, hipStream_t s) {
  if (n_work <= 0) return hipSuccess;
  if (a.K < 1 || a.K > kl || a.DP % kMsDC || !work) return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_work), block(256);
#define CWQ_MSG(ISO_, KL_, SHQ_) \
  hipLaunchKernelGGL((mask_scan_kernel<ISO_, KL_, SHQ_, true>), grid, block, 0, s, X, A, B, a, work)
  if (iso) {
    if (kl == 16) { if (shq) CWQ_MSG(true, 16, true); else CWQ_MSG(true, 16, false); }
    else { if (shq) CWQ_MSG(true, 64, true); else CWQ_MSG(true, 64, false); }
  } else {
    if (kl == 16) { if (shq) CWQ_MSG(false, 16, true); else CWQ_MSG(false, 16, false); }
    else { if (shq) CWQ_MSG(false, 64, true); else CWQ_MSG(false, 64, false); }
  }
#undef CWQ_MSG
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// merge_expand_kernel with the sentence bitset: the merged top-K rows (all live) expand into
// their allowed sentences only; a row's sentences keep their ascending order and its score.
// ---------------------------------------------------------------------------
// one wave: the entries [base, base + nent) of the partial lists into result row q
__device__ __forceinline__ void mask_merge_expand_one(const float* __restrict__ pkey, const float* __restrict__ paux,
                                                      const int* __restrict__ prow, size_t base, int nent, int K,
                                                      int k, const int64_t* __restrict__ sent_ptr,
                                                      const int64_t* __restrict__ sent_ids,
                                                      const uint32_t* __restrict__ bits, int64_t* ids, float* scores,
                                                      int q, int lane) {
  float lk = -CWQ_INF, la = 0.f;
  int lr = 0x7fffffff;
  for (int e0 = 0; e0 < nent; e0 += kWave) {
    const int e = e0 + lane;
    float ek = -CWQ_INF, ea = 0.f;
    int er = 0x7fffffff;
    if (e < nent) {
      ek = pkey[base + e];
      ea = paux[base + e];
      er = prow[base + e];
    }
    const float tk = rl_f(lk, K - 1);
    const int tr = rl_i(lr, K - 1);
    const bool c = ek != -CWQ_INF && (ek > tk || (ek == tk && er < tr));
    uint64_t mask = __ballot(c);
    while (mask) {
      const int j = __builtin_ctzll(mask);
      mask &= mask - 1;
      list_insert<64>(lk, la, lr, 0, lane, rl_f(ek, j), rl_f(ea, j), rl_i(er, j), K);
    }
  }
  const bool valid = lane < K && lk != -CWQ_INF && lr != 0x7fffffff;
  const uint64_t vm = __ballot(valid);
  const int nvalid = (~vm) ? __builtin_ctzll(~vm) : 64;
  int64_t s0 = 0;
  int cnt_all = 0, cnt = 0;
  if (lane < nvalid) {
    s0 = sent_ptr[lr];
    cnt_all = (int)(sent_ptr[lr + 1] - s0);
    for (int j = 0; j < cnt_all; ++j) cnt += bit_set(bits, sent_ids[s0 + j]) ? 1 : 0;
  }
  int off = cnt;   // inclusive scan
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(off, d, 64);
    if (lane >= d) off += o;
  }
  const int total = __shfl(off, 63, 64);
  off -= cnt;
  for (int j = 0; j < cnt_all && off < k; ++j) {
    const int64_t sid = sent_ids[s0 + j];
    if (!bit_set(bits, sid)) continue;
    ids[(size_t)q * k + off] = sid;
    if (scores) scores[(size_t)q * k + off] = lk;
    ++off;
  }
  for (int t = total + lane; t < k; t += kWave) {
    ids[(size_t)q * k + t] = -1;
    if (scores) scores[(size_t)q * k + t] = -CWQ_INF;
  }
}

__global__ __launch_bounds__(256) void mask_merge_expand_kernel(const float* __restrict__ pkey,
                                                                const float* __restrict__ paux,
                                                                const int* __restrict__ prow, int nq, int nent, int K,
                                                                int k, const int64_t* __restrict__ sent_ptr,
                                                                const int64_t* __restrict__ sent_ids,
                                                                const uint32_t* __restrict__ bits, int64_t* ids,
                                                                float* scores) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
  if (q >= nq) return;
  mask_merge_expand_one(pkey, paux, prow, (size_t)q * nent, nent, K, k, sent_ptr, sent_ids, bits, ids, scores, q, lane);
}

// the grouped form: the lists, the bitset and the result row per staged query
__global__ __launch_bounds__(256) void mask_merge_expand_multi_kernel(const float* __restrict__ pkey,
                                                                      const float* __restrict__ paux,
                                                                      const int* __restrict__ prow,
                                                                      const MaskMergeQ* __restrict__ mq, int n, int K,
                                                                      int k, const int64_t* __restrict__ sent_ptr,
                                                                      const int64_t* __restrict__ sent_ids,
                                                                      int64_t* ids, float* scores) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
  if (i >= n) return;
  const MaskMergeQ m = mq[i];
  mask_merge_expand_one(pkey, paux, prow, (size_t)m.lfirst * K, m.nlists * K, K, k, sent_ptr, sent_ids, m.bits, ids,
                        scores, m.orig, lane);
}

hipError_t launch_mask_merge_expand(const float* pkey, const float* paux, const int* prow, int nq, int nent, int K,
                                    int k, const int64_t* sent_ptr, const int64_t* sent_ids, const uint32_t* bits,
                                    int64_t* ids, float* scores, hipStream_t s) {
  if (K > kWave || K < 1) return hipErrorInvalidValue;
  dim3 grid((unsigned)((nq + kWavesPerWG - 1) / kWavesPerWG)), block(256);
  hipLaunchKernelGGL(mask_merge_expand_kernel, grid, block, 0, s, pkey, paux, prow, nq, nent, K, k, sent_ptr, sent_ids,
                     bits, ids, scores);
  return hipGetLastError();
}

hipError_t launch_mask_merge_expand_multi(const float* pkey, const float* paux, const int* prow, const MaskMergeQ* mq,
                                          int n, int K, int k, const int64_t* sent_ptr, const int64_t* sent_ids,
                                          int64_t* ids, float* scores, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (K > kWave || K < 1 || !mq) return hipErrorInvalidValue;
  dim3 grid((unsigned)((n + kWavesPerWG - 1) / kWavesPerWG)), block(256);
  hipLaunchKernelGGL(mask_merge_expand_multi_kernel, grid, block, 0, s, pkey, paux, prow, mq, n, K, k, sent_ptr,
                     sent_ids, ids, scores);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Over-fetch compaction: the allowed entries of an unmasked top-kp result (kp <= 64), in order,
// cut to k and padded.  flag[q] = the query came up short: fewer than min(k, n_allowed)
// survived, so allowed sentences rank below the unmasked top-kp (the gathered scan redoes it).
// ---------------------------------------------------------------------------
// one wave: row q of the unmasked top-kp result into result row and flag o
__device__ __forceinline__ void mask_overfetch_one(const int64_t* __restrict__ tid, const float* __restrict__ ts, int q,
                                                   int kp, int k, const uint32_t* __restrict__ bits, int64_t n_allowed,
                                                   int64_t* ids, float* scores, int* flag, int o, int lane) {
  int64_t sid = -1;
  float sc = -CWQ_INF;
  if (lane < kp) {
    sid = tid[(size_t)q * kp + lane];
    sc = ts[(size_t)q * kp + lane];
  }
  const bool ok = sid >= 0 && bit_set(bits, sid);
  const uint64_t m = __ballot(ok);
  const int pos = __popcll(m & ((1ull << lane) - 1ull));
  const int n = __popcll(m);
  if (ok && pos < k) {
    ids[(size_t)o * k + pos] = sid;
    if (scores) scores[(size_t)o * k + pos] = sc;
  }
  for (int t = n + lane; t < k; t += kWave) {
    ids[(size_t)o * k + t] = -1;
    if (scores) scores[(size_t)o * k + t] = -CWQ_INF;
  }
  if (lane == 0) flag[o] = (int64_t)n < (n_allowed < (int64_t)k ? n_allowed : (int64_t)k) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mask_overfetch_kernel(const int64_t* __restrict__ tid,
                                                             const float* __restrict__ ts, int nq, int kp, int k,
                                                             const uint32_t* __restrict__ bits, int64_t n_allowed,
                                                             int64_t* ids, float* scores, int* flag) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
  if (q >= nq) return;
  mask_overfetch_one(tid, ts, q, kp, k, bits, n_allowed, ids, scores, flag, q, lane);
}

// the same for gathered queries of several masks: the bitset and n_allowed of query i from
// slots[qslot[i]], its result row and short flag at its position in the call, qorig[i]
__global__ __launch_bounds__(256) void mask_overfetch_multi_kernel(const int64_t* __restrict__ tid,
                                                                   const float* __restrict__ ts, int n, int kp, int k,
                                                                   const MaskSlot* __restrict__ slots,
                                                                   const int* __restrict__ qslot,
                                                                   const int* __restrict__ qorig, int64_t* ids,
                                                                   float* scores, int* flag) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
  if (i >= n) return;
  const MaskSlot m = slots[qslot[i]];
  mask_overfetch_one(tid, ts, i, kp, k, m.bits, m.n_allowed, ids, scores, flag, qorig[i], lane);
}

hipError_t launch_mask_overfetch(const int64_t* tid, const float* ts, int nq, int kp, int k, const uint32_t* bits,
                                 int64_t n_allowed, int64_t* ids, float* scores, int* flag, hipStream_t s) {
  if (kp > kWave || kp < 1) return hipErrorInvalidValue;
  dim3 grid((unsigned)((nq + kWavesPerWG - 1) / kWavesPerWG)), block(256);
  hipLaunchKernelGGL(mask_overfetch_kernel, grid, block, 0, s, tid, ts, nq, kp, k, bits, n_allowed, ids, scores, flag);
  return hipGetLastError();
}

hipError_t launch_mask_overfetch_multi(const int64_t* tid, const float* ts, int n, int kp, int k, const MaskSlot* slots,
                                       const int* qslot, const int* qorig, int64_t* ids, float* scores, int* flag,
                                       hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (kp > kWave || kp < 1) return hipErrorInvalidValue;
  dim3 grid((unsigned)((n + kWavesPerWG - 1) / kWavesPerWG)), block(256);
  hipLaunchKernelGGL(mask_overfetch_multi_kernel, grid, block, 0, s, tid, ts, n, kp, k, slots, qslot, qorig, ids,
                     scores, flag);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k > 64: the materialised keys of the rows that are not live -> -inf (before the sort), and
// the masked expansion of the sorted rows (expand_kernel with the bitset).
// ---------------------------------------------------------------------------
__global__ void mask_kill_kernel(float* rowkey, int64_t ld, int NL, const uint8_t* __restrict__ live) {
  const int q = blockIdx.y;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < NL; r += gridDim.x * blockDim.x)
    if (!live[r]) rowkey[(size_t)q * ld + r] = -CWQ_INF;
}

hipError_t launch_mask_kill(float* rowkey, int64_t ld, int nq, int NL, const uint8_t* live, hipStream_t s) {
  if (NL <= 0 || nq <= 0) return hipSuccess;
  dim3 grid((unsigned)std::min((NL + 255) / 256, 4096), (unsigned)nq);
  hipLaunchKernelGGL(mask_kill_kernel, grid, dim3(256), 0, s, rowkey, ld, NL, live);
  return hipGetLastError();
}

__global__ void mask_expand_kernel(const float* __restrict__ okey, const int* __restrict__ orow, int nq, int K, int k,
                                   const int64_t* __restrict__ sent_ptr, const int64_t* __restrict__ sent_ids,
                                   const uint32_t* __restrict__ bits, int64_t* ids, float* scores) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int cnt = 0;
  for (int i = 0; i < K && cnt < k; ++i) {
    const float key = okey[(size_t)q * K + i];
    const int row = orow[(size_t)q * K + i];
    if (key == -CWQ_INF || row == 0x7fffffff) break;
    for (int64_t s = sent_ptr[row]; s < sent_ptr[row + 1] && cnt < k; ++s) {
      const int64_t sid = sent_ids[s];
      if (!bit_set(bits, sid)) continue;
      ids[(size_t)q * k + cnt] = sid;
      if (scores) scores[(size_t)q * k + cnt] = key;
      ++cnt;
    }
  }
  for (; cnt < k; ++cnt) {
    ids[(size_t)q * k + cnt] = -1;
    if (scores) scores[(size_t)q * k + cnt] = -CWQ_INF;
  }
}

hipError_t launch_mask_expand(const float* okey, const int* orow, int nq, int K, int k, const int64_t* sent_ptr,
                              const int64_t* sent_ids, const uint32_t* bits, int64_t* ids, float* scores,
                              hipStream_t s) {
  hipLaunchKernelGGL(mask_expand_kernel, dim3((nq + 127) / 128), dim3(128), 0, s, okey, orow, nq, K, k, sent_ptr,
                     sent_ids, bits, ids, scores);
  return hipGetLastError();
}

// every id -1, every score -inf (a mask without live rows)
__global__ void mask_fill_kernel(int64_t* ids, float* scores, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    ids[i] = -1;
    if (scores) scores[i] = -CWQ_INF;
  }
}

hipError_t launch_mask_fill(int64_t* ids, float* scores, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(mask_fill_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, ids,
                     scores, n);
  return hipGetLastError();
}

// the rows idx[0, n) only (the queries of masks without a live row, among others' queries)
__global__ void mask_fill_rows_kernel(int64_t* ids, float* scores, int k, const int* __restrict__ idx, int n) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < (int64_t)n * k;
       t += (int64_t)gridDim.x * blockDim.x) {
    const size_t o = (size_t)idx[t / k] * k + t % k;
    ids[o] = -1;
    if (scores) scores[o] = -CWQ_INF;
  }
}

hipError_t launch_mask_fill_rows(int64_t* ids, float* scores, int k, const int* idx, int n, hipStream_t s) {
  if (n <= 0 || k <= 0) return hipSuccess;
  const int64_t tot = (int64_t)n * k;
  hipLaunchKernelGGL(mask_fill_rows_kernel, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 4096)), dim3(256), 0, s,
                     ids, scores, k, idx, n);
  return hipGetLastError();
}

}  // namespace cwq
