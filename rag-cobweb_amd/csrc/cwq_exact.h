// Device helpers shared by the exact scan (cwq_kernels.hip) and the masked scan (cwq_mask.hip):
// readlane wrappers, the per-wave sorted top-K list held in VGPRs, and its order.  Moved here
// verbatim from cwq_kernels.hip so that both files insert into and merge the lists with one
// piece of code.  Device only.
#pragma once
#include <hip/hip_runtime.h>

namespace cwq {

#define CWQ_INF __builtin_inff()

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float rl_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ int rl_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// Shift a per-lane list entry one slot up (slot i receives slot i-1) inside a
// group of KL lanes.  KL = 16: DPP row_shr:1 (rows of 16 lanes); KL = 64: DPP
// wave_shr:1 (GFX9 whole-wave shift; lane 0 keeps its value, never used as a shifted
// entry) -- a VALU op instead of a ds_bpermute round trip through the LDS unit.
template <int KL>
__device__ __forceinline__ int shift_up(int v);
template <>
__device__ __forceinline__ int shift_up<16>(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x111, 0xF, 0xF, false);
}
template <>
__device__ __forceinline__ int shift_up<64>(int v) {
  return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false);
}

// List order of an entry (key k, aux a, row r) before (k2, a2, r2): key descending, then
// row ascending; categorize lists (CAT) put the smaller aux (= the row's own lp) first
// among equal keys, so that a list cut inside a tie at its last key G holds every row
// whose own lp IS G (the rows that attain their path bottleneck; §4.7 two-level replay).
template <bool CAT>
__device__ __forceinline__ bool list_before(float k, float a, int r, float k2, float a2, int r2) {
  if (k != k2) return k > k2;
  if (CAT && a != a2) return a < a2;
  return r < r2;
}

// Insert candidate (ck, ca, cr) into the sorted list held by lane group g (list_before
// order).  The first K slots are the top-K.
template <int KL, bool CAT = false>
__device__ __forceinline__ void list_insert(float& lk, float& la, int& lr, int g, int lane, float ck, float ca,
                                            int cr, int K) {
  const bool ing = (KL == 64) || ((lane >> 4) == g);
  const int slot = lane & (KL - 1);
  const bool prec = ing && list_before<CAT>(lk, la, lr, ck, ca, cr);
  const int pos = __popcll(__ballot(prec));
  if (pos < K) {
    const float sk = __int_as_float(shift_up<KL>(__float_as_int(lk)));
    const float sa = __int_as_float(shift_up<KL>(__float_as_int(la)));
    const int sr = shift_up<KL>(lr);
    if (ing) {
      if (slot == pos) {
        lk = ck;
        la = ca;
        lr = cr;
      } else if (slot > pos) {
        lk = sk;
        la = sa;
        lr = sr;
      }
    }
  }
}

}  // namespace cwq
