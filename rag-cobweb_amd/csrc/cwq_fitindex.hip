// libcwq: the query index straight from a device-resident fit handle (cwq_fitdev.hip), and
// the handle's in-place growth -- no [Nn, D] array crosses PCIe between an insert and the
// next query.
//
// cwq_fit_flatten numbers the live slot tree breadth first, exactly as CobwebTree.flatten
// (tree.py) numbers the host tree: the root is node 0, a node's children are consecutive in
// child-list order, levels in order.  Per level the frontier (slots in BFS order) is
// expanded by
//   counts   cnt[i] = ccnt[frontier[i]]
//   scan     off = exclusive scan of cnt (three launches: tile sums, the scan of the tile
//            sums by one workgroup, the tiles' own scans), total = the next frontier's size
//   expand   one thread per CHILD POSITION p in [0, total): the frontier node i with
//            off[i] <= p < off[i] + cnt[i] by binary search, child j = p - off[i] ->
//            next[p] = arena[coff[slot] + j] (a flat tree's 1M children of one node expand
//            over 1M threads)
// and the host reads `total` back (8 bytes per level; at most kFlatMaxDepth levels).  Slots
// a split removed (parent == -2) hang under no child list: they are never reached.  Then the
// statistics move in BFS order: mean rows gathered whole (one wave per node, float4 when
// dim % 4 == 0), the variances meanSq / count + prior_var computed from the gathered node's
// meanSq row with the division and op order of fd_lvar_kernel (contraction off: numpy's
// float32 bits), kept as one scalar per node plus a flag "the D values are not all the same
// bits" (CompactVar.from_full's rule); a scan over the flags compacts the flagged nodes to
// an_nodes (ascending) and only those get a [D] variance row.  Every kernel here is a plain
// data-parallel launch: no workgroup waits for another inside a launch.
//
// cwq_fit_grow re-allocates the pool and the child arena at a larger capacity, device to
// device, every slot number unchanged; the child lists are re-packed at max(4, 2 ccnt) each
// (cwq_fit_load's layout; the slabs that list doublings abandoned are not copied) with the
// same scan.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cobweb_query.h"
#include "cwq_internal.h"

namespace cwq {

constexpr int kFlatMaxDepth = 64;   // levels below the root; deeper trees are refused (CWQ_ERR_ARG)
constexpr int kScanThreads = 256;
constexpr int kScanPer = 4;
constexpr int kScanTile = kScanThreads * kScanPer;   // 1024 elements per workgroup
constexpr int kBsumThreads = 1024;

// exclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS, two
// buffers of blockDim values); total = the workgroup's sum
template <int T>
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t* buf, int64_t& total) {
  const int t = threadIdx.x;
  int cur = 0;
  buf[t] = v;
  __syncthreads();
#pragma unroll
  for (int step = 1; step < T; step <<= 1) {
    const int64_t a = buf[cur * T + t] + (t >= step ? buf[cur * T + t - step] : 0);
    buf[(cur ^ 1) * T + t] = a;
    cur ^= 1;
    __syncthreads();
  }
  const int64_t incl = buf[cur * T + t];
  total = buf[cur * T + T - 1];
  __syncthreads();
  return incl - v;
}

// tile sums: bsum[b] = sum of in[b * kScanTile ..)
__global__ __launch_bounds__(kScanThreads) void fi_scan_reduce_kernel(const int* __restrict__ in, int64_t n,
                                                                     int64_t* __restrict__ bsum) {
  __shared__ int64_t buf[2 * kScanThreads];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int64_t v = 0;
#pragma unroll
  for (int u = 0; u < kScanPer; ++u)
    if (base + u < n) v += in[base + u];
  int64_t total;
  (void)block_excl_scan<kScanThreads>(v, buf, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum[0..nb) -> its exclusive scan in place, total[0] = the sum
__global__ __launch_bounds__(kBsumThreads) void fi_scan_bsum_kernel(int64_t* __restrict__ bsum, int64_t nb,
                                                                    int64_t* __restrict__ total) {
  __shared__ int64_t buf[2 * kBsumThreads];
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < nb; c0 += kBsumThreads) {
    const int64_t i = c0 + threadIdx.x;
    const int64_t v = i < nb ? bsum[i] : 0;
    int64_t tot;
    const int64_t ex = block_excl_scan<kBsumThreads>(v, buf, tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) total[0] = carry;
}

// out[i] = bsum[tile] + exclusive scan of in within the tile
__global__ __launch_bounds__(kScanThreads) void fi_scan_apply_kernel(const int* __restrict__ in, int64_t n,
                                                                    const int64_t* __restrict__ bsum,
                                                                    int64_t* __restrict__ out) {
  __shared__ int64_t buf[2 * kScanThreads];
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
  int x[kScanPer];
  int64_t v = 0;
#pragma unroll
  for (int u = 0; u < kScanPer; ++u) {
    x[u] = base + u < n ? in[base + u] : 0;
    v += x[u];
  }
  int64_t total;
  int64_t ex = block_excl_scan<kScanThreads>(v, buf, total) + bsum[blockIdx.x];
#pragma unroll
  for (int u = 0; u < kScanPer; ++u) {
    if (base + u < n) out[base + u] = ex;
    ex += x[u];
  }
}

// exclusive scan of in[0..n) (int32, device) -> out (int64, device), total -> d_total[0];
// bsum: ceil(n / kScanTile) words of scratch.  Three launches.
static hipError_t launch_scan(const int* in, int64_t n, int64_t* out, int64_t* bsum, int64_t* d_total,
                              hipStream_t s) {
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(fi_scan_reduce_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n, bsum);
  hipLaunchKernelGGL(fi_scan_bsum_kernel, dim3(1), dim3(kBsumThreads), 0, s, bsum, nb, d_total);
  hipLaunchKernelGGL(fi_scan_apply_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, in, n, bsum, out);
  return hipGetLastError();
}

static inline unsigned grid_for(int64_t n, int threads) {
  return (unsigned)std::min<int64_t>((n + threads - 1) / threads, 1 << 20);
}

// ---- BFS numbering ----
__global__ void fi_root_kernel(const int* __restrict__ ctrl, int used, int* slot_of_node, int* node_of_slot,
                               int64_t* parent, int* err) {
  const int root = ctrl[2];
  parent[0] = -1;
  if ((unsigned)root >= (unsigned)used) {   // the host stops on err; slot 0 keeps the next read in bounds
    err[0] = 1;
    slot_of_node[0] = 0;
    return;
  }
  slot_of_node[0] = root;
  node_of_slot[root] = 0;
}

// cnt[i] = ccnt[frontier[i]], the frontier = slot_of_node[lo .. lo + m)
__global__ void fi_counts_kernel(const int* __restrict__ ccnt, const int* __restrict__ slot_of_node, int64_t lo,
                                 int64_t m, int* __restrict__ cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
    cnt[i] = ccnt[slot_of_node[lo + i]];
}

// one thread per child position of the level [lo, lo + m): the next level at [hi, hi + total)
__global__ void fi_expand_kernel(const int* __restrict__ arena, const int64_t* __restrict__ coff,
                                 const int64_t* __restrict__ off, int64_t lo, int64_t m, int64_t hi, int64_t total,
                                 int used, int64_t arena_cap, int* __restrict__ slot_of_node,
                                 int* __restrict__ node_of_slot, int64_t* __restrict__ parent, int* err) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = 0, b = m;   // the last i with off[i] <= p (nodes without children share their successor's offset)
    while (b - a > 1) {
      const int64_t mid = (a + b) >> 1;
      if (off[mid] <= p) a = mid;
      else b = mid;
    }
    const int slot = slot_of_node[lo + a];
    const int64_t src = coff[slot] + (p - off[a]);
    // a damaged tree must not become a wild access: the host stops on err, and slot 0
    // keeps the next level's reads in bounds
    const int c = src >= 0 && src < arena_cap ? arena[src] : -1;
    if ((unsigned)c >= (unsigned)used) {
      err[0] = 1;
      slot_of_node[hi + p] = 0;
      parent[hi + p] = lo + a;
      continue;
    }
    slot_of_node[hi + p] = c;
    node_of_slot[c] = (int)(hi + p);
    parent[hi + p] = lo + a;
  }
}

__global__ void fi_sentence_kernel(const int* __restrict__ slot_of_sentence, int64_t n_sent, int used,
                                   const int* __restrict__ node_of_slot, int64_t* __restrict__ nos) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_sent; i += (int64_t)gridDim.x * blockDim.x) {
    const int sl = slot_of_sentence[i];
    nos[i] = (unsigned)sl < (unsigned)used ? (int64_t)node_of_slot[sl] : -1;
  }
}

// ---- statistics in BFS order ----
// compute_var (CobwebTorchTree.py:336-342, acuity_cutoff off) of one element: fd_lvar_kernel's
// division and op order; an empty node (count 0) has var = prior_var
__device__ __forceinline__ float fi_var(float m2, float c, float pv) {
#pragma clang fp contract(off)
  return c > 0.f ? m2 / c + pv : pv;
}

// One wave per node i: mean row slot_of_node[i] -> mean_out[i], its count; var_row[i] = the variance of
// dimension 0; flag[i] = 1 when some dimension's variance has other bits.  VEC: float4 rows.
template <bool VEC>
__global__ __launch_bounds__(256) void fi_gather_kernel(const FitDev f, const int* __restrict__ slot_of_node,
                                                        int64_t n_nodes, float* __restrict__ mean_out,
                                                        float* __restrict__ count_out, float* __restrict__ var_row,
                                                        int* __restrict__ flag) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int D = f.D;
  const float pv = f.pv;
  for (int64_t i = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); i < n_nodes;
       i += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    const int slot = slot_of_node[i];
    const float c = f.count[slot];
    const float* __restrict__ ms = f.mean + (size_t)slot * D;
    const float* __restrict__ qs = f.meanSq + (size_t)slot * D;
    float* __restrict__ md = mean_out + (size_t)i * D;
    const float v0 = fi_var(qs[0], c, pv);
    const unsigned b0 = __float_as_uint(v0);
    bool differ = false;
    if (VEC) {
      const float4* ms4 = reinterpret_cast<const float4*>(ms);
      const float4* qs4 = reinterpret_cast<const float4*>(qs);
      float4* md4 = reinterpret_cast<float4*>(md);
      for (int d = lane; d < (D >> 2); d += 64) {
        md4[d] = ms4[d];
        const float4 q = qs4[d];
        differ |= __float_as_uint(fi_var(q.x, c, pv)) != b0 || __float_as_uint(fi_var(q.y, c, pv)) != b0 ||
                  __float_as_uint(fi_var(q.z, c, pv)) != b0 || __float_as_uint(fi_var(q.w, c, pv)) != b0;
      }
    } else {
      for (int d = lane; d < D; d += 64) {
        md[d] = ms[d];
        differ |= __float_as_uint(fi_var(qs[d], c, pv)) != b0;
      }
    }
    const bool any = __any(differ);
    if (lane == 0) {
      count_out[i] = c;
      var_row[i] = v0;
      flag[i] = any ? 1 : 0;
    }
  }
}

// flagged nodes -> an_nodes (ascending: pos = the exclusive scan of the flags), an_map
__global__ void fi_compact_kernel(const int* __restrict__ flag, const int64_t* __restrict__ pos, int64_t n_nodes,
                                  int64_t* __restrict__ an_nodes, int* __restrict__ an_map) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_nodes; i += (int64_t)gridDim.x * blockDim.x) {
    if (flag[i]) {
      an_nodes[pos[i]] = i;
      an_map[i] = (int)pos[i];
    } else {
      an_map[i] = -1;
    }
  }
}

// one wave per flagged node: its [D] variance row
template <bool VEC>
__global__ __launch_bounds__(256) void fi_anvar_kernel(const FitDev f, const int* __restrict__ slot_of_node,
                                                       const int64_t* __restrict__ an_nodes, int64_t n_an,
                                                       float* __restrict__ an_var) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int D = f.D;
  const float pv = f.pv;
  for (int64_t j = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); j < n_an;
       j += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    const int slot = slot_of_node[an_nodes[j]];
    const float c = f.count[slot];
    const float* __restrict__ qs = f.meanSq + (size_t)slot * D;
    float* __restrict__ vd = an_var + (size_t)j * D;
    if (VEC) {
      const float4* qs4 = reinterpret_cast<const float4*>(qs);
      float4* vd4 = reinterpret_cast<float4*>(vd);
      for (int d = lane; d < (D >> 2); d += 64) {
        const float4 q = qs4[d];
        vd4[d] = make_float4(fi_var(q.x, c, pv), fi_var(q.y, c, pv), fi_var(q.z, c, pv), fi_var(q.w, c, pv));
      }
    } else {
      for (int d = lane; d < D; d += 64) vd[d] = fi_var(qs[d], c, pv);
    }
  }
}

// ---- grow ----
// the re-packed capacity of every slot's child list: max(4, 2 ccnt); a removed slot keeps none
__global__ void fi_newcap_kernel(const int* __restrict__ parent, const int* __restrict__ ccnt, int used,
                                 int* __restrict__ ncap) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < used; i += gridDim.x * blockDim.x)
    ncap[i] = parent[i] == -2 ? 0 : (ccnt[i] < 4 ? 4 : 2 * ccnt[i]);
}

// one wave per slot: its child list into the new arena at noff[slot]
__global__ __launch_bounds__(256) void fi_repack_kernel(const int* __restrict__ parent, const int* __restrict__ ccnt,
                                                        const int64_t* __restrict__ coff, const int* __restrict__ arena,
                                                        int64_t arena_cap, int used, const int* __restrict__ ncap,
                                                        const int64_t* __restrict__ noff, int64_t new_arena_cap,
                                                        int* __restrict__ new_ccap, int64_t* __restrict__ new_coff,
                                                        int* __restrict__ new_arena) {
  const int lane = threadIdx.x & 63;
  for (int64_t s = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6); s < used;
       s += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    const int n = parent[s] == -2 ? 0 : ccnt[s];
    const int64_t src = coff[s], dst = noff[s];
    if (lane == 0) {
      new_ccap[s] = ncap[s];
      new_coff[s] = ncap[s] ? dst : 0;
    }
    if (n <= 0 || src < 0 || src + n > arena_cap || dst + n > new_arena_cap) continue;
    for (int j = lane; j < n; j += 64) new_arena[dst + j] = arena[src + j];
  }
}

__global__ void fi_count_removed_kernel(const int* __restrict__ parent, int used, int* __restrict__ out) {
  int c = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < used; i += gridDim.x * blockDim.x) c += parent[i] == -2;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

}  // namespace cwq

using namespace cwq;

// The flattened tree of one cwq_fit_flatten call (device arrays, owned by the object).
struct cwq_fit_flat {
  int device = 0;
  int D = 0;
  int64_t n_nodes = 0, n_an = 0, n_sent = 0, used = 0;
  int depth = 0;
  int64_t bytes = 0;
  float* mean = nullptr;        // [n_nodes][D]
  float* count = nullptr;       // [n_nodes]
  float* var_row = nullptr;     // [n_nodes]
  int64_t* an_nodes = nullptr;  // [n_an]
  float* an_var = nullptr;      // [n_an][D]
  int* an_map = nullptr;        // [n_nodes]
  int64_t* parent = nullptr;    // [used] (n_nodes valid)
  int64_t* nos = nullptr;       // [n_sent]
  int* slot_of_node = nullptr;  // [used] (n_nodes valid)
  std::vector<void*> allocs;
  ~cwq_fit_flat() {
    for (void* p : allocs) (void)hipFree(p);
  }
  template <typename T>
  bool al(T** p, size_t n) {
    const size_t b = n * sizeof(T);
    if (hipMalloc((void**)p, b < 256 ? 256 : b) != hipSuccess) return false;
    allocs.push_back((void*)*p);
    bytes += (int64_t)(b < 256 ? 256 : b);
    return true;
  }
  void release(void* p) {
    if (!p) return;
    (void)hipFree(p);
    allocs.erase(std::remove(allocs.begin(), allocs.end(), p), allocs.end());
  }
};

namespace {

struct DevRestore {
  int prev = -1;
  explicit DevRestore(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(dev);
  }
  ~DevRestore() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int both_fail(int code, const char* msg) {
  (void)index_fail(code, msg);
  return fit_fail(code, msg);
}

#define FICHK(expr, what)                                                         \
  do {                                                                            \
    if ((expr) != hipSuccess) return fit_fail(CWQ_ERR_HIP, what " failed");       \
  } while (0)

int read_ctrl(const cwq_fit* h, hipStream_t s, int* ctrl, int64_t* c64) {
  FICHK(hipMemcpyAsync(ctrl, h->f.ctrl, 64, hipMemcpyDeviceToHost, s), "control read");
  FICHK(hipMemcpyAsync(c64, h->f.ctrl64, 64, hipMemcpyDeviceToHost, s), "control read");
  FICHK(hipStreamSynchronize(s), "control read");
  return CWQ_OK;
}

int flatten_impl(cwq_fit* h, const int32_t* slot_of_sentence, int64_t n_sent, hipStream_t s, cwq_fit_flat* fl) {
  const FitDev& f = h->f;
  int ctrl[16];
  int64_t c64[8];
  int rc = read_ctrl(h, s, ctrl, c64);
  if (rc) return rc;
  const int used = ctrl[0];
  if (used <= 0 || used > f.cap) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flatten: the handle holds no tree");
  fl->device = h->device;
  fl->D = f.D;
  fl->used = used;
  fl->n_sent = n_sent;
  const size_t U = (size_t)used;
  int *node_of_slot = nullptr, *tmp = nullptr, *err = nullptr;
  int64_t *off = nullptr, *bsum = nullptr, *d_total = nullptr;
  const size_t nb = (U + kScanTile - 1) / kScanTile + 1;
  if (!fl->al(&fl->slot_of_node, U) || !fl->al(&fl->parent, U) || !fl->al(&node_of_slot, U) || !fl->al(&tmp, U) ||
      !fl->al(&off, U) || !fl->al(&bsum, nb) || !fl->al(&d_total, 1) || !fl->al(&err, 1) ||
      !fl->al(&fl->nos, (size_t)std::max<int64_t>(n_sent, 1)))
    return fit_fail(CWQ_ERR_OOM, "cwq_fit_flatten: device allocation failed");
  FICHK(hipMemsetAsync(node_of_slot, 0xff, U * sizeof(int), s), "cwq_fit_flatten reset");
  FICHK(hipMemsetAsync(err, 0, sizeof(int), s), "cwq_fit_flatten reset");
  hipLaunchKernelGGL(fi_root_kernel, dim3(1), dim3(1), 0, s, f.ctrl, used, fl->slot_of_node, node_of_slot, fl->parent,
                     err);
  FICHK(hipGetLastError(), "cwq_fit_flatten root launch");
  // ---- level by level ----
  int64_t lo = 0, m = 1;
  int depth = 0;
  while (true) {
    hipLaunchKernelGGL(fi_counts_kernel, dim3(grid_for(m, 256)), dim3(256), 0, s, f.ccnt, fl->slot_of_node, lo, m, tmp);
    FICHK(hipGetLastError(), "cwq_fit_flatten counts launch");
    FICHK(launch_scan(tmp, m, off, bsum, d_total, s), "cwq_fit_flatten scan launch");
    int64_t total = 0;
    int herr = 0;
    FICHK(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s), "cwq_fit_flatten level read");
    FICHK(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s), "cwq_fit_flatten level read");
    FICHK(hipStreamSynchronize(s), "cwq_fit_flatten level sync");
    if (herr || total < 0 || lo + m + total > used)
      return fit_fail(CWQ_ERR_HIP, "cwq_fit_flatten: the device tree is inconsistent (child lists outside the pool)");
    if (total == 0) break;
    if (++depth > kFlatMaxDepth) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flatten: the tree is deeper than 64 levels");
    const int64_t hi = lo + m;
    hipLaunchKernelGGL(fi_expand_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, f.arena, f.coff, off, lo, m, hi,
                       total, used, f.arena_cap, fl->slot_of_node, node_of_slot, fl->parent, err);
    FICHK(hipGetLastError(), "cwq_fit_flatten expand launch");
    lo = hi;
    m = total;
  }
  const int64_t Nn = lo + m;
  fl->n_nodes = Nn;
  fl->depth = depth;
  if (n_sent > 0) {
    hipLaunchKernelGGL(fi_sentence_kernel, dim3(grid_for(n_sent, 256)), dim3(256), 0, s, slot_of_sentence, n_sent, used,
                       node_of_slot, fl->nos);
    FICHK(hipGetLastError(), "cwq_fit_flatten sentence launch");
  }
  // ---- statistics ----
  const size_t D = (size_t)f.D;
  int* flag = tmp;   // the level counts are done with
  if (!fl->al(&fl->mean, (size_t)Nn * D) || !fl->al(&fl->var_row, (size_t)Nn) || !fl->al(&fl->count, (size_t)Nn) || !fl->al(&fl->an_map, (size_t)Nn))
    return fit_fail(CWQ_ERR_OOM, "cwq_fit_flatten: device allocation failed");
  const bool vec = f.D % 4 == 0;
  const unsigned gw = grid_for(Nn, 4);
  if (vec)
    hipLaunchKernelGGL(fi_gather_kernel<true>, dim3(gw), dim3(256), 0, s, f, fl->slot_of_node, Nn, fl->mean,
                       fl->count, fl->var_row, flag);
  else
    hipLaunchKernelGGL(fi_gather_kernel<false>, dim3(gw), dim3(256), 0, s, f, fl->slot_of_node, Nn, fl->mean,
                       fl->count, fl->var_row, flag);
  FICHK(hipGetLastError(), "cwq_fit_flatten gather launch");
  FICHK(launch_scan(flag, Nn, off, bsum, d_total, s), "cwq_fit_flatten flag scan launch");
  int64_t n_an = 0;
  int herr = 0;
  FICHK(hipMemcpyAsync(&n_an, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s), "cwq_fit_flatten read");
  FICHK(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, s), "cwq_fit_flatten read");
  FICHK(hipStreamSynchronize(s), "cwq_fit_flatten sync");
  if (herr || n_an < 0 || n_an > Nn)
    return fit_fail(CWQ_ERR_HIP, "cwq_fit_flatten: the device tree is inconsistent (child lists outside the pool)");
  fl->n_an = n_an;
  if (!fl->al(&fl->an_nodes, (size_t)std::max<int64_t>(n_an, 1)) ||
      !fl->al(&fl->an_var, (size_t)std::max<int64_t>(n_an, 1) * D))
    return fit_fail(CWQ_ERR_OOM, "cwq_fit_flatten: device allocation failed");
  hipLaunchKernelGGL(fi_compact_kernel, dim3(grid_for(Nn, 256)), dim3(256), 0, s, flag, off, Nn, fl->an_nodes,
                     fl->an_map);
  FICHK(hipGetLastError(), "cwq_fit_flatten compact launch");
  if (n_an > 0) {
    const unsigned ga = grid_for(n_an, 4);
    if (vec)
      hipLaunchKernelGGL(fi_anvar_kernel<true>, dim3(ga), dim3(256), 0, s, f, fl->slot_of_node, fl->an_nodes, n_an,
                         fl->an_var);
    else
      hipLaunchKernelGGL(fi_anvar_kernel<false>, dim3(ga), dim3(256), 0, s, f, fl->slot_of_node, fl->an_nodes, n_an,
                         fl->an_var);
    FICHK(hipGetLastError(), "cwq_fit_flatten variance launch");
  }
  FICHK(hipStreamSynchronize(s), "cwq_fit_flatten sync");
  // the scratch leaves before the index is built next to this
  fl->release(node_of_slot);
  fl->release(tmp);
  fl->release(off);
  fl->release(bsum);
  fl->release(d_total);
  fl->release(err);
  return CWQ_OK;
}

}  // namespace

extern "C" int cwq_fit_flatten(cwq_fit* h, const int32_t* slot_of_sentence, int64_t n_sent, void* stream,
                               cwq_fit_flat** out) {
  if (!out) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flatten: out is NULL");
  *out = nullptr;
  if (!h) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flatten: NULL handle");
  if (n_sent < 0 || (n_sent > 0 && !slot_of_sentence)) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flatten: bad sentence map");
  DevRestore dg(h->device);
  std::unique_ptr<cwq_fit_flat> fl(new cwq_fit_flat());
  const int rc = flatten_impl(h, slot_of_sentence, n_sent, (hipStream_t)stream, fl.get());
  if (rc) {
    (void)hipStreamSynchronize((hipStream_t)stream);   // nothing in flight reads what is freed now
    return rc;
  }
  *out = fl.release();
  return CWQ_OK;
}

extern "C" int cwq_fit_flat_info(const cwq_fit_flat* fl, int64_t* o) {
  if (!fl || !o) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flat_info: NULL argument");
  o[0] = fl->n_nodes;
  o[1] = fl->n_an;
  o[2] = fl->n_sent;
  o[3] = fl->D;
  o[4] = fl->depth;
  o[5] = fl->used;
  o[6] = fl->bytes;
  o[7] = 0;
  return CWQ_OK;
}

extern "C" int cwq_fit_flat_copy(const cwq_fit_flat* fl, float* mean, float* count, float* var_row, int64_t* an_nodes, float* an_var,
                                 int64_t* parent, int64_t* node_of_sentence, int32_t* slot_of_node, void* stream) {
  if (!fl) return fit_fail(CWQ_ERR_ARG, "cwq_fit_flat_copy: NULL handle");
  DevRestore dg(fl->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t Nn = (size_t)fl->n_nodes, D = (size_t)fl->D, na = (size_t)fl->n_an;
#define FCOPY(dst, src, bytes)                                                                              \
  if ((dst) && (bytes) && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)        \
    return fit_fail(CWQ_ERR_HIP, "cwq_fit_flat_copy failed");
  FCOPY(mean, fl->mean, Nn * D * 4);
  FCOPY(count, fl->count, Nn * 4);
  FCOPY(var_row, fl->var_row, Nn * 4);
  FCOPY(an_nodes, fl->an_nodes, na * 8);
  FCOPY(an_var, fl->an_var, na * D * 4);
  FCOPY(parent, fl->parent, Nn * 8);
  FCOPY(node_of_sentence, fl->nos, (size_t)fl->n_sent * 8);
  FCOPY(slot_of_node, fl->slot_of_node, Nn * 4);
#undef FCOPY
  FICHK(hipStreamSynchronize(s), "cwq_fit_flat_copy sync");
  return CWQ_OK;
}

extern "C" int cwq_fit_flat_destroy(cwq_fit_flat* fl) {
  if (!fl) return CWQ_OK;
  DevRestore dg(fl->device);
  delete fl;
  return CWQ_OK;
}

extern "C" int cwq_index_create_from_fit(cwq_fit* h, const int32_t* slot_of_sentence, int64_t n_sent,
                                         const double* level_w, int32_t n_w, void* stream, cwq_index** out) {
  if (!out) return both_fail(CWQ_ERR_ARG, "cwq_index_create_from_fit: out is NULL");
  *out = nullptr;
  if (!h) return both_fail(CWQ_ERR_ARG, "cwq_index_create_from_fit: NULL handle");
  if (n_sent < 0 || (n_sent > 0 && !slot_of_sentence) || n_w < 0 || (n_w > 0 && !level_w))
    return both_fail(CWQ_ERR_ARG, "cwq_index_create_from_fit: bad sentence map or level weights");
  hipStream_t s = (hipStream_t)stream;
  DevRestore dg(h->device);
  cwq_fit_flat* raw = nullptr;
  int rc = cwq_fit_flatten(h, slot_of_sentence, n_sent, stream, &raw);
  if (rc) return index_fail(rc, cwq_fit_last_error());
  std::unique_ptr<cwq_fit_flat> fl(raw);
  // the integer structure is all that goes to the host: 8 B per node, 8 B per sentence
  std::vector<int64_t> parent((size_t)fl->n_nodes), nos((size_t)std::max<int64_t>(n_sent, 1));
  if (hipMemcpyAsync(parent.data(), fl->parent, parent.size() * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      (n_sent > 0 && hipMemcpyAsync(nos.data(), fl->nos, (size_t)n_sent * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess)
    return both_fail(CWQ_ERR_HIP, "cwq_index_create_from_fit: structure download failed");
  fl->release(fl->parent);
  fl->parent = nullptr;
  fl->release(fl->nos);
  fl->nos = nullptr;
  fl->release(fl->slot_of_node);
  fl->slot_of_node = nullptr;
  const VarSrc vs{nullptr, fl->var_row, fl->an_map, fl->an_var};
  const char* msg = nullptr;
  rc = index_create_device(h->device, fl->n_nodes, fl->D, fl->mean, vs, parent.data(), nos.data(), n_sent, level_w,
                           n_w, s, out, &msg);
  (void)hipStreamSynchronize(s);   // the build kernels read the flat arrays (an error path may return early)
  if (rc) (void)fit_fail(rc, msg ? msg : "index build failed");
  return rc;
}

extern "C" int cwq_fit_info(cwq_fit* h, int64_t* o, void* stream) {
  if (!h || !o) return fit_fail(CWQ_ERR_ARG, "cwq_fit_info: NULL argument");
  DevRestore dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  int ctrl[16];
  int64_t c64[8];
  int rc = read_ctrl(h, s, ctrl, c64);
  if (rc) return rc;
  int removed = 0;
  if (ctrl[0] > 0) {
    int* d = h->f.dbg + 15;   // a spare word of the progress block (the insert kernel resets the block itself)
    FICHK(hipMemsetAsync(d, 0, sizeof(int), s), "cwq_fit_info reset");
    hipLaunchKernelGGL(fi_count_removed_kernel, dim3(grid_for(ctrl[0], 256)), dim3(256), 0, s, h->f.parent, ctrl[0], d);
    FICHK(hipGetLastError(), "cwq_fit_info launch");
    FICHK(hipMemcpyAsync(&removed, d, sizeof(int), hipMemcpyDeviceToHost, s), "cwq_fit_info read");
    FICHK(hipStreamSynchronize(s), "cwq_fit_info sync");
  }
  o[0] = h->f.cap;
  o[1] = ctrl[0];
  o[2] = ctrl[2];
  o[3] = removed;
  o[4] = c64[0];
  o[5] = h->f.arena_cap;
  o[6] = c64[1];
  o[7] = c64[2];
  return CWQ_OK;
}

extern "C" int cwq_fit_rewind(cwq_fit* h, void* stream) {
  if (!h) return fit_fail(CWQ_ERR_ARG, "cwq_fit_rewind: NULL handle");
  DevRestore dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  FICHK(hipMemsetAsync(h->f.ctrl64 + 1, 0, sizeof(int64_t), s), "cwq_fit_rewind");
  return CWQ_OK;
}

extern "C" int cwq_fit_set_rng(cwq_fit* h, const uint32_t* state625, void* stream) {
  if (!h || !state625) return fit_fail(CWQ_ERR_ARG, "cwq_fit_set_rng: NULL argument");
  if (state625[kMtN] > (uint32_t)kMtN) return fit_fail(CWQ_ERR_ARG, "cwq_fit_set_rng: state index out of range");
  DevRestore dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int idx = (int)state625[kMtN];
  FICHK(hipMemcpyAsync(h->f.mt, state625, (size_t)kMtN * 4, hipMemcpyHostToDevice, s), "cwq_fit_set_rng upload");
  FICHK(hipMemcpyAsync(h->f.ctrl + 4, &idx, 4, hipMemcpyHostToDevice, s), "cwq_fit_set_rng upload");
  FICHK(hipStreamSynchronize(s), "cwq_fit_set_rng sync");   // the host words may change after the return
  return CWQ_OK;
}

extern "C" int cwq_fit_get_rng(cwq_fit* h, uint32_t* state625, void* stream) {
  if (!h || !state625) return fit_fail(CWQ_ERR_ARG, "cwq_fit_get_rng: NULL argument");
  DevRestore dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  int idx = 0;
  FICHK(hipMemcpyAsync(state625, h->f.mt, (size_t)kMtN * 4, hipMemcpyDeviceToHost, s), "cwq_fit_get_rng download");
  FICHK(hipMemcpyAsync(&idx, h->f.ctrl + 4, 4, hipMemcpyDeviceToHost, s), "cwq_fit_get_rng download");
  FICHK(hipStreamSynchronize(s), "cwq_fit_get_rng sync");
  state625[kMtN] = (uint32_t)idx;
  return CWQ_OK;
}

extern "C" int cwq_fit_grow(cwq_fit* h, int32_t new_cap_nodes, void* stream) {
  if (!h) return fit_fail(CWQ_ERR_ARG, "cwq_fit_grow: NULL handle");
  if (new_cap_nodes <= h->f.cap) return fit_fail(CWQ_ERR_ARG, "cwq_fit_grow: the new capacity must exceed the old");
  DevRestore dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const FitDev& o = h->f;
  int ctrl[16];
  int64_t c64[8];
  int rc = read_ctrl(h, s, ctrl, c64);
  if (rc) return rc;
  const int used = ctrl[0];
  if (used < 0 || used > o.cap) return fit_fail(CWQ_ERR_HIP, "cwq_fit_grow: the handle's slot count is out of range");
  FitDev n = o;
  std::vector<void*> allocs;
  int *ncap = nullptr;
  int64_t *noff = nullptr, *bsum = nullptr, *d_total = nullptr;
  std::vector<void*> tmp;
  auto tal = [&](void** p, size_t b) -> bool {
    if (hipMalloc(p, b < 256 ? 256 : b) != hipSuccess) return false;
    tmp.push_back(*p);
    return true;
  };
  auto drop = [&](std::vector<void*>& v) {
    for (void* p : v) (void)hipFree(p);
    v.clear();
  };
  const size_t U = (size_t)std::max(used, 1);
  if (!fit_alloc(n, new_cap_nodes, allocs)) return fit_fail(CWQ_ERR_OOM, "cwq_fit_grow: device allocation failed");
  if (!tal((void**)&ncap, U * 4) || !tal((void**)&noff, U * 8) ||
      !tal((void**)&bsum, ((U + kScanTile - 1) / kScanTile + 1) * 8) || !tal((void**)&d_total, 8)) {
    drop(tmp);
    drop(allocs);
    return fit_fail(CWQ_ERR_OOM, "cwq_fit_grow: device allocation failed");
  }
  auto bail = [&](int code, const char* msg) {
    (void)hipStreamSynchronize(s);
    drop(tmp);
    drop(allocs);
    return fit_fail(code, msg);
  };
  const size_t D = (size_t)o.D;
  int64_t top = 0;
  bool ok = true;
  if (used > 0) {
    hipLaunchKernelGGL(fi_newcap_kernel, dim3(grid_for(used, 256)), dim3(256), 0, s, o.parent, o.ccnt, used, ncap);
    ok = hipGetLastError() == hipSuccess && launch_scan(ncap, used, noff, bsum, d_total, s) == hipSuccess &&
         hipMemcpyAsync(&top, d_total, 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return bail(CWQ_ERR_HIP, "cwq_fit_grow: the child-list scan failed");
    if (top > n.arena_cap / 2) return bail(CWQ_ERR_ARG, "cwq_fit_grow: the child lists exceed half of the new arena");
    hipLaunchKernelGGL(fi_repack_kernel, dim3(grid_for(used, 4)), dim3(256), 0, s, o.parent, o.ccnt, o.coff, o.arena,
                       o.arena_cap, used, ncap, noff, n.arena_cap, n.ccap, n.coff, n.arena);
    ok = hipGetLastError() == hipSuccess;
#define GCOPY(field, bytes) ok = ok && hipMemcpyAsync(n.field, o.field, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess
    GCOPY(count, U * 4);
    GCOPY(mean, U * D * 4);
    GCOPY(meanSq, U * D * 4);
    GCOPY(lvar, U * D * 4);
    GCOPY(parent, U * 4);
    GCOPY(ccnt, U * 4);
  }
  GCOPY(ctrl, 64);
  GCOPY(ctrl64, 64);
  GCOPY(mt, (size_t)kMtN * 4);
  GCOPY(dbg, 64);
#undef GCOPY
  ok = ok && hipMemcpyAsync(n.ctrl64, &top, 8, hipMemcpyHostToDevice, s) == hipSuccess;   // the packed arena's top
  ok = ok && hipStreamSynchronize(s) == hipSuccess;
  if (!ok) return bail(CWQ_ERR_HIP, "cwq_fit_grow: the device copy failed");
  drop(tmp);
  for (void* p : h->allocs) (void)hipFree(p);
  h->allocs = std::move(allocs);
  h->f = n;
  return CWQ_OK;
}
