// The plan of cwq_score_topk_masked_multi's grouped gathered scan: host only, no
// HIP call and no HIP header, so scripts/maskplan_check.cpp compiles it with the host compiler
// and checks it over random and edge shapes -- a wrong plan is an out-of-bounds access on the
// device.  Included by cwq_internal.h (the kernels read MaskWork / MaskMergeQ) and by
// cwq_maskcalls.hip (which fills in the device pointers).
//
// A group is one mask's queries that go through the gathered scan.  The plan
//   - gives every group its form (<= kMpShqMaxQ queries: the shared-query 256-row form, else
//     the 64-row, 64-query form) and, per segment (0 isotropic, 1 anisotropic), its slab split:
//     whole tiles, at least one slab, sized for 4 resident workgroups per CU over the call, the
//     lists per query of both segments together <= kMpMaxSlabs;
//   - cuts the call into workspace chunks at group boundaries (a group larger than a chunk is
//     split at multiples of 64 queries);
//   - stages a chunk's queries sorted by group, each piece from a kMpXQ boundary of the
//     interleaved X layout, so the queries of a workgroup always share one row list;
//   - lists the work items of every (segment, form) -- one kernel launch each, so at most four
//     gathered launches a chunk however many masks the call names -- with the query blocks of
//     one tile adjacent;
//   - lays the partial lists out as a CSR per staged query (first list, list count).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace cwq {

constexpr int kMpXQ = 16;         // = kXQ: queries per scalar-load group
constexpr int kMpWaves = 4;       // = kWavesPerWG
constexpr int kMpShqMaxQ = 32;    // groups up to here take the shared-query form
constexpr int kMpMaxSlabs = 2048; // partial lists per query, at most (both segments together)
constexpr int kMpSplitQ = 64;     // a group larger than a chunk is split at multiples of this

constexpr int mp_tile(bool shq) { return shq ? 256 : 64; }          // = mask_scan_tile
constexpr int mp_lists(bool shq) { return shq ? kMpWaves : 1; }     // = mask_scan_lists
constexpr int mp_qblock(bool shq) { return shq ? kMpXQ : kMpXQ * kMpWaves; }

// One workgroup's job in the grouped gathered scan.  The planner fills everything but `list`.
struct MaskWork {
  const int* list;   // the group's row list of this segment (device; the host layer sets it)
  int64_t lbase;     // first partial list of the piece's first query
  int i_begin;       // the slab: entries [i_begin, i_end) of `list`
  int i_end;
  int q0;            // first staged query of the block (a multiple of kMpXQ)
  int q_end;         // end of the piece's staged queries
  int gq0;           // first staged query of the piece
  int lpq;           // partial lists per query of the group
  int lslot;         // this slab's first list among a query's lpq
  int group;         // index into the planner's groups
};

// One staged query of the grouped merge.  The planner fills everything but `bits` and `orig`.
struct MaskMergeQ {
  const uint32_t* bits;   // the query's mask (device; the host layer sets it)
  int64_t lfirst;         // the query's partial lists: [lfirst, lfirst + nlists)
  int nlists;
  int orig;               // the query's position in the call (the host layer sets it)
  int slot;               // its staged position in the chunk
  int group;
  int gidx;               // which of the group's queries
};

struct MpGroup {      // in
  int nq;             // queries to scan
  int n_live[2];      // live rows: isotropic, anisotropic
};

struct MpGroupCfg {   // out, per group
  bool shq;
  int nslab[2], rps[2];   // slabs and list entries per slab (a multiple of the tile), per segment
  int lpq;                // (nslab[0] + nslab[1]) * mp_lists(shq)
};

struct MpPiece {      // a group's queries [qa, qb) staged at slots [slot, slot + qb - qa)
  int group, qa, qb, slot;
  int64_t lbase;
};

struct MpChunk {
  std::vector<MpPiece> pieces;
  int n_slots = 0;         // staged positions (a multiple of kMpXQ), gaps included
  int64_t n_lists = 0;     // partial lists of the chunk
  std::vector<MaskWork> work[2][2];   // [segment][shq]
  std::vector<MaskMergeQ> queries;    // the real staged queries, in staged order
  int launches() const {
    int n = 0;
    for (int s = 0; s < 2; ++s)
      for (int f = 0; f < 2; ++f) n += work[s][f].empty() ? 0 : 1;
    return n;
  }
};

struct MpParams {
  int cus;               // compute units
  int K;                 // list length (min(k, 64))
  size_t budget;         // workspace bytes a chunk may take
  size_t slot_bytes;     // fixed workspace bytes per staged position
  size_t entry_bytes;    // bytes per partial-list entry (key, aux, row: 12)
};

struct MaskPlan {
  std::vector<MpGroupCfg> cfg;
  std::vector<MpChunk> chunks;
};

inline int64_t mp_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workspace bytes of nq queries of a group
inline size_t mp_cost(const MpParams& p, const MpGroupCfg& c, int nq) {
  return (size_t)mp_ceil(nq, kMpXQ) * kMpXQ * p.slot_bytes + (size_t)nq * c.lpq * p.K * p.entry_bytes;
}

inline void mask_plan(const std::vector<MpGroup>& groups, const MpParams& p, MaskPlan& out) {
  const int G = (int)groups.size();
  out.cfg.assign(G, MpGroupCfg());
  out.chunks.clear();
  // ---- forms, and the tiles a slab should hold (tps).  4 workgroups per CU are resident at
  // once.  Two candidates: the balanced split, tile jobs / (4 per CU) -- every workgroup at
  // most that long, which suits groups of unequal size, whose small workgroups leave their
  // slots early; and the fewest tiles for which the call's workgroups number at most 4 per
  // CU, which suits equal groups (slab_split's choice for one mask: one workgroup more would
  // run alone in a second round).  Between them, by a replay of the launch: the workgroups
  // in launch order onto 4 slots per CU, the shortest finish wins. ----
  int64_t max_tiles = 1, tile_jobs = 0;
  for (int g = 0; g < G; ++g) {
    MpGroupCfg& c = out.cfg[g];
    c.shq = groups[g].nq <= kMpShqMaxQ;
    if (groups[g].nq <= 0) continue;
    for (int s = 0; s < 2; ++s) {
      const int64_t tiles = mp_ceil(std::max(groups[g].n_live[s], 0), mp_tile(c.shq));
      max_tiles = std::max(max_tiles, tiles);
      tile_jobs += tiles * mp_ceil(groups[g].nq, mp_qblock(c.shq));
    }
  }
  const int64_t target = (int64_t)4 * std::max(p.cus, 1);
  // slabs of a segment with `tiles` tiles at tps tiles a slab
  auto slabs_of = [](int64_t tiles, int64_t tps, bool shq) {
    return std::max<int64_t>(1, std::min<int64_t>(kMpMaxSlabs / (2 * mp_lists(shq)), mp_ceil(tiles, tps)));
  };
  auto workgroups = [&](int64_t tps) {
    int64_t n = 0;
    for (int g = 0; g < G; ++g) {
      if (groups[g].nq <= 0) continue;
      const bool shq = out.cfg[g].shq;
      for (int s = 0; s < 2; ++s)
        if (groups[g].n_live[s] > 0)
          n += mp_ceil(groups[g].nq, mp_qblock(shq)) * slabs_of(mp_ceil(groups[g].n_live[s], mp_tile(shq)), tps, shq);
    }
    return n;
  };
  // finish time of the launches at tps: a workgroup costs its slab's tiles (both forms do 4096
  // row-queries a tile step), each goes to the slot that is free first
  auto finish = [&](int64_t tps) {
    std::vector<int64_t> heap((size_t)target, 0);   // min-heap of the slots' busy-until times
    int64_t end = 0;
    for (int g = 0; g < G; ++g) {
      if (groups[g].nq <= 0) continue;
      const bool shq = out.cfg[g].shq;
      const int64_t nqb = mp_ceil(groups[g].nq, mp_qblock(shq));
      for (int s = 0; s < 2; ++s) {
        if (groups[g].n_live[s] <= 0) continue;
        const int64_t tiles = mp_ceil(groups[g].n_live[s], mp_tile(shq)), n = slabs_of(tiles, tps, shq);
        const int64_t per = mp_ceil(tiles, n);
        for (int64_t i = 0; i < n * nqb; ++i) {
          std::pop_heap(heap.begin(), heap.end(), std::greater<int64_t>());
          heap.back() += per;
          end = std::max(end, heap.back());
          std::push_heap(heap.begin(), heap.end(), std::greater<int64_t>());
        }
      }
    }
    return end;
  };
  int64_t lo = 1, hi = max_tiles;   // workgroups(tps) does not grow with tps
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if (workgroups(mid) <= target) hi = mid; else lo = mid + 1;
  }
  const int64_t tps_cap = lo, tps_bal = std::min(tps_cap, std::max<int64_t>(1, mp_ceil(tile_jobs, target)));
  int64_t tps = tps_cap, best = finish(tps_cap);
  for (int64_t t = tps_bal; t < tps_cap; t = std::max(t + 1, t + t / 4)) {
    const int64_t f = finish(t);
    if (f < best) {
      best = f;
      tps = t;
    }
  }
  for (int g = 0; g < G; ++g) {
    MpGroupCfg& c = out.cfg[g];
    const int tile = mp_tile(c.shq), cap = kMpMaxSlabs / (2 * mp_lists(c.shq));
    for (int s = 0; s < 2; ++s) {
      c.nslab[s] = c.rps[s] = 0;
      const int n_live = groups[g].n_live[s];
      if (n_live <= 0 || groups[g].nq <= 0) continue;
      const int64_t tiles = mp_ceil(n_live, tile);
      const int64_t n = std::max<int64_t>(1, std::min<int64_t>(cap, mp_ceil(tiles, tps)));
      c.rps[s] = (int)(mp_ceil(tiles, n) * tile);
      c.nslab[s] = (int)mp_ceil(n_live, c.rps[s]);
    }
    c.lpq = (c.nslab[0] + c.nslab[1]) * mp_lists(c.shq);
  }
  // ---- chunks: whole groups while they fit, a group larger than a chunk in pieces ----
  MpChunk cur;
  size_t used = 0;
  auto flush = [&]() {
    if (!cur.pieces.empty()) out.chunks.push_back(std::move(cur));
    cur = MpChunk();
    used = 0;
  };
  auto add_piece = [&](int g, int qa, int qb) {
    const MpGroupCfg& c = out.cfg[g];
    MpPiece pc;
    pc.group = g;
    pc.qa = qa;
    pc.qb = qb;
    pc.slot = cur.n_slots;
    pc.lbase = cur.n_lists;
    cur.pieces.push_back(pc);
    cur.n_slots += (int)(mp_ceil(qb - qa, kMpXQ) * kMpXQ);
    cur.n_lists += (int64_t)(qb - qa) * c.lpq;
    used += mp_cost(p, c, qb - qa);
  };
  for (int g = 0; g < G; ++g) {
    const int nq = groups[g].nq;
    if (nq <= 0 || out.cfg[g].lpq == 0) continue;   // nothing to scan
    const MpGroupCfg& c = out.cfg[g];
    if (used + mp_cost(p, c, nq) <= p.budget) {
      add_piece(g, 0, nq);
      continue;
    }
    if (mp_cost(p, c, nq) <= p.budget) {   // fits a chunk of its own: cut at the group boundary
      flush();
      add_piece(g, 0, nq);
      continue;
    }
    flush();
    const size_t per64 = std::max<size_t>(1, mp_cost(p, c, kMpSplitQ));
    const int step = (int)std::min<int64_t>((int64_t)1 << 24, std::max<size_t>(1, p.budget / per64)) * kMpSplitQ;
    for (int qa = 0; qa < nq; qa += step) {
      add_piece(g, qa, std::min(nq, qa + step));
      if (qa + step < nq) flush();
    }
  }
  flush();
  // ---- work items and the list CSR ----
  for (MpChunk& ch : out.chunks) {
    for (const MpPiece& pc : ch.pieces) {
      const MpGroupCfg& c = out.cfg[pc.group];
      const int n = pc.qb - pc.qa, qblk = mp_qblock(c.shq), lps = mp_lists(c.shq);
      const int nqb = (int)mp_ceil(n, qblk);
      for (int s = 0; s < 2; ++s)
        for (int slab = 0; slab < c.nslab[s]; ++slab)
          for (int qb = 0; qb < nqb; ++qb) {   // queries fastest: a tile's query blocks are adjacent
            MaskWork w;
            w.list = nullptr;
            w.lbase = pc.lbase;
            w.i_begin = slab * c.rps[s];
            w.i_end = std::min(w.i_begin + c.rps[s], groups[pc.group].n_live[s]);
            w.q0 = pc.slot + qb * qblk;
            w.q_end = pc.slot + n;
            w.gq0 = pc.slot;
            w.lpq = c.lpq;
            w.lslot = (s ? c.nslab[0] * lps : 0) + slab * lps;
            w.group = pc.group;
            ch.work[s][c.shq ? 1 : 0].push_back(w);
          }
      for (int j = 0; j < n; ++j) {
        MaskMergeQ m;
        m.bits = nullptr;
        m.lfirst = pc.lbase + (int64_t)j * c.lpq;
        m.nlists = c.lpq;
        m.orig = -1;
        m.slot = pc.slot + j;
        m.group = pc.group;
        m.gidx = pc.qa + j;
        ch.queries.push_back(m);
      }
    }
  }
}

}  // namespace cwq
