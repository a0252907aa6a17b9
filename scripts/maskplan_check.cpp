// Checks the planner of cwq_score_topk_masked_multi's grouped gathered scan
// (rag-cobweb_amd/csrc/cwq_maskplan.h) on the host: a wrong plan would be an
// out-of-bounds access on the device.  Stand-alone, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/maskplan_check.cpp -o maskplan_check && ./maskplan_check
//
// (without the sanitizers where the toolchain does not link them: the checks below do not need
// them).  Runs the planner over edge and random shapes and checks, per plan:
//   - every (group, tile, query block) is covered exactly once, per segment;
//   - every work item's rows lie inside its group's row list, its queries inside its piece's
//     staged range, its piece inside the chunk's staged positions;
//   - every staged piece starts on a kMpXQ boundary and pieces do not overlap;
//   - the lists a work item writes lie inside its queries' list ranges, every list of every
//     staged query is written exactly once, the ranges are disjoint and inside the buffer;
//   - lists per query <= kMpMaxSlabs; launches per chunk <= 4; slabs are whole tiles;
//   - every query of every group is staged exactly once over the chunks.
// Exit status 0: all shapes passed.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../rag-cobweb_amd/csrc/cwq_maskplan.h"

using namespace cwq;

static long n_plans = 0;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "maskplan_check: %s failed (line %d)\n", #c, __LINE__); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static void check(const std::vector<MpGroup>& groups, const MpParams& p) {
  MaskPlan plan;
  mask_plan(groups, p, plan);
  ++n_plans;
  const int G = (int)groups.size();
  REQUIRE((int)plan.cfg.size() == G);
  std::vector<std::vector<int>> staged(G);   // times each query of each group is staged
  for (int g = 0; g < G; ++g) staged[g].assign(std::max(groups[g].nq, 0), 0);
  for (int g = 0; g < G; ++g) {
    const MpGroupCfg& c = plan.cfg[g];
    if (groups[g].nq <= 0) continue;
    REQUIRE(c.shq == (groups[g].nq <= kMpShqMaxQ));
    REQUIRE(c.lpq <= kMpMaxSlabs);
    for (int s = 0; s < 2; ++s) {
      const int n = groups[g].n_live[s];
      if (n <= 0) {
        REQUIRE(c.nslab[s] == 0);
        continue;
      }
      REQUIRE(c.nslab[s] >= 1);
      REQUIRE(c.rps[s] > 0 && c.rps[s] % mp_tile(c.shq) == 0);
      REQUIRE((int64_t)c.nslab[s] * c.rps[s] >= n && (int64_t)(c.nslab[s] - 1) * c.rps[s] < n);
    }
    REQUIRE(c.lpq == (c.nslab[0] + c.nslab[1]) * mp_lists(c.shq));
  }
  for (const MpChunk& ch : plan.chunks) {
    REQUIRE(ch.launches() <= 4);
    REQUIRE(!ch.pieces.empty());
    REQUIRE(ch.n_slots % kMpXQ == 0);
    // pieces: aligned, in order, inside the chunk; their list ranges disjoint, inside the buffer
    int slot = 0;
    int64_t lists = 0;
    std::map<int, const MpPiece*> piece_at;   // first slot -> piece
    for (const MpPiece& pc : ch.pieces) {
      const MpGroupCfg& c = plan.cfg[pc.group];
      REQUIRE(pc.group >= 0 && pc.group < G);
      REQUIRE(0 <= pc.qa && pc.qa < pc.qb && pc.qb <= groups[pc.group].nq);
      REQUIRE(pc.slot == slot && pc.slot % kMpXQ == 0);
      REQUIRE(pc.lbase == lists);
      slot += (int)(mp_ceil(pc.qb - pc.qa, kMpXQ) * kMpXQ);
      lists += (int64_t)(pc.qb - pc.qa) * c.lpq;
      piece_at[pc.slot] = &pc;
      for (int j = pc.qa; j < pc.qb; ++j) ++staged[pc.group][j];
    }
    REQUIRE(slot == ch.n_slots && lists == ch.n_lists);
    // the merge's queries: one per real staged query, its lists inside its piece's range
    REQUIRE((int64_t)ch.queries.size() <= ch.n_slots);
    std::vector<char> written((size_t)ch.n_lists, 0);
    size_t qi = 0;
    for (const MpPiece& pc : ch.pieces)
      for (int j = pc.qa; j < pc.qb; ++j, ++qi) {
        REQUIRE(qi < ch.queries.size());
        const MaskMergeQ& m = ch.queries[qi];
        REQUIRE(m.group == pc.group && m.gidx == j && m.slot == pc.slot + (j - pc.qa));
        REQUIRE(m.nlists == plan.cfg[pc.group].lpq && m.nlists <= kMpMaxSlabs);
        REQUIRE(m.lfirst == pc.lbase + (int64_t)(j - pc.qa) * m.nlists);
        REQUIRE(m.lfirst >= 0 && m.lfirst + m.nlists <= ch.n_lists);
      }
    REQUIRE(qi == ch.queries.size());
    // work items: what the kernel derives from them, replayed
    std::vector<std::tuple<int, int, int, int>> covered;   // (piece slot, segment, tile, 16-query block)
    for (int s = 0; s < 2; ++s)
      for (int f = 0; f < 2; ++f)
        for (const MaskWork& w : ch.work[s][f]) {
          const bool shq = f == 1;
          REQUIRE(w.group >= 0 && w.group < G);
          const MpGroupCfg& c = plan.cfg[w.group];
          REQUIRE(c.shq == shq);
          REQUIRE(piece_at.count(w.gq0));
          const MpPiece& pc = *piece_at[w.gq0];
          REQUIRE(pc.group == w.group && w.lbase == pc.lbase && w.lpq == c.lpq);
          REQUIRE(w.q_end == pc.slot + (pc.qb - pc.qa) && w.q_end <= ch.n_slots);
          REQUIRE(w.q0 % kMpXQ == 0 && w.q0 >= w.gq0 && w.q0 < w.q_end);
          REQUIRE((w.q0 - w.gq0) % mp_qblock(shq) == 0);
          REQUIRE(0 <= w.i_begin && w.i_begin < w.i_end && w.i_end <= groups[w.group].n_live[s]);
          REQUIRE(w.i_begin % mp_tile(shq) == 0 && w.i_begin % c.rps[s] == 0 && w.i_end - w.i_begin <= c.rps[s]);
          const int seg0 = s ? c.nslab[0] * mp_lists(shq) : 0;
          REQUIRE(w.lslot == seg0 + w.i_begin / c.rps[s] * mp_lists(shq));
          REQUIRE(w.lslot >= 0 && w.lslot + mp_lists(shq) <= w.lpq);
          // the waves' queries and the lists they write (mask_scan_kernel's own arithmetic)
          for (int wave = 0; wave < kMpWaves; ++wave) {
            const int q0 = w.q0 + (shq ? 0 : wave * kMpXQ);
            // the wave reads X and P of the staged positions [q0, q0 + nvq)
            const int nvq = std::max(0, std::min(kMpXQ, w.q_end - q0));
            REQUIRE(nvq == 0 || q0 + nvq <= ch.n_slots);
            for (int qq = q0; qq < q0 + kMpXQ; ++qq) {
              if (qq >= w.q_end) continue;
              const int64_t l = w.lbase + (int64_t)(qq - w.gq0) * w.lpq + w.lslot + (shq ? wave : 0);
              REQUIRE(l >= 0 && l < ch.n_lists);
              REQUIRE(!written[(size_t)l]);
              written[(size_t)l] = 1;
            }
          }
          for (int t = w.i_begin / mp_tile(shq); t < (int)mp_ceil(w.i_end, mp_tile(shq)); ++t)
            for (int qq = w.q0; qq < std::min(w.q_end, w.q0 + mp_qblock(shq)); qq += kMpXQ)
              covered.emplace_back(w.gq0, s, t, qq);
        }
    for (char c : written) REQUIRE(c);
    size_t want = 0;
    for (const MpPiece& pc : ch.pieces) {
      const MpGroupCfg& c = plan.cfg[pc.group];
      for (int s = 0; s < 2; ++s)
        want += (size_t)mp_ceil(std::max(groups[pc.group].n_live[s], 0), mp_tile(c.shq)) *
                (size_t)mp_ceil(pc.qb - pc.qa, kMpXQ);
    }
    REQUIRE(covered.size() == want);   // each once: as many as there are, no two the same
    std::sort(covered.begin(), covered.end());
    REQUIRE(std::adjacent_find(covered.begin(), covered.end()) == covered.end());
  }
  for (int g = 0; g < G; ++g) {
    const bool scanned = groups[g].nq > 0 && groups[g].n_live[0] + groups[g].n_live[1] > 0;
    for (int v : staged[g]) REQUIRE(v == (scanned ? 1 : 0));
  }
}

int main() {
  const int nqs[] = {0, 1, 15, 16, 17, 32, 33, 64, 65};
  const int lives[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000000};
  MpParams p;
  p.entry_bytes = 12;
  // every group size x live-row count, alone and beside a second group, both segments
  for (int cus : {1, 256})
    for (int K : {10, 64})
      for (size_t budget : {(size_t)1 << 16, (size_t)16 << 30})
        for (int nq : nqs)
          for (int li : lives)
            for (int la : {0, 1, 65, 257}) {
              if (li == 1000000 && (K != 10 || la == 1 || la == 257)) continue;   // keeps the run short
              p.cus = cus;
              p.K = K;
              p.budget = budget;
              p.slot_bytes = 128 * 4 + 8;
              check({MpGroup{nq, {li, la}}}, p);
              check({MpGroup{17, {300, 0}}, MpGroup{nq, {li, la}}, MpGroup{70, {0, 129}}}, p);
            }
  // random shapes, up to 4096 masks
  std::mt19937 rng(12345);
  for (int it = 0; it < 1000; ++it) {
    const int G = it < 2 ? 4096 : 1 + (int)(rng() % (it % 10 == 0 ? 600 : 40));
    std::vector<MpGroup> gs((size_t)G);
    for (MpGroup& g : gs) {
      g.nq = nqs[rng() % 9];
      if (rng() % 4 == 0) g.nq = (int)(rng() % 300);
      const int pick = (int)(rng() % 10);
      g.n_live[0] = pick < 9 ? lives[rng() % 8] : (int)(rng() % 20000);
      g.n_live[1] = rng() % 3 ? 0 : lives[rng() % 8];
      if (G <= 8 && rng() % 16 == 0) g.n_live[0] = 1000000;
    }
    p.cus = rng() % 2 ? 256 : 1 + (int)(rng() % 300);
    p.K = 1 + (int)(rng() % 64);
    p.slot_bytes = 128 + 4 * (size_t)(rng() % 4000);
    p.budget = (size_t)1 << (16 + rng() % 18);
    check(gs, p);
  }
  std::printf("maskplan_check: %ld plans ok\n", n_plans);
  return 0;
}
