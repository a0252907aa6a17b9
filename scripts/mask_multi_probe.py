"""Per-query masks probe: one cwq_score_topk_masked_multi call against what a
caller did before it, a loop of single-mask calls over the groups of the batch.

    python scripts/mask_multi_probe.py [--n 1000000] [--dim 768] [--k 10] [--masks 2,16,128,1000]
                                       [--nq 64,1024,10000] [--fractions 0.5,0.1,0.01,disjoint]

Shape: C3, the flat-synth tree bench.py builds.  Per cell (G masks, nq queries spread evenly and
shuffled, per-mask allowed fraction; "disjoint": G tenants that split the corpus):
  (a) score_topk(Q, k, masks=, mask_of_query=), one call;
  (b) for every mask g: score_topk(Q[idx_g], k, mask=m_g), the results scattered back -- the
      single-mask call is the same code before and after this feature;
  (c) rank_scores -> per-query masked_fill -> topk, at the smallest cell only.
Timed as scripts/mask_probe.py does: events around warm calls, the arms interleaved in one
process, medians with [min, max]; every arm's ids and scores are compared with (a)'s.  The
verdict per cell compares the medians' gap with the arms' own spread (max - min).  Also: the
gathered scan's row-queries/s of (a) under CWQ_MASK_PATH=2 (live rows x queries over the call's
time -- the whole call, so a lower bound of the kernel's rate), a mixed cell (1,000 tenants of
unequal size and a few dense masks), and the multi call with one mask beside the single-mask
call it delegates to."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cobweb_pkg  # noqa: E402


def timed_interleaved(fns, reps):
    """Per arm: (last output, median, min, max) ms of `reps` warm calls, the arms taking turns."""
    outs = [fn() for fn in fns]
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[i] = fn()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1))
    return [(o, statistics.median(t), min(t), max(t)) for o, t in zip(outs, ts)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--masks", default="2,16,128,1000")
    ap.add_argument("--nq", default="64,1024,10000")
    ap.add_argument("--fractions", default="0.5,0.1,0.01,disjoint")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-mixed", action="store_true")
    a = ap.parse_args()
    pkg = cobweb_pkg.load()
    N, D, k = a.n, a.dim, a.k
    X = pkg.synth.synthetic_corpus(N, D, seed=0)
    t = pkg.synth.flat_synth(X, compact=True)
    ix = pkg.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
    del t
    print(f"# mask_multi_probe: flat {N} x {D}, top-{k}, build {pkg.lib().cwq_build_id().decode()}, "
          f"{torch.cuda.get_device_name(0)}, {a.reps} reps, medians [min, max] ms", flush=True)
    nq_max = max(int(v) for v in a.nq.split(","))
    Qall, _ = pkg.synth.synthetic_queries(X, nq_max, seed=1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    os.environ.pop("CWQ_MASK_PATH", None)

    def loop_call(Q, masks, groups):
        ids = torch.empty((Q.shape[0], k), dtype=torch.int64, device=Q.device)
        sc = torch.empty((Q.shape[0], k), dtype=torch.float32, device=Q.device)
        for m, idx in zip(masks, groups):
            if idx.numel():
                ids[idx], sc[idx] = ix.score_topk(Q[idx], k, mask=m)
        return ids, sc

    def cell(label, masks, moq, Q, with_c=False, flags=None):
        G = len(masks)
        groups = [torch.nonzero(moq == g).flatten() for g in range(G)]
        moq_h = moq.cpu().numpy()
        fns = [lambda: ix.score_topk(Q, k, masks=masks, mask_of_query=moq_h), lambda: loop_call(Q, masks, groups)]
        if with_c:
            def arm_c():
                s = ix.rank_scores(Q)
                s = s.masked_fill(~flags[moq], float("-inf"))
                v, i = torch.topk(s, k, dim=1)
                return i, v
            fns.append(arm_c)
        res = timed_interleaved(fns, a.reps)
        st = ix.last_mask_multi_stats() if G > 1 else {}
        (ia, sa), ma, lo_a, hi_a = res[0]
        (ib, sb), mb, lo_b, hi_b = res[1]
        same = bool(torch.equal(ia, ib) and torch.equal(sa, sb))
        spread = max(hi_a - lo_a, hi_b - lo_b)
        verdict = "multi faster" if mb - ma > spread else "multi SLOWER" if ma - mb > spread else "within spread"
        line = (f"{label:<34} multi {ma:9.3f} [{lo_a:.3f}, {hi_a:.3f}]  loop {mb:9.3f} [{lo_b:.3f}, {hi_b:.3f}]  "
                f"x{mb / ma:6.2f}  {verdict}  same={same}")
        if with_c:
            (ic, sc_), mc, lo_c, hi_c = res[2]
            # torch.topk breaks ties its own way and rank_scores gives -inf outside the tree: ids where scores differ
            agree = float((ic == ia).float().mean())
            line += f"  torch {mc:9.3f} [{lo_c:.3f}, {hi_c:.3f}] ids agree {agree:.4f}"
        # the gathered scan alone: every mask through it
        os.environ["CWQ_MASK_PATH"] = "2"
        (r2, m2, lo2, hi2), = timed_interleaved([fns[0]], max(2, a.reps // 2))
        os.environ.pop("CWQ_MASK_PATH", None)
        rq = sum((m.info["live_iso_rows"] + m.info["live_aniso_rows"]) * int(g.numel()) for m, g in zip(masks, groups))
        same2 = bool(torch.equal(r2[0], ia) and torch.equal(r2[1], sa))
        line += (f"  | gathered-only {m2:9.3f} [{lo2:.3f}, {hi2:.3f}] {rq / m2 / 1e6:7.2f} G row-q/s same={same2}"
                 f"  | stats {st}")
        print(line, flush=True)
        return same and same2

    ok = True
    Gs = [int(v) for v in a.masks.split(",")]
    first = True
    for G in Gs:
        for frac in a.fractions.split(","):
            if frac == "disjoint":
                owner = torch.randint(0, G, (N,), device="cuda", generator=gen)
                flags = torch.stack([owner == g for g in range(G)]) if G <= 16 else None
                masks = [ix.sentence_mask(owner == g) for g in range(G)]
            else:
                f = float(frac)
                flags = None
                masks = []
                fl = []
                for g in range(G):
                    m = torch.rand(N, device="cuda", generator=gen) < f
                    masks.append(ix.sentence_mask(m))
                    if G <= 2:
                        fl.append(m)
                if G <= 2:
                    flags = torch.stack(fl)
            for nq in (int(v) for v in a.nq.split(",")):
                Q = Qall[:nq].contiguous()
                moq = (torch.arange(nq, device="cuda") % G)[torch.randperm(nq, device="cuda", generator=gen)]
                with_c = first and flags is not None and nq <= 64
                ok &= cell(f"G={G:<5} nq={nq:<6} f={frac:<8}", masks, moq, Q, with_c, flags)
                first = first and not with_c
            for m in masks:
                m.close()
            del masks, flags
    if not a.no_mixed:
        # 1,000 tenants of unequal size (a power law over the corpus) and four dense masks
        G = 1000
        w = torch.arange(1, G + 1, device="cuda", dtype=torch.float64) ** -1.0
        owner = torch.multinomial(w / w.sum(), N, replacement=True, generator=gen)
        masks = [ix.sentence_mask(owner == g) for g in range(G)]
        masks += [ix.sentence_mask(torch.rand(N, device="cuda", generator=gen) < f) for f in (1.0, 0.5, 0.5, 0.1)]
        nq = nq_max
        moq = torch.multinomial(torch.cat([w / w.sum(), torch.full((4,), 0.01, device="cuda", dtype=torch.float64)]), nq,
                                replacement=True, generator=gen)
        ok &= cell(f"mixed G={len(masks)} nq={nq}", masks, moq, Qall[:nq].contiguous(), False, None)
        # one mask: the multi call delegates to the single-mask call
        for j in (0, G + 1):
            one = torch.full((nq,), j).numpy()
            Q = Qall[:nq].contiguous()
            res = timed_interleaved([lambda: ix.score_topk(Q, k, masks=masks, mask_of_query=one),
                                     lambda: ix.score_topk(Q, k, mask=masks[j])], a.reps)
            same = torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][0][1], res[1][0][1])
            ok &= bool(same)
            print(f"one mask (slot {j}, nq={nq}): multi {res[0][1]:.3f} [{res[0][2]:.3f}, {res[0][3]:.3f}]  single "
                  f"{res[1][1]:.3f} [{res[1][2]:.3f}, {res[1][3]:.3f}]  same={same}", flush=True)
        for m in masks:
            m.close()
    print("# all arms identical:", ok, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
