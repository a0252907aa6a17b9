"""In-process A/B of libcwq builds on the bench workload (flat-synth N x D, Q queries).

Each library gets its own index over the same data; the builds then run in
interleaved rounds (A B C A B C ...), so clock/DVFS drift hits every arm alike.
Reports per-arm median call time and median summed fgemm launch time, and checks
that every arm returns the same ids/scores.  GPU only.

    python scripts/ab_libs.py --libs rag-cobweb_amd/libcwq.so,rag-cobweb_amd/libcwq_b.so

An arm may carry run-time knobs: `lib.so@CWQ_FG_CUTS=32,128;CWQ_FG_SAMPLE_DIV=128` sets
those variables while that arm's index is built and while it runs (arms are separated
by spaces when knobs contain commas: pass --libs once per arm).

    python scripts/ab_libs.py --libs a.so,b.so --rank-ce 1,16,256

--rank-ce times cwq_rank_ce with its gradient instead (HIP events, the arms taking turns inside
every repetition) and checks that the arms return the same bits; with --topk-loss K it times
cwq_rank_ce_topk at that K the same way.

    python scripts/ab_libs.py --libs a.so,b.so --clusters 100 --categorize 1,64,1024

    python scripts/ab_libs.py --libs parent.so,new.so --masked 1,16,10000 --fractions 1,0.5,0.1,0.01

--masked times the single-mask call score_topk(Q, k, mask=) per query count and allowed fraction
(scripts/mask_probe.py's cells; each arm builds its own mask from the same flags; HIP events,
the arms taking turns inside every repetition) and checks that the arms return the same bits.

--categorize times Basic (categorize) on the list paths (CWQ_CAT_DIRECT=0): host wall time of
the call plus a device synchronize (time.perf_counter, not HIP events), the arms taking turns
inside every repetition, and checks that the arms return the same nodes, found counts and call
counts.  The query counts run in the order given on each arm's one index, so the handle's
categorize policy state (cat_two_spec, cat_count_idle) carries from one count to the next --
the same sequence in every arm.
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402


@contextlib.contextmanager
def env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rank_ce_ab(paths, arms, Q, nqs, reps, K=0):
    gen = torch.Generator(device=Q.device).manual_seed(7)
    T = float(arms[0].rank_scores(Q[:1]).std())
    name = f"rank_ce_topk K={K}" if K else "rank_ce"

    def run(ix, q, labels):
        return ix.rank_ce_topk(q, labels, K, T, grad=True) if K else ix.rank_ce(q, labels, T, grad=True)

    for nq in nqs:
        q = Q[:nq].contiguous()
        labels = torch.randint(0, arms[0].n_sent, (nq,), device=Q.device, generator=gen)
        outs = [run(ix, q, labels) for ix in arms]
        same = all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
        torch.cuda.synchronize()
        ts = [[] for _ in arms]
        for _ in range(reps):
            for i, ix in enumerate(arms):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(ix, q, labels)
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b))
        med = [statistics.median(t) for t in ts]
        for p, t, m in zip(paths, ts, med):
            print(f"{name} nq={nq} {os.path.basename(p)[:60]}: {m:.3f} ms [{min(t):.3f}, {max(t):.3f}]  "
                  f"x{m / med[0]:.4f} vs first, own spread {(max(t) - min(t)) / m:.1%}  "
                  f"{'same bits' if same else 'MISMATCH'}", flush=True)


def masked_ab(paths, arms, Q, nqs, fractions, reps, k):
    gen = torch.Generator(device=Q.device).manual_seed(7)
    n = arms[0].n_sent
    for f in fractions:
        flags = torch.rand(n, device=Q.device, generator=gen) < f if f < 1 else torch.ones(n, dtype=torch.bool, device=Q.device)
        masks = [ix.sentence_mask(flags) for ix in arms]
        for nq in nqs:
            q = Q[:nq].contiguous()
            outs = [ix.score_topk(q, k, mask=m) for ix, m in zip(arms, masks)]
            same = all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
            path = [ix.last_mask_stats()["path"] for ix in arms]
            torch.cuda.synchronize()
            ts = [[] for _ in arms]
            for _ in range(reps):
                for i, (ix, m) in enumerate(zip(arms, masks)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ix.score_topk(q, k, mask=m)
                    b.record()
                    b.synchronize()
                    ts[i].append(a.elapsed_time(b))
            med = [statistics.median(t) for t in ts]
            for p, t, m, pa in zip(paths, ts, med, path):
                print(f"masked f={f:g} nq={nq} {os.path.basename(p)[:60]}: {m:.3f} ms [{min(t):.3f}, {max(t):.3f}]  "
                      f"x{m / med[0]:.4f} vs first, own spread {(max(t) - min(t)) / m:.1%}  path {pa}  "
                      f"{'same bits' if same else 'MISMATCH'}", flush=True)
        for m in masks:
            m.close()


def categorize_ab(paths, arms, Q, nqs, reps, k):
    """Basic (categorize) per arm, the arms taking turns inside every repetition (host wall time
    of the call plus a synchronize); nodes, found and calls must be equal between the arms.  CWQ_CAT_DIRECT=0 as in the tests: the path choice is
    measured at run time otherwise, and the arms could take different paths."""
    with env({"CWQ_CAT_DIRECT": "0"}):
        for nq in nqs:
            q = Q[:nq].contiguous()
            outs = [ix.categorize(q, k, 100000) for ix in arms]
            same = all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
            torch.cuda.synchronize()
            ts = [[] for _ in arms]
            for _ in range(reps):
                for i, ix in enumerate(arms):
                    t0 = time.perf_counter()
                    ix.categorize(q, k, 100000)
                    torch.cuda.synchronize()
                    ts[i].append((time.perf_counter() - t0) * 1e3)
            med = [statistics.median(t) for t in ts]
            for p, t, m in zip(paths, ts, med):
                print(f"categorize nq={nq} {os.path.basename(p)[:60]}: {m:.3f} ms [{min(t):.3f}, {max(t):.3f}]  "
                      f"x{m / med[0]:.4f} vs first  {'same nodes/found/calls' if same else 'MISMATCH'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, action="append")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--share-index", action="store_true",
                    help="one index for every arm (same library; knobs read per call only)")
    ap.add_argument("--rank-ce", default="", help="query counts: time rank_ce (loss + grad_q) per arm instead")
    ap.add_argument("--topk-loss", type=int, default=0, help="--rank-ce: time rank_ce_topk at this K instead")
    ap.add_argument("--categorize", default="", help="query counts: time categorize per arm instead")
    ap.add_argument("--masked", default="", help="query counts: time the single-mask score_topk(mask=) per arm instead")
    ap.add_argument("--fractions", default="1,0.5,0.1,0.01", help="--masked: allowed fractions")
    ap.add_argument("--reps", type=int, default=9, help="--rank-ce / --categorize: repetitions")
    ap.add_argument("--clusters", type=int, default=0, help="0: flat tree; G: root -> G random clusters -> leaves")
    args = ap.parse_args()
    pkg = cobweb_pkg.load()
    L = pkg._lib
    dev = torch.device("cuda", 0)
    X = pkg.synth.synthetic_corpus(args.n, args.dim, seed=0, device=dev)
    if args.clusters:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        labels = torch.randint(0, args.clusters, (args.n,), generator=g, device=dev)
        fs = pkg.synth.two_level_synth(X, labels)
    else:
        fs = pkg.synth.flat_synth(X)
    Q, _ = pkg.synth.synthetic_queries(X, args.queries, seed=1)
    del X
    paths = args.libs[0].split(",") if len(args.libs) == 1 and "@" not in args.libs[0] else args.libs
    knobs = {}
    for p in paths:
        kv = p.split("@", 1)[1] if "@" in p else ""
        knobs[p] = dict(x.split("=", 1) for x in kv.split(";") if x)
    arms = []
    for p in paths:
        if args.share_index and arms:
            arms.append(arms[0])
            continue
        with env(knobs[p]):
            L._lib = L.load_library(os.path.abspath(p.split("@")[0]), strict=False)
            ix = pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"], device=dev)
            if not args.rank_ce and not args.categorize:
                ix.set_filter(1)
                ix.score_topk(Q, args.k)
        arms.append(ix)
    del fs
    torch.cuda.empty_cache()
    if args.rank_ce:
        rank_ce_ab(paths, arms, Q, [int(v) for v in args.rank_ce.split(",")], args.reps, args.topk_loss)
        return
    if args.masked:
        masked_ab(paths, arms, Q, [int(v) for v in args.masked.split(",")], [float(v) for v in args.fractions.split(",")],
                  args.reps, args.k)
        return
    if args.categorize:
        categorize_ab(paths, arms, Q, [int(v) for v in args.categorize.split(",")], args.reps, args.k)
        return
    call = {p: [] for p in paths}
    fg = {p: [] for p in paths}
    smp = {p: [] for p in paths}   # sample_ms (sample pass + select + thresholds) and rerank_ms per round
    rer = {p: [] for p in paths}
    ref = None
    for r in range(args.rounds):
        for p, ix in zip(paths, arms):
            with env(knobs[p]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, sc = ix.score_topk(Q, args.k)
                torch.cuda.synchronize()
                call[p].append((time.perf_counter() - t0) * 1e3)
                ix.set_timing(True)
                ix.score_topk(Q, args.k)
                tm = ix.last_timing()
                fg[p].append(tm["fgemm_ms"])
                smp[p].append(tm["sample_ms"])
                rer[p].append(tm["rerank_ms"])
                ix.set_timing(False)
                if ref is None:
                    ref = (ids.cpu(), sc.cpu())
                elif not (torch.equal(ref[0], ids.cpu()) and torch.equal(ref[1], sc.cpu())):
                    print(f"MISMATCH {p} round {r}", flush=True)
        print(f"round {r}: " + "  ".join(f"{os.path.basename(p)[:60]} {call[p][-1]:.2f}/{fg[p][-1]:.3f}" for p in paths),
              flush=True)
    base = statistics.median(fg[paths[0]])
    for p, ix in zip(paths, arms):
        mc, mf = statistics.median(call[p]), statistics.median(fg[p])
        st = ix.last_stats()   # of the arm's last call
        print(f"{os.path.basename(p)[:60]}: call {mc:.3f} ms ({args.queries / mc * 1e3:.0f} q/s)  fgemm {mf:.3f} ms "
              f"(x{base / mf:.3f} vs first)  min {min(fg[p]):.3f}  sample {statistics.median(smp[p]):.3f} ms  rerank "
              f"{statistics.median(rer[p]):.3f} ms  cand/q {st['candidates']} reranks/q "
              f"{st['exact_reranks']} fallback {st['fallback_queries']} int8 launches {st.get('fg_i8_launches', 0)}",
              flush=True)


if __name__ == "__main__":
    main()
