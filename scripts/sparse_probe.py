"""Sparse differentiable scores against the dense paths, in one process, HIP
events, the arms taking turns inside every repetition, median of --reps with [min, max].  GPU only.

    python scripts/sparse_probe.py --n 1000000 --nq 1,16,256            # flat tree (C3)
    python scripts/sparse_probe.py --balanced 10,4 --n 100000 --nq 1,16,256   # 11,111 internal nodes, leaves at depth 5

Arms per nq:
  (a) rank_ce fwd + bwd (skipped above --full-max queries: it streams every row twice per tile)
  (b) rank_ce_topk at K = 10 and 64, fwd + bwd and forward only
  (c) score_topk without grad at the same K, beside (b)'s forward
  (d) score_pairs + score_pairs_backward at m = 64 against rank_scores + gather +
      rank_scores_backward of the scattered upstream, with peak torch memory
Every arm's outputs are cross-checked: (b)'s candidates and target score against (c) and
rank_scores, (b)'s loss against (a)'s within its own tail bound, (d)'s two sides against each
other.  --tail prints the distribution of tail_bound and of the true L_full - loss at K = 64
for T = 1 and T = the score standard deviation.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402
from scripts.grad_probe import event_all, peak_mb  # noqa: E402


def fmt(t):
    return f"{t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def probe(ix, Q, nqs, reps, T, tag, full_max):
    dev = ix.device
    gen = torch.Generator(device=dev).manual_seed(7)
    for nq in nqs:
        q = Q[:nq].contiguous()
        labels = torch.randint(0, ix.n_sent, (nq,), device=dev, generator=gen)
        with_full = nq <= full_max
        fns, names = [], []
        if with_full:
            fns.append(lambda: ix.rank_ce(q, labels, T, grad=True))
            names.append("(a) rank_ce fwd+bwd")
        for K in (10, 64):
            fns += [lambda K=K: ix.rank_ce_topk(q, labels, K, T, grad=True), lambda K=K: ix.rank_ce_topk(q, labels, K, T),
                    lambda K=K: ix.score_topk(q, K)]
            names += [f"(b) rank_ce_topk K={K} fwd+bwd", f"(b) rank_ce_topk K={K} fwd", f"(c) score_topk k={K}"]
        # cross-checks
        S = ix.rank_scores(q[:16])
        for K in (10, 64):
            loss, gq, ts, rank, bound, cand = ix.rank_ce_topk(q, labels, K, T, grad=True)
            ids, _ = ix.score_topk(q, K)
            assert torch.equal(cand, ids)
            assert torch.equal(ts[:16], S[torch.arange(min(nq, 16), device=dev), labels[:16]])
            assert torch.isfinite(gq).all()
            if with_full:
                lf, gf, tsf, rf = ix.rank_ce(q, labels, T, grad=True)
                eps = 1e-5 * lf.abs().clamp(min=1)
                assert bool(((lf - loss) >= -eps).all()) and bool(((lf - loss) <= bound * (1 + 1e-5) + eps).all())
                assert torch.equal(rank, torch.where(rf <= K, rf, torch.full_like(rf, K + 1)))
        ts_ = event_all(fns, reps)
        for n_, t in zip(names, ts_):
            print(f"sparse {tag} nq={nq} T={T:.3g}: {n_} {fmt(t)}", flush=True)
        if with_full:
            b64 = ts_[names.index("(b) rank_ce_topk K=64 fwd+bwd")]
            a = ts_[0]
            sep = "ranges do not overlap" if b64[2] < a[1] else "RANGES OVERLAP" if b64[1] <= a[2] else "TOPK SLOWER"
            print(f"sparse {tag} nq={nq}: (b) K=64 fwd+bwd / (a) = {b64[0] / a[0]:.4f}  ({sep})", flush=True)
        # (d) m = 64 pairs against the dense route
        m = 64
        ids = torch.randint(0, ix.n_sent, (nq, m), device=dev, generator=gen)
        g = torch.randn((nq, m), device=dev, generator=gen)

        def d_sparse():
            return ix.score_pairs(q, ids), ix.score_pairs_backward(q, ids, g)

        def d_dense():
            s = ix.rank_scores(q).gather(1, ids)
            G = torch.zeros((nq, ix.n_sent), device=dev).scatter_add_(1, ids, g)
            return s, ix.rank_scores_backward(q, G)
        if nq <= full_max:
            (s1, g1), (s2, g2) = d_sparse(), d_dense()
            assert torch.equal(s1, s2)
            rel = float(((g1 - g2).double().norm(dim=1) / g2.double().norm(dim=1)).max())
            td = event_all((d_sparse, d_dense), reps)
            print(f"sparse {tag} nq={nq}: (d) score_pairs + backward m=64 {fmt(td[0])}  rank_scores + gather + "
                  f"rank_scores_backward {fmt(td[1])}  peak torch memory {peak_mb(d_sparse):.3f} / {peak_mb(d_dense):.1f} MiB  "
                  f"grad max rel L2 {rel:.3g}", flush=True)
        else:
            td = event_all((d_sparse,), reps)
            print(f"sparse {tag} nq={nq}: (d) score_pairs + backward m=64 {fmt(td[0])}  (dense route skipped above "
                  f"{full_max} queries)", flush=True)


def tail(ix, Q, nq, tag):
    """tail_bound and the true L_full - loss at K = 64 over nq queries with random labels."""
    dev = ix.device
    q = Q[:nq].contiguous()
    labels = torch.randint(0, ix.n_sent, (nq,), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    for name, T in (("T=1", 1.0), ("T=std", float(ix.rank_scores(q[:1]).std()))):
        loss, _, _, _, bound, _ = ix.rank_ce_topk(q, labels, 64, T)
        lf = ix.rank_ce(q, labels, T)[0]
        gap = (lf - loss).double()
        qs = torch.tensor([0.0, 0.5, 0.9, 0.99, 1.0], device=dev, dtype=torch.float64)
        print(f"tail {tag} K=64 {name} ({T:.4g}) nq={nq}: tail_bound quantiles 0/50/90/99/100% "
              f"{[float(f'{v:.3g}') for v in torch.quantile(bound.double(), qs)]}  true L_full - loss "
              f"{[float(f'{v:.3g}') for v in torch.quantile(gap, qs)]}  loss median {float(loss.median()):.4g}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--balanced", default="", help="b,depth: synth.balanced_synth over the --n rows instead of a flat tree")
    ap.add_argument("--nq", default="1,16,256")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--full-max", type=int, default=256, help="largest nq at which the dense arms run")
    ap.add_argument("--tail", type=int, default=0, help="queries of the tail-bound distribution (0: none)")
    ap.add_argument("--temperature", type=float, default=0.0, help="0 = the standard deviation of the first query's scores")
    args = ap.parse_args()
    pkg = cobweb_pkg.load()
    dev = torch.device("cuda", 0)
    nqs = [int(v) for v in args.nq.split(",")]
    if args.balanced:
        b, L = (int(v) for v in args.balanced.split(","))
        X = pkg.synth.synthetic_corpus(args.n, args.dim, seed=0, device=dev)
        t = pkg.synth.balanced_synth(X, b, L)
        tag = f"balanced b={b} depth={L} n={args.n} d={args.dim}"
    else:
        X = pkg.synth.synthetic_corpus(args.n, args.dim, seed=0, device=dev)
        t = pkg.synth.flat_synth(X)
        tag = f"flat n={args.n} d={args.dim}"
    Q, _ = pkg.synth.synthetic_queries(X, max(max(nqs), args.tail, 16), seed=1)
    del X
    ix = pkg.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=dev)
    del t
    torch.cuda.empty_cache()
    print(f"{tag}: {ix.info}", flush=True)
    T = args.temperature or float(ix.rank_scores(Q[:1]).std())
    probe(ix, Q, nqs, args.reps, T, tag, args.full_max)
    if args.tail:
        tail(ix, Q, args.tail, tag)
    print("done", flush=True)


if __name__ == "__main__":
    main()
