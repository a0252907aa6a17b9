"""Differentiable rank_scores timing: forward (cwq_rank_scores) and backward
(cwq_rank_scores_backward) over the flat-synth C3 tree (1M x 768) for nq = 1 and 16, like a
training step through cobweb_rank_scores (CobwebWrapper.py:267-294,
src/training/cobweb_query_train.py:104-126).  GPU only.

    python scripts/grad_probe.py --n 1000000 --nq 1,16

Prints, per nq, the HIP-event times and the mean-stream rate rows * DP * 4 bytes / time of
each pass as a fraction of the achievable HBM rate (6.3 TB/s), and for comparison the time of
torch autograd through a dense torch restatement of CobwebWrapper.py:283-292 (what a user
would otherwise run) at --torch-n rows on the same GPU.

    python scripts/grad_probe.py --ce --n 1000000 --nq 1,16,256

--ce measures the fused ranking loss instead (cwq_rank_ce), in this one
process: per nq the median [min, max] of --reps alternating runs of (a) rank_scores with grad ->
F.cross_entropy(reduction="sum") -> backward, (b) rank_ce with its gradient, (c) the
forward-only pair, and the peak of torch.cuda.max_memory_allocated() across (a) and across (b).

    python scripts/grad_probe.py --lw --n 1000000 --nq 1,16,256

--lw measures the call-time level weights (cwq_rank_ce_w), paths taking turns
in this one process: (a) rank_ce with grad_q only (the index's own weights), (b) rank_ce with
call-time weights and grad_q, (c) the same with grad_q and grad_w, (d) / (e) the forward-only
calls without and with call-time weights.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes/s, streaming reads


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def torch_dense(fs, Q, n, reps):
    """fwd + bwd of the reference expression in torch on the GPU, flat tree of n leaves, one
    query at a time as cobweb_rank_scores is called."""
    M = fs["mean"][:n + 1].contiguous()
    V = torch.as_tensor(fs["var"])[:n + 1].to(M.device).contiguous()
    logdet = torch.log(V).sum(dim=1)

    def step(nq):
        for b in range(nq):
            x = Q[b].clone().requires_grad_()
            lp = -0.5 * (logdet + (((x.unsqueeze(0) - M) ** 2) / V).sum(dim=1))
            scores = 0.5 * lp[0] + 0.5 * lp[1:]       # path matrix of a flat tree: 1/2 root, 1/2 leaf
            scores.sum().backward()
    return {nq: event_ms(lambda: step(nq), reps) for nq in (1, 16)}


def event_all(fns, reps):
    """Per function (median, min, max) of reps HIP-event timings, the functions taking turns
    inside every repetition (drift of the box hits them alike), after one warm-up call each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def peak_mb(fn):
    """Peak of torch's allocator over one call of fn, above what is allocated before it (the
    library's own workspace is not torch memory: reported separately)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ce_probe(ix, Q, nqs, reps, T, tag):
    """--ce: the training step's loss through (a) rank_scores with grad -> F.cross_entropy ->
    backward, (b) the fused rank_ce with its gradient, and (c) rank_ce forward only against
    rank_scores + a count of the scores above the target's; peak torch memory of (a) and (b)."""
    F = torch.nn.functional
    dev = ix.device
    gen = torch.Generator(device=dev).manual_seed(7)
    for nq in nqs:
        q = Q[:nq].contiguous()
        labels = torch.randint(0, ix.n_sent, (nq,), device=dev, generator=gen)

        def a():
            x = q.clone().requires_grad_()
            F.cross_entropy(ix.rank_scores(x) / T, labels, reduction="sum").backward()
            return x.grad

        def b():
            return ix.rank_ce(q, labels, T, grad=True)

        def c_old():
            s = ix.rank_scores(q)
            return (s > s.gather(1, labels[:, None])).sum(1)

        def c_new():
            return ix.rank_ce(q, labels, T)

        ga, (lb, gb, _, rb) = a(), b()
        rel = float(((ga - gb).double().norm(dim=1) / ga.double().norm(dim=1)).max())
        assert bool((c_old() + 1 <= rb).all())   # the count above, plus ties before the target
        ta, tb, tco, tcn = event_all((a, b, c_old, c_new), reps)
        # the unfused path's spread and the fused path's, each as (max - min) / median
        spread = max((ta[2] - ta[1]) / ta[0], (tb[2] - tb[1]) / tb[0])
        verdict = "neutral (within the spread)" if abs(ta[0] - tb[0]) <= spread * ta[0] else \
            ("fused faster" if tb[0] < ta[0] else "FUSED SLOWER")
        pa, pb = peak_mb(a), peak_mb(b)
        print(f"rank_ce {tag} nq={nq} T={T:g}: (a) rank_scores+cross_entropy fwd+bwd {ta[0]:.3f} ms "
              f"[{ta[1]:.3f}, {ta[2]:.3f}]  (b) rank_ce fwd+bwd {tb[0]:.3f} ms [{tb[1]:.3f}, {tb[2]:.3f}]  "
              f"b/a {tb[0] / ta[0]:.3f}, spread {spread:.1%}: {verdict}", flush=True)
        print(f"rank_ce {tag} nq={nq}: (c) forward only: rank_scores + count {tco[0]:.3f} ms "
              f"[{tco[1]:.3f}, {tco[2]:.3f}]  rank_ce {tcn[0]:.3f} ms [{tcn[1]:.3f}, {tcn[2]:.3f}]", flush=True)
        print(f"rank_ce {tag} nq={nq}: peak torch memory above the inputs (a) {pa:.1f} MiB  (b) {pb:.3f} MiB; "
              f"grad (a) vs (b) max rel L2 {rel:.3g}", flush=True)


def lw_probe(ix, Q, nqs, reps, T, tag):
    """--lw: what call-time level weights and their gradient add to a rank_ce training step."""
    dev = ix.device
    gen = torch.Generator(device=dev).manual_seed(7)
    w = torch.ones(ix.info["max_depth"] + 1, device=dev)
    for nq in nqs:
        q = Q[:nq].contiguous()
        labels = torch.randint(0, ix.n_sent, (nq,), device=dev, generator=gen)
        fns = (lambda: ix.rank_ce(q, labels, T, grad=True),
               lambda: ix.rank_ce(q, labels, T, grad=True, level_weights=w),
               lambda: ix.rank_ce(q, labels, T, grad=True, level_weights=w, weight_grad=True),
               lambda: ix.rank_ce(q, labels, T),
               lambda: ix.rank_ce(q, labels, T, level_weights=w))
        a, b, c = fns[0](), fns[1](), fns[2]()
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, c[:4]))
        assert torch.equal(c[4], fns[2]()[4])
        ta, tb, tc, td, te = event_all(fns, reps)
        spread = max((t[2] - t[1]) / t[0] for t in (ta, tb, tc))
        print(f"lweight {tag} nq={nq}: (a) rank_ce grad_q {ta[0]:.3f} ms [{ta[1]:.3f}, {ta[2]:.3f}]  "
              f"(b) + call-time weights {tb[0]:.3f} ms [{tb[1]:.3f}, {tb[2]:.3f}]  "
              f"(c) + grad_w {tc[0]:.3f} ms [{tc[1]:.3f}, {tc[2]:.3f}]  b/a {tb[0] / ta[0]:.3f}  c/a {tc[0] / ta[0]:.3f}  "
              f"spread {spread:.1%}", flush=True)
        print(f"lweight {tag} nq={nq}: forward only (d) baked weights {td[0]:.3f} ms [{td[1]:.3f}, {td[2]:.3f}]  "
              f"(e) call-time weights {te[0]:.3f} ms [{te[1]:.3f}, {te[2]:.3f}]  e/d {te[0] / td[0]:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", default="1,16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--torch-n", type=int, default=100_000)
    ap.add_argument("--ce", action="store_true", help="the fused ranking loss (rank_ce) against rank_scores + "
                    "torch cross_entropy, in this one process")
    ap.add_argument("--lw", action="store_true", help="call-time level weights and their gradient (rank_ce_w) "
                    "against rank_ce, in this one process")
    ap.add_argument("--temperature", type=float, default=0.0, help="--ce / --lw: 0 = the standard deviation of the "
                    "first query's scores")
    args = ap.parse_args()
    pkg = cobweb_pkg.load()
    dev = torch.device("cuda", 0)
    X = pkg.synth.synthetic_corpus(args.n, args.dim, seed=0, device=dev)
    fs = pkg.synth.flat_synth(X)
    nqs = [int(v) for v in args.nq.split(",")]
    Q, _ = pkg.synth.synthetic_queries(X, max(max(nqs), 16), seed=1)
    del X
    if args.ce or args.lw:
        ix = pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"], device=dev)
        del fs
        torch.cuda.empty_cache()
        T = args.temperature or float(ix.rank_scores(Q[:1]).std())
        (ce_probe if args.ce else lw_probe)(ix, Q, nqs, args.reps, T, f"n={args.n} d={args.dim}")
        print("done", flush=True)
        return
    tn = min(args.torch_n, args.n)
    tt = torch_dense(fs, Q, tn, 3)
    ix = pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"], device=dev)
    del fs
    torch.cuda.empty_cache()
    rows = ix.info["leaf_rows"] + ix.info["internal_nodes"]
    dp = (args.dim + 31) // 32 * 32
    stream = rows * dp * 4
    for nq in nqs:
        q = Q[:nq].contiguous()
        G = torch.randn((nq, ix.n_sent), device=dev)
        f = event_ms(lambda: ix.rank_scores(q), args.reps)
        b = event_ms(lambda: ix.rank_scores_backward(q, G), args.reps)
        assert torch.equal(ix.rank_scores_backward(q, G), ix.rank_scores_backward(q, G))

        def both():
            x = q.clone().requires_grad_()
            ix.rank_scores(x).backward(G)
        fb = event_ms(both, args.reps)
        print(f"grad n={args.n} d={args.dim} nq={nq}: forward {f:.3f} ms ({stream / f / 1e9:.2f} TB/s, "
              f"{stream / (f * 1e-3) / HBM_ACHIEVABLE:.0%} of 6.3)  backward {b:.3f} ms "
              f"({stream / b / 1e9:.2f} TB/s, {stream / (b * 1e-3) / HBM_ACHIEVABLE:.0%} of 6.3)  "
              f"autograd fwd+bwd {fb:.3f} ms  mean stream {stream / 1e9:.2f} GB", flush=True)
    for nq, ms in tt.items():
        print(f"torch dense restatement n={tn} d={args.dim} nq={nq} (one query per call): fwd+bwd {ms:.3f} ms",
              flush=True)
    print("done", flush=True)


if __name__ == "__main__":
    main()
