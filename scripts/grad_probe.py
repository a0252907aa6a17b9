"""Differentiable rank_scores timing: forward (cwq_rank_scores) and backward
(cwq_rank_scores_backward) over the flat-synth C3 tree (1M x 768) for nq = 1 and 16, like a
training step through cobweb_rank_scores (CobwebWrapper.py:267-294,
src/training/cobweb_query_train.py:104-126).  GPU only.

    python scripts/grad_probe.py --n 1000000 --nq 1,16

Prints, per nq, the HIP-event times and the mean-stream rate rows * DP * 4 bytes / time of
each pass as a fraction of the achievable HBM rate (6.3 TB/s), and for comparison the time of
torch autograd through a dense torch restatement of CobwebWrapper.py:283-292 (what a user
would otherwise run) at --torch-n rows on the same GPU.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", default="1,16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--torch-n", type=int, default=100_000)
    args = ap.parse_args()
    pkg = cobweb_pkg.load()
    dev = torch.device("cuda", 0)
    X = pkg.synth.synthetic_corpus(args.n, args.dim, seed=0, device=dev)
    fs = pkg.synth.flat_synth(X)
    nqs = [int(v) for v in args.nq.split(",")]
    Q, _ = pkg.synth.synthetic_queries(X, max(max(nqs), 16), seed=1)
    del X
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
