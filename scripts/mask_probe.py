"""Masked Fast top-k probe: what each path of cwq_score_topk_masked costs by
allowed fraction, mask shape and batch size, beside the unmasked call and beside what a caller
did before (rank_scores -> masked_fill -> torch.topk in blocks of 256 queries).

    python scripts/mask_probe.py [--n 1000000] [--dim 768] [--k 10] [--nq 1,16,10000]

Shape: C3, the flat-synth tree bench.py builds.  Per cell (fraction f, random / contiguous mask,
nq): the masked call under CWQ_MASK_PATH = 1 (over-fetch first), 2 (gathered scan), 0 (the
rule), the unmasked call at k and at k' = 64, and the time of sentence_mask.  Timed with events
around warm calls, the arms interleaved in one process; every arm's ids and scores are compared
with the others' here.  Prints one line per cell and a summary of the rule against the better
forced arm."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cobweb_pkg  # noqa: E402


def timed(fn, reps):
    """Median / min / max milliseconds of `reps` warm calls (one untimed call first)."""
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return out, statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", default="1,16,10000")
    ap.add_argument("--fractions", default="1,0.9,0.5,0.35,0.2,0.1,0.01,0.001")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ksweep", default="10,16,17,20,24,28,32,40,48,56,64")
    a = ap.parse_args()
    pkg = cobweb_pkg.load()
    N, D, k = a.n, a.dim, a.k
    X = pkg.synth.synthetic_corpus(N, D, seed=0)
    t = pkg.synth.flat_synth(X, compact=True)
    ix = pkg.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
    del t
    print(f"# mask_probe: flat {N} x {D}, top-{k}, build {pkg.lib().cwq_build_id().decode()}, "
          f"{torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rule_worst = 0.0
    spread_worst = 0.0
    for nq in [int(v) for v in a.nq.split(",")]:
        Q, _ = pkg.synth.synthetic_queries(X, nq, seed=100 + nq)
        reps = a.reps if nq <= 64 else max(3, a.reps // 2 + 1)
        os.environ.pop("CWQ_MASK_PATH", None)
        _, t_k, lo, hi = timed(lambda: ix.score_topk(Q, k), reps)
        _, t_64, lo64, hi64 = timed(lambda: ix.score_topk(Q, 64), reps)
        print(f"nq={nq:6d} unmasked: k={k} {t_k:9.3f} ms [{lo:.3f}, {hi:.3f}]   k=64 {t_64:9.3f} ms [{lo64:.3f}, {hi64:.3f}]")
        # what the over-fetch leg costs by its k': the unmasked call at each
        sweep = []
        for kp in [int(v) for v in a.ksweep.split(",") if v]:
            _, med, lo, hi = timed(lambda: ix.score_topk(Q, kp), reps)
            sweep.append(f"k'={kp} {med:.3f} [{lo:.3f}, {hi:.3f}]")
        print(f"nq={nq:6d} unmasked by k' (ms): " + "  ".join(sweep))
        for f in [float(v) for v in a.fractions.split(",")]:
            for kind in (("random",) if f >= 1 else ("random", "block")):
                n_allow = max(1, int(round(f * N)))
                flags = torch.zeros(N, dtype=torch.bool, device="cuda")
                if f >= 1:
                    flags[:] = True
                elif kind == "random":
                    flags[torch.randperm(N, generator=g, device="cuda")[:n_allow]] = True
                else:
                    s0 = (N - n_allow) // 3
                    flags[s0:s0 + n_allow] = True
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = ix.sentence_mask(flags)
                t_mask = (time.perf_counter() - t0) * 1e3
                res, tm, st = {}, {}, {}
                for p in (1, 2, 0):   # interleaved: every arm is timed inside the same cell
                    os.environ["CWQ_MASK_PATH"] = str(p)
                    res[p], med, lo, hi = timed(lambda: ix.score_topk(Q, k, mask=m), reps)
                    tm[p] = (med, lo, hi)
                    st[p] = ix.last_mask_stats()
                os.environ.pop("CWQ_MASK_PATH", None)
                for p in (2, 0):
                    assert torch.equal(res[p][0], res[1][0]) and torch.equal(res[p][1], res[1][1]), (nq, f, kind, p)
                live = m.info["live_iso_rows"] + m.info["live_aniso_rows"]
                best = min(tm[1][0], tm[2][0])
                spread = max((tm[p][2] - tm[p][1]) / tm[p][0] for p in (1, 2, 0))
                rule_worst = max(rule_worst, tm[0][0] / best - 1.0)
                spread_worst = max(spread_worst, spread)
                t2 = tm[2][0] * 1e-3
                print(f"nq={nq:6d} f={f:<6g} {kind:6s} live={live:8d} mask={t_mask:7.2f} ms | "
                      f"path1 {tm[1][0]:9.3f} [{tm[1][1]:.3f}, {tm[1][2]:.3f}] k'={st[1]['overfetch_k']} redone={st[1]['redone_queries']} | "
                      f"path2 {tm[2][0]:9.3f} [{tm[2][1]:.3f}, {tm[2][2]:.3f}] | "
                      f"auto {tm[0][0]:9.3f} [{tm[0][1]:.3f}, {tm[0][2]:.3f}] took {st[0]['path']} | "
                      f"gathered: {live * nq / t2 / 1e9:8.2f} G row-queries/s, "
                      f"{live * D * 4 / t2 / 1e9:8.1f} GB/s rows once, "
                      f"{live * D * 4 * ((nq + 63) // 64) / t2 / 1e9:9.1f} GB/s per query block")
                # the baseline a caller had before, once per batch size (its cost does not depend on f)
                if f == 0.5 and kind == "random":
                    def baseline():
                        ids, sc = [], []
                        for q0 in range(0, nq, 256):
                            s = ix.rank_scores(Q[q0:q0 + 256]).masked_fill_(~flags, float("-inf"))
                            v, i = torch.topk(s, k, dim=1)
                            ids.append(i)
                            sc.append(v)
                        return torch.cat(ids), torch.cat(sc)
                    torch.cuda.reset_peak_memory_stats()
                    base0 = torch.cuda.memory_allocated()
                    (bi, bs), tb, lo, hi = timed(baseline, 2)
                    peak = torch.cuda.max_memory_allocated() - base0
                    assert torch.equal(bs, res[1][1]), "baseline scores differ"
                    print(f"nq={nq:6d} baseline rank_scores -> masked_fill -> topk (blocks of 256): {tb:9.3f} ms "
                          f"[{lo:.3f}, {hi:.3f}], peak torch memory {peak / 2 ** 20:.0f} MiB (scores equal)")
                m.close()
    print(f"# rule vs the better forced arm: worst excess {100 * rule_worst:.1f}%; "
          f"worst run-to-run spread of an arm (max - min over median) {100 * spread_worst:.1f}%")


if __name__ == "__main__":
    main()
