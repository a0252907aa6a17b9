"""Masked ranking-loss probe: what each path of cwq_rank_ce_masked costs by allowed
fraction and batch size, beside the unmasked loss, beside what a caller did before
(rank_scores -> masked_fill -> F.cross_entropy -> backward) and beside the top-K forms.

    python scripts/mask_loss_probe.py [--n 1000000] [--dim 768] [--nq 1,16,256]

Shape: the flat-synth tree bench.py builds.  Per cell (allowed fraction f, nq), loss with
gradient: the masked call under CWQ_MASK_CE_PATH = 1 (full), 2 (gathered) and 0 (the rule), the
torch workaround, cwq_rank_ce unmasked, and the top-K form at K = 64 and K = 10 masked and
unmasked.  Timed with events around warm calls; the arms take turns inside each repetition, in one
process; median of --reps with [min, max].  The paths' loss / score / rank are compared here.
Prints one line per cell and, at the end, the rule against the better forced arm."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cobweb_pkg  # noqa: E402


def interleaved(arms, reps):
    """{name: (median, min, max) ms}: one untimed round, then `reps` rounds of every arm in turn."""
    ts = {k: [] for k in arms}
    for r in range(reps + 1):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                ts[name].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", default="1,16,256")
    ap.add_argument("--fractions", default="1,0.5,0.25,0.1,0.01,0.001")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-torch", action="store_true", help="skip the [nq, n_sent] workaround arm")
    a = ap.parse_args()
    pkg = cobweb_pkg.load()
    N, D = a.n, a.dim
    X = pkg.synth.synthetic_corpus(N, D, seed=0)
    t = pkg.synth.flat_synth(X, compact=True)
    ix = pkg.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
    del t
    print(f"# mask_loss_probe: flat {N} x {D}, loss + grad_q, median of {a.reps} [min, max] ms, build "
          f"{pkg.lib().cwq_build_id().decode()}, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    T = 50.0
    verdicts = []
    for nq in [int(v) for v in a.nq.split(",")]:
        Q, _ = pkg.synth.synthetic_queries(X, nq, seed=11)
        Q = Q.contiguous()
        for f in [float(v) for v in a.fractions.split(",")]:
            flags = torch.ones(N, dtype=torch.bool, device="cuda") if f >= 1 else torch.rand(N, device="cuda", generator=g) < f
            ids = torch.nonzero(flags)[:, 0]
            tg = ids[torch.randint(0, ids.numel(), (nq,), device="cuda", generator=g)]
            m = ix.sentence_mask(flags)
            keep = {}

            def masked(path, tag):
                def fn():
                    os.environ["CWQ_MASK_CE_PATH"] = str(path)
                    keep[tag] = ix.rank_ce(Q, tg, T, grad=True, mask=m)
                return fn

            def workaround():
                q = Q.clone().requires_grad_()
                s = ix.rank_scores(q).masked_fill(~flags, float("-inf"))
                torch.nn.functional.cross_entropy(s / T, tg, reduction="sum").backward()
                keep["torch"] = q.grad

            arms = {"full": masked(1, "full"), "gathered": masked(2, "gathered"), "auto": masked(0, "auto"),
                    "unmasked": lambda: ix.rank_ce(Q, tg, T, grad=True)}
            if not a.no_torch:
                arms["torch"] = workaround
            for K in (64, 10):
                arms[f"top{K}_masked"] = lambda K=K: ix.rank_ce_topk(Q, tg, K, T, grad=True, mask=m)
                arms[f"top{K}_unmasked"] = lambda K=K: ix.rank_ce_topk(Q, tg, K, T, grad=True)
            r = interleaved(arms, a.reps)
            os.environ["CWQ_MASK_CE_PATH"] = "0"
            ix.rank_ce(Q, tg, T, mask=m)
            auto_path = {5: "full", 6: "gathered"}[ix.last_mask_stats()["path"]]
            same = all(torch.equal(keep["full"][i], keep["gathered"][i]) and torch.equal(keep["full"][i], keep["auto"][i])
                       for i in (0, 2, 3))
            gerr = float((keep["gathered"][1] - keep["full"][1]).norm() / keep["full"][1].norm().clamp_min(1e-30))
            cells = "  ".join(f"{k} {v[0]:.3f} [{v[1]:.3f}, {v[2]:.3f}]" for k, v in r.items())
            print(f"nq={nq} f={f:g} live={m.info['live_iso_rows'] + m.info['live_aniso_rows']} auto->{auto_path} "
                  f"loss/score/rank equal={same} grad rel diff {gerr:.2g}  {cells}", flush=True)
            best = min(("full", "gathered"), key=lambda k: r[k][0])
            spread = max(r[best][2] - r[best][1], r["auto"][2] - r["auto"][1])
            verdicts.append((nq, f, auto_path, best, r["auto"][0], r[best][0], spread))
            m.close()
            keep.clear()
    print("# the rule against the better forced arm (ok: auto within the arms' own spread of it)")
    for nq, f, ap_, best, ta, tb, spread in verdicts:
        print(f"# nq={nq} f={f:g}: auto={ap_} {ta:.3f} ms, better forced={best} {tb:.3f} ms, spread {spread:.3f} ms: "
              f"{'ok' if ta - tb <= spread else 'MISS'}")


if __name__ == "__main__":
    main()
