"""categorize over several workspace chunks against the same call in one chunk.  GPU only.

    python scripts/cat_chunk_probe.py

A device-ifit tree of 40 Gaussian clusters (20,000 x 64, the tree of
tests/test_gpu_cat_count.py) and 600 queries: under CWQ_WS_BUDGET_MB=1 the call runs in chunks
of 256, 256 and 88 queries with the filter and of 128 without, so later chunks' queries go
through the gathered two-level replay (default) or the DENSE re-run (CWQ_CAT_TWO=0) at q0 > 0.
For set_filter(-1) and (0), (k, max_nodes) in (10, 100000), (64, 100000), (10, 40), default knobs
and CWQ_CAT_TWO=0 it prints whether nodes, n_found and n_calls are torch.equal to the
single-chunk call, a hash of the chunked results (run with PYTHONHASHSEED=0 to compare two
builds) and both calls' stats.  At k = 64 = the list length the two-level replay certifies no
query (two_level 0, every query DENSE), so this is a measurement, not a test.  Exit status 1
on a mismatch.  CWQ_CAT_DIRECT=0 as in the tests (the list paths)."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402


def run(ix, Q, k, mx, **env):
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        out = ix.categorize(Q, k, mx)
        torch.cuda.synchronize()
        return out, ix.last_categorize_stats()
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v


def main():
    pkg = cobweb_pkg.load()
    os.environ["CWQ_CAT_DIRECT"] = "0"
    bad = 0
    for filt in (-1, 0):
        rng = np.random.default_rng(5)
        n, d, nc = 20_000, 64, 40
        C = rng.standard_normal((nc, d)).astype(np.float32) * 2.0
        X = (C[rng.integers(0, nc, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
        random.seed(5)
        w = pkg.CobwebWrapper(corpus=None, corpus_embeddings=X)
        w.build_prediction_index()
        ix = w._index
        ix.set_filter(filt)
        Qn = np.concatenate([X[:450] + 0.05 * rng.standard_normal((450, d)),
                             C[rng.integers(0, nc, 150)] + 0.3 * rng.standard_normal((150, d))]).astype(np.float32)
        Q = torch.from_numpy(Qn).cuda()
        for k, mx in [(10, 100000), (64, 100000), (10, 40)]:
            for env in ({}, {"CWQ_CAT_TWO": "0"}):
                one, st1 = run(ix, Q, k, mx, **env)
                many, st = run(ix, Q, k, mx, CWQ_WS_BUDGET_MB="1", **env)
                eq = all(torch.equal(a, b) for a, b in zip(one, many))
                bad += not eq
                h = hash(tuple(int(x) for t in many for x in t.flatten().cpu().tolist()))
                print(f"filt {filt} k {k} mx {mx} env {env}: equal {eq} hash {h} one {st1} chunked {st}", flush=True)
    print("MISMATCHES", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
