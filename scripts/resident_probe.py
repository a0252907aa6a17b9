"""The incremental cycle, default against resident: a small add into a large tree, then a
query (CobwebWrapper.add_sentences -> build_prediction_index -> cobweb_predict_fast,
CobwebWrapper.py:52-89, 210-265).  GPU only.

    python scripts/resident_probe.py --n 100000          # bench.py's hier corpus (C2 shape)
    python scripts/resident_probe.py --n 10000           # a quick run

Builds the tree once over synth.clustered_corpus (n x 768, 100 clusters: the corpus of
bench.py's hier leg), makes a default and a resident wrapper of it in this process, and times
--reps rounds of add_sentences(16 rows) + build_prediction_index() + one
cobweb_predict_fast on each, alternating.  The default call is broken down by wrapping its
steps (host flatten, cwq_fit_create + cwq_fit_load, cwq_fit_insert, cwq_fit_export + node
rebuild, CobwebTree.flatten, CobwebIndex); the resident call by ResidentTree.stats.  Then
cwq_fit_flatten alone: its time, the bytes it moves (mean + meanSq read, meanSq read again
for the nodes that keep a variance row, mean + an_var written) as a fraction of the
achievable HBM rate (6.3 TB/s), and the device memory held while the pool, the BFS copy and
the index coexist.
"""
import argparse
import ctypes
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # bytes/s


class Clock:
    """Wall seconds per named step, GPU drained at both ends of a step."""

    def __init__(self):
        self.t = {}

    def wrap(self, name, fn):
        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                torch.cuda.synchronize()
                self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return timed

    def take(self):
        out, self.t = self.t, {}
        return out


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=100)
    ap.add_argument("--add", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--synthetic", type=int, default=0, metavar="NODES",
                    help="only cwq_fit_flatten, on a made-up tree of about NODES nodes (fan-out 8, random "
                         "statistics, count-1 leaves) loaded into a handle: for a kernel trace of the flatten")
    args = ap.parse_args()
    pkg = cobweb_pkg.load()
    if args.synthetic:
        return flatten_alone(pkg, synthetic_tree(pkg, args.synthetic, args.dim), args.dim, args.reps)
    fit, tree_mod, index_mod = pkg.fit, pkg.tree, pkg.index
    L = pkg.lib()
    n, D = args.n, args.dim
    X, Qn, _ = pkg.synth.clustered_corpus(n, D, args.clusters, 8)
    rng = np.random.default_rng(11)          # the rows added later: new points near corpus rows
    m = args.add * (args.reps + 1)
    extra = (X[rng.choice(n, m, replace=False)] + 0.2 * rng.standard_normal((m, D))).astype(np.float32)
    random.seed(2)
    t0 = time.perf_counter()
    wd = pkg.CobwebWrapper(corpus=[f"p{i}" for i in range(n)], corpus_embeddings=X)
    torch.cuda.synchronize()
    print(f"tree: {n} x {D} clustered rows ({args.clusters} clusters) inserted in {time.perf_counter() - t0:.1f} s")
    free0, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    wr = pkg.CobwebWrapper.from_tree(wd.tree, wd.sentences, resident=True)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    pool_bytes = free0 - free1
    print(f"resident wrapper loaded from the host tree in {time.perf_counter() - t0:.2f} s; pool "
          f"{wr.resident_tree.stats['cap_nodes']} slots, {pool_bytes / 1e9:.2f} GB of device memory")

    # the default path's steps, wrapped
    ck = Clock()
    F = fit.DeviceTreeFitter
    F._flatten = ck.wrap("host flatten (DeviceTreeFitter._flatten)", F._flatten)
    F._rebuild = ck.wrap("node rebuild (_rebuild)", F._rebuild)
    tree_mod.CobwebTree.flatten = ck.wrap("index flatten (CobwebTree.flatten)", tree_mod.CobwebTree.flatten)
    index_mod.CobwebIndex.__init__ = ck.wrap("upload + cwq_index_create", index_mod.CobwebIndex.__init__)
    for sym, name in (("cwq_fit_create", "upload (cwq_fit_create + cwq_fit_load)"),
                      ("cwq_fit_load", "upload (cwq_fit_create + cwq_fit_load)"),
                      ("cwq_fit_insert", "insert kernel (cwq_fit_insert)"),
                      ("cwq_fit_export", "export (cwq_fit_export)")):
        setattr(L, sym, ck.wrap(name, getattr(L, sym)))

    q = Qn[0]
    rows = {False: [], True: []}
    parts = {False: [], True: []}
    answers = {False: [], True: []}
    second = {False: [], True: []}
    for rep in range(args.reps + 1):          # round 0 warms both paths
        batch = extra[rep * args.add:(rep + 1) * args.add]
        names = [f"x{rep}_{i}" for i in range(len(batch))]
        state = random.getstate()
        for resident, w in ((False, wd), (True, wr)):
            random.setstate(state)            # both paths draw the same random() stream
            before = dict(w.resident_tree.stats) if resident else None
            ck.take()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w.add_sentences(names, batch)
            t1 = time.perf_counter()
            w.build_prediction_index()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ans = w.cobweb_predict_fast(q, 10, return_ids=True)
            t3 = time.perf_counter()
            w.cobweb_predict_fast(Qn[1], 10, return_ids=True)     # a second query of the same index
            t4 = time.perf_counter()
            if resident:
                after = w.resident_tree.stats
                p = {"insert kernel (cwq_fit_insert)": after["kernel_s"] - before["kernel_s"],
                     "index from the handle (cwq_index_create_from_fit)": after["index_build_s"] - before["index_build_s"]}
                ck.take()
            else:
                p = ck.take()
            if rep:
                rows[resident].append((t1 - t0, t2 - t1, t3 - t2))
                second[resident].append(t4 - t3)
                parts[resident].append(p)
            answers[resident].append(ans)
    assert answers[False] == answers[True], "the two paths answered differently"
    for resident in (False, True):
        r = rows[resident]
        tot = [sum(x) for x in r]
        print(f"\nresident={resident}: add_sentences({args.add}) + build_prediction_index + cobweb_predict_fast, "
              f"median of {len(r)}: {med(tot) * 1e3:.1f} ms [min {min(tot) * 1e3:.1f}, max {max(tot) * 1e3:.1f}]")
        print(f"  add {med([x[0] for x in r]) * 1e3:.1f} ms, index build {med([x[1] for x in r]) * 1e3:.1f} ms, "
              f"query {med([x[2] for x in r]) * 1e3:.2f} ms (a second query of the same index, not in the sum: "
              f"{med(second[resident]) * 1e3:.2f} ms)")
        for key in parts[resident][0]:
            print(f"    {key}: {med([p.get(key, 0.0) for p in parts[resident]]) * 1e3:.1f} ms")
    td, tr = med([sum(x) for x in rows[False]]), med([sum(x) for x in rows[True]])
    print(f"\ndefault / resident: {td / tr:.1f}x")

    ix_bytes = wr._index.info["device_bytes"]
    flat_bytes = flatten_alone(pkg, wr.resident_tree, D, args.reps)
    print(f"  device memory while the pool, the BFS copy and the index coexist: pool {pool_bytes / 1e9:.2f} GB + "
          f"flatten arrays {flat_bytes / 1e9:.2f} GB (its scratch included) + index {ix_bytes / 1e9:.2f} GB = "
          f"{(pool_bytes + flat_bytes + ix_bytes) / 1e9:.2f} GB")


def synthetic_tree(pkg, nodes, D, fan=8):
    """A resident tree of about `nodes` nodes: every internal node has `fan` children; random
    means, random meanSq on internal nodes, count-1 leaves with meanSq = 0."""
    rng = np.random.default_rng(0)
    n_int = max(1, (nodes - 1) // fan)
    Nn = 1 + n_int * fan
    parent = np.concatenate([[-1], np.repeat(np.arange(n_int), fan)]).astype(np.int32)   # BFS = slot order
    child_ptr = np.minimum(np.arange(Nn + 1, dtype=np.int64) * fan, Nn - 1).astype(np.int32)
    child_idx = np.arange(1, Nn, dtype=np.int32)
    count = np.where(np.arange(Nn) < n_int, 9.0, 1.0).astype(np.float32)
    mean = rng.standard_normal((Nn, D), dtype=np.float32)
    m2 = rng.random((Nn, D), dtype=np.float32)
    m2[n_int:] = 0
    leaves = np.arange(n_int, Nn)
    return pkg.resident.ResidentTree.from_slots(parent, child_ptr, child_idx, count, mean, m2, 0,
                                                {int(s): [i] for i, s in enumerate(leaves)}, len(leaves))


def flatten_alone(pkg, rt, D, reps):
    """cwq_fit_flatten's own time, bytes and rate; returns the device bytes it held."""
    L = pkg.lib()
    sos = rt._sos[:rt.n_sent]
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ts, tf, o = [], [], np.zeros(8, np.int64)
    for _ in range(reps + 1):
        fl = ctypes.c_void_p()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.cwq_fit_flatten(rt._h, ctypes.c_void_p(sos.data_ptr()), rt.n_sent, sp, ctypes.byref(fl))
        ts.append(time.perf_counter() - t0)
        assert rc == 0, L.cwq_fit_last_error()
        L.cwq_fit_flat_info(fl, o.ctypes.data_as(ctypes.c_void_p))
        t0 = time.perf_counter()
        L.cwq_fit_flat_destroy(fl)
        tf.append(time.perf_counter() - t0)
    Nn, n_an, depth, flat_bytes = int(o[0]), int(o[1]), int(o[4]), int(o[6])
    moved = 4 * D * (2 * Nn + n_an) + 4 * D * (Nn + n_an)
    t = med(ts[1:])
    print(f"\ncwq_fit_flatten alone (the call: {5 * depth + 12} launches, {depth + 3} small readbacks, its "
          f"allocations): {t * 1e3:.2f} ms for {Nn} nodes ({n_an} with a variance row), {depth} levels")
    print(f"  bytes moved {moved / 1e9:.3f} GB -> {moved / t / 1e12:.2f} TB/s = "
          f"{100 * moved / t / HBM_ACHIEVABLE:.0f}% of the achievable HBM rate ({HBM_ACHIEVABLE / 1e12} TB/s)")
    print(f"  freeing its arrays afterwards (cwq_fit_flat_destroy): {med(tf[1:]) * 1e3:.2f} ms")
    st = rt.stats
    print(f"  resident tree: {st['slots_in_use']} slots in use, {st['removed_slots']} removed by splits, "
          f"{st['grows']} grows, capacity {st['cap_nodes']}")
    return flat_bytes


if __name__ == "__main__":
    main()
