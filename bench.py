"""Benchmark: "Cobweb Fast" batched queries/s on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[2]): synthetic flat-synth tree
over X ~ N(0, I), N = 1,000,000 x D = 768 fp32 (seed 0), 10,000 queries per step per
GPU (half corpus points + 0.1*N(0,I), half fresh N(0,I); seed 1 + rank), k = 10.
A step = one libcwq cwq_score_topk call over the batch (scan + path score + top-k
+ merge + sentence ids), inputs resident in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--preset c1|c2|c3|c4|c5] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run does what the headline figure needs and no more: it builds the tree and the
index, warms up, times the K steps and prints one JSON line (`value` = queries/s,
`ms_per_step` = milliseconds per timed step).  `--dump-outputs DIR` then writes what the
last timed step returned -- the arrays a cwq_score_topk caller receives -- as DIR/ids.npy
(float64) and DIR/scores.npy (float32); the inputs are seeded, so two builds can be
compared output for output.  The other legs, described below, run only with `--full`.

Multi-GPU (the functions of rag-cobweb_amd/dist.py, covered by tests/test_dist.py on
gloo): rank 0 synthesises the tree and `broadcast_tree` sends the frozen node
statistics over RCCL (var compressed to one scalar per isotropic row; timed
separately); `timed_steps` brackets the loop with barrier + sync and takes the max
over ranks.  Preset c3 (default): every rank scans its own 10k-query batch (weak
scaling).  Preset c4 (BASELINE configs[3]): 10M x 1024, 100k queries per step split
over the ranks by `sharded_query` (strong scaling).  No collective in the timed loop.

With `--full`, also reported: `roofline` (HIP-event time of the dominant kernel, in calls of
its own), `recall@10` against exact brute force, `per_call` (the reference harness's
one-query-per-call mode at nq = 1, 8,
64, plus the wrapper's numpy-query Fast and Basic calls: harness_call_nq1,
harness_basic_nq1), `hier` (a device-ifit Cobweb tree over a 100k x 768 clustered corpus:
ifit inserts/s, Fast batch / per call, Basic batch / per call, the filter and pruning
stats; hier_leg) and `cpu_baseline` (the reference op sequence in torch-CPU, all threads +
1 thread).
"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import cobweb_pkg  # noqa: E402

PEAK_FP32_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 vector = FP32 MFMA dense peak
PEAK_BF16_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16 MFMA dense peak (no sparsity)
PEAK_HBM_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PEAK_CLOCK_GHZ = 2.4       # MI355X_MICROARCH.md: max clock (the dense peaks assume it)


def config_label(N, D):
    """Which BASELINE.json config a run measures (SURVEY §8 shorthand)."""
    if (N, D) == (1_000_000, 768):
        return "BASELINE configs[2], C3"
    if (N, D) == (10_000_000, 1024):
        return "BASELINE configs[3], C4 per-GPU shard"
    if (N, D) == (1_500, 384):
        return "BASELINE configs[0] shape, C1 (synthetic stand-in for the QQP embeddings)"
    if (N, D) == (100_000, 768):
        return "BASELINE configs[1] shape, C2 (synthetic stand-in for MS-MARCO 100k)"
    if (N, D) == (8_800_000, 256):
        return "BASELINE configs[4] shape, C5 (synthetic stand-in for whitened MS-MARCO 8.8M)"
    return "custom size"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def cpu_model():
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return platform.processor() or "unknown"


def cpu_baseline(X_host, root_mean, root_var, Q_host, k, sample_all, sample_1t, ids_gpu):
    """The reference's Fast query as its own torch-CPU op sequence (oracle.TorchFastIndex:
    CobwebWrapper.py:222-257 -- diff_sq, log-var sum, (diff_sq/var) sum, sparse.mm over
    the COO path matrix, topk) on the FULL flat-synth tree, one query per call like the
    reference harness (benchmark_utils.py:801-805).  Two legs: all host
    threads this process may use, and 1 thread.  Checker only: the sampled queries' ids
    are compared with the GPU's."""
    from oracle import cobweb_oracle as O
    N, D = X_host.shape
    T = O.TorchFastIndex.flat(root_mean, root_var, X_host)
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    # SURVEY §8(d) asks for len(sched_getaffinity) threads.  The GPU pool gives each
    # one-GPU job a CPU share, exports it as OMP_NUM_THREADS and asks jobs to size their
    # thread pools to it (affinity lists the whole machine's CPUs), so the all-cores leg
    # runs at that share when the variable is set
    n_all = min(aff, omp) if omp > 0 else aff
    cap_reason = (f"capped at the pool's per-job CPU share OMP_NUM_THREADS={omp} (affinity lists {aff} CPUs of "
                  f"the whole machine)" if 0 < omp < aff else f"all {aff} affinity CPUs")
    prev = torch.get_num_threads()
    legs, agree = {}, 0
    for name, threads, sample in (("all", n_all, sample_all), ("1t", 1, sample_1t)):
        if sample <= 0:
            continue
        torch.set_num_threads(threads)
        T.predict(Q_host[0], k)                          # warm-up (allocator, thread pool)
        times = []
        for i in range(sample):
            t = time.perf_counter()
            got = T.predict(Q_host[i % len(Q_host)], k)
            times.append(time.perf_counter() - t)
            if name == "all" and i < len(ids_gpu):
                agree += int(list(got) == list(ids_gpu[i]))
        sec = float(np.mean(times))
        legs[name] = {"threads": threads, "queries": sample, "s_per_query": round(sec, 4),
                      "queries_per_s": round(1.0 / sec, 4)}
    torch.set_num_threads(prev)
    main = legs.get("all") or legs.get("1t")
    return {"value": main["queries_per_s"], "unit": "queries/s", "cores": main["threads"], "kind": "port",
            "sample": f"reference op sequence in torch-CPU (oracle.TorchFastIndex, CobwebWrapper.py:222-257) on the "
                      f"full flat-synth {N}x{D} tree, one query per call; {legs['all']['queries'] if 'all' in legs else 0} "
                      f"queries at {n_all} threads ({cap_reason}) and "
                      f"{legs['1t']['queries'] if '1t' in legs else 0} at 1 thread; CPU: {cpu_model()}; GPU top-{k} "
                      f"identical on {agree}/{min(len(ids_gpu), legs['all']['queries'] if 'all' in legs else 0)}",
            "legs": legs}


def recall_truth(pkg, X, Q, k, n_eval):
    """Exact brute-force top-k (flat-L2 and flat-IP = the reference's FAISS / Torch Dot
    baselines, benchmark_utils.py:536-614), scored in float64
    (harness.brute_force_topk(exact=True)).  Computed before the timed loop so the
    corpus copy can be freed (C4: 41 GB) while the index runs."""
    Qe = Q[:n_eval]
    gt_l2 = pkg.harness.brute_force_topk(X, Qe, k, "l2", exact=True).cpu().numpy()
    gt_ip = pkg.harness.brute_force_topk(X, Qe, k, "ip", exact=True).cpu().numpy()
    return gt_l2, gt_ip


def recall_at_k(gt, ids, targets, k, n_eval):
    """recall@k of the Fast ranking against recall_truth's lists."""
    gt_l2, gt_ip = gt
    got = ids[:n_eval].cpu().numpy()
    r_l2 = np.mean([len(set(a) & set(b)) / k for a, b in zip(got, gt_l2)])
    r_ip = np.mean([len(set(a) & set(b)) / k for a, b in zip(got, gt_ip)])
    tg = targets.cpu().numpy()
    r_tgt = float(np.mean([t in set(row) for t, row in zip(tg, ids[:len(tg)].cpu().numpy())])) if len(tg) else None
    return round(float(r_l2), 4), round(float(r_ip), 4), r_tgt


PRESETS = {
    # BASELINE configs[2] (C3): 10k queries per GPU per step (weak scaling)
    "c3": dict(n=1_000_000, dim=768, queries=10_000, strong=False),
    # BASELINE configs[3] (C4): 10M x 1024, 100k queries split over the ranks (strong scaling)
    "c4": dict(n=10_000_000, dim=1024, queries=100_000, strong=True),
    # the other configs' shapes with N(0,I) stand-ins (no datasets or encoders offline):
    # C1 QQP 1.5k x 384, 300 queries; C2 MS-MARCO 100k x 768, 1k queries; C5 8.8M x 256
    # (PCA-whitened MS-MARCO; 10k queries per GPU per step)
    "c1": dict(n=1_500, dim=384, queries=300, strong=False),
    "c2": dict(n=100_000, dim=768, queries=1_000, strong=False),
    "c5": dict(n=8_800_000, dim=256, queries=10_000, strong=False),
}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, ids, scores, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: the (ids, scores) of the last timed step as DIR/ids.npy (float64: sentence
    ids, exact) and DIR/scores.npy (float32).  A result over `limit` bytes is cut to a fixed
    seeded sample of its query rows (their numbers in DIR/rows.npy)."""
    os.makedirs(dirname, exist_ok=True)
    ids = ids.cpu().numpy().astype(np.float64)
    scores = scores.cpu().numpy().astype(np.float32)
    row_bytes = (ids.nbytes + scores.nbytes + 8 * len(ids)) / max(1, len(ids))
    limit -= 3 * 4096                                      # room for the .npy headers
    if len(ids) * row_bytes > limit:
        rows = np.sort(np.random.default_rng(0).choice(len(ids), int(limit // row_bytes), replace=False))
        ids, scores = ids[rows], scores[rows]
        np.save(os.path.join(dirname, "rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(dirname, "ids.npy"), ids)
    np.save(os.path.join(dirname, "scores.npy"), scores)


def per_call(index, Q, k, nqs=(1, 8, 64), reps=20):
    """The reference harness's mode: one cobweb_predict_fast-sized call at a time with a
    host sync after each (benchmark_utils.py:801-805).  Median us per call; for the
    small-batch stream filter (cwq_stream.hip, nq <= 64) the HBM rate of its pass over
    the row panel: bytes = isotropic rows x (2*DPB bf16, or DPB for the int8 pass, + 32 B row
    constants), divided by the filter launch's HIP-event time, against the 8 TB/s HBM peak."""
    NL, D = index.info["isotropic_rows"], index.dim
    DPB = max(128, -(-D // 64) * 64)                     # fgemm_dpb: whole 64-dim stage pairs
    out = {"bytes_per_pass_bf16": NL * (2.0 * DPB + 32.0), "bytes_per_pass_int8": NL * (1.0 * DPB + 32.0)}
    for nq in nqs:
        q = Q[:nq].contiguous()
        index.score_topk(q, k)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            index.score_topk(q, k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        ts.sort()
        index.set_timing(True)
        tm = []
        for _ in range(5):
            index.score_topk(q, k)
            tm.append(index.last_timing())
        index.set_timing(False)
        st = index.last_stats()
        med = {key: float(np.median([t[key] for t in tm])) for key in tm[0]}
        row = {"us_per_call": round(ts[len(ts) // 2] * 1e6, 1), "queries_per_s": round(nq / ts[len(ts) // 2], 1),
               "path": st["path"], "call_ms_events": round(med["call_ms"], 4)}
        if st["path"] == "stream":
            row["pass"] = "int8" if st["int8_pass"] else "bf16"
            gbs = out["bytes_per_pass_" + row["pass"]] / (med["fgemm_ms"] * 1e-3) / 1e9
            row.update({"stream_filter_ms": round(med["fgemm_ms"], 4), "probe_ms": round(med["sample_ms"], 4),
                        "rerank_ms": round(med["rerank_ms"], 4),
                        "hbm_roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS,
                                         "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4)}})
        out[str(nq)] = row
    return out


def pmc_candidates(explicit):
    """The PMC file to read: the one given, else profiles/pmc_rNN_fgemm.json newest round first
    (the first whose workload and kernel match the run is used)."""
    if explicit:
        return [explicit]
    import glob
    import re
    fs = glob.glob(os.path.join(ROOT, "profiles", "pmc_r*_fgemm.json"))
    return sorted(fs, key=lambda f: int(re.search(r"pmc_r(\d+)_", f).group(1)), reverse=True)


class _Names:
    """Sentence strings "s<i>" of the synthetic corpus, made on demand (no 1M-10M list)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return f"s{i}"


def per_call_harness(pkg, index, Q, k, reps=200, basic=False, node_of_sentence=None):
    """The reference harness's own timed call (benchmark_utils.py:576-579, 801-805):
    `latency = time.time()` around `cobweb.cobweb_predict_fast(query_emb, k)` with a numpy
    query and sentence strings out -- the drop-in CobwebWrapper over this index, so the
    host->device copy of the query, the result sync and the id -> sentence mapping
    (wrapper.cobweb_predict_indexed) are inside the time.  basic=True times "Cobweb Basic"
    instead (benchmark_utils.py:580-581: `cobweb.cobweb_predict(query_emb, k)`, best-first
    categorize, wrapper.cobweb_predict) over the same tree."""
    w = pkg.CobwebWrapper.from_index(index, _Names(index.n_sent), node_of_sentence=node_of_sentence)
    fn = w.cobweb_predict if basic else w.cobweb_predict_fast
    Qh = Q[:reps].cpu().numpy()
    fn(Qh[0], k)
    ts = []
    for i in range(reps):
        t = time.perf_counter()
        fn(Qh[i], k)
        ts.append(time.perf_counter() - t)
    ts.sort()
    name = "cobweb_predict" if basic else "cobweb_predict_fast"
    out = {"call": f"CobwebWrapper.{name}(numpy_query, k) -> list of sentences",
           "queries": reps, "us_per_call_median": round(ts[reps // 2] * 1e6, 1),
           "us_per_call_p10": round(ts[reps // 10] * 1e6, 1), "us_per_call_mean": round(float(np.mean(ts)) * 1e6, 1),
           "queries_per_s": round(reps / float(np.sum(ts)), 1)}
    if basic:
        # where the call's time goes: the search itself (cwq_categorize_host, host query in,
        # node ids out) and the wrapper's advance of Python's global `random` stream by the
        # reference's draw count (one random() per log_prob call and per retrieval,
        # CobwebTorchTree.py:243,268,285 -- a million on this flat tree)
        import random as _random
        tc, tr = [], []
        for i in range(reps):
            t = time.perf_counter()
            _, found, calls = index.categorize_host(Qh[i:i + 1], k, w.max_init_search)
            tc.append(time.perf_counter() - t)
            st = _random.getstate()
            t = time.perf_counter()
            pkg.wrapper.advance_random(int(calls[0]) + int(found[0]))
            tr.append(time.perf_counter() - t)
            _random.setstate(st)
        tc.sort()
        tr.sort()
        out["categorize_host_us_median"] = round(tc[reps // 2] * 1e6, 1)
        out["rng_advance_us_median"] = round(tr[reps // 2] * 1e6, 1)
        out["log_prob_calls_per_query"] = int(calls[0])
    return out


def hier_leg(pkg, n=100_000, dim=768, n_clusters=100, nq=1000, k=10, calls=100):
    """A real-shaped Cobweb tree in the driver's record (BASELINE configs[1]'s shape, C2):
    the drop-in's own device ifit over the clustered stand-in corpus (synth.clustered_corpus,
    the corpus of tests/test_gpu_c2.py) -- the reference's workflow, CobwebWrapper(corpus,
    embeddings) (CobwebWrapper.py:13-80 via benchmark_utils.py:438-467) then
    build_prediction_index and queries (benchmark_utils.py:576-581, 801-805).  Reports the
    ifit inserts/s and tree shape, the tree-adaptive cut, Fast batch q/s with its filter and
    pruning stats (ids and scores checked against the exact scan), Fast per call (nq = 1, 8,
    64, and the harness's cobweb_predict_fast(numpy, k)), Basic batch q/s and the harness's
    cobweb_predict(numpy, k).  Not the headline `value` (a 1,000-query batch on a 100k tree)."""
    import random as _random
    X, Qn, pick = pkg.synth.clustered_corpus(n, dim, n_clusters, nq)
    _random.seed(2)
    w0 = pkg.CobwebWrapper(corpus=None, corpus_embeddings=X[:8])   # libcwq warm (fitter kernels loaded)
    w0.build_prediction_index()
    torch.cuda.synchronize()
    _random.seed(2)
    t0 = time.perf_counter()
    w = pkg.CobwebWrapper(corpus=[f"p{i}" for i in range(n)], corpus_embeddings=X)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    w.build_prediction_index()
    torch.cuda.synchronize()
    t_ix = time.perf_counter() - t0
    ix = w._index
    inf = ix.info
    out = {"workload": f"device-ifit Cobweb tree over {n}x{dim} clustered embeddings ({n_clusters} Gaussian clusters, "
                       f"synth.clustered_corpus seed 2), {nq} queries, k={k} (BASELINE configs[1] shape, C2)",
           "ifit_s": round(t_fit, 2), "ifit_inserts_per_s": round(n / t_fit, 1), "index_build_s": round(t_ix, 3),
           "tree": {"nodes": inf["n_nodes"], "internal": inf["internal_nodes"], "max_depth": inf["max_depth"],
                    "root_children": len(w.tree.root.children)},
           "cut": ix.cut_info(), "filter_rows": ix.filter_info()}
    Q = torch.from_numpy(Qn).cuda()

    def med(f, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        ts.sort()
        return ts[len(ts) // 2]

    ix.set_filter(0)
    ids0, s0 = ix.score_topk(Q, k)
    t_scan = med(lambda: ix.score_topk(Q, k), 5)
    ix.set_filter(-1)
    ids1, s1 = ix.score_topk(Q, k)
    t_fast = med(lambda: ix.score_topk(Q, k), 11)
    st, ps = ix.last_stats(), ix.last_prune_stats()
    out["fast_batch"] = {"ms": round(t_fast * 1e3, 3), "queries_per_s": round(nq / t_fast, 1),
                         "exact_scan_ms": round(t_scan * 1e3, 3),
                         "equal_to_exact_scan": bool(torch.equal(ids0, ids1) and torch.equal(s0, s1)),
                         "filter": {k_: st[k_] for k_ in ("filter_used", "fallback_queries", "candidates",
                                                          "exact_reranks")},
                         "prune": ps,
                         "perturbed_row_first": round(float((ids1[:len(pick), 0].cpu().numpy() == pick).mean()), 4)}
    pc = {}
    for m in (1, 8, 64):
        qs = [Q[i:i + m].contiguous() for i in range(0, min(nq, calls * m), m)][:calls]
        same = all(torch.equal(ix.score_topk(q, k)[0], ids0[i * m:i * m + m]) for i, q in enumerate(qs[:10]))
        ts = []
        for q in qs:
            t = time.perf_counter()
            ix.score_topk(q, k)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        ts.sort()
        pc[str(m)] = {"us_per_call": round(ts[len(ts) // 2] * 1e6, 1), "path": ix.last_stats()["path"],
                      "equal_to_exact_scan": bool(same)}
    out["fast_per_call"] = pc
    ts = []
    for i in range(calls):
        t = time.perf_counter()
        w.cobweb_predict_fast(Qn[i % nq], k)
        ts.append(time.perf_counter() - t)
    ts.sort()
    out["harness_call_nq1_us"] = round(ts[len(ts) // 2] * 1e6, 1)
    nodes, found, ncalls = ix.categorize(Q, k, w.max_init_search)
    t_b = med(lambda: ix.categorize(Q, k, w.max_init_search), 5)
    out["basic_batch"] = {"ms": round(t_b * 1e3, 3), "queries_per_s": round(nq / t_b, 1),
                          "found_k": round(float((found == k).float().mean()), 4),
                          "log_prob_calls_per_query": round(float(ncalls.float().mean()), 1),
                          "resolved": ix.last_categorize_stats()}
    ts = []
    for i in range(calls):
        t = time.perf_counter()
        w.cobweb_predict(Qn[i % nq], k)
        ts.append(time.perf_counter() - t)
    ts.sort()
    out["harness_basic_nq1_us"] = round(ts[len(ts) // 2] * 1e6, 1)
    w._invalidate_prediction_index()
    w0._invalidate_prediction_index()
    return out


def roofline_leg(index, Ql, k, st, N, D, pmc_file):
    """--full: the dominant kernel's time (HIP events on the launch stream, three calls of their
    own with timing on) against its pipe's peak, with the HBM traffic and the held clock of a
    matching PMC summary.  `st` = last_stats() of a timed step."""
    index.set_timing(True)
    tms = []
    for _ in range(3):
        index.score_topk(Ql, k)
        tms.append(index.last_timing())
    index.set_timing(False)
    call_ms = float(np.mean([t["call_ms"] for t in tms]))
    nql = len(Ql)
    NL = index.info["leaf_rows"]
    if st["filter_used"]:
        # bf16-MFMA candidate filter (cwq_mfma.hip fgemm): 2*D flops per (query, leaf row)
        kern_ms = float(np.mean([t["fgemm_ms"] for t in tms]))
        flops_launch = 2.0 * D * NL * nql
        peak, kname, pipe = PEAK_BF16_TFLOPS, "fgemm_kernel<0> (bf16 MFMA filter pass)", "bf16 MFMA dense"
        launches = max(1, round(float(np.mean([t["leaf_scan_launches"] for t in tms]))))   # filter phases
        phases = {"sample_ms": round(float(np.mean([t["sample_ms"] for t in tms])), 3),
                  "fgemm_ms": round(kern_ms, 3),
                  "rerank_ms": round(float(np.mean([t["rerank_ms"] for t in tms])), 3)}
    else:
        kern_ms = float(np.mean([t["leaf_scan_ms"] / max(1, t["leaf_scan_launches"]) for t in tms]))
        flops_launch = 4.0 * D * NL * nql                 # 4*Nn*D per query (leaf rows)
        peak, kname, pipe = PEAK_FP32_TFLOPS, "scan_kernel<ISO,TOPK> (exact fp32 leaf scan)", "fp32 VALU"
        phases = {}
        launches = 1
    achieved_tf = flops_launch / (kern_ms * 1e-3) / 1e12
    traffic = clk = pmc_used = None
    for pf in pmc_candidates(pmc_file):
        try:
            pm = json.load(open(pf))
        except (OSError, ValueError):
            continue
        if pm.get("workload") == [N, D, nql, k] and pm.get("kernel") == kname.split(" ")[0]:
            # per step (the filter launches of one call), like `achieved`; files before round 5
            # stored the per-call figure under the key hbm_bytes_per_launch
            traffic = pm.get("hbm_bytes_per_call", pm.get("hbm_bytes_per_launch"))
            clk = pm.get("effective_clock_ghz")   # GRBM_GUI_ACTIVE / kernel time, same PMC run
            pmc_used = os.path.relpath(pf, ROOT)
            break
    return {"bound": "mfma", "pipe": pipe,
            "achieved": round(achieved_tf, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved_tf / peak, 4), "traffic": traffic, "traffic_unit": "bytes per step",
            "pmc_file": pmc_used,
            "kernel": kname, "kernel_ms": round(kern_ms, 3), "launches_per_step": launches,
            "avg_launch_ms": round(kern_ms / launches, 3),
            "call_ms": round(call_ms, 3), "flops_per_step": flops_launch, "phases_ms": phases,
            # the dense peak assumes the 2.4 GHz peak clock; under this load the chip
            # holds the PMC-measured clock, so this is the fraction of what it can issue
            "clock_ghz_held": clk,
            "frac_at_held_clock": (round(achieved_tf / (peak * clk / PEAK_CLOCK_GHZ), 4)
                                   if clk and pipe.startswith("bf16") else None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", choices=sorted(PRESETS), default="c3")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--dim", type=int, default=None)
    ap.add_argument("--queries", type=int, default=None,
                    help="queries per GPU per step (weak) or per step in total (--strong)")
    ap.add_argument("--strong", action="store_true", default=None, help="split --queries over the ranks")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the (ids, scores) the last timed step returned to DIR/ids.npy, DIR/scores.npy")
    ap.add_argument("--full", action="store_true",
                    help="also measure the roofline, recall@10, per-call, hierarchical and CPU-baseline legs "
                         "(the options below choose among them)")
    ap.add_argument("--cpu-sample", type=int, default=20, help="CPU baseline queries at all host threads")
    ap.add_argument("--cpu-sample-1t", type=int, default=20, help="CPU baseline queries at 1 thread")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-per-call", action="store_true")
    ap.add_argument("--recall-queries", type=int, default=512)
    ap.add_argument("--no-hier", action="store_true",
                    help="skip the hierarchical leg (device ifit of a 100k x 768 clustered corpus + its queries)")
    ap.add_argument("--hier-n", type=int, default=100_000)
    ap.add_argument("--pmc-file", default=None,
                    help="PMC summary (scripts/pmc_summary.py) of the filter kernel; default: the newest "
                         "profiles/pmc_rNN_fgemm.json whose workload matches this run")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="rehearsal only: gloo lets several ranks share one GPU (RCCL refuses that)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    pre = PRESETS[args.preset]
    N = args.n or pre["n"]
    D = args.dim or pre["dim"]
    Qarg = args.queries or pre["queries"]
    strong = pre["strong"] if args.strong is None else args.strong
    k = args.k

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE {world}; using WORLD_SIZE")
    if args.dist_backend == "gloo":   # rehearsal of the N-rank path on fewer GPUs
        local %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    pkg = cobweb_pkg.load()
    pkg.lib()
    D_ = pkg.dist

    # ---- tree: synthesised on rank 0, broadcast over RCCL (dist.broadcast_tree) ----
    t0 = time.perf_counter()
    root_mu = None
    def dev_used():
        fr, tot = torch.cuda.mem_get_info(dev)
        return tot - fr

    if rank == 0:
        X = pkg.synth.synthetic_corpus(N, D, seed=0, device=dev)
        # variances in compact form: one scalar per leaf (prior_var), the root's row in full
        tree = pkg.synth.flat_synth(X, compact=True)
        mean, var, parent, nos = tree["mean"], tree["var"], tree["parent"], tree["node_of_sentence"]
        root_mu = tree["root"][1]
        del tree, X
    else:
        mean = var = parent = nos = None
    torch.cuda.synchronize()
    t_synth = time.perf_counter() - t0
    t_bcast, bstats = 0.0, {}
    if world > 1:
        dist.barrier()
        t1 = time.perf_counter()
        mean, var, parent, nos = D_.broadcast_tree(mean, var, parent, nos, src=0, device=dev, stats=bstats,
                                                   compact=True)
        torch.cuda.synchronize()
        t_bcast = time.perf_counter() - t1
    t1 = time.perf_counter()
    index = pkg.index.CobwebIndex(mean, var, parent, nos, device=dev)
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t1
    torch.cuda.empty_cache()
    used_create = dev_used()              # caller's mean + compact var + the index's own copies
    X = mean[1:]                          # leaf means are the corpus rows
    root_var_host = var[0].cpu().numpy() if rank == 0 else None
    del var

    # ---- queries: weak = Qarg per rank (seed 1 + rank); strong = Qarg in total, split ----
    if strong:
        Q, targets = pkg.synth.synthetic_queries(X, Qarg, seed=1)
        q_lo, q_hi = D_.shard_bounds(Qarg, rank, world)
        total_q = Qarg

        def step():
            return D_.sharded_query(index.score_topk, Q, k, gather=False)
    else:
        Q, targets = pkg.synth.synthetic_queries(X, Qarg, seed=1 + rank)
        q_lo, q_hi = 0, Qarg
        total_q = world * Qarg

        def step():
            return index.score_topk(Q, k)

    # everything that reads the corpus rows happens now; then the caller's copies go
    # (the index holds its own), so a rank holds the index + its workspace only
    Ql = Q[q_lo:q_hi]
    nql = q_hi - q_lo
    n_rec = min(args.recall_queries, nql) if args.full else 0
    gt = recall_truth(pkg, X, Ql, k, n_rec) if rank == 0 and n_rec > 0 else None
    Xh = X.cpu().numpy() if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline else None
    del X, mean
    torch.cuda.empty_cache()
    used_freed = dev_used()

    # ---- timed loop (barrier + sync on both sides, max over ranks) ----
    last = [None]

    def kept_step():                      # the timed path, its latest result kept for --dump-outputs
        last[0] = step()

    dt = D_.timed_steps(kept_step, args.steps, args.warmup, torch.cuda.synchronize)
    qps = total_q * args.steps / dt
    ids, scores = last[0]
    st = index.last_stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ids, scores)

    roof = roofline_leg(index, Ql, k, st, N, D, args.pmc_file) if args.full else None
    bytes_q = 8.0 * (N + 1) * D + 8.0 * 2 * N + 4.0 * D + 12.0 * k   # SURVEY §8(d) bytes per query

    torch.cuda.empty_cache()
    used_steady = dev_used()              # + the handle's workspace after the timed calls
    mem = {"index_bytes": index.info["device_bytes"], "device_used_after_index_create": used_create,
           "device_used_after_caller_copies_freed": used_freed,
           "device_used_after_timed_steps": used_steady,
           "peak_sampled": max(used_create, used_freed, used_steady),
           "device_total": torch.cuda.mem_get_info(dev)[1],
           "note": "device-wide used bytes (mem_get_info) on this rank, sampled after index create (caller's "
                   "mean still resident; the per-call int8 panel is built with the index), after the caller's "
                   "copies are freed, after the timed steps (index + the handle's workspace) and, with "
                   "--full, after the per-call legs"}

    rec_l2 = rec_ip = rec_tgt = None
    if gt is not None:
        tg = targets if q_lo == 0 else targets[:0]
        rec_l2, rec_ip, rec_tgt = recall_at_k(gt, ids, tg, k, n_rec)

    pc = None
    if args.full and rank == 0 and not args.no_per_call:
        pc = per_call(index, Ql, k)
        pc["harness_call_nq1"] = per_call_harness(pkg, index, Ql, k)
        try:
            pc["harness_basic_nq1"] = per_call_harness(pkg, index, Ql, k, reps=50, basic=True,
                                                       node_of_sentence=nos)
            pc["harness_basic_nq1"]["tree"] = "the bench's flat-synth tree (root -> leaves): Basic pops the root, " \
                                              "scores every leaf, retrieves the k best"
        except Exception as e:            # recorded, never hides the Fast legs
            pc["harness_basic_nq1"] = {"error": repr(e)}
        torch.cuda.empty_cache()
        mem["device_used_after_per_call"] = dev_used()
        mem["peak_sampled"] = max(mem["peak_sampled"], mem["device_used_after_per_call"])

    hier = None
    if args.full and rank == 0 and world == 1 and not args.no_hier:
        log(f"hierarchical leg: device ifit of {args.hier_n} x 768 clustered rows + queries ...")
        try:
            hier = hier_leg(pkg, n=args.hier_n)
        except Exception as e:            # recorded, never hides the headline line
            hier = {"error": repr(e)}
        torch.cuda.empty_cache()

    base = None
    if Xh is not None:
        log(f"cpu baseline: {args.cpu_sample} queries (all threads) + {args.cpu_sample_1t} (1 thread) ...")
        base = cpu_baseline(Xh, root_mu[0].cpu().numpy(), root_var_host, Ql[:max(args.cpu_sample, 1)].cpu().numpy(),
                            k, args.cpu_sample, args.cpu_sample_1t, ids[:args.cpu_sample].cpu().numpy())
        del Xh

    if rank == 0:
        out = {
            "metric": "queries/sec + recall@10 vs FAISS-flat, 1M×768 corpus, 1/2/4/8 MI355X",
            "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1000 * dt / args.steps, 3), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "full": args.full,
            "config": {"workload": f"Cobweb Fast top-{k}: synthetic flat-synth tree (root + {N} leaves), "
                                   f"X~N(0,I) {N}x{D} fp32, " +
                                   (f"{Qarg} queries/step split over {world} GPU(s)" if strong else
                                    f"{Qarg} queries/step/GPU") + f" ({config_label(N, D)})",
                       "preset": args.preset, "corpus": N, "dim": D, "queries_per_step": total_q,
                       "queries_per_gpu": nql, "k": k, "tree": "flat-synth",
                       "parallelism": f"query-shard x{world}, index broadcast over " + ("RCCL" if args.dist_backend == "nccl" else "gloo (rehearsal)") if world > 1
                       else "single GPU"},
            "roofline": roof,
            "filter": {k_: st[k_] for k_ in ("filter_used", "fallback_queries", "candidates", "exact_reranks",
                                              "sample_rows")},
            # the reference algorithm reads every node's mean+var once per query; a batch
            # shares each streamed byte, so this is a reuse ratio, not a roofline fraction
            "per_query_bytes_ratio": {"bytes_per_query_ref": bytes_q,
                                      "per_query_hbm_roof_qps": round(PEAK_HBM_GBS * 1e9 / bytes_q, 1),
                                      "qps_over_that_roof": round(qps / world * bytes_q / (PEAK_HBM_GBS * 1e9), 3)},
            "per_call": pc,
            "hier": hier,
            "recall@10": {"vs_flat_l2": rec_l2, "vs_flat_ip": rec_ip, "target_in_top10": rec_tgt,
                          "n_queries": n_rec,
                          # N(0,I) data: inner product and L2 rank differently (|x|^2 varies by
                          # ~5% of its mean at D=768), and the Fast key of a flat tree is an L2
                          # ranking, so recall vs flat-IP is low by construction, not a defect
                          "note_ip": "the Fast ranking on a flat tree is exact L2 k-NN; on N(0,I) rows |x|^2 "
                                     "varies, so flat-IP picks different neighbours"},
            "cpu_baseline": base,
            "memory_bytes_rank0": mem,
            "setup_s": {"synth": round(t_synth, 3), "rccl_broadcast": round(t_bcast, 3),
                        "rccl_broadcast_bytes": bstats.get("bytes"), "index_build": round(t_index, 3)},
        }
        print(json.dumps(out), flush=True)
    index.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
