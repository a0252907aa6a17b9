"""Pretest survival of the batch filter with bf16 vs int8 row/query splits (VERDICT r3 #3:
"measure the pretest survival per 16x64 block before writing the epilogue").

CPU model of the certified bound of fgemm_kernel (cwq_mfma.hip fg_bounds2) on the C3
workload's distribution (X ~ N(0,I), 768-d, half perturbed / half fresh queries), on a
row subset: per (query, row) the squared distance S and the bound's half-width in S units
  bf16: 2 (|x_hi| beta + |x_lo| delta),  beta = |mu_lo| + gamma |mu_hi|, delta = |mu_hi| + |mu_lo|
  int8: 2 (|x_q| beta8 + |x_r| delta8) + 2^-21 |x'.mu'|   (per-row / per-query scale s = max|v|/127,
        the split v = s q + r formed exactly -- the per-call int8 pass)
A row survives the filter when S - w <= S_(K) + w_(K) -- the threshold after tightening is
the K-th best upper bound of the candidates (in S units).  K is scaled to the subset so
that the survivors per query estimate the full 1M-row case.  Reported: survivors per
query (x 1M / rows) and the fraction of 16-query x 64-row MFMA blocks holding a survivor
(the blocks whose epilogue leaves the one-max-per-element fast path).

    python scripts/i8_batch_survival.py [--rows 262144] [--queries 256] [--hybrid]

--hybrid adds the table of the policy the batch filter runs (bf16 launches up to a cut of
the rows, int8 after it; hybrid() below) -- profiles/fgi8_model_c3.log, DESIGN Appendix C.1.
--hub adds the table of the threshold sample with hub rows (strided + lowest-norm rows) and of
the first int8 phase, launch by launch with the tighten passes (pipeline() below) --
profiles/hub_model_c3.log.  With --full equal to --rows the model runs a shape as it is
(the ratios the tests in tests/test_gpu_hub_sample.py ask for).
--direct adds the table of the direct schedule (direct() below): the threshold from the exact
keys of the rows an int8 ranking of the sample picks, against the certified-bound threshold,
with five launches, one launch and a few other cuts -- profiles/direct_model_c3.log.
"""
import argparse

import numpy as np


def bf16_split(v):
    """hi = bf16(v) (round to nearest even on the top 16 bits of fp32), lo = v - hi."""
    u = v.astype(np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    hi = r.view(np.float32)
    return hi, (v - hi).astype(np.float32)


def i8_split(v):
    s = np.abs(v).max(axis=1, keepdims=True) / 127.0
    q = np.clip(np.rint(v / s), -127, 127)
    hi = s * q
    return hi, v - hi


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262_144)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--full", type=int, default=1_000_000)
    ap.add_argument("--hybrid", action="store_true", help="also the bf16-then-int8 policy table (hybrid())")
    ap.add_argument("--hub", action="store_true", help="also the hub-sample / early int8 schedule table (hub())")
    ap.add_argument("--direct", action="store_true", help="also the direct-schedule table (direct())")
    args = ap.parse_args(argv)
    rng = np.random.default_rng(0)
    N, Q, D = args.rows, args.queries, args.dim
    X = rng.standard_normal((N, D), dtype=np.float32)
    c = X.mean(0)
    Xc = X - c
    pick = rng.choice(N, Q // 2, replace=False)
    qs = np.concatenate([X[pick] + 0.1 * rng.standard_normal((Q // 2, D), dtype=np.float32),
                         rng.standard_normal((Q - Q // 2, D), dtype=np.float32)]) - c
    K = max(1, int(round(args.k * N / args.full)))   # the subset's K-th ~ the full set's k-th
    gamma = (D + 64) * 2.0 ** -23
    out = {}
    dots = qs.astype(np.float64) @ Xc.astype(np.float64).T
    S = (qs.astype(np.float64) ** 2).sum(1)[:, None] + (Xc.astype(np.float64) ** 2).sum(1)[None, :] - 2 * dots
    for name in ("bf16", "int8"):
        if name == "bf16":
            rh, rl = bf16_split(Xc)
            xh, xl = bf16_split(qs)
            beta = np.linalg.norm(rl, axis=1) + gamma * np.linalg.norm(rh, axis=1)
            extra = 0.0
        else:
            rh, rl = i8_split(Xc.astype(np.float64))
            xh, xl = i8_split(qs.astype(np.float64))
            beta = np.linalg.norm(rl, axis=1)
            extra = 2.0 ** -21 * np.abs(dots)
        delta = np.linalg.norm(rh, axis=1) + np.linalg.norm(rl, axis=1)
        w = 2 * (np.linalg.norm(xh, axis=1)[:, None] * beta[None, :] +
                 np.linalg.norm(xl, axis=1)[:, None] * delta[None, :]) + 2 * extra
        ub = S + w
        thr = np.partition(ub, K - 1, axis=1)[:, K - 1]          # K-th best upper bound (S units)
        surv = (S - w) <= thr[:, None]
        per_q = surv.sum(1) * (args.full / N)
        nb_q, nb_r = Q // 16, N // 64
        blocks = surv[:nb_q * 16, :nb_r * 64].reshape(nb_q, 16, nb_r, 64).any(axis=(1, 3))
        out[name] = (np.median(per_q), per_q.mean(), blocks.mean(), float(np.median(w)))
        print(f"{name}: survivors per query (scaled to {args.full} rows) median {out[name][0]:.0f} mean "
              f"{out[name][1]:.0f}; 16x64 blocks with a survivor {100 * out[name][2]:.2f}%; median half-width "
              f"{out[name][3]:.3f} (S units)", flush=True)
    print(f"int8 / bf16: survivors x{out['int8'][1] / out['bf16'][1]:.2f}, active blocks "
          f"x{out['int8'][2] / out['bf16'][2]:.2f}", flush=True)
    if args.hybrid:
        hybrid(args, S, dots, Xc, qs, gamma, K)
    if args.hub:
        hub(args, S, dots, Xc, qs, gamma, K)
    if args.direct:
        return direct(args, S, dots, Xc, qs, gamma, K)


def sample_rows(N, norm2, sdiv=128, hub_div=None):
    """build_filter's threshold sample (cwq_build.hip): S = N/sdiv strided rows (whole 256-row
    tiles), then H hub rows (lowest |mu'|^2 = largest row term on a flat tree; ties by row
    index; rows of the strided part skipped), H = S/2 or N/hub_div (0: none; none when
    N < 4 S), hub j in the 4-row group j mod H/4."""
    S = min(32768, max(256, N // sdiv // 256 * 256))
    stride = max(1, N // S)
    rows = [r for r in (j * stride for j in range(S)) if r < N]
    H = S // 2 if hub_div is None else (N // hub_div // 256 * 256 if hub_div > 0 else 0)
    H = min(H, (32768 - len(rows)) // 4 * 4)
    if N < 4 * S or H <= 0:
        return np.array(rows), 0
    seen = set(rows)
    order = np.lexsort((np.arange(N), norm2))[:H + len(rows)]
    hubs = [int(r) for r in order if int(r) not in seen][:H]
    ng = (len(hubs) + 3) // 4
    rows += [hubs[j] for g in range(ng) for j in range(g, len(hubs), ng)]
    return np.array(rows), len(hubs)


def pipeline(S, wb, w8, wbt, w8t, K, samp, i8_from, cuts=(32, 96, 256, 512), T0=None):
    """The batch filter's launches (run_iso_filter) in S units (smaller = better key): T = the
    K-th best certified bound of the bf16 sample pass (per 4-row group when the sample has
    >= 64 K rows), then one launch per row phase -- int8 bounds from phase i8_from on, bf16
    before -- each followed by the tighten pass (T = K-th best candidate bound so far).
    Returns per query: candidates, raw records (pretest with the 256-row tile maxima),
    reranks by the K-th-best-bound rule, reranks by the exact-seeded rule (final_kernel),
    and the flagged shares of 16x64 blocks and 16x16 sub-blocks of the int8 launches.
    T0: the thresholds the first launch runs with instead of the sample pass's bound (the
    direct schedule's exact keys, exact_threshold()); cuts=(): one launch over every row."""
    Q, N = S.shape
    if T0 is None:
        sb = (S + wb)[:, samp]
        if len(samp) >= 64 * K:
            pad = (-len(samp)) % 4
            sb = np.pad(sb, ((0, 0), (0, pad)), constant_values=np.inf).reshape(Q, -1, 4).min(2)
        T = np.partition(sb, K - 1, axis=1)[:, K - 1]
    else:
        T = T0.copy()
    n_rt = (N + 255) // 256
    edges = [0]
    for f in cuts:
        c = max(edges[-1] // 256 + 1, n_rt * f // 1024)
        if c < n_rt:
            edges.append(c * 256)
    edges.append(N)
    cand = np.zeros((Q, N), bool)
    raw = np.zeros(Q)
    lo, hi = np.empty((Q, N)), np.empty((Q, N))
    flag64, flag16, n64, n16 = 0, 0, 0, 0
    for ph in range(len(edges) - 1):
        a, b = edges[ph], edges[ph + 1]
        w, wt = (w8, w8t) if ph >= i8_from else (wb, wbt)
        lo[:, a:b], hi[:, a:b] = (S - w)[:, a:b], (S + w)[:, a:b]
        cand[:, a:b] = lo[:, a:b] <= T[:, None]
        rec = (S - wt)[:, a:b] <= T[:, None]
        raw += rec.sum(1)
        if ph >= i8_from:
            for width in (64, 16):
                nq_, nr_ = Q // 16, (b - a) // width
                m = rec[:nq_ * 16, :nr_ * width].reshape(nq_, 16, nr_, width).any(axis=(1, 3))
                if width == 64:
                    flag64, n64 = flag64 + m.sum(), n64 + m.size
                else:
                    flag16, n16 = flag16 + m.sum(), n16 + m.size
        kth = np.partition(np.where(cand, hi, np.inf), K - 1, axis=1)[:, K - 1]
        T = np.minimum(T, kth)
    hic = np.where(cand, hi, np.inf)
    t2 = np.partition(hic, K - 1, axis=1)[:, K - 1]
    rer = (cand & (lo <= t2[:, None])).sum(1)
    seeds = np.argpartition(hic, K - 1, axis=1)[:, :K]
    t2s = np.minimum(t2, np.take_along_axis(S, seeds, 1).max(1))
    notseed = cand.copy()
    np.put_along_axis(notseed, seeds, False, 1)
    rer_s = K + (notseed & (lo <= t2s[:, None])).sum(1)
    return (cand.sum(1), raw, rer, rer_s, flag64 / max(n64, 1), flag16 / max(n16, 1))


def hub(args, S, dots, Xc, qs, gamma, K):
    """Hub rows in the threshold sample and the early int8 schedule: the
    pipeline() model per sample and first int8 phase -- profiles/hub_model_c3.log."""
    N, Q = S.shape[1], S.shape[0]
    scale = args.full / N

    def widths(split, extra):
        rh, rl = split(Xc.astype(np.float64))
        xh, xl = split(qs.astype(np.float64))
        nh, nl = np.linalg.norm(rh, axis=1), np.linalg.norm(rl, axis=1)
        beta = nl + (gamma * nh if extra is None else 0.0)
        delta = nh + nl
        a, c = np.linalg.norm(xh, axis=1)[:, None], np.linalg.norm(xl, axis=1)[:, None]
        w = 2 * (a * beta[None, :] + c * delta[None, :]) + (0.0 if extra is None else 2 * extra)
        nt = N // 256 * 256
        bm = np.repeat(beta[:nt].reshape(-1, 256).max(1), 256)
        dm = np.repeat(delta[:nt].reshape(-1, 256).max(1), 256)
        wt = np.full_like(w, np.inf)   # (rows of a last partial tile: always flagged)
        wt[:, :nt] = 2 * (a * bm[None, :] + c * dm[None, :])
        return w, np.maximum(w, wt)

    wb, wbt = widths(lambda v: bf16_split(v.astype(np.float32)), None)
    w8, w8t = widths(i8_split, 2.0 ** -21 * np.abs(dots))
    norm2 = (Xc.astype(np.float64) ** 2).sum(1)
    kth = np.partition(S, K - 1, axis=1)[:, K - 1]
    print(f"hub model, K = {K} of {N} x {Xc.shape[1]} rows, {Q} queries, x{scale:.2f} to {args.full} rows")
    for name, hd in (("strided", 0), ("strided + hub S/2", None), ("strided + hub 1/128", 128)):
        samp, nh = sample_rows(N, norm2, hub_div=hd)
        best = np.partition(S[:, samp], K - 1, axis=1)[:, K - 1]
        rank = (S < best[:, None]).sum(1) * scale
        print(f"sample {name}: {len(samp)} rows ({nh} hub); rank of its K-th best key median {np.median(rank):.0f} "
              f"max {rank.max():.0f}; K-th best key overall in the sample for {100 * (best <= kth).mean():.0f}% of queries")
    print("| sample | first int8 phase | cand/q | raw records/q | 16x64 blocks | 16x16 sub-blocks | reranks/q bound rule | "
          "reranks/q exact-seeded |")
    for name, hd, i8_from in (("strided", 0, 3), ("strided", 0, 0), ("strided + hub S/2", None, 3),
                              ("strided + hub S/2", None, 1), ("strided + hub S/2", None, 0),
                              ("strided + hub 1/128", 128, 0), ("strided", 0, 9), ("strided + hub S/2", None, 9)):
        samp, _ = sample_rows(N, norm2, hub_div=hd)
        c, raw, rer, rer_s, b64, b16 = pipeline(S, wb, w8, wbt, w8t, K, samp, i8_from)
        first = {3: "3 (a quarter)", 9: "none (bf16)"}.get(i8_from, str(i8_from))
        print(f"| {name} | {first} | {c.mean() * scale:.0f} | {raw.mean() * scale:.0f} | {100 * b64:.1f}% | "
              f"{100 * b16:.1f}% | {rer.mean() * scale:.0f} | {rer_s.mean() * scale:.0f} |", flush=True)


def exact_threshold(S, S8, samp, K, pick=1):
    """The direct schedule's threshold (sample_threshold_kernel) in S units: the sample rows are
    ranked by the int8 dot's approximate key S8, one value per group of 4 sample rows; the
    pick * K best groups' best rows are scored exactly and T is the K-th best of those exact
    keys.  Valid whatever the ranking picks: K distinct rows have keys at least as good."""
    Q = S.shape[0]
    pad = (-len(samp)) % 4
    a8 = np.pad(S8[:, samp], ((0, 0), (0, pad)), constant_values=np.inf).reshape(Q, -1, 4)
    rows = np.pad(samp, (0, pad))[None, :].repeat(Q, 0).reshape(Q, -1, 4)
    jb = a8.argmin(2)
    grp = np.argpartition(a8.min(2), pick * K - 1, axis=1)[:, :pick * K]
    chosen = np.take_along_axis(np.take_along_axis(rows, jb[:, :, None], 2)[:, :, 0], grp, 1)
    return np.partition(np.take_along_axis(S, chosen, 1), K - 1, axis=1)[:, K - 1]


def split_widths(Xc, qs, gamma, split, extra):
    """Half-widths w of the certified bounds per (query, row) and wt, the pretest's, with the
    256-row tile maxima of beta and delta (hub()'s and hybrid()'s widths), and the hi parts."""
    N = Xc.shape[0]
    rh, rl = split(Xc.astype(np.float64))
    xh, xl = split(qs.astype(np.float64))
    nh, nl = np.linalg.norm(rh, axis=1), np.linalg.norm(rl, axis=1)
    beta = nl + (gamma * nh if extra is None else 0.0)
    delta = nh + nl
    a, c = np.linalg.norm(xh, axis=1)[:, None], np.linalg.norm(xl, axis=1)[:, None]
    w = 2 * (a * beta[None, :] + c * delta[None, :]) + (0.0 if extra is None else 2 * extra)
    nt = N // 256 * 256
    bm = np.repeat(beta[:nt].reshape(-1, 256).max(1), 256)
    dm = np.repeat(delta[:nt].reshape(-1, 256).max(1), 256)
    wt = np.full_like(w, np.inf)   # (rows of a last partial tile: always flagged)
    wt[:, :nt] = 2 * (a * bm[None, :] + c * dm[None, :])
    return w, np.maximum(w, wt), xh, rh


def direct(args, S, dots, Xc, qs, gamma, K):
    """The direct schedule against the early one: hub S/2 sample, every launch on
    the int8 operands, the first launch's threshold from the certified bf16 bounds of the sample
    (today) or from exact keys of the rows the int8 ranking picks, by launch cuts.  Returns
    {(threshold, cuts): candidates per query} for tests/test_direct_model_cpu.py."""
    N = S.shape[1]
    scale = args.full / N
    wb, wbt, _, _ = split_widths(Xc, qs, gamma, lambda v: bf16_split(v.astype(np.float32)), None)
    w8, w8t, xh8, rh8 = split_widths(Xc, qs, gamma, i8_split, 2.0 ** -21 * np.abs(dots))
    norm2 = (Xc.astype(np.float64) ** 2).sum(1)
    S8 = (qs.astype(np.float64) ** 2).sum(1)[:, None] + norm2[None, :] - 2 * (xh8 @ rh8.T)
    samp, nh = sample_rows(N, norm2)
    print(f"direct model, K = {K} of {N} x {Xc.shape[1]} rows, {S.shape[0]} queries, x{scale:.2f} to {args.full} "
          f"rows; sample {len(samp)} rows ({nh} hub)")
    print("| threshold | cuts | cand/q | raw records/q | 16x16 sub-blocks | reranks/q exact-seeded |")
    out = {}
    five = (32, 96, 256, 512)
    for name, T0 in (("bf16 bound", None), ("exact keys", exact_threshold(S, S8, samp, K)),
                     ("exact keys, 2K rows", exact_threshold(S, S8, samp, K, 2))):
        for cuts in (five, ()) if T0 is None or "2K" in name else (five, (), (32,), (128,), (32, 256)):
            c, raw, _, rer_s, _, b16 = pipeline(S, wb, w8, wbt, w8t, K, samp, 0, cuts, T0)
            out[name, cuts] = c.mean() * scale
            print(f"| {name} | {','.join(map(str, cuts)) or 'one launch'} | {c.mean() * scale:.0f} | "
                  f"{raw.mean() * scale:.0f} | {100 * b16:.1f}% | {rer_s.mean() * scale:.0f} |", flush=True)
    return out


def hybrid(args, S, dots, Xc, qs, gamma, K):
    """The hybrid policy of run_iso_filter: bf16 launches over the first `cut` of
    the rows set T (the K-th best bf16 upper bound there, frozen -- the pipeline tightens
    again at 1/2, so this is pessimistic), int8 launches take the rest.  Per cut, for the rest
    of the rows in bf16 and in int8: candidates per query (scaled to --full rows), raw records
    per query (the pretest, with the 256-row tile maxima of beta and delta) and the share of
    16x64 blocks holding a raw record; then the exact reranks per query when every candidate
    keeps the bounds of the pass that produced it (T2 = K-th best upper bound of all
    candidates; reranked: lower bound within T2)."""
    N, Q = S.shape[1], S.shape[0]
    scale = args.full / N

    def widths(split, extra):
        rh, rl = split(Xc.astype(np.float64))
        xh, xl = split(qs.astype(np.float64))
        nh, nl = np.linalg.norm(rh, axis=1), np.linalg.norm(rl, axis=1)
        beta = nl + (gamma * nh if extra is None else 0.0)
        delta = nh + nl
        a, c = np.linalg.norm(xh, axis=1)[:, None], np.linalg.norm(xl, axis=1)[:, None]
        w = 2 * (a * beta[None, :] + c * delta[None, :]) + (0.0 if extra is None else 2 * extra)
        nt = N // 256 * 256
        bm = np.repeat(beta[:nt].reshape(-1, 256).max(1), 256)
        dm = np.repeat(delta[:nt].reshape(-1, 256).max(1), 256)
        wt = np.full_like(w, np.inf)   # (rows of a last partial tile: always flagged)
        wt[:, :nt] = 2 * (a * bm[None, :] + c * dm[None, :])
        return w, np.maximum(w, wt)

    wb, wbt = widths(lambda v: bf16_split(v.astype(np.float32)), None)
    w8, w8t = widths(i8_split, 2.0 ** -21 * np.abs(dots))
    print(f"hybrid policy, K = {K} of {N} rows, x{scale:.2f} to {args.full} rows; kFgCapQ / 4 = 1024")
    print("| bf16 over the first | rest bf16: cand/q, blocks | rest int8: cand/q, raw records/q, blocks | total cand/q "
          "bf16 / hybrid | reranks/q bf16 / hybrid |")
    for num, den in ((1, 32), (3, 32), (1, 4), (1, 2)):
        n0 = N * num // den
        thr = np.partition((S + wb)[:, :n0], K - 1, axis=1)[:, K - 1][:, None]
        head = ((S - wb)[:, :n0] <= thr)
        rest = {"bf16": ((S - wb)[:, n0:] <= thr, (S - wbt)[:, n0:] <= thr),
                "int8": ((S - w8)[:, n0:] <= thr, (S - w8t)[:, n0:] <= thr)}

        def blocks(m):
            nq_, nr_ = Q // 16, m.shape[1] // 64
            return m[:nq_ * 16, :nr_ * 64].reshape(nq_, 16, nr_, 64).any(axis=(1, 3)).mean()

        rer = {}
        for name, wr in (("bf16", wb), ("int8", w8)):
            cand = np.concatenate([head, rest[name][0]], axis=1)
            ub = np.where(cand, np.concatenate([(S + wb)[:, :n0], (S + wr)[:, n0:]], axis=1), np.inf)
            lo = np.concatenate([(S - wb)[:, :n0], (S - wr)[:, n0:]], axis=1)
            t2 = np.partition(ub, K - 1, axis=1)[:, K - 1][:, None]
            rer[name] = (cand & (lo <= t2)).sum(1).mean() * scale
        cb, c8 = rest["bf16"][0].sum(1).mean() * scale, rest["int8"][0].sum(1).mean() * scale
        hd = head.sum(1).mean() * scale
        print(f"| {num}/{den} | {cb:.0f}, {100 * blocks(rest['bf16'][1]):.0f} % | {c8:.0f}, "
              f"{rest['int8'][1].sum(1).mean() * scale:.0f}, {100 * blocks(rest['int8'][1]):.0f} % | "
              f"{hd + cb:.0f} / {hd + c8:.0f} | {rer['bf16']:.0f} / {rer['int8']:.0f} |", flush=True)


if __name__ == "__main__":
    main()
