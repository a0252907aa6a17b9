"""GPU tests of the masked ranking loss (cwq_rank_ce_masked / cwq_rank_ce_topk_masked, DESIGN.md
§4.19): the cross-entropy, its gradient, the target's score and rank over a mask's allowed
sentences, on both paths (CWQ_MASK_CE_PATH = 1 full, 2 gathered).

Yardstick: the unmasked tests' (ce_yardstick / grad_yardstick / sparse_yardstick) with the
disallowed columns of the library's own fp32 scores set to -inf -- which tests/
test_masked_loss_cpu.py shows to be the plain yardstick on the sub-corpus of allowed sentences.
Temperature: the standard deviation of the tree's finite scores (one per tree: the C ABI takes
one per call) and, on the flat and the multi-sentence golden, the reference's T = 1.0."""
import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import sparse_yardstick as SY
import test_gpu_grad as TG
import test_gpu_rank_ce as RC
import test_gpu_sparse_scores as SS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
PATHS = (1, 2)
INF = float("inf")


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


class MaskedDense:
    """A dense scorer with the disallowed columns at -inf (ce_through reads .M and .scores)."""

    def __init__(self, dense, flags):
        self.d, self.M, self.keep = dense, dense.M, torch.as_tensor(np.asarray(flags, bool))

    def scores(self, x):
        s = self.d.scores(x)
        return torch.where(self.keep, s, torch.full_like(s, -INF))


def call(ix, m, Q, tg, T, path, monkeypatch, grad=True):
    """One masked call on a forced path; the stats name that path."""
    monkeypatch.setenv("CWQ_MASK_CE_PATH", str(path))
    out = ix.rank_ce(Q, tg, T, grad=grad, mask=m)
    st = ix.last_mask_stats()
    assert st["path"] == (5 if path == 1 else 6), st
    assert st["live_rows"] == m.info["live_iso_rows"] + m.info["live_aniso_rows"], st
    return out


def both_paths(ix, m, Q, tg, T, monkeypatch, label):
    """(full, gathered): loss, target_score and rank bit-identical, grad_q within Y.LIMIT."""
    a = call(ix, m, Q, tg, T, 1, monkeypatch)
    b = call(ix, m, Q, tg, T, 2, monkeypatch)
    for i in (0, 2, 3):
        assert torch.equal(a[i], b[i]), (label, "paths differ", i)
    ga, gb = a[1].cpu().numpy().astype(np.float64), b[1].cpu().numpy().astype(np.float64)
    nz = np.linalg.norm(ga, axis=1) > 0
    assert not gb[~nz].any(), label
    if nz.any():
        e = Y.rel_l2(gb[nz], ga[nz])
        print(f"{label}: gathered grad_q against the full path's max {e.max():.3g}")
        assert e.max() < Y.LIMIT, (label, e)
    return a, b


def masked_scores(S, flags):
    Sm = S.clone()
    Sm[:, torch.as_tensor(~np.asarray(flags, bool), device=S.device)] = -INF
    return Sm


def check_masked(ix, Q, nos, flags, tg, T, monkeypatch, label, S=None):
    """Both paths against the yardstick on the library's own scores: target_score, rank, the loss
    in fp64, and grad_q against the dense backward of the fp64 softmax - one-hot.  Valid targets."""
    Q = torch.as_tensor(Q, dtype=torch.float32, device=DEV)
    S = ix.rank_scores(Q) if S is None else S
    Sm = masked_scores(S, flags)
    Sc = Sm.cpu().numpy()
    tgt = torch.as_tensor(np.asarray(tg, np.int64), device=DEV)
    m = ix.sentence_mask(np.asarray(flags, bool))
    try:
        outs = both_paths(ix, m, Q, tgt, T, monkeypatch, label)
    finally:
        m.close()
    want_rank = C.rank_of_targets(Sm, tg, nos)
    lS = C.loss_on_scores(Sc, tg, np.float64(np.float32(T)))
    G32 = torch.from_numpy(C.softmax_grad_on_scores(Sc, tg, np.float64(np.float32(T))).astype(np.float32))
    gB = ix.rank_scores_backward(Q, G32).cpu().numpy().astype(np.float64)
    for path, (lo, gq, ts, rk) in zip(PATHS, outs):
        assert torch.equal(ts, S.gather(1, tgt[:, None])[:, 0]), (label, path, "target_score")
        assert torch.equal(rk, want_rank), (label, path, "rank", rk, want_rank)
        loss = lo.double().cpu().numpy()
        grad = gq.cpu().numpy().astype(np.float64)
        assert np.isfinite(loss).all() and np.isfinite(grad).all(), (label, path)
        e3 = np.abs(loss - lS) / np.maximum(1.0, np.abs(lS))
        nz = np.linalg.norm(gB, axis=1) > 0
        assert not grad[~nz].any(), (label, path)      # one allowed sentence: the loss is constant
        e4 = Y.rel_l2(grad[nz], gB[nz]) if nz.any() else np.zeros(1)
        print(f"{label} path {path}: loss vs fp64 on own masked scores max {e3.max():.3g}  grad vs backward of the "
              f"fp64 softmax max {e4.max():.3g}")
        assert e3.max() <= 1e-5, (label, path, e3)
        assert e4.max() < Y.LIMIT, (label, path, e4)
    return outs, Sm


def third_allowed(Sm, nos):
    """Per query the third-ranked allowed sentence (the last one when fewer are allowed)."""
    Sc = Sm.cpu().numpy()
    out = []
    for q in range(Sc.shape[0]):
        o = SY.order(Sc[q], nos)
        o = o[np.isfinite(Sc[q, o])]
        out.append(o[min(2, len(o) - 1)])
    return np.array(out, np.int64)


# ---- 1. the goldens at four allowed fractions, 2. the all-ones mask ---------------------------
FRACTIONS = {"all": 1.0, "half": 0.5, "tenth": 0.1, "single": 0.0}


def mask_flags(nos, frac, seed):
    n = len(nos)
    in_tree = np.nonzero(nos >= 0)[0]
    if frac >= 1.0:
        return np.ones(n, bool)
    if frac == 0.0:
        f = np.zeros(n, bool)
        f[in_tree[len(in_tree) // 2]] = True
        return f
    f = np.random.default_rng(seed).random(n) < frac
    f[in_tree[:3]] = True              # at least three allowed sentences in the tree
    return f


@pytest.mark.parametrize("frac", list(FRACTIONS))
@pytest.mark.parametrize("name", TG.GOLDENS)
def test_goldens(gpu, name, frac, monkeypatch):
    arrays, Xq, d64, d32, _ = TG.setup(name)
    nos = arrays[3]
    ix = TG.make_index(gpu, arrays)
    S = ix.rank_scores(Xq)
    flags = mask_flags(nos, FRACTIONS[frac], 11)
    Sm = masked_scores(S, flags)
    tg = third_allowed(Sm, nos)
    Tsd = float(np.float32(S[torch.isfinite(S)].double().std().item()))
    for T in [Tsd] + ([1.0] if name in ("g10_grad_d24", "g2_flat_d768") else []):
        label = f"{name} {frac} T={T:.3g}"
        outs, _ = check_masked(ix, Xq, nos, flags, tg, T, monkeypatch, label, S)
        # end to end: fp64 autograd of the whole masked loss, under the unmasked tests' rule
        l64, g64 = C.ce_through(MaskedDense(d64, flags), Xq, tg, np.full(len(Xq), np.float64(np.float32(T))))
        l32, g32 = C.ce_through(MaskedDense(d32, flags), Xq, tg, np.full(len(Xq), np.float64(np.float32(T))))
        nz = np.linalg.norm(g64, axis=1) > 0
        den = np.maximum(np.abs(l64), 1e-300)
        for path, (lo, gq, _, _) in zip(PATHS, outs):
            loss = lo.double().cpu().numpy()
            if frac == "single":       # the target alone: loss 0, gradient 0, nothing relative to take
                assert np.abs(loss).max() <= 1e-5 and np.abs(l64).max() <= 1e-9 and not nz.any()
                continue
            e5 = Y.rel_l2(gq.cpu().numpy()[nz], g64[nz])
            e5l = np.abs(loss - l64) / den
            e_g32, e_l32 = Y.rel_l2(g32[nz], g64[nz]), np.abs(l32 - l64) / den
            print(f"{label} path {path}: end to end grad max {e5.max():.3g} (E_ref {e_g32.max():.3g})  loss max "
                  f"{e5l.max():.3g} (E_ref {e_l32.max():.3g})")
            assert e5.max() <= C.rule(e_g32), (label, path, e5, e_g32)
            assert e5l.max() <= C.rule(e_l32), (label, path, e5l, e_l32)
        if frac == "all":              # 2: the all-ones mask is cwq_rank_ce
            tgt = torch.as_tensor(tg, device=DEV)
            plain = ix.rank_ce(Xq, tgt, T, grad=True)
            assert all(torch.equal(a, b) for a, b in zip(outs[0], plain)), label          # full path: every bit
            assert all(torch.equal(outs[1][i], plain[i]) for i in (0, 2, 3)), label
            assert Y.rel_l2(outs[1][1].cpu().numpy(), plain[1].cpu().numpy().astype(np.float64)).max() < Y.LIMIT


# ---- 3. edges of the gathered tile (64 rows, 256 shared-query) and of a CE part (2,048 rows) ---
_edge = {}


def edge_tree(gpu):
    """Flat 4,200 x 40: D is no multiple of 16, three CE parts with the last one partial."""
    if not _edge:
        X = gpu.synth.synthetic_corpus(4200, 40, seed=71, device=DEV)
        t = gpu.synth.flat_synth(X)
        ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
        Q, _ = gpu.synth.synthetic_queries(X, 65, seed=72)
        Q = Q.contiguous()
        S = ix.rank_scores(Q)
        nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
        _edge.update(ix=ix, Q=Q, S=S, nos=nos, T=float(np.float32(S.double().std().item())))
    return _edge


@pytest.mark.parametrize("n_live", [1, 63, 64, 65, 255, 256, 257, 2047, 2049, 4199])
def test_tile_and_part_edges(gpu, n_live, monkeypatch):
    e = edge_tree(gpu)
    ix, Q, S, nos, T = e["ix"], e["Q"], e["S"], e["nos"], e["T"]
    n = ix.n_sent
    rows = np.sort(np.random.default_rng(n_live).choice(n, n_live, replace=False))
    flags = np.zeros(n, bool)
    flags[rows] = True
    tg = np.where(np.arange(65) % 2 == 0, rows[0], rows[-1]).astype(np.int64)   # the first and the last live row
    for nq in (65, 17, 16, 1):
        check_masked(ix, Q[:nq], nos, flags, tg[:nq], T, monkeypatch, f"edges live={n_live} nq={nq}", S[:nq])


# ---- 4. mixed isotropic / anisotropic rows ----------------------------------------------------
def test_mixed_row_classes(gpu, monkeypatch):
    """test_gpu_masked_topk.mixed's tree: 6,000 x 64 with 700 anisotropic leaves."""
    X = gpu.synth.synthetic_corpus(6000, 64, seed=3)
    fs = gpu.synth.flat_synth(X)
    var = fs["var"].clone()
    g = torch.Generator(device=X.device)
    g.manual_seed(5)
    an = torch.randperm(6000, generator=g, device=X.device)[:700] + 1
    var[an] = var[an] * (0.5 + torch.rand((700, 64), generator=g, device=X.device))
    ix = gpu.index.CobwebIndex(fs["mean"], var, fs["parent"], fs["node_of_sentence"], device=DEV)
    assert ix.info["isotropic_rows"] == 5300
    Q, _ = gpu.synth.synthetic_queries(X, 33, seed=9)
    Q = Q.to(DEV).contiguous()
    nos = np.asarray(torch.as_tensor(fs["node_of_sentence"]).cpu())
    an_sent = np.zeros(6000, bool)
    an_sent[(an - 1).cpu().numpy()] = True
    S = ix.rank_scores(Q)
    T = float(np.float32(S.double().std().item()))
    for tag, flags in (("anisotropic only", an_sent), ("isotropic only", ~an_sent),
                       ("both", np.random.default_rng(4).random(6000) < 0.5)):
        tg = third_allowed(masked_scores(S, flags), nos)
        for nq in (33, 16):            # the query-split and the shared-query form of the gathered scan
            check_masked(ix, Q[:nq], nos, flags, tg[:nq], T, monkeypatch, f"mixed {tag} nq={nq}", S[:nq])


# ---- 5. rows with several sentences, sentences outside the tree -------------------------------
def test_partly_allowed_multi_sentence_leaves(gpu, monkeypatch):
    """g10: of a leaf's sentences some are allowed and some are not -- the row's count in the
    softmax, the target's place inside its own row and the coefficient all use the allowed count."""
    arrays, Xq, _, _, _ = TG.setup("g10_grad_d24")
    nos = arrays[3]
    ix = TG.make_index(gpu, arrays)
    S = ix.rank_scores(Xq)
    T = float(np.float32(S[torch.isfinite(S)].double().std().item()))
    nodes, counts = np.unique(nos[nos >= 0], return_counts=True)
    multi = nodes[counts > 1]
    assert len(multi) >= 3
    base = np.random.default_rng(5).random(len(nos)) < 0.6
    for nd in multi[:4]:
        sids = np.nonzero(nos == nd)[0]
        for drop in (sids[0], sids[-1]):               # the first / the last sentence of the leaf is not allowed
            flags = base.copy()
            flags[sids] = True
            flags[drop] = False
            ranks = []
            for s in sids[sids != drop]:
                outs, _ = check_masked(ix, Xq, nos, flags, np.full(len(Xq), s, np.int64), T, monkeypatch,
                                       f"g10 leaf {nd} without {drop} target {s}", S)
                ranks.append(outs[0][3])
            for a, b in zip(ranks, ranks[1:]):
                assert torch.equal(b, a + 1), nd       # neighbours among the ALLOWED sentences of the leaf


def test_sentences_outside_the_tree(gpu, monkeypatch):
    """g1 with every 7th sentence removed, some of the removed ones allowed: they count for nothing."""
    (mean, var, parent, nos), Xq, _, _, _ = TG.setup("g1_hier_d32")
    nos = nos.copy()
    miss = np.arange(0, len(nos), 7)
    nos[miss] = -1
    ix = TG.make_index(gpu, (mean, var, parent, nos))
    S = ix.rank_scores(Xq)
    flags = np.random.default_rng(8).random(len(nos)) < 0.4
    flags[miss[::2]] = True
    Sm = masked_scores(S, flags)
    tg = third_allowed(Sm, nos)
    T = float(np.float32(Sm[torch.isfinite(Sm)].double().std().item()))
    m = ix.sentence_mask(flags)
    assert m.info["allowed"] == int((flags & (nos >= 0)).sum())
    m.close()
    check_masked(ix, Xq, nos, flags, tg, T, monkeypatch, "g1 with missing sentences", S)


# ---- 6. invalid targets -----------------------------------------------------------------------
def test_invalid_targets(gpu, monkeypatch):
    (mean, var, parent, nos), Xq, _, _, _ = TG.setup("g1_hier_d32")
    nos = nos.copy()
    nos[5] = -1
    ix = TG.make_index(gpu, (mean, var, parent, nos))
    S = ix.rank_scores(Xq)
    flags = np.random.default_rng(9).random(len(nos)) < 0.5
    flags[5] = True                                    # allowed, but outside the tree
    tg = third_allowed(masked_scores(S, flags), nos)
    T = 3.0
    not_allowed = int(np.nonzero(~flags & (nos >= 0))[0][0])
    m = ix.sentence_mask(flags)
    empty = ix.sentence_mask(np.zeros(len(nos), bool))
    try:
        good = both_paths(ix, m, torch.as_tensor(Xq, device=DEV), torch.as_tensor(tg, device=DEV), T, monkeypatch, "valid")
        bad = tg.copy()
        bad[1], bad[3], bad[4], bad[6] = not_allowed, len(nos), 5, -2
        inv = torch.zeros(len(Xq), dtype=torch.bool, device=DEV)
        inv[[1, 3, 4, 6]] = True
        outs = both_paths(ix, m, torch.as_tensor(Xq, device=DEV), torch.as_tensor(bad, device=DEV), T, monkeypatch, "mixed")
        for (lo, gq, ts, rk), ref in zip(outs, good):
            assert (lo[inv] == INF).all() and (ts[inv] == -INF).all() and (rk[inv] == -1).all()
            assert not gq[inv].any()
            for a, b in zip((lo, gq, ts, rk), ref):
                assert torch.equal(a[~inv], b[~inv])   # the valid rows: undisturbed
        for path in PATHS:                             # an empty mask: that result for every query, no scan
            monkeypatch.setenv("CWQ_MASK_CE_PATH", str(path))
            lo, gq, ts, rk = ix.rank_ce(Xq, tg, T, grad=True, mask=empty)
            assert (lo == INF).all() and (ts == -INF).all() and (rk == -1).all() and not gq.any()
            lo, gq, ts, rk = ix.rank_ce(Xq, tg, T, mask=empty)
            assert gq is None and (lo == INF).all() and (rk == -1).all()
            assert ix.last_mask_stats()["live_rows"] == 0
    finally:
        m.close()
        empty.close()


# ---- 7. rank <= k iff the masked top-k returns the target; 8. batch and chunk independence ----
def test_rank_against_masked_topk(gpu, monkeypatch):
    t, Q, ix, S, _, temps = RC.synth(gpu, "flat")
    nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
    flags = np.random.default_rng(12).random(ix.n_sent) < 0.3
    Sc = masked_scores(S, flags).cpu().numpy()
    pos = [0, 1, 8, 9, 10, 11, 62, 63, 64, 65, 300]    # around every k
    tg = np.array([(lambda o: o[np.isfinite(Sc[q, o])][pos[q % len(pos)]])(SY.order(Sc[q], nos)) for q in range(33)])
    tgt = torch.as_tensor(tg, device=DEV)
    m = ix.sentence_mask(flags)
    try:
        for path in PATHS:
            _, _, _, rk = call(ix, m, Q, tgt, 1.0, path, monkeypatch, grad=False)
            assert rk.cpu().tolist() == [pos[q % len(pos)] + 1 for q in range(33)]
            for k in (1, 10, 64):
                ids, _ = ix.score_topk(Q, k, mask=m)
                assert torch.equal((ids == tgt[:, None]).any(1), rk <= k), (path, k)
    finally:
        m.close()


def test_batch_and_chunk_independence(gpu, monkeypatch):
    t, Q, ix, S, _, temps = RC.synth(gpu, "flat")
    nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
    flags = np.random.default_rng(13).random(ix.n_sent) < 0.25
    tg = torch.as_tensor(third_allowed(masked_scores(S, flags), nos), device=DEV)
    T = float(temps.mean())
    m = ix.sentence_mask(flags)
    try:
        for path in PATHS:
            full = call(ix, m, Q, tg, T, path, monkeypatch)
            again = call(ix, m, Q, tg, T, path, monkeypatch)
            assert all(torch.equal(a, b) for a, b in zip(full, again))
            fwd = call(ix, m, Q, tg, T, path, monkeypatch, grad=False)
            assert fwd[1] is None and all(torch.equal(fwd[i], full[i]) for i in (0, 2, 3))
            for qi in range(33):
                one = call(ix, m, Q[qi:qi + 1], tg[qi:qi + 1], T, path, monkeypatch)
                assert all(torch.equal(a[0], b[qi]) for a, b in zip(one, full)), (path, qi)
            monkeypatch.setenv("CWQ_WS_BUDGET_MB", "1")
            rep = call(ix, m, Q.repeat(10, 1), tg.repeat(10), T, path, monkeypatch)
            monkeypatch.delenv("CWQ_WS_BUDGET_MB")
            assert all(torch.equal(a, b.repeat(10, *([1] * (b.dim() - 1)))) for a, b in zip(rep, full)), path
    finally:
        m.close()


# ---- 9. the top-K form ------------------------------------------------------------------------
def check_topk_masked(ix, Q, nos, d64, d32, flags, targets, T, K, monkeypatch, label):
    """test_gpu_sparse_scores.check_topk_loss with the mask: sparse_yardstick on the masked scores
    with the disallowed sentences taken out of the tree (nos -1)."""
    nq = Q.shape[0]
    tg = torch.as_tensor(np.asarray(targets, np.int64), device=DEV)
    S = ix.rank_scores(Q)
    Sm = masked_scores(S, flags)
    nos_m = np.where(flags, nos, -1)
    m = ix.sentence_mask(flags)
    try:
        ids_ref, _ = ix.score_topk(Q, K, mask=m)
        monkeypatch.setenv("CWQ_MASK_CE_PATH", "1")
        full, _, ts_full, rank_full = ix.rank_ce(Q, tg, T, mask=m)
        loss, gq, tscore, rank, bound, cand = ix.rank_ce_topk(Q, tg, K, T, grad=True, mask=m)
        loss0, none, ts0, rk0, b0, c0 = ix.rank_ce_topk(Q, tg, K, T, mask=m)
    finally:
        m.close()
    assert none is None and torch.equal(loss0, loss) and torch.equal(b0, bound) and torch.equal(rk0, rank)
    assert torch.equal(cand, ids_ref), label
    assert torch.equal(tscore, Sm[torch.arange(nq, device=DEV), tg]) and torch.equal(tscore, ts_full), label
    want_rank = torch.where((rank_full <= K) | (rank_full < 0), rank_full, torch.full_like(rank_full, K + 1))
    assert torch.equal(rank, want_rank), (label, rank, rank_full)
    Tq = np.full(nq, np.float64(np.float32(T)))
    r = SY.truncated(Sm.cpu().numpy(), nos_m, targets, Tq, K)
    for q in range(nq):
        assert np.array_equal(r["cand"][q], cand[q].cpu().numpy()[:len(r["cand"][q])]), (label, q)
    assert np.array_equal(r["rank"], rank.cpu().numpy())
    l, b, lf = (v.cpu().numpy().astype(np.float64) for v in (loss, bound, full))
    ok = np.isfinite(r["loss"])
    assert np.array_equal(np.isinf(l), ~ok) and (b[~ok] == 0).all() and not gq[torch.as_tensor(~ok, device=DEV)].any()
    el = np.abs(l[ok] - r["loss"][ok]) / np.maximum(1, np.abs(r["loss"][ok]))
    eps = 1e-5 * np.maximum(1, np.abs(lf[ok]))
    gap = lf[ok] - l[ok]
    print(f"{label}: loss rel err max {el.max():.3g}  L_full - loss in [{gap.min():.3g}, {gap.max():.3g}]  "
          f"tail_bound in [{b.min():.3g}, {b.max():.3g}]  restated bound max {r['bound'].max():.3g}")
    assert el.max() <= 1e-5, (label, el)
    assert np.allclose(b[ok], r["bound"][ok], rtol=1e-4, atol=1e-7), (label, b, r["bound"])
    assert (gap >= -eps).all() and (gap <= b[ok] * (1 + 1e-5) + eps).all(), (label, gap, b)
    Xq = Q.cpu().numpy()[ok]
    cands = cand.cpu().numpy()[ok]
    _, g64 = SS.chain_through(d64, Xq, cands, np.asarray(targets)[ok], Tq[ok])
    _, g32 = SS.chain_through(d32, Xq, cands, np.asarray(targets)[ok], Tq[ok])
    got = gq.cpu().numpy().astype(np.float64)[ok]
    # constant-loss queries (the target alone, sentences of one leaf): judged against one entry's
    # |d score / d x| / T, as test_gpu_sparse_scores.check_topk_loss does
    one = np.zeros((len(Xq), len(nos)))
    one[np.arange(len(Xq)), np.asarray(targets)[ok]] = 1.0
    scale = np.linalg.norm(Y.grad_through(d64, Xq, one), axis=1) / Tq[ok]
    flat = np.linalg.norm(g64, axis=1) <= 1e-9 * scale
    if flat.any():
        a, a_ref = np.linalg.norm(got[flat], axis=1) / scale[flat], np.linalg.norm(g32[flat], axis=1) / scale[flat]
        assert a.max() < C.rule(a_ref), (label, a, a_ref)
    if (~flat).any():
        e_ref, e = Y.rel_l2(g32[~flat], g64[~flat]), Y.rel_l2(got[~flat], g64[~flat])
        print(f"{label}: grad_q max {e.max():.3g}  E_ref max {e_ref.max():.3g}")
        assert e.max() < C.rule(e_ref), (label, e, e_ref)


@pytest.mark.parametrize("name", ["g10_grad_d24", "g1_hier_d32", "flat17"])
def test_topk_form(gpu, name, monkeypatch):
    ix, Q, nos, d64, d32 = SS.tree(gpu, name)
    Qs = Q[:6].contiguous()
    S = ix.rank_scores(Qs)
    Tsd = float(S[torch.isfinite(S)].double().std())
    flags = np.random.default_rng(21).random(len(nos)) < 0.5
    Sc = masked_scores(S, flags).cpu().numpy()
    for K in (1, 10, 64):
        for where, pos in (("inside", min(2, K - 1)), ("just outside", K), ("far outside", 10 ** 9)):
            tg = []
            for q in range(6):
                o = SY.order(Sc[q], nos)
                o = o[np.isfinite(Sc[q, o])]
                tg.append(o[min(pos, len(o) - 1)])
            tg = np.array(tg, np.int64)
            if where == "far outside":                 # one target that is not allowed among them
                tg[4] = int(np.nonzero(~flags & (nos >= 0))[0][0])
            check_topk_masked(ix, Qs, nos, d64, d32, flags, tg, Tsd, K, monkeypatch, f"{name} K={K} {where}")


@pytest.mark.parametrize("mask_path", [1, 2])
def test_topk_form_multi_mask_rows_equal_single_calls(gpu, mask_path, monkeypatch):
    """5 masks x 40 queries, an empty and an all-ones mask among them: every row of the one call
    equals the single-mask call on that query alone, bit for bit in every output."""
    t, Q, ix, S, _, temps = RC.synth(gpu, "flat")
    n = ix.n_sent
    rng = np.random.default_rng(31)
    sets = [rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.02, rng.random(n) < 0.2]
    Q40 = torch.cat([Q, Q[:7] * 1.01]).contiguous()
    moq = rng.integers(0, 5, 40)
    moq[:5] = np.arange(5)
    tg = rng.integers(0, n, 40)                        # mostly outside the top-K, some not allowed
    Sc = torch.cat([S, ix.rank_scores(Q[:7] * 1.01)]).cpu().numpy()
    for q in range(0, 40, 3):                          # every third one inside its mask's top-K
        f = sets[moq[q]]
        if f.any():
            tg[q] = np.flatnonzero(f)[np.argsort(-Sc[q, f], kind="stable")[q % 4]]
    tgt = torch.as_tensor(tg, device=DEV)
    T, K = float(temps.mean()), 10
    masks = [ix.sentence_mask(f) for f in sets]
    monkeypatch.setenv("CWQ_MASK_PATH", str(mask_path))
    try:
        multi = ix.rank_ce_topk(Q40, tgt, K, T, grad=True, masks=masks, mask_of_query=moq)
        ids, _ = ix.score_topk(Q40, K, masks=masks, mask_of_query=moq)
        assert torch.equal(multi[5], ids)
        assert int((multi[3] > 0).sum()) >= 10 and int((multi[3] == -1).sum()) >= 5
        for q in range(40):
            one = ix.rank_ce_topk(Q40[q:q + 1], tgt[q:q + 1], K, T, grad=True, mask=masks[moq[q]])
            assert all(torch.equal(a[0], b[q]) for a, b in zip(one, multi)), (mask_path, q)
    finally:
        for m in masks:
            m.close()


# ---- 10. the wrapper --------------------------------------------------------------------------
def test_wrapper(gpu, monkeypatch):
    # test_gpu_rank_ce.wrapped's wrapper: the product's own fit over the g10 corpus, its tree's scorers
    g = TG.golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], device=DEV)
    w.build_prediction_index()
    _, parent, mean, var, nos, _ = w.tree.flatten(len(w.sentences))
    mean, var, nos = np.asarray(mean, np.float32), np.asarray(var, np.float32), np.asarray(nos)
    P = Y.path_matrix(parent, nos)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    Xq = g["Xq"]
    n = len(nos)
    flags = np.random.default_rng(41).random(n) < 0.5
    S = w._index.rank_scores(torch.tensor(Xq))
    Sm = masked_scores(S, flags)
    tg = third_allowed(Sm, nos)
    labels = torch.as_tensor(tg)
    T = float(np.float32(Sm[torch.isfinite(Sm)].double().std().item()))
    md64, md32 = MaskedDense(d64, flags), MaskedDense(d32, flags)
    for reduction in ("mean", "sum", "none"):
        x64 = torch.tensor(Xq, dtype=torch.float64, requires_grad=True)
        l64 = RC.dense_loss(md64, x64, labels, T, reduction)
        (g64,) = torch.autograd.grad(l64.sum(), [x64])
        x32 = torch.tensor(Xq, dtype=torch.float32, requires_grad=True)
        l32 = RC.dense_loss(md32, x32, labels, T, reduction)
        (g32,) = torch.autograd.grad(l32.sum(), [x32])
        e_ref = Y.rel_l2(g32.numpy(), g64.numpy())
        e_ref_l = float((l32.detach().double() - l64.detach()).abs().max() / l64.detach().abs().max())
        q = torch.tensor(Xq, device=DEV).requires_grad_()
        loss = w.cobweb_ranking_loss(q, labels.to(DEV), T, reduction, allowed=flags)
        assert loss.grad_fn is not None and loss.shape == l64.shape
        loss.sum().backward()
        e = Y.rel_l2(q.grad.cpu().numpy(), g64.numpy())
        el = float((loss.detach().double().cpu() - l64.detach()).abs().max() / l64.detach().abs().max())
        print(f"wrapper allowed= {reduction}: grad max {e.max():.3g} (E_ref {e_ref.max():.3g})  loss {el:.3g} "
              f"(E_ref {e_ref_l:.3g})")
        assert e.max() <= C.rule(e_ref) and el <= C.rule(e_ref_l)
    # a kept SentenceMask is used as it is; ids, a bool tensor and a mask are the same set
    m = w.sentence_mask(flags)
    a = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", allowed=m)
    b = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", allowed=np.flatnonzero(flags))
    assert not m.closed and torch.equal(a, b)
    rank, score = w.cobweb_target_ranks(torch.tensor(Xq), labels, allowed=m)
    assert rank.dtype == torch.int64 and torch.equal(rank, C.rank_of_targets(Sm, tg, nos))
    assert torch.equal(score, S.gather(1, labels.to(DEV)[:, None])[:, 0])
    rk5, _ = w.cobweb_target_ranks(torch.tensor(Xq), labels, allowed=m, top_k=5)
    assert torch.equal(rk5, torch.where(rank <= 5, rank, torch.full_like(rank, 6)))
    lk = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", top_k=n + 3, allowed=m)
    assert torch.allclose(lk, a, rtol=1e-5, atol=1e-6)                  # K past the allowed set: the full masked loss
    # through a small encoder
    torch.manual_seed(3)
    enc = torch.nn.Linear(12, 24).to(DEV)
    feats = torch.randn(len(Xq), 12, device=DEV)
    out = w.cobweb_ranking_loss(0.1 * enc(feats) + torch.tensor(Xq, device=DEV), labels.to(DEV), T, allowed=m)
    out.backward()
    assert torch.isfinite(enc.weight.grad).all() and float(enc.weight.grad.abs().sum()) > 0
    # allowed_sets without top_k: the loop of single-set calls, rows in order; with top_k: one call
    flags2 = ~flags
    flags2[tg[::2]] = True
    soq = np.arange(len(Xq)) % 2
    soq[~flags2[tg]] = 0                               # every label is allowed in its query's set
    both = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", allowed_sets=[m, flags2], set_of_query=soq)
    one0 = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", allowed=m)
    one1 = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", allowed=flags2)
    pick = torch.as_tensor(soq == 0, device=DEV)
    assert torch.equal(both, torch.where(pick, one0, one1)) and torch.isfinite(both).all()
    rboth, _ = w.cobweb_target_ranks(torch.tensor(Xq), labels, allowed_sets=[m, flags2], set_of_query=torch.as_tensor(soq))
    r1, _ = w.cobweb_target_ranks(torch.tensor(Xq), labels, allowed=flags2)
    assert torch.equal(rboth, torch.where(pick, rank, r1))
    kboth = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", top_k=4, allowed_sets=[m, flags2], set_of_query=soq)
    k0 = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", top_k=4, allowed=m)
    k1 = w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, "none", top_k=4, allowed=flags2)
    assert torch.equal(kboth, torch.where(pick, k0, k1))
    # the errors
    for kw in (dict(allowed=m, level_weights=[1.0, 1.0]), dict(allowed=m, allowed_sets=[m], set_of_query=soq * 0),
               dict(allowed_sets=[m]), dict(set_of_query=soq), dict(allowed_sets=[m, flags2], set_of_query=soq + 5),
               dict(allowed_sets=[m, flags2], set_of_query=soq[:3]), dict(allowed=np.ones(n + 1, bool))):
        with pytest.raises(ValueError):
            w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, **kw)
        with pytest.raises(ValueError):
            w.cobweb_target_ranks(torch.tensor(Xq), labels, **kw)
    with pytest.raises(ValueError):
        w._index.rank_ce(torch.tensor(Xq), labels, T, mask=m, level_weights=[1.0])
    # a SentenceMask of an earlier index is refused; so is the C ABI's own check of a foreign mask
    other = TG.make_index(gpu, TG.setup("g1_hier_d32")[0])
    mo = other.sentence_mask(np.ones(other.n_sent, bool))
    with pytest.raises(gpu._lib.CwqError):
        w._index.rank_ce(torch.tensor(Xq), labels, T, mask=mo)
    with pytest.raises(gpu._lib.CwqError):
        w._index.rank_ce_topk(torch.tensor(Xq), labels, 4, T, mask=mo)
    mo.close()
    w.force_rebuild_index()
    with pytest.raises(ValueError):
        w.cobweb_ranking_loss(torch.tensor(Xq), labels, T, allowed=m)
    with pytest.raises(ValueError):
        w.cobweb_target_ranks(torch.tensor(Xq), labels, allowed=m)
    m.close()
