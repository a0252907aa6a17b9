"""GPU tests of the sparse differentiable scores (cwq_score_pairs, cwq_score_pairs_backward,
cwq_rank_ce_topk).

Yardsticks: the library's own dense paths for bits (rank_scores columns, score_topk rows,
rank_ce's rank and loss), and fp64 -- the truncated loss restated on the library's fp32 scores
(tests/sparse_yardstick.py; limit 1e-5 relative to max(1, |loss|), §4.12's) and autograd through
the dense scorer of grad_yardstick (limit ce_yardstick.rule = max(1e-5, 4 E_ref), E_ref the same
chain in fp32).  Every accuracy test prints its figures before it asserts."""
import gc
import os

import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import sparse_yardstick as SY
import test_gpu_grad as TG

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
TREES = ["g10_grad_d24", "g1_hier_d32", "g9_interleaved_d16", "g4_twolevel_d48", "g2_flat_d768", "flat17", "balanced"]


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


_trees = {}


def tree(pkg, name):
    """(index, queries [33, D] on the device, node_of_sentence, dense fp64 / fp32 scorers) of a
    tree, made once.  Goldens lose every 7th sentence (sentences outside the tree)."""
    if name in _trees:
        return _trees[name]
    if name in ("flat17", "balanced"):
        if name == "flat17":     # 5,000 x 17: a partly filled last 16-wide chunk
            X = pkg.synth.synthetic_corpus(5000, 17, seed=21, device=DEV)
            t = pkg.synth.flat_synth(X)
            Q, _ = pkg.synth.synthetic_queries(X, 33, seed=22)
        else:
            t, Q = TG.synth_tree(pkg, "balanced")
        mean, var = torch.as_tensor(t["mean"]).cpu().numpy(), torch.as_tensor(t["var"]).cpu().numpy()
        parent = np.asarray(torch.as_tensor(t["parent"]).cpu())
        nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu()).copy()
        Q = Q.contiguous()
        sparse = True
    else:
        (mean, var, parent, nos), Xq, _, _, _ = TG.setup(name)
        nos = nos.copy()
        rng = np.random.default_rng(5)
        Q = np.concatenate([Xq] + [Xq + 0.05 * rng.standard_normal(Xq.shape).astype(np.float32) for _ in range(4)])[:33]
        Q = torch.from_numpy(np.ascontiguousarray(Q)).to(DEV)
        sparse = False
    nos[::7] = -1
    ix = pkg.index.CobwebIndex(mean, var, parent, nos, device=DEV)
    P = Y.path_matrix(parent, nos, sparse=sparse)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    _trees[name] = (ix, Q, nos, d64, d32)
    return _trees[name]


def mixed_ids(ns, nq, m, seed):
    """Valid ids with -1, out-of-range ids, sentences outside the tree (every 7th) and duplicates."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ns, (nq, m))
    ids[rng.random((nq, m)) < 0.1] = -1
    ids[rng.random((nq, m)) < 0.05] = ns + 3
    ids[rng.random((nq, m)) < 0.05] = -(2 ** 40)
    ids[rng.random((nq, m)) < 0.1] = 7 * (rng.integers(0, ns) // 7)
    if m > 2:
        ids[:, m - 1] = ids[:, 0]
        ids[:, m // 2] = ids[:, 0]
    return ids.astype(np.int64)


def gather_columns(S, ids, nos):
    ns = S.shape[1]
    t = torch.as_tensor(ids, device=S.device)
    ok = (t >= 0) & (t < ns)
    out = S.gather(1, t.clamp(0, ns - 1))
    return torch.where(ok, out, torch.full_like(out, -np.inf))


# ---- 1. pair scores ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", TREES)
def test_pair_scores_are_rank_scores_columns(gpu, name):
    ix, Q, nos, _, _ = tree(gpu, name)
    S = ix.rank_scores(Q[:17])
    for nq in (1, 5, 17):
        for m in (1, 63, 64, 65, 130):
            ids = mixed_ids(ix.n_sent, nq, m, 100 * nq + m)
            got = ix.score_pairs(Q[:nq], ids)
            want = gather_columns(S[:nq], ids, nos)
            assert got.shape == (nq, m) and torch.equal(got, want), (name, nq, m)
            bad = (ids < 0) | (ids >= ix.n_sent) | (nos[ids.clip(0, ix.n_sent - 1)] < 0)
            assert torch.isinf(got[torch.as_tensor(bad, device=DEV)]).all()
            assert torch.isfinite(got[torch.as_tensor(~bad, device=DEV)]).all()


# ---- 2. sparse backward -----------------------------------------------------------------------
def dense_upstream(ids, g, nos):
    """The sparse upstream scattered into [nq, n_sent] in fp64 (duplicates add, invalid dropped)."""
    G = np.zeros((ids.shape[0], len(nos)))
    for q in range(ids.shape[0]):
        for sid, gj in zip(ids[q], g[q]):
            if 0 <= sid < len(nos) and nos[sid] >= 0:
                G[q, sid] += gj
    return G


@pytest.mark.parametrize("name", TREES)
def test_sparse_backward_against_dense_and_fp64(gpu, name):
    ix, Q, nos, d64, d32 = tree(gpu, name)
    nq, m = 8, 40
    ids = mixed_ids(ix.n_sent, nq, m, 7)
    rng = np.random.default_rng(8)
    g = rng.standard_normal((nq, m)).astype(np.float32)
    valid = (ids >= 0) & (ids < ix.n_sent) & (nos[ids.clip(0, ix.n_sent - 1)] >= 0)
    G64 = dense_upstream(ids, g.astype(np.float64), nos)
    Xq = Q[:nq].cpu().numpy()
    g64 = Y.grad_through(d64, Xq, G64)
    e_ref = Y.rel_l2(Y.grad_through(d32, Xq, G64.astype(np.float32)), g64)
    gn = g.copy()
    gn[~valid] = np.nan                         # never read
    got = ix.score_pairs_backward(Q[:nq], ids, gn)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ix.score_pairs_backward(Q[:nq], ids, g))
    dense = ix.rank_scores_backward(Q[:nq], torch.from_numpy(G64.astype(np.float32)))
    e, e_dense = Y.rel_l2(got.cpu().numpy(), g64), Y.rel_l2(dense.cpu().numpy(), g64)
    print(f"{name}: sparse max {e.max():.3g}  dense path max {e_dense.max():.3g}  E_ref max {e_ref.max():.3g}")
    assert e.max() < C.rule(e_ref), (name, e)
    # duplicates = one entry with the summed upstream
    ids1 = np.stack([np.nonzero(G64[q])[0][:12] for q in range(nq)])
    g1 = np.stack([G64[q, ids1[q]] for q in range(nq)]).astype(np.float32)
    dup = ix.score_pairs_backward(Q[:nq], np.concatenate([ids1, ids1], 1), np.concatenate([0.25 * g1, 0.75 * g1], 1))
    one64 = Y.grad_through(d64, Xq, dense_upstream(ids1, g1.astype(np.float64), nos))
    assert Y.rel_l2(dup.cpu().numpy(), one64).max() < C.rule(e_ref)


def test_sparse_backward_entry_limit(gpu):
    ix, Q, nos, d64, d32 = tree(gpu, "g1_hier_d32")
    rng = np.random.default_rng(3)
    ids = rng.integers(0, ix.n_sent, (2, 4096))
    g = rng.standard_normal((2, 4096)).astype(np.float32)
    got = ix.score_pairs_backward(Q[:2], ids, g)
    G64 = dense_upstream(ids, g.astype(np.float64), nos)
    Xq = Q[:2].cpu().numpy()
    g64 = Y.grad_through(d64, Xq, G64)
    e_ref = Y.rel_l2(Y.grad_through(d32, Xq, G64.astype(np.float32)), g64)
    e = Y.rel_l2(got.cpu().numpy(), g64)
    print(f"m = 4096: sparse max {e.max():.3g}  E_ref max {e_ref.max():.3g}")
    assert e.max() < C.rule(e_ref)
    with pytest.raises(gpu._lib.CwqError) as ei:
        ix.score_pairs_backward(Q[:2], rng.integers(0, ix.n_sent, (2, 4097)), np.zeros((2, 4097), np.float32))
    assert ei.value.rc == gpu._lib.CWQ_ERR_ARG and "cwq_rank_scores_backward" in str(ei.value)
    assert ix.score_pairs(Q[:2], rng.integers(0, ix.n_sent, (2, 4097))).shape == (2, 4097)   # the forward takes any m


# ---- 3. differentiable top-k ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g10_grad_d24", "flat17", "balanced"])
def test_topk_scores_carry_the_gradient(gpu, name):
    ix, Q, nos, _, _ = tree(gpu, name)
    for k in (1, 10, 64):
        ids0, sc0 = ix.score_topk(Q[:9], k)
        q = Q[:9].clone().requires_grad_()
        ids, sc = ix.score_topk(q, k)
        assert torch.equal(ids, ids0) and torch.equal(sc, sc0)
        assert sc.grad_fn is not None and not ids.requires_grad
        W = torch.randn(sc.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(k))
        (sc * W).sum().backward()
        assert torch.equal(q.grad, ix.score_pairs_backward(Q[:9], ids0, W)), (name, k)
        with torch.no_grad():
            ids1, sc1 = ix.score_topk(q, k)
        assert sc1.grad_fn is None and torch.equal(sc1, sc0) and torch.equal(ids1, ids0)


def test_topk_gradient_through_masks_and_padded_tail(gpu):
    ix, Q, nos, _, _ = tree(gpu, "g1_hier_d32")
    ns = ix.n_sent
    few = ix.sentence_mask(np.arange(1, 6))             # at most 5 allowed: a -1 / -inf tail at k = 10
    half = ix.sentence_mask(np.arange(ns) % 2 == 0)
    try:
        moq = np.arange(9) % 2
        for kw in ({"mask": few}, {"mask": half}, {"masks": [few, half], "mask_of_query": moq}):
            ids0, sc0 = ix.score_topk(Q[:9], 10, **kw)
            q = Q[:9].clone().requires_grad_()
            ids, sc = ix.score_topk(q, 10, **kw)
            assert torch.equal(ids, ids0) and torch.equal(sc, sc0) and sc.grad_fn is not None
            W = torch.randn(sc.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
            torch.where(ids >= 0, sc * W, torch.zeros_like(sc)).sum().backward()
            assert torch.isfinite(q.grad).all()
            assert torch.equal(q.grad, ix.score_pairs_backward(Q[:9], ids0, W))
            if kw.get("mask") is few:
                assert (ids0[:, 5:] == -1).all() and torch.isinf(sc0[:, 5:]).all()
                Wn = W.clone()
                Wn[:, 5:] = float("nan")                # the padded tail contributes nothing
                assert torch.equal(q.grad, ix.score_pairs_backward(Q[:9], ids0, Wn))
    finally:
        few.close()
        half.close()
    with pytest.raises(ValueError):                     # the sparse backward's entry limit, said at the call
        ix.score_topk(Q[:1].clone().requires_grad_(), 4097)
    assert ix.score_topk(Q[:1], 4097)[1].grad_fn is None
    # k > n_sent on a plain call: the tail past the sentences of the tree
    ids0, sc0 = ix.score_topk(Q[:3], ns + 5)
    q = Q[:3].clone().requires_grad_()
    ids, sc = ix.score_topk(q, ns + 5)
    torch.where(ids >= 0, sc, torch.zeros_like(sc)).sum().backward()
    ones = np.zeros((3, ns), np.float32)
    ones[:, nos >= 0] = 1
    dense = ix.rank_scores_backward(Q[:3], torch.from_numpy(ones))
    assert (ids0[:, -5:] == -1).all() and torch.isfinite(q.grad).all()
    assert Y.rel_l2(q.grad.cpu().numpy(), dense.cpu().numpy().astype(np.float64)).max() < Y.LIMIT


# ---- 4. top-K loss ----------------------------------------------------------------------------
def chain_through(dense, Xq, cands, targets, temps):
    """(loss, d loss / d x) of the truncated cross-entropy over given candidate sets by autograd
    through the dense scorer in its own dtype."""
    dt = dense.M.dtype
    L, G = [], []
    for q in range(len(Xq)):
        x = torch.tensor(Xq[q], dtype=dt, requires_grad=True)
        t = int(targets[q])
        Cq = [int(c) for c in cands[q] if c >= 0]
        if t not in Cq:
            Cq.append(t)
        s = dense.scores(x)
        loss = torch.logsumexp(s[Cq] / float(temps[q]), 0) - s[t] / float(temps[q])
        (gx,) = torch.autograd.grad(loss, [x])
        L.append(float(loss.detach()))
        G.append(gx.numpy())
    return np.array(L), np.stack(G)


def check_topk_loss(ix, Q, nos, d64, d32, targets, T, K, label, grads=True):
    nq = Q.shape[0]
    tg = torch.as_tensor(np.asarray(targets, np.int64), device=DEV)
    S = ix.rank_scores(Q)
    ids_ref, _ = ix.score_topk(Q, K)
    full, _, ts_full, rank_full = ix.rank_ce(Q, tg, T)
    with_grad = K + 1 <= 4096                          # the backward's entry limit applies to K + 1
    loss, gq, tscore, rank, bound, cand = ix.rank_ce_topk(Q, tg, K, T, grad=with_grad)
    assert torch.equal(cand, ids_ref), label
    assert torch.equal(tscore, S[torch.arange(nq, device=DEV), tg]) and torch.equal(tscore, ts_full), label
    want_rank = torch.where(rank_full <= K, rank_full, torch.full_like(rank_full, K + 1))
    assert torch.equal(rank, want_rank), (label, rank, rank_full)
    r = SY.truncated(S.cpu().numpy(), nos, targets, np.full(nq, np.float64(np.float32(T))), K)
    for q in range(nq):
        assert np.array_equal(r["cand"][q], cand[q].cpu().numpy()[:len(r["cand"][q])]), (label, q)
    assert np.array_equal(r["rank"], rank.cpu().numpy())
    l, b, lf = loss.cpu().numpy().astype(np.float64), bound.cpu().numpy().astype(np.float64), full.cpu().numpy().astype(np.float64)
    el = np.abs(l - r["loss"]) / np.maximum(1, np.abs(r["loss"]))
    eps = 1e-5 * np.maximum(1, np.abs(lf))
    gap = lf - l
    print(f"{label}: loss rel err max {el.max():.3g}  L_full - loss in [{gap.min():.3g}, {gap.max():.3g}]  "
          f"tail_bound in [{b.min():.3g}, {b.max():.3g}]  restated bound max {r['bound'].max():.3g}")
    assert el.max() <= 1e-5, (label, el)
    assert np.allclose(b, r["bound"], rtol=1e-4, atol=1e-7), (label, b, r["bound"])
    assert (gap >= -eps).all() and (gap <= b * (1 + 1e-5) + eps).all(), (label, gap, b)
    n_tree = int((nos >= 0).sum())
    if K >= n_tree:
        assert (b == 0).all() and (np.abs(gap) <= eps).all()
    # forward only: the same bits
    loss0, none, ts0, rk0, b0, c0 = ix.rank_ce_topk(Q, tg, K, T)
    assert none is None and (gq is not None) == with_grad and torch.equal(loss0, loss) and torch.equal(b0, bound) and torch.equal(rk0, rank)
    if grads and with_grad:
        Xq = Q.cpu().numpy()
        temps = np.full(nq, np.float64(np.float32(T)))
        cands = cand.cpu().numpy()
        _, g64 = chain_through(d64, Xq, cands, targets, temps)
        _, g32 = chain_through(d32, Xq, cands, targets, temps)
        got = gq.cpu().numpy().astype(np.float64)
        # A candidate set whose scores are all one value (the target alone; sentences of one leaf;
        # copies of one row) has a constant loss: the fp64 gradient is zero and there is no relative
        # error to take.  Such a query is judged against the size of the terms that cancel, one
        # entry's |d score / d x| / T, by the same limit.
        one = np.zeros((nq, len(nos)))
        one[np.arange(nq), np.asarray(targets)] = 1.0
        scale = np.linalg.norm(Y.grad_through(d64, Xq, one), axis=1) / temps
        flat = np.linalg.norm(g64, axis=1) <= 1e-9 * scale
        if flat.any():
            a, a_ref = np.linalg.norm(got[flat], axis=1) / scale[flat], np.linalg.norm(g32[flat], axis=1) / scale[flat]
            print(f"{label}: {int(flat.sum())} constant-loss queries: |grad_q| / term max {a.max():.3g}  fp32 autograd {a_ref.max():.3g}")
            assert a.max() < C.rule(a_ref), (label, a, a_ref)
        if (~flat).any():
            e_ref = Y.rel_l2(g32[~flat], g64[~flat])
            e = Y.rel_l2(got[~flat], g64[~flat])
            print(f"{label}: grad_q max {e.max():.3g}  E_ref max {e_ref.max():.3g}")
            assert e.max() < C.rule(e_ref), (label, e, e_ref)
    return loss, gq, tscore, rank, bound, cand


def targets_by_rank(ix, Q, nos, pos):
    """Per query the sentence at 0-based position pos of the library's own ranking (clipped)."""
    S = ix.rank_scores(Q).cpu().numpy()
    out = []
    for q in range(len(S)):
        o = SY.order(S[q], nos)
        out.append(o[min(pos, len(o) - 1)])
    return np.array(out, np.int64), S


@pytest.mark.parametrize("name", TREES)
def test_topk_loss(gpu, name):
    ix, Q, nos, d64, d32 = tree(gpu, name)
    Qs = Q[:6].contiguous()
    S = ix.rank_scores(Qs)
    Tsd = float(S[torch.isfinite(S)].double().std())
    n_tree = int((nos >= 0).sum())
    for K in (1, 10, 64, ix.n_sent + 5):
        for where, pos in (("inside", min(2, K - 1)), ("just outside", K), ("far outside", 10 ** 9)):
            if K > n_tree and where != "inside":
                continue
            targets, _ = targets_by_rank(ix, Qs, nos, pos)
            for T in (Tsd, 1.0):
                out = check_topk_loss(ix, Qs, nos, d64, d32, targets, T, K, f"{name} K={K} {where} T={T:.3g}")
                if K == 1 and where == "inside":      # C is the target alone: g = (1/1 - 1)/T, exactly zero
                    assert (out[1] == 0).all()


def test_topk_loss_cut_splits_a_multi_sentence_leaf(gpu):
    """g10: a query at a multi-sentence leaf's mean ranks that leaf's sentences first; K = 1 cuts
    the leaf, and the target is its second sentence (rank 2 = K + 1, score = s_K)."""
    arrays, _, d64, d32, _ = TG.setup("g10_grad_d24")
    mean, var, parent, nos = arrays
    ix = TG.make_index(gpu, arrays)
    nodes, counts = np.unique(nos[nos >= 0], return_counts=True)
    multi = nodes[counts > 1][:4]
    assert len(multi) >= 3
    Q = torch.from_numpy(np.ascontiguousarray(mean[multi])).to(DEV)
    S = ix.rank_scores(Q).cpu().numpy()
    targets, keep = [], []
    for q, nd in enumerate(multi):
        o = SY.order(S[q], nos)
        if nos[o[0]] == nos[o[1]]:
            keep.append(q)
            targets.append(o[1])
    assert keep
    Q = Q[keep].contiguous()
    loss, gq, ts, rank, bound, cand = check_topk_loss(ix, Q, nos, d64, d32, np.array(targets), 1.0, 1, "g10 split leaf",
                                                       grads=False)
    assert (rank == 2).all()
    # C is two sentences of one leaf: equal scores, loss = log 2 whatever the query, and the two
    # upstream entries 1/2 and 1/2 - 1 of the one row cancel exactly -- a zero gradient, no
    # relative error to take
    assert torch.allclose(loss, torch.full_like(loss, float(np.log(2.0))), rtol=1e-6, atol=0) and (gq == 0).all()
    # K = 2 takes the whole pair and a third candidate: the gradient through fp64 again
    t3 = np.array([next(s for s in SY.order(S[q], nos) if nos[s] != multi[q]) for q in keep])   # the best other leaf
    check_topk_loss(ix, Q, nos, d64, d32, t3, 1.0, 2, "g10 leaf pair + third")
    _, sc = ix.score_topk(Q, 1)
    assert torch.equal(ts, sc[:, 0])                    # the target's key is the top-1's: one leaf


def test_topk_loss_equal_keys_in_different_leaves(gpu):
    X = gpu.synth.synthetic_corpus(3000, 32, seed=14, device=DEV).clone()
    X[2800:3000] = X[100:300]
    t = gpu.synth.flat_synth(X)
    ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
    nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
    mean, var = torch.as_tensor(t["mean"]).cpu().numpy(), torch.as_tensor(t["var"]).cpu().numpy()
    P = Y.path_matrix(np.asarray(torch.as_tensor(t["parent"]).cpu()), nos, sparse=True)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    Q = (X[100:112] + 0.01 * torch.randn((12, 32), device=DEV, generator=torch.Generator(DEV).manual_seed(1))).contiguous()
    early = np.arange(100, 112)
    for K in (1, 2, 10):
        for tag, tg in (("early", early), ("late", early + 2700)):
            out = check_topk_loss(ix, Q, nos, d64, d32, tg, 1.0, K, f"equal keys K={K} {tag}")
            _, _, _, rank_full = ix.rank_ce(Q, tg)
            assert torch.equal(out[3], rank_full.clamp(max=K + 1))


def test_topk_loss_invalid_targets(gpu):
    ix, Q, nos, d64, d32 = tree(gpu, "g1_hier_d32")
    Qs = Q[:8].contiguous()
    good, _ = targets_by_rank(ix, Qs, nos, 4)
    tg = good.copy()
    tg[1], tg[4], tg[6] = -1, ix.n_sent + 7, 7          # sentence 7 is outside the tree
    bad = np.array([1, 4, 6])
    ok = np.array([0, 2, 3, 5, 7])
    for K in (3, 10):
        loss, gq, ts, rank, bound, cand = ix.rank_ce_topk(Qs, tg, K, 0.7, grad=True)
        assert torch.isinf(loss[bad]).all() and (loss[bad] > 0).all()
        assert (gq[bad] == 0).all() and torch.isinf(ts[bad]).all() and (ts[bad] < 0).all()
        assert (rank[bad] == -1).all() and (bound[bad] == 0).all()
        assert torch.equal(cand, ix.score_topk(Qs, K)[0])
        ref = ix.rank_ce_topk(Qs[ok].contiguous(), good[ok], K, 0.7, grad=True)
        for a, b in zip((loss, gq, ts, rank, bound, cand), ref):
            assert torch.equal(a[ok], b)
        check_topk_loss(ix, Qs[ok].contiguous(), nos, d64, d32, good[ok], 0.7, K, f"neighbours of invalid targets K={K}")


# ---- 5. independence --------------------------------------------------------------------------
def all_three(ix, Q, ids, g, tg, K):
    return (ix.score_pairs(Q, ids), ix.score_pairs_backward(Q, ids, g)) + tuple(
        x for x in ix.rank_ce_topk(Q, tg, K, 0.9, grad=True))


@pytest.mark.parametrize("name", ["flat17", "balanced", "g2_flat_d768"])
def test_alone_in_a_batch_chunked_and_on_a_stream(gpu, name):
    """330 queries under a 1 MiB workspace budget: a chunk is the budget over the bytes per query,
    rounded down to a multiple of 128 queries (at least 128), so the call splits where a query
    needs more than 1 MiB / 384 = 2.7 KiB -- g2 (DP = 768: 3 KiB of padded query alone, 9 KiB in
    the backward) and the balanced tree (341 internal nodes: 2.9 KiB), not flat17."""
    ix, Q, nos, _, _ = tree(gpu, name)
    if name != "flat17":   # the forward's chunk, at its smallest bytes per query, is below the call
        per_q = (ix.dim + 31) // 32 * 32 * 4 + 2 * max(ix.info["internal_nodes"], 1) * 4
        assert (2 ** 20) // per_q // 128 * 128 < 330
    ids = torch.as_tensor(mixed_ids(ix.n_sent, 33, 20, 4), device=DEV)
    g = torch.randn((33, 20), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    tg = torch.as_tensor(targets_by_rank(ix, Q, nos, 12)[0], device=DEV)
    full = all_three(ix, Q, ids, g, tg, 10)
    again = all_three(ix, Q, ids, g, tg, 10)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for qi in range(33):
        one = all_three(ix, Q[qi:qi + 1], ids[qi:qi + 1], g[qi:qi + 1], tg[qi:qi + 1], 10)
        assert all(torch.equal(a[0], b[qi]) for a, b in zip(one, full)), qi
    rep = lambda x: x.repeat((10,) + (1,) * (x.dim() - 1)).contiguous()
    os.environ["CWQ_WS_BUDGET_MB"] = "1"
    try:
        big = all_three(ix, rep(Q), rep(ids), rep(g), rep(tg), 10)
    finally:
        del os.environ["CWQ_WS_BUDGET_MB"]
    assert all(torch.equal(a, rep(b)) for a, b in zip(big, full))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = all_three(ix, Q, ids, g, tg, 10)
    st.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(other, full))


# ---- 6. wrapper -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapped(gpu):
    g = TG.golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], device=DEV)
    w.build_prediction_index()
    _, parent, mean, var, nos, _ = w.tree.flatten(len(w.sentences))
    mean, var = np.asarray(mean, np.float32), np.asarray(var, np.float32)
    P = Y.path_matrix(parent, nos)
    return w, g, np.asarray(nos), Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)


def test_wrapper_topk_loss_through_an_encoder(gpu, wrapped):
    w, g, nos, d64, d32 = wrapped
    K, T = 10, 0.8
    torch.manual_seed(2)
    enc64 = torch.nn.Linear(12, 24).double()
    with torch.no_grad():
        enc64.weight.mul_(0.1)
    feats = torch.randn(4, 12, dtype=torch.float64)
    base = torch.tensor(g["Xq"][:4], dtype=torch.float64)
    enc = torch.nn.Linear(12, 24).to(DEV)
    with torch.no_grad():
        enc.weight.copy_(enc64.weight.float())
        enc.bias.copy_(enc64.bias.float())
    q = enc(feats.float().to(DEV)) + base.float().to(DEV)
    labels, _ = targets_by_rank(w._index, q.detach().contiguous(), nos, 14)      # outside the top 10
    loss = w.cobweb_ranking_loss(q, torch.as_tensor(labels), temperature=T, top_k=K)
    assert loss.grad_fn is not None
    loss.backward()
    cands = w._index.score_topk(q.detach().contiguous(), K)[0].cpu().numpy()

    def chain(dense, encoder):
        dt = dense.M.dtype
        for p in encoder.parameters():
            p.grad = None
        qq = encoder(feats.to(dt)) + base.to(dt)
        tot = 0
        for b in range(4):
            Cq = [int(c) for c in cands[b]] + ([int(labels[b])] if labels[b] not in cands[b] else [])
            s = dense.scores(qq[b])
            tot = tot + torch.logsumexp(s[Cq] / T, 0) - s[int(labels[b])] / T
        (tot / 4).backward()
        return float(tot.detach() / 4), [p.grad.numpy().reshape(1, -1).copy() for p in encoder.parameters()]
    l64, g64 = chain(d64, enc64)
    enc32 = torch.nn.Linear(12, 24)
    with torch.no_grad():
        enc32.weight.copy_(enc64.weight.float())
        enc32.bias.copy_(enc64.bias.float())
    _, g32 = chain(d32, enc32)
    assert abs(float(loss.detach()) - l64) <= 1e-5 * max(1, abs(l64))
    for name, p, a64, a32 in zip(("weight", "bias"), enc.parameters(), g64, g32):
        e, e_ref = Y.rel_l2(p.grad.cpu().numpy().reshape(1, -1), a64), Y.rel_l2(a32, a64)
        print(f"encoder {name} grad through top_k={K}: rel L2 {e.max():.3g}  E_ref {e_ref.max():.3g}")
        assert e.max() < C.rule(e_ref)


def test_wrapper_keywords_and_candidates(gpu, wrapped):
    w, g, nos, d64, _ = wrapped
    Q = torch.tensor(g["Xq"], device=DEV)
    labels, _ = targets_by_rank(w._index, Q, nos, 14)
    labels = torch.as_tensor(labels, device=DEV)
    # top_k=None: the call without the keyword, bit for bit
    assert torch.equal(w.cobweb_ranking_loss(Q, labels, 0.8, "none", top_k=None), w.cobweb_ranking_loss(Q, labels, 0.8, "none"))
    r0, s0 = w.cobweb_target_ranks(Q, labels)
    r1, s1 = w.cobweb_target_ranks(Q, labels, top_k=None)
    assert torch.equal(r0, r1) and torch.equal(s0, s1)
    for K in (5, 14, 15, 64):
        rk, sk = w.cobweb_target_ranks(Q, labels, top_k=K)
        assert torch.equal(rk, r0.clamp(max=K + 1)) and torch.equal(sk, s0)
    with pytest.raises(ValueError):
        w.cobweb_ranking_loss(Q, labels, top_k=5, level_weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        w.cobweb_target_ranks(Q, labels, top_k=5, level_weights=[1.0, 2.0])
    # candidates: a no-grad path and a grad path; a CPU leaf gets its gradient on the CPU
    ids = torch.as_tensor(mixed_ids(len(w.sentences), 8, 12, 9))
    S = w.cobweb_rank_scores_batch(Q)
    plain = w.cobweb_score_candidates(Q, ids)
    assert plain.grad_fn is None and torch.equal(plain, gather_columns(S, ids.numpy(), nos))
    x = torch.tensor(g["Xq"]).requires_grad_()
    sc = w.cobweb_score_candidates(x, ids)
    assert sc.grad_fn is not None and torch.equal(sc.detach(), plain)
    Wt = torch.randn(sc.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    torch.where(torch.isfinite(sc), sc * Wt, torch.zeros_like(sc)).sum().backward()
    assert x.grad.device.type == "cpu" and torch.equal(x.grad, w._index.score_pairs_backward(Q, ids, Wt).cpu())
    # predict_batch scores: differentiable, indices not
    xb = Q.clone().requires_grad_()
    pid, psc = w.cobweb_predict_batch(xb, 5)
    pid0, psc0 = w.cobweb_predict_batch(Q, 5)
    assert psc.grad_fn is not None and psc0.grad_fn is None and torch.equal(pid, pid0) and torch.equal(psc, psc0)


def test_sparse_backward_after_index_rebuild(gpu):
    g = TG.golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(150)], corpus_embeddings=g["X"][:150], device=DEV)
    ids = torch.arange(0, 40, device=DEV)[None, :]
    x0 = torch.tensor(g["Xq"][2:3], device=DEV).requires_grad_()
    w.cobweb_score_candidates(x0, ids).sum().backward()
    x1 = torch.tensor(g["Xq"][2:3], device=DEV).requires_grad_()
    s = w.cobweb_score_candidates(x1, ids)
    x2 = torch.tensor(g["Xq"][2:3], device=DEV).requires_grad_()
    _, ps = w.cobweb_predict_batch(x2, 5)
    x3 = torch.tensor(g["Xq"][2:3], device=DEV).requires_grad_()
    _, ps3 = w.cobweb_predict_batch(x3, 5)
    ps3.sum().backward()
    old = w._index
    w.add_sentences([f"s{i}" for i in range(150, 200)], g["X"][150:200])      # closes and rebuilds the index
    assert w._index is not old
    s.sum().backward()                                                          # still the old tree
    ps.sum().backward()
    assert torch.equal(x1.grad, x0.grad) and torch.equal(x2.grad, x3.grad)
    del s, ps, ps3
    gc.collect()
    assert not old._h.value                                                     # released with the graphs
