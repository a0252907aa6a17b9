"""GPU tests of the fused ranking loss (cwq_rank_ce): cross-entropy over all
sentence scores with its gradient, the target's score and rank, with no [nq, n_sent] tensor.

Yardsticks (tests/ce_yardstick.py, tests/grad_yardstick.py): the library's own
rank_scores for the keys, the rank and the isolated loss / coefficient checks; fp64 torch
autograd through the dense restatement of the reference expression for the whole chain, with
E_ref = the same restatement in fp32 (the reference's own arithmetic) printed beside every
kernel figure.  Targets are the third-ranked sentence, temperatures the query's score
standard deviation (grad_yardstick.upstreams) and the reference's T = 1.0."""
import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import test_gpu_grad as TG   # its goldens, cached fp64 setups and synthetic trees (made once)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


_ce_cache = {}


def ce_setup(name, weights=None):
    """TG.setup plus the targets, temperatures and fp64 / fp32 end-to-end yardsticks, once."""
    key = (name, None if weights is None else tuple(weights))
    if key not in _ce_cache:
        arrays, Xq, d64, d32, cases = TG.setup(name, weights)
        tg, temps, _ = C.targets_and_temps(d64, Xq)
        cfg = {"std": temps}
        if weights is None and name in ("g10_grad_d24", "g2_flat_d768"):
            cfg["T1"] = np.ones(len(Xq))
        ends = {}
        for tag, T in cfg.items():
            l64, g64 = C.ce_through(d64, Xq, tg, T)
            l32, g32 = C.ce_through(d32, Xq, tg, T)
            ends[tag] = (T, l64, g64, np.abs(l32 - l64) / np.abs(l64), Y.rel_l2(g32, g64))
        _ce_cache[key] = (arrays, Xq, tg, ends)
    return _ce_cache[key]


def run_checks(ix, Xq, nos, tg, ends, label):
    """Checks 1-5 for one index: keys, rank, isolated loss, isolated coefficients, end to end."""
    S = ix.rank_scores(Xq)
    Sc = S.cpu().numpy()
    tgt = torch.as_tensor(tg, device=DEV)
    want_rank = C.rank_of_targets(S, tg, nos)
    for tag, (T, l64, g64, e_l32, e_g32) in ends.items():
        # the C ABI takes one temperature per call: one call per distinct T
        loss = np.zeros(len(Xq))
        grad = np.zeros((len(Xq), ix.dim), np.float32)
        assert np.array_equal(T, C.f32(T))
        for Tv in np.unique(T):
            sel = np.nonzero(T == Tv)[0]
            seld = torch.as_tensor(sel, device=DEV)
            lo, gq, ts, rk = ix.rank_ce(Xq[sel], tg[sel], float(Tv), grad=True)
            assert torch.equal(ts, S[seld, tgt[seld]]), (label, "target_score")       # 1
            assert torch.equal(rk, want_rank[seld]), (label, "rank")                  # 2
            loss[sel] = lo.double().cpu().numpy()
            grad[sel] = gq.cpu().numpy()
        assert np.isfinite(loss).all() and np.isfinite(grad).all()
        # 3: the loss against fp64 on the library's own fp32 scores
        T32 = T
        lS = C.loss_on_scores(Sc, tg, T32)
        e3 = np.abs(loss - lS) / np.maximum(1.0, np.abs(lS))
        e3t = np.abs(C.torch_ce_fp32(Sc, tg, T32) - lS) / np.maximum(1.0, np.abs(lS))
        print(f"{label} {tag}: loss vs fp64 on own scores max {e3.max():.3g}  (torch fp32 cross_entropy {e3t.max():.3g})")
        assert e3.max() <= 1e-5, (label, tag, e3)
        # 4: the coefficients: the same tree and stream kernels fed the fp64 softmax - onehot
        G32 = torch.from_numpy(C.softmax_grad_on_scores(Sc, tg, T32).astype(np.float32))
        gB = ix.rank_scores_backward(Xq, G32).cpu().numpy()
        e4 = Y.rel_l2(grad, gB)
        print(f"{label} {tag}: grad vs backward of the fp64 softmax max {e4.max():.3g}")
        assert e4.max() < Y.LIMIT, (label, tag, e4)
        # 5: end to end against fp64 autograd of the whole loss
        e5 = Y.rel_l2(grad, g64)
        e5l = np.abs(loss - l64) / np.abs(l64)
        print(f"{label} {tag}: end to end grad max {e5.max():.3g} (E_ref {e_g32.max():.3g})  "
              f"loss max {e5l.max():.3g} (E_ref {e_l32.max():.3g})")
        assert e5.max() <= C.rule(e_g32), (label, tag, e5, e_g32)
        assert e5l.max() <= C.rule(e_l32), (label, tag, e5l, e_l32)
    return S, want_rank


def check_topk(ix, Xq, tg, rank):
    for k in (1, 10):
        ids, _ = ix.score_topk(Xq, k)
        inside = (ids == torch.as_tensor(tg, device=DEV)[:, None]).any(1)
        assert torch.equal(inside, rank <= k), k


@pytest.mark.parametrize("name", TG.GOLDENS)
def test_goldens(gpu, name):
    arrays, Xq, tg, ends = ce_setup(name)
    ix = TG.make_index(gpu, arrays)
    _, rank = run_checks(ix, Xq, arrays[3], tg, ends, name)
    check_topk(ix, Xq, tg, rank)


@pytest.mark.parametrize("wname", ["w3", "exp", "zero"])
def test_level_weights_g1(gpu, wname):
    g = TG.golden("g1_hier_d32")
    w = {"w3": [1.0, 2.0, 0.5], "exp": list(g["weights_exp"]), "zero": [1.0, 0.0, 1.0, 0.5]}[wname]
    arrays, Xq, tg, ends = ce_setup("g1_hier_d32", w)
    run_checks(TG.make_index(gpu, arrays, w), Xq, arrays[3], tg, ends, f"g1 weights {wname}")


_synth = {}


def synth(gpu, kind):
    """TG.synth_tree's trees (flat 5,000 x 96: three parts of 2,048 rows, the last ragged;
    balanced b = 4 depth 4), their index and 33 queries: three query tiles, the last ragged."""
    if kind not in _synth:
        t, Q = TG.synth_tree(gpu, kind)
        ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
        S = ix.rank_scores(Q)
        tg = torch.argsort(-S, dim=1, stable=True)[:, 2].contiguous()
        _synth[kind] = (t, Q, ix, S, tg, C.f32(S.double().std(dim=1, unbiased=False).cpu().numpy()))
    return _synth[kind]


@pytest.mark.parametrize("kind", ["flat", "balanced"])
def test_synthetic_trees(gpu, kind):
    t, Q, ix, S, tg, temps = synth(gpu, kind)
    sel = [0, 15, 16, 32]          # the first / last queries of each tile
    nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
    mean = torch.as_tensor(t["mean"]).cpu().numpy()
    var = torch.as_tensor(t["var"]).cpu().numpy()
    P = Y.path_matrix(t["parent"], nos, sparse=True)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    Xs, tgs, Ts = Q[sel].cpu().numpy(), tg[sel].cpu().numpy(), temps[sel]
    l64, g64 = C.ce_through(d64, Xs, tgs, Ts)
    l32, g32 = C.ce_through(d32, Xs, tgs, Ts)
    ends = {"std": (Ts, l64, g64, np.abs(l32 - l64) / np.abs(l64), Y.rel_l2(g32, g64))}
    _, rank = run_checks(ix, Xs, nos, tgs, ends, f"synthetic {kind}")
    check_topk(ix, Xs, tgs, rank)
    # every query of the batch: keys and ranks
    _, _, ts, rk = ix.rank_ce(Q, tg, 1.0)
    assert torch.equal(ts, S.gather(1, tg[:, None])[:, 0])
    assert torch.equal(rk, C.rank_of_targets(S, tg.cpu().numpy(), nos))


def test_rank_equal_keys_in_different_leaves(gpu):
    """A flat tree in which 200 rows are exact copies of other rows: equal keys in different
    leaves, ordered by node index.  Targets: the earlier and the later copy."""
    X = gpu.synth.synthetic_corpus(3000, 32, seed=14, device=DEV).clone()
    X[2800:3000] = X[100:300]
    t = gpu.synth.flat_synth(X)
    ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
    nos = np.asarray(torch.as_tensor(t["node_of_sentence"]).cpu())
    Q = (X[100:140] + 0.01 * torch.randn((40, 32), device=DEV, generator=torch.Generator(DEV).manual_seed(1))).contiguous()
    S = ix.rank_scores(Q)
    early = np.arange(100, 140)
    late = early + 2700
    assert torch.equal(S[:, early], S[:, late])                      # the copies' keys are equal bits
    assert np.all(nos[early] < nos[late])
    out = {}
    for tag, tg in (("early", early), ("late", late)):
        _, _, ts, rk = ix.rank_ce(Q, tg)
        assert torch.equal(rk, C.rank_of_targets(S, tg, nos)), tag
        assert torch.equal(ts, S[torch.arange(40, device=DEV), torch.as_tensor(tg, device=DEV)])
        check_topk(ix, Q, tg, rk)
        out[tag] = rk
    assert torch.equal(out["late"], out["early"] + 1)                # the query's own copy pair: ranks 1 and 2
    assert out["early"].min() == 1


def test_rank_inside_multi_sentence_leaves(gpu):
    """g10: sentences of one leaf share its key; the later sentence id ranks after the earlier."""
    arrays, Xq, _, _ = ce_setup("g10_grad_d24")
    nos = arrays[3]
    ix = TG.make_index(gpu, arrays)
    S = ix.rank_scores(Xq)
    nodes, counts = np.unique(nos[nos >= 0], return_counts=True)
    multi = nodes[counts > 1]
    assert len(multi) >= 3
    for nd in multi:
        sids = np.nonzero(nos == nd)[0]
        ranks = []
        for s in sids:
            tg = np.full(len(Xq), s, np.int64)
            _, _, _, rk = ix.rank_ce(Xq, tg)
            assert torch.equal(rk, C.rank_of_targets(S, tg, nos)), (nd, s)
            ranks.append(rk)
        for a, b in zip(ranks, ranks[1:]):
            assert torch.equal(b, a + 1), nd


def test_sentences_outside_the_tree(gpu):
    """g1 with every 7th sentence removed: the loss is the loss over the remaining columns; a
    target that is removed, negative or >= n_sent gives +inf / a zero row / -inf / -1 and
    leaves its neighbours' bits alone."""
    (mean, var, parent, nos), Xq, _, _, _ = TG.setup("g1_hier_d32")
    nos = nos.copy()
    miss = np.arange(0, len(nos), 7)
    nos[miss] = -1
    ix = TG.make_index(gpu, (mean, var, parent, nos))
    S = ix.rank_scores(Xq)
    assert torch.isinf(S[:, miss]).all()
    keep = np.nonzero(nos >= 0)[0]
    Sc = S.cpu().numpy()
    tg = torch.argsort(-S, dim=1, stable=True)[:, 2].cpu().numpy()
    T = float(np.float32(Sc[:, keep].astype(np.float64).std()))
    loss, gq, ts, rk = ix.rank_ce(Xq, tg, T, grad=True)
    l64 = C.loss_on_scores(Sc[:, keep], np.searchsorted(keep, tg), T)
    e = np.abs(loss.double().cpu().numpy() - l64) / np.maximum(1.0, np.abs(l64))
    print(f"missing sentences: loss vs fp64 over the remaining columns max {e.max():.3g}")
    assert e.max() <= 1e-5
    assert torch.equal(rk, C.rank_of_targets(S, tg, nos))
    G32 = torch.from_numpy(C.softmax_grad_on_scores(Sc, tg, T).astype(np.float32))
    e4 = Y.rel_l2(gq.cpu().numpy(), ix.rank_scores_backward(Xq, G32).cpu().numpy())
    assert e4.max() < Y.LIMIT
    for bad in (int(miss[1]), -5, len(nos)):
        tb = tg.copy()
        tb[3] = bad
        lb, gb, tsb, rkb = ix.rank_ce(Xq, tb, T, grad=True)
        assert float(lb[3]) == float("inf") and float(tsb[3]) == float("-inf") and int(rkb[3]) == -1, bad
        assert not gb[3].any(), bad
        ok = torch.arange(len(Xq), device=DEV) != 3
        for a, b in ((lb, loss), (gb, gq), (tsb, ts), (rkb, rk)):
            assert torch.equal(a[ok], b[ok]), bad


def test_batch_and_chunk_independence(gpu, monkeypatch):
    """Flat 5,000 x 96, nq = 33: a query alone gives the bits it gives in the batch; two runs
    are equal; and under CWQ_WS_BUDGET_MB=1 the batch repeated to 330 queries -- the smallest
    chunk the library makes is 128 queries, so three chunks, the last ragged -- gives every
    copy the same bits again."""
    t, Q, ix, S, tg, temps = synth(gpu, "flat")
    T = float(temps.mean())
    full = ix.rank_ce(Q, tg, T, grad=True)
    again = ix.rank_ce(Q, tg, T, grad=True)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    fwd = ix.rank_ce(Q, tg, T)
    assert fwd[1] is None and all(torch.equal(fwd[i], full[i]) for i in (0, 2, 3))
    for qi in range(33):
        one = ix.rank_ce(Q[qi:qi + 1], tg[qi:qi + 1], T, grad=True)
        assert all(torch.equal(a[0], b[qi]) for a, b in zip(one, full)), qi
    monkeypatch.setenv("CWQ_WS_BUDGET_MB", "1")
    small = ix.rank_ce(Q, tg, T, grad=True)
    assert all(torch.equal(a, b) for a, b in zip(small, full))
    rep = ix.rank_ce(Q.repeat(10, 1), tg.repeat(10), T, grad=True)
    assert all(torch.equal(a, b.repeat(10, *([1] * (b.dim() - 1)))) for a, b in zip(rep, full))


# ---- autograd end to end -------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapped(gpu):
    """A wrapper built by the product's own fit over the g10 corpus, and the fp64 / fp32
    yardsticks of its tree (flattened as the wrapper flattens it)."""
    g = TG.golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], device=DEV)
    w.build_prediction_index()
    _, parent, mean, var, nos, _ = w.tree.flatten(len(w.sentences))
    mean, var = np.asarray(mean, np.float32), np.asarray(var, np.float32)
    P = Y.path_matrix(parent, nos)
    return w, g, Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32), np.asarray(nos)


def dense_loss(dense, q, labels, T, reduction):
    ce = torch.nn.CrossEntropyLoss(reduction=reduction)
    return ce(torch.stack([dense.scores(q[b]) for b in range(q.shape[0])]) / T, labels)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_autograd_ranking_loss(gpu, wrapped, reduction):
    w, g, d64, d32, _ = wrapped
    Xq = g["Xq"]
    tg, temps, _ = C.targets_and_temps(d64, Xq)
    T = float(C.f32(temps.mean()))
    labels = torch.as_tensor(tg)
    x64 = torch.tensor(Xq, dtype=torch.float64, requires_grad=True)
    l64 = dense_loss(d64, x64, labels, T, reduction)
    (g64,) = torch.autograd.grad(l64, [x64])
    x32 = torch.tensor(Xq, dtype=torch.float32, requires_grad=True)
    l32 = dense_loss(d32, x32, labels, T, reduction)
    (g32,) = torch.autograd.grad(l32, [x32])
    e_ref = Y.rel_l2(g32.numpy(), g64.numpy())
    l32, l64 = float(l32.detach()), float(l64.detach())
    e_ref_l = abs(l32 - l64) / abs(l64)
    q = torch.tensor(Xq, device=DEV).requires_grad_()
    loss = w.cobweb_ranking_loss(q, labels.to(DEV), T, reduction)
    assert loss.grad_fn is not None and loss.dim() == 0
    loss.backward()
    q2 = torch.tensor(Xq, device=DEV).requires_grad_()             # the unfused path on this library
    loss2 = torch.nn.functional.cross_entropy(w.cobweb_rank_scores_batch(q2) / T, labels.to(DEV), reduction=reduction)
    loss2.backward()
    e, e2 = Y.rel_l2(q.grad.cpu().numpy(), g64.numpy()), Y.rel_l2(q2.grad.cpu().numpy(), g64.numpy())
    el, el2 = (abs(float(v.detach()) - l64) / abs(l64) for v in (loss, loss2))
    print(f"ranking loss {reduction}: fused grad max {e.max():.3g}, rank_scores + F.cross_entropy {e2.max():.3g}, "
          f"E_ref {e_ref.max():.3g}; loss {el:.3g} / {el2:.3g} / E_ref {e_ref_l:.3g}")
    assert e.max() <= C.rule(e_ref) and e2.max() <= C.rule(e_ref)
    assert el <= C.rule(e_ref_l) and el2 <= C.rule(e_ref_l)
    none = w.cobweb_ranking_loss(torch.tensor(Xq, device=DEV), labels.to(DEV), T, "none")
    assert none.shape == (len(Xq),) and none.grad_fn is None
    red = none.double().mean() if reduction == "mean" else none.double().sum()
    assert abs(float(red) - float(loss.detach())) <= 1e-6 * abs(float(red))
    with pytest.raises(ValueError):
        w.cobweb_ranking_loss(q, labels, T, "max")


def test_autograd_through_encoder(gpu, wrapped):
    """FixedDocsRankingLoss through a small nn.Linear query encoder (test_gpu_grad.py's)."""
    w, g, d64, d32, _ = wrapped
    torch.manual_seed(2)
    enc64 = torch.nn.Linear(12, 24).double()
    with torch.no_grad():
        enc64.weight.mul_(0.1)
    feats = torch.randn(4, 12, dtype=torch.float64)
    base = torch.tensor(g["Xq"][:4], dtype=torch.float64)
    with torch.no_grad():
        emb = enc64(feats) + base
        S = torch.stack([d64.scores(emb[b]) for b in range(4)])
    labels = torch.argsort(-S, dim=1, stable=True)[:, 2]
    T = float(C.f32(float(S.std(unbiased=False))))
    loss64 = dense_loss(d64, enc64(feats) + base, labels, T, "mean")
    loss64.backward()
    enc32 = torch.nn.Linear(12, 24)
    enc = torch.nn.Linear(12, 24).to(DEV)
    with torch.no_grad():
        for e_ in (enc32, enc):
            e_.weight.copy_(enc64.weight.float())
            e_.bias.copy_(enc64.bias.float())
    dense_loss(d32, enc32(feats.float()) + base.float(), labels, T, "mean").backward()
    loss = w.cobweb_ranking_loss(enc(feats.float().to(DEV)) + base.float().to(DEV), labels.to(DEV), temperature=T)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-4 * abs(float(loss64.detach()))
    for name, p, p32, p64 in (("weight", enc.weight, enc32.weight, enc64.weight), ("bias", enc.bias, enc32.bias, enc64.bias)):
        e = Y.rel_l2(p.grad.cpu().numpy().reshape(1, -1), p64.grad.numpy().reshape(1, -1))
        e_ref = Y.rel_l2(p32.grad.numpy().reshape(1, -1), p64.grad.numpy().reshape(1, -1))
        print(f"encoder {name} grad through the fused loss: rel L2 {e.max():.3g} (E_ref {e_ref.max():.3g})")
        assert e.max() <= C.rule(e_ref)


def test_cpu_leaf_no_grad_and_target_ranks(gpu, wrapped, monkeypatch):
    w, g, d64, _, nos = wrapped
    Xq = g["Xq"]
    tg, temps, _ = C.targets_and_temps(d64, Xq)
    labels = torch.as_tensor(tg)
    x = torch.tensor(Xq).requires_grad_()                          # a CPU leaf
    loss = w.cobweb_ranking_loss(x, labels, float(temps.mean()))
    assert loss.device.type == "cuda" and loss.grad_fn is not None
    loss.backward()
    assert x.grad is not None and x.grad.device.type == "cpu" and x.grad.shape == x.shape
    dev = torch.tensor(Xq, device=DEV).requires_grad_()
    w.cobweb_ranking_loss(dev, labels.to(DEV), float(temps.mean())).backward()
    assert torch.equal(x.grad, dev.grad.cpu())
    # no gradient wanted: the library call gets no grad_q
    seen = []
    real = w._index.rank_ce

    def spy(q, target, temperature=1.0, grad=False):
        out = real(q, target, temperature, grad)
        seen.append((grad, out[1]))
        return out
    monkeypatch.setattr(w._index, "rank_ce", spy)
    with torch.no_grad():
        ng = w.cobweb_ranking_loss(x, labels, 1.0)
    plain = w.cobweb_ranking_loss(torch.tensor(Xq), labels, 1.0)
    assert ng.grad_fn is None and plain.grad_fn is None and torch.equal(ng, plain)
    rank, score = w.cobweb_target_ranks(torch.tensor(Xq), labels)
    assert [s for s in seen] == [(False, None)] * 3
    w.cobweb_ranking_loss(dev, labels.to(DEV), 1.0)
    assert seen[-1][0] is True and seen[-1][1] is not None
    monkeypatch.undo()
    S = w._index.rank_scores(torch.tensor(Xq))
    assert rank.dtype == torch.int64 and torch.equal(rank, C.rank_of_targets(S, tg, nos))
    assert torch.equal(score, S.gather(1, labels.to(DEV)[:, None])[:, 0])
    for k in (1, 10):
        ids, _ = w._index.score_topk(torch.tensor(Xq), k)
        assert torch.equal((ids == labels.to(DEV)[:, None]).any(1), rank <= k)


def test_two_streams_equal_serial(gpu):
    """Two calls on two torch streams back to back, no host synchronisation between them:
    the second waits for the first's use of the handle workspace (tests/test_gpu_streams.py)."""
    X = gpu.synth.synthetic_corpus(20_000, 128, seed=31, device=DEV)
    t = gpu.synth.flat_synth(X)
    ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
    Q1, _ = gpu.synth.synthetic_queries(X, 2048, seed=32)   # a long first call: 128 query tiles
    Q2, _ = gpu.synth.synthetic_queries(X, 33, seed=33)
    gen = torch.Generator(device=DEV).manual_seed(5)
    t1 = torch.randint(0, 20_000, (2048,), device=DEV, generator=gen)
    t2 = torch.randint(0, 20_000, (33,), device=DEV, generator=gen)
    T = 50.0
    ref1 = ix.rank_ce(Q1, t1, T, grad=True)
    ref2 = ix.rank_ce(Q2, t2, T, grad=True)
    ref3 = ix.rank_ce(Q2, t2, T)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            a = ix.rank_ce(Q1, t1, T, grad=True)
        with torch.cuda.stream(s2):
            b = ix.rank_ce(Q2, t2, T, grad=True)
        with torch.cuda.stream(s1):
            c = ix.rank_ce(Q2, t2, T)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, ref1))
        assert all(torch.equal(x, y) for x, y in zip(b, ref2))
        assert c[1] is None and all(torch.equal(c[i], ref3[i]) for i in (0, 2, 3))
    ix.close()
