"""GPU tests of the call-time level weights and their gradient (cwq_rank_scores_w,
cwq_rank_scores_backward_w, cwq_rank_ce_w).

Forward identity: an index built with default weights and given `level_weights=w` returns,
bit for bit, what an index built with w returns without them.  Weight gradient: per query
|g - g64|_2 / |g64|_2 over the [n_w] vector against fp64 autograd through the dense restatement
with the weights a torch leaf (tests/lw_yardstick.py); the limit is ce_yardstick.rule(E_ref),
E_ref the same restatement in fp32 on the same queries, and both are printed per tree.
Determinism, the edge cases, the autograd surface and the wrapper follow."""
import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import lp_yardstick as L
import lw_yardstick as W
import test_gpu_grad as TG   # its goldens and synthetic trees

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TREES = ["g10_grad_d24", "g1_hier_d32", "g9_interleaved_d16", "g4_twolevel_d48", "g2_flat_d768", "ifit5", "ifit17"]
WNAMES = list(W.WEIGHTS)


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def w32(wname):
    return torch.tensor(W.WEIGHTS[wname], dtype=torch.float32)


def built_weights(w):
    return [float(x) for x in torch.as_tensor(w).float()]


_trees, _refs = {}, {}


def ifit_arrays(pkg, D):
    """About 300 rows fitted by the product at a dimension that leaves the last 16-wide chunk
    partly filled: leaves at several depths, five leaves of two exact copies."""
    rng = np.random.default_rng(700 + D)
    X = L.corpus(D, 300, 3, rng)
    for j in range(5):
        X[299 - j] = X[3 * j]
    w = pkg.CobwebWrapper(corpus=[f"s{i}" for i in range(300)], corpus_embeddings=X, device=DEV)
    w.build_prediction_index()
    _, parent, mean, var, nos, _ = w.tree.flatten(300)
    Xq = L.queries(X, rng, TG.NQ)
    return (np.asarray(mean, np.float32), np.asarray(var, np.float32), np.asarray(parent, np.int64),
            np.asarray(nos, np.int64)), Xq


def tree(pkg, name):
    """(tree arrays, 8 queries, fp64 / fp32 scorers, the index built with default weights), once."""
    if name not in _trees:
        if name.startswith("ifit"):
            arrays, Xq = ifit_arrays(pkg, int(name[4:]))
        else:
            g = TG.golden(name)
            arrays = Y.tree_arrays(g)
            Xq = (g["Xq"] if "Xq" in g else g["Q1"])[:TG.NQ].astype(np.float32)
        A = W.depth_matrices(arrays[2], arrays[3])
        d64, d32 = (W.DenseW(arrays[0], arrays[1], A, dt) for dt in (torch.float64, torch.float32))
        _trees[name] = (arrays, Xq, d64, d32, TG.make_index(pkg, arrays))
    return _trees[name]


def ref(pkg, name, wname):
    """Targets and temperatures under the weights in use, and the fp64 / fp32 gradients of the
    cross-entropy and of the three upstream cases, once."""
    if (name, wname) not in _refs:
        arrays, Xq, d64, d32, _ = tree(pkg, name)
        w = W.WEIGHTS[wname]
        tg, temps, _ = W.targets_and_temps(d64, Xq, w)
        _, _, gw64 = W.ce_through(d64, Xq, tg, temps, w)
        _, _, gw32 = W.ce_through(d32, Xq, tg, temps, w)
        ups = {}
        for case, G in W.upstreams(d64, Xq, w, tg, temps).items():
            u64 = W.grad_through(d64, Xq, G, w)[1]
            u32 = W.grad_through(d32, Xq, G.astype(np.float32), w)[1]
            ups[case] = (G, u64, Y.rel_l2(u32, u64))
        _refs[(name, wname)] = (tg, temps, gw64, Y.rel_l2(gw32, gw64), ups)
    return _refs[(name, wname)]


# ---- forward identity ---------------------------------------------------------------------
@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("name", TREES)
def test_forward_identity(gpu, name, wname):
    arrays, Xq, _, _, ix0 = tree(gpu, name)
    tg, temps, _, _, _ = ref(gpu, name, wname)
    T = float(C.f32(temps.mean()))
    w = w32(wname)
    ixw = TG.make_index(gpu, arrays, built_weights(w))
    G = torch.randn((len(Xq), ix0.n_sent), generator=torch.Generator().manual_seed(3))
    for wt in (w, w.to(DEV)):                                   # a host vector and a device one
        assert torch.equal(ix0.rank_scores(Xq, level_weights=wt), ixw.rank_scores(Xq))
        got = ix0.rank_ce(Xq, tg, T, grad=True, level_weights=wt)
        want = ixw.rank_ce(Xq, tg, T, grad=True)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(ix0.rank_scores_backward(Xq, G, level_weights=wt), ixw.rank_scores_backward(Xq, G))
    # asking for the weight gradient changes nothing else
    got5 = ix0.rank_ce(Xq, tg, T, grad=True, level_weights=w, weight_grad=True)
    assert len(got5) == 5 and all(torch.equal(a, b) for a, b in zip(got5[:4], want))
    gq, gw = ix0.rank_scores_backward(Xq, G, level_weights=w, weight_grad=True)
    assert torch.equal(gq, ixw.rank_scores_backward(Xq, G)) and gw.shape == (len(Xq), len(w))
    # no call-time weights (None: the old entry points; an empty vector: NULL through the new
    # ones): the index's own weights, today's bits
    e = torch.empty(0)
    for ix in (ix0, ixw):
        assert torch.equal(ix.rank_scores(Xq, level_weights=None), ix.rank_scores(Xq))
        assert torch.equal(ix.rank_scores(Xq, level_weights=e), ix.rank_scores(Xq))
        today = ix.rank_ce(Xq, tg, T, grad=True)
        for lw in (None, e):
            assert all(torch.equal(a, b) for a, b in zip(ix.rank_ce(Xq, tg, T, grad=True, level_weights=lw), today))
        assert torch.equal(ix.rank_scores_backward(Xq, G, level_weights=e), ix.rank_scores_backward(Xq, G))
    ixw.close()


# ---- the weight gradient against fp64 -----------------------------------------------------
@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("name", TREES)
def test_weight_gradient_against_fp64(gpu, name, wname):
    """Measured on an MI355X: see DESIGN.md §4.15 (kernel and E_ref per tree and weight vector)."""
    arrays, Xq, d64, _, ix = tree(gpu, name)
    tg, temps, gw64, e_ref, ups = ref(gpu, name, wname)
    w = w32(wname)
    nq, n_w = len(Xq), len(w)
    # the cross-entropy: one call per temperature (the C ABI takes one per call)
    got = np.zeros((nq, n_w), np.float32)
    for qi in range(nq):
        out = ix.rank_ce(Xq[qi:qi + 1], tg[qi:qi + 1], float(temps[qi]), grad=True, level_weights=w, weight_grad=True)
        got[qi] = out[4][0].cpu().numpy()
    e = Y.rel_l2(got, gw64)
    lim = C.rule(e_ref)
    print(f"{name} {wname}: rank_ce grad_w max {e.max():.3g}  E_ref max {e_ref.max():.3g}  limit {lim:.3g}")
    assert np.isfinite(got).all()
    nl = d64.nl
    assert not got[:, nl:].any(), "columns beyond the tree's depth must be exactly zero"
    assert e.max() <= lim, (name, wname, e, e_ref)
    if name == "g4_twolevel_d48":   # every leaf at depth 2: the depth-0 component is exactly 0 in truth
        r0 = np.abs(got[:, 0]) / np.linalg.norm(gw64, axis=1)
        print(f"{name} {wname}: depth-0 component / |g64| max {r0.max():.3g}")
        assert r0.max() <= lim
    # the three upstream cases through rank_scores autograd, per query
    for case, (G, u64, e_ref_u) in ups.items():
        G32 = torch.from_numpy(G.astype(np.float32)).to(DEV)
        gotu = np.zeros((nq, n_w), np.float32)
        for qi in range(nq):
            wp = torch.nn.Parameter(w.to(DEV).clone())
            ix.rank_scores(torch.from_numpy(Xq[qi:qi + 1]).to(DEV), level_weights=wp).backward(G32[qi:qi + 1])
            gotu[qi] = wp.grad.cpu().numpy()
        _, direct = ix.rank_scores_backward(Xq, G32, level_weights=w, weight_grad=True)
        assert np.array_equal(direct.cpu().numpy(), gotu), (name, wname, case)   # alone = its row in the batch
        eu = Y.rel_l2(gotu, u64)
        print(f"{name} {wname} {case}: grad_w max {eu.max():.3g}  E_ref max {e_ref_u.max():.3g}")
        assert not gotu[:, nl:].any()
        assert eu.max() <= C.rule(e_ref_u), (name, wname, case, eu, e_ref_u)


# ---- determinism --------------------------------------------------------------------------
_synth = {}


def synth(gpu, kind):
    if kind not in _synth:
        t, Q = TG.synth_tree(gpu, kind)
        ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device=DEV)
        w = torch.tensor([1.0, 2.0, 0.5, 0.25, 1.5], device=DEV)
        S = ix.rank_scores(Q, level_weights=w)
        tg = torch.argsort(-S, dim=1, stable=True)[:, 2].contiguous()
        T = float(C.f32(float(S.double().std(dim=1, unbiased=False).mean())))
        _synth[kind] = (Q, ix, w, tg, T)
    return _synth[kind]


@pytest.mark.parametrize("kind", ["flat", "balanced"])
def test_batch_chunk_and_run_independence(gpu, kind, monkeypatch):
    """33 queries (three query tiles, the last ragged) over 5,000 x 96 flat (20 parts of 256
    rows, the last ragged) and over the balanced depth-4 tree: a query alone gives the bits of
    its row in the batch; two runs are equal; 330 queries under CWQ_WS_BUDGET_MB=1 (chunks of
    128 queries, the last ragged) give every copy the same bits."""
    Q, ix, w, tg, T = synth(gpu, kind)
    full = ix.rank_ce(Q, tg, T, grad=True, level_weights=w, weight_grad=True)
    again = ix.rank_ce(Q, tg, T, grad=True, level_weights=w, weight_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert full[4].abs().sum() > 0
    only_w = ix.rank_ce(Q, tg, T, level_weights=w, weight_grad=True)         # without grad_q
    assert only_w[1] is None and torch.equal(only_w[4], full[4])
    G = torch.randn((33, ix.n_sent), device=DEV, generator=torch.Generator(DEV).manual_seed(11))
    bfull = ix.rank_scores_backward(Q, G, level_weights=w, weight_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(bfull, ix.rank_scores_backward(Q, G, level_weights=w, weight_grad=True)))
    nog = ix.rank_scores_backward(Q, G, level_weights=w, weight_grad=True, query_grad=False)
    assert nog[0] is None and torch.equal(nog[1], bfull[1])
    for qi in range(33):
        one = ix.rank_ce(Q[qi:qi + 1], tg[qi:qi + 1], T, grad=True, level_weights=w, weight_grad=True)
        assert all(torch.equal(a[0], b[qi]) for a, b in zip(one, full)), qi
        b1 = ix.rank_scores_backward(Q[qi:qi + 1], G[qi:qi + 1], level_weights=w, weight_grad=True)
        assert all(torch.equal(a[0], b[qi]) for a, b in zip(b1, bfull)), qi
    monkeypatch.setenv("CWQ_WS_BUDGET_MB", "1")
    rep = ix.rank_ce(Q.repeat(10, 1), tg.repeat(10), T, grad=True, level_weights=w, weight_grad=True)
    assert all(torch.equal(a, b.repeat(10, *([1] * (b.dim() - 1)))) for a, b in zip(rep, full))
    brep = ix.rank_scores_backward(Q.repeat(10, 1), G.repeat(10, 1), level_weights=w, weight_grad=True)
    assert all(torch.equal(a, b.repeat(10, 1)) for a, b in zip(brep, bfull))


# ---- edge cases ---------------------------------------------------------------------------
def test_invalid_target_gives_a_zero_row(gpu):
    arrays, Xq, _, _, ix = tree(gpu, "g1_hier_d32")
    tg, temps, _, _, _ = ref(gpu, "g1_hier_d32", "w3")
    w, T = w32("w3"), float(C.f32(temps.mean()))
    good = ix.rank_ce(Xq, tg, T, grad=True, level_weights=w, weight_grad=True)
    for bad in (-5, ix.n_sent):
        tb = tg.copy()
        tb[3] = bad
        out = ix.rank_ce(Xq, tb, T, grad=True, level_weights=w, weight_grad=True)
        assert float(out[0][3]) == float("inf") and not out[4][3].any() and not out[1][3].any()
        ok = torch.arange(len(Xq), device=DEV) != 3
        assert all(torch.equal(a[ok], b[ok]) for a, b in zip(out, good)), bad


def test_more_weights_than_levels(gpu):
    """g2 has three levels: of ten weights seven are unused, their columns exactly zero, and
    everything else equals the three-weight call's."""
    arrays, Xq, d64, _, ix = tree(gpu, "g2_flat_d768")
    tg, temps, _, _, _ = ref(gpu, "g2_flat_d768", "exp10")
    T = float(C.f32(temps.mean()))
    w10, nl = w32("exp10"), d64.nl
    assert nl == 3
    a = ix.rank_ce(Xq, tg, T, grad=True, level_weights=w10, weight_grad=True)
    b = ix.rank_ce(Xq, tg, T, grad=True, level_weights=w10[:nl], weight_grad=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    assert torch.equal(a[4][:, :nl], b[4]) and not a[4][:, nl:].any() and (a[4][:, :nl] != 0).all()
    with pytest.raises(ValueError):
        ix.rank_ce(Xq, tg, T, level_weights=torch.ones(65))
    with pytest.raises(ValueError):
        ix.rank_ce(Xq, tg, T, weight_grad=True)


# ---- the autograd surface -----------------------------------------------------------------
def test_autograd_surface(gpu, monkeypatch):
    arrays, Xq, _, _, ix = tree(gpu, "g10_grad_d24")
    tg, temps, _, _, _ = ref(gpu, "g10_grad_d24", "w3")
    T = float(C.f32(temps.mean()))
    from rag_cobweb_amd.autograd import rank_ce_autograd
    w = w32("w3")
    per_q = ix.rank_ce(Xq, tg, T, grad=True, level_weights=w, weight_grad=True)
    want_w = per_q[4].double().sum(0)
    G = torch.randn((len(Xq), ix.n_sent), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    bq, bw = ix.rank_scores_backward(Xq, G, level_weights=w, weight_grad=True)
    for make in (lambda: torch.nn.Parameter(w.double().clone()),             # CPU fp64
                 lambda: torch.nn.Parameter(w.to(DEV).clone())):             # device fp32
        for q_grad, w_grad in ((True, False), (False, True), (True, True)):
            wp = make().requires_grad_(w_grad)
            q = torch.tensor(Xq, device=DEV).requires_grad_(q_grad)
            loss, ts, rk = rank_ce_autograd(ix, q, tg, T, wp)
            assert loss.grad_fn is not None and torch.equal(loss.detach(), per_q[0])
            assert torch.equal(ts, per_q[2]) and torch.equal(rk, per_q[3])
            loss.sum().backward()
            assert (q.grad is not None) == q_grad and (wp.grad is not None) == w_grad
            if q_grad:
                assert torch.equal(q.grad, per_q[1])
            if w_grad:
                assert wp.grad.shape == wp.shape and wp.grad.device == wp.device and wp.grad.dtype == wp.dtype
                assert torch.allclose(wp.grad.double().cpu(), want_w.cpu(), rtol=1e-6, atol=0.0)
            # rank_scores: the same surface
            wp = make().requires_grad_(w_grad)
            q = torch.tensor(Xq, device=DEV).requires_grad_(q_grad)
            S = ix.rank_scores(q, level_weights=wp)
            assert S.grad_fn is not None and torch.equal(S.detach(), ix.rank_scores(Xq, level_weights=w))
            S.backward(G)
            assert (q.grad is not None) == q_grad and (wp.grad is not None) == w_grad
            if q_grad:
                assert torch.equal(q.grad, bq)
            if w_grad:
                assert wp.grad.shape == wp.shape and wp.grad.device == wp.device and wp.grad.dtype == wp.dtype
                assert torch.allclose(wp.grad.double().cpu(), bw.double().sum(0).cpu(), rtol=1e-6, atol=0.0)
    # under no_grad: no gradient pass, the same values
    seen = []
    real_ce, real_bw = ix.rank_ce, ix.rank_scores_backward

    def spy_ce(*a, **k):
        seen.append(("ce", k.get("grad", False), k.get("weight_grad", False)))
        return real_ce(*a, **k)

    def spy_bw(*a, **k):
        seen.append(("bw",))
        return real_bw(*a, **k)
    monkeypatch.setattr(ix, "rank_ce", spy_ce)
    monkeypatch.setattr(ix, "rank_scores_backward", spy_bw)
    wp = torch.nn.Parameter(w.to(DEV).clone())
    q = torch.tensor(Xq, device=DEV).requires_grad_()
    with torch.no_grad():
        loss, _, _ = rank_ce_autograd(ix, q, tg, T, wp)
        S = ix.rank_scores(q, level_weights=wp)
    assert loss.grad_fn is None and S.grad_fn is None
    assert torch.equal(loss, per_q[0]) and torch.equal(S, ix.rank_scores(Xq, level_weights=w))
    assert seen == [("ce", False, False)]
    monkeypatch.undo()


# ---- through the wrapper ------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True])
def test_wrapper_sweep_and_learn(gpu, resident):
    g = TG.golden("g10_grad_d24")
    wr = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], device=DEV,
                           resident=resident)
    Q = torch.tensor(g["Xq"], device=DEV)
    S0 = wr.cobweb_rank_scores_batch(Q)
    labels = torch.argsort(-S0, dim=1, stable=True)[:, 2].contiguous()
    T = float(C.f32(float(S0.double().std(dim=1, unbiased=False).mean())))
    base = wr.cobweb_ranking_loss(Q, labels, T)
    assert torch.equal(wr.cobweb_ranking_loss(Q, labels, T, level_weights=None), base)
    assert torch.equal(wr.cobweb_rank_scores_batch(Q, level_weights=None), S0)
    # twenty SGD steps on the weights alone lower the batch loss
    wp = torch.nn.Parameter(torch.ones(6, device=DEV))
    first = wr.cobweb_ranking_loss(Q, labels, T, level_weights=wp)
    assert torch.equal(first.detach(), base)                  # ones: the default weights
    first.backward()
    opt = torch.optim.SGD([wp], lr=0.02 / float(wp.grad.abs().max()))
    losses = [float(first.detach())]
    for _ in range(20):
        opt.zero_grad()
        loss = wr.cobweb_ranking_loss(Q, labels, T, level_weights=wp)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    final = float(wr.cobweb_ranking_loss(Q, labels, T, level_weights=wp.detach()))
    print(f"resident={resident}: loss {losses[0]:.6g} -> {final:.6g} after 20 SGD steps on w")
    assert final < losses[0]
    # the learned weights against a rebuild with them
    w = wp.detach().clone()
    sweep_loss = wr.cobweb_ranking_loss(Q, labels, T, reduction="none", level_weights=w)
    sweep_rank, sweep_score = wr.cobweb_target_ranks(Q, labels, level_weights=w)
    sweep_S = wr.cobweb_rank_scores_batch(Q, level_weights=w)
    old = wr._index
    wr.set_level_weights(w.tolist())
    assert torch.equal(wr.cobweb_ranking_loss(Q, labels, T, reduction="none"), sweep_loss)
    assert wr._index is not old
    rank, score = wr.cobweb_target_ranks(Q, labels)
    assert torch.equal(rank, sweep_rank) and torch.equal(score, sweep_score)
    assert torch.equal(wr.cobweb_rank_scores_batch(Q), sweep_S)
