"""GPU tests of the differentiable rank scores (cwq_rank_scores_backward, autograd.py).

Yardstick: fp64 torch autograd on the CPU through the dense restatement of the reference
expression (tests/grad_yardstick.py).  Metric: per query |g - g64|_2 / |g64|_2, limit 1e-5
(the project's RTOL for scores; the reference's own fp32 autograd sits at 5e-8 .. 3e-7 by
this metric, so the limit leaves room for another summation order and none for a wrong
coefficient).  Every accuracy test prints the kernel's error and the reference's fp32 error
E_ref before it asserts."""
import os

import numpy as np
import pytest

import grad_yardstick as Y
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDENS = ["g10_grad_d24", "g1_hier_d32", "g4_twolevel_d48", "g5_hier_d384", "g2_flat_d768", "g9_interleaved_d16"]
NQ = 8


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def golden(name):
    if name.startswith("g10"):
        path = os.path.join(GOLDEN, name + ".npz")
        assert os.path.exists(path), "gradient golden missing"
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    return load_golden(name)


_cache = {}


def setup(name, weights=None):
    """(tree arrays, queries, fp64 scorer, fp32 scorer, upstream cases) of a golden, made once."""
    key = (name, None if weights is None else tuple(weights))
    if key not in _cache:
        g = golden(name)
        mean, var, parent, nos = Y.tree_arrays(g)
        Xq = (g["Xq"] if "Xq" in g else g["Q1"])[:NQ].astype(np.float32)
        P = Y.path_matrix(parent, nos, weights)
        d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
        _, cases = Y.upstreams(d64, Xq)
        _cache[key] = ((mean, var, parent, nos), Xq, d64, d32, cases)
    return _cache[key]


def make_index(pkg, arrays, weights=None):
    mean, var, parent, nos = arrays
    return pkg.index.CobwebIndex(mean, var, parent, nos, weights, device="cuda:0")


def check_case(ix, Xq, d32, G64, g64, label):
    G = G64.astype(np.float32)
    got = ix.rank_scores_backward(Xq, torch.from_numpy(G)).cpu().numpy()
    e = Y.rel_l2(got, g64)
    e_ref = Y.rel_l2(Y.grad_through(d32, Xq, G), g64)
    print(f"{label}: kernel max {e.max():.3g}  E_ref (fp32 autograd) max {e_ref.max():.3g}")
    assert np.isfinite(got).all()
    assert e.max() < Y.LIMIT, (label, e)


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_three_upstreams(gpu, name):
    arrays, Xq, d64, d32, cases = setup(name)
    ix = make_index(gpu, arrays)
    for case, (G64, g64) in cases.items():
        check_case(ix, Xq, d32, G64, g64, f"{name} {case}")


def test_g10_against_reference_recorded_grads(gpu):
    """The reference's own x.grad (fp32 autograd through its sparse path matrix)."""
    g = golden("g10_grad_d24")
    arrays = Y.tree_arrays(g)
    for tag, w in (("", None), ("_w3", list(g["weights_w3"]))):
        ix = make_index(gpu, arrays, w)
        ones = torch.ones((8, 200))
        got = ix.rank_scores_backward(g["Xq"], ones).cpu().numpy()
        assert Y.rel_l2(got, g["grad_sum" + tag]).max() < Y.LIMIT
        got = ix.rank_scores_backward(g["Xq"], torch.from_numpy(g["W"])).cpu().numpy()
        assert Y.rel_l2(got, g["grad_wsum" + tag]).max() < Y.LIMIT


@pytest.mark.parametrize("wname", ["w3", "exp", "zero"])
def test_level_weights_g1(gpu, wname):
    g = golden("g1_hier_d32")
    w = {"w3": [1.0, 2.0, 0.5], "exp": list(g["weights_exp"]), "zero": [1.0, 0.0, 1.0, 0.5]}[wname]
    arrays, Xq, d64, d32, cases = setup("g1_hier_d32", w)
    ix = make_index(gpu, arrays, w)
    for case, (G64, g64) in cases.items():
        check_case(ix, Xq, d32, G64, g64, f"g1 weights {wname} {case}")


def test_missing_sentences_nan_upstream(gpu):
    """Sentences outside the tree (node_of_sentence = -1) score -inf; their grad_out columns
    are never read: NaN there gives the gradient zeros give, bit for bit."""
    (mean, var, parent, nos), Xq, _, _, _ = setup("g1_hier_d32")
    nos = nos.copy()
    miss = np.arange(0, len(nos), 7)
    nos[miss] = -1
    ix = make_index(gpu, (mean, var, parent, nos))
    assert torch.isinf(ix.rank_scores(Xq)[:, miss]).all()
    P = Y.path_matrix(parent, nos)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    G = np.random.default_rng(3).standard_normal((len(Xq), len(nos)))
    G[:, miss] = 0.0
    Gn = G.astype(np.float32)
    Gn[:, miss] = np.nan
    g0 = ix.rank_scores_backward(Xq, torch.from_numpy(G.astype(np.float32)))
    gn = ix.rank_scores_backward(Xq, torch.from_numpy(Gn))
    assert torch.isfinite(gn).all() and torch.equal(g0, gn)
    g64 = Y.grad_through(d64, Xq, G)
    e = Y.rel_l2(gn.cpu().numpy(), g64)
    print(f"missing sentences: kernel max {e.max():.3g}  E_ref max "
          f"{Y.rel_l2(Y.grad_through(d32, Xq, G.astype(np.float32)), g64).max():.3g}")
    assert e.max() < Y.LIMIT


def synth_tree(pkg, kind):
    torch.manual_seed(0)
    if kind == "flat":      # 5,000 x 96: several slabs, a ragged last one; the root's rows split
        X = pkg.synth.synthetic_corpus(5000, 96, seed=4, device="cuda:0")
        t = pkg.synth.flat_synth(X)
    else:                   # b = 4, depth 4: 341 internal nodes, small fan-out
        X = pkg.synth.synthetic_corpus(1024, 40, seed=5, device="cuda:0")
        t = pkg.synth.balanced_synth(X, 4, 4)
    Q, _ = pkg.synth.synthetic_queries(X, 33, seed=6)
    return t, Q.contiguous()


@pytest.mark.parametrize("kind", ["flat", "balanced"])
def test_query_tiles_slab_edges_and_reproducibility(gpu, kind):
    t, Q = synth_tree(gpu, kind)
    ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
    ns = ix.n_sent
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(11)
    G = torch.randn((33, ns), generator=gen, device="cuda:0")
    full = ix.rank_scores_backward(Q, G)
    assert torch.equal(full, ix.rank_scores_backward(Q, G))            # run to run
    for nq in (1, 16, 17):
        assert torch.equal(ix.rank_scores_backward(Q[:nq], G[:nq]), full[:nq]), nq
    for qi in (0, 15, 16, 32):                                         # one query alone, bit for bit
        assert torch.equal(ix.rank_scores_backward(Q[qi:qi + 1], G[qi:qi + 1])[0], full[qi]), qi
    # accuracy on the first / last queries of each tile
    mean = torch.as_tensor(t["mean"]).cpu().numpy()
    var = torch.as_tensor(t["var"]).cpu().numpy()
    P = Y.path_matrix(t["parent"], t["node_of_sentence"], sparse=True)
    d64, d32 = Y.Dense(mean, var, P, torch.float64), Y.Dense(mean, var, P, torch.float32)
    sel = [0, 15, 16, 32]
    Xs, Gs = Q[sel].cpu().numpy(), G[sel].cpu().numpy()
    g64 = Y.grad_through(d64, Xs, Gs.astype(np.float64))
    e = Y.rel_l2(full[sel].cpu().numpy(), g64)
    print(f"synthetic {kind}: kernel max {e.max():.3g}  E_ref max {Y.rel_l2(Y.grad_through(d32, Xs, Gs), g64).max():.3g}")
    assert e.max() < Y.LIMIT


def test_full_and_compact_variance_identical(gpu):
    X = gpu.synth.synthetic_corpus(700, 48, seed=8, device="cuda:0")
    Q, _ = gpu.synth.synthetic_queries(X, 5, seed=9)
    G = torch.randn((5, 700), device="cuda:0")
    out = []
    for compact in (False, True):
        t = gpu.synth.flat_synth(X, compact=compact)
        ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
        out.append(ix.rank_scores_backward(Q, G))
    assert torch.equal(out[0], out[1])


# ---- autograd end to end -------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapped(gpu):
    """A wrapper built by the product's own fit over the g10 corpus, and the yardstick of
    its tree (flattened as the wrapper flattens it)."""
    g = golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], device="cuda:0")
    w.build_prediction_index()
    _, parent, mean, var, nos, _ = w.tree.flatten(len(w.sentences))
    mean, var = np.asarray(mean, np.float32), np.asarray(var, np.float32)
    d64 = Y.Dense(mean, var, Y.path_matrix(parent, nos), torch.float64)
    return w, g, d64


def train_loss(score_fn, q, labels, T):
    """src/training/cobweb_query_train.py:116-126."""
    ce = torch.nn.CrossEntropyLoss()
    batch_loss = []
    for b in range(q.size(0)):
        leaf_scores = score_fn(q[b])
        logits = leaf_scores.unsqueeze(0) / T
        batch_loss.append(ce(logits, labels[b].unsqueeze(0)))
    return torch.stack(batch_loss).mean()


def test_autograd_training_loss_through_encoder(gpu, wrapped):
    w, g, d64 = wrapped
    x = torch.tensor(g["Xq"][0], device="cuda:0").requires_grad_()
    assert w.cobweb_rank_scores(x, is_embedding=True).grad_fn is not None
    torch.manual_seed(2)
    enc64 = torch.nn.Linear(12, 24).double()
    with torch.no_grad():   # an encoder near the identity on the queries: embeddings inside the corpus
        enc64.weight.mul_(0.1)
    feats = torch.randn(4, 12, dtype=torch.float64)
    base = torch.tensor(g["Xq"][:4], dtype=torch.float64)
    with torch.no_grad():
        S = torch.stack([d64.scores(enc64(feats)[b] + base[b]) for b in range(4)])
    labels = torch.argsort(-S, dim=1, stable=True)[:, 2]          # not the top-1
    T = float(S.std(unbiased=False))
    loss64 = train_loss(d64.scores, enc64(feats) + base, labels, T)
    loss64.backward()
    enc = torch.nn.Linear(12, 24).to("cuda:0")
    with torch.no_grad():
        enc.weight.copy_(enc64.weight.float())
        enc.bias.copy_(enc64.bias.float())
    q = enc(feats.float().to("cuda:0")) + base.float().to("cuda:0")
    loss = train_loss(lambda e: w.cobweb_rank_scores(e, is_embedding=True), q, labels.to("cuda:0"), T)
    loss.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-4 * abs(float(loss64.detach()))
    for name, p, p64 in (("weight", enc.weight, enc64.weight), ("bias", enc.bias, enc64.bias)):
        e = Y.rel_l2(p.grad.cpu().numpy().reshape(1, -1), p64.grad.numpy().reshape(1, -1))
        print(f"encoder {name} grad: rel L2 {e.max():.3g}")
        assert e.max() < Y.LIMIT
    # the batch entry point: the same loss over one [4, n_sent] block
    enc.zero_grad()
    q = enc(feats.float().to("cuda:0")) + base.float().to("cuda:0")
    Sb = w.cobweb_rank_scores_batch(q)
    assert Sb.shape == (4, len(w.sentences)) and Sb.grad_fn is not None
    torch.nn.CrossEntropyLoss()(Sb / T, labels.to("cuda:0")).backward()
    e = Y.rel_l2(enc.weight.grad.cpu().numpy().reshape(1, -1), enc64.weight.grad.numpy().reshape(1, -1))
    assert e.max() < Y.LIMIT


def test_autograd_cpu_leaf_and_no_grad_paths(gpu, wrapped):
    w, g, d64 = wrapped
    x = torch.tensor(g["Xq"][1]).requires_grad_()                  # a CPU leaf
    s = w.cobweb_rank_scores(x, is_embedding=True)
    assert s.grad_fn is not None and s.device.type == "cuda"
    s.sum().backward()
    assert x.grad is not None and x.grad.device.type == "cpu" and x.grad.shape == x.shape
    x64 = torch.tensor(g["Xq"][1], dtype=torch.float64, requires_grad=True)
    (g64,) = torch.autograd.grad(d64.scores(x64).sum(), [x64])
    assert Y.rel_l2(x.grad.numpy()[None], g64.numpy()[None]).max() < Y.LIMIT
    # no history wanted: today's path, bit for bit
    today = w._index.rank_scores(torch.tensor(g["Xq"][1], device="cuda:0")[None])[0]
    plain = w.cobweb_rank_scores(torch.tensor(g["Xq"][1]), is_embedding=True)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, today)
    with torch.no_grad():
        ng = w.cobweb_rank_scores(x, is_embedding=True)
    assert ng.grad_fn is None and torch.equal(ng, today)
    assert torch.equal(s.detach(), today)
    # is_embedding=False cuts the graph (the reference's torch.tensor(emb))
    w.encode_func = lambda batch: [x]
    cut = w.cobweb_rank_scores("text", is_embedding=False)
    w.encode_func = lambda v: v
    assert cut.grad_fn is None and torch.equal(cut, today)


def test_backward_after_index_rebuild(gpu):
    g = golden("g10_grad_d24")
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(150)], corpus_embeddings=g["X"][:150], device="cuda:0")
    x0 = torch.tensor(g["Xq"][2], device="cuda:0").requires_grad_()
    w.cobweb_rank_scores(x0, is_embedding=True).sum().backward()
    x1 = torch.tensor(g["Xq"][2], device="cuda:0").requires_grad_()
    s = w.cobweb_rank_scores(x1, is_embedding=True)
    old = w._index
    w.add_sentences([f"s{i}" for i in range(150, 200)], g["X"][150:200])      # closes and rebuilds the index
    assert w.cobweb_rank_scores(x1.detach(), is_embedding=True).shape[0] == 200
    assert w._index is not old
    s.sum().backward()                                                          # still the old tree
    assert torch.equal(x1.grad, x0.grad)
    del s
    import gc
    gc.collect()
    assert not old._h.value                                                     # released with the graph


def test_non_default_stream_same_bits(gpu, wrapped):
    w, g, _ = wrapped
    Q = torch.tensor(g["Xq"], device="cuda:0")
    G = torch.randn((8, len(w.sentences)), device="cuda:0")

    def run():
        q = Q.clone().requires_grad_()
        s = w.cobweb_rank_scores_batch(q)
        s.backward(G)
        return s.detach(), q.grad
    s0, g0 = run()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s1, g1 = run()
    st.synchronize()
    assert torch.equal(s0, s1) and torch.equal(g0, g1)
