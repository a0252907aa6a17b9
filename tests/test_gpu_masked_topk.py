"""Masked Fast top-k (cwq_score_topk_masked): for every mask the result is the
unmasked full Fast ranking with the disallowed sentences removed, cut to k -- ids AND scores
bit for bit.

Reference on synthetic trees: the exact full ranking, set_filter(0) + score_topk(Q, n_sent),
filtered in numpy.  On the reference goldens: the fixture's reference-generated rank_scores
through topk_equiv / RTOL.  Every case runs on all three settings of CWQ_MASK_PATH (1 over-fetch
first, 2 gathered scan only, 0 automatic) and checks the path cwq_last_mask_stats reports."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import HIER, RTOL, index_from_golden, rel_err, topk_equiv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = [1, 2, 0]


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def flat_index(pkg, X, nos=None):
    fs = pkg.synth.flat_synth(X)
    return pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"] if nos is None else nos,
                                 device="cuda:0")


def full_ranking(ix, Q):
    """The exact full ranking of every query: (ids, scores) [nq, n_sent] numpy, -1 / -inf past
    the sentences in the tree."""
    ix.set_filter(0)
    ids, sc = ix.score_topk(Q, ix.n_sent)
    ix.set_filter(-1)
    return ids.cpu().numpy(), sc.cpu().numpy()


def expected(full, allowed, k):
    """The full ranking without the disallowed sentences, cut to k, padded with -1 / -inf."""
    fid, fsc = full
    allowed = np.asarray(allowed, bool)
    nq = fid.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    sc = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        keep = (fid[q] >= 0) & allowed[np.maximum(fid[q], 0)]
        sel = np.flatnonzero(keep)[:k]
        ids[q, :len(sel)] = fid[q, sel]
        sc[q, :len(sel)] = fsc[q, sel]
    return torch.from_numpy(ids), torch.from_numpy(sc)


def masked(ix, Q, k, mask, path, monkeypatch):
    """One masked call under CWQ_MASK_PATH=path; the reported path is the forced one (3 for
    k > 64, which always sorts).  Returns (ids, scores, stats) on the host."""
    monkeypatch.setenv("CWQ_MASK_PATH", str(path))
    ids, sc = ix.score_topk(Q, k, mask=mask)
    st = ix.last_mask_stats()
    if k > 64:
        assert st["path"] == 3, st
    elif path:
        assert st["path"] == path, st
    else:
        assert st["path"] in (1, 2), st
    return ids.cpu(), sc.cpu(), st


def check(ix, Q, k, allowed, full, path, monkeypatch):
    m = ix.sentence_mask(allowed)
    ids, sc, st = masked(ix, Q, k, m, path, monkeypatch)
    m.close()
    flags = np.zeros(ix.n_sent, bool)
    a = np.asarray(allowed.cpu() if torch.is_tensor(allowed) else allowed)
    if a.dtype == np.bool_:
        flags = a
    else:
        flags[a.astype(np.int64)] = True
    eid, esc = expected(full, flags, k)
    assert torch.equal(ids, eid), (path, k, int(flags.sum()))
    assert torch.equal(sc, esc), (path, k, int(flags.sum()))
    return st


# ---------------------------------------------------------------- flat 5000 x 64, 64 queries
@pytest.fixture(scope="module")
def flat5k(gpu):
    X = gpu.synth.synthetic_corpus(5000, 64, seed=101)
    ix = flat_index(gpu, X)
    Q, _ = gpu.synth.synthetic_queries(X, 64, seed=102)
    return ix, Q, full_ranking(ix, Q)


@pytest.mark.parametrize("k", [1, 10, 64, 100])
@pytest.mark.parametrize("path", PATHS)
def test_flat_every_mask(gpu, flat5k, path, k, monkeypatch):
    ix, Q, full = flat5k
    n = ix.n_sent
    rng = np.random.default_rng(1000 + k)
    block = np.zeros(n, bool)
    block[1234:1234 + 900] = True
    masks = {
        "all": np.ones(n, bool),
        "none": np.zeros(n, bool),
        "one": np.arange(n) == 4321,
        "half": rng.random(n) < 0.5,
        "one64th": rng.random(n) < 1.0 / 64,
        "exactly_k": np.isin(np.arange(n), rng.choice(n, k, replace=False)),
        "k_minus_1": np.isin(np.arange(n), rng.choice(n, k - 1, replace=False)),   # pads the tail
        "block": block,
    }
    ix.set_filter(1)   # the over-fetch leg runs the certified filter
    try:
        for name, flags in masks.items():
            st = check(ix, Q, k, flags, full, path, monkeypatch)
            assert st["live_rows"] == int(flags.sum()), name
    finally:
        ix.set_filter(-1)


@pytest.mark.parametrize("path", PATHS)
def test_adversarial_mask_redoes_every_query(gpu, flat5k, path, monkeypatch):
    """Everything in any query's unmasked top-64 is disallowed: the over-fetch finds nothing,
    so every query comes up short and is redone by the gathered scan -- same answers."""
    ix, Q, full = flat5k
    flags = np.ones(ix.n_sent, bool)
    flags[np.unique(full[0][:, :64])] = False
    ix.set_filter(1)
    try:
        st = check(ix, Q, 10, flags, full, path, monkeypatch)
    finally:
        ix.set_filter(-1)
    if path == 1:
        assert st["redone_queries"] == Q.shape[0], st


# ---------------------------------------------------------------- tile edges of the row list
@pytest.fixture(scope="module")
def flat1k(gpu):
    out = {}
    for n in (1000, 1003):   # 1003: the row count is no multiple of 64
        X = gpu.synth.synthetic_corpus(n, 32, seed=200 + n)
        ix = flat_index(gpu, X)
        Q, _ = gpu.synth.synthetic_queries(X, 40, seed=201)
        out[n] = (ix, Q, full_ranking(ix, Q))
    return out


# the gathered scan steps through the row list 128 entries at a time (two rows a lane), 256 in
# its shared-query form for calls of <= 32 queries (64 rows a wave): counts around every edge
@pytest.mark.parametrize("n_live", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
@pytest.mark.parametrize("path", PATHS)
def test_tile_edges(gpu, flat1k, path, n_live, monkeypatch):
    for n in (1000, 1003):
        ix, Q, full = flat1k[n]
        for nq in (20, 40):   # the shared-query form, the query-split form
            fq = (full[0][:nq], full[1][:nq])
            for start in (0, n - n_live, 40, 200):   # the first rows, the last rows, across a 64- / 256-row boundary
                check(ix, Q[:nq], 10, np.arange(start, start + n_live), fq, path, monkeypatch)


@pytest.mark.parametrize("D", [17, 100])
@pytest.mark.parametrize("path", PATHS)
def test_odd_dimensions(gpu, path, D, monkeypatch):
    """A partly filled last 16-wide slice (D = 17, 100: padded to 32, 128)."""
    X = gpu.synth.synthetic_corpus(1000, D, seed=300 + D)
    ix = flat_index(gpu, X)
    Q, _ = gpu.synth.synthetic_queries(X, 33, seed=301)
    full = full_ranking(ix, Q)
    flags = np.random.default_rng(D).random(1000) < 0.25
    for k in (10, 20):
        check(ix, Q, k, flags, full, path, monkeypatch)


# ---------------------------------------------------------------- mixed isotropic / anisotropic rows
@pytest.fixture(scope="module")
def mixed(gpu):
    """The tree of test_gpu_filter.test_mixed_iso_aniso_rows: 6000 x 64 with 700 anisotropic leaves."""
    X = gpu.synth.synthetic_corpus(6000, 64, seed=3)
    fs = gpu.synth.flat_synth(X)
    var = fs["var"].clone()
    g = torch.Generator(device=X.device)
    g.manual_seed(5)
    an = torch.randperm(6000, generator=g, device=X.device)[:700] + 1
    var[an] = var[an] * (0.5 + torch.rand((700, 64), generator=g, device=X.device))
    ix = gpu.index.CobwebIndex(fs["mean"], var, fs["parent"], fs["node_of_sentence"], device="cuda:0")
    assert ix.info["isotropic_rows"] == 5300
    Q, _ = gpu.synth.synthetic_queries(X, 70, seed=9)
    an_sent = np.zeros(6000, bool)
    an_sent[(an - 1).cpu().numpy()] = True   # node i + 1 holds sentence i
    return ix, Q, full_ranking(ix, Q), an_sent


@pytest.mark.parametrize("path", PATHS)
def test_mixed_rows(gpu, mixed, path, monkeypatch):
    ix, Q, full, an_sent = mixed
    ix.set_filter(1)
    try:
        for k in (5, 20):
            st = check(ix, Q, k, an_sent, full, path, monkeypatch)        # only anisotropic rows
            assert st["live_rows"] == 700
            st = check(ix, Q, k, ~an_sent, full, path, monkeypatch)       # only isotropic rows
            assert st["live_rows"] == 5300
            check(ix, Q, k, np.random.default_rng(k).random(6000) < 0.5, full, path, monkeypatch)
            f16 = (full[0][:16], full[1][:16])   # a small call: the shared-query form on both segments
            check(ix, Q[:16], k, an_sent, f16, path, monkeypatch)
            check(ix, Q[:16], k, np.random.default_rng(k + 1).random(6000) < 0.5, f16, path, monkeypatch)
        m = ix.sentence_mask(an_sent)
        assert (m.info["allowed"], m.info["live_iso_rows"], m.info["live_aniso_rows"]) == (700, 0, 700)
        m.close()
    finally:
        ix.set_filter(-1)


# ---------------------------------------------------------------- rows with two sentences, sentences outside the tree
@pytest.mark.parametrize("path", PATHS)
def test_shared_rows_and_sentences_outside_the_tree(gpu, path, monkeypatch):
    N, extra = 1000, 200
    X = gpu.synth.synthetic_corpus(N, 32, seed=400)
    nos = np.concatenate([np.arange(1, N + 1), np.arange(1, extra + 1)]).astype(np.int64)   # sentence N + j shares leaf j
    gone = np.arange(500, 521)
    nos[gone] = -1                                       # sentences 500..520 are in no node
    ix = flat_index(gpu, X, nos)
    Q, _ = gpu.synth.synthetic_queries(X, 40, seed=401)
    full = full_ranking(ix, Q)
    n = N + extra
    # one of a row's two sentences: only that one comes back, with the row's score
    only_second = np.zeros(n, bool)
    only_second[N:] = True
    check(ix, Q, 10, only_second, full, path, monkeypatch)
    m = ix.sentence_mask(only_second)
    ids, sc, _ = masked(ix, Q, 10, m, path, monkeypatch)
    m.close()
    assert bool((ids >= N).all())
    fid, fsc = full
    for q in range(3):
        first = int(ids[q, 0])
        pos = int(np.flatnonzero(fid[q] == first - N)[0])   # the row's other sentence in the full ranking
        assert fsc[q, pos] == float(sc[q, 0])
    # allowed sentences that are in no node never come back; their count is not "allowed in the tree"
    flags = np.random.default_rng(7).random(n) < 0.3
    flags[gone] = True
    for k in (10, 100):
        check(ix, Q, k, flags, full, path, monkeypatch)
    m = ix.sentence_mask(gone)
    assert m.info["allowed"] == 0 and m.info["live_iso_rows"] == 0
    ids, sc, _ = masked(ix, Q, 5, m, path, monkeypatch)
    m.close()
    assert bool((ids == -1).all()) and bool(torch.isinf(sc).all())


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("path", PATHS)
def test_ties_keep_row_then_sentence_order(gpu, path, monkeypatch):
    """200 identical leaves around each query (test_gpu_filter.test_boundary_ties); the mask
    removes the lower-numbered half of them: the tied rows left come in row order."""
    X = gpu.synth.synthetic_corpus(5000, 48, seed=11)
    X[1000:1200] = X[1000]
    ix = flat_index(gpu, X)
    Q = X[1000].repeat(50, 1) + 0.01 * gpu.synth.synthetic_corpus(50, 48, seed=12)
    full = full_ranking(ix, Q)
    flags = np.ones(5000, bool)
    flags[1000:1100] = False
    ix.set_filter(1)
    try:
        for k in (10, 64):
            check(ix, Q, k, flags, full, path, monkeypatch)
        m = ix.sentence_mask(flags)
        ids, sc, _ = masked(ix, Q, 10, m, path, monkeypatch)
        m.close()
    finally:
        ix.set_filter(-1)
    assert torch.equal(ids, torch.arange(1100, 1110).repeat(50, 1))
    assert bool((sc == sc[:, :1]).all())


# ---------------------------------------------------------------- the reference's goldens
@pytest.mark.parametrize("name", HIER)
@pytest.mark.parametrize("path", PATHS)
def test_hierarchical_goldens(gpu, path, name, monkeypatch):
    """Against the fixture's reference-generated rank_scores: the masked top-k is the top-k of
    the reference scores over the allowed sentences, up to swaps the reference itself cannot
    separate (topk_equiv) and RTOL on the scores."""
    g = load_golden(name)
    ix = index_from_golden(gpu, g)
    n = int(g["n_sent"])
    k = int(g["k"])
    rng = np.random.default_rng(len(name))
    three = np.zeros(n, bool)
    three[rng.choice(n, 3, replace=False)] = True
    for flags in (rng.random(n) < 0.5, three):
        m = ix.sentence_mask(flags)
        ids, sc, _ = masked(ix, g["Xq"], k, m, path, monkeypatch)
        m.close()
        ids, sc = ids.numpy(), sc.numpy()
        for qi in range(len(g["Xq"])):
            ref = g["rank_scores"][qi].astype(np.float64)
            ok = flags & np.isfinite(ref)
            cand = np.flatnonzero(ok)
            want = cand[np.argsort(-ref[cand], kind="stable")][:k]
            nv = min(k, len(cand))
            assert np.all(ids[qi, nv:] == -1) and np.all(np.isinf(sc[qi, nv:]))
            got = ids[qi, :nv]
            assert np.all(ok[got]) and len(set(got.tolist())) == nv
            topk_equiv(got, want, ref)
            assert rel_err(sc[qi, :nv], ref[got]) < RTOL


# ---------------------------------------------------------------- the handle's rules
def test_mask_of_another_index_is_an_argument_error(gpu, flat1k):
    ixa, Q, _ = flat1k[1000]
    ixb = flat_index(gpu, gpu.synth.synthetic_corpus(1000, 32, seed=999))   # same shape, another index
    m = ixa.sentence_mask([1, 2, 3])
    with pytest.raises(gpu._lib.CwqError) as e:
        ixb.score_topk(Q, 5, mask=m)
    assert e.value.rc == gpu._lib.CWQ_ERR_ARG and "another index" in str(e.value)
    L = gpu.lib()
    ids = torch.empty((Q.shape[0], 5), dtype=torch.int64, device="cuda:0")
    for k in (0, -1):   # k <= 0 with real handles: CWQ_ERR_ARG, as topk_args
        assert L.cwq_score_topk_masked(ixa._h, m._h, Q.data_ptr(), Q.shape[0], k, ids.data_ptr(), None, None) == \
            gpu._lib.CWQ_ERR_ARG
    assert L.cwq_score_topk_masked(ixa._h, m._h, None, 0, 5, None, None, None) == 0   # nq == 0: a no-op
    with pytest.raises(gpu._lib.CwqError):   # a bitset of another length
        h = ctypes.c_void_p()
        gpu._lib.check(L.cwq_mask_create(ixa._h, Q.data_ptr(), 999, None, ctypes.byref(h)))
    m.close()
    with pytest.raises(ValueError):
        ixa.score_topk(Q, 5, mask=m)   # closed


@pytest.mark.parametrize("path", PATHS)
def test_one_mask_many_calls_two_streams(gpu, flat1k, path, monkeypatch):
    ix, Q, full = flat1k[1000]
    flags = np.random.default_rng(5).random(1000) < 0.2
    eid, esc = expected(full, flags, 10)
    m = ix.sentence_mask(flags)
    for _ in range(3):
        ids, sc, _ = masked(ix, Q, 10, m, path, monkeypatch)
        assert torch.equal(ids, eid) and torch.equal(sc, esc)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(ix.score_topk(Q, 10, mask=m))
    torch.cuda.synchronize()
    for ids, sc in outs:
        assert torch.equal(ids.cpu(), eid) and torch.equal(sc.cpu(), esc)
    m.close()


def test_mask_and_index_destroyed_in_either_order(gpu):
    X = gpu.synth.synthetic_corpus(300, 32, seed=77)
    Q, _ = gpu.synth.synthetic_queries(X, 4, seed=78)
    for index_first in (False, True):
        ix = flat_index(gpu, X)
        m = ix.sentence_mask(np.arange(0, 300, 3))
        ids, _ = ix.score_topk(Q, 5, mask=m)
        assert bool((ids % 3 == 0).all())
        torch.cuda.synchronize()
        if index_first:
            ix._destroy()   # the device index goes first; the mask holds no pointer into it
            m.close()
        else:
            m.close()
            ix.close()
        assert m.closed


# ---------------------------------------------------------------- the drop-in wrapper
def test_wrapper_allowed(gpu, monkeypatch):
    monkeypatch.delenv("CWQ_MASK_PATH", raising=False)
    rng = np.random.default_rng(3)
    n, D, k = 240, 24, 7
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(n)], corpus_embeddings=X)
    Q = torch.from_numpy(X[:12] + 0.05 * rng.standard_normal((12, D)).astype(np.float32)).cuda()
    flags = torch.from_numpy(rng.random(n) < 0.4).cuda()
    w.build_prediction_index()
    m = w.sentence_mask(flags)
    want_ids, want_sc = w._index.score_topk(Q, k, mask=m)
    ids, sc = w.cobweb_predict_batch(Q, k, allowed=flags)                   # a bool tensor
    assert torch.equal(ids, want_ids) and torch.equal(sc, want_sc)
    ids, sc = w.cobweb_predict_batch(Q, k, allowed=m)                       # a reusable mask
    assert torch.equal(ids, want_ids) and torch.equal(sc, want_sc)
    id_list = torch.nonzero(flags).flatten().tolist()
    for qi in range(3):
        got = w.cobweb_predict_fast(Q[qi], k, return_ids=True, is_embedding=True, allowed=id_list)
        assert got == [s for s in want_ids[qi].tolist() if s >= 0]
        got = w.cobweb_predict_indexed(X[qi], k, is_embedding=True, allowed=m)   # a host embedding, sentences out
        assert all(s in w.sentences for s in got) and len(got) == k
    # allowed=None is the plain call
    a_ids, a_sc = w.cobweb_predict_batch(Q, k, allowed=None)
    b_ids, b_sc = w.cobweb_predict_batch(Q, k)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc, b_sc)
    assert w.cobweb_predict_fast(Q[0], k, True, True, allowed=None) == w.cobweb_predict_fast(Q[0], k, True, True)
    # a rebuild makes the mask and a bool tensor of the old length stale; an id list still works
    w.add_sentences([f"t{i}" for i in range(10)], rng.standard_normal((10, D)).astype(np.float32))
    with pytest.raises(ValueError, match="rebuilt"):
        w.cobweb_predict_batch(Q, k, allowed=m)
    with pytest.raises(ValueError, match="one entry per sentence"):
        w.cobweb_predict_batch(Q, k, allowed=flags)
    ids, _ = w.cobweb_predict_batch(Q, k, allowed=id_list)
    assert bool(torch.isin(ids, torch.tensor(id_list, device=ids.device)).all())
    for rebuild in (lambda: w.set_level_weights([1.0, 0.5, 0.25]), w.force_rebuild_index):
        m2 = w.sentence_mask(id_list)
        rebuild()
        with pytest.raises(ValueError, match="rebuilt"):
            w.cobweb_predict_fast(Q[0], k, True, True, allowed=m2)
        m2.close()
    m.close()
