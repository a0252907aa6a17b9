"""Per-query masks (cwq_score_topk_masked_multi): row i of one multi call is the
unmasked full Fast ranking of query i with the sentences its own mask disallows removed, cut to
k -- ids AND scores bit for bit, for any mix of masks.

Reference, helpers and trees are test_gpu_masked_topk's (the exact full ranking filtered in
numpy; the fixtures' reference rank_scores for the hierarchical goldens).  Every case runs under
CWQ_MASK_PATH 1 (over-fetch first), 2 (gathered scan only) and 0 (the rule, per mask)."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_masked_topk import PATHS, expected, flat_index, full_ranking
from test_gpu_parity import HIER, RTOL, index_from_golden, rel_err, topk_equiv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def expected_multi(full, flag_list, moq, k):
    fid, fsc = full
    moq = np.asarray(moq)
    ids = torch.empty((len(moq), k), dtype=torch.int64)
    sc = torch.empty((len(moq), k), dtype=torch.float32)
    for j, flags in enumerate(flag_list):
        sel = np.flatnonzero(moq == j)
        if len(sel):
            e = expected((fid[sel], fsc[sel]), flags, k)
            ids[sel], sc[sel] = e
    return ids, sc


def multi(ix, Q, k, flag_list, moq, path, monkeypatch, full=None):
    """One multi call under CWQ_MASK_PATH=path -> (ids, scores, multi stats); checked against the
    filtered full ranking when `full` is given."""
    monkeypatch.setenv("CWQ_MASK_PATH", str(path))
    masks = [ix.sentence_mask(f) for f in flag_list]
    try:
        ids, sc = ix.score_topk(Q, k, masks=masks, mask_of_query=moq)
        st = ix.last_mask_multi_stats()
        assert ix.last_mask_stats()["path"] == 4
    finally:
        for m in masks:
            m.close()
    ids, sc = ids.cpu(), sc.cpu()
    if full is not None:
        eid, esc = expected_multi(full, flag_list, moq, k)
        bad = torch.nonzero((ids != eid).any(1) | (sc != esc).any(1)).flatten().tolist()
        assert torch.equal(ids, eid) and torch.equal(sc, esc), (path, k, bad[:8], [int(np.asarray(moq)[b]) for b in bad[:8]])
    return ids, sc, st


def eight_masks(n, k, seed):
    rng = np.random.default_rng(seed)
    block = np.zeros(n, bool)
    block[1234:1234 + 900] = True
    return [np.ones(n, bool), np.zeros(n, bool), np.arange(n) == 4321, rng.random(n) < 0.5, rng.random(n) < 1.0 / 64,
            np.isin(np.arange(n), rng.choice(n, k, replace=False)),
            np.isin(np.arange(n), rng.choice(n, k - 1, replace=False)), block]


# ---------------------------------------------------------------- flat 5000 x 64
@pytest.fixture(scope="module")
def flat5k(gpu):
    X = gpu.synth.synthetic_corpus(5000, 64, seed=101)
    ix = flat_index(gpu, X)
    Q, _ = gpu.synth.synthetic_queries(X, 256, seed=102)
    return ix, Q, full_ranking(ix, Q)


@pytest.mark.parametrize("k", [1, 10, 64, 100])
@pytest.mark.parametrize("path", PATHS)
def test_flat_eight_masks_64_queries(gpu, flat5k, path, k, monkeypatch):
    ix, Q, full = flat5k
    nq = 64
    flags = eight_masks(ix.n_sent, k, 1000 + k)
    moq = np.random.default_rng(k).permutation(np.arange(nq) % 8).astype(np.int32)   # round-robin, shuffled
    ix.set_filter(1)   # the over-fetch leg runs the certified filter
    try:
        _, _, st = multi(ix, Q[:nq], k, flags, moq, path, monkeypatch, (full[0][:nq], full[1][:nq]))
    finally:
        ix.set_filter(-1)
    n_none = sum(int((moq == j).sum()) for j, f in enumerate(flags) if not f.any())   # k = 1: "k - 1" is empty too
    assert st["masks_referenced"] == 8
    if k > 64:
        assert st["sort_queries"] == nq - n_none
        return
    assert st["overfetch_queries"] + st["short_queries"] + st["gathered_queries"] == nq - n_none, st
    if path == 0 and k == 10:   # "all" over-fetches at k' = 10, "half" at 40; 1/64 would want 1280
        assert st["overfetch_queries"] > 0 and st["gathered_queries"] > 0, st
    if path == 2:
        assert st["overfetch_queries"] == 0 and st["gathered_queries"] == nq - n_none


@pytest.mark.parametrize("path", PATHS)
def test_flat_eight_masks_200_queries(gpu, flat5k, path, monkeypatch):
    """A batch (the over-fetch cap of 40): "half" still over-fetches at k' = 40, 1/64 is gathered."""
    ix, Q, full = flat5k
    Q, full = Q[:200], (full[0][:200], full[1][:200])
    k = 10
    flags = eight_masks(ix.n_sent, k, 77)
    moq = np.random.default_rng(5).permutation(np.arange(200) % 8).astype(np.int32)
    ix.set_filter(1)
    try:
        _, _, st = multi(ix, Q, k, flags, moq, path, monkeypatch, full)
    finally:
        ix.set_filter(-1)
    assert st["overfetch_queries"] + st["short_queries"] + st["gathered_queries"] == 200 - 25, st
    if path == 0:
        assert st["overfetch_widths"] >= 2, st   # the widths 16 ("all", k' = 10) and 40 ("half")
        assert st["gathered_queries"] >= 25      # 1/64 at least


@pytest.mark.parametrize("path", PATHS)
def test_adversarial_half_is_redone(gpu, flat5k, path, monkeypatch):
    """Everything in any query's unmasked top-64 disallowed for half the queries, "all" for the
    others: path 1 redoes exactly the adversarial half."""
    ix, Q, full = flat5k
    nq = 64
    adv = np.ones(ix.n_sent, bool)
    adv[np.unique(full[0][:nq, :64])] = False
    moq = (np.arange(nq) % 2).astype(np.int32)
    ix.set_filter(1)
    try:
        _, _, st = multi(ix, Q[:nq], 10, [np.ones(ix.n_sent, bool), adv], moq, path, monkeypatch,
                         (full[0][:nq], full[1][:nq]))
    finally:
        ix.set_filter(-1)
    if path == 1:
        assert st["short_queries"] == nq // 2 and st["overfetch_queries"] == nq // 2, st


def test_launch_count_does_not_depend_on_the_mask_count(gpu, flat5k, monkeypatch):
    ix, Q, full = flat5k
    perm = np.random.default_rng(9).permutation(ix.n_sent)

    def run(n_masks):
        flags = []
        for j in range(n_masks):
            f = np.zeros(ix.n_sent, bool)
            f[perm[j::64]] = True   # disjoint, ~78 sentences each
            flags.append(f)
        nq = 4 * n_masks
        moq = np.repeat(np.arange(n_masks), 4).astype(np.int32)
        _, _, st = multi(ix, Q[:nq], 10, flags, moq, 2, monkeypatch, (full[0][:nq], full[1][:nq]))
        return st

    st64, st2 = run(64), run(2)
    assert st64["masks_referenced"] == 64 and st2["masks_referenced"] == 2
    assert 1 <= st64["gathered_launches"] <= 4
    assert st64["gathered_launches"] == st2["gathered_launches"]
    assert st64["gathered_work_items"] >= 64


@pytest.mark.parametrize("path", PATHS)
def test_equivalence_with_the_single_mask_call(gpu, flat5k, path, monkeypatch):
    ix, Q, _ = flat5k
    monkeypatch.setenv("CWQ_MASK_PATH", str(path))
    flags = eight_masks(ix.n_sent, 10, 5)
    moq = np.random.default_rng(6).integers(0, 8, 150).astype(np.int32)
    masks = [ix.sentence_mask(f) for f in flags]
    ids, sc = ix.score_topk(Q[:150], 10, masks=masks, mask_of_query=torch.from_numpy(moq).cuda())   # a device tensor
    for j, m in enumerate(masks):
        sel = torch.from_numpy(np.flatnonzero(moq == j)).cuda()
        one_ids, one_sc = ix.score_topk(Q[:150][sel], 10, mask=m)
        assert torch.equal(ids[sel], one_ids) and torch.equal(sc[sel], one_sc), j
    # every query names the same mask: the single-mask call, its path and its stats
    for j in (3, 4):
        ids, sc = ix.score_topk(Q[:150], 10, masks=masks, mask_of_query=np.full(150, j))
        st = ix.last_mask_stats()
        one_ids, one_sc = ix.score_topk(Q[:150], 10, mask=masks[j])
        assert torch.equal(ids, one_ids) and torch.equal(sc, one_sc)
        assert st == ix.last_mask_stats() and st["path"] in (1, 2)
    for m in masks:
        m.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [10, 100])
def test_loop_form_gives_the_same_rows(gpu, flat5k, path, k, monkeypatch):
    """CWQ_MASK_MULTI_FORM=2: the form the planner takes where the gathered scan's own work
    dwarfs the per-call saving (one single-mask call per mask inside the multi call)."""
    ix, Q, full = flat5k
    nq = 150
    flags = eight_masks(ix.n_sent, k, 31)
    moq = np.random.default_rng(8).integers(0, 8, nq).astype(np.int32)
    monkeypatch.setenv("CWQ_MASK_MULTI_FORM", "2")
    ix.set_filter(1)
    try:
        _, _, st = multi(ix, Q[:nq], k, flags, moq, path, monkeypatch, (full[0][:nq], full[1][:nq]))
    finally:
        ix.set_filter(-1)
    n_none = sum(int((moq == j).sum()) for j, f in enumerate(flags) if not f.any())
    assert st["gathered_launches"] == 0 and st["masks_referenced"] == 8
    if k <= 64:
        assert st["overfetch_queries"] + st["short_queries"] + st["gathered_queries"] == nq - n_none, st


def test_dense_small_group_runs_as_a_call_of_its_own(gpu, flat5k, monkeypatch):
    """200 queries cap the over-fetch at k' = 40; a mask of fraction 0.45 wants k' = 45, which a
    call of its own 20 queries (cap 64) over-fetches: it runs as a single-mask call inside the
    multi call instead of a gathered scan over 45% of the corpus.  Same rows either way."""
    ix, Q, full = flat5k
    Q, full = Q[:200], (full[0][:200], full[1][:200])
    rng = np.random.default_rng(21)
    flags = [np.ones(5000, bool), rng.random(5000) < 0.45, rng.random(5000) < 1.0 / 64]
    moq = np.asarray([0] * 90 + [1] * 20 + [2] * 90, np.int32)[rng.permutation(200)]
    ix.set_filter(1)
    try:
        _, _, st = multi(ix, Q, 10, flags, moq, 0, monkeypatch, full)
        monkeypatch.setenv("CWQ_MASK_MULTI_FORM", "1")   # grouped only
        _, _, st1 = multi(ix, Q, 10, flags, moq, 0, monkeypatch, full)
    finally:
        ix.set_filter(-1)
    assert st["overfetch_queries"] + st["short_queries"] == 110 and st["gathered_queries"] == 90, st
    assert st1["overfetch_queries"] + st1["short_queries"] == 90 and st1["gathered_queries"] == 110, st1
    assert st["gathered_work_items"] < st1["gathered_work_items"]


# ---------------------------------------------------------------- tile and group edges in one call
@pytest.mark.parametrize("path", PATHS)
def test_tile_and_group_edges(gpu, path, monkeypatch):
    n = 1003
    X = gpu.synth.synthetic_corpus(n, 32, seed=200 + n)
    ix = flat_index(gpu, X)
    lives = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    starts = [0, n - 63, 40, 200, 0, n - 128, 40, 200, n - 256, 40]   # first rows, last rows, across 64 / 256
    sizes = [1, 15, 16, 17, 33, 70]
    flags, moq = [], []
    for j, (nl, st0) in enumerate(zip(lives, starts)):
        f = np.zeros(n, bool)
        f[st0:st0 + nl] = True
        assert int(f.sum()) == nl
        flags.append(f)
        moq += [j] * sizes[j % len(sizes)]
    moq = np.random.default_rng(1).permutation(np.asarray(moq, np.int32))
    Q, _ = gpu.synth.synthetic_queries(X, len(moq), seed=201)
    full = full_ranking(ix, Q)
    _, _, st = multi(ix, Q, 10, flags, moq, path, monkeypatch, full)
    if path == 2:
        assert st["gathered_launches"] <= 4 and st["gathered_launches"] == 2, st   # one segment, both forms
        assert st["gathered_work_items"] >= 10
        assert st["gathered_queries"] == len(moq)


# ---------------------------------------------------------------- mixed isotropic / anisotropic rows
@pytest.fixture(scope="module")
def mixed(gpu):
    """test_gpu_masked_topk.mixed: 6000 x 64 with 700 anisotropic leaves."""
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
    an_sent[(an - 1).cpu().numpy()] = True
    return ix, Q, full_ranking(ix, Q), an_sent


@pytest.mark.parametrize("path", PATHS)
def test_mixed_rows(gpu, mixed, path, monkeypatch):
    ix, Q, full, an_sent = mixed
    rng = np.random.default_rng(4)
    flags = [an_sent, ~an_sent, rng.random(6000) < 0.5, rng.random(6000) < 0.05]
    assert (flags[3] & an_sent).any() and (flags[3] & ~an_sent).any()
    moq = rng.integers(0, 4, 70).astype(np.int32)
    ix.set_filter(1)
    try:
        for k in (5, 20):
            multi(ix, Q, k, flags, moq, path, monkeypatch, full)
    finally:
        ix.set_filter(-1)


# ---------------------------------------------------------------- shared rows, sentences in no node
@pytest.mark.parametrize("path", PATHS)
def test_shared_rows_and_sentences_outside_the_tree(gpu, path, monkeypatch):
    N, extra = 1000, 200
    X = gpu.synth.synthetic_corpus(N, 32, seed=400)
    nos = np.concatenate([np.arange(1, N + 1), np.arange(1, extra + 1)]).astype(np.int64)
    gone = np.arange(500, 521)
    nos[gone] = -1
    ix = flat_index(gpu, X, nos)
    Q, _ = gpu.synth.synthetic_queries(X, 40, seed=401)
    full = full_ranking(ix, Q)
    n = N + extra
    only_second = np.zeros(n, bool)
    only_second[N:] = True
    outside = np.zeros(n, bool)
    outside[gone] = True
    normal = np.random.default_rng(7).random(n) < 0.3
    moq = (np.arange(40) % 3).astype(np.int32)
    for k in (10, 100):
        ids, sc, _ = multi(ix, Q, k, [only_second, outside, normal], moq, path, monkeypatch, full)
        assert bool((ids[moq == 1] == -1).all()) and bool(torch.isinf(sc[moq == 1]).all())
        got = ids[moq == 0]
        assert bool(((got >= N) | (got == -1)).all()) and bool((got[:, 0] >= N).all())


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("path", PATHS)
def test_ties_keep_row_order_per_mask(gpu, path, monkeypatch):
    X = gpu.synth.synthetic_corpus(5000, 48, seed=11)
    X[1000:1200] = X[1000]
    ix = flat_index(gpu, X)
    Q = X[1000].repeat(50, 1) + 0.01 * gpu.synth.synthetic_corpus(50, 48, seed=12)
    full = full_ranking(ix, Q)
    lower, upper = np.ones(5000, bool), np.ones(5000, bool)
    lower[1000:1100] = False   # removes the lower-numbered half of the tied rows
    upper[1100:1200] = False
    moq = (np.arange(50) % 2).astype(np.int32)
    ix.set_filter(1)
    try:
        for k in (10, 64):
            ids, sc, _ = multi(ix, Q, k, [lower, upper], moq, path, monkeypatch, full)
    finally:
        ix.set_filter(-1)
    assert torch.equal(ids[moq == 0], torch.arange(1100, 1164).repeat(25, 1))
    assert torch.equal(ids[moq == 1], torch.arange(1000, 1064).repeat(25, 1))
    assert bool((sc == sc[:, :1]).all())


@pytest.mark.parametrize("D", [17, 100])
@pytest.mark.parametrize("path", PATHS)
def test_odd_dimensions(gpu, path, D, monkeypatch):
    X = gpu.synth.synthetic_corpus(1000, D, seed=300 + D)
    ix = flat_index(gpu, X)
    Q, _ = gpu.synth.synthetic_queries(X, 33, seed=301)
    full = full_ranking(ix, Q)
    rng = np.random.default_rng(D)
    flags = [rng.random(1000) < 0.25, rng.random(1000) < 0.6, rng.random(1000) < 0.02]
    multi(ix, Q, 10, flags, (np.arange(33) % 3).astype(np.int32), path, monkeypatch, full)


# ---------------------------------------------------------------- the reference's goldens
@pytest.mark.parametrize("name", HIER)
@pytest.mark.parametrize("path", PATHS)
def test_hierarchical_goldens(gpu, path, name, monkeypatch):
    g = load_golden(name)
    ix = index_from_golden(gpu, g)
    n, k = int(g["n_sent"]), int(g["k"])
    rng = np.random.default_rng(len(name))
    three = np.zeros(n, bool)
    three[rng.choice(n, 3, replace=False)] = True
    flag_list = [rng.random(n) < 0.5, three]
    nq = len(g["Xq"])
    moq = (np.arange(nq) % 2).astype(np.int32)
    ids, sc, _ = multi(ix, g["Xq"], k, flag_list, moq, path, monkeypatch)
    ids, sc = ids.numpy(), sc.numpy()
    for qi in range(nq):
        flags = flag_list[moq[qi]]
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
def test_handle_rules(gpu, flat5k, monkeypatch):
    monkeypatch.delenv("CWQ_MASK_PATH", raising=False)
    ixa, Q, full = flat5k
    Q, full = Q[:40], (full[0][:40], full[1][:40])
    ixb = flat_index(gpu, gpu.synth.synthetic_corpus(5000, 64, seed=999))   # same shape, another index
    fa = np.random.default_rng(1).random(5000) < 0.2
    fb = np.random.default_rng(2).random(5000) < 0.7
    ma, mb, other = ixa.sentence_mask(fa), ixa.sentence_mask(fb), ixb.sentence_mask([1, 2, 3])
    moq = (np.arange(40) % 2).astype(np.int32)
    with pytest.raises(gpu._lib.CwqError) as e:   # a mask of another index at slot 3
        ixa.score_topk(Q, 5, masks=[ma, mb, ma, other], mask_of_query=moq)
    assert e.value.rc == gpu._lib.CWQ_ERR_ARG and "another index" in str(e.value)
    for bad in (2, -1):
        with pytest.raises(gpu._lib.CwqError) as e:
            ixa.score_topk(Q, 5, masks=[ma, mb], mask_of_query=np.where(np.arange(40) == 7, bad, moq))
        assert e.value.rc == gpu._lib.CWQ_ERR_ARG and "mask_of_query[7]" in str(e.value)
    with pytest.raises(ValueError):
        ixa.score_topk(Q, 5, masks=[ma, mb], mask_of_query=moq[:39])   # wrong length
    with pytest.raises(ValueError):
        ixa.score_topk(Q, 5, masks=[ma, fb], mask_of_query=moq)        # not a SentenceMask
    # the same mask in two slots, and an unused slot
    eid, esc = expected_multi(full, [fa, fb], moq, 10)
    ids, sc = ixa.score_topk(Q, 10, masks=[ma, mb, ma, mb], mask_of_query=moq + 2 * (np.arange(40) % 4 >= 2))
    assert torch.equal(ids.cpu(), eid) and torch.equal(sc.cpu(), esc)
    assert ixa.last_mask_multi_stats()["masks_referenced"] == 2
    ids, sc = ixa.score_topk(Q, 10, masks=[mb, ma, mb], mask_of_query=(1 + moq).tolist())   # slot 0 unused; a list
    assert torch.equal(ids.cpu(), eid) and torch.equal(sc.cpu(), esc)
    # two streams, the same masks
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(ixa.score_topk(Q, 10, masks=[ma, mb], mask_of_query=moq))
    torch.cuda.synchronize()
    for ids, sc in outs:
        assert torch.equal(ids.cpu(), eid) and torch.equal(sc.cpu(), esc)
    other.close()
    mb.close()
    with pytest.raises(ValueError):
        ixa.score_topk(Q, 5, masks=[ma, mb], mask_of_query=moq)   # closed
    ma.close()


# ---------------------------------------------------------------- the drop-in wrapper
def test_wrapper_allowed_sets_on_g4(gpu, monkeypatch):
    """cobweb_predict_batch(allowed_sets=, set_of_query=) on the G4 corpus and queries, the tree
    fitted here: every query's row is the index's exact full ranking over its own set."""
    monkeypatch.delenv("CWQ_MASK_PATH", raising=False)
    g = load_golden("g4_twolevel_d48")
    n, k = len(g["X"]), int(g["k"])
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(n)], corpus_embeddings=g["X"])
    rng = np.random.default_rng(3)
    sets = [rng.random(n) < 0.5, np.sort(rng.choice(n, 40, replace=False)).tolist(), torch.from_numpy(rng.random(n) < 0.1)]
    flags = []
    for a in sets:
        f = np.zeros(n, bool)
        a = np.asarray(a)
        f[a if a.dtype != np.bool_ else np.flatnonzero(a)] = True
        flags.append(f)
    nq = len(g["Xq"])
    soq = torch.arange(nq) % 3
    Q = torch.from_numpy(g["Xq"]).cuda()
    w.build_prediction_index()
    full = full_ranking(w._index, Q)
    ids, sc = w.cobweb_predict_batch(Q, k, allowed_sets=sets, set_of_query=soq)
    eid, esc = expected_multi(full, flags, soq.numpy(), k)
    assert torch.equal(ids.cpu(), eid) and torch.equal(sc.cpu(), esc)
    assert bool((ids >= 0).all())
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    # a reusable mask among sets made for the call: it stays open, the others are closed here
    m = w.sentence_mask(sets[0])
    ids2, sc2 = w.cobweb_predict_batch(Q, k, allowed_sets=[m, sets[1], sets[2]], set_of_query=soq.tolist())
    assert np.array_equal(ids2.cpu().numpy(), ids) and np.array_equal(sc2.cpu().numpy(), sc)
    assert not m.closed
    with pytest.raises(ValueError, match="not both"):
        w.cobweb_predict_batch(Q, k, allowed=m, allowed_sets=[m], set_of_query=[0] * nq)
    m.close()


def test_sentence_masks_by_label(gpu, monkeypatch):
    monkeypatch.delenv("CWQ_MASK_PATH", raising=False)
    rng = np.random.default_rng(3)
    n, D, k = 240, 24, 7
    X = rng.standard_normal((n, D)).astype(np.float32)
    w = gpu.CobwebWrapper(corpus=[f"s{i}" for i in range(n)], corpus_embeddings=X)
    Q = torch.from_numpy(X[:12] + 0.05 * rng.standard_normal((12, D)).astype(np.float32)).cuda()
    lab = np.asarray([3, 4, 900, 901])[rng.integers(0, 4, n)]   # an unused value range between 4 and 900
    masks, values = w.sentence_masks_by_label(lab)
    assert values.tolist() == [3, 4, 900, 901] and len(masks) == 4
    for j, m in enumerate(masks):
        assert m.info["allowed"] == int((lab == values[j].item()).sum())
    qlab = torch.as_tensor([3, 901, 900, 4] * 3)
    soq = torch.searchsorted(values, qlab)   # the docstring's recipe
    ids, sc = w.cobweb_predict_batch(Q, k, allowed_sets=masks, set_of_query=soq)
    for qi in range(12):
        one_ids, one_sc = w.cobweb_predict_batch(Q[qi:qi + 1], k, allowed=masks[int(soq[qi])])
        assert torch.equal(ids[qi:qi + 1], one_ids) and torch.equal(sc[qi:qi + 1], one_sc)
        assert all(lab[s] == int(qlab[qi]) for s in ids[qi].tolist() if s >= 0)
    with pytest.raises(ValueError):
        w.sentence_masks_by_label(lab[:-1])
    for m in masks:
        m.close()
