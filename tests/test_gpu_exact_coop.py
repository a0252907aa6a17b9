"""The wave-cooperative exact keys of the batch rerank (cwq_mfma.hip exact_iso_acc_coop in
sample_threshold_kernel<true> and final_kernel<true>): the lanes of a wave take (row, 16-dim
slice) items, the partials go through LDS, and lane r adds row r's partials in slice order, so
the keys are the per-lane form's (exact_iso_key) bit for bit.  Every case runs the filtered
call in both forms (CWQ_EXACT_COOP unset / 0, read per call) and the exact fp32 scan
(cwq_set_filter 0): ids AND scores bit-identical, and the candidates, exact reranks and
re-run queries of the two forms equal.  CWQ_FG_I8_EARLY=2 gives the small indices here the
direct schedule, whose thresholds come from sample_threshold_kernel.

Seen to fail on a wrong order: with the ordered sum of exact_iso_acc_coop walking a chunk's
partials from the last slice to the first, every test here fails but the two-level one (which
keeps the per-lane chain form, as it checks)."""
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DIRECT = {"CWQ_FG_I8_EARLY": "2"}
PERLANE = {"CWQ_FG_I8_EARLY": "2", "CWQ_EXACT_COOP": "0"}
KNOBS = ("CWQ_FG_I8", "CWQ_FG_I8_EARLY", "CWQ_FG_CUTS", "CWQ_FG_PHASES", "CWQ_EXACT_COOP")


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def flat_index(pkg, X, n_first_sentence=0):
    """Flat index over X; the leaves before n_first_sentence hold no sentence (unusable rows)."""
    fs = pkg.synth.flat_synth(X)
    old = os.environ.pop("CWQ_FG_HUB_DIV", None)
    try:
        return pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"][n_first_sentence:],
                                     device="cuda:0")
    finally:
        if old is not None:
            os.environ["CWQ_FG_HUB_DIV"] = old


def filt(ix, Q, k, mp, knobs, path="fgemm"):
    """One filtered call under the given per-call knobs (a fresh guard record) -> ids, scores, stats, filter_info."""
    for name in KNOBS:
        mp.delenv(name, raising=False)
    for name, v in knobs.items():
        mp.setenv(name, v)
    ix.set_filter(1)
    try:
        ids, s = ix.score_topk(Q, k)
        st, fi = ix.last_stats(), ix.filter_info()
    finally:
        ix.set_filter(-1)
        for name in knobs:
            mp.delenv(name)
    print(knobs, st, fi)
    assert st["filter_used"] and st["path"] == path, st
    return ids.cpu(), s.cpu(), st, fi


def exact(ix, Q, k):
    ix.set_filter(0)
    ids, s = ix.score_topk(Q, k)
    assert not ix.last_stats()["filter_used"]
    ix.set_filter(-1)
    return ids.cpu(), s.cpu()


def check_forms(ix, Q, k, mp, fallbacks=0, direct=True, knobs=None):
    """Both forms of the exact keys against the exact scan and against each other -> the coop stats."""
    ids0, s0 = exact(ix, Q, k)
    ids1, s1, st1, fi1 = filt(ix, Q, k, mp, dict(DIRECT, **(knobs or {})))
    ids2, s2, st2, fi2 = filt(ix, Q, k, mp, dict(PERLANE, **(knobs or {})))
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1), "coop against the exact scan"
    assert torch.equal(ids0, ids2) and torch.equal(s0, s2), "per-lane against the exact scan"
    for name in ("candidates", "exact_reranks", "fallback_queries"):
        assert st1[name] == st2[name], (name, st1, st2)
    assert fi1["direct_last_call"] == fi2["direct_last_call"]
    if direct is not None:
        assert fi1["direct_last_call"] == direct, fi1
    if fallbacks is not None:
        assert st1["fallback_queries"] == fallbacks, st1
    return st1


# 48 slices (three chunks of 16); 4 slices (a partial chunk); 65 slices (more than a wave's lanes,
# a last chunk of one slice)
SHAPES = [(20000, 768), (65536, 64), (8192, 1040)]


@pytest.fixture(scope="module")
def gaussian(gpu):
    out = {}
    for N, D in SHAPES:
        X = gpu.synth.synthetic_corpus(N, D, seed=N + D + 1)
        Q, _ = gpu.synth.synthetic_queries(X, 300, seed=N + 1)
        out[N, D] = (flat_index(gpu, X), Q)
    return out


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("N,D", SHAPES)
def test_gaussian_flat_index(gaussian, N, D, k, monkeypatch):
    ix, Q = gaussian[N, D]
    # k = 64 at 20,000 x 768 may flood the record buffers (the guard's case): whatever the filter
    # leaves to the exact re-run, the two forms leave the same
    check_forms(ix, Q, k, monkeypatch, fallbacks=None if k == 64 else 0, direct=None if k == 64 else True)


N_EDGE, D_EDGE = 33000, 64   # 129 row tiles, the last one partial


def test_more_than_64_survivors(gpu, monkeypatch):
    """20 centres, 200 rows within 1e-3 of each, the queries half a standard deviation a dimension
    from a centre: the bounds cannot tell a centre's rows apart, so pass 2 scores more than 64 rows
    of one query (several rounds, the pending list carried from one to the next).  (Queries much
    nearer would not do: a raw sum far below logdet leaves the key no trace of its rounding.)"""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=211)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(212)
    C = X[:20].clone()
    X[:4000] = C.repeat_interleave(200, 0) + 1e-3 * torch.randn((4000, D_EDGE), generator=g, device="cuda:0")
    Q = (C.repeat(15, 1) + 0.5 * torch.randn((300, D_EDGE), generator=g, device="cuda:0")).contiguous()
    ix = flat_index(gpu, X.contiguous())
    for k in (10, 64):
        st = check_forms(ix, Q, k, monkeypatch, direct=None)
        assert st["exact_reranks"] > 64 + k, st


def test_tied_keys_across_the_k_boundary(gpu, monkeypatch):
    """Every row twice: the k-th and (k+1)-th keys tie exactly for odd k."""
    X = gpu.synth.synthetic_corpus(N_EDGE // 2, D_EDGE, seed=231)
    X = torch.cat([X, X]).contiguous()
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=232)
    ix = flat_index(gpu, X)
    for k in (1, 9):
        check_forms(ix, Q, k, monkeypatch)


def test_query_equal_to_a_hub_row(gpu, monkeypatch):
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=241)
    hubs = (X - X.mean(0)[None, :]).norm(dim=1).argsort()[:150]   # the lowest-norm rows: hub rows among them
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=242)
    Q[:150] = X[hubs]
    ix = flat_index(gpu, X)
    for k in (1, 10):
        check_forms(ix, Q.contiguous(), k, monkeypatch)


def test_fewer_than_k_and_exactly_k_candidates(gpu, monkeypatch):
    """Only the last leaves hold a sentence.  3,000 of them: 48 usable sample groups, fewer than
    K = 64 (T = -inf, every query re-run exactly) and more than K = 10.  64 of them: K = 64 rows
    can be candidates at all."""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=251)
    Q, _ = gpu.synth.synthetic_queries(X[30000:].contiguous(), 300, seed=252)
    ix = flat_index(gpu, X, n_first_sentence=30000)
    check_forms(ix, Q, 64, monkeypatch, fallbacks=300)
    check_forms(ix, Q, 10, monkeypatch)
    ix = flat_index(gpu, X, n_first_sentence=N_EDGE - 64)
    check_forms(ix, Q, 64, monkeypatch, fallbacks=None, direct=None)
    check_forms(ix, Q, 10, monkeypatch, fallbacks=None, direct=None)


@pytest.mark.parametrize("nq", [300, 257])
def test_partial_tiles(gpu, nq, monkeypatch):
    """A partial last row tile (33,000 rows) and a padded last query tile (a wave of the last
    workgroup without a query at 257)."""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=261)
    Q, _ = gpu.synth.synthetic_queries(X, nq, seed=262)
    ix = flat_index(gpu, X)
    check_forms(ix, Q, 10, monkeypatch)


def test_categorize_caller(gpu, monkeypatch):
    """Basic over a flat index, 300 queries a call (more than the workgroup-per-query form takes):
    the isotropic list's rerank is final_kernel with the key min(BF[parent], lp).  40 rows differ
    from one row by 1e-5 in one dimension each and 20 queries lie one standard deviation a dimension
    from it, so those rows' keys are a few ulp apart and the pop order follows their rounding.
    Both forms against the exact heap replay: pop order, n_found and call counts."""
    X = gpu.synth.synthetic_corpus(20000, 64, seed=271)
    X[3000:3040] = X[3000]
    X[3000:3040] += 1e-5 * torch.eye(64, device="cuda:0")[:40]
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=272)
    Q[:20] = X[3000][None, :] + gpu.synth.synthetic_corpus(20, 64, seed=273)
    ix = flat_index(gpu, X.contiguous())
    out = []
    for coop in (None, "0"):
        if coop is not None:
            monkeypatch.setenv("CWQ_EXACT_COOP", coop)
        ix.set_filter(1)
        try:
            out.append([t.cpu() for t in ix.categorize(Q.contiguous(), 10, 100000)])
        finally:
            ix.set_filter(-1)
        monkeypatch.delenv("CWQ_EXACT_COOP", raising=False)
    ix.set_filter(0)
    monkeypatch.setenv("CWQ_CAT_COUNT", "0")
    try:
        ref = [t.cpu() for t in ix.categorize(Q.contiguous(), 10, 100000)]
    finally:
        ix.set_filter(-1)
    for name, r, a, b in zip(("nodes", "n_found", "n_calls"), ref, *out):
        assert torch.equal(r, a), ("coop against the exact replay", name)
        assert torch.equal(r, b), ("per-lane against the exact replay", name)


def test_two_level_tree_keeps_the_chain_form(gpu, monkeypatch):
    """Root -> 150 clusters -> leaves: the parents' prefixes come from the exact chain, and the
    per-lane keys stay (CWQ_EXACT_COOP changes nothing)."""
    X = gpu.synth.synthetic_corpus(20000, 96, seed=281)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(282)
    t = gpu.synth.two_level_synth(X, torch.randint(0, 150, (X.shape[0],), generator=g, device="cuda:0"))
    ix = gpu.index.CobwebIndex(t["mean"], t["var"], t["parent"], t["node_of_sentence"], device="cuda:0")
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=283)
    check_forms(ix, Q, 10, monkeypatch, fallbacks=None, direct=None)
