"""The exact-seeded rerank of final_kernel (cwq_mfma.hip): the K candidates with the largest
lower bounds are scored exactly first, the K-th largest of those keys raises the rerank
threshold T2, and only then the remaining candidates with an upper bound >= T2 are scored.
Keys, tie rule and outputs are the exact scan's.  Batches of 300 queries: final_kernel (a
wave per query) serves chunks of more than 256 queries."""
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def flat_index(pkg, X):
    fs = pkg.synth.flat_synth(X)
    return pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"], device="cuda:0")


def both(ix, Q, k):
    ix.set_filter(0)
    ids0, s0 = ix.score_topk(Q, k)
    assert not ix.last_stats()["filter_used"]
    ix.set_filter(1)
    ids1, s1 = ix.score_topk(Q, k)
    st = ix.last_stats()
    ix.set_filter(-1)
    print(st)
    assert st["filter_used"] and st["path"] == "fgemm", st
    return ids0.cpu(), s0.cpu(), ids1.cpu(), s1.cpu(), st


@pytest.fixture(scope="module")
def tied(gpu):
    X = gpu.synth.synthetic_corpus(20000, 64, seed=61)
    X[7000:7012] = X[7000]
    Q = X[7000][None, :].repeat(300, 1) + 0.01 * gpu.synth.synthetic_corpus(300, 64, seed=62)
    return flat_index(gpu, X), Q.contiguous()


@pytest.mark.parametrize("k", [10, 12])
def test_ties_across_the_k_boundary(tied, k):
    """12 identical rows next to every query: with k = 10 the K-th best key is shared by rows
    inside and outside the seed round, and all 12 must be scored (ties go by row index)."""
    ix, Q = tied
    ids0, s0, ids1, s1, st = both(ix, Q, k)
    assert st["exact_reranks"] >= 12 and st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    assert sorted(ids1[0].tolist()) == list(range(7000, 7000 + k))


def test_fewer_candidates_than_k(gpu):
    """40 rows, k = 64: no query has K candidates, every one goes to the exact scan."""
    X = gpu.synth.synthetic_corpus(40, 64, seed=63)
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=64)
    ids0, s0, ids1, s1, st = both(flat_index(gpu, X), Q, 64)
    assert st["fallback_queries"] == 300, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


def test_exactly_k_candidates(gpu):
    """64 rows, k = 64: every row is a candidate and the seed round scores them all."""
    X = gpu.synth.synthetic_corpus(64, 64, seed=65)
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=66)
    ids0, s0, ids1, s1, st = both(flat_index(gpu, X), Q, 64)
    assert st["fallback_queries"] == 0 and st["candidates"] == 64 and st["exact_reranks"] == 64, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


def test_categorize_caller(gpu):
    """cwq_categorize's isotropic list comes from the same kernel with the key
    min(BF[parent], lp): pop order, n_found and call counts of the exact heap replay."""
    X = gpu.synth.synthetic_corpus(20000, 64, seed=67)
    X[3000:3012] = X[3000]
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=68)
    Q[:20] = X[3000][None, :] + 0.01 * gpu.synth.synthetic_corpus(20, 64, seed=69)
    ix = flat_index(gpu, X)
    ix.set_filter(1)
    got = ix.categorize(Q, 10, 100000)
    ix.set_filter(0)
    os.environ["CWQ_CAT_COUNT"] = "0"
    try:
        ref = ix.categorize(Q, 10, 100000)
    finally:
        del os.environ["CWQ_CAT_COUNT"]
        ix.set_filter(-1)
    for name, a, b in zip(("nodes", "n_found", "n_calls"), ref, got):
        assert torch.equal(a, b), name


# exact_reranks per query on the inputs of test_reranks_do_not_grow, measured on an MI355X:
# the parent library (strided sample, rerank threshold from lower bounds alone) 18 of 125
# candidates; this one (hub rows in the sample, seeded rerank) 13 of 59
# (profiles/hub_reranks_20kx768.log).  The parent is the reference.
PARENT_RERANKS = 18


def test_reranks_do_not_grow(gpu):
    """C3's distribution at 20,000 x 768, k = 10, default policy."""
    X = gpu.synth.synthetic_corpus(20000, 768, seed=41)
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=42)
    ids0, s0, ids1, s1, st = both(flat_index(gpu, X), Q, 10)
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    print("exact_reranks", st["exact_reranks"], "parent", PARENT_RERANKS)
    assert st["exact_reranks"] <= PARENT_RERANKS, st
