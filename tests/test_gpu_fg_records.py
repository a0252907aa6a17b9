"""Raw filter records (fgemm_kernel<0, true, true> + bucket_raw_kernel, cwq_mfma.hip): on
all-uniform launches the tile epilogue appends {q, row, d, ex} straight from the
accumulators, carries the record list from tile to tile, and the bucket pass evaluates the
bounds.  Every case compares the filter (cwq_set_filter 1) with the exact fp32 scan
(mode 0): ids AND scores bit-identical."""
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
def small_flat(gpu):
    """The two small flat shapes (N, nq not multiples of 256; D not a multiple of 64), built once."""
    out = {}
    for N, D in ((5000, 64), (3000, 200)):
        X = gpu.synth.synthetic_corpus(N, D, seed=N + D)
        out[N, D] = (flat_index(gpu, X), gpu.synth.synthetic_queries(X, 300, seed=N)[0])
    return out


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("N,D", [(5000, 64), (3000, 200)])
def test_small_flat(small_flat, N, D, k):
    ix, Q = small_flat[N, D]
    ids0, s0, ids1, s1, st = both(ix, Q, k)
    assert st["filter_queries"] == 300
    assert torch.equal(ids0, ids1)
    assert torch.equal(s0, s1)


def test_records_carried_over_tiles(gpu):
    """2,048 tiles for 256 workgroups and hundreds of candidates per query: every workgroup
    carries its record list over several tiles and flushes it in mid-launch."""
    X = gpu.synth.synthetic_corpus(262144, 32, seed=31)
    ix = flat_index(gpu, X)
    Q, _ = gpu.synth.synthetic_queries(X, 512, seed=32)
    ids0, s0, ids1, s1, st = both(ix, Q, 64)
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1)
    assert torch.equal(s0, s1)


def test_dense_tiles(gpu):
    """Ten groups of 12 identical rows, 30 queries next to each: the tile of a group gets
    360 records, between half of the record list's capacity and all of it."""
    X = gpu.synth.synthetic_corpus(40000, 64, seed=33)
    for g in range(10):
        X[4000 * g + 100:4000 * g + 112] = X[4000 * g + 100]
    ix = flat_index(gpu, X)
    Q = X[100:40000:4000].repeat(30, 1) + 0.01 * gpu.synth.synthetic_corpus(300, 64, seed=34)
    ids0, s0, ids1, s1, st = both(ix, Q, 10)
    assert st["exact_reranks"] >= 12, st
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1)
    assert torch.equal(s0, s1)


def test_raw_path_equals_in_kernel_path(small_flat, monkeypatch):
    """CWQ_FG_NO_ALLUNI=1 takes the generic instantiation with the in-kernel bounds."""
    ix, Q = small_flat[5000, 64]
    ids0, s0, ids1, s1, st1 = both(ix, Q, 10)
    monkeypatch.setenv("CWQ_FG_NO_ALLUNI", "1")
    _, _, ids2, s2, st2 = both(ix, Q, 10)
    assert torch.equal(ids1, ids2) and torch.equal(s1, s2)
    assert torch.equal(ids0, ids2) and torch.equal(s0, s2)
    assert st1["fallback_queries"] == st2["fallback_queries"], (st1, st2)
