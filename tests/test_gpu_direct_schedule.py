"""The batch filter's direct schedule (cwq_filter.hip fg_i8_from / run_iso_filter, cwq_mfma.hip
fgemm_kernel<1, true, false, true> and sample_threshold_kernel): the sample pass ranks the
sample rows on the int8 operands, T[q] is the K-th largest EXACT key of the K rows it picks,
and no bf16 query panel is prepared.  CWQ_FG_I8_EARLY=2 (read per call) gives the small
indices here that schedule; by default it runs where the early schedule ran by the size rule.
It keeps the five launches of the phase cuts (one launch over every row tile measured slower
at C3, DESIGN Appendix C.1); every case also runs it with one launch (CWQ_FG_PHASES=0).
Every case compares with the exact fp32 scan (cwq_set_filter 0): ids AND scores
bit-identical."""
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DIRECT = {"CWQ_FG_I8_EARLY": "2"}
DIRECT1 = {"CWQ_FG_I8_EARLY": "2", "CWQ_FG_PHASES": "0"}   # one launch over every row tile
KNOBS = ("CWQ_FG_I8", "CWQ_FG_I8_EARLY", "CWQ_FG_CUTS", "CWQ_FG_PHASES")


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


def call(ix, Q, k, mp, knobs):
    """One filtered call under the given per-call knobs -> ids, scores, stats, filter_info."""
    for name in KNOBS:
        mp.delenv(name, raising=False)
    for name, v in knobs.items():
        mp.setenv(name, v)
    ids, s = ix.score_topk(Q, k)
    st, fi = ix.last_stats(), ix.filter_info()
    for name in knobs:
        mp.delenv(name)
    print(knobs, st, fi)
    assert st["filter_used"] and st["path"] == "fgemm", st
    return ids.cpu(), s.cpu(), st, fi


def filt(ix, Q, k, mp, knobs):
    ix.set_filter(1)   # (a fresh guard record, too)
    try:
        return call(ix, Q, k, mp, knobs)
    finally:
        ix.set_filter(-1)


def exact(ix, Q, k):
    ix.set_filter(0)
    ids, s = ix.score_topk(Q, k)
    assert not ix.last_stats()["filter_used"]
    ix.set_filter(-1)
    return ids.cpu(), s.cpu()


def check_direct(ix, Q, k, mp, fallbacks=0):
    """The direct schedule with the phase cuts (five launches at every size here) and with one
    launch: both exact, both with the expected re-runs.  -> the stats of the first."""
    ids0, s0 = exact(ix, Q, k)
    out = None
    for knobs, launches in ((DIRECT, 5), (DIRECT1, 1)):
        ids1, s1, st, fi = filt(ix, Q, k, mp, knobs)
        assert fi["direct_last_call"] and st["fg_i8_launches"] == launches, (knobs, st, fi)
        assert st["fallback_queries"] == fallbacks, (knobs, st)
        assert torch.equal(ids0, ids1) and torch.equal(s0, s1), knobs
        out = out or st
    return out


SHAPES = [(20000, 768), (65536, 64)]


@pytest.fixture(scope="module")
def gaussian(gpu):
    out = {}
    for N, D in SHAPES:
        X = gpu.synth.synthetic_corpus(N, D, seed=N + D)
        Q, _ = gpu.synth.synthetic_queries(X, 300, seed=N)
        out[N, D] = (flat_index(gpu, X), Q)
    return out


@pytest.mark.parametrize("N,D,k", [(20000, 768, 1), (20000, 768, 10), (65536, 64, 10)])
def test_gaussian_flat_index(gaussian, N, D, k, monkeypatch):
    ix, Q = gaussian[N, D]
    S = max(256, N // 128 // 256 * 256)
    st = check_direct(ix, Q, k, monkeypatch)
    assert st["sample_rows"] == S + S // 2, st
    if (N, D, k) == (20000, 768, 10):
        # exact-key thresholds against bound thresholds on the same index and cuts (the CPU model at
        # this size, scripts/i8_batch_survival.py --direct: 169 against 181 candidates per query);
        # at 65,536 x 64 one launch passes more (model: 174 against 81), the documented limit
        _, _, st1, fi1 = filt(ix, Q, k, monkeypatch, {"CWQ_FG_I8_EARLY": "1"})
        assert st1["fg_i8_launches"] == 5 and not fi1["direct_last_call"], (st1, fi1)
        print(f"candidates per query: direct {st['candidates']}, early {st1['candidates']}")
        assert st["candidates"] <= st1["candidates"], (st, st1)


N_EDGE, D_EDGE = 33000, 64   # 129 row tiles, the last one partial; S = 256, H = 128


def test_tied_keys_at_the_threshold(gpu, monkeypatch):
    """Every row twice: the k-th and (k+1)-th keys tie exactly for odd k, so T may equal the
    K-th best key and the filter's >= has to hold throughout."""
    X = gpu.synth.synthetic_corpus(N_EDGE // 2, D_EDGE, seed=131)
    X = torch.cat([X, X]).contiguous()
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=132)
    ix = flat_index(gpu, X)
    for k in (1, 9):
        check_direct(ix, Q, k, monkeypatch)


def test_query_equal_to_a_hub_row(gpu, monkeypatch):
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=141)
    hubs = (X - X.mean(0)[None, :]).norm(dim=1).argsort()[:150]   # the lowest-norm rows: hub rows among them
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=142)
    Q[:150] = X[hubs]
    ix = flat_index(gpu, X)
    assert ix.filter_info()["sample_hub_rows"] == 128
    for k in (1, 10):
        check_direct(ix, Q.contiguous(), k, monkeypatch)


def test_top64_inside_the_sample(gpu, monkeypatch):
    """The construction of test_hub_rows_are_distinct_from_the_strided_rows: the strided rows
    are the lowest-norm rows and the queries sit next to the root mean, so the whole top-64 is
    in the sample and T is the 64th best key itself."""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=71)
    X[0:256 * 128:128] *= 0.01
    g = torch.Generator(device="cuda:0")
    g.manual_seed(72)
    Q = (X.mean(0)[None, :] + 0.05 * torch.randn((300, D_EDGE), generator=g, device="cuda:0")).contiguous()
    ix = flat_index(gpu, X)
    check_direct(ix, Q, 64, monkeypatch)


def test_fewer_usable_groups_than_k(gpu, monkeypatch):
    """Only the last 3,000 leaves hold a sentence: 21 strided sample rows in 16 groups and 128
    hub rows in 32 groups are usable, 48 groups for K = 64.  T = -inf: every query is re-run
    exactly, the results are the exact scan's."""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=151)
    Q, _ = gpu.synth.synthetic_queries(X[30000:].contiguous(), 300, seed=152)
    ix = flat_index(gpu, X, n_first_sentence=30000)
    assert ix.filter_info()["sample_hub_rows"] == 128
    check_direct(ix, Q, 64, monkeypatch, fallbacks=300)
    check_direct(ix, Q, 10, monkeypatch)   # 48 groups >= 10: thresholds again


@pytest.mark.parametrize("nq", [300, 257])
def test_partial_tiles(gpu, nq, monkeypatch):
    """A partial last row tile (33,000 rows) and a padded last query tile."""
    X = gpu.synth.synthetic_corpus(N_EDGE, D_EDGE, seed=161)
    Q, _ = gpu.synth.synthetic_queries(X, nq, seed=162)
    ix = flat_index(gpu, X)
    check_direct(ix, Q, 10, monkeypatch)


def test_guard_trips_on_a_flood_of_candidates(gpu, monkeypatch):
    """k = 64 on 20,000 x 768 with one launch passes more than 1,024 candidates per query or
    overflows the record buffers: the call is exact, and the next one is back on the quarter
    rule (bf16 sample pass, five launches, two of them on the int8 operands), as under
    CWQ_FG_I8_EARLY=1."""
    X = gpu.synth.synthetic_corpus(20000, 768, seed=91)
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=92)
    ix = flat_index(gpu, X)
    ids0, s0 = exact(ix, Q, 64)
    ix.set_filter(1)
    try:
        ids1, s1, st1, fi1 = call(ix, Q, 64, monkeypatch, DIRECT1)
        assert fi1["direct_last_call"] and st1["fg_i8_launches"] == 1, (st1, fi1)
        assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
        assert st1["fallback_queries"] > 0 or st1["candidates"] > 1024, st1
        ids2, s2, st2, fi2 = call(ix, Q, 64, monkeypatch, DIRECT)
        assert not fi2["direct_last_call"] and st2["fg_i8_launches"] == 2, (st2, fi2)
        assert torch.equal(ids0, ids2) and torch.equal(s0, s2)
    finally:
        ix.set_filter(-1)


def test_knobs(gaussian, monkeypatch):
    ix, Q = gaussian[20000, 768]
    S = 256
    ids0, s0 = exact(ix, Q, 10)
    assert ix.filter_info()["schedule"] in ("bf16", "quarter")   # below the size rule: no schedule of its own
    for knobs, launches, direct in (({"CWQ_FG_I8_EARLY": "1"}, 5, False),     # the early schedule, as before
                                    ({"CWQ_FG_I8_EARLY": "0"}, 2, False),     # the quarter rule
                                    ({"CWQ_FG_I8_EARLY": "2", "CWQ_FG_CUTS": "8,16,32,64"}, 5, True),
                                    ({"CWQ_FG_I8_EARLY": "2", "CWQ_FG_CUTS": "128"}, 2, True),
                                    ({"CWQ_FG_I8_EARLY": "2", "CWQ_FG_I8": "-1"}, 0, False)):   # bf16 only
        ids1, s1, st, fi = filt(ix, Q, 10, monkeypatch, knobs)
        assert st["fg_i8_launches"] == launches and fi["direct_last_call"] == direct, (knobs, st, fi)
        assert st["sample_rows"] == S + S // 2 and st["fallback_queries"] == 0, (knobs, st)
        assert torch.equal(ids0, ids1) and torch.equal(s0, s1), knobs


def test_batch_split_invariance(gaussian, monkeypatch):
    ix, Q = gaussian[20000, 768]
    ids, s, st, fi = filt(ix, Q, 10, monkeypatch, DIRECT)
    assert fi["direct_last_call"]
    for a, b in ((0, 256), (100, 300)):
        ids1, s1, st1, fi1 = filt(ix, Q[a:b].contiguous(), 10, monkeypatch, DIRECT)
        assert fi1["direct_last_call"] and st1["fg_i8_launches"] == 5, (st1, fi1)
        assert torch.equal(ids[a:b], ids1) and torch.equal(s[a:b], s1)
