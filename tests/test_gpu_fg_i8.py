"""Int8 first-level launches of the batch filter (fgemm_kernel<0, true, true, true> +
bucket_raw_kernel's int8 bounds, cwq_mfma.hip; the policy and the CWQ_FG_I8 knob in
cwq_filter.hip run_iso_filter / fg_i8_from).  Every case compares the filter (cwq_set_filter 1)
with the exact fp32 scan (mode 0): ids AND scores bit-identical.

CWQ_FG_I8 is read per call: negative = bf16 only, n >= 0 = int8 from filter phase n on (the
int8 panel is built whatever the index's size), unset = the default policy (int8 from a
quarter of the row tiles on, on an index that has its panel).  The indices here are far
below the size at which an index gets its panel by itself, so the default-policy cases
first make one call with CWQ_FG_I8=99: past the last phase, it builds the panel and runs
bf16 only."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORCED, DEFAULT, OFF = "0", None, "-1"


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


def flat_index(pkg, X):
    fs = pkg.synth.flat_synth(X)
    return pkg.index.CobwebIndex(fs["mean"], fs["var"], fs["parent"], fs["node_of_sentence"], device="cuda:0")


def filt(ix, Q, k, mp, knob):
    """One filter call under CWQ_FG_I8 = knob (None: unset) -> ids, scores, stats."""
    if knob is None:
        mp.delenv("CWQ_FG_I8", raising=False)
    else:
        mp.setenv("CWQ_FG_I8", knob)
    ix.set_filter(1)
    ids, s = ix.score_topk(Q, k)
    st = ix.last_stats()
    ix.set_filter(-1)
    mp.delenv("CWQ_FG_I8", raising=False)
    print(knob, st)
    assert st["filter_used"] and st["path"] == "fgemm", st
    return ids.cpu(), s.cpu(), st


def exact(ix, Q, k):
    ix.set_filter(0)
    ids, s = ix.score_topk(Q, k)
    assert not ix.last_stats()["filter_used"]
    ix.set_filter(-1)
    return ids.cpu(), s.cpu()


def with_panel(ix, Q, mp):
    _, _, st = filt(ix, Q[:1].repeat(65, 1), 1, mp, "99")   # (65 queries: the batch path)
    assert st["fg_i8_launches"] == 0, st
    return ix


@pytest.fixture(scope="module")
def small_flat(gpu):
    """The two small flat shapes (N, nq not multiples of 256; D not a multiple of 64; DPB 128:
    two int8 stages per tile, and 256), built once."""
    out = {}
    for N, D in ((5000, 64), (3000, 200)):
        X = gpu.synth.synthetic_corpus(N, D, seed=N + D)
        out[N, D] = (flat_index(gpu, X), gpu.synth.synthetic_queries(X, 300, seed=N)[0])
    return out


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("N,D", [(5000, 64), (3000, 200)])
def test_small_flat(small_flat, N, D, k, monkeypatch):
    ix, Q = small_flat[N, D]
    ids0, s0 = exact(ix, Q, k)
    ids1, s1, st = filt(ix, Q, k, monkeypatch, FORCED)
    assert st["filter_queries"] == 300
    assert st["fg_i8_launches"] == (5 if N == 5000 else 1), st   # every launch (20 / 12 row tiles)
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    ids2, s2, st = filt(ix, Q, k, monkeypatch, DEFAULT)   # the panel exists now
    # 20 tiles: the launches from tiles 5 and 10 on; 12 tiles: one launch, from tile 0 -- bf16
    assert st["fg_i8_launches"] == (2 if N == 5000 else 0), st
    assert torch.equal(ids0, ids2) and torch.equal(s0, s2)


def test_c3_distribution_small(gpu, monkeypatch):
    """C3's rows and queries (N(0, I), 768-d) at 20,000 rows, default policy."""
    X = gpu.synth.synthetic_corpus(20000, 768, seed=41)
    Q, _ = gpu.synth.synthetic_queries(X, 300, seed=42)
    ix = with_panel(flat_index(gpu, X), Q, monkeypatch)
    ids0, s0 = exact(ix, Q, 10)
    ids1, s1, st = filt(ix, Q, 10, monkeypatch, DEFAULT)
    assert st["fg_i8_launches"] == 2, st
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


@pytest.fixture(scope="module")
def many_tiles(gpu):
    X = gpu.synth.synthetic_corpus(262144, 32, seed=31)
    Q, _ = gpu.synth.synthetic_queries(X, 512, seed=32)
    ix = flat_index(gpu, X)
    return ix, Q, exact(ix, Q, 64)


@pytest.mark.parametrize("knob", [DEFAULT, FORCED])
def test_records_carried_over_tiles(many_tiles, knob, monkeypatch):
    """1,024 tiles for 256 workgroups and hundreds of candidates per query: every workgroup
    carries its record list over several tiles and flushes it in mid-launch.  Forced from
    phase 0 the int8 launches run on the sample threshold and the lists may overflow: the
    exact re-run is then the designed outcome, so only the default policy bounds it."""
    ix, Q, (ids0, s0) = many_tiles
    with_panel(ix, Q, monkeypatch)
    ids1, s1, st = filt(ix, Q, 64, monkeypatch, knob)
    assert st["fg_i8_launches"] == (2 if knob is DEFAULT else 5), st
    if knob is DEFAULT:
        assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


def test_dense_tiles(gpu, monkeypatch):
    """Ten groups of 12 identical rows, 30 queries next to each (test_gpu_fg_records'
    construction): seven of the groups lie in the int8 launches' rows."""
    X = gpu.synth.synthetic_corpus(40000, 64, seed=33)
    for g in range(10):
        X[4000 * g + 100:4000 * g + 112] = X[4000 * g + 100]
    Q = X[100:40000:4000].repeat(30, 1) + 0.01 * gpu.synth.synthetic_corpus(300, 64, seed=34)
    ix = with_panel(flat_index(gpu, X), Q, monkeypatch)
    ids0, s0 = exact(ix, Q, 10)
    ids1, s1, st = filt(ix, Q, 10, monkeypatch, DEFAULT)
    assert st["fg_i8_launches"] == 2, st
    assert st["exact_reranks"] >= 12, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


@pytest.mark.parametrize("case", ["one_component_x1000", "scale_0.01"])
def test_hostile_quantisation(gpu, case, monkeypatch):
    """Rows whose per-row int8 scale zeroes all components but one, and rows of tiny scale:
    the bounds are wide or tight in absolute terms, the answer is the exact scan's (a
    fallback to it is allowed; the call returns)."""
    if case == "scale_0.01":
        X = gpu.synth.synthetic_corpus(8000, 128, seed=21) * 0.01
        Q, _ = gpu.synth.synthetic_queries(X, 200, seed=22, sigma=0.001)
    else:
        X = gpu.synth.synthetic_corpus(4000, 64, seed=51)
        X[:, 7] *= 1000.0
        Q, _ = gpu.synth.synthetic_queries(X, 200, seed=52)
    ix = flat_index(gpu, X)
    ids0, s0 = exact(ix, Q, 10)
    ids1, s1, st = filt(ix, Q, 10, monkeypatch, FORCED)
    assert st["fg_i8_launches"] == 5, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


def test_i8_path_equals_bf16_path(small_flat, monkeypatch):
    ix, Q = small_flat[5000, 64]
    ids1, s1, st1 = filt(ix, Q, 10, monkeypatch, OFF)
    ids2, s2, st2 = filt(ix, Q, 10, monkeypatch, FORCED)
    assert st1["fg_i8_launches"] == 0 and st2["fg_i8_launches"] == 5, (st1, st2)
    assert torch.equal(ids1, ids2) and torch.equal(s1, s2)
