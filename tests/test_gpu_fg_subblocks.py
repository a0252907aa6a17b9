"""Sub-block flags and batched record claims of the raw filter epilogue (fgemm_kernel<0, true,
true, I8>, cwq_mfma.hip): one flag per 16-row x 16-query sub-block (jb, ib) of a wave's tile, and
one list claim per flagged sub-block.  Every case compares the filter (cwq_set_filter 1) with
the exact fp32 scan (mode 0): ids AND scores bit-identical.  A query that falls back to the
exact scan would hide a missed flag, so the cases assert fallback_queries == 0 as well (except
where the docstring says why not).

Layout behind the constructions (flat index: filter row r is leaf r): a tile is 256 queries x
256 rows; wave (wq, wr) owns queries wq * 128 .. + 127 and rows wr * 64 .. + 63; its sub-block
(jb, ib) is rows jb * 16 .. + 15 by queries ib * 16 .. + 15, and lane (r16, c16) holds row r16
and queries 4 c16 .. 4 c16 + 3 of it."""
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
    """The int8 panel of a small index: one call past the last phase builds it (bf16 only)."""
    _, _, st = filt(ix, Q[:1].repeat(65, 1), 1, mp, "99")
    assert st["fg_i8_launches"] == 0, st
    return ix


# Row tiles that get planted near-duplicates: 16 + 1 among the first quarter of the 512 row
# tiles (bf16 launches under the default policy), 16 + 1 among the rest (int8 launches).
BF_TILES = [3 + 7 * t for t in range(16)]      # .. 108
I8_TILES = [130 + 23 * t for t in range(16)]   # .. 475
ODD = ((120, 5), (500, 11))                    # (tile, shift)


@pytest.fixture(scope="module")
def positions(gpu):
    """131,072 x 64 (DPB 128: two int8 stages; 512 row tiles x 2 query tiles for 256
    workgroups: several tiles each, both pretest-term parities, carried lists), 300 queries (a
    padded second query tile).  In the t-th planted tile of either region, row (i + 16 t) mod
    256 is query i plus noise (i < 256): query block i / 16 meets row block (i / 16 + t) mod 16,
    so the 16 shifts put a survivor into every sub-block (jb, ib) of every wave, in lanes r16 =
    i mod 16, c16 = (i mod 16) / 4.  Two tiles with odd shifts (5, 11) hit lanes off that
    diagonal; the queries planted there (i mod 16 < 8) are left out of the last shifted tile
    of each region, whose sub-blocks keep 8 survivors each.  Every query i < 256 thus has
    exactly 32 near-duplicates, each tile with its own noise magnitude (0.02 .. 0.19, against
    a distance of about sqrt(128) to an unrelated row): its top 32 is that set, and a dropped
    sub-block is a missing id."""
    N, D, k = 131072, 64, 32
    X = gpu.synth.synthetic_corpus(N, D, seed=71)
    # (the first 256 queries fresh draws: a perturbed corpus row would be a 33rd near-duplicate)
    Q = torch.cat([gpu.synth.synthetic_corpus(256, D, seed=72), gpu.synth.synthetic_queries(X, 44, seed=74)[0]])
    noise = gpu.synth.synthetic_corpus(34 * 256, D, seed=73).view(34, 256, D)
    i = torch.arange(256, device=X.device)
    half = (i % 16) < 8
    planted = torch.zeros(256, dtype=torch.int64, device=X.device)
    tiles = [(tl, 16 * t) for t, tl in enumerate(BF_TILES)] + [(tl, 16 * t) for t, tl in enumerate(I8_TILES)]
    for n, (tl, shift) in enumerate(tiles + list(ODD)):
        if (tl, shift) in ODD:
            sel = half
        elif shift == 240:
            sel = ~half
        else:
            sel = torch.ones_like(half)
        rows = tl * 256 + (i + shift) % 256
        X[rows[sel]] = Q[:256][sel] + (0.02 + 0.005 * n) * noise[n][sel]
        planted += sel
    assert bool((planted == k).all())
    ix = flat_index(gpu, X)
    return ix, Q, k, exact(ix, Q, k)


@pytest.mark.parametrize("knob", [DEFAULT, OFF, FORCED])
def test_every_subblock_position(positions, knob, monkeypatch):
    """Forced from phase 0 the int8 launches run on the sample threshold and the lists may
    legitimately overflow: equality only there, the fallback count is printed."""
    ix, Q, k, (ids0, s0) = positions
    with_panel(ix, Q, monkeypatch)
    ids1, s1, st = filt(ix, Q, k, monkeypatch, knob)
    print("fallback_queries", st["fallback_queries"])
    assert (st["fg_i8_launches"] > 0) == (knob is not OFF), st
    if knob is not FORCED:
        assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    # the planted rows are what the exact scan finds (the construction is what it claims)
    tiles = torch.tensor(BF_TILES + I8_TILES + [t for t, _ in ODD])
    assert bool(torch.isin(ids0[:256] // 256, tiles).all())


@pytest.fixture(scope="module")
def dense(gpu):
    """test_dense_tiles' construction at 40,000 x 64 (157 row tiles; int8 from tile 39 on), once in
    each region: 16 identical rows aligned to a 16-row block (rows 80 .. 95 of the tile: wave
    wr = 1, jb = 1) and 64 queries next to them, aligned to four query blocks -- four full
    sub-blocks, each one claim of 256 records -- and 5 more copies of the row in the block
    before it (jb = 0, walked first: four claims of 80).  With a carried list of c < 256
    records the wave's first full claim covers slots 320 + c .. 575 + c, across kFgCap = 512
    (or a 80-record claim does), and the later ones lie in the overflow area entirely."""
    X = gpu.synth.synthetic_corpus(40000, 64, seed=81)
    Q = gpu.synth.synthetic_queries(X, 300, seed=82)[0]
    eps = gpu.synth.synthetic_corpus(128, 64, seed=83)
    for g, tile in enumerate((10, 100)):
        r = tile * 256 + 80
        X[r - 5:r + 16] = X[r]
        Q[64 * g:64 * g + 64] = X[r] + 0.01 * eps[64 * g:64 * g + 64]
    ix = flat_index(gpu, X)
    return ix, Q, exact(ix, Q, 16)


@pytest.mark.parametrize("knob", [DEFAULT, FORCED])
def test_full_subblock_and_straddling_claim(dense, knob, monkeypatch):
    ix, Q, (ids0, s0) = dense
    with_panel(ix, Q, monkeypatch)
    ids1, s1, st = filt(ix, Q, 16, monkeypatch, knob)
    assert st["fg_i8_launches"] == (2 if knob is DEFAULT else 5), st
    assert st["exact_reranks"] >= 21, st
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


def test_bf16_int8_exact_odd_dim(gpu, monkeypatch):
    """(3000, 200): D is not a multiple of 64, N and nq are not multiples of 256."""
    X = gpu.synth.synthetic_corpus(3000, 200, seed=3200)
    Q = gpu.synth.synthetic_queries(X, 300, seed=3000)[0]
    ix = flat_index(gpu, X)
    ids0, s0 = exact(ix, Q, 10)
    ids1, s1, st1 = filt(ix, Q, 10, monkeypatch, OFF)
    ids2, s2, st2 = filt(ix, Q, 10, monkeypatch, FORCED)
    assert st1["fg_i8_launches"] == 0 and st2["fg_i8_launches"] > 0, (st1, st2)
    assert st1["fallback_queries"] == 0 and st2["fallback_queries"] == 0, (st1, st2)
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    assert torch.equal(ids0, ids2) and torch.equal(s0, s2)
