"""Staged records of the raw filter epilogue (fgemm_kernel<0, true, true, I8>, cwq_mfma.hip): the
pretest writes a flagged sub-block's survivors to the wave's staging area (256 records), the wave
commits them to the carried list (kFgCap = 512 slots) with one claim per tile, a sub-block that
does not fit the area is deferred whole to the rolled walk, and records past the list's end are
drained from the area.  Every case compares the filter (cwq_set_filter 1) with the exact fp32 scan
(mode 0): ids AND scores bit-identical, and fallback_queries == 0 -- a query re-run by the exact
scan would hide a lost record.

Layout behind the constructions (flat index: filter row r is leaf r): a tile is 256 queries x 256
rows; wave (wq, wr) owns queries wq * 128 .. + 127 and rows wr * 64 .. + 63; its sub-block (jb, ib)
is rows jb * 16 .. + 15 by queries ib * 16 .. + 15.  The pretest visits a wave's sub-blocks with
ib outermost (ib = 0: jb = 0 .. 3, then ib = 1, ...); the walk takes the deferred ones in the
order jb * 8 + ib.  Waves 0 .. 3 (wr = 0, 1) enter the epilogue one barrier interval before waves
4 .. 7.  Under the default policy the first quarter of the row tiles runs in bf16 launches and the
rest in int8 launches; CWQ_FG_I8 = -1 / 0 takes every tile through the one or the other.  The int8
instantiation stages; the bf16 one defers every flagged sub-block to the walk, and runs the same
constructions through the walk's claims and its overflow drain."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORCED, DEFAULT, OFF = "0", None, "-1"
KNOBS = [DEFAULT, OFF, FORCED]


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


def check(ix, Q, k, ref, planted, mp, knob):
    """Filter == exact scan, no fallback, and the construction's premise: the exact scan's top
    min(k, copies) of a planted query are planted rows."""
    ids0, s0 = ref[k]
    for qs, rows in planted:
        n = min(k, len(rows))
        got = ids0[qs][:, :n]
        assert bool(torch.isin(got, torch.tensor(rows)).all()), (qs, got)
    with_panel(ix, Q, mp)
    ids1, s1, st = filt(ix, Q, k, mp, knob)
    assert (st["fg_i8_launches"] > 0) == (knob is not OFF), st
    assert st["fallback_queries"] == 0, st
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)


# (name, bf16-region tile, int8-region tile, first query, local rows): 16 queries first .. + 15, one
# aligned query block, next to one vector of which every listed row of both tiles is a copy.
# 40,000 rows: 157 row tiles, int8 from tile 39 on; queries 0 .. 255: query tile 0, wq = 0 up to 127.
R = lambda a, n: list(range(a, a + n))   # noqa: E731
CASES = [
    # one sub-block of 256 survivors in wave (0, 1): staged, area exactly full, nothing deferred
    ("full", 5, 60, 0, R(80, 16)),
    # + a copy in sub-block jb = 2 of the same wave, visited after the full one: 16 more, deferred
    ("full_then_more", 8, 70, 16, R(80, 16) + [99]),
    # + a copy in sub-block jb = 0, visited before: 16 staged, the full sub-block deferred to the walk
    ("more_then_full", 11, 80, 32, [67] + R(80, 16)),
    # commit across kFgCap: waves (0, wr) stage 256, 80, 208 and 256 records.  In every order of the
    # four commits but one (both 256 first) a batch meets a carried count of 256 < c < 512 and
    # straddles slot 512, and the last batch (c >= 544) goes through the overflow drain whole.
    ("straddle", 14, 90, 48, R(0, 16) + R(64, 5) + R(128, 13) + R(192, 16)),
    # four batches of 256: slots 0 .. 1023, the last two drained whole (c = 512, 768)
    ("past_cap", 17, 100, 64, R(0, 16) + R(64, 16) + R(128, 16) + R(192, 16)),
    # wave (0, 1) alone, four full sub-blocks: jb = 0 staged and committed, jb = 1 .. 3 deferred; the
    # walk's 768 appends run past slot 512 and reuse the area the commit just read as overflow area
    ("staged_and_overflowing_walk", 20, 110, 80, R(64, 64)),
]


@pytest.fixture(scope="module")
def small(gpu):
    """40,000 x 64 (DPB 128: two int8 stages), 300 queries: the second query tile is padded past
    query 299 and the last row tile (156) past row 39,999.  CASES, and the edge case: rows 39,984
    .. 39,999 (tile 156, wave wr = 0, jb = 3, the last valid row in lane r16 = 15) copies of one
    vector next to queries 288 .. 299 (query tile 1, ib = 2, the last valid query in its lane's
    fourth element)."""
    X = gpu.synth.synthetic_corpus(40000, 64, seed=91)
    Q = gpu.synth.synthetic_queries(X, 300, seed=92)[0]
    V = gpu.synth.synthetic_corpus(len(CASES) + 1, 64, seed=93)
    eps = gpu.synth.synthetic_corpus(300, 64, seed=94)
    planted = {}
    for c, (name, tb, ti, q, rows) in enumerate(CASES):
        allrows = [t * 256 + r for t in (tb, ti) for r in rows]
        X[allrows] = V[c]
        Q[q:q + 16] = V[c] + 0.01 * eps[q:q + 16]
        planted[name] = (slice(q, q + 16), allrows)
    X[39984:40000] = V[-1]
    Q[288:300] = V[-1] + 0.01 * eps[288:300]
    planted["edges"] = (slice(288, 300), R(39984, 16))
    ix = flat_index(gpu, X)
    return ix, Q, {k: exact(ix, Q, k) for k in (1, 10, 32)}, list(planted.values())


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("k", [1, 10, 32])
def test_staging_area_commit_and_fallback(small, k, knob, monkeypatch):
    ix, Q, ref, planted = small
    check(ix, Q, k, ref, planted, monkeypatch, knob)


E_TILES = [2 + 8 * n for n in range(64)]     # 16 in the bf16 region (tiles < 128), 48 in the int8 one
F_TILES = [1 + 4 * n for n in range(128)]    # .. 509 of 512
E_QUERIES = [wq * 128 + 16 * wr + 3 for wq in range(2) for wr in range(4)]


@pytest.fixture(scope="module")
def eight(gpu):
    """131,072 x 64: 512 row tiles x 2 query tiles for 256 workgroups -- four tiles each, claimed
    at run time, so the constructions are repeated over many tiles to meet every position in a
    workgroup's sequence.  E tiles (64): for each wave (wq, wr), query wq * 128 + 16 wr + 3 has
    one near-duplicate in the wave's rows (row block (wq + wr) mod 4), each tile with its own
    noise magnitude: all eight waves stage one record and commit it, in first, odd and even
    tiles of a workgroup.  F tiles (128, every fourth row tile): 16 copies of one vector next to
    one of four blocks of 16 queries (64 .. 127): 256 records, so the workgroup's next tile
    starts with a flush; with a quarter of the row tiles of query tile 0 flushing, some of the
    64 E tiles follow one directly (none does with probability (7/8)^64)."""
    N, D = 131072, 64
    assert max(E_TILES + F_TILES) < N // 256 and not set(E_TILES) & set(F_TILES)
    X = gpu.synth.synthetic_corpus(N, D, seed=95)
    Q = torch.cat([gpu.synth.synthetic_corpus(256, D, seed=96), gpu.synth.synthetic_queries(X, 44, seed=97)[0]])
    noise = gpu.synth.synthetic_corpus(64 * 8, D, seed=98).view(64, 8, D)
    V = gpu.synth.synthetic_corpus(4, D, seed=99)
    eps = gpu.synth.synthetic_corpus(64, D, seed=100)
    planted = []
    erows = [[] for _ in E_QUERIES]
    for n, t in enumerate(E_TILES):
        for e, q in enumerate(E_QUERIES):
            wq, wr = e // 4, e % 4
            row = t * 256 + wr * 64 + 16 * ((wq + wr) % 4) + 9
            X[row] = Q[q] + (0.02 + 0.002 * n) * noise[n][e]
            erows[e].append(row)
    planted += [(slice(q, q + 1), rows) for q, rows in zip(E_QUERIES, erows)]
    for g in range(4):
        rows = [t * 256 + 144 + r for t in F_TILES[g::4] for r in range(16)]
        X[rows] = V[g]
        Q[64 + 16 * g:80 + 16 * g] = V[g] + 0.01 * eps[16 * g:16 * g + 16]
        planted.append((slice(64 + 16 * g, 80 + 16 * g), rows))
    ix = flat_index(gpu, X)
    return ix, Q, {k: exact(ix, Q, k) for k in (1, 32)}, planted


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("k", [1, 32])
def test_eight_waves_commit_every_parity_and_after_flush(eight, k, knob, monkeypatch):
    ix, Q, ref, planted = eight
    check(ix, Q, k, ref, planted, monkeypatch, knob)
