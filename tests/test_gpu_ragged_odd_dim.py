"""Ragged ifit trees at odd dimensions through every query path, against fp64.

Six trees built by the oracle's own ifit (tests/lp_yardstick.py: D = 1, 3, 5, 17, 100, 23;
leaves at ragged depths 2..10, paths longer than the weight list, leaves with count > 1; the
D = 23 tree has 47 internal nodes and takes the internal pass's small form, the others the
general one) and one 17-dimensional tree built by the library's device ifit that is large
enough for the filters to engage.  None of these dimensions fills its last 16-wide chunk.

Yardstick: the fp64 log-likelihood of the fp32 node statistics, judged in the
condition-scaled unit of lp_yardstick (RTOL relative to the score cannot judge these shapes:
the log-probability crosses zero and the oracle itself misses 1e-5 there).  Every limit is
computed at run time from the reference: 4 x max(the oracle's own maximum on this tree in the
same units, 1); the 4 covers the other summation order (16-dimension partials) and the
reciprocal-sigma form.  Basic is checked against the library's exact heap replay for every
query and against OTree.categorize for the queries the oracle may judge (lp_yardstick.decisive).

An ifit tree has only isotropic leaf rows (a leaf of exact copies has meanSq = 0), so the
D = 3, 17 and 23 trees come a second time ("3s", "17s", "23s": lp_yardstick.spread) with a third
of their leaves spread per dimension and three sentences in internal nodes: anisotropic rows
among isotropic ones through the scan, the lists and the filters.

The measured figures (MI355X) stand in the docstring of the test that measures them; the
whole file takes 13 s, 3.7 s of it the device-ifit fixture, the slowest other test 1.5 s."""
import os
import random
import time

import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import lp_yardstick as L
from oracle import cobweb_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
DIMS = list(L.TREES)
SPREAD = ["3s", "17s", "23s"]      # lp_yardstick.spread: anisotropic leaf rows, sentences in internal nodes
ALL = DIMS + SPREAD


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


class Case:
    """One tree: the record, its 64 queries, the fp64 values and the oracle's own error."""

    def __init__(self, pkg, T, Q, weights=None):
        self.T, self.Q, self.weights = T, Q, weights
        self.pkg = pkg
        self.Qd = torch.from_numpy(Q).to(DEV)
        self.ix = self.index(weights)
        self.lp32 = L.oracle_lp32_rows(T, Q)
        self.ref = {f: L.lp64(T.mean, T.var, Q, full=f) for f in (False, True)}
        self.S = {f: L.scale(T.mean, T.var, Q, full=f) for f in (False, True)}
        self.oracle_units = {True: L.units(self.lp32, self.ref[True], self.S[True]).max(),
                             False: L.units(L.oracle_lpp32(T, Q), self.ref[False], self.S[False]).max()}
        self._rank = {}

    def index(self, weights=None):
        T = self.T
        return self.pkg.index.CobwebIndex(T.mean, T.var, T.parent, T.nos, weights, device=DEV)

    def limit(self, full):
        return 4.0 * max(self.oracle_units[full], 1.0)

    def rank(self, weights=None):
        """(fp64 scores, scale, limit) of Fast's rank scores under a weight list, once."""
        key = None if weights is None else tuple(weights)
        if key not in self._rank:
            T = self.T
            ref, S = L.rank_scores64(T, self.Q, weights)
            idx = O.flatten_tree(T.tree.root, len(T.nos), weights)
            pa = O.path_arrays(idx)
            orc = np.stack([O.rank_scores_vec(x, idx, pa) for x in self.Q[::4]])
            ou = L.units(orc, ref[::4], S[::4]).max()
            self._rank[key] = (ref, S, 4.0 * max(ou, 1.0), ou)
        return self._rank[key]


_cases = {}


def case(pkg, D):
    if D not in _cases:
        T, Q = L.spread(int(D[:-1])) if isinstance(D, str) else L.ragged(D)
        _cases[D] = Case(pkg, T, Q)
    return _cases[D]


def tiled(c, nq):
    """nq queries: the 64 repeated; (device tensor, index of each into the 64)."""
    idx = np.arange(nq) % L.NQ
    return c.Qd[torch.from_numpy(idx).to(DEV)].contiguous(), idx


# ---------------------------------------------------------------------------------------------
# a. node log-probabilities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ALL)
def test_node_logprob(gpu, D):
    """node_logprob (lp' and the full form) of every node against lp64, all 64 queries, in
    units; the finiteness patterns equal; the row of a query bit-identical whether the call
    holds 1 (raw_split), 7, 64, 65 (the shared-query scan configuration) or 257 queries
    (configuration 0).

    Measured on an MI355X, kernel max units (oracle max units; the limit is 4 x the oracle's):
      D      full form      lp'
      1      5.23 (3.66)    6.29 (4.14)
      3      4.18 (3.64)    4.11 (3.85)
      5      3.68 (3.74)    4.12 (3.33)
      17     4.29 (3.51)    4.95 (4.18)
      100    2.71 (3.17)    2.78 (3.57)
      23     3.31 (3.10)    3.69 (3.49)
      3s     4.18 (3.64)    4.46 (3.85)
      17s    5.11 (3.51)    5.08 (4.18)
      23s    3.31 (3.10)    3.81 (3.39)"""
    c = case(gpu, D)
    for full in (True, False):
        ref, S, lim = c.ref[full], c.S[full], c.limit(full)
        base = c.ix.node_logprob(c.Qd, full=full).cpu().numpy()
        u = L.units(base, ref, S)
        print(f"D={D} full={full}: kernel max {u.max():.2f} units, oracle max {c.oracle_units[full]:.2f}, limit {lim:.2f}")
        assert u.max() <= lim, (D, full, u.max(), lim)
        for nq in (1, 7, 65, 257):
            Qn, idx = tiled(c, nq)
            got = c.ix.node_logprob(Qn, full=full).cpu().numpy()
            assert np.array_equal(got, base[idx]), (D, full, nq)
        # a query alone, wherever it sits in the batch
        for qi in (31, 32, 63):
            one = c.ix.node_logprob(c.Qd[qi:qi + 1].contiguous(), full=full).cpu().numpy()
            assert np.array_equal(one[0], base[qi]), (D, full, qi)


# ---------------------------------------------------------------------------------------------
# b. rank scores and Fast
# ---------------------------------------------------------------------------------------------
def all_modes(ix, Q, k):
    out = []
    for mode in (0, 1, -1):
        ix.set_filter(mode)
        ids, sc = ix.score_topk(Q, k)
        out.append((ids.cpu().numpy(), sc.cpu().numpy()))
    ix.set_filter(-1)
    for mode, (ids, sc) in zip((1, -1), out[1:]):
        assert np.array_equal(ids, out[0][0]) and np.array_equal(sc.view(np.int32), out[0][1].view(np.int32)), (k, mode)
    return out[0]


def check_topk(ids, sc, ref, S, nos, lim, k):
    """One query's top-k against the fp64 ranking: a position that differs holds two sentences
    whose fp64 scores are closer than both may err, lim units each; the scores within lim."""
    n = len(nos)
    m = min(k, n)
    order = L.rank_order64(ref, nos)[:m]
    assert np.all(ids[m:] == -1)
    got = ids[:m]
    assert len(set(got.tolist())) == m and got.min() >= 0 and got.max() < n
    for a, b in zip(got, order):
        if a != b:
            assert abs(ref[a] - ref[b]) <= lim * L.EPS * (S[a] + S[b]), (a, b, ref[a], ref[b])
    u = L.units(sc[:m], ref[got], S[got])
    assert u.max() <= lim, (u.max(), lim)
    assert np.all(np.diff(sc[:m]) <= 0)


@pytest.mark.parametrize("D", ALL)
def test_rank_scores_and_fast(gpu, D):
    """rank_scores against the fp64 path-weighted mean in units; score_topk by the exact scan,
    the forced filter and the automatic choice bit-identical, for k = 1, 5, 16, 17, 64, 70 and
    n + 3, with 1, 64 (stream path) and 65 (batch path) queries per call; the ids against the
    fp64 ranking, -1 past the sentence count.

    Measured on an MI355X, rank_scores kernel max units (oracle max units, every fourth query):
      D = 1: 3.65 (3.48)   3: 2.91 (3.80)   5: 2.95 (3.12)   17: 3.09 (2.83)   100: 2.17 (2.08)
      23: 2.95 (2.66)   3s: 3.10 (2.89)   17s: 3.44 (3.07)   23s: 2.95 (3.29)"""
    c = case(gpu, D)
    ref, S, lim, ou = c.rank()
    n = len(c.T.nos)
    rs = c.ix.rank_scores(c.Qd).cpu().numpy()
    u = L.units(rs, ref, S)
    print(f"D={D}: rank_scores kernel max {u.max():.2f} units, oracle max {ou:.2f}, limit {lim:.2f}; "
          f"index {c.ix.info}")
    assert u.max() <= lim, (D, u.max(), lim)
    for k in (1, 5, 16, 17, 64, 70, n + 3):
        full = None
        for nq in (64, 1, 65):
            Qn, idx = tiled(c, nq)
            ids, sc = all_modes(c.ix, Qn, k)
            if full is None:
                full = (ids, sc)
                for qi in range(L.NQ):
                    check_topk(ids[qi], sc[qi], ref[qi], S[qi], c.T.nos, lim, k)
                # the scores are rank_scores' own values
                m = min(k, n)
                assert np.array_equal(sc[:, :m], np.take_along_axis(rs, ids[:, :m], 1)), k
            else:
                assert np.array_equal(ids, full[0][idx]) and np.array_equal(sc, full[1][idx]), (D, k, nq)


# ---------------------------------------------------------------------------------------------
# c. level weights
# ---------------------------------------------------------------------------------------------
WEIGHTS = {"short": [1.0, 2.0, 0.5], "zero inside": [0.25, 1.0, 3.0, 1.0, 0.0, 2.0],
           "negative": [1.0, -0.5, 2.0, 0.75], "all zero": [0.0, 0.0, 0.0]}


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("D", [3, 17, 23])
def test_level_weights(gpu, D, wname):
    """Weight lists shorter than the deepest path (weight 1.0 past the end), with a zero, a
    negative entry, and all zero (only the levels past the list count; a sentence whose whole
    path lies inside it scores exactly 0): rank_scores against rank_scores64 in units, Fast
    equal across the three strategies."""
    c = case(gpu, D)
    w = WEIGHTS[wname]
    assert c.T.depth.max() >= len(w) or wname == "zero inside"
    ref, S, lim, ou = c.rank(w)
    ix = c.index(w)
    rs = ix.rank_scores(c.Qd).cpu().numpy()
    u = L.units(rs, ref, S)
    print(f"D={D} weights {wname}: rank_scores kernel max {u.max():.2f} units, oracle max {ou:.2f}, limit {lim:.2f}")
    assert u.max() <= lim, (D, wname, u.max(), lim)
    for k in (1, 10, 64):
        for nq in (64, 1, 65):
            Qn, idx = tiled(c, nq)
            ids, sc = all_modes(ix, Qn, k)
            if wname != "all zero":        # (all zero: whole tie groups at 0; the order is the tie rule's)
                for j in (0, nq - 1):
                    check_topk(ids[j], sc[j], ref[idx[j]], S[idx[j]], c.T.nos, lim, k)
    ix.close()


# ---------------------------------------------------------------------------------------------
# d. Basic
# ---------------------------------------------------------------------------------------------
def exact_replay(ix, Q, k, mx):
    """The library's exact heap replay on the exact scan's keys (test_gpu_group.check_basic)."""
    ix.set_filter(0)
    os.environ["CWQ_CAT_COUNT"] = "0"
    try:
        return ix.categorize(Q, k, mx)
    finally:
        del os.environ["CWQ_CAT_COUNT"]
        ix.set_filter(-1)


def same(ref, got, what):
    for name, a, b in zip(("nodes", "n_found", "n_calls"), ref, got):
        assert torch.equal(a, b), (what, name)


def basic_against_replay(ix, Qd, k, mx, monkeypatch, what):
    ref = exact_replay(ix, Qd, k, mx)
    same(ref, ix.categorize(Qd, k, mx), (what, "lists"))             # the conftest's pinned list paths
    monkeypatch.setenv("CWQ_CAT_DIRECT", "1")
    for pre in ("0", "1"):
        monkeypatch.setenv("CWQ_LAZY_PRE", pre)
        same(ref, ix.categorize(Qd, k, mx), (what, "direct", pre))
    monkeypatch.delenv("CWQ_LAZY_PRE")
    monkeypatch.setenv("CWQ_CAT_DIRECT", "0")
    return ref


def basic_against_oracle(T, Q, lp32, ref64, got, k, mx, queries):
    """The decisive queries of `queries` against OTree.categorize; returns how many there were."""
    nodes, found, calls = (t.cpu().numpy() for t in got)
    nd = 0
    for qi in queries:
        dec, ret, ncalls, short = L.decisive(T, Q[qi], k, mx, lp32[qi], ref64[qi])
        if not dec:
            continue
        nd += 1
        want, wcalls, wshort = L.oracle_categorize(T, Q[qi], k, mx)
        assert wshort == short
        if not short:      # (where the reference raises IndexError the watched search has its list)
            assert (want, wcalls) == (ret, ncalls), qi
        assert (int(found[qi]) < k) == short, (qi, k, mx)
        assert nodes[qi][:found[qi]].tolist() == ret and np.all(nodes[qi][found[qi]:] == -1), (qi, k, mx)
        assert int(calls[qi]) == ncalls, (qi, k, mx)
    return nd


@pytest.mark.parametrize("D", ALL)
def test_basic(gpu, D, monkeypatch):
    """categorize for (k, max_nodes) = (1, 5, 20, 70 with no limit; 5 with 12 nodes): every
    query equals the exact heap replay under the list paths and under the exact lazy replay
    (both run-merge kernels), 64 queries per call and one per call; every decisive query equals
    OTree.categorize: nodes, log_prob calls, and fewer than k found exactly where the reference
    raises IndexError.

    Measured: every decisive query equal to the oracle; their numbers of 64, for the five cases
    in this order, D = 1: 63 59 59 62 59; 3: 64 63 60 64 54; 5: 64 62 53 64 20; 17: 58 56 42 64
    23; 100: 56 51 51 62 30; 23: 63 60 56 63 37; 3s: 64 64 62 64 57; 17s: 64 64 56 64 46;
    23s: 64 62 59 63 52 (the counts of tests/test_lp_yardstick_cpu.py)."""
    c = case(gpu, D)
    for k, mx in L.BASIC:
        ref = basic_against_replay(c.ix, c.Qd, k, mx, monkeypatch, (D, k, mx))
        nd = basic_against_oracle(c.T, c.Q, c.lp32, c.ref[True], ref, k, mx, range(L.NQ))
        print(f"D={D} k={k} max_nodes={mx}: {nd} decisive queries equal the oracle")
        assert nd >= L.DECISIVE_MIN[(k, mx)]
        for qi in range(8):
            one = basic_against_replay(c.ix, c.Qd[qi:qi + 1].contiguous(), k, mx, monkeypatch, (D, k, mx, qi))
            same([t[qi:qi + 1] for t in ref], one, (D, k, mx, qi, "alone"))


# ---------------------------------------------------------------------------------------------
# e. gradient and ranking loss
# ---------------------------------------------------------------------------------------------
GRAD_Q = [0, 1, 2, 3, 32, 33, 34, 35]     # four near queries, four far ones


@pytest.mark.parametrize("D", [5, 17, 23, "17s"])
def test_gradient_and_rank_ce(gpu, D):
    """rank_scores_backward under grad_yardstick's rule (three upstreams, rel_l2 < LIMIT against
    fp64 autograd) and rank_ce under ce_yardstick's (test_gpu_rank_ce.run_checks), on the dense
    scorer written out from this tree's arrays."""
    import test_gpu_grad as TG
    import test_gpu_rank_ce as TC
    c = case(gpu, D)
    T = c.T
    Xq = c.Q[GRAD_Q]
    P = Y.path_matrix(T.parent, T.nos)
    d64, d32 = Y.Dense(T.mean, T.var, P, torch.float64), Y.Dense(T.mean, T.var, P, torch.float32)
    _, cases = Y.upstreams(d64, Xq)
    for name, (G64, g64) in cases.items():
        TG.check_case(c.ix, Xq, d32, G64, g64, f"ragged D={D} {name}")
    tg, temps, _ = C.targets_and_temps(d64, Xq)
    l64, g64 = C.ce_through(d64, Xq, tg, temps)
    l32, g32 = C.ce_through(d32, Xq, tg, temps)
    ends = {"std": (temps, l64, g64, np.abs(l32 - l64) / np.abs(l64), Y.rel_l2(g32, g64))}
    _, rank = TC.run_checks(c.ix, Xq, T.nos, tg, ends, f"ragged D={D}")
    TC.check_topk(c.ix, Xq, tg, rank)


# ---------------------------------------------------------------------------------------------
# f. prefix bounds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [17, 100, "17s"])
def test_prefix_bounds(gpu, D):
    """The exact pass's internal prefixes against the fp64 prefix in units, and the filter's
    bf16 bounds around them: lo <= exact <= hi in fp32 wherever the filter reads a bound, which
    includes every internal node with an isotropic leaf row below it.

    Measured (MI355X): exact prefixes at most 4.05 units at D = 17 and on "17s", 2.00 at D = 100
    (the oracle's lp' 4.18 and 3.57)."""
    c = case(gpu, D)
    T = c.T
    lo, hi, ex = (t.cpu().numpy() for t in c.ix.prefix_bounds(c.Qd))
    internal = np.nonzero(~T.is_leaf)[0]
    assert ex.shape == (L.NQ, len(internal))
    ref = L.path_prefix(T.parent, T.depth, c.ref[False])[:, internal]
    S = L.path_prefix(T.parent, T.depth, c.S[False], absolute=True)[:, internal]
    lim = c.limit(False)
    u = L.units(ex, ref, S)
    print(f"D={D}: exact prefixes max {u.max():.2f} units (oracle lp' max {c.oracle_units[False]:.2f}, limit {lim:.2f})")
    assert u.max() <= lim
    fin = np.isfinite(lo) & np.isfinite(hi)
    iso = (T.var.view(np.int32) == T.var.view(np.int32)[:, :1]).all(1)
    need = np.zeros(len(T.parent), bool)
    need[T.parent[1:][T.is_leaf[1:] & iso[1:]]] = True
    assert fin[:, need[internal]].all(), "an internal node with isotropic leaf rows has no bounds"
    assert np.all((lo <= ex)[fin]) and np.all((ex <= hi)[fin])


# ---------------------------------------------------------------------------------------------
# g. a tree large enough for the filters to engage
# ---------------------------------------------------------------------------------------------
BIG_N, BIG_D, BIG_CLUSTERS, BIG_NQ = 20_000, 17, 12, 300


@pytest.fixture(scope="module")
def big(gpu):
    """20,000 x 17 in 12 clusters through the library's device ifit; its arrays exported to the
    oracle as test_gpu_c2 does, so the checks do not depend on how the tree was built.
    (n and the build time: see test_big_tree_filters_engage.)"""
    rng = np.random.default_rng(BIG_D + BIG_N)
    X = L.corpus(BIG_D, BIG_N, BIG_CLUSTERS, rng)
    Q = L.queries(X, rng, BIG_NQ)
    random.seed(BIG_D + BIG_N)
    old = os.environ.get("CWQ_FIT_DEVICE")
    os.environ["CWQ_FIT_DEVICE"] = "1"
    try:
        t0 = time.perf_counter()
        w = gpu.CobwebWrapper(corpus=[None] * BIG_N, corpus_embeddings=X)
        w.build_prediction_index()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        if old is None:
            del os.environ["CWQ_FIT_DEVICE"]
        else:
            os.environ["CWQ_FIT_DEVICE"] = old
    nodes = w._nodes
    parent = w.tree.flatten(BIG_N)[1]
    sid_ptr = np.concatenate([[0], np.cumsum([len(n.sentence_id or []) for n in nodes])]).astype(np.int64)
    sid_list = np.array([s for n in nodes for s in (n.sentence_id or [])], np.int64)
    T = L.from_arrays(np.asarray(parent, np.int64), np.array([n.count for n in nodes], np.float32),
                      np.stack([n.mean for n in nodes]), np.stack([n.meanSq for n in nodes]), sid_ptr, sid_list,
                      BIG_N, X)
    print(f"device ifit of {BIG_N} x {BIG_D}: {dt:.2f} s with the index; {w._index.info}")
    yield w, T, Q, torch.from_numpy(Q).to(DEV), dt
    w._invalidate_prediction_index()


def test_big_tree_filters_engage(big, monkeypatch):
    """n = 20,000: the device ifit with the index build takes 3.2 - 3.3 s on an MI355X (29,316
    nodes, depth 11), so the first size tried stays; with 20,000 isotropic rows the automatic
    choice takes the batch filter as well.  Measured: rank_scores 2.69 units (oracle 2.66), 15
    of the first 16 queries decisive.  The forced filter is used for 64 queries (stream) and 300
    (batch); the three strategies bit-identical for k = 1, 10, 64; 8 queries agree with
    rank_scores64 and its fp64 top-k; Basic equals the exact replay for all queries and the
    oracle on the decisive ones among the first 16."""
    w, T, Q, Qd, dt = big
    ix = w._index
    assert ix.info["max_depth"] >= 5 and ix.info["n_sent"] == BIG_N
    for nq, path in ((64, "stream"), (BIG_NQ, "fgemm")):
        ix.set_filter(1)
        ix.score_topk(Qd[:nq].contiguous(), 10)
        st = ix.last_stats()
        assert st["filter_used"] and st["path"] == path, (nq, st)
        for k in (1, 10, 64):
            all_modes(ix, Qd[:nq].contiguous(), k)
    qs = [0, 1, 31, 149, 150, 151, 250, 299]
    ref, S = L.rank_scores64(T, Q[qs])
    pa = O.path_arrays(T.flat)
    ou = L.units(np.stack([O.rank_scores_vec(Q[q], T.flat, pa) for q in qs]), ref, S).max()
    lim = 4.0 * max(ou, 1.0)
    rs = ix.rank_scores(Qd[qs]).cpu().numpy()
    u = L.units(rs, ref, S)
    print(f"big tree: rank_scores kernel max {u.max():.2f} units, oracle max {ou:.2f}, limit {lim:.2f}")
    assert u.max() <= lim
    ids, sc = all_modes(ix, Qd[qs].contiguous(), 10)
    for j in range(len(qs)):
        check_topk(ids[j], sc[j], ref[j], S[j], T.nos, lim, 10)
    k, mx = 10, 100000
    got = basic_against_replay(ix, Qd, k, mx, monkeypatch, "big")
    first = range(16)
    lp32 = L.oracle_lp32_rows(T, Q[:16])
    nd = basic_against_oracle(T, Q, lp32, L.lp64(T.mean, T.var, Q[:16]), got, k, mx, first)
    print(f"big tree: {nd} of 16 queries decisive and equal to the oracle")
    assert nd >= 4
