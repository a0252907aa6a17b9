"""What tests/test_gpu_ragged_odd_dim.py assumes about its six trees and its yardstick
(tests/lp_yardstick.py), pinned on the CPU so that a change of seed or recipe cannot quietly
empty the GPU tests.

Measured with the recipe as written (seed = D + n), D = 1, 3, 5, 17, 100, 23:
  nodes / internal nodes     552/255  672/275  320/122  2177/685  810/215  196/47
  leaf depth                 4..10    4..10    3..7     3..8      3..6     2..5
  leaves with count > 1      3        3        2        8         5        1
  oracle log_prob, max units (every fourth query, all nodes)
                             3.46     3.39     2.84     3.34      2.66     3.04
  oracle pairs over 1e-5 relative (every fourth query)
                             9/8832   7/10752  3/5120   1/34832   0        0
  decisive queries of 64, (k, max_nodes) =
    (1, 100000)              63       64       64       58        56       63
    (5, 100000)              59       63       62       56        51       60
    (20, 100000)             59       60       53       42        51       56
    (5, 12)                  62       64       64       64        62       63
    (70, 100000)             59       54       20       23        30       37
  queries short of k at max_nodes = 12
                             64       64       61       64        64       64"""
import numpy as np
import pytest

import lp_yardstick as L
from oracle import cobweb_oracle as O

DIMS = list(L.TREES)


@pytest.fixture(scope="module", params=DIMS, ids=[f"D{d}" for d in DIMS])
def case(request):
    T, Q = L.ragged(request.param)
    return request.param, T, Q, L.oracle_lp32(T, Q), L.lp64(T.mean, T.var, Q)


def test_tree_shape(case):
    D, T, Q, _, _ = case
    leaf = T.is_leaf
    print(f"D={D}: nodes {len(T.parent)} internal {T.n_internal} leaf depth {T.depth[leaf].min()}..{T.depth[leaf].max()} "
          f"leaves with count > 1: {int((T.count[leaf] > 1).sum())}")
    assert (len(T.parent), T.n_internal) == L.SHAPE[D]
    assert (T.n_internal <= 64) == (D == 23)            # int_small's form only on the D = 23 tree
    assert int((T.count[leaf] > 1).sum()) >= 1          # leaves of exact copies (several sentences)
    assert T.depth[leaf].max() >= 5 and T.depth[leaf].min() < T.depth[leaf].max()
    assert (T.nos >= 0).all() and Q.shape == (L.NQ, D) and Q.dtype == np.float32
    # a leaf holds as many sentences as rows went into it; only leaves hold any
    assert np.array_equal(np.diff(T.sid_ptr)[leaf], T.count[leaf].astype(np.int64))
    assert not np.diff(T.sid_ptr)[~leaf].any()
    # the flattened index the oracle's Fast path reads is the same tree
    assert np.array_equal(T.flat.parent, T.parent) and np.array_equal(T.flat.vars, T.var)


def test_oracle_in_units(case):
    """O.log_prob below 4 units against lp64 (every fourth query, all nodes)."""
    D, T, Q, lp32, ref = case
    u = L.units(lp32, ref, L.scale(T.mean, T.var, Q))
    print(f"D={D}: oracle log_prob max units {u[::4].max():.2f} (all 64 queries {u.max():.2f})")
    assert u[::4].max() < 4.0
    assert np.array_equal(L.oracle_lp32_rows(T, Q), lp32)     # the row-wise form: the same bits
    # and the form without the 2 pi term, on its own scale
    up = L.units(L.oracle_lpp32(T, Q[::4]), L.lp64(T.mean, T.var, Q[::4], full=False),
                 L.scale(T.mean, T.var, Q[::4], full=False))
    print(f"D={D}: oracle lp' max units {up.max():.2f}")
    assert up.max() < 5.0      # (measured up to 4.18: S loses its D/2 log 2 pi, the error does not shrink)


@pytest.mark.parametrize("D", [1, 3])
def test_relative_yardstick_fails_the_oracle(D):
    """Why the unit: at D = 1 and 3 the oracle itself misses RTOL = 1e-5 relative to the score."""
    T, Q = L.ragged(D)
    lp32, ref = L.oracle_lp32(T, Q[::4]), L.lp64(T.mean, T.var, Q[::4])
    rel = np.abs(lp32 - ref) / np.abs(ref)
    print(f"D={D}: {(rel > 1e-5).sum()} of {rel.size} pairs over 1e-5 relative, max {rel.max():.2g}")
    assert (rel > 1e-5).sum() >= 1


def test_decisive_shares(case):
    """Conditions, not measurements: enough queries per tree on which the oracle may judge Basic."""
    D, T, Q, lp32, ref = case
    for k, mx in L.BASIC:
        res = [L.decisive(T, Q[qi], k, mx, lp32[qi], ref[qi]) for qi in range(L.NQ)]
        nd, short = sum(r[0] for r in res), sum(r[3] for r in res)
        print(f"D={D} k={k} max_nodes={mx}: decisive {nd} of {L.NQ}, short of k {short}")
        assert nd >= L.DECISIVE_MIN[(k, mx)], (D, k, mx, nd)
        if mx == 12:
            assert short >= 61        # the reference's IndexError case
        # the watched search is the oracle's search
        for qi in (0, 31, 32, 63):
            got, calls, sh = L.oracle_categorize(T, Q[qi], k, mx)
            assert sh == res[qi][3]
            if not sh:
                assert (got, calls) == (res[qi][1], res[qi][2]), (D, k, mx, qi)


def test_decisive_rejects_ties():
    """Two equal children: the gap is 0, the query is not decisive whatever e is."""
    T, Q = L.ragged(23)
    lp32 = L.oracle_lp32(T, Q[:1])[0].copy()
    kids = [i for i in range(len(T.parent)) if T.parent[i] == 0]
    lp32[kids[1]] = lp32[kids[0]] = max(lp32[kids])
    assert not L.decisive(T, Q[0], 5, 100000, lp32, lp32.astype(np.float64))[0]


@pytest.mark.parametrize("D", [3, 17, 23])
def test_spread_variants(D):
    """lp_yardstick.spread: the ifit trees themselves have only isotropic leaf rows (asserted),
    the variants a third anisotropic ones and three sentences in internal nodes; the oracle
    stays below 4 units on them and the decisive shares hold.  Measured, D = 3, 17, 23:
    anisotropic of all leaf-class rows 136/400, 501/1495, 53/152; oracle max units (all 64
    queries) 3.64, 3.51, 3.10; decisive of 64 for the five Basic cases 64 64 62 64 57,
    64 64 56 64 46, 64 62 59 63 52; short of k at max_nodes = 12: 37, 54, 63."""
    def bits_iso(T):
        b = T.var.view(np.int32)
        return (b == b[:, :1]).all(1)
    T0, _ = L.ragged(D)
    assert bits_iso(T0)[T0.is_leaf].all()
    T, Q = L.spread(D)
    rows = T.is_leaf | (np.diff(T.sid_ptr) > 0)
    iso = bits_iso(T)
    print(f"D={D} spread: {rows.sum()} leaf-class rows, {(rows & ~iso).sum()} anisotropic")
    assert (rows & ~iso).sum() >= 16 and (rows & iso).sum() >= 16
    assert (rows & ~T.is_leaf).sum() == 3 and len(T.nos) == len(T0.nos) + 3 and (T.nos >= 0).all()
    assert np.array_equal(T.parent, T0.parent) and np.array_equal(T.mean, T0.mean)
    lp32, ref = L.oracle_lp32_rows(T, Q), L.lp64(T.mean, T.var, Q)
    u = L.units(lp32, ref, L.scale(T.mean, T.var, Q))
    print(f"D={D} spread: oracle log_prob max units {u.max():.2f}")
    assert u[::4].max() < 4.0
    for k, mx in L.BASIC:
        res = [L.decisive(T, Q[qi], k, mx, lp32[qi], ref[qi]) for qi in range(L.NQ)]
        print(f"D={D} spread k={k} max_nodes={mx}: decisive {sum(r[0] for r in res)}, short of k {sum(r[3] for r in res)}")
        assert sum(r[0] for r in res) >= L.DECISIVE_MIN[(k, mx)]
        got, calls, sh = L.oracle_categorize(T, Q[0], k, mx)
        assert sh == res[0][3] and (sh or (got, calls) == (res[0][1], res[0][2]))


def test_rank_scores64_follow_the_oracle(case):
    """The fp64 path-weighted mean against the oracle's fp32 rank scores, in units, with a
    weight list shorter than the depth (weight 1.0 past its end) and a negative entry."""
    D, T, Q, _, _ = case
    for w in (None, [1.0, 2.0, 0.5], [0.5, -1.0, 2.0, 1.0]):
        idx = O.flatten_tree(T.tree.root, len(T.nos), w)
        pa = O.path_arrays(idx)
        got = np.stack([O.rank_scores_vec(x, idx, pa) for x in Q[::8]])
        ref, S = L.rank_scores64(T, Q[::8], w)
        u = L.units(got, ref, S)
        print(f"D={D} weights {w}: oracle rank scores max units {u.max():.2f}")
        assert u.max() < 6.0   # (measured up to 3.8: lp' plus a rounded coefficient and an add per level)
