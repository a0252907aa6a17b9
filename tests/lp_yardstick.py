"""The yardstick of the ragged, odd-dimension tree tests (tests/test_lp_yardstick_cpu.py,
tests/test_gpu_ragged_odd_dim.py): six small trees built by the oracle's own ifit, the Gaussian
log-likelihood of every node in fp64, and the unit the GPU's values are judged in.  Plain
numpy, no GPU.

Why a unit of its own.  The project's score tolerance is RTOL = 1e-5 relative to the score.
On hierarchical trees at small D the log-probability crosses zero, and there the reference's
own fp32 arithmetic (oracle log_prob) misses 1e-5 relative against fp64 (D = 1: 1.6e-4).  The
error of a sum does not shrink with the sum: it follows the terms.  So the unit is

    S(query, node) = sum_d [ 0.5 |log var_d| + 0.5 log 2 pi + 0.5 (|x_d| + |mu_d|)^2 / var_d ]
    units = |value - lp64| / (2^-24 * S)

(the 2 pi term dropped for lp', the form without it).  The (|x| + |mu|)^2 / var term bounds the
rounding of the library's x * (1/sigma) - mu/sigma form as well as the reference's
(x - mu)^2 / var form.  In these units the oracle's error is flat from D = 1 to D = 100
(maximum 2.7 .. 3.5 on the six trees).

Reference semantics: CobwebTorchNode.py:100-104 (log_prob), CobwebWrapper.py:160-169, 283-292
(path-weighted mean of lp'), CobwebTorchTree.py:235-289 (categorize)."""
import functools
import heapq
import random
from dataclasses import dataclass

import numpy as np

from oracle import cobweb_oracle as O

F32 = np.float32
EPS = 2.0 ** -24
LOG_2PI = float(np.log(2.0 * np.pi))

# D -> (D, n, clusters, dup); seed = D + n
TREES = {1: (1, 300, 0, 5), 3: (3, 400, 4, 5), 5: (5, 200, 3, 3), 17: (17, 1500, 12, 10),
         100: (100, 600, 6, 5), 23: (23, 150, 0, 2)}
# (nodes, internal nodes) of those trees: the D = 23 tree takes the internal pass's small form
SHAPE = {1: (552, 255), 3: (672, 275), 5: (320, 122), 17: (2177, 685), 100: (810, 215), 23: (196, 47)}
# Basic's (k, max_nodes) cases and the least number of decisive queries (of 64) each must keep
BASIC = [(1, 100000), (5, 100000), (20, 100000), (5, 12), (70, 100000)]
DECISIVE_MIN = {(1, 100000): 32, (5, 100000): 32, (20, 100000): 32, (5, 12): 32, (70, 100000): 16}
NQ = 64


@dataclass
class Ragged:
    tree: object            # O.OTree
    X: np.ndarray           # [n, D] fp32 corpus
    rng: object             # the numpy generator, continued after the corpus (queries())
    parent: np.ndarray      # BFS arrays
    count: np.ndarray
    mean: np.ndarray
    meanSq: np.ndarray
    sid_ptr: np.ndarray
    sid_list: np.ndarray
    var: np.ndarray         # compute_var (PRIOR_VAR where count == 0), fp32
    nos: np.ndarray         # node of each sentence
    depth: np.ndarray       # depth of each node (root 0)
    nodes: list             # the oracle's nodes in BFS order
    flat: object            # O.FlatIndex

    @property
    def n_internal(self):
        return int((np.bincount(self.parent[1:], minlength=len(self.parent)) > 0).sum())

    @property
    def is_leaf(self):
        return np.bincount(self.parent[1:], minlength=len(self.parent)) == 0


def corpus(D, n, clusters, rng):
    """Clustered: centres N(0, 4I), spread 0.3; unclustered (clusters = 0): N(0, I)."""
    if clusters:
        C = rng.standard_normal((clusters, D)).astype(F32) * 2
        return (C[rng.integers(0, clusters, n)] + 0.3 * rng.standard_normal((n, D))).astype(F32)
    return rng.standard_normal((n, D)).astype(F32)


def bfs_arrays(root, n_sent):
    """(nodes, parent, count, mean, meanSq, sid_ptr, sid_list, var, nos, depth) of a node tree."""
    nodes = O.bfs_nodes(root)
    pos = {id(nd): i for i, nd in enumerate(nodes)}
    parent = np.array([pos[id(nd.parent)] if nd.parent is not None else -1 for nd in nodes], np.int64)
    count = np.array([nd.count for nd in nodes], F32)
    mean = np.stack([nd.mean for nd in nodes]).astype(F32)
    meanSq = np.stack([nd.meanSq for nd in nodes]).astype(F32)
    sid_ptr = np.concatenate([[0], np.cumsum([len(nd.sentence_id) for nd in nodes])]).astype(np.int64)
    sid_list = np.array([s for nd in nodes for s in nd.sentence_id], np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = O.compute_var(meanSq, count[:, None]).astype(F32)
    var[count == 0] = O.PRIOR_VAR
    nos = np.full(n_sent, -1, np.int64)
    for i, nd in enumerate(nodes):
        for s in nd.sentence_id:
            nos[s] = i
    depth = np.zeros(len(nodes), np.int64)
    for i in range(1, len(nodes)):
        depth[i] = depth[parent[i]] + 1
    return nodes, parent, count, mean, meanSq, sid_ptr, sid_list, var, nos, depth


def build_tree(D, n, clusters, dup, seed, weights=None):
    """The corpus and the oracle's ifit tree of it.  For j < dup row n-1-j is an exact copy of
    row 3j: the copies land in the same leaf (count > 1, several sentences)."""
    rng = np.random.default_rng(seed)
    X = corpus(D, n, clusters, rng)
    for j in range(dup):
        X[n - 1 - j] = X[3 * j]
    tree = O.OTree(D, rng=random.Random(seed))
    for i, x in enumerate(X):
        tree.ifit(x).sentence_id.append(i)
    arr = bfs_arrays(tree.root, n)
    return Ragged(tree, X, rng, *arr[1:], arr[0], O.flatten_tree(tree.root, n, weights))


def from_arrays(parent, count, mean, meanSq, sid_ptr, sid_list, n_sent, X=None, rng=None):
    """The same record for a tree exported as BFS arrays (a tree another builder made)."""
    tree = O.OTree(mean.shape[1])
    tree.root = O.tree_from_arrays(parent, count, mean, meanSq, sid_ptr, sid_list)
    arr = bfs_arrays(tree.root, n_sent)
    return Ragged(tree, X, rng, *arr[1:], arr[0], O.flatten_tree(tree.root, n_sent))


def spread_variant(T, seed):
    """The same ragged tree with what ifit cannot give it: leaf-class rows whose variances
    differ by dimension.  (A leaf of exact copies has meanSq = 0 and var = prior_var in every
    dimension, like a count-1 leaf, so all leaf rows of an ifit tree are isotropic; the
    library keeps anisotropic rows in a segment of their own.)  Every third leaf gets a meanSq
    as if its rows were spread 0.05 .. 0.45 per dimension, and three internal nodes (the root, a
    depth-1 and a depth-2 node) hold a further sentence each, ids n .. n + 2."""
    rng = np.random.default_rng(seed)
    meanSq = T.meanSq.copy()
    leaves = np.nonzero(T.is_leaf)[0][::3]
    sd = (0.05 + 0.4 * rng.random((len(leaves), meanSq.shape[1]))).astype(F32)
    meanSq[leaves] = T.count[leaves, None] * sd * sd
    n = len(T.nos)
    inner = [0] + [int(np.nonzero(~T.is_leaf & (T.depth == d))[0][-1]) for d in (1, 2)]
    sents = [list(T.sid_list[T.sid_ptr[i]:T.sid_ptr[i + 1]]) for i in range(len(T.parent))]
    for j, i in enumerate(inner):
        sents[i].append(n + j)
    sid_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    sid_list = np.array([s for ss in sents for s in ss], np.int64)
    return from_arrays(T.parent, T.count, T.mean, meanSq, sid_ptr, sid_list, n + 3, T.X)


@functools.lru_cache(maxsize=None)
def spread(D):
    """(spread_variant of the tree of dimension D, the same 64 queries)."""
    T, Q = ragged(D)
    return spread_variant(T, 1000 + D), Q


def queries(X, rng, nq=NQ):
    """nq/2 near queries (the first rows + 0.05 N(0, I)) and nq/2 far ones (2 N(0, I)), fp32."""
    h = nq // 2
    D = X.shape[1]
    near = X[:h] + 0.05 * rng.standard_normal((h, D))
    far = 2 * rng.standard_normal((nq - h, D))
    return np.concatenate([near, far]).astype(F32)


@functools.lru_cache(maxsize=None)
def ragged(D):
    """(tree record, queries [64, D]) of one of the six trees, built once per process."""
    d, n, clusters, dup = TREES[D]
    T = build_tree(d, n, clusters, dup, seed=d + n)
    return T, queries(T.X, T.rng)


# ---------------------------------------------------------------------------------------------
# node log-probabilities
# ---------------------------------------------------------------------------------------------
def lp64(mean, var, Xq, full=True):
    """[nq, n_nodes] fp64: -(0.5 log var + 0.5 log 2 pi + 0.5 (x - mu)^2 / var).sum(-1) on the
    fp32 inputs cast to fp64; full=False: without the 2 pi term (lp')."""
    m, v, x = (np.asarray(a, np.float64) for a in (mean, var, Xq))
    out = np.empty((x.shape[0], m.shape[0]))
    ld = 0.5 * np.log(v).sum(1) + (0.5 * LOG_2PI * m.shape[1] if full else 0.0)
    for qi in range(x.shape[0]):
        out[qi] = -(ld + (0.5 * (x[qi] - m) ** 2 / v).sum(1))
    return out


def scale(mean, var, Xq, full=True):
    """[nq, n_nodes] fp64: the condition-scaled unit's S (module docstring)."""
    m, v, x = (np.asarray(a, np.float64) for a in (mean, var, Xq))
    out = np.empty((x.shape[0], m.shape[0]))
    base = 0.5 * np.abs(np.log(v)).sum(1) + (0.5 * LOG_2PI * m.shape[1] if full else 0.0)
    for qi in range(x.shape[0]):
        out[qi] = base + (0.5 * (np.abs(x[qi]) + np.abs(m)) ** 2 / v).sum(1)
    return out


def units(value, ref, S):
    """|value - ref| / (2^-24 S), elementwise; the finiteness patterns must be equal."""
    value = np.asarray(value, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(value), fin), "finiteness patterns differ"
    out = np.zeros(ref.shape)
    pos = fin & (S > 0)
    out[pos] = np.abs(value[pos] - ref[pos]) / (EPS * S[pos])
    zero = fin & ~pos                       # a sum whose every term is zero (all-zero weights): exact
    out[zero] = np.where(value[zero] == ref[zero], 0.0, np.inf)
    return out


def oracle_lp32(T, Xq):
    """[nq, n_nodes] fp32: O.log_prob of every node (the reference's own arithmetic)."""
    return np.array([[O.log_prob(nd, x) for nd in T.nodes] for x in np.asarray(Xq, F32)], F32)


def oracle_lp32_rows(T, Xq):
    """oracle_lp32 a query at a time over the node arrays: O.log_prob's expression on [n_nodes, D]
    with the sum along D (numpy's pairwise fp32 reduction of each row, as in the 1-D call) --
    the same bits (pinned by tests/test_lp_yardstick_cpu.py), without a Python call per node."""
    h = F32(0.5)
    return np.stack([-(h * np.log(T.var) + h * O.LOG_2PI_F32 + h * np.square(x - T.mean) / T.var).sum(axis=1)
                     for x in np.asarray(Xq, F32)]).astype(F32)


def oracle_lpp32(T, Xq):
    """[nq, n_nodes] fp32: O.node_logprob_prime (the reference's lp', no 2 pi term)."""
    return np.stack([O.node_logprob_prime(x, T.mean, T.var) for x in np.asarray(Xq, F32)])


# ---------------------------------------------------------------------------------------------
# path sums: Fast's rank scores and the internal prefixes
# ---------------------------------------------------------------------------------------------
def level_w(depth, weights):
    w = list(O.DEFAULT_LEVEL_WEIGHTS) if weights is None else list(weights)
    return np.array([w[d] if d < len(w) else 1.0 for d in depth], np.float64)


def path_prefix(parent, depth, vals, weights=None, absolute=False):
    """[nq, n_nodes] fp64: sum over node i's root-to-i path of w[depth] * vals (weight 1.0 past
    the list); absolute=True: with |w| (the scale of that sum when vals is S)."""
    w = level_w(depth, weights)
    if absolute:
        w = np.abs(w)
    P = np.empty_like(vals, dtype=np.float64)
    P[:, 0] = w[0] * vals[:, 0]
    for i in range(1, vals.shape[1]):
        P[:, i] = P[:, parent[i]] + w[i] * vals[:, i]
    return P


def rank_scores64(T, Xq, weights=None):
    """([nq, n_sent] fp64 scores, their scale): the path-weighted mean of lp' -- weight
    w[depth] / len(path), 1.0 past the end of the list -- and the same sum of S with |w|.
    A sentence outside the tree scores -inf."""
    lpp = lp64(T.mean, T.var, Xq, full=False)
    S = scale(T.mean, T.var, Xq, full=False)
    L = (T.depth + 1).astype(np.float64)
    sc = path_prefix(T.parent, T.depth, lpp, weights) / L
    ss = path_prefix(T.parent, T.depth, S, weights, absolute=True) / L
    inside = T.nos >= 0
    out = np.full((len(Xq), len(T.nos)), -np.inf)
    outS = np.ones((len(Xq), len(T.nos)))
    out[:, inside] = sc[:, T.nos[inside]]
    outS[:, inside] = ss[:, T.nos[inside]]
    return out, outS


def rank_order64(scores, nos):
    """The fp64 ranking of one query: higher score, then lower node, then lower sentence id."""
    return np.lexsort((np.arange(len(nos)), nos, -scores))


# ---------------------------------------------------------------------------------------------
# Basic: may the oracle judge this query?
# ---------------------------------------------------------------------------------------------
def children_lists(parent):
    ch = [[] for _ in range(len(parent))]
    for i in range(1, len(parent)):
        ch[parent[i]].append(i)
    return ch


def decisive(T, x, k, max_nodes, lp32=None, lp64_row=None):
    """The reference heap search (OTree.categorize's loop: CobwebTorchTree.py:235-289, ties by
    BFS index) on the oracle's fp32 keys, watched: at each pop the gap between the popped key
    and the best key left in the heap; e = the largest |lp32 - lp64| over the nodes the search
    scored.  The query is decisive when the smallest gap exceeds 16 e.

    The margin: a kernel within 4x the oracle's own error has keys that differ from the
    oracle's by less than 5 e per node, so no pop can flip unless a gap is under 10 e; 16
    leaves room.  An exact tie (gap 0) is never decisive.

    lp32 / lp64_row [n_nodes]: the keys if already computed (else computed here).
    Returns (decisive, retrieved BFS ids, log_prob calls, short: fewer than k retrieved --
    the reference's IndexError)."""
    x = np.asarray(x, F32)
    if lp32 is None:
        lp32 = oracle_lp32(T, x[None])[0]
    if lp64_row is None:
        lp64_row = lp64(T.mean, T.var, x[None])[0]
    ch = getattr(T, "_children", None)
    if ch is None:
        ch = T._children = children_lists(T.parent)
    has_sent = np.diff(T.sid_ptr) > 0
    scored = [0]
    heap = [(-lp32[0], 0.0, 0)]     # the reference's key: (-lp, lp of the parent, tie-break)
    calls, visited, retrieved, min_gap = 1, 0, [], np.inf
    while heap:
        neg, _, cur = heapq.heappop(heap)
        if heap:
            min_gap = min(min_gap, float(heap[0][0]) - float(neg))
        visited += 1
        if visited >= max_nodes:
            break
        if has_sent[cur]:
            retrieved.append(cur)
        if len(retrieved) == k:
            break
        for c in ch[cur]:
            calls += 1
            scored.append(c)
            heapq.heappush(heap, (-lp32[c], -neg, c))
    e = float(np.max(np.abs(lp32[scored].astype(np.float64) - lp64_row[scored])))
    return bool(min_gap > 0 and min_gap > 16 * e), retrieved, calls, len(retrieved) < k


def oracle_categorize(T, x, k, max_nodes):
    """OTree.categorize with ties by BFS index: (BFS ids, calls, short)."""
    order = getattr(T, "_order", None)
    if order is None:
        order = T._order = {id(nd): i for i, nd in enumerate(T.nodes)}
    try:
        leaves, calls = T.tree.categorize(x, k, max_nodes, order=order)
        return [order[id(nd)] for nd in leaves], calls, False
    except IndexError:
        return None, None, True
