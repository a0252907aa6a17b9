"""The device-resident tree (resident.py, cwq_fitindex.hip): the flatten kernels against the
numpy yardstick (tests/resident_yardstick.py, pinned to the reference's trees on the CPU) and
the golden BFS arrays; the reference's own trees rebuilt through CobwebWrapper(resident=True);
resident == default on interleaved add / query sequences; in-place growth; the wrapper's
surface.  Every comparison is exact: the resident path reorders no arithmetic."""
import json
import random

import numpy as np
import pytest

from conftest import load_golden
from resident_yardstick import bfs_flatten, scramble

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _flat_np(rt):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rt.flatten().items()}


def _check_flat(f, y):
    """Device flatten == yardstick, every array, bit for bit."""
    for k in ("parent", "node_of_sentence", "an_nodes", "slot_of_node"):
        np.testing.assert_array_equal(f[k], y[k], err_msg=k)
    for k in ("mean", "count", "var_row", "an_var"):
        np.testing.assert_array_equal(_bits(f[k]), _bits(y[k]), err_msg=k)
    assert f["depth"] == y["depth"]


# ---------------------------------------------------------------- 1. flatten alone
@pytest.mark.parametrize("name,seed", [("g1_hier_d32", 1), ("g5_hier_d384", 5), ("g9_interleaved_d16", 9)])
def test_flatten_scrambled_golden(pkg, name, seed):
    """cwq_fit_load of a reference tree under a scrambled slot numbering (removed and unused
    slots mixed in, the root not at slot 0), then cwq_fit_flatten: the golden BFS arrays, and
    variances with the bits of numpy float32 meanSq / count + prior_var."""
    _gpu()
    g = load_golden(name)
    s = scramble(g, seed)
    y = bfs_flatten(s["parent"], s["child_ptr"], s["child_idx"], s["root"], s["count"], s["mean"], s["meanSq"],
                    g["prior_var"], s["slot_of_sentence"], s["slot_sids"])
    rt = pkg.resident.ResidentTree.from_slots(s["parent"], s["child_ptr"], s["child_idx"], s["count"], s["mean"],
                                              s["meanSq"], s["root"], s["slot_sids"], s["n_sent"],
                                              prior_var=g["prior_var"])
    try:
        f = _flat_np(rt)
        _check_flat(f, y)
        np.testing.assert_array_equal(f["parent"], g["parent"])
        np.testing.assert_array_equal(f["mean"], g["mean"])
        np.testing.assert_array_equal(f["count"], g["count"])
        want = g["meanSq"] / g["count"][:, None] + np.float32(g["prior_var"])
        full = np.repeat(f["var_row"][:, None], want.shape[1], 1)
        full[f["an_nodes"]] = f["an_var"]
        np.testing.assert_array_equal(_bits(full), _bits(want))
        sids = [v for sl in f["slot_of_node"] for v in rt.leaf_sids.get(int(sl), [])]
        np.testing.assert_array_equal(sids, g["sid_list"])
        # a sentence that is in no slot, one in a removed slot, one past the pool: -1
        rt._sos[3] = -1
        rt._sos[4] = int(np.nonzero(s["parent"] == -2)[0][0])
        rt._sos[6] = 10 ** 6
        nos = rt.flatten(stats=False)["node_of_sentence"].cpu().numpy()
        assert nos[3] == -1 and nos[4] == -1 and nos[6] == -1
        keep = np.setdiff1d(np.arange(len(nos)), [3, 4, 6])
        np.testing.assert_array_equal(nos[keep], y["node_of_sentence"][keep])
        assert rt.stats["removed_slots"] == int((s["parent"] == -2).sum())
    finally:
        rt.close()


@pytest.mark.parametrize("D", [6, 8])
def test_flatten_wide_levels(pkg, D):
    """Levels of 3,000 and 5,000 nodes (several 1,024-element scan tiles, tile sums that carry
    across tiles), children of one node next to nodes without any, leaves with one value
    repeated next to leaves with a variance row, an empty leaf; D = 6: rows that cannot be
    moved as float4."""
    _gpu()
    rng = np.random.default_rng(D)
    n1, per = 3000, 5
    inner = np.arange(1, n1 + 1)[::3]                       # every third depth-1 node has children
    parent = np.concatenate([[-1], np.zeros(n1, np.int64), np.repeat(inner, per)])
    Nn = len(parent)
    nchild = np.bincount(parent[1:], minlength=Nn)
    count = np.where(nchild > 0, 7.0, rng.integers(1, 3, Nn)).astype(np.float32)
    count[5] = 0                                            # an empty leaf: var = prior_var
    mean = rng.standard_normal((Nn, D)).astype(np.float32)
    m2 = rng.random((Nn, D)).astype(np.float32)
    m2[(count == 1) & (nchild == 0)] = 0                    # count-1 leaves: one value repeated
    m2[7] = np.float32(0.375)                               # and a row of one repeated non-zero value
    leaves = np.nonzero(nchild == 0)[0]
    sid_ptr = np.zeros(Nn + 1, np.int64)
    sid_ptr[leaves + 1] = 1
    sid_ptr = np.cumsum(sid_ptr)
    g = {"parent": parent, "count": count, "mean": mean, "meanSq": m2, "sid_ptr": sid_ptr,
         "sid_list": rng.permutation(len(leaves)), "n_sent": len(leaves)}
    s = scramble(g, 100 + D, extra=501)
    pv = np.float32(0.05)
    y = bfs_flatten(s["parent"], s["child_ptr"], s["child_idx"], s["root"], s["count"], s["mean"], s["meanSq"], pv,
                    s["slot_of_sentence"], s["slot_sids"])
    np.testing.assert_array_equal(y["parent"], parent)
    rt = pkg.resident.ResidentTree.from_slots(s["parent"], s["child_ptr"], s["child_idx"], s["count"], s["mean"],
                                              s["meanSq"], s["root"], s["slot_sids"], s["n_sent"], prior_var=pv)
    try:
        f = _flat_np(rt)
        _check_flat(f, y)
        assert f["depth"] == 2 and 5 not in f["an_nodes"] and 7 not in f["an_nodes"]
        assert 0 < len(f["an_nodes"]) < Nn and f["var_row"][5] == pv
        # growth re-packs every child list: the same flatten afterwards
        assert rt._L.cwq_fit_grow(rt._h, 3 * len(s["parent"]), None) == 0
        _check_flat(_flat_np(rt), y)
        assert rt.stats["cap_nodes"] == 3 * len(s["parent"])
    finally:
        rt.close()


# ---------------------------------------------------------------- 2. reference trees
def _check_resident_against_golden(w, g):
    rt = w.resident_tree
    f = _flat_np(rt)
    np.testing.assert_array_equal(f["parent"], g["parent"])
    np.testing.assert_array_equal(f["count"], g["count"])
    np.testing.assert_array_equal(f["mean"], g["mean"])
    want = g["meanSq"] / g["count"][:, None] + np.float32(g["prior_var"])
    full = np.repeat(f["var_row"][:, None], want.shape[1], 1)
    full[f["an_nodes"]] = f["an_var"]
    np.testing.assert_array_equal(_bits(full), _bits(want))
    sids = [v for sl in f["slot_of_node"] for v in rt.leaf_sids.get(int(sl), [])]
    np.testing.assert_array_equal(sids, g["sid_list"])
    owner = np.repeat(np.arange(len(g["count"])), np.diff(g["sid_ptr"]))
    nos = np.full(int(g["n_sent"]), -1, np.int64)
    nos[g["sid_list"]] = owner
    np.testing.assert_array_equal(f["node_of_sentence"], nos)


@pytest.mark.parametrize("name", ["g1_hier_d32", "g5_hier_d384"])
def test_resident_reproduces_reference_tree(pkg, name):
    _gpu()
    g = load_golden(name)
    random.seed(0)   # gen_golden.py seeds the reference the same way
    w = pkg.CobwebWrapper(corpus=[f"s{i}" for i in range(len(g["X"]))], corpus_embeddings=g["X"], resident=True)
    assert type(w).__name__ == "ResidentCobwebWrapper" and isinstance(w, pkg.CobwebWrapper)
    _check_resident_against_golden(w, g)
    k = int(g["k"])
    for qi in range(4):
        got = w.cobweb_predict_fast(g["Xq"][qi], k, return_ids=True)
        rs = g["rank_scores"][qi]
        for a, b in zip(got, g["fast_ids"][qi]):
            if a != b:
                assert abs(rs[a] - rs[b]) <= 1e-5 * abs(rs[b])
        basic = w.cobweb_predict(g["Xq"][qi], k, return_ids=True)
        exp = [s for nid in g["cat_nodes"][qi] for s in
               sorted(g["sid_list"][g["sid_ptr"][nid]:g["sid_ptr"][nid + 1]])]
        assert basic == exp
    with pytest.raises(IndexError):
        w.cobweb_predict(g["Xq"][0], int(g["n_leaf_nodes"]) + 1)


def test_resident_interleaved_matches_reference(pkg):
    """Golden G9 from the real reference (39 leaves hold several sentences): add -> six Basic
    queries -> IndexError at max_init_search = 3 -> add -> queries -> add, on one random()
    stream.  The per-slot sentence lists carry the reference's in-place shuffles across the
    index rebuilds."""
    _gpu()
    g = load_golden("g9_interleaved_d16")

    def ragged(ptr, ids):
        return [list(ids[ptr[i]:ptr[i + 1]]) for i in range(len(ptr) - 1)]

    random.seed(int(g["seed"]))
    w = pkg.CobwebWrapper(corpus=[f"a{i}" for i in range(len(g["XA"]))], corpus_embeddings=g["XA"], resident=True)
    assert [w.cobweb_predict(q, 4, return_ids=True) for q in g["Q1"]] == ragged(g["out1_ptr"], g["out1_ids"])
    w.max_init_search = 3
    with pytest.raises(IndexError):
        w.cobweb_predict(g["Q1"][0], 4, return_ids=True)
    w.max_init_search = 100000
    w.add_sentences([f"b{i}" for i in range(len(g["XB"]))], g["XB"])
    assert [w.cobweb_predict(q, 5, return_ids=True) for q in g["Q2"]] == ragged(g["out2_ptr"], g["out2_ids"])
    w.add_sentences([f"c{i}" for i in range(len(g["XC"]))], g["XC"])
    assert random.random() == float(g["random_after"])
    _check_resident_against_golden(w, g)
    assert w._host is None, "nothing above reads the host tree"


# ---------------------------------------------------------------- 3. resident == default
def _tree_arrays(tree):
    a = tree.to_arrays()
    return a["parent"], a["count"], a["mean"], a["meanSq"], a["sid_ptr"], a["sid_list"]


def _data(D, n, clusters):
    rng = np.random.default_rng(D + n)      # the generator of test_device_fit_equals_host_fit
    if clusters:
        C = rng.standard_normal((clusters, D)).astype(np.float32) * 2.0
        X = (C[rng.integers(0, clusters, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    else:
        X = rng.standard_normal((n, D)).astype(np.float32)
    if n >= 5:
        X[n // 3] = X[n // 5]               # an exact match: a leaf that holds two sentences
    return X, rng.standard_normal((6, D)).astype(np.float32)


def _run_interleaved(pkg, X, Q, resident, cuts):
    """Three add_sentences calls with Fast and Basic queries between them; everything a caller
    can observe, as host arrays."""
    random.seed(7)
    n = len(X)
    Qd = torch.from_numpy(Q).cuda()
    w, seen = None, []
    for a, b in zip([0] + cuts, cuts + [n]):
        if a == b:
            continue
        names = [f"s{i}" for i in range(a, b)]
        if w is None:
            w = pkg.CobwebWrapper(corpus=names, corpus_embeddings=X[a:b], resident=resident)
        else:
            w.add_sentences(names, X[a:b])
        w.build_prediction_index()
        k = min(5, b)
        ids, scores = w.cobweb_predict_batch(Qd, k)
        rs = w.cobweb_rank_scores_batch(Qd)
        nodes, found, calls = w.cobweb_categorize_batch(Qd, k)
        step = {"info": dict(w._index.info), "ids": ids.cpu(), "scores": scores.cpu(), "rs": rs.cpu(),
                "nodes": nodes.cpu(), "found": found.cpu(), "calls": calls.cpu(),
                "fast": w.cobweb_predict_fast(Q[0], k, return_ids=True)}
        try:
            step["basic"] = [w.cobweb_predict(q, min(3, b), return_ids=True) for q in Q[:3]]
        except IndexError:
            step["basic"] = "IndexError"
        seen.append(step)
    return w, seen, random.random()


@pytest.mark.parametrize("D,n,clusters", [(48, 1500, 12), (768, 1000, 0), (5, 600, 4), (1024, 64, 0), (16, 1, 0),
                                          (16, 2, 0)])
def test_resident_equals_default_interleaved(pkg, D, n, clusters):
    """(48, 1500, 12): 2,074 nodes, depth 7, 534 slots removed by splits, one level 1,039
    nodes wide -- more than one 1,024-element scan tile (measured on MI355X with the Basic
    queries between the adds; the CPU oracle's tree from this data alone, OTree with
    random.Random(7), has 2,074 nodes, 537 splits, 586 merges and a level of 1,041);
    (768, 1000, 0): a root of > 900 children, a child list longer than a
    workgroup; (5, 600, 4): rows that cannot be vectorised; (1024, 64, 0): the largest
    dimension; 1 and 2 rows: the root alone and the first fringe split."""
    _gpu()
    X, Q = _data(D, n, clusters)
    cuts = [n // 2, n // 2 + n // 4] if n >= 4 else [1, 1]
    wd, seen_d, rd = _run_interleaved(pkg, X, Q, False, cuts)
    wr, seen_r, rr = _run_interleaved(pkg, X, Q, True, cuts)
    assert len(seen_d) == len(seen_r) >= 1
    for a, b in zip(seen_d, seen_r):
        assert a["info"] == b["info"]
        for key in ("ids", "scores", "rs", "nodes", "found", "calls"):
            assert torch.equal(a[key], b[key]), key
        assert a["fast"] == b["fast"] and a["basic"] == b["basic"]
    assert rd == rr
    st = wr.resident_tree.stats
    assert st["rows"] == n
    if clusters:
        assert st["removed_slots"] > 0      # splits happened: the flatten skipped their slots
    if D == 768:
        assert seen_r[-1]["info"]["n_nodes"] > 900 and seen_r[-1]["info"]["max_depth"] <= 3
    par = wr.resident_tree.flatten(stats=False)["parent"].cpu().numpy()
    depth = np.zeros(len(par), np.int64)
    for i in range(1, len(par)):
        depth[i] = depth[par[i]] + 1
    widest = int(np.bincount(depth).max())
    print(f"resident tree ({D}, {n}, {clusters}): {len(par)} nodes, depth {depth.max()}, widest level {widest}, "
          f"{st['removed_slots']} removed slots, {st['grows']} grows")
    if (D, n) == (48, 1500):
        assert widest > 1024                # wider than one scan tile
    if (D, n) == (768, 1000):
        assert int(np.bincount(par[1:]).max()) > 900   # one child list longer than a workgroup
    assert wr._host is None                 # no query above needed the host tree
    for x, y in zip(_tree_arrays(wd.tree), _tree_arrays(wr.resident_tree.to_tree())):
        np.testing.assert_array_equal(x, y)
    assert json.loads(wd.dump_json()) == json.loads(wr.dump_json())
    assert sorted(wr.sentence_to_node) == list(range(n))


# ---------------------------------------------------------------- 4. growth
def _growth_data():
    rng = np.random.default_rng(77)         # test_device_fit_small_pool_reloads_and_fallback's data
    n, D, ncl = 600, 64, 8
    C = rng.standard_normal((ncl, D)).astype(np.float32) * 2.0
    X = (C[rng.integers(0, ncl, n)] + 0.4 * rng.standard_normal((n, D))).astype(np.float32)
    X[n // 2] = X[n // 7]
    return X


def test_pool_grows_in_place(pkg):
    """cap_nodes just above the first batch's need: the later batches stop for room and the
    pool doubles in place at least three times.  Tree, sentence placement and random()
    position equal the default path's, and the first batch's sentences still resolve to
    their nodes: slot numbers survived every grow."""
    _gpu()
    X = _growth_data()
    n, n0 = len(X), 40
    random.seed(11)
    wd = pkg.CobwebWrapper(corpus=[f"s{i}" for i in range(n0)], corpus_embeddings=X[:n0])
    wd.add_sentences([f"s{i}" for i in range(n0, n)], X[n0:])
    rd = random.random()
    want = _tree_arrays(wd.tree)

    rt = pkg.resident.ResidentTree(X.shape[1], cap_nodes=4 * n0 + 64)
    random.seed(11)
    assert rt.add(X[:n0]) == list(range(n0))
    slots0 = rt._sos[:n0].cpu().numpy().copy()
    assert rt.add(X[n0:300]) == list(range(n0, 300))
    assert rt.add(X[300:]) == list(range(300, n))
    assert random.random() == rd
    st = rt.stats
    assert st["grows"] >= 3 and st["rows"] == n and st["removed_slots"] > 0
    assert st["slots_in_use"] - st["removed_slots"] == len(want[0])
    np.testing.assert_array_equal(rt._sos[:n0].cpu().numpy(), slots0)
    for x, y in zip(want, _tree_arrays(rt.to_tree())):
        np.testing.assert_array_equal(x, y)
    f = _flat_np(rt)
    owner = np.repeat(np.arange(len(want[1])), np.diff(want[4]))
    nos = np.full(n, -1, np.int64)
    nos[want[5]] = owner
    np.testing.assert_array_equal(f["node_of_sentence"], nos)
    np.testing.assert_array_equal(f["slot_of_node"][f["node_of_sentence"][:n0]], slots0)
    np.testing.assert_array_equal(f["mean"], want[2])
    rt.close()


def test_failed_grow_leaves_the_tree_usable(pkg, monkeypatch):
    """cwq_fit_grow failing (out of memory) surfaces as an exception; the rows before the stop
    are in the tree with their ids, and the same object takes the rest afterwards."""
    _gpu()
    X = _growth_data()[:300]
    n, n0 = len(X), 40
    random.seed(11)
    wd = pkg.CobwebWrapper(corpus=[f"s{i}" for i in range(n)], corpus_embeddings=X)
    rd = random.random()
    want = _tree_arrays(wd.tree)

    random.seed(11)
    w = pkg.CobwebWrapper(resident=True)
    w._rt = pkg.resident.ResidentTree(X.shape[1], cap_nodes=4 * n0 + 64)
    w.add_sentences([f"s{i}" for i in range(n0)], X[:n0])
    L = w.resident_tree._L
    real = L.cwq_fit_grow
    calls = {"n": 0}

    def grow(*a):
        calls["n"] += 1
        return -3 if calls["n"] == 2 else real(*a)
    monkeypatch.setattr(L, "cwq_fit_grow", grow)
    with pytest.raises(RuntimeError, match="cwq_fit_grow failed"):
        w.add_sentences([f"s{i}" for i in range(n0, n)], X[n0:])
    done = len(w)
    assert n0 < done < n and w.resident_tree.n_sent == done and calls["n"] == 2
    assert len(w.cobweb_predict_fast(X[done - 1], 3, return_ids=True)) == 3      # the tree answers
    w.add_sentences([f"s{i}" for i in range(done, n)], X[done:])
    assert len(w) == n and random.random() == rd
    for x, y in zip(want, _tree_arrays(w.tree)):
        np.testing.assert_array_equal(x, y)


def test_grow_argument_errors(pkg):
    _gpu()
    rt = pkg.resident.ResidentTree(8, cap_nodes=200)
    L = rt._L
    assert L.cwq_fit_grow(rt._h, 200, None) == pkg._lib.CWQ_ERR_ARG
    assert L.cwq_fit_grow(rt._h, 100, None) == pkg._lib.CWQ_ERR_ARG
    assert b"exceed" in L.cwq_fit_last_error()
    assert rt.add(np.ones((3, 8), np.float32)) == [0, 1, 2] and rt.stats["cap_nodes"] == 200
    rt.close()
    with pytest.raises(RuntimeError, match="closed"):
        rt.add(np.ones((1, 8), np.float32))


# ---------------------------------------------------------------- 5. wrapper surface
def test_resident_wrapper_surface(pkg, tmp_path):
    _gpu()
    g = load_golden("g1_hier_d32")
    X, Xq = g["X"], torch.from_numpy(g["Xq"][:8]).cuda()
    names = [f"s{i}" for i in range(len(X))]
    out = {}
    for resident in (False, True):
        random.seed(3)
        w = pkg.CobwebWrapper(corpus=names[:250], corpus_embeddings=X[:250], resident=resident)
        w.add_sentences(names[250:], X[250:])
        o = out[resident] = {"w": w}
        o["json"] = json.loads(w.dump_json())
        path = str(tmp_path / f"tree_{int(resident)}.npz")
        w.save_binary(path)
        o["path"] = path
        o["stats"] = [tuple(t.cpu().numpy() for t in w.get_node_path_stats(s)) for s in (0, 17, 299)]
        o["none"] = w.get_node_path_stats(10 ** 6)
        w.set_weight_schedule("exponential", base=0.5)
        o["weights"] = list(w.get_level_weights())
        o["rs_sched"] = w.cobweb_rank_scores_batch(Xq).cpu()
        w.add_sentences(["fresh"], X[7:8] + np.float32(0.25))
        q = (Xq[:3] + 0.1).clone().requires_grad_(True)
        loss = w.cobweb_ranking_loss(q, torch.tensor([len(w) - 1, 5, 250]), temperature=0.7)
        loss.backward()
        o["loss"], o["grad"] = loss.detach().cpu(), q.grad.cpu()
        o["info"] = w.get_prediction_index_info()
    d, r = out[False], out[True]
    assert d["json"] == r["json"]
    for (am, av), (bm, bv) in zip(d["stats"], r["stats"]):
        np.testing.assert_array_equal(am, bm)
        np.testing.assert_array_equal(av, bv)
    assert d["none"] == r["none"] == (None, None)
    assert d["weights"] == r["weights"] and torch.equal(d["rs_sched"], r["rs_sched"])
    assert torch.equal(d["loss"], r["loss"]) and torch.equal(d["grad"], r["grad"])
    assert d["info"]["n_nodes"] == r["info"]["n_nodes"] == r["info"]["total_nodes"]
    with np.load(d["path"]) as za, np.load(r["path"]) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            np.testing.assert_array_equal(za[k], zb[k])
    # the loaders with resident=True: the same answers as the default loader's wrapper, and
    # after one more add
    Q = torch.from_numpy(g["Xq"][:6]).cuda()
    more = X[:20] * np.float32(1.01)
    js = r["w"].dump_json()
    for load in (lambda res: pkg.CobwebWrapper.load_json(js, resident=res),
                 lambda res: pkg.CobwebWrapper.load_binary(r["path"], resident=res),
                 lambda res: pkg.CobwebWrapper.from_tree(pkg.CobwebTree.load_binary(d["path"]), names,
                                                          resident=res)):
        got = {}
        for res in (False, True):
            w2 = load(res)
            assert (type(w2).__name__ == "ResidentCobwebWrapper") == res and len(w2) in (300, 301)
            random.seed(5)
            a = w2.cobweb_predict_batch(Q, 10)
            b1 = w2.cobweb_predict(g["Xq"][0], 4, return_ids=True)
            w2.add_sentences([f"m{i}" for i in range(20)], more)
            b = w2.cobweb_predict_batch(Q, 10)
            got[res] = (a[0].cpu(), a[1].cpu(), b[0].cpu(), b[1].cpu(), b1, random.random(), _tree_arrays(w2.tree))
        for x, y in zip(got[False][:4], got[True][:4]):
            assert torch.equal(x, y)
        assert got[False][4:6] == got[True][4:6]
        for x, y in zip(got[False][6], got[True][6]):
            np.testing.assert_array_equal(x, y)
