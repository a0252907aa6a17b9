"""The certified filter bounds on inputs where Cauchy-Schwarz is tight (tests/bounds_model.py;
the fixtures' conditions are proven on the CPU by tests/test_bounds_model_cpu.py): operands
whose rounding residuals have one sign in every dimension, with the rows' true keys placed so
that a bound a few percent too narrow drops a true top-k row.  Every case runs the filter and
the exact scan: ids and scores bit-identical, no query re-run by the exact scan (a fallback
would hide a broken bound), the expected path, ids equal to the fp64 order and scores within
RTOL of fp64 -- batch bf16 and int8 launches, tile placement, the per-call stream filter,
Basic through the filter, group-centred rows, and the internal-node bounds."""
import numpy as np
import pytest

import bounds_model as B

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLOTS = (0, 15, 16, 255, 256, 298, 299)   # 16-query blocks, 256-query tiles; two groups: s and s + 1


@pytest.fixture(scope="module")
def gpu(pkg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg


_cache = {}


def indexed(pkg, kind, operand, D, kmax=64, **kw):
    """(fixture, index, fp64 keys of the engineered queries), built once per module."""
    key = (kind, operand, D, kmax) + tuple(sorted(kw.items()))
    if key not in _cache:
        fx = B.fixture(kind, operand, D, kmax, **kw)
        mean, var, parent, nos = fx.tree()
        ix = pkg.index.CobwebIndex(torch.from_numpy(mean), torch.from_numpy(var), parent, nos, device="cuda:0")
        assert ix.info["isotropic_rows"] == len(fx.rows) >= 16384
        _cache[key] = (fx, ix, B.true_keys(fx.xq, fx.rows, ix.level_weights))
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_indices():
    yield
    for _, ix, _ in _cache.values():
        ix.close()
    _cache.clear()


def exact(ix, Q, k):
    ix.set_filter(0)
    ids, s = ix.score_topk(Q, k)
    assert not ix.last_stats()["filter_used"]
    ix.set_filter(-1)
    return ids.cpu(), s.cpu()


def check(ix, fx, key64, Q, where, k, path, env, mp, i8_launches=None, int8_pass=None):
    """One automatic-mode call under `env` against the exact scan and the fp64 order."""
    Qd = torch.from_numpy(Q).to("cuda:0")
    ids0, s0 = exact(ix, Qd, k)
    for name, v in env.items():
        mp.setenv(name, v)
    ids1, s1 = ix.score_topk(Qd, k)
    st = ix.last_stats()
    for name in env:
        mp.delenv(name)
    print(fx.kind, fx.operand, k, env, st)
    assert st["filter_used"] and st["path"] == path and st["filter_queries"] == len(Q), st
    assert st["fallback_queries"] == 0, st
    if i8_launches is not None:
        assert (st["fg_i8_launches"] > 0) == i8_launches, st
    if int8_pass is not None:
        assert st["int8_pass"] == int8_pass, st
    ids1, s1 = ids1.cpu(), s1.cpu()
    assert torch.equal(ids0, ids1) and torch.equal(s0, s1)
    assert where
    for slot, g in where:
        top = B.fp64_topk(key64[g], k)
        assert ids1[slot].tolist() == top.tolist(), (slot, g)
        got = s1[slot].numpy().astype(np.float64)
        assert (np.abs(got - key64[g][top]) <= B.RTOL * np.abs(key64[g][top])).all(), (slot, g)
    return st


def with_panel(ix, Q, mp):
    """The int8 panel on an index below the size that gets one by itself: one call with
    CWQ_FG_I8 past the last phase builds it and runs bf16 only (tests/test_gpu_fg_i8.py)."""
    mp.setenv("CWQ_FG_I8", "99")
    ix.set_filter(1)
    ix.score_topk(torch.from_numpy(Q[:1]).to("cuda:0").repeat(65, 1), 1)
    st = ix.last_stats()
    ix.set_filter(-1)
    mp.delenv("CWQ_FG_I8")
    assert st["fg_i8_launches"] == 0 and ix.filter_info()["int8_panel"], st


BATCH = [(kind, kmax, k, 64) for kind in ("upper", "lower") for k in (1, 10, 64) for kmax in (64,)] + \
        [(kind, k, k, 64) for kind in ("qside", "both") for k in (1, 10, 64)] + \
        [("upper", 64, 10, 200), ("lower", 64, 64, 200), ("qside", 10, 10, 200), ("upper", 64, 64, 768)]


@pytest.mark.parametrize("kind,kmax,k,D", BATCH)
def test_batch_bf16(gpu, kind, kmax, k, D, monkeypatch):
    """300 queries, bf16 launches only; the engineered query in several 16-query blocks and
    both 256-query tiles, ordinary queries around it."""
    fx, ix, key64 = indexed(gpu, kind, "bf16", D, kmax)
    Q, where = fx.queries(300, SLOTS)
    check(ix, fx, key64, Q, where, k, "fgemm", {"CWQ_FG_I8": "-1"}, monkeypatch, i8_launches=False)


@pytest.mark.parametrize("env", [{}, {"CWQ_FG_NO_ALLUNI": "1"}, {"CWQ_FG_CUTS": "8,16,32,64"}],
                         ids=["default", "no_alluni", "cuts"])
@pytest.mark.parametrize("background", ["gauss", "exact"])
@pytest.mark.parametrize("N", [16640, 16500])
@pytest.mark.parametrize("kind", ["upper", "lower", "qside"])
def test_tile_placement(gpu, kind, N, background, env, monkeypatch):
    """Engineered rows at filter rows 0, 255, 256 and at the end of the last row tile (N =
    16,500: the partial one; bounds_model.positions).  bf16-exact background rows leave the
    tiles' beta_max (upper) and delta_max (qside) to the engineered rows alone, so the pretest
    decides; in-kernel bounds (no all-uniform launches) and other phase cuts read the same
    tables."""
    fx, ix, key64 = indexed(gpu, kind, "bf16", 64, 10 if kind == "qside" else 16, N=N, place="tiles",
                            background=background)
    Q, where = fx.queries(300, SLOTS)
    for k in (1, 10):
        check(ix, fx, key64, Q, where, k, "fgemm", dict(env, CWQ_FG_I8="-1"), monkeypatch, i8_launches=False)


@pytest.mark.parametrize("kind,kmax,k,D", BATCH[:12] + [("upper", 64, 10, 200), ("upper", 64, 64, 768)])
@pytest.mark.parametrize("operand", ["int8", "bf16"])
def test_batch_int8(gpu, operand, kind, kmax, k, D, monkeypatch):
    """Every filter launch on the int8 operands, on the int8 fixtures and on the bf16 ones (each
    operand type survives the other's worst case)."""
    fx, ix, key64 = indexed(gpu, kind, operand, D, kmax)
    Q, where = fx.queries(300, SLOTS)
    with_panel(ix, Q, monkeypatch)
    check(ix, fx, key64, Q, where, k, "fgemm", {"CWQ_FG_I8": "0"}, monkeypatch, i8_launches=True)


@pytest.mark.parametrize("N", [16640, 16500])
@pytest.mark.parametrize("kind", ["upper", "lower", "qside"])
def test_batch_int8_tile_placement(gpu, kind, N, monkeypatch):
    """The int8 tables' beta_max / delta_max (tiles_i8_kernel) with the engineered rows at the
    tiles' edges and in the last tile (full: its last rows; partial); default policy: int8
    from a quarter of the row tiles on, the rows at the end in an int8 launch and rows 0-256
    in a bf16 one."""
    fx, ix, key64 = indexed(gpu, kind, "int8", 64, 10 if kind == "qside" else 16, N=N, place="tiles")
    Q, where = fx.queries(300, SLOTS)
    with_panel(ix, Q, monkeypatch)
    for env in ({"CWQ_FG_I8": "0"}, {}):
        for k in (1, 10):
            check(ix, fx, key64, Q, where, k, "fgemm", env, monkeypatch, i8_launches=True)


@pytest.mark.parametrize("i8", ["0", "1"])
@pytest.mark.parametrize("nq", [1, 16, 17, 64])
@pytest.mark.parametrize("operand", ["bf16", "int8"])
def test_stream(gpu, operand, nq, i8, monkeypatch):
    """The per-call stream filter, bf16 and int8 pass, on both fixture families."""
    for kind, kmax, k in (("upper", 64, 64), ("lower", 64, 10), ("qside", 10, 10), ("both", 1, 1)):
        fx, ix, key64 = indexed(gpu, kind, operand, 64, kmax)
        Q, where = fx.queries(nq, (0, 16, nq - 2) if nq > 16 else (0,))
        check(ix, fx, key64, Q, where, k, "stream", {"CWQ_STREAM_I8": i8}, monkeypatch, int8_pass=i8 == "1")


@pytest.mark.parametrize("nq", [8, 70])
@pytest.mark.parametrize("operand", ["bf16", "int8"])
@pytest.mark.parametrize("kind", ["upper", "lower", "qside", "both", "both10"])
def test_basic_through_the_filter(gpu, kind, operand, nq, monkeypatch):
    """categorize's 64-row lists through the filter (per-call lists and the batch filter, the
    categorize key) and through the exact scan: the same nodes, n_found and n_calls.  The
    key is min(lp(parent), lp(leaf)): the upper and lower fixtures' rows lie next to the query,
    above the root's lp, and tie at it, so only the qside and both fixtures (rows |x| away,
    below the root's lp) make the bound decide the list, and only at its end; both10 has 10
    top rows over 64 bottom rows, so that a bound too narrow loses one of the 10 nodes asked
    for."""
    fx, ix, _ = indexed(gpu, "both", operand, 64, 10, nbot=64) if kind == "both10" else indexed(gpu, kind, operand, 64, 64)
    Q, where = fx.queries(nq, (0, 5))
    Qd = torch.from_numpy(Q).to("cuda:0")
    got = ix.categorize(Qd, 10)
    st = ix.last_categorize_stats()
    monkeypatch.setenv("CWQ_CAT_FILTER", "0")
    ref = ix.categorize(Qd, 10)
    monkeypatch.delenv("CWQ_CAT_FILTER")
    print(kind, operand, nq, st)
    for name, a, b in zip(("nodes", "n_found", "n_calls"), ref, got):
        assert torch.equal(a, b), name
    assert st["filter_reruns"] == 0, st
    for slot, g in where:   # a flat tree: the leaves in key order (node = filter row + 1)
        assert got[0][slot].tolist() == (fx.eng[g][:10] + 1).tolist(), (slot, g)


@pytest.mark.parametrize("kind", ["upper", "lower"])
def test_group_centred_rows(gpu, kind, monkeypatch):
    """Rows stored centred at their cluster's mean (cwq_group.hip): the engineered rows'
    residuals are coherent relative to that centre.  Batch and per-call filter against the
    exact scan, with group pruning on and off."""
    fx = B.GroupedFixture(kind)
    mean, var, parent, nos = fx.tree()
    monkeypatch.setenv("CWQ_GROUP_CENTRE", "1")
    ix = gpu.index.CobwebIndex(torch.from_numpy(mean), torch.from_numpy(var), parent, nos, device="cuda:0")
    monkeypatch.delenv("CWQ_GROUP_CENTRE")
    fi = ix.filter_info()
    assert fi["group_centred"] and fi["groups"] == len(fx.centres) and fi["group_rows"] == len(fx.rows), fi
    key64 = fx.keys(ix.level_weights)
    for prune in (True, False):
        assert ix.last_prune_stats()["available"]
        for nq, path in ((300, "fgemm"), (8, "stream")):
            Q, where = fx.queries(nq, SLOTS if nq > 64 else (0, 5))
            for k in (1, 10):
                check(ix, fx, key64, Q, where, k, path, {} if prune else {"CWQ_GROUP_PRUNE": "0"}, monkeypatch)
                assert (ix.last_prune_stats()["queries"] > 0) == prune, ix.last_prune_stats()
    ix.close()


# ----------------------------------------------------------------------------------------
# internal-node bounds (int_path_prep_kernel / int_prep_kernel, query_prep2_kernel)
# ----------------------------------------------------------------------------------------
def path_operands(mean, var, parent, weights, nodes):
    """int_path_prep_kernel's operand rows restated in numpy: Bsum(n) = fl32(sum_a w_a b'_a)
    over the non-root nodes a of n's path, b'_a = [-w/2, fl(mu_a - c) w] in fp32 with
    A = 1 / sqrtf(var), w = A A (int_prep_kernel), c the root mean."""
    f32 = np.float32
    w_of = lambda d: weights[d] if weights is not None and d < len(weights) else 1.0
    depth = np.zeros(len(parent), np.int64)
    for i in range(1, len(parent)):
        depth[i] = depth[parent[i]] + 1
    out = np.zeros((len(nodes), 2 * mean.shape[1]), np.float64)
    for j, n in enumerate(nodes):
        a = int(n)
        while parent[a] >= 0:
            A = f32(1.0) / np.sqrt(var[a].astype(f32))
            w = (A * A).astype(f32)
            b = np.concatenate([f32(-0.5) * w, (mean[a] - mean[0]).astype(f32) * w]).astype(f32)
            out[j] += w_of(depth[a]) * b.astype(np.float64)
            a = int(parent[a])
    return out.astype(f32)


def query_operand(x, c):
    """query_prep2_kernel: a = [x'^2, x'] in fp32, x' = fl(x - c)."""
    xc = (x.astype(np.float32) - c.astype(np.float32)).astype(np.float32)
    return np.concatenate([(xc * xc).astype(np.float32), xc], axis=-1)


def coherent_query(b, c, sign, rng, n_cand=256):
    """A query whose split error against the operand row b is as large as its dimensions allow
    with the sign `sign`: the error a.b - a_hi.b_hi is a sum over dimensions, so each
    dimension takes, of n_cand values of magnitude 0.5-1.5, the one whose terms (x'^2 and x'
    against b's two halves: the signs of x', of its residual and of the residual of x'^2)
    add most in that direction."""
    D = len(c)
    cand = (rng.uniform(0.5, 1.5, (n_cand, D)) * rng.choice([-1.0, 1.0], (n_cand, D))).astype(np.float32)
    a = query_operand(cand, c)                                   # [n_cand, 2D]
    ah, al = B.split(a, "bf16")
    bh, bl = B.split(b[None], "bf16")
    e = ah * bl + al * bh + al * bl
    e = e[:, :D] + e[:, D:]                                      # per dimension
    pick = np.argmax(sign * e, axis=0)
    return cand[pick, np.arange(D)]


def split_error_ratio(x, b, c):
    """|a.b - a_hi.b_hi| over its Cauchy-Schwarz bound |a_hi||b_lo| + |a_lo||b_hi| + |a_lo||b_lo|."""
    ah, al = B.split(query_operand(x, c)[None], "bf16")
    bh, bl = B.split(b[None], "bf16")
    n = lambda v: float(np.sqrt((v * v).sum()))
    real = float((ah * bl + al * bh + al * bl).sum())
    return abs(real) / (n(ah) * n(bl) + n(al) * n(bh) + n(al) * n(bl))


@pytest.mark.parametrize("path", ["1", "0"])
@pytest.mark.parametrize("tree", ["three_level", "two_level"])
def test_prefix_bounds_enclose_exact_coherent(gpu, tree, path, monkeypatch):
    """tests/test_gpu_filter.py test_prefix_bounds_enclose_exact on queries whose rounding
    residuals are coherent with the node operands: for 16 leaf parents a query that pushes the
    split error of the path-sum dot up and one that pushes it down.  Input condition (fp64,
    from the inputs alone): for at least one (query, leaf parent) pair the real split error is
    at least half its Cauchy-Schwarz bound (Gaussian queries: ~1/sqrt(2 D))."""
    from test_gpu_filter import _bounds_tree
    monkeypatch.setenv("CWQ_INT_PATH", path)
    X, mean, var, parent, nos, w = _bounds_tree(gpu, tree)
    ix = gpu.index.CobwebIndex(mean, var, parent, nos, w, device="cuda:0")
    mean_h, var_h = mean.cpu().numpy(), var.cpu().numpy()
    n = parent.shape[0]
    nch = np.bincount(parent[1:], minlength=n)
    internal = np.nonzero(nch > 0)[0]
    leafpar = np.zeros(n, dtype=bool)
    kids = np.arange(1, n)
    leafpar[parent[1:][nch[kids] == 0]] = True
    lp_nodes = np.nonzero(leafpar)[0]
    targets = np.concatenate([lp_nodes[:8], lp_nodes[-8:]])
    Bsum = path_operands(mean_h, var_h, parent, w, targets)
    rng = np.random.default_rng(91)
    Q = np.stack([coherent_query(b, mean_h[0], s, rng) for b in Bsum for s in (1.0, -1.0)])
    ratio = np.array([split_error_ratio(Q[2 * j + i], Bsum[j], mean_h[0]) for j in range(len(targets)) for i in (0, 1)])
    gauss = split_error_ratio(rng.standard_normal(mean_h.shape[1]).astype(np.float32), Bsum[0], mean_h[0])
    print(f"{tree} path={path}: split error / Cauchy-Schwarz bound: coherent min {ratio.min():.3f} "
          f"max {ratio.max():.3f}, a Gaussian query {gauss:.4f}")
    assert ratio.max() >= 0.5
    lo, hi, ex = ix.prefix_bounds(torch.from_numpy(Q).to("cuda:0"))
    need = torch.from_numpy(leafpar[internal]).to("cuda:0")
    fin = torch.isfinite(lo) & torch.isfinite(hi)
    assert bool(fin[:, need].all()), "a leaf parent without bounds"
    assert bool(torch.isfinite(ex).all())
    bad = (~((lo <= ex) & (ex <= hi)) & fin).nonzero()
    assert bad.shape[0] == 0, [(int(q), int(i), float(lo[q, i]), float(ex[q, i]), float(hi[q, i]))
                               for q, i in bad[:5].tolist()]
    ix.close()
