"""CPU-side checks of the call-time level weights (cwq_rank_scores_w,
cwq_rank_scores_backward_w, cwq_rank_ce_w): the C ABI's argument checks, which
happen before any device work (no GPU here: the non-NULL pointers below are never
dereferenced), and the yardstick of the GPU tests (tests/lw_yardstick.py) against the
project's existing one and the reference's recorded scores."""
import ctypes

import numpy as np
import pytest

import grad_yardstick as Y
import lw_yardstick as W
from conftest import load_golden

torch = pytest.importorskip("torch")

P = ctypes.c_void_p(256)


def scores_w(pkg, idx=P, q=P, nq=1, w=P, n_w=3, out=P):
    return pkg.lib().cwq_rank_scores_w(idx, q, nq, w, n_w, out, None)


def backward_w(pkg, idx=P, q=P, nq=1, g=P, w=P, n_w=3, gq=P, gw=P):
    return pkg.lib().cwq_rank_scores_backward_w(idx, q, nq, g, w, n_w, gq, gw, None)


def ce_w(pkg, idx=P, q=P, nq=1, target=P, T=1.0, w=P, n_w=3, loss=P, gq=None, gw=None, ts=None, rank=None):
    return pkg.lib().cwq_rank_ce_w(idx, q, nq, target, T, w, n_w, loss, gq, gw, ts, rank, None)


def test_symbols_exported_with_signatures(pkg):
    L = pkg.lib()
    for name, n, wpos in (("cwq_rank_scores_w", 7, 3), ("cwq_rank_scores_backward_w", 9, 4), ("cwq_rank_ce_w", 13, 5)):
        assert hasattr(L, name)
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n and args[wpos + 1] is ctypes.c_int32
        assert len(getattr(L, name).argtypes) == n


@pytest.mark.parametrize("n_w", [-1, 65])
def test_bad_n_w(pkg, n_w):
    for fn in (scores_w, backward_w, ce_w):
        assert fn(pkg, n_w=n_w) == pkg._lib.CWQ_ERR_ARG
        assert b"n_w" in pkg.lib().cwq_last_error()
        assert fn(pkg, n_w=n_w, w=None) == pkg._lib.CWQ_ERR_ARG


def test_null_required_pointers(pkg):
    E = pkg._lib.CWQ_ERR_ARG
    for null in ("idx", "q", "out"):
        assert scores_w(pkg, **{null: None}) == E and b"NULL" in pkg.lib().cwq_last_error()
    for null in ("idx", "q", "g"):
        assert backward_w(pkg, **{null: None}) == E and b"NULL" in pkg.lib().cwq_last_error()
    assert backward_w(pkg, gq=None, gw=None) == E          # nothing to compute
    for null in ("idx", "q", "target", "loss"):
        assert ce_w(pkg, **{null: None}) == E and b"NULL" in pkg.lib().cwq_last_error()
    assert ce_w(pkg, T=0.0) == E and ce_w(pkg, nq=-1) == E


def test_empty_batch_is_a_noop(pkg):
    for w in (P, None):   # NULL weights: the index's own
        assert scores_w(pkg, nq=0, w=w) == pkg._lib.CWQ_OK
        assert backward_w(pkg, nq=0, w=w) == pkg._lib.CWQ_OK
        assert ce_w(pkg, nq=0, w=w, gq=P, gw=P) == pkg._lib.CWQ_OK


# ---- the yardstick ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g10():
    g = load_golden("g10_grad_d24")
    mean, var, parent, nos = Y.tree_arrays(g)
    return g, parent, nos, W.DenseW(mean, var, W.depth_matrices(parent, nos), torch.float64)


@pytest.mark.parametrize("wname", list(W.WEIGHTS))
def test_path_matrix_equals_grad_yardstick(g10, wname):
    """sum_d w[d] A_d against path_matrix's w[d] / L: equal up to the one fp64 rounding between
    w (1 / L) and w / L."""
    _, parent, nos, d64 = g10
    w = W.WEIGHTS[wname]
    mine = d64.path_matrix(torch.tensor(w, dtype=torch.float64)).numpy()
    want = Y.path_matrix(parent, nos, w)
    assert np.array_equal(mine != 0, want != 0)
    assert np.allclose(mine, want, rtol=4 * np.finfo(np.float64).eps, atol=0.0)


def test_scores_reproduce_recorded_reference_scores(g10):
    g, _, _, d64 = g10
    for key, w in (("rank_scores", W.WEIGHTS["default"]), ("rank_scores_w3", list(g["weights_w3"]))):
        wt = torch.tensor(w, dtype=torch.float64)
        S = torch.stack([d64.scores(torch.tensor(x, dtype=torch.float64), wt) for x in g["Xq"]]).numpy()
        e = np.abs(S - g[key]) / np.abs(S)
        print(f"g10 {key}: fp64 restatement vs recorded fp32 scores max rel {e.max():.3g}")
        assert e.max() < Y.LIMIT


@pytest.mark.parametrize("wname", list(W.WEIGHTS))
def test_weight_jacobian_is_the_unit_difference(g10, wname):
    """The score is linear in w: d scores / d w[d] = scores(w + e_d) - scores(w), to the
    rounding of that difference (a few ulp of the scores)."""
    g, _, _, d64 = g10
    w = torch.tensor(W.WEIGHTS[wname], dtype=torch.float64)
    x = torch.tensor(g["Xq"][0], dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: d64.scores(x, v), w)   # [n_sent, n_w]
    S0 = d64.scores(x, w)
    tol = 16 * np.finfo(np.float64).eps * float(S0.abs().max())
    for d in range(len(w)):
        e = torch.zeros_like(w)
        e[d] = 1.0
        diff = d64.scores(x, w + e) - S0
        assert float((J[:, d] - diff).abs().max()) <= tol, d
    assert len(w) <= d64.nl or not J[:, d64.nl:].any()   # past the tree's depth: zero
