"""CPU-side checks of the differentiable rank scores: the C ABI of the backward entry point,
the gradient golden from the real reference (tests/golden/gen_golden_grad.py), and the
yardstick itself -- the fp64 dense restatement (tests/grad_yardstick.py) must reproduce the
reference's own recorded x.grad.  No GPU compute here."""
import ctypes
import os

import numpy as np

import grad_yardstick as Y
from conftest import GOLDEN

G10 = os.path.join(GOLDEN, "g10_grad_d24.npz")


def load_g10():
    assert os.path.exists(G10), "tests/golden/g10_grad_d24.npz is missing (gen_golden_grad.py writes it)"
    with np.load(G10, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_backward_symbol_exported_with_signature(pkg):
    L = pkg.lib()
    assert hasattr(L, "cwq_rank_scores_backward")
    res, args = pkg._lib.SIGNATURES["cwq_rank_scores_backward"]
    assert res is ctypes.c_int and len(args) == 6
    assert L.cwq_rank_scores_backward.argtypes is not None and len(L.cwq_rank_scores_backward.argtypes) == 6


def test_backward_null_arguments(pkg):
    """NULL arguments are CWQ_ERR_ARG before any device work (no GPU here)."""
    L = pkg.lib()
    p = ctypes.c_void_p(256)   # never dereferenced: another argument is NULL
    for args in [(None, p, 1, p, p, None), (p, None, 1, p, p, None), (p, p, 1, None, p, None), (p, p, 1, p, None, None)]:
        assert L.cwq_rank_scores_backward(*args) == pkg._lib.CWQ_ERR_ARG
        assert b"NULL" in L.cwq_last_error()


def test_g10_fixture_contents():
    g = load_g10()
    assert g["Xq"].shape == (8, 24) and g["X"].shape == (200, 24) and int(g["n_sent"]) == 200
    assert int(np.sum(np.diff(g["sid_ptr"]) > 1)) >= 3       # leaves that hold several sentences
    for tag in ("", "_w3"):
        for name in ("sum", "wsum", "ce"):
            a = g[f"grad_{name}{tag}"]
            assert a.shape == (8, 24) and np.isfinite(a).all() and np.abs(a).max() > 0
        s = g["rank_scores" + tag]
        assert np.all(g["ce_target" + tag] != np.argmax(s, axis=1))   # the target is not the top-1


def test_yardstick_reproduces_reference_grads():
    """fp64 autograd through the dense restatement against the reference's recorded x.grad
    (fp32 autograd through its sparse path matrix), default weights and [1.0, 2.0, 0.5]."""
    g = load_g10()
    mean, var, parent, nos = Y.tree_arrays(g)
    for tag, w in (("", None), ("_w3", list(g["weights_w3"]))):
        d64 = Y.Dense(mean, var, Y.path_matrix(parent, nos, w), Y.torch.float64)
        S, cases = Y.upstreams(d64, g["Xq"], targets=g["ce_target" + tag], temps=g["ce_T" + tag])
        assert np.max(np.abs(S - g["rank_scores" + tag]) / np.abs(S)) < Y.LIMIT
        # sum and ce carry the recorded target / temperature; wsum the recorded weighting
        want = {"sum": cases["sum"][1], "ce": cases["ce"][1],
                "wsum": Y.grad_through(d64, g["Xq"], g["W"].astype(np.float64))}
        for name, g64 in want.items():
            e = Y.rel_l2(g[f"grad_{name}{tag}"], g64)
            print(f"g10{tag} {name}: reference fp32 vs fp64 restatement, max rel L2 {e.max():.3g}")
            assert e.max() < Y.LIMIT, (tag, name, e)
