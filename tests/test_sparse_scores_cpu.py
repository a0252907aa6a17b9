"""CPU checks of the sparse differentiable scores: the fp64 restatement of the
truncated loss and its bound (tests/sparse_yardstick.py) against the full loss on the dense fp64
scorer, the gathered backward against autograd, the exported symbols and the argument errors of
the three entry points (before any device work)."""
import ctypes

import numpy as np
import pytest

import ce_yardstick as C
import grad_yardstick as Y
import sparse_yardstick as SY
import test_gpu_grad as TG

NEW = {"cwq_score_pairs": 7, "cwq_score_pairs_backward": 8, "cwq_rank_ce_topk": 13}


@pytest.mark.parametrize("name", TG.GOLDENS)
def test_truncated_loss_bound_and_gathered_grad(name):
    arrays, Xq, d64, _, _ = TG.setup(name)
    mean, var, parent, nos = arrays
    tg3, temps, S = C.targets_and_temps(d64, Xq)
    ns = S.shape[1]
    last = np.array([SY.order(S[q], nos)[-1] for q in range(len(Xq))])
    for T in (temps, np.ones(len(Xq))):
        for targets in (tg3, last):
            full = C.loss_on_scores(S, targets, T)
            for K in (1, 3, 10, 64, ns):
                r = SY.truncated(S, nos, targets, T, K)
                gap = full - r["loss"]
                assert (gap >= -1e-12 * np.maximum(1, np.abs(full))).all(), (name, K, gap)
                assert (gap <= r["bound"] + 1e-12 * np.maximum(1, np.abs(full))).all(), (name, K, gap, r["bound"])
                if K >= ns:
                    assert np.abs(gap).max() <= 1e-12 * np.abs(full).max() and (r["bound"] == 0).all()
                    assert np.allclose(r["G"], C.softmax_grad_on_scores(S, targets, T), rtol=1e-10, atol=1e-14)
                exact = np.array([int(np.nonzero(SY.order(S[q], nos) == targets[q])[0][0]) + 1 for q in range(len(Xq))])
                assert (r["rank"] == np.minimum(exact, K + 1)).all()
    # autograd through the dense scorer with the sparse upstream = the gathered restatement
    r = SY.truncated(S, nos, last, temps, 10)
    auto = Y.grad_through(d64, Xq, r["G"])
    for q in range(len(Xq)):
        ids = np.nonzero(r["G"][q])[0]
        assert len(ids) == 11
        got = SY.gathered_grad(mean, var, parent, nos, Xq[q], ids, r["G"][q, ids])
        assert np.linalg.norm(got - auto[q]) <= 1e-10 * np.linalg.norm(auto[q]), (name, q)


def test_gathered_grad_skips_invalid_and_adds_duplicates():
    arrays, Xq, d64, _, _ = TG.setup("g10_grad_d24")
    mean, var, parent, nos = arrays
    ids = np.array([5, -1, 5, len(nos) + 3, 17])
    g = np.array([0.5, np.nan, 0.25, np.nan, -1.0])
    G = np.zeros((1, len(nos)))
    G[0, 5], G[0, 17] = 0.75, -1.0
    want = Y.grad_through(d64, Xq[:1], G)[0]
    got = SY.gathered_grad(mean, var, parent, nos, Xq[0], ids, g)
    assert np.isfinite(got).all() and np.linalg.norm(got - want) <= 1e-10 * np.linalg.norm(want)


def test_symbols_exported_with_signatures(pkg):
    L = pkg.lib()
    for name, nargs in NEW.items():
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args


def test_argument_errors_before_device_work(pkg):
    """NULL / m = 0 / K = 0 / a bad temperature: CWQ_ERR_ARG, decided from the arguments alone --
    the handle and the buffers here are host memory no kernel could read."""
    L = pkg.lib()
    E = pkg._lib.CWQ_ERR_ARG
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.cwq_score_pairs(None, p, 1, p, 1, p, None) == E
    assert L.cwq_score_pairs(p, None, 1, p, 1, p, None) == E
    assert L.cwq_score_pairs(p, p, 1, None, 1, p, None) == E
    assert L.cwq_score_pairs(p, p, 1, p, 1, None, None) == E
    assert L.cwq_score_pairs(p, p, -1, p, 1, p, None) == E
    assert L.cwq_score_pairs(p, p, 1, p, 0, p, None) == E
    assert b"m must be" in L.cwq_last_error()
    assert L.cwq_score_pairs_backward(None, p, 1, p, 1, p, p, None) == E
    assert L.cwq_score_pairs_backward(p, p, 1, p, 1, None, p, None) == E
    assert L.cwq_score_pairs_backward(p, p, 1, p, 1, p, None, None) == E
    assert L.cwq_score_pairs_backward(p, p, 1, p, 0, p, p, None) == E
    assert L.cwq_score_pairs_backward(p, p, -2, p, 1, p, p, None) == E
    assert L.cwq_score_pairs_backward(p, p, 1, p, 4097, p, p, None) == E
    assert b"cwq_rank_scores_backward" in L.cwq_last_error()
    assert L.cwq_rank_ce_topk(None, p, 1, p, 1.0, 4, p, p, p, p, p, p, None) == E
    assert L.cwq_rank_ce_topk(p, p, 1, None, 1.0, 4, p, p, p, p, p, p, None) == E
    assert L.cwq_rank_ce_topk(p, p, 1, p, 1.0, 4, None, p, p, p, p, p, None) == E
    assert L.cwq_rank_ce_topk(p, p, 1, p, 1.0, 0, p, p, p, p, p, p, None) == E
    assert b"K must be" in L.cwq_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.cwq_rank_ce_topk(p, p, 1, p, bad, 4, p, p, p, p, p, p, None) == E
        assert b"temperature" in L.cwq_last_error()
    assert L.cwq_rank_ce_topk(p, p, 1, p, 1.0, 4096, p, p, p, p, p, p, None) == E    # the backward's K + 1
    assert b"cwq_rank_scores_backward" in L.cwq_last_error()
    # nq == 0 is a no-op, also decided before the handle is touched
    assert L.cwq_score_pairs(p, p, 0, p, 3, p, None) == 0
    assert L.cwq_score_pairs_backward(p, p, 0, p, 3, p, p, None) == 0
    assert L.cwq_rank_ce_topk(p, p, 0, p, 1.0, 4, p, p, p, p, p, p, None) == 0
