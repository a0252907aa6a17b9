"""CPU-side checks of the masked ranking loss: the two entry points are
exported and declared, every argument error that can be raised without a device is CWQ_ERR_ARG
before any device work, and the GPU tests' own reference -- the unmasked yardsticks on scores
whose disallowed columns are -inf -- equals the plain yardsticks on the sub-corpus of allowed
sentences."""
import ctypes
import os
import re

import numpy as np
import pytest

import ce_yardstick as C
import sparse_yardstick as SY
from conftest import ROOT

torch = pytest.importorskip("torch")

HEADER = os.path.join(ROOT, "include", "cobweb_query.h")
NEW = ("cwq_rank_ce_masked", "cwq_rank_ce_topk_masked")


def test_symbols_exported_and_declared(pkg):
    txt = open(HEADER).read()
    L = pkg.lib()
    for s in NEW:
        assert re.search(r"^\s*int\s+" + s + r"\s*\(", txt, re.M), s
        assert hasattr(L, s) and s in pkg._lib.SIGNATURES, s
    assert "cwq_masklosscalls.hip" in pkg.build.SOURCES


def test_argument_errors_without_a_device(pkg):
    """The checks that read no handle come first, so a block of zero bytes can stand for the index
    and the mask: each call must return before it would touch either (or a device)."""
    L = pkg.lib()
    ERR = pkg._lib.CWQ_ERR_ARG
    fake_ix = ctypes.create_string_buffer(1 << 16)
    fake_m = ctypes.create_string_buffer(1 << 12)
    ix, m = ctypes.addressof(fake_ix), ctypes.addressof(fake_m)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    masks = (ctypes.c_void_p * 2)(m, m)
    moq = np.array([0, 1, 2, 0], np.int32)

    def dense(ix_=ix, m_=m, q=p, nq=4, target=p, T=1.0, loss=p):
        return L.cwq_rank_ce_masked(ix_, m_, q, nq, target, T, loss, None, None, None, None)

    def topk(ix_=ix, masks_=masks, n_masks=2, moq_=moq.ctypes.data, q=p, nq=4, target=p, T=1.0, K=4, loss=p, grad=None):
        return L.cwq_rank_ce_topk_masked(ix_, masks_, n_masks, moq_, q, nq, target, T, K, loss, grad, None, None, None,
                                         None, None)

    for kw in (dict(ix_=None), dict(m_=None), dict(q=None), dict(target=None), dict(loss=None), dict(nq=-1),
               dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf"))):
        assert dense(**kw) == ERR, kw
        assert L.cwq_last_error()
    for kw in (dict(ix_=None), dict(masks_=None), dict(q=None), dict(target=None), dict(loss=None), dict(nq=-1),
               dict(K=0), dict(K=-3), dict(T=0.0), dict(T=float("nan")), dict(T=float("inf")), dict(n_masks=0),
               dict(moq_=None), dict(K=4096, grad=p), dict(n_masks=2)):   # the last: moq names slot 2 of 2
        assert topk(**kw) == ERR, kw
        assert L.cwq_last_error()
    assert b"mask_of_query[2]" in L.cwq_last_error()
    null_entry = (ctypes.c_void_p * 2)(None, None)
    assert topk(masks_=null_entry, moq_=np.zeros(4, np.int32).ctypes.data) == ERR
    assert b"masks[0]" in L.cwq_last_error()


def test_masked_yardstick_is_the_plain_yardstick_on_the_allowed_subcorpus():
    """-inf columns add nothing to the fp64 loss, softmax and rank, and taking the disallowed
    sentences out of the tree is the top-K yardstick of the sub-corpus."""
    rng = np.random.default_rng(0)
    nq, ns = 7, 60
    nos = rng.integers(1, 25, ns)              # several sentences share a node: equal scores, ordered by id
    S = (rng.standard_normal((nq, 25)).astype(np.float32) * 3)[:, nos]
    nos[::11] = -1
    S[:, nos < 0] = -np.inf
    flags = rng.random(ns) < 0.5
    keep = np.nonzero(flags)[0]
    T = np.full(nq, 1.7)
    Sm = S.copy()
    Sm[:, ~flags] = -np.inf
    allowed_in_tree = keep[nos[keep] >= 0]
    tg = allowed_in_tree[rng.integers(0, len(allowed_in_tree), nq)]
    tsub = np.searchsorted(keep, tg)
    assert np.allclose(C.loss_on_scores(Sm, tg, T), C.loss_on_scores(S[:, keep], tsub, T), rtol=0, atol=1e-12)
    G = C.softmax_grad_on_scores(Sm, tg, T)
    assert not G[:, ~flags].any()
    assert np.allclose(G[:, keep], C.softmax_grad_on_scores(S[:, keep], tsub, T), rtol=0, atol=1e-15)
    assert torch.equal(C.rank_of_targets(torch.from_numpy(Sm), tg, nos),
                       C.rank_of_targets(torch.from_numpy(S[:, keep]), tsub, nos[keep]))
    for K in (1, 5, 40):
        a = SY.truncated(Sm, np.where(flags, nos, -1), tg, T, K)
        b = SY.truncated(S[:, keep], nos[keep], tsub, T, K)
        for q in range(nq):
            assert np.array_equal(a["cand"][q], keep[b["cand"][q]])
        assert np.array_equal(a["rank"], b["rank"])
        assert np.allclose(a["loss"], b["loss"], rtol=0, atol=1e-12) and np.allclose(a["bound"], b["bound"], rtol=0, atol=1e-12)
        assert np.allclose(a["G"][:, keep], b["G"], rtol=0, atol=1e-15) and not a["G"][:, ~flags].any()
