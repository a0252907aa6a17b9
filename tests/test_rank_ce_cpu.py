"""CPU-side checks of the fused ranking loss's C ABI (cwq_rank_ce): every invalid argument is
CWQ_ERR_ARG with a message, before any device work; an empty batch is a no-op.  No GPU here:
the non-NULL pointers below are never dereferenced."""
import ctypes
import math

import pytest

P = ctypes.c_void_p(256)


def call(pkg, idx=P, q=P, nq=1, target=P, T=1.0, loss=P, grad=None, tscore=None, rank=None):
    return pkg.lib().cwq_rank_ce(idx, q, nq, target, T, loss, grad, tscore, rank, None)


def test_symbol_exported_with_signature(pkg):
    L = pkg.lib()
    assert hasattr(L, "cwq_rank_ce")
    res, args = pkg._lib.SIGNATURES["cwq_rank_ce"]
    assert res is ctypes.c_int and len(args) == 10 and args[4] is ctypes.c_float
    assert len(L.cwq_rank_ce.argtypes) == 10
    assert L.cwq_version() >= 300


@pytest.mark.parametrize("null", ["idx", "q", "target", "loss"])
def test_null_arguments(pkg, null):
    assert call(pkg, **{null: None}) == pkg._lib.CWQ_ERR_ARG
    assert b"NULL" in pkg.lib().cwq_last_error()


@pytest.mark.parametrize("T", [0.0, -1.0, math.inf, -math.inf, math.nan])
def test_bad_temperature(pkg, T):
    assert call(pkg, T=T) == pkg._lib.CWQ_ERR_ARG
    assert b"temperature" in pkg.lib().cwq_last_error()
    assert call(pkg, T=T, nq=0) == pkg._lib.CWQ_ERR_ARG   # also for an empty batch


def test_negative_nq(pkg):
    assert call(pkg, nq=-1) == pkg._lib.CWQ_ERR_ARG
    assert b"nq" in pkg.lib().cwq_last_error()


def test_empty_batch_is_a_noop(pkg):
    assert call(pkg, nq=0) == pkg._lib.CWQ_OK
    assert call(pkg, nq=0, grad=P, tscore=P, rank=P) == pkg._lib.CWQ_OK
