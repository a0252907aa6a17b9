"""Per-query masks (cwq_score_topk_masked_multi), the parts that need no GPU: the
export and its ctypes signature, every argument error (CWQ_ERR_ARG with a message, before any
device work -- checked with NULL and fake handles, which would crash anything that went
further), the keyword rules of the Python calls, and the planner's stand-alone check program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_and_signature(pkg):
    L = pkg.lib()
    for name in ("cwq_score_topk_masked_multi", "cwq_last_mask_multi_stats"):
        assert name in pkg._lib.SIGNATURES
        assert hasattr(L, name)
    res, args = pkg._lib.SIGNATURES["cwq_score_topk_masked_multi"]
    assert res is ctypes.c_int and len(args) == 10
    assert len(pkg._lib.SIGNATURES["cwq_last_mask_multi_stats"][1]) == 2
    assert L.cwq_version() >= 310


def fake_handles(serial_index=7, serial_mask=7):
    """Zeroed memory with only the serial number set (the first field of both structs): enough
    for the argument checks, which read the handles' plain fields and nothing on a device."""
    ix = (ctypes.c_uint64 * 4096)()
    m = (ctypes.c_uint64 * 64)()
    ix[0] = serial_index
    m[0] = serial_mask
    return ix, m


def test_argument_errors_before_device_work(pkg):
    L = pkg.lib()
    ERR = pkg._lib.CWQ_ERR_ARG
    call = L.cwq_score_topk_masked_multi
    ix, m = fake_handles()
    masks = (ctypes.c_void_p * 4)(*[ctypes.addressof(m)] * 4)
    moq = (ctypes.c_int32 * 3)(0, 3, 1)
    q = (ctypes.c_float * 8)()
    ids = (ctypes.c_int64 * 64)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)
    # NULL idx / masks / mask_of_query (also at nq == 0), NULL q / ids at nq > 0
    assert call(None, masks, 4, moq, q, 3, 5, ids, None, None) == ERR
    assert b"NULL" in L.cwq_last_error()
    assert call(P(ix), None, 4, moq, q, 3, 5, ids, None, None) == ERR
    assert call(P(ix), masks, 4, None, q, 3, 5, ids, None, None) == ERR
    assert call(P(ix), masks, 4, None, None, 0, 5, None, None, None) == ERR
    assert call(P(ix), masks, 4, moq, None, 3, 5, ids, None, None) == ERR
    assert call(P(ix), masks, 4, moq, q, 3, 5, None, None, None) == ERR
    assert b"NULL" in L.cwq_last_error()
    # n_masks < 1
    for n in (0, -2):
        assert call(P(ix), masks, n, moq, q, 3, 5, ids, None, None) == ERR
        assert b"n_masks" in L.cwq_last_error()
    # k <= 0
    for k in (0, -3):
        assert call(P(ix), masks, 4, moq, q, 3, k, ids, None, None) == ERR
        assert b"k must be" in L.cwq_last_error()
    # a NULL entry
    holes = (ctypes.c_void_p * 4)(ctypes.addressof(m), ctypes.addressof(m), None, ctypes.addressof(m))
    assert call(P(ix), holes, 4, moq, q, 3, 5, ids, None, None) == ERR
    assert b"masks[2]" in L.cwq_last_error() and b"NULL" in L.cwq_last_error()
    # a mask of another index: the single-mask call's message
    _, other = fake_handles(serial_mask=8)
    mixed = (ctypes.c_void_p * 4)(ctypes.addressof(m), ctypes.addressof(m), ctypes.addressof(m), ctypes.addressof(other))
    assert call(P(ix), mixed, 4, moq, q, 3, 5, ids, None, None) == ERR
    multi_msg = L.cwq_last_error()
    assert L.cwq_score_topk_masked(P(ix), P(other), q, 3, 5, ids, None, None) == ERR
    assert multi_msg == L.cwq_last_error() and b"another index" in multi_msg
    # mask_of_query outside [0, n_masks): the first offending query is named
    for bad, where in (((0, 4, 9), b"mask_of_query[1]"), ((0, 1, -1), b"mask_of_query[2]"), ((-5, 7, 1), b"mask_of_query[0]")):
        assert call(P(ix), masks, 4, (ctypes.c_int32 * 3)(*bad), q, 3, 5, ids, None, None) == ERR
        assert where in L.cwq_last_error(), L.cwq_last_error()
    # nq == 0 with good arguments: a no-op
    assert call(P(ix), masks, 4, moq, None, 0, 5, None, None, None) == 0
    # the stats call
    out8 = (ctypes.c_int64 * 8)()
    assert L.cwq_last_mask_multi_stats(None, out8) == ERR
    assert L.cwq_last_mask_multi_stats(P(ix), None) == ERR
    assert L.cwq_last_mask_multi_stats(P(ix), out8) == 0 and list(out8) == [0] * 8


def test_keyword_rules_raise_before_anything_else(pkg):
    """masks= with mask=, allowed_sets= with allowed=, and either half of a pair alone: ValueError
    before the object is touched (so bare objects without an index serve)."""
    ix = object.__new__(pkg.index.CobwebIndex)
    q = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError, match="not both"):
        ix.score_topk(q, 3, mask=object(), masks=[object()], mask_of_query=[0, 0])
    with pytest.raises(ValueError, match="go together"):
        ix.score_topk(q, 3, masks=[object()])
    with pytest.raises(ValueError, match="go together"):
        ix.score_topk(q, 3, mask_of_query=[0, 0])
    w = object.__new__(pkg.CobwebWrapper)
    with pytest.raises(ValueError, match="not both"):
        w.cobweb_predict_batch(q, 3, allowed=[1, 2], allowed_sets=[[1], [2]], set_of_query=[0, 1])
    with pytest.raises(ValueError, match="go together"):
        w.cobweb_predict_batch(q, 3, allowed_sets=[[1], [2]])
    with pytest.raises(ValueError, match="go together"):
        w.cobweb_predict_batch(q, 3, set_of_query=[0, 1])


def test_planner_check_program(tmp_path):
    """scripts/maskplan_check.cpp: the planner over edge and random shapes, with the address and
    undefined-behaviour sanitizers where the host toolchain links them."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found (CXX, c++, g++, clang++)")
    src = os.path.join(ROOT, "scripts", "maskplan_check.cpp")
    exe = str(tmp_path / "maskplan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)   # a toolchain without the sanitizer runtimes
        assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plans ok" in r.stdout
