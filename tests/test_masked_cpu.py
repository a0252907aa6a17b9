"""Masked Fast top-k, the parts that need no GPU: the sentence bitset cwq_mask_create reads
(pack_sentence_bits) against numpy.packbits, and the new entry points' argument checks, which
fail before any device work."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def want_words(flags):
    """numpy's little-bit-order packing, padded to whole uint32 words, read little-endian."""
    b = np.packbits(np.asarray(flags, bool), bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)])
    return b.view("<u4")


def words_of(t):
    assert t.dtype == torch.int32
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_bit_packing_matches_numpy_packbits(pkg, n):
    rng = np.random.default_rng(n)
    for flags in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
        want = want_words(flags)
        assert len(want) == (n + 31) // 32
        np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(flags, n)), want)               # ndarray
        np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(torch.from_numpy(flags), n)), want)   # tensor
        ids = np.flatnonzero(flags)
        np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(ids.tolist(), n)), want)        # id list
        np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(torch.from_numpy(ids), n)), want)


def test_id_lists_with_duplicates(pkg):
    n = 100
    ids = [3, 3, 64, 0, 99, 64, 3, 31, 32]
    flags = np.zeros(n, bool)
    flags[ids] = True
    np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(ids, n)), want_words(flags))
    np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits(torch.tensor(ids, dtype=torch.int32), n)),
                                  want_words(flags))
    np.testing.assert_array_equal(words_of(pkg.index.pack_sentence_bits([], n)), want_words(np.zeros(n, bool)))


@pytest.mark.parametrize("bad", [[-1], [100], [0, 5, 100], [2 ** 40]])
def test_out_of_range_ids_raise(pkg, bad):
    with pytest.raises(ValueError, match="sentence ids"):
        pkg.index.pack_sentence_bits(bad, 100)
    with pytest.raises(ValueError, match="sentence ids"):
        pkg.index.pack_sentence_bits(torch.tensor(bad), 100)


@pytest.mark.parametrize("length", [0, 99, 101])
def test_wrong_length_bool_masks_raise(pkg, length):
    with pytest.raises(ValueError, match="one entry per sentence"):
        pkg.index.pack_sentence_bits(np.ones(length, bool), 100)
    with pytest.raises(ValueError, match="one entry per sentence"):
        pkg.index.pack_sentence_bits(torch.ones(length, dtype=torch.bool), 100)


def test_float_allowed_raises(pkg):
    with pytest.raises(ValueError):
        pkg.index.pack_sentence_bits(np.ones(100, np.float32), 100)


def test_masked_entry_points_reject_bad_arguments_before_device_work(pkg):
    """NULL handles / pointers and k <= 0 are CWQ_ERR_ARG with a message, as in
    test_error_path_without_gpu_compute: nothing here touches a device.  (k <= 0 with real
    handles is checked on the GPU, tests/test_gpu_masked_topk.py.)"""
    L = pkg.lib()
    ERR = pkg._lib.CWQ_ERR_ARG
    h = ctypes.c_void_p()
    out4 = (ctypes.c_int64 * 4)()
    assert L.cwq_mask_create(None, None, 0, None, ctypes.byref(h)) == ERR
    assert b"NULL" in L.cwq_last_error()
    assert L.cwq_mask_create(None, None, 10, None, None) == ERR
    assert L.cwq_mask_info(None, out4) == ERR
    assert L.cwq_mask_info(None, None) == ERR
    assert L.cwq_last_mask_stats(None, out4) == ERR
    assert L.cwq_score_topk_masked(None, None, None, 1, 10, None, None, None) == ERR
    assert b"NULL" in L.cwq_last_error()
    assert L.cwq_score_topk_masked(None, None, None, 0, 10, None, None, None) == ERR   # NULL idx / mask even at nq 0
    for k in (0, -3):
        assert L.cwq_score_topk_masked(None, None, None, 1, k, None, None, None) == ERR
    assert L.cwq_mask_destroy(None) == 0


def test_signatures_cover_the_masked_entry_points(pkg):
    for name in ("cwq_mask_create", "cwq_mask_destroy", "cwq_mask_info", "cwq_score_topk_masked",
                 "cwq_last_mask_stats"):
        assert name in pkg._lib.SIGNATURES
        assert hasattr(pkg.lib(), name)
