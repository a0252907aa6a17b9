"""CPU checks of the device-resident tree's test yardstick and of its C entry points'
argument validation.  No GPU compute here."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from resident_yardstick import bfs_flatten, scramble


@pytest.mark.parametrize("name,seed", [("g1_hier_d32", 1), ("g5_hier_d384", 5), ("g9_interleaved_d16", 9)])
def test_yardstick_reproduces_golden_bfs(name, seed):
    """The reference's own trees, scrambled into a random slot numbering with removed and
    unused slots mixed in, come back from the yardstick in the goldens' BFS order: parent,
    sid_ptr, sid_list (G9's lists are in the order the reference's shuffles left them),
    counts, means, and variances with numpy's float32 meanSq / count + prior_var bits."""
    g = load_golden(name)
    s = scramble(g, seed)
    assert (s["parent"] == -2).sum() > 10 and len(s["parent"]) > len(g["parent"])
    y = bfs_flatten(s["parent"], s["child_ptr"], s["child_idx"], s["root"], s["count"], s["mean"], s["meanSq"],
                    g["prior_var"], s["slot_of_sentence"], s["slot_sids"])
    np.testing.assert_array_equal(y["parent"], g["parent"])
    np.testing.assert_array_equal(y["sid_ptr"], g["sid_ptr"])
    np.testing.assert_array_equal(y["sid_list"], g["sid_list"])
    np.testing.assert_array_equal(y["count"], g["count"])
    np.testing.assert_array_equal(y["mean"], g["mean"])
    want = g["meanSq"] / g["count"][:, None] + np.float32(g["prior_var"])
    assert want.dtype == np.float32
    np.testing.assert_array_equal(y["var"].view(np.int32), want.view(np.int32))
    # node_of_sentence agrees with the lists; the compact form rebuilds the full array
    owner = np.repeat(np.arange(len(g["count"])), np.diff(g["sid_ptr"]))
    nos = np.full(int(g["n_sent"]), -1, np.int64)
    nos[g["sid_list"]] = owner
    np.testing.assert_array_equal(y["node_of_sentence"], nos)
    full = np.repeat(y["var_row"][:, None], want.shape[1], 1)
    full[y["an_nodes"]] = y["an_var"]
    np.testing.assert_array_equal(full.view(np.int32), want.view(np.int32))
    iso = np.setdiff1d(np.arange(len(want)), y["an_nodes"])
    assert (want[iso].view(np.int32) == want[iso, :1].view(np.int32)).all()
    assert len(y["an_nodes"]) and (np.diff(y["an_nodes"]) > 0).all()
    if name != "g9_interleaved_d16":     # without the lists: ascending ids per node
        y2 = bfs_flatten(s["parent"], s["child_ptr"], s["child_idx"], s["root"], s["count"], s["mean"],
                         s["meanSq"], g["prior_var"], s["slot_of_sentence"])
        np.testing.assert_array_equal(y2["sid_list"], g["sid_list"])


def test_yardstick_skips_sentences_outside_the_tree():
    g = load_golden("g1_hier_d32")
    s = scramble(g, 3)
    sos = s["slot_of_sentence"].copy()
    dead = int(np.nonzero(s["parent"] == -2)[0][0])
    sos[5], sos[7] = -1, dead
    y = bfs_flatten(s["parent"], s["child_ptr"], s["child_idx"], s["root"], s["count"], s["mean"], s["meanSq"],
                    g["prior_var"], sos)
    assert y["node_of_sentence"][5] == -1 and y["node_of_sentence"][7] == -1
    assert (np.delete(y["node_of_sentence"], [5, 7]) >= 0).all()


def test_resident_entry_points_validate_before_device_work(pkg):
    """NULL handles and outputs, a negative sentence count: CWQ_ERR_ARG and a message, before
    any device work (the pattern of test_error_path_without_gpu_compute)."""
    L = pkg.lib()
    ERR = pkg._lib.CWQ_ERR_ARG
    out = ctypes.c_void_p()
    buf = np.zeros(625, np.uint32).ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(16)       # never dereferenced: the other argument fails first

    def msg():
        return L.cwq_fit_last_error()

    assert L.cwq_index_create_from_fit(None, None, 0, None, 0, None, ctypes.byref(out)) == ERR
    assert b"cwq_index_create_from_fit" in msg() and b"cwq_index_create_from_fit" in L.cwq_last_error()
    assert L.cwq_index_create_from_fit(fake, None, 0, None, 0, None, None) == ERR and b"out is NULL" in msg()
    assert L.cwq_index_create_from_fit(fake, None, -1, None, 0, None, ctypes.byref(out)) == ERR
    assert b"sentence map" in msg() and b"sentence map" in L.cwq_last_error()
    assert L.cwq_index_create_from_fit(fake, None, 3, None, 0, None, ctypes.byref(out)) == ERR
    assert L.cwq_fit_flatten(None, None, 0, None, ctypes.byref(out)) == ERR and b"NULL handle" in msg()
    assert L.cwq_fit_flatten(fake, None, 0, None, None) == ERR and b"out is NULL" in msg()
    assert L.cwq_fit_flatten(fake, None, -1, None, ctypes.byref(out)) == ERR and b"sentence map" in msg()
    assert L.cwq_fit_flat_info(None, buf) == ERR and L.cwq_fit_flat_copy(None, *[None] * 9) == ERR
    assert L.cwq_fit_flat_destroy(None) == 0
    assert L.cwq_fit_grow(None, 100, None) == ERR and b"cwq_fit_grow" in msg()
    assert L.cwq_fit_set_rng(None, buf, None) == ERR and b"cwq_fit_set_rng" in msg()
    assert L.cwq_fit_set_rng(fake, None, None) == ERR and b"cwq_fit_set_rng" in msg()
    assert L.cwq_fit_get_rng(None, buf, None) == ERR and b"cwq_fit_get_rng" in msg()
    assert L.cwq_fit_get_rng(fake, None, None) == ERR and b"cwq_fit_get_rng" in msg()
    assert L.cwq_fit_rewind(None, None) == ERR and L.cwq_fit_info(None, buf, None) == ERR
    assert L.cwq_fit_info(fake, None, None) == ERR
    assert out.value is None
