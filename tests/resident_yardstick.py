"""The yardstick of the device flatten (cwq_fit_flatten): a small numpy BFS over slot arrays.

A tree in slot form is what a cwq_fit handle holds: per slot a parent (-1 at the root, -2
for a slot that is not in the tree), the children in list order as CSR, count / mean /
meanSq, and for every sentence the slot that holds it.  `bfs_flatten` numbers the live
nodes as CobwebTree.flatten does (root 0, children consecutive in list order, levels in
order) and returns what the device must produce.  `scramble` turns BFS arrays (a golden
file) into slot arrays under a random slot numbering with unused and removed slots mixed
in.  tests/test_resident_cpu.py pins both against the reference's own trees.
"""
import numpy as np

F32 = np.float32


def bfs_flatten(parent, child_ptr, child_idx, root, count, mean, meanSq, prior_var, slot_of_sentence,
                slot_sids=None):
    """-> dict: parent [Nn] int64, slot_of_node [Nn], node_of_sentence [n_sent] int64 (-1: not
    in the tree), count [Nn], mean [Nn, D], var [Nn, D] float32 = meanSq / count + prior_var
    (prior_var for count 0), var_row [Nn] = var[:, 0], an_nodes (ascending: the rows whose D
    values are not all the same bits), an_var, depth (levels below the root), and sid_ptr /
    sid_list (each node's sentence ids: `slot_sids[slot]` in its order when given, else
    ascending)."""
    parent = np.asarray(parent)
    order, par, lo, depth = [int(root)], [-1], 0, 0
    while lo < len(order):          # one level per pass
        hi = len(order)
        for i in range(lo, hi):
            s = order[i]
            assert parent[s] != -2, "a removed slot is reachable"
            for c in child_idx[child_ptr[s]:child_ptr[s + 1]]:
                order.append(int(c))
                par.append(i)
        lo = hi
        if len(order) > hi:
            depth += 1
    son = np.asarray(order, np.int64)
    node_of_slot = np.full(len(parent), -1, np.int64)
    node_of_slot[son] = np.arange(len(son))
    sos = np.asarray(slot_of_sentence, np.int64)
    nos = np.where((sos >= 0) & (sos < len(parent)), node_of_slot[np.clip(sos, 0, len(parent) - 1)], -1)
    cnt = np.asarray(count, F32)[son]
    m2 = np.asarray(meanSq, F32)[son]
    pv = F32(prior_var)
    var = np.full(m2.shape, pv, F32)
    nz = cnt > 0
    var[nz] = m2[nz] / cnt[nz, None] + pv
    bits = var.view(np.int32)
    an = np.nonzero(~(bits == bits[:, :1]).all(1))[0].astype(np.int64)
    if slot_sids is None:
        lists = [np.nonzero(nos == i)[0].tolist() for i in range(len(son))]
    else:
        lists = [list(slot_sids.get(int(s), [])) for s in son]
    sid_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    sid_list = np.asarray([v for x in lists for v in x], np.int64)
    return {"parent": np.asarray(par, np.int64), "slot_of_node": son, "node_of_sentence": nos, "count": cnt,
            "mean": np.asarray(mean, F32)[son], "var": var, "var_row": var[:, 0].copy(), "an_nodes": an,
            "an_var": var[an], "depth": depth, "sid_ptr": sid_ptr, "sid_list": sid_list}


def scramble(g, seed, extra=37):
    """BFS arrays of a golden file (parent, count, mean, meanSq, sid_ptr, sid_list) -> slot
    arrays under a random slot numbering, with `extra` slots that are not in the tree mixed
    in: half marked removed (parent -2, junk statistics), half unused (parent -1, empty).
    -> dict: parent int32, child_ptr, child_idx, root, count, mean, meanSq, slot_of_sentence
    int32 [n_sent], slot_sids {slot: ids in the golden's order}."""
    rng = np.random.default_rng(seed)
    gp = np.asarray(g["parent"], np.int64)
    Nn, D = g["mean"].shape
    S = Nn + extra
    slot = rng.permutation(S)[:Nn]            # BFS node -> slot
    parent = np.full(S, -1, np.int32)
    dead = np.setdiff1d(np.arange(S), slot)
    parent[dead[::2]] = -2
    count = np.zeros(S, F32)
    mean = np.zeros((S, D), F32)
    m2 = np.zeros((S, D), F32)
    junk = dead[::2]
    count[junk] = 3
    mean[junk] = rng.standard_normal((len(junk), D)).astype(F32)
    m2[junk] = rng.random((len(junk), D)).astype(F32)
    count[slot], mean[slot], m2[slot] = g["count"], g["mean"], g["meanSq"]
    parent[slot[1:]] = slot[gp[1:]]
    kids = [[] for _ in range(S)]
    for i in range(1, Nn):                    # BFS order keeps every child list in list order
        kids[slot[gp[i]]].append(int(slot[i]))
    child_ptr = np.concatenate([[0], np.cumsum([len(k) for k in kids])]).astype(np.int32)
    child_idx = np.asarray([c for k in kids for c in k], np.int32)
    n_sent = int(g["n_sent"])
    sos = np.full(n_sent, -1, np.int32)
    slot_sids = {}
    for i in range(Nn):
        ids = [int(v) for v in g["sid_list"][g["sid_ptr"][i]:g["sid_ptr"][i + 1]]]
        if ids:
            slot_sids[int(slot[i])] = ids
            sos[ids] = slot[i]
    return {"parent": parent, "child_ptr": child_ptr, "child_idx": child_idx, "root": int(slot[0]), "count": count,
            "mean": mean, "meanSq": m2, "slot_of_sentence": sos, "slot_sids": slot_sids, "n_sent": n_sent}
