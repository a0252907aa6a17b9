"""A concept tree that stays on the GPU between adds and queries.

`ResidentTree` owns one `cwq_fit` handle (include/cobweb_query.h) for its lifetime:
`add(X)` runs the device insert loop (cwq_fitdev.hip) on the live tree -- the random()
state goes up before and comes back after (cwq_fit_set_rng / cwq_fit_get_rng), a full pool
is grown in place (cwq_fit_grow) -- and `build_index()` makes the query index from the handle
on the device (cwq_index_create_from_fit, cwq_fitindex.hip).  Nothing that scales with the
tree passes through the host between the two: the CobwebWrapper.add_sentences ->
cobweb_predict* cycle (CobwebWrapper.py:52-89) costs the insert kernel plus a flatten at
memory speed, where the default path flattens, uploads, exports and re-flattens every node
around each batch (fit.py DeviceTreeFitter, tree.py CobwebTree.flatten).

Nodes are named by their SLOT, which never changes while the handle lives (growth keeps
slot numbers; a node removed by a split keeps its slot, unused).  Sentence ids are kept per
slot on the host (`leaf_sids`), because the reference's Basic query shuffles a retrieved
leaf's list in place (CobwebWrapper.py:456) and a later exact-match add appends to the
shuffled list: the lists must outlive every index rebuild.

`ResidentCobwebWrapper` is `CobwebWrapper(..., resident=True)`.
"""
import ctypes
import random as _random_mod
import time

import numpy as np
import torch

from ._lib import CWQ_ERR_OOM, lib
from .fit import _MAX_DEVICE_DIM, _ROOM, DeviceTreeFitter, _np_ptr
from .index import CobwebIndex
from .tree import PRIOR_VAR, CobwebTree, Node
from .wrapper import CobwebWrapper

F32 = np.float32
_ROOM_SLOTS = 64      # cwq_fit_insert stops for room with fewer free slots than this


class ResidentGrowError(RuntimeError):
    """The pool could not grow in the middle of `ResidentTree.add`.  The tree is whole and
    usable: the rows before the stop are in it, `ids` are the sentence ids they got."""

    def __init__(self, msg, ids):
        super().__init__(msg)
        self.ids = ids


class ResidentTree:
    def __init__(self, dim, prior_var=None, device=None, rng=_random_mod, cap_nodes=None):
        dim = int(dim)
        if not 0 < dim <= _MAX_DEVICE_DIM:
            raise ValueError(f"ResidentTree supports 0 < dim <= {_MAX_DEVICE_DIM}")
        self.dim = dim
        self.prior_var = F32(PRIOR_VAR if prior_var is None else prior_var)
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.rng = rng if rng is not None else _random_mod
        self._L = lib()
        self._h = None
        self._broken = None
        self.n_sent = 0
        self.leaf_sids = {}          # slot -> sentence ids, in the order the reference's list has them
        self._sos = torch.full((1024,), -1, dtype=torch.int32, device=self.dev)   # slot of every sentence
        self._stats = {"rows": 0, "kernel_s": 0.0, "grows": 0, "flatten_s": 0.0, "index_build_s": 0.0}
        self._budget = DeviceTreeFitter(CobwebTree((dim,), self.prior_var), device=self.dev)
        self._create(int(cap_nodes) if cap_nodes else self._budget._pool_cap(1, 0))
        z = np.zeros((1, dim), F32)
        self._load(np.array([-1], np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, F32), z, z)

    # ---- handle ----
    def _sp(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _err(self, rc, call):
        return RuntimeError(f"{call} failed (status {rc}): {self._L.cwq_fit_last_error().decode(errors='replace')}")

    def _create(self, cap):
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            rc = self._L.cwq_fit_create(self.dev.index, self.dim, float(self.prior_var), int(cap), ctypes.byref(h))
        if rc:
            raise self._err(rc, "cwq_fit_create")
        self._h = h

    def _mt(self):
        return np.ascontiguousarray(np.asarray(self.rng.getstate()[1], np.uint32))   # 624 words + index

    def _load(self, parent, cptr, cidx, count, mean, m2, root=0):
        with torch.cuda.device(self.dev):
            rc = self._L.cwq_fit_load(self._h, len(parent), int(root), _np_ptr(parent), _np_ptr(cptr), _np_ptr(cidx),
                                      _np_ptr(count), _np_ptr(mean), _np_ptr(m2), _np_ptr(self._mt()), self._sp())
        if rc:
            raise self._err(rc, "cwq_fit_load")

    def _usable(self):
        if self._h is None:
            raise RuntimeError("the resident tree is closed")
        if self._broken:
            raise RuntimeError(f"the resident tree is unusable after a failed insert: {self._broken}")

    def _info(self):
        o = np.zeros(8, np.int64)
        with torch.cuda.device(self.dev):
            rc = self._L.cwq_fit_info(self._h, _np_ptr(o), self._sp())
        if rc:
            raise self._err(rc, "cwq_fit_info")
        return {"cap": int(o[0]), "used": int(o[1]), "root": int(o[2]), "removed": int(o[3]),
                "arena_top": int(o[4]), "arena_cap": int(o[5])}

    @property
    def stats(self):
        """rows inserted, insert-kernel seconds, pool grows, slots in use / removed by splits,
        seconds in flatten() and in build_index() (each cumulative)."""
        out = dict(self._stats)
        out["kernel_s"] = round(out["kernel_s"], 4)
        if self._h is not None and not self._broken:
            i = self._info()
            out.update(slots_in_use=i["used"], removed_slots=i["removed"], cap_nodes=i["cap"])
        return out

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._L.cwq_fit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- add ----
    def _grow(self, used):
        """Double the pool (capped by DeviceTreeFitter._pool_cap's free-memory budget)."""
        cap = self._info()["cap"]
        limit = self._budget._pool_cap(used, 1 << 28)
        new_cap = min(2 * cap, limit)
        if new_cap < used + 2 * _ROOM_SLOTS or new_cap <= cap:
            raise RuntimeError(f"the node pool cannot grow beyond {cap} slots within the device-memory budget")
        with torch.cuda.device(self.dev):
            rc = self._L.cwq_fit_grow(self._h, int(new_cap), self._sp())
        if rc:
            raise self._err(rc, "cwq_fit_grow")
        self._stats["grows"] += 1

    def _commit(self, leaf, k):
        """Rows 0..k-1 of the batch are in the tree: hand the random() state back, give them
        the next sentence ids and record their leaf slots."""
        L = self._L
        mt = np.zeros(625, np.uint32)
        with torch.cuda.device(self.dev):
            rc = L.cwq_fit_get_rng(self._h, _np_ptr(mt), self._sp())
        if rc:
            raise self._err(rc, "cwq_fit_get_rng")
        old = self.rng.getstate()
        self.rng.setstate((old[0], tuple(int(v) for v in mt), old[2]))
        start = self.n_sent
        if start + k > self._sos.numel():
            grown = torch.full((max(2 * self._sos.numel(), start + k),), -1, dtype=torch.int32, device=self.dev)
            grown[:start] = self._sos[:start]
            self._sos = grown
        self._sos[start:start + k] = leaf[:k]
        for i, s in enumerate(leaf[:k].cpu().tolist()):
            self.leaf_sids.setdefault(s, []).append(start + i)
        self.n_sent = start + k
        self._stats["rows"] += k
        return list(range(start, start + k))

    def add(self, X):
        """Insert the rows of X in order (CobwebTorchTree.ifit per row); returns their
        sentence ids.  The pool grows in place when the insert stops for room."""
        self._usable()
        L = self._L
        X = torch.as_tensor(X if torch.is_tensor(X) else np.asarray(X, F32), dtype=torch.float32)
        X = X.to(self.dev).reshape(-1, self.dim).contiguous()
        n = int(X.shape[0])
        if n == 0:
            return []
        leaf = torch.full((n,), -1, dtype=torch.int32, device=self.dev)
        info = np.zeros(4, np.int64)
        with torch.cuda.device(self.dev):
            sp = self._sp()
            rc = L.cwq_fit_set_rng(self._h, _np_ptr(self._mt()), sp) or L.cwq_fit_rewind(self._h, sp)
            if rc:
                raise self._err(rc, "cwq_fit_set_rng")
            done, stalled = 0, False
            while True:
                t0 = time.perf_counter()
                rc = L.cwq_fit_insert(self._h, ctypes.c_void_p(X.data_ptr()), n, ctypes.c_void_p(leaf.data_ptr()),
                                      _np_ptr(info), sp)
                self._stats["kernel_s"] += time.perf_counter() - t0
                if rc:
                    err = self._err(rc, "cwq_fit_insert")
                    if rc == CWQ_ERR_OOM:     # the device tree stopped inside an operation
                        self._broken = str(err)
                    raise err
                k = int(info[0])
                if int(info[2]) != _ROOM:
                    if k != n:
                        raise RuntimeError(f"device fit stopped after {k} of {n} rows (status {int(info[2])})")
                    break
                if k == done and stalled:
                    self._commit(leaf, k)
                    raise RuntimeError("device fit made no progress after the pool grew")
                stalled = k == done
                done = k
                try:
                    self._grow(int(info[3]))
                except RuntimeError as e:
                    raise ResidentGrowError(str(e), self._commit(leaf, k)) from e
        return self._commit(leaf, n)

    # ---- index, flatten ----
    def build_index(self, level_weights=None):
        self._usable()
        t0 = time.perf_counter()
        ix = CobwebIndex.from_fit(self._h, self._sos[:self.n_sent], level_weights, device=self.dev)
        self._stats["index_build_s"] += time.perf_counter() - t0
        return ix

    def flatten(self, stats=True):
        """cwq_fit_flatten's arrays as device tensors: mean [Nn, D], count [Nn], var_row [Nn], an_nodes
        [n_an], an_var [n_an, D], parent [Nn], node_of_sentence [n_sent], slot_of_node [Nn],
        and depth (levels below the root).  stats=False: the integer structure only."""
        self._usable()
        L = self._L
        fl = ctypes.c_void_p()
        sos = self._sos[:self.n_sent]
        t0 = time.perf_counter()
        with torch.cuda.device(self.dev):
            sp = self._sp()
            rc = L.cwq_fit_flatten(self._h, ctypes.c_void_p(sos.data_ptr()) if self.n_sent else None, self.n_sent,
                                   sp, ctypes.byref(fl))
            if rc:
                raise self._err(rc, "cwq_fit_flatten")
            self._stats["flatten_s"] += time.perf_counter() - t0
            try:
                o = np.zeros(8, np.int64)
                L.cwq_fit_flat_info(fl, _np_ptr(o))
                Nn, na, D = int(o[0]), int(o[1]), self.dim
                kw = {"device": self.dev}
                out = {"parent": torch.empty(Nn, dtype=torch.int64, **kw),
                       "node_of_sentence": torch.empty(self.n_sent, dtype=torch.int64, **kw),
                       "slot_of_node": torch.empty(Nn, dtype=torch.int32, **kw)}
                if stats:
                    out.update(mean=torch.empty((Nn, D), dtype=torch.float32, **kw),
                               count=torch.empty(Nn, dtype=torch.float32, **kw),
                               var_row=torch.empty(Nn, dtype=torch.float32, **kw),
                               an_nodes=torch.empty(na, dtype=torch.int64, **kw),
                               an_var=torch.empty((na, D), dtype=torch.float32, **kw))

                def p(name):
                    t = out.get(name)
                    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
                rc = L.cwq_fit_flat_copy(fl, p("mean"), p("count"), p("var_row"), p("an_nodes"), p("an_var"), p("parent"),
                                         p("node_of_sentence"), p("slot_of_node"), sp)
                if rc:
                    raise self._err(rc, "cwq_fit_flat_copy")
                out["depth"] = int(o[4])
                out["device_bytes"] = int(o[6])
            finally:
                L.cwq_fit_flat_destroy(fl)
        return out

    # ---- host tree in and out ----
    def to_tree(self, return_slots=False):
        """The tree as a host CobwebTree (cwq_fit_export), every leaf's sentence_id being this
        object's own per-slot list.  return_slots: also the slot -> Node list."""
        self._usable()
        used = self._info()["used"]
        D = self.dim
        out2 = np.zeros(2, np.int32)
        P = np.zeros(used, np.int32)
        CP = np.zeros(used + 1, np.int32)
        CI = np.zeros(max(used, 1), np.int32)
        CNT = np.zeros(used, F32)
        MEAN = np.zeros((used, D), F32)
        M2 = np.zeros((used, D), F32)
        mt = np.zeros(625, np.uint32)
        with torch.cuda.device(self.dev):
            rc = self._L.cwq_fit_export(self._h, _np_ptr(out2), _np_ptr(P), _np_ptr(CP), _np_ptr(CI), _np_ptr(CNT),
                                        _np_ptr(MEAN), _np_ptr(M2), _np_ptr(mt), self._sp())
        if rc:
            raise self._err(rc, "cwq_fit_export")
        objs = [Node(D) if P[i] != -2 else None for i in range(used)]
        for i, o in enumerate(objs):
            if o is None:
                continue
            o.count = F32(CNT[i])
            o.mean = MEAN[i]
            o.meanSq = M2[i]
            o.parent = objs[P[i]] if P[i] >= 0 else None
            o.children = [objs[c] for c in CI[CP[i]:CP[i + 1]]]
            ids = self.leaf_sids.get(i)
            o.sentence_id = ids if ids is not None else []
        t = CobwebTree((D,), self.prior_var)
        t.root = objs[int(out2[1])]
        return (t, objs) if return_slots else t

    @classmethod
    def from_slots(cls, parent, child_ptr, child_idx, count, mean, meanSq, root, slot_sids, n_sentences,
                   prior_var=None, device=None, rng=_random_mod, cap_nodes=None):
        """Load slot arrays as cwq_fit_load takes them (parent -1 at the root, -2 for a slot
        that is not in the tree; children as CSR in list order) with the sentence ids of every
        slot (`slot_sids`: slot -> list)."""
        mean = np.ascontiguousarray(mean, F32)
        self = cls.__new__(cls)
        ResidentTree.__init__(self, mean.shape[1], prior_var, device, rng,
                              cap_nodes if cap_nodes else len(parent) + 1024)
        self._load(np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(child_ptr, np.int32),
                   np.ascontiguousarray(child_idx if len(child_idx) else [0], np.int32),
                   np.ascontiguousarray(count, F32), mean, np.ascontiguousarray(meanSq, F32), root)
        self._place(slot_sids, n_sentences)
        return self

    def _place(self, slot_sids, n_sentences):
        top = -1
        for s, ids in slot_sids.items():
            if len(ids):
                self.leaf_sids[int(s)] = [int(v) for v in ids]
                top = max(top, max(self.leaf_sids[int(s)]))
        self.n_sent = top + 1 if n_sentences is None else int(n_sentences)
        sos = np.full(max(self.n_sent, 1), -1, np.int32)
        for s, ids in self.leaf_sids.items():
            for v in ids:
                if 0 <= v < self.n_sent:
                    sos[v] = s
        self._sos = torch.from_numpy(sos).to(self.dev)

    @classmethod
    def from_tree(cls, tree, n_sentences=None, device=None, rng=_random_mod, cap_nodes=None):
        """Load a host CobwebTree (cwq_fit_load; slots = DFS preorder).  Sentence ids come
        from the nodes' sentence_id lists, kept in their order; ids >= n_sentences (default:
        the largest id + 1) stay in the lists but are not in the index, as in
        CobwebTree.flatten."""
        fitter = DeviceTreeFitter(tree, device=device)
        nodes, parent, cptr, cidx, count, mean, m2 = fitter._flatten()
        self = cls.__new__(cls)
        ResidentTree.__init__(self, tree.dim, tree.prior_var, device, rng,
                              cap_nodes if cap_nodes else fitter._pool_cap(len(nodes), 0))
        if self._info()["cap"] < len(nodes):
            raise RuntimeError(f"cap_nodes {self._info()['cap']} is below the tree's {len(nodes)} nodes")
        self._load(parent, cptr, cidx, count, mean, m2)
        self._place({s: nd.sentence_id for s, nd in enumerate(nodes) if nd.sentence_id}, n_sentences)
        return self


class _SlotSentences:
    """`wrapper._nodes` without host nodes: [BFS node id] -> an object whose sentence_id is the
    resident tree's per-slot list (shared, so Basic's in-place shuffle persists)."""

    class _Ref:
        __slots__ = ("sentence_id",)

        def __init__(self, ids):
            self.sentence_id = ids

    def __init__(self, rt, slot_of_node):
        self._rt = rt
        self._son = slot_of_node     # device [Nn] int32

    def __len__(self):
        return int(self._son.numel())

    def __getitem__(self, i):
        ids = self._rt.leaf_sids.get(int(self._son[int(i)]))
        return self._Ref(ids if ids is not None else [])


class _LazyPaths:
    """`wrapper._leaf_to_path_indices`: one root-to-node BFS index path per sentence (None for
    a sentence outside the tree), made from the integer structure on first item access."""

    def __init__(self, wrapper, n):
        self._w = wrapper
        self._n = n
        self._paths = None

    def __len__(self):
        return self._n

    def _make(self):
        if self._paths is None:
            st = self._w._structure()
            par = st["parent"].cpu().numpy()
            paths = []
            for s in st["node_of_sentence"].cpu().numpy():
                path, j = [], int(s)
                while j >= 0:
                    path.append(j)
                    j = int(par[j])
                paths.append(path[::-1] if s >= 0 else None)
            self._paths = paths
        return self._paths

    def __getitem__(self, i):
        return self._make()[i]

    def __iter__(self):
        return iter(self._make())


class ResidentCobwebWrapper(CobwebWrapper):
    """CobwebWrapper(..., resident=True): the same interface and the same results, with the
    tree in a ResidentTree.  The host Node tree (`tree`, `sentence_to_node`, node statistics
    behind `_nodes`) exists only while something reads it -- dump_json, save_binary,
    get_node_path_stats, print_tree, or the attributes themselves -- and is dropped by the
    next add."""

    _rt = None          # the ResidentTree (made by the first add or by _adopt)
    _host = None        # (CobwebTree, slot -> Node, sentence id -> Node) while materialised
    _struct = None      # device parent / node_of_sentence / slot_of_node of the current tree
    _paths = None
    _shape = None

    # ---- the host views, made on demand ----
    def _materialise(self):
        if self._host is None and self._rt is not None:
            tree, objs = self._rt.to_tree(return_slots=True)
            s2n = {}
            for slot, ids in self._rt.leaf_sids.items():
                for s in ids:
                    s2n[s] = objs[slot]
            self._host = (tree, objs, s2n)
        return self._host

    def _structure(self):
        if self._struct is None:
            self._struct = self._rt.flatten(stats=False)
        return self._struct

    @property
    def tree(self):
        if self._rt is None:
            return CobwebTree(self._shape) if self._shape is not None else None
        return self._materialise()[0]

    @tree.setter
    def tree(self, value):
        if value is not None and self._rt is None:
            self._shape = tuple(value.shape)

    @property
    def sentence_to_node(self):
        return self._materialise()[2] if self._rt is not None else {}

    @sentence_to_node.setter
    def sentence_to_node(self, value):
        pass

    @property
    def _nodes(self):
        if self._rt is None or not self._prediction_index_valid:
            return None
        st = self._structure()
        if self._host is not None:      # host nodes in BFS order (their sentence_id: the same lists)
            if "host_nodes" not in st:
                objs = self._host[1]
                st["host_nodes"] = [objs[s] for s in st["slot_of_node"].cpu().tolist()]
            return st["host_nodes"]
        return _SlotSentences(self._rt, st["slot_of_node"])

    @_nodes.setter
    def _nodes(self, value):
        pass

    @property
    def _leaf_to_path_indices(self):
        return self._paths if self._prediction_index_valid else None

    @_leaf_to_path_indices.setter
    def _leaf_to_path_indices(self, value):
        self._paths = None

    # ---- add, index ----
    def add_sentences(self, new_sentences, new_vectors=None):
        """CobwebWrapper.py:52-80 through ResidentTree.add."""
        if new_vectors is None:
            new_embeddings = np.asarray(self.encode_func(new_sentences), dtype=np.float32)
        else:
            new_embeddings = new_vectors
            if isinstance(new_embeddings, list):
                new_embeddings = np.asarray(new_embeddings, dtype=np.float32)
            dim = self._rt.dim if self._rt is not None else (self._shape[0] if self._shape else None)
            if dim is not None and new_embeddings.shape[1] != dim:
                print(f"[Warning] Provided vector dim {new_embeddings.shape[1]} != tree dim "
                      f"{dim}, re-encoding...")
                new_embeddings = np.asarray(self.encode_func(new_sentences), dtype=np.float32)
        X = new_embeddings.detach().to(torch.float32) if torch.is_tensor(new_embeddings) else np.asarray(
            new_embeddings, dtype=np.float32)
        n = len(new_sentences)
        if self._rt is None:
            self._shape = tuple(X.shape[1:])
            self._rt = ResidentTree(X.shape[1], device=self.device)
        self._host = None
        self._struct = None
        self._invalidate_prediction_index()
        try:
            ids = self._rt.add(X[:n])
        except ResidentGrowError as e:
            self.sentences.extend(new_sentences[:len(e.ids)])
            raise
        assert ids == list(range(len(self.sentences), len(self.sentences) + n))
        self.sentences.extend(new_sentences)
        self.last_fit_stats = self._rt.stats

    def build_prediction_index(self):
        """CobwebWrapper.py:91-208 on the device (cwq_index_create_from_fit)."""
        if self._prediction_index_valid:
            return
        if self._rt is None:
            raise ValueError("the tree is empty: add sentences first")
        weights = list(self._level_weights) if self._level_weights is not None else [1.0] * 6
        self._index = self._rt.build_index(weights)
        self._paths = _LazyPaths(self, self._index.n_sent)
        if self._index.n_sent:
            # every leaf of an ifit-built tree holds a sentence: the deepest sentence's path
            self.max_depth = max(self.max_depth, self._index.info["max_depth"] + 1)
        self._prediction_index_valid = True

    def get_prediction_index_info(self):
        info = super().get_prediction_index_info()
        if self._prediction_index_valid:
            info["total_nodes"] = self._index.n_nodes
        return info

    def get_node_path_stats(self, sentence_id):
        """CobwebWrapper.py:297-313 (reads the materialised host nodes)."""
        self.build_prediction_index()
        self._materialise()
        return super().get_node_path_stats(sentence_id)

    def print_tree(self, max_depth=3):
        """The top of the tree, one line per node (materialises the host tree)."""
        stack = [(self.tree.root, 0)]
        while stack:
            n, d = stack.pop()
            print("  " * d + f"count={float(n.count):g} children={len(n.children)} sentences={len(n.sentence_id)}")
            if d < max_depth:
                stack.extend((c, d + 1) for c in reversed(n.children))

    @property
    def resident_tree(self):
        return self._rt

    @classmethod
    def _adopt(cls, w):
        """A resident wrapper over the host tree of the default wrapper `w` (the loaders)."""
        r = cls(encode_func=w.encode_func, device=w.device, resident=True)
        r.sentences = w.sentences
        r.max_init_search = w.max_init_search
        if w.tree is not None:
            r._shape = tuple(w.tree.shape)
            r._rt = ResidentTree.from_tree(w.tree, n_sentences=len(w.sentences), device=w.device)
        return r
