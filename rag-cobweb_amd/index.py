"""Device-resident Cobweb query index: a thin Python handle over libcwq.

`CobwebIndex` owns one `cwq_index*` (include/cobweb_query.h).  It is the MI355X
replacement of the flattened prediction index the reference caches in
CobwebWrapper.build_prediction_index (CobwebWrapper.py:91-208) and of the query
op sequences that read it (:210-294, CobwebTorchTree.py:235-310).

Inputs/outputs are torch tensors on the index device; torch only supplies device
memory and the current HIP stream -- every computation runs in libcwq.
"""
import ctypes

import numpy as np
import torch

from ._lib import check, lib

DEFAULT_LEVEL_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)   # CobwebWrapper.py:155


def _dev(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"CobwebIndex lives on a GPU, got device {device}")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_raw(index):
    """torch's current HIP stream on device `index` as an int (the per-call path: no
    Stream object, no device switch -- libcwq sets its device itself)."""
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class CompactVar:
    """Node variances in compact form (cwq_index_create_cv): `row[i]` is node i's variance
    in every dimension -- every count-1 leaf has var = prior_var exactly
    (CobwebTorchTree.py:336-342) -- except for the nodes `an_nodes` (int64, ascending),
    whose full rows are `an_var` [n_an, D].  A flat 10M x 1024 tree's variances are 40 MB
    this way instead of 41 GB."""

    def __init__(self, row, an_nodes, an_var):
        self.row = row
        self.an_nodes = an_nodes
        self.an_var = an_var

    @property
    def shape(self):
        return (int(self.row.shape[0]), int(self.an_var.shape[1]))

    @classmethod
    def from_full(cls, var):
        """Compress a full [Nn, D] variance tensor (bitwise: a row counts as one value
        only when all D values have the same bits)."""
        var = torch.as_tensor(var, dtype=torch.float32)
        bits = var.view(torch.int32)
        iso = (bits == bits[:, :1]).all(1)
        an = torch.nonzero(~iso).squeeze(1).to(torch.int64)
        return cls(var[:, 0].contiguous(), an, var[an].contiguous())

    def full(self):
        """The [Nn, D] array it stands for (tests / small trees)."""
        n, d = self.shape
        out = self.row[:, None].expand(n, d).clone()
        if self.an_nodes.numel():
            out[self.an_nodes.to(out.device)] = self.an_var.to(out.device)
        return out

    def __getitem__(self, i):   # one node's variance row (bench's root var, small reads)
        i = int(i)
        hit = (self.an_nodes == i).nonzero()
        if hit.numel():
            return self.an_var[int(hit[0, 0])]
        return self.row[i].expand(self.shape[1])


def pack_sentence_bits(allowed, n_sent):
    """The bitset cwq_mask_create reads, as an int32 tensor of ceil(n_sent / 32) words on the
    device `allowed` is on (the CPU for arrays and lists): bit (s % 32) of word (s // 32), least
    significant bit first, set = sentence s is allowed (numpy.packbits(..., bitorder="little")
    read as little-endian uint32).  `allowed`: a bool tensor / ndarray / list of length n_sent,
    or an integer tensor / ndarray / list of sentence ids (duplicates are fine).  ValueError for
    a bool mask of another length and for an id outside [0, n_sent)."""
    n_sent = int(n_sent)
    if not torch.is_tensor(allowed):
        a = np.asarray(allowed)
        if a.size == 0 and a.dtype != np.bool_:
            a = a.astype(np.int64)
        allowed = torch.from_numpy(np.ascontiguousarray(a))
    a = allowed.detach().reshape(-1)
    if a.dtype == torch.bool:
        if a.numel() != n_sent:
            raise ValueError(f"a bool mask must have one entry per sentence: got {a.numel()}, the index has {n_sent}")
        flags = a
    elif a.dtype.is_floating_point or a.dtype.is_complex:
        raise ValueError("allowed must be a bool mask or integer sentence ids")
    else:
        ids = a.to(torch.int64)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_sent):
            raise ValueError(f"sentence ids must be in [0, {n_sent})")
        flags = torch.zeros(n_sent, dtype=torch.bool, device=ids.device)
        flags[ids] = True
    words = (n_sent + 31) // 32
    pad = torch.zeros(words * 32, dtype=torch.int64, device=flags.device)
    pad[:n_sent] = flags
    w = (pad.view(words, 32) << torch.arange(32, dtype=torch.int64, device=flags.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


class SentenceMask:
    """An allowed-sentence set of one CobwebIndex (a cwq_mask handle; no reference counterpart):
    made by CobwebIndex.sentence_mask, passed to score_topk(mask=...), reusable across calls and
    streams.  It keeps its index alive (an index closed meanwhile is destroyed when the last of
    its masks is).  info: allowed sentences that are in the tree, live isotropic / anisotropic
    rows, device bytes."""

    def __init__(self, index, allowed):
        self._h = ctypes.c_void_p()
        self._index = None
        bits = pack_sentence_bits(allowed, index.n_sent).to(index.device).contiguous()
        h = ctypes.c_void_p()
        with torch.cuda.device(index.device):
            check(index._L.cwq_mask_create(index._h, _ptr(bits) if bits.numel() else None, index.n_sent,
                                           _stream(index.device), ctypes.byref(h)))
        self._h = h
        self._index = index
        index._pin()
        out = np.zeros(4, np.int64)
        check(index._L.cwq_mask_info(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        self.info = dict(zip(["allowed", "live_iso_rows", "live_aniso_rows", "device_bytes"], (int(v) for v in out)))

    @property
    def closed(self):
        return not (self._h and self._h.value)

    def close(self):
        if not self.closed:
            self._index._L.cwq_mask_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._index._unpin()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CobwebIndex:
    """Immutable flattened tree on one GPU.

    mean               [Nn, D] float32 (torch on any device, or numpy), BFS order
    var                [Nn, D] float32, or a CompactVar (one scalar per node with full rows
                       only where the D variances differ)
    parent             [Nn] int64, parent[0] = -1, non-decreasing (BFS)
    node_of_sentence   [n_sent] int64, node holding each sentence id (-1: none)
    level_weights      per-depth weights (CobwebWrapper.py:153-168)
    """

    def __init__(self, mean, var, parent, node_of_sentence, level_weights=None, device=None):
        self.device = _dev(device)
        L = self._L = lib()   # the handle belongs to the library that created it
        mean = torch.as_tensor(mean, dtype=torch.float32).to(self.device).contiguous()
        compact = isinstance(var, CompactVar)
        if compact:
            vrow = torch.as_tensor(var.row, dtype=torch.float32).to(self.device).contiguous()
            an_nodes = np.ascontiguousarray(np.asarray(torch.as_tensor(var.an_nodes).cpu(), dtype=np.int64))
            an_var = torch.as_tensor(var.an_var, dtype=torch.float32).to(self.device).contiguous()
            if (mean.dim() != 2 or vrow.shape != (mean.shape[0],) or an_var.dim() != 2
                    or an_var.shape != (an_nodes.size, mean.shape[1])):
                raise ValueError("compact var: row [n_nodes], an_var [n_an, dim] for mean [n_nodes, dim]")
        else:
            var = torch.as_tensor(var, dtype=torch.float32).to(self.device).contiguous()
            if mean.shape != var.shape or mean.dim() != 2:
                raise ValueError("mean and var must both be [n_nodes, dim]")
        parent = np.ascontiguousarray(np.asarray(parent, dtype=np.int64))
        nos = np.ascontiguousarray(np.asarray(node_of_sentence, dtype=np.int64))
        w = np.ascontiguousarray(np.asarray(
            DEFAULT_LEVEL_WEIGHTS if level_weights is None else level_weights, dtype=np.float64))
        self.n_nodes, self.dim = mean.shape
        self.n_sent = int(nos.size)
        self.level_weights = [float(x) for x in w]
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            if compact:
                check(L.cwq_index_create_cv(self.device.index, self.n_nodes, self.dim, _ptr(mean), _ptr(vrow),
                                            an_nodes.ctypes.data_as(ctypes.c_void_p), an_nodes.size, _ptr(an_var),
                                            parent.ctypes.data_as(ctypes.c_void_p),
                                            nos.ctypes.data_as(ctypes.c_void_p), self.n_sent,
                                            w.ctypes.data_as(ctypes.c_void_p), w.size, _stream(self.device),
                                            ctypes.byref(h)))
            else:
                check(L.cwq_index_create(self.device.index, self.n_nodes, self.dim, _ptr(mean), _ptr(var),
                                         parent.ctypes.data_as(ctypes.c_void_p), nos.ctypes.data_as(ctypes.c_void_p),
                                         self.n_sent, w.ctypes.data_as(ctypes.c_void_p), w.size,
                                         _stream(self.device), ctypes.byref(h)))
        self._h = h
        self.info = self._info()

    @classmethod
    def from_fit(cls, fit, slot_of_sentence, level_weights=None, device=None):
        """The index of a device-resident tree (a cwq_fit handle, resident.ResidentTree)
        built on the device (cwq_index_create_from_fit): `slot_of_sentence` [n_sent] int32 on
        the device holds each sentence's slot (-1: not in the tree).  Same index as
        CobwebIndex(mean, var, parent, node_of_sentence) of the flattened tree; only the
        integer structure passes through the host."""
        self = cls.__new__(cls)
        self.device = _dev(device)
        L = self._L = lib()
        sos = torch.as_tensor(slot_of_sentence, dtype=torch.int32).to(self.device).contiguous()
        w = np.ascontiguousarray(np.asarray(
            DEFAULT_LEVEL_WEIGHTS if level_weights is None else level_weights, dtype=np.float64))
        self.level_weights = [float(x) for x in w]
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(L.cwq_index_create_from_fit(fit, _ptr(sos) if sos.numel() else None, int(sos.numel()),
                                              w.ctypes.data_as(ctypes.c_void_p), w.size, _stream(self.device),
                                              ctypes.byref(h)))
        self._h = h
        self.info = self._info()
        self.n_nodes, self.dim, self.n_sent = self.info["n_nodes"], self.info["dim"], self.info["n_sent"]
        return self

    def _info(self):
        out = np.zeros(8, np.int64)
        check(self._L.cwq_index_info(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        keys = ["n_nodes", "dim", "n_sent", "internal_nodes", "leaf_rows", "isotropic_rows", "max_depth",
                "device_bytes"]
        return dict(zip(keys, (int(v) for v in out)))

    def filter_info(self):
        """How the filters centre their rows (cwq_index_filter_info): group-centred rows on
        clustered trees, the number of groups / group-centred rows, the int8 panel, the hub
        rows of the batch filter's threshold sample (of last_stats()["sample_rows"]), the batch
        filter's launch schedule on this index by the default rules ("bf16", "quarter", "early"
        or "direct") and whether the last Fast batch call ran the direct schedule."""
        out = np.zeros(7, np.int64)
        check(self._L.cwq_index_filter_info(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"group_centred": bool(out[0]), "groups": int(out[1]), "group_rows": int(out[2]),
                "int8_panel": bool(out[3]), "sample_hub_rows": int(out[4]),
                "schedule": ("bf16", "quarter", "early", "direct")[int(out[5])], "direct_last_call": bool(out[6])}

    def cut_info(self):
        """The tree-adaptive cut (cwq_index_cut_info): groups, top nodes (computed exactly by
        every pruned query), the deepest centre, groups whose rows are centred."""
        out = np.zeros(4, np.int64)
        check(self._L.cwq_index_cut_info(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"groups": int(out[0]), "top_nodes": int(out[1]), "max_centre_depth": int(out[2]),
                "centred_groups": int(out[3])}

    def set_timing(self, enable=True):
        check(self._L.cwq_set_timing(self._h, int(bool(enable))))

    def last_timing(self):
        """Phase times (ms) of the last score_topk call, from HIP events on its stream."""
        out = np.zeros(8, np.float32)
        check(self._L.cwq_last_timing(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"leaf_scan_ms": float(out[0]), "internal_ms": float(out[1]), "merge_ms": float(out[2]),
                "call_ms": float(out[3]), "leaf_scan_launches": int(out[4]), "sample_ms": float(out[5]),
                "fgemm_ms": float(out[6]), "rerank_ms": float(out[7])}

    def set_filter(self, mode):
        """Isotropic-row strategy of score_topk: -1 automatic, 0 exact fp32 scan,
        1 bf16-MFMA candidate filter + exact rerank (k <= 64).  Results are identical."""
        check(self._L.cwq_set_filter(self._h, int(mode)))

    def last_stats(self):
        out = np.zeros(6, np.int64)
        check(self._L.cwq_last_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"filter_queries": int(out[0]), "fallback_queries": int(out[1]), "filter_used": bool(out[2]),
                "path": {0: "scan", 1: "fgemm", 2: "stream"}.get(int(out[2]) & 255, "?"),
                "int8_pass": bool(int(out[2]) & 256),
                "fg_i8_launches": int(out[2]) >> 16,   # batch filter launches on the int8 operands

                "candidates": int(out[3]), "exact_reranks": int(out[4]), "sample_rows": int(out[5])}

    def last_prune_stats(self):
        """Group pruning of the last Fast call (cwq_last_prune_stats): whether the
        index has it, the queries of the pruned chunk (0: not pruned), the (query, group)
        pairs its stage B computed beyond each query's best group, and the group count."""
        out = np.zeros(4, np.int64)
        check(self._L.cwq_last_prune_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"available": bool(out[0]), "queries": int(out[1]), "extra_pairs": int(out[2]), "groups": int(out[3])}

    def last_categorize_stats(self):
        """How the last categorize call resolved its queries (cwq_last_stats after
        cwq_categorize): counting over the bottleneck order, heap replay, the two-level
        replay of lists that end inside a bottleneck tie, DENSE re-runs."""
        out = np.zeros(6, np.int64)
        check(self._L.cwq_last_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"queries": int(out[0]), "dense_reruns": int(out[1]), "filter_reruns": int(out[2]),
                "by_count": int(out[3]), "by_replay": int(out[4]), "two_level": int(out[5])}

    def last_lazy_stats(self):
        """The last categorize call's exact lazy replays (cwq_last_lazy_stats): queries replayed
        straight away (the list paths skipped), and DENSE re-runs done by the lazy replay."""
        out = np.zeros(2, np.int64)
        check(self._L.cwq_last_lazy_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"direct": int(out[0]), "dense_lazy": int(out[1])}

    def close(self):
        """Destroy the device index.  While an autograd graph still holds this index for a
        pending backward (autograd._Pin), the destruction waits for the last such graph."""
        if getattr(self, "_pins", 0) > 0:
            self._close_pending = True
            return
        self._destroy()

    def _destroy(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.cwq_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def _pin(self):
        self._pins = getattr(self, "_pins", 0) + 1

    def _unpin(self):
        self._pins -= 1
        if self._pins == 0 and getattr(self, "_close_pending", False):
            self._close_pending = False
            self._destroy()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # ---- queries ----
    def _queries(self, q):
        q = torch.as_tensor(q, dtype=torch.float32)
        if q.dim() == 1:
            q = q[None, :]
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}]")
        return q.to(self.device).contiguous()

    def sentence_mask(self, allowed):
        """A SentenceMask of this index: `allowed` is a bool tensor / ndarray of length n_sent
        or an integer tensor / list of sentence ids (pack_sentence_bits)."""
        return SentenceMask(self, allowed)

    def last_mask_stats(self):
        """The last score_topk(mask=...) call (cwq_last_mask_stats): the path taken (1 over-fetch,
        2 gathered scan, 3 sort for k > 64), the over-fetch k', the queries the over-fetch left
        short (redone by the gathered scan), the mask's live rows.  After rank_ce(mask=...) the path
        is 5 (full) or 6 (gathered: both streams over the mask's live rows only)."""
        out = np.zeros(4, np.int64)
        check(self._L.cwq_last_mask_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {"path": int(out[0]), "overfetch_k": int(out[1]), "redone_queries": int(out[2]), "live_rows": int(out[3])}

    def last_mask_multi_stats(self):
        """The last score_topk(masks=...) call over more than one distinct mask
        (cwq_last_mask_multi_stats): queries answered by the over-fetch leg, distinct over-fetch
        widths run, queries the over-fetch left short, queries planned straight to the gathered
        scan, gathered-scan kernel launches and work items, distinct masks referenced, queries
        through the k > 64 sort.  A mask that ran as a single-mask call of its own inside the call
         counts its queries by what that call did; the launches and work items are
        the grouped scan's only."""
        out = np.zeros(8, np.int64)
        check(self._L.cwq_last_mask_multi_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        names = ["overfetch_queries", "overfetch_widths", "short_queries", "gathered_queries", "gathered_launches",
                 "gathered_work_items", "masks_referenced", "sort_queries"]
        return dict(zip(names, (int(v) for v in out)))

    def score_topk(self, q, k, mask=None, masks=None, mask_of_query=None):
        """Top-k sentence ids/scores per query ("Cobweb Fast", A6).  One call per query is
        the reference harness's mode (benchmark_utils.py:801-805), so a float32 [nq, dim]
        tensor already on the index device goes straight through: no conversion, no device
        switch (the library selects its device itself), the raw current stream.
        mask (a SentenceMask of this index): the ranking restricted to its allowed sentences --
        the full ranking with the others removed, cut to k, padded with -1 / -inf
        (cwq_score_topk_masked).
        masks (a sequence of open SentenceMasks of this index) with mask_of_query (an int tensor /
        array / list of length nq; a device tensor is copied to the host once): query i is
        restricted to masks[mask_of_query[i]], in one call (cwq_score_topk_masked_multi; each row
        is what the single-mask call returns for it).  Not together with mask=.
        A q that requires grad (with grad enabled) gets scores with autograd history, as
        torch.topk's values have and its indices do not (autograd.TopKScores; the backward is
        cwq_score_pairs_backward over the returned ids); k <= 4096 then, ValueError
        above.  Without grad the call is the one described above."""
        if getattr(q, "requires_grad", False) and torch.is_grad_enabled():
            # values carry the gradient, indices do not (torch.topk); the backward needs only the ids
            from .autograd import topk_scores_autograd
            return topk_scores_autograd(self, q, k, mask, masks, mask_of_query)
        if masks is not None and mask is not None:
            raise ValueError("pass mask= or masks=, not both")
        if (masks is None) != (mask_of_query is None):
            raise ValueError("masks= and mask_of_query= go together")
        if not (type(q) is torch.Tensor and q.dtype == torch.float32 and q.device == self.device and q.dim() == 2
                and q.shape[1] == self.dim and q.is_contiguous()):
            q = self._queries(q)
        nq = q.shape[0]
        k = int(k)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if masks is not None:
            masks = list(masks)
            if not masks or any(not isinstance(m, SentenceMask) or m.closed for m in masks):
                raise ValueError("masks must be a non-empty sequence of open SentenceMasks (CobwebIndex.sentence_mask)")
            moq = mask_of_query.detach().cpu().numpy() if torch.is_tensor(mask_of_query) else np.asarray(mask_of_query)
            if moq.ndim != 1 or moq.shape[0] != nq or moq.dtype.kind not in "iu":
                raise ValueError(f"mask_of_query must be {nq} integers, one per query")
            moq = np.ascontiguousarray(moq.clip(-1, 2 ** 31 - 1), dtype=np.int32)   # out of range stays out of range
            handles = (ctypes.c_void_p * len(masks))(*[m._h.value for m in masks])
            check(self._L.cwq_score_topk_masked_multi(self._h, handles, len(masks), moq.ctypes.data, q.data_ptr(), nq, k,
                                                      ids.data_ptr(), scores.data_ptr(),
                                                      _stream_raw(self.device.index)))
            return ids, scores
        if mask is not None:
            if not isinstance(mask, SentenceMask) or mask.closed:
                raise ValueError("mask must be an open SentenceMask (CobwebIndex.sentence_mask)")
            check(self._L.cwq_score_topk_masked(self._h, mask._h, q.data_ptr(), nq, k, ids.data_ptr(),
                                                scores.data_ptr(), _stream_raw(self.device.index)))
            return ids, scores
        check(self._L.cwq_score_topk(self._h, q.data_ptr(), nq, k, ids.data_ptr(), scores.data_ptr(),
                                     _stream_raw(self.device.index)))
        return ids, scores

    def score_topk_host(self, q, k):
        """score_topk for a host (numpy) query batch -> numpy (ids [nq, k] int64, scores [nq, k]
        float32), the reference harness's call shape (cwq_score_topk_host: pinned staging in,
        the kernels write the results into mapped host memory; no torch tensors per call)."""
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}]")
        nq, k = q.shape[0], int(k)
        ids = np.empty((nq, k), np.int64)
        scores = np.empty((nq, k), np.float32)
        check(self._L.cwq_score_topk_host(self._h, q.ctypes.data, nq, k, ids.ctypes.data, scores.ctypes.data,
                                          _stream_raw(self.device.index)))
        return ids, scores

    def categorize_host(self, q, k, max_nodes=100000):
        """categorize for a host (numpy) query batch -> numpy (nodes [nq, k] int64, found [nq]
        int32, calls [nq] int64): cwq_categorize_host, the harness's Basic call shape (pinned
        staging in, the kernels write the results into mapped host memory)."""
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32))
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}]")
        nq, k = q.shape[0], int(k)
        nodes = np.empty((nq, k), np.int64)
        found = np.empty(nq, np.int32)
        calls = np.empty(nq, np.int64)
        mx = int(min(max_nodes, 2 ** 62)) if max_nodes != float("inf") else 2 ** 62
        check(self._L.cwq_categorize_host(self._h, q.ctypes.data, nq, k, mx, nodes.ctypes.data, found.ctypes.data,
                                          calls.ctypes.data, _stream_raw(self.device.index)))
        return nodes, found, calls

    def _level_weights(self, w):
        """Call-time level weights as a float32 [n_w] tensor on the index device (None: the
        weights baked into the index).  A device tensor goes through without a host read."""
        if w is None:
            return None
        w = torch.as_tensor(w, dtype=torch.float32).detach()
        if w.dim() != 1 or w.shape[0] > 64:
            raise ValueError("level_weights must be a vector of at most 64 values")
        return w.to(self.device).contiguous()

    def rank_scores(self, q, level_weights=None):
        """All sentence scores (A8), [nq, n_sent].  A tensor that requires grad (with grad
        enabled) gets scores with autograd history (autograd.RankScores: the backward is
        cwq_rank_scores_backward); the gradient arrives on q's own device and dtype.
        level_weights [n_w] (a depth >= n_w weighs 1.0): the scores under these level weights
        instead of the index's own, bit for bit those of an index built with them; it may
        require grad too (cwq_rank_scores_w)."""
        if torch.is_grad_enabled() and ((torch.is_tensor(q) and q.requires_grad) or
                                        (torch.is_tensor(level_weights) and level_weights.requires_grad)):
            from .autograd import rank_scores_autograd
            return rank_scores_autograd(self, torch.as_tensor(q), level_weights)
        q = self._queries(q)
        w = self._level_weights(level_weights)
        out = torch.empty((q.shape[0], self.n_sent), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if w is None:
                check(self._L.cwq_rank_scores(self._h, _ptr(q), q.shape[0], _ptr(out), _stream(self.device)))
            elif q.shape[0] > 0:
                check(self._L.cwq_rank_scores_w(self._h, _ptr(q), q.shape[0], _ptr(w) if w.numel() else None,
                                                w.numel(), _ptr(out), _stream(self.device)))
        return out

    def rank_scores_backward(self, q, grad_out, level_weights=None, weight_grad=False, query_grad=True):
        """Gradient of rank_scores with respect to the queries: grad_out [nq, n_sent] (the
        upstream gradient of every score; columns of sentences that are not in the tree are
        never read) -> [nq, dim] float32.  Needs nothing from the forward call; bit-identical
        from run to run and for a query alone or in a batch.
        level_weights: the gradient under these level weights.  weight_grad=True returns
        (grad_q, grad_w) with grad_w [nq, n_w] float32, d(sum grad_out * scores[q]) / d w per
        query (n_w = len(level_weights)); query_grad=False then skips grad_q (None)."""
        q = self._queries(q)
        g = torch.as_tensor(grad_out, dtype=torch.float32)
        if g.dim() == 1:
            g = g[None, :]
        if g.shape != (q.shape[0], self.n_sent):
            raise ValueError(f"grad_out must be [{q.shape[0]}, {self.n_sent}]")
        g = g.to(self.device).contiguous()
        w = self._level_weights(level_weights)
        if weight_grad and w is None:
            raise ValueError("weight_grad needs level_weights (their length sets the gradient's)")
        if not (weight_grad or query_grad):
            raise ValueError("nothing to compute")
        nq = q.shape[0]
        out = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device) if query_grad or not weight_grad else None
        if w is None:
            with torch.cuda.device(self.device):
                check(self._L.cwq_rank_scores_backward(self._h, _ptr(q), nq, _ptr(g), _ptr(out), _stream(self.device)))
            return out
        n_w = w.numel()
        gw = torch.zeros((nq, n_w), dtype=torch.float32, device=self.device) if weight_grad else None
        if nq > 0:
            with torch.cuda.device(self.device):
                check(self._L.cwq_rank_scores_backward_w(
                    self._h, _ptr(q), nq, _ptr(g), _ptr(w) if n_w else None, n_w, _ptr(out) if out is not None else None,
                    _ptr(gw) if weight_grad and n_w else None, _stream(self.device)))
        return (out, gw) if weight_grad else out

    def _open_mask(self, mask):
        if not isinstance(mask, SentenceMask) or mask.closed:
            raise ValueError("mask must be an open SentenceMask (CobwebIndex.sentence_mask)")
        return mask

    def rank_ce(self, q, target, temperature=1.0, grad=False, level_weights=None, weight_grad=False, mask=None):
        """Cross-entropy ranking loss over all sentence scores (cwq_rank_ce): q [nq, dim],
        target [nq] sentence ids -> (loss [nq] = logsumexp(scores / T) - scores[target] / T,
        grad_q [nq, dim] = d loss / d q or None when grad is False, target_score [nq], rank [nq]
        int64: the target's 1-based position in score_topk's order).  No [nq, n_sent] tensor is
        made.  A target outside the tree: loss inf, a zero gradient row, score -inf, rank -1.
        level_weights [n_w]: everything under these level weights instead of the index's own
        (cwq_rank_ce_w); weight_grad=True appends grad_w [nq, n_w] = d loss / d w per query to
        the returned tuple.
        mask (a SentenceMask of this index): the loss, gradient, score and rank over the mask's
        allowed sentences only (cwq_rank_ce_masked); a target that is not allowed
        is an invalid target.  Not together with level_weights (ValueError)."""
        if mask is not None:
            self._open_mask(mask)
            if level_weights is not None or weight_grad:
                raise ValueError("mask and level_weights do not go together (call-time weights are not masked)")
        q = self._queries(q)
        nq = q.shape[0]
        t = torch.as_tensor(target)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("target must hold integer sentence ids")
        t = t.reshape(-1).to(self.device, torch.int64).contiguous()
        if t.shape[0] != nq:
            raise ValueError(f"target must be [{nq}]")
        temperature = float(temperature)
        if not (np.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be finite and > 0")
        w = self._level_weights(level_weights)
        if weight_grad and w is None:
            raise ValueError("weight_grad needs level_weights (their length sets the gradient's)")
        loss = torch.empty(nq, dtype=torch.float32, device=self.device)
        tscore = torch.empty(nq, dtype=torch.float32, device=self.device)
        rank = torch.empty(nq, dtype=torch.int64, device=self.device)
        gq = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device) if grad else None
        gw = torch.zeros((nq, w.numel()), dtype=torch.float32, device=self.device) if weight_grad else None
        if nq == 0:   # empty tensors have no device pointer to pass
            return (loss, gq, tscore, rank, gw) if weight_grad else (loss, gq, tscore, rank)
        with torch.cuda.device(self.device):
            if mask is not None:
                check(self._L.cwq_rank_ce_masked(self._h, mask._h, _ptr(q), nq, _ptr(t), temperature, _ptr(loss),
                                                 _ptr(gq) if grad else None, _ptr(tscore), _ptr(rank),
                                                 _stream(self.device)))
            elif w is None:
                check(self._L.cwq_rank_ce(self._h, _ptr(q), nq, _ptr(t), temperature, _ptr(loss),
                                          _ptr(gq) if grad else None, _ptr(tscore), _ptr(rank), _stream(self.device)))
            else:
                n_w = w.numel()
                check(self._L.cwq_rank_ce_w(self._h, _ptr(q), nq, _ptr(t), temperature, _ptr(w) if n_w else None, n_w,
                                            _ptr(loss), _ptr(gq) if grad else None,
                                            _ptr(gw) if weight_grad and n_w else None, _ptr(tscore), _ptr(rank),
                                            _stream(self.device)))
        return (loss, gq, tscore, rank, gw) if weight_grad else (loss, gq, tscore, rank)

    def _pair_ids(self, ids, nq):
        t = torch.as_tensor(ids)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("ids must hold integer sentence ids")
        if t.dim() == 1:
            t = t[None, :] if nq == 1 else t[:, None]
        if t.dim() != 2 or t.shape[0] != nq or t.shape[1] < 1:
            raise ValueError(f"ids must be [{nq}, m] with m >= 1")
        return t.to(self.device, torch.int64).contiguous()

    def score_pairs(self, q, ids):
        """The Fast scores of given sentences (cwq_score_pairs): q [nq, dim], ids
        [nq, m] sentence ids per query -> [nq, m] float32, each the bits rank_scores has in that
        column; -inf for an id of -1, an id outside [0, n_sent) and a sentence outside the tree.
        No [nq, n_sent] tensor is made.  A q that requires grad (with grad enabled) gets scores
        with autograd history (autograd.PairScores)."""
        if getattr(q, "requires_grad", False) and torch.is_grad_enabled():
            from .autograd import pair_scores_autograd
            return pair_scores_autograd(self, q, ids)
        q = self._queries(q)
        nq = q.shape[0]
        ids = self._pair_ids(ids, nq)
        out = torch.empty(ids.shape, dtype=torch.float32, device=self.device)
        if nq > 0:
            with torch.cuda.device(self.device):
                check(self._L.cwq_score_pairs(self._h, _ptr(q), nq, _ptr(ids), ids.shape[1], _ptr(out),
                                              _stream(self.device)))
        return out

    def score_pairs_backward(self, q, ids, grad):
        """Gradient of score_pairs with respect to the queries (cwq_score_pairs_backward): grad
        [nq, m], the upstream gradient of every score (entries whose score is -inf are never
        read; duplicates add) -> [nq, dim] float32.  m <= 4096.  Needs nothing from the forward
        call; bit-identical from run to run and for a query alone or in a batch."""
        q = self._queries(q)
        nq = q.shape[0]
        ids = self._pair_ids(ids, nq)
        g = torch.as_tensor(grad, dtype=torch.float32)
        if g.dim() == 1:
            g = g.reshape(ids.shape) if g.numel() == ids.numel() else g
        if g.shape != ids.shape:
            raise ValueError(f"grad must be {list(ids.shape)}")
        g = g.to(self.device).contiguous()
        out = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device)
        if nq > 0:
            with torch.cuda.device(self.device):
                check(self._L.cwq_score_pairs_backward(self._h, _ptr(q), nq, _ptr(ids), ids.shape[1], _ptr(g),
                                                       _ptr(out), _stream(self.device)))
        return out

    def rank_ce_topk(self, q, target, K, temperature=1.0, grad=False, mask=None, masks=None, mask_of_query=None):
        """Cross-entropy loss over the exact top-K plus the target (cwq_rank_ce_topk, DESIGN
        §4.18): -> (loss [nq], grad_q [nq, dim] or None when grad is False, target_score [nq],
        rank [nq] int64: exact inside the top-K, else K + 1, tail_bound [nq]: an upper bound of
        rank_ce's loss minus this loss, cand_ids [nq, K]: score_topk's row).  A target outside
        the tree: loss inf, a zero gradient row, score -inf, rank -1, bound 0.
        mask, or masks with mask_of_query (as score_topk takes them): the candidates are the
        masked retrieval's, the tail bound counts the query's own mask's allowed sentences and a
        target that is not allowed is invalid (cwq_rank_ce_topk_masked)."""
        if masks is not None and mask is not None:
            raise ValueError("pass mask= or masks=, not both")
        if (masks is None) != (mask_of_query is None):
            raise ValueError("masks= and mask_of_query= go together")
        q = self._queries(q)
        nq = q.shape[0]
        t = torch.as_tensor(target)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("target must hold integer sentence ids")
        t = t.reshape(-1).to(self.device, torch.int64).contiguous()
        if t.shape[0] != nq:
            raise ValueError(f"target must be [{nq}]")
        K = int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        temperature = float(temperature)
        if not (np.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be finite and > 0")
        loss = torch.empty(nq, dtype=torch.float32, device=self.device)
        tscore = torch.empty(nq, dtype=torch.float32, device=self.device)
        rank = torch.empty(nq, dtype=torch.int64, device=self.device)
        bound = torch.empty(nq, dtype=torch.float32, device=self.device)
        cand = torch.empty((nq, K), dtype=torch.int64, device=self.device)
        gq = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device) if grad else None
        moq = None
        if mask is not None:
            masks = [self._open_mask(mask)]
        elif masks is not None:
            masks = list(masks)
            if not masks or any(not isinstance(m, SentenceMask) or m.closed for m in masks):
                raise ValueError("masks must be a non-empty sequence of open SentenceMasks (CobwebIndex.sentence_mask)")
            moq = mask_of_query.detach().cpu().numpy() if torch.is_tensor(mask_of_query) else np.asarray(mask_of_query)
            if moq.ndim != 1 or moq.shape[0] != nq or moq.dtype.kind not in "iu":
                raise ValueError(f"mask_of_query must be {nq} integers, one per query")
            moq = np.ascontiguousarray(moq.clip(-1, 2 ** 31 - 1), dtype=np.int32)   # out of range stays out of range
        if nq > 0 and masks is not None:
            handles = (ctypes.c_void_p * len(masks))(*[m._h.value for m in masks])
            with torch.cuda.device(self.device):
                check(self._L.cwq_rank_ce_topk_masked(self._h, handles, len(masks), moq.ctypes.data if moq is not None else None,
                                                      _ptr(q), nq, _ptr(t), temperature, K, _ptr(loss),
                                                      _ptr(gq) if grad else None, _ptr(tscore), _ptr(rank), _ptr(bound),
                                                      _ptr(cand), _stream(self.device)))
        elif nq > 0:
            with torch.cuda.device(self.device):
                check(self._L.cwq_rank_ce_topk(self._h, _ptr(q), nq, _ptr(t), temperature, K, _ptr(loss),
                                               _ptr(gq) if grad else None, _ptr(tscore), _ptr(rank), _ptr(bound),
                                               _ptr(cand), _stream(self.device)))
        return loss, gq, tscore, rank, bound, cand

    def node_logprob(self, q, full=False):
        """Per-node log-likelihood in BFS order: lp' (full=False) or log_prob (full=True)."""
        q = self._queries(q)
        out = torch.empty((q.shape[0], self.n_nodes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._L.cwq_node_logprob(self._h, _ptr(q), q.shape[0], int(bool(full)), _ptr(out),
                                         _stream(self.device)))
        return out

    def prefix_bounds(self, q):
        """Diagnostic: (lo, hi, exact) [nq, n_internal] -- the Fast path prefixes of the
        internal nodes (BFS order) by the exact pass, and the bf16-MFMA bounds the filter
        uses on hierarchical trees (NaN where the filter reads none)."""
        q = self._queries(q)
        shape = (q.shape[0], int(self.info["internal_nodes"]))
        lo, hi, ex = (torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            check(self._L.cwq_prefix_bounds(self._h, _ptr(q), q.shape[0], _ptr(lo), _ptr(hi), _ptr(ex),
                                          _stream(self.device)))
        return lo, hi, ex

    def categorize(self, q, k, max_nodes=100000):
        """Best-first categorize ("Cobweb Basic", A4): retrieved BFS node ids in pop
        order [nq, k], number found [nq], log_prob call count [nq]."""
        q = self._queries(q)
        nq = q.shape[0]
        nodes = torch.full((nq, k), -1, dtype=torch.int64, device=self.device)
        found = torch.empty(nq, dtype=torch.int32, device=self.device)
        calls = torch.empty(nq, dtype=torch.int64, device=self.device)
        mx = int(min(max_nodes, 2 ** 62)) if max_nodes != float("inf") else 2 ** 62
        with torch.cuda.device(self.device):
            check(self._L.cwq_categorize(self._h, _ptr(q), nq, int(k), mx, _ptr(nodes), _ptr(found), _ptr(calls),
                                       _stream(self.device)))
        return nodes, found, calls


def welford_groups(X, order, group_ptr):
    """Sequential-Welford stats per row group on the GPU (libcwq cwq_welford_groups).
    X [n, D] float32 cuda; order, group_ptr int64 cuda.  Returns (count, mean, meanSq)."""
    n, D = X.shape
    G = group_ptr.numel() - 1
    count = torch.empty(G, dtype=torch.float32, device=X.device)
    mean = torch.empty((G, D), dtype=torch.float32, device=X.device)
    meanSq = torch.empty((G, D), dtype=torch.float32, device=X.device)
    for g0 in range(0, G, 65535):
        g1 = min(G, g0 + 65535)
        with torch.cuda.device(X.device):
            check(lib().cwq_welford_groups(_ptr(X), n, D, _ptr(order), ctypes.c_void_p(group_ptr[g0:].data_ptr()),
                                           g1 - g0, ctypes.c_void_p(count[g0:].data_ptr()),
                                           ctypes.c_void_p(mean[g0:].data_ptr()),
                                           ctypes.c_void_p(meanSq[g0:].data_ptr()), _stream(X.device)))
    return count, mean, meanSq
