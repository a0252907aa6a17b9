"""Drop-in `CobwebWrapper` for src/cobweb/CobwebWrapper.py, backed by libcwq on MI355X.

Same constructor, method names, argument meanings, return types and error
behaviour as the reference class (file:line per method), so harness code such as
src/utils/benchmark_utils.py:576-581 (`retrieve_cobweb_basic`) runs unchanged:

    cobweb.cobweb_predict_fast(query_emb, k)   -> list of sentences   (A6)
    cobweb.cobweb_predict(query_emb, k)        -> list of sentences   (A4/A5)

Differences (documented in DESIGN.md §6):
  * scoring runs on the GPU through libcwq; there is no CPU path;
  * exact score ties are broken deterministically (lower node / sentence id)
    instead of by randn*1e-6 noise (CobwebWrapper.py:246-256) or the heap's random()
    key (CobwebTorchTree.py:243,285); the global random() stream is still advanced by
    the draws the reference makes and the retrieved leaves' lists are shuffled with it
    (CobwebWrapper.py:456), so add -> Basic query -> add builds the reference's tree;
  * `cobweb_rank_scores` is differentiable with respect to a tensor embedding that
    requires grad, as in the reference (the training loss of
    src/training/cobweb_query_train.py:104-126 backpropagates into the query encoder);
    the backward is a libcwq kernel (autograd.py), not torch autograd over node tensors;
  * batched entry points `cobweb_predict_batch` / `cobweb_categorize_batch` take a
    [Q, D] query block and return id tensors; `cobweb_rank_scores_batch` is the
    differentiable [Q, n_sentences] counterpart of `cobweb_rank_scores`.
"""
import json
import math
import os
import random

import numpy as np
import torch

from .index import CobwebIndex, SentenceMask
from .tree import CobwebTree

MAX_INIT_SEARCH = 100000   # CobwebWrapper.py:24


_NATIVE_SKIP_MIN = 4096   # below this many draws getrandbits is cheaper than a state round trip


def advance_random(n, rng=random):
    """Advance `rng` (the global `random` module by default) past `n` random() draws:
    random() takes two 32-bit MT19937 outputs (CobwebTorchTree.py:243,268,285).  Small n:
    getrandbits(64*n), which takes exactly 2*n; large n (a flat 1M tree: ~1M draws per
    Basic query, 4.5 ms through an 8 MB integer): the state is twisted forward natively
    (libcwq cwq_mt19937_skip) and set back -- the same state bit for bit."""
    if n <= 0:
        return
    if n < _NATIVE_SKIP_MIN:
        rng.getrandbits(64 * n)
        return
    from . import _lib
    ver, words, gauss = rng.getstate()
    st = np.array(words, dtype=np.uint32)
    _lib.check(_lib.lib().cwq_mt19937_skip(st.ctypes.data, 2 * int(n)))
    rng.setstate((ver, tuple(st.tolist()), gauss))


class CobwebWrapper:
    def __new__(cls, *args, resident=False, **kwargs):
        # resident=True: the same interface over a tree that stays on the GPU between adds
        # and queries (resident.ResidentCobwebWrapper); the default is this class itself
        if resident and cls is CobwebWrapper:
            from .resident import ResidentCobwebWrapper
            cls = ResidentCobwebWrapper
        return object.__new__(cls)

    def __init__(self, corpus=None, corpus_embeddings=None, encode_func=lambda x: x, device=None, resident=False):
        """CobwebWrapper.py:13-50.  resident: see __new__ (it chose the class)."""
        self.encode_func = encode_func
        self.sentences = []
        self.sentence_to_node = {}
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("rag_cobweb_amd.CobwebWrapper needs a ROCm GPU (libcwq has no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.max_init_search = MAX_INIT_SEARCH
        self._prediction_index_valid = False
        self._index = None
        self._nodes = None
        self._node_to_index = {}
        self._leaf_to_path_indices = None
        self._level_weights = None
        self._weight_schedule = None
        self._schedule_params = {}
        self.max_depth = 0

        embedding_shape = None
        if corpus_embeddings is not None:
            corpus_embeddings = np.asarray(corpus_embeddings, dtype=np.float32) if isinstance(
                corpus_embeddings, list) else corpus_embeddings
            embedding_shape = tuple(corpus_embeddings.shape[1:])
        elif corpus and len(corpus) > 0:
            embedding_shape = tuple(np.asarray(self.encode_func([corpus[0]])).shape[1:])
        self.tree = CobwebTree(embedding_shape) if embedding_shape is not None else None

        if corpus_embeddings is not None:
            if corpus is None:
                corpus = [None] * len(corpus_embeddings)
            self.add_sentences(corpus, corpus_embeddings)
        elif corpus is not None and len(corpus) > 0:
            self.add_sentences(corpus)

    # ------------------------------------------------------------------ add path
    def add_sentences(self, new_sentences, new_vectors=None):
        """CobwebWrapper.py:52-80: incremental fit of each embedding, then the
        prediction index is invalidated."""
        if new_vectors is None:
            new_embeddings = np.asarray(self.encode_func(new_sentences), dtype=np.float32)
        else:
            new_embeddings = new_vectors
            if isinstance(new_embeddings, list):
                new_embeddings = np.asarray(new_embeddings, dtype=np.float32)
            if self.tree is not None and new_embeddings.shape[1] != self.tree.shape[0]:
                print(f"[Warning] Provided vector dim {new_embeddings.shape[1]} != tree dim "
                      f"{self.tree.shape[0]}, re-encoding...")
                new_embeddings = np.asarray(self.encode_func(new_sentences), dtype=np.float32)
        from .fit import _MAX_DEVICE_DIM, DeviceTreeFitter, TreeFitter
        X = np.asarray(new_embeddings.detach().cpu().numpy() if torch.is_tensor(new_embeddings)
                       else new_embeddings, dtype=np.float32)
        if self.tree is None:
            self.tree = CobwebTree(X.shape[1:])
        start = len(self.sentences)
        n = len(new_sentences)
        # the device-resident insert loop (one kernel for the whole batch) unless disabled
        # (CWQ_FIT_DEVICE=0) or the dimension is past its LDS budget: then the host-driven
        # fitter (per level one KL launch) -- both build the same tree
        use_dev = os.environ.get("CWQ_FIT_DEVICE", "1") != "0" and self.tree.dim <= _MAX_DEVICE_DIM
        if use_dev:
            fitter = DeviceTreeFitter(self.tree, device=self.device)
            leaves = fitter.fit_batch(X[:n])
            self.last_fit_stats = dict(fitter.stats)   # rows, kernel seconds, draws, ... (diagnostics)
        else:
            fitter = TreeFitter(self.tree, device=self.device)
            leaves = [fitter.ifit(X[i]) for i in range(n)]
            fitter.sync_to_host()
        for i, sent in enumerate(new_sentences):
            self.sentences.append(sent)
            leaf = leaves[i]
            if leaf.sentence_id is None:
                leaf.sentence_id = []
            leaf.sentence_id.append(start + i)
            self.sentence_to_node[start + i] = leaf
        self._invalidate_prediction_index()

    # --------------------------------------------------------------- index build
    def _invalidate_prediction_index(self):
        """CobwebWrapper.py:82-89."""
        self._prediction_index_valid = False
        if self._index is not None:
            self._index.close()
        self._index = None
        self._nodes = None
        self._node_to_index = {}
        self._leaf_to_path_indices = None

    def build_prediction_index(self):
        """CobwebWrapper.py:91-208: BFS flatten (O(Nn), not the reference's O(Nn^2)),
        then the device index (dim-major stats, path structure, level weights)."""
        if self._prediction_index_valid:
            return
        if set(self.sentence_to_node.keys()) != set(range(len(self.sentences))):
            raise ValueError("sentence_to_node mapping is inconsistent with sentence indices.")
        nodes, parent, mean, var, nos, max_depth = self.tree.flatten(len(self.sentences))
        for i, node in enumerate(nos):
            if node < 0:
                print(f"[Warning] Leaf path index for sentence ID {i} is None. "
                      f"This may indicate missing sentences in the tree.")
        weights = list(self._level_weights) if self._level_weights is not None else [1.0] * 6
        self._index = CobwebIndex(mean, var, parent, nos, weights, device=self.device)
        self._nodes = nodes
        self._node_to_index = {id(n): i for i, n in enumerate(nodes)}
        par = parent
        paths = []
        for s in nos:
            path, j = [], int(s)
            while j >= 0:
                path.append(j)
                j = int(par[j])
            paths.append(path[::-1] if s >= 0 else None)
        self._leaf_to_path_indices = paths
        self.max_depth = max(self.max_depth, max_depth)
        self._prediction_index_valid = True

    def force_rebuild_index(self):
        self._invalidate_prediction_index()
        self.build_prediction_index()

    def get_prediction_index_info(self):
        """CobwebWrapper.py:315-333 (the reference crashes here once the index is
        valid -- `_node_to_index` is never set; this one reports)."""
        info = {"index_valid": self._prediction_index_valid,
                "total_nodes": len(self._node_to_index) if self._prediction_index_valid else 0,
                "leaf_paths_cached": len(self._leaf_to_path_indices) if self._prediction_index_valid else 0,
                "means_cached": self._prediction_index_valid, "vars_cached": self._prediction_index_valid}
        if self._prediction_index_valid:
            info["means_shape"] = (self._index.n_nodes, self._index.dim)
            info["vars_shape"] = (self._index.n_nodes, self._index.dim)
            info["device"] = str(self.device)
            info.update(self._index.info)
        return info

    def get_node_path_stats(self, sentence_id):
        """CobwebWrapper.py:297-313."""
        self.build_prediction_index()
        if not (0 <= sentence_id < len(self._leaf_to_path_indices)) or self._leaf_to_path_indices[sentence_id] is None:
            return None, None
        path = self._leaf_to_path_indices[sentence_id]
        ns = [self._nodes[i] for i in path]
        means = torch.tensor(np.stack([n.mean for n in ns]), device=self.device)
        vars_ = torch.tensor(np.stack([self.tree.compute_var(n.meanSq, n.count) if n.count > 0
                                       else np.full(self.tree.dim, self.tree.prior_var, np.float32)
                                       for n in ns]), device=self.device)
        return means, vars_

    # ------------------------------------------------------------- level weights
    def set_level_weights(self, weights):
        """CobwebWrapper.py:335-346."""
        self._level_weights = weights
        self._weight_schedule = None
        self._invalidate_prediction_index()

    def set_weight_schedule(self, schedule_type, max_depth=10, **kwargs):
        """CobwebWrapper.py:348-366."""
        if self._prediction_index_valid:
            max_depth = self.max_depth
        self._weight_schedule = schedule_type
        self._schedule_params = kwargs
        self._level_weights = self._generate_weight_schedule(schedule_type, max_depth, **kwargs)
        self._invalidate_prediction_index()

    def _generate_weight_schedule(self, schedule_type, max_depth, **kwargs):
        """CobwebWrapper.py:368-408."""
        weights = []
        if schedule_type == "constant":
            weights = [kwargs.get("value", 1.0)] * max_depth
        elif schedule_type == "linear":
            start, end = kwargs.get("start", 1.0), kwargs.get("end", 1.0)
            if kwargs.get("direction", "increase") == "decrease":
                start, end = end, start
            if max_depth == 1:
                weights = [start]
            else:
                step = (end - start) / (max_depth - 1)
                weights = [start + i * step for i in range(max_depth)]
        elif schedule_type == "quadratic":
            start_n = kwargs.get("start_n", 1)
            for i in range(max_depth):
                n = start_n + i
                if n == 0:
                    n = 1
                weights.append(1 / (n ** 2))
        elif schedule_type == "exponential":
            base = kwargs.get("base", 0.5)
            weights = [base ** i for i in range(max_depth)]
        else:
            raise ValueError(f"Unknown schedule type: {schedule_type}")
        return weights

    def get_level_weights(self):
        return self._level_weights if self._level_weights is not None else [1.0, 1.0, 1.0, 1.0]

    def get_weight_schedule_info(self):
        return {"schedule_type": self._weight_schedule, "schedule_params": self._schedule_params,
                "current_weights": self.get_level_weights()}

    # ------------------------------------------------------------------ queries
    def _embed(self, input, is_embedding):
        emb = input if is_embedding else self.encode_func([input])[0]
        if torch.is_tensor(emb):
            return emb.detach().to(self.device, torch.float32).reshape(-1)
        return torch.as_tensor(np.asarray(emb, dtype=np.float32), device=self.device).reshape(-1)

    def sentence_mask(self, allowed):
        """An allowed-sentence set to pass as `allowed=` to the Fast calls again and again (no
        reference counterpart): a bool tensor / array with one entry per sentence, or sentence
        ids.  It belongs to the current prediction index: after add_sentences, set_level_weights
        or force_rebuild_index make a new one."""
        self.build_prediction_index()
        return self._index.sentence_mask(allowed)

    def _mask_for(self, allowed):
        """(mask, made here) for a call's `allowed`: a SentenceMask of the current index as it
        is, anything else through sentence_mask (the caller closes that one after its call)."""
        if isinstance(allowed, SentenceMask):
            if allowed.closed:
                raise ValueError("the SentenceMask is closed")
            if allowed._index is not self._index:
                raise ValueError("the SentenceMask belongs to an earlier prediction index: the index was rebuilt "
                                 "since (add_sentences, set_level_weights or force_rebuild_index); make a new "
                                 "one with sentence_mask()")
            return allowed, False
        return self._index.sentence_mask(allowed), True

    def cobweb_predict_indexed(self, input, k=5, return_ids=False, is_embedding=False, allowed=None):
        """CobwebWrapper.py:210-265 ("Cobweb Fast").  allowed (no reference counterpart): a
        SentenceMask, a bool mask over the sentences or sentence ids -- only these sentences
        are ranked."""
        self.build_prediction_index()
        n = self._index.n_sent if self._leaf_to_path_indices is None else len(self._leaf_to_path_indices)
        if n == 0:
            return []
        emb = input if is_embedding else self.encode_func([input])[0]
        if allowed is not None:
            mask, mine = self._mask_for(allowed)
            try:
                ids, _ = self._index.score_topk(self._embed(emb, True)[None, :], min(k, n), mask=mask)
                row = ids[0].tolist()
            finally:
                if mine:
                    mask.close()
            return [s if return_ids else self.sentences[s] for s in row if 0 <= s < len(self.sentences)]
        if not torch.is_tensor(emb):
            # a host embedding (the harness's numpy query): host memory in and out
            ids, _ = self._index.score_topk_host(np.asarray(emb, dtype=np.float32).reshape(1, -1), min(k, n))
        else:
            ids, _ = self._index.score_topk(self._embed(emb, True)[None, :], min(k, n))
        row = ids[0].tolist()
        out = []
        for s in row:
            if 0 <= s < len(self.sentences):
                out.append(s if return_ids else self.sentences[s])
        return out

    def cobweb_predict_fast(self, input, k=5, return_ids=False, is_embedding=False, allowed=None):
        """CobwebWrapper.py:428-433 (alias)."""
        if allowed is None:
            return self.cobweb_predict_indexed(input, k, return_ids, is_embedding)
        return self.cobweb_predict_indexed(input, k, return_ids, is_embedding, allowed=allowed)

    def cobweb_rank_scores(self, input, is_embedding=False):
        """CobwebWrapper.py:267-294: [n_sentences] leaf scores.  Differentiable: a tensor
        embedding that requires grad (on any device) gets scores with a grad_fn; with
        is_embedding=False the graph is cut, as by the reference's torch.tensor(emb)."""
        self.build_prediction_index()
        x = input.to(self.device) if is_embedding else self._embed(input, False)
        if len(self._leaf_to_path_indices) == 0:
            return torch.empty(0, device=self.device)
        return self._index.rank_scores(x.reshape(1, -1))[0]

    def cobweb_rank_scores_batch(self, queries, level_weights=None):
        """[Q, D] queries -> [Q, n_sentences] scores, differentiable like cobweb_rank_scores:
        one pass over the node means forward and one backward for the whole block (a training
        step of 16 queries streams them once, not 16 times).
        level_weights (a vector of up to 64 values, depth >= its length weighs 1.0): the scores
        under these level weights instead of the ones set by set_level_weights, without
        rebuilding the index, and differentiable in them too (a tensor that requires grad)."""
        self.build_prediction_index()
        if level_weights is None:
            return self._index.rank_scores(queries)
        return self._index.rank_scores(queries, level_weights)

    def cobweb_score_candidates(self, queries, sentence_ids):
        """[Q, D] queries and [Q, m] sentence ids (from another retriever, a hard-negative list,
        ...) -> [Q, m] Fast scores, the values cobweb_rank_scores_batch has in those columns,
        without the [Q, n_sentences] block (no reference counterpart; cwq_score_pairs).  -inf
        for an id of -1, an id out of range and a sentence outside the tree.  Differentiable
        with respect to `queries` like cobweb_rank_scores_batch."""
        self.build_prediction_index()
        return self._index.score_pairs(queries, sentence_ids)

    def _loss_sets(self, allowed, allowed_sets, set_of_query, level_weights, nq):
        """The masks of a masked loss / rank call: ([(mask, made here)], set_of_query as a host
        int64 array or None).  Accepts what cobweb_predict_batch accepts."""
        if allowed_sets is not None and allowed is not None:
            raise ValueError("pass allowed= or allowed_sets=, not both")
        if (allowed_sets is None) != (set_of_query is None):
            raise ValueError("allowed_sets= and set_of_query= go together")
        if level_weights is not None:
            raise ValueError("allowed / allowed_sets and level_weights do not go together: call-time level weights "
                             "are not masked")
        if allowed is not None:
            return [self._mask_for(allowed)], None
        soq = set_of_query.detach().cpu().numpy() if torch.is_tensor(set_of_query) else np.asarray(set_of_query)
        if soq.ndim != 1 or soq.shape[0] != nq or soq.dtype.kind not in "iu":
            raise ValueError(f"set_of_query must be {nq} integers, one per query")
        sets = list(allowed_sets)
        if not sets:
            raise ValueError("allowed_sets must not be empty")
        if soq.size and (int(soq.min()) < 0 or int(soq.max()) >= len(sets)):
            raise ValueError(f"set_of_query entries must be in [0, {len(sets)})")
        made = []
        try:
            for a in sets:
                made.append(self._mask_for(a))
        except Exception:
            for m, mine in made:
                if mine:
                    m.close()
            raise
        return made, soq.astype(np.int64)

    def _masked_rank_ce(self, q, labels, temperature, top_k, made, soq):
        """(loss, target_score, rank) over the call's masks: the top-K form in one call; the dense
        form once per set over that set's queries, the rows put back in order."""
        from .autograd import rank_ce_autograd, rank_ce_topk_autograd
        masks = [m for m, _ in made]
        if top_k is not None:
            if soq is None:
                out = rank_ce_topk_autograd(self._index, q, labels, top_k, temperature, mask=masks[0])
            else:
                out = rank_ce_topk_autograd(self._index, q, labels, top_k, temperature, masks=masks, mask_of_query=soq)
            return out[0], out[1], out[2]
        if soq is None:
            return rank_ce_autograd(self._index, q, labels, temperature, mask=masks[0])
        lab = torch.as_tensor(labels).reshape(-1)
        parts, order = [], []
        for j in np.unique(soq):
            idx = torch.from_numpy(np.nonzero(soq == j)[0])
            parts.append(rank_ce_autograd(self._index, q[idx.to(q.device)], lab[idx.to(lab.device)], temperature,
                                          mask=masks[int(j)]))
            order.append(idx)
        if not parts:
            return rank_ce_autograd(self._index, q, lab, temperature, mask=masks[0])
        inv = torch.argsort(torch.cat(order)).to(self._index.device)
        return tuple(torch.cat([p[i] for p in parts])[inv] for i in range(3))

    def cobweb_ranking_loss(self, queries, labels, temperature=1.0, reduction="mean", level_weights=None,
                            top_k=None, allowed=None, allowed_sets=None, set_of_query=None):
        """FixedDocsRankingLoss.forward (src/training/cobweb_query_train.py:104-126) for a
        block: [Q, D] query embeddings and [Q] labels (sentence ids) -> CrossEntropyLoss(
        cobweb_rank_scores(q) / temperature, label) averaged over the batch ("mean", the
        reference), summed ("sum") or per query ("none").  Differentiable with respect to
        `queries`; the scores are never materialised (cwq_rank_ce: one forward scan, and one
        backward stream when a gradient is wanted).
        level_weights: the loss under these level weights (see cobweb_rank_scores_batch); an
        nn.Parameter here is learned by any torch optimiser against the fixed index, and
        written back once with set_level_weights(w.tolist()).
        top_k: the cross-entropy over the exact top_k retrieved sentences plus the label instead
        of over all sentences (hard-negative training at retrieval speed; cwq_rank_ce_topk,
        DESIGN §4.18).  Not together with level_weights: retrieval reads the baked weights.
        allowed, or allowed_sets with set_of_query (no reference counterpart; what
        cobweb_predict_batch accepts): the cross-entropy over the allowed sentences only -- a
        tenant, ACL group or corpus split trains against its own negatives (cwq_rank_ce_masked /
        cwq_rank_ce_topk_masked).  A label that is not allowed gives an infinite
        loss for its query.  With top_k, allowed_sets is one call; without, each set runs once
        over its queries.  Not together with level_weights (ValueError)."""
        if reduction not in ("mean", "sum", "none"):
            raise ValueError('reduction must be "mean", "sum" or "none"')
        if top_k is not None and level_weights is not None:
            raise ValueError("top_k and level_weights do not go together: retrieval reads the level weights baked "
                             "into the index (set_level_weights)")
        self.build_prediction_index()
        if allowed is not None or allowed_sets is not None or set_of_query is not None:
            q = torch.as_tensor(queries)
            if q.dim() == 1:
                q = q[None, :]
            made, soq = self._loss_sets(allowed, allowed_sets, set_of_query, level_weights, q.shape[0])
            try:
                loss = self._masked_rank_ce(q, labels, temperature, top_k, made, soq)[0]
            finally:
                for m, mine in made:
                    if mine:
                        m.close()
            return loss if reduction == "none" else loss.mean() if reduction == "mean" else loss.sum()
        if top_k is not None:
            from .autograd import rank_ce_topk_autograd
            loss = rank_ce_topk_autograd(self._index, torch.as_tensor(queries), labels, top_k, temperature)[0]
            return loss if reduction == "none" else loss.mean() if reduction == "mean" else loss.sum()
        from .autograd import rank_ce_autograd
        if level_weights is None:
            loss, _, _ = rank_ce_autograd(self._index, torch.as_tensor(queries), labels, temperature)
        else:
            loss, _, _ = rank_ce_autograd(self._index, torch.as_tensor(queries), labels, temperature, level_weights)
        return loss if reduction == "none" else loss.mean() if reduction == "mean" else loss.sum()

    def cobweb_target_ranks(self, queries, labels, level_weights=None, top_k=None, allowed=None, allowed_sets=None,
                            set_of_query=None):
        """evaluate()'s two per-query numbers (src/training/cobweb_query_train.py:213-304)
        without forming a ranking: (rank [Q] int64, the 1-based position of the label in the
        Fast ranking -- -1 for a label outside the tree --, true_score [Q]).
        level_weights: the ranks under these level weights (recall / MRR of a schedule sweep
        against a fixed index).
        top_k: ranks from one top_k retrieval instead of a scan of all leaves, capped at
        top_k + 1 ("at least top_k + 1"); not together with level_weights.
        allowed, or allowed_sets with set_of_query (as cobweb_ranking_loss takes them): the
        label's rank among the allowed sentences only -- the rank the caller's own
        cobweb_predict_batch(..., allowed=...) ranking gives it; -1 / -inf for a label that is
        not allowed.  Not together with level_weights (ValueError)."""
        if top_k is not None and level_weights is not None:
            raise ValueError("top_k and level_weights do not go together: retrieval reads the level weights baked "
                             "into the index (set_level_weights)")
        self.build_prediction_index()
        with torch.no_grad():
            if allowed is not None or allowed_sets is not None or set_of_query is not None:
                q = torch.as_tensor(queries).detach()
                if q.dim() == 1:
                    q = q[None, :]
                made, soq = self._loss_sets(allowed, allowed_sets, set_of_query, level_weights, q.shape[0])
                try:
                    _, tscore, rank = self._masked_rank_ce(q, labels, 1.0, top_k, made, soq)
                finally:
                    for m, mine in made:
                        if mine:
                            m.close()
                return rank, tscore
            if top_k is not None:
                _, _, tscore, rank, _, _ = self._index.rank_ce_topk(torch.as_tensor(queries).detach(), labels, top_k)
                return rank, tscore
            if level_weights is None:
                _, _, tscore, rank = self._index.rank_ce(torch.as_tensor(queries).detach(), labels)
            else:
                _, _, tscore, rank = self._index.rank_ce(torch.as_tensor(queries).detach(), labels,
                                                         level_weights=level_weights)
        return rank, tscore

    def cobweb_predict(self, input, k=5, return_ids=False, is_embedding=False):
        """CobwebWrapper.py:435-461 ("Cobweb Basic"): best-first categorize with
        retrieve_k=k and max_nodes=max_init_search; IndexError when fewer than k
        nodes with sentences are retrieved (CobwebTorchTree.py:289)."""
        self.build_prediction_index()
        emb = input if is_embedding else self.encode_func([input])[0]
        if torch.is_tensor(emb):
            x = emb.detach().to(self._index.device, torch.float32).reshape(1, -1)
            nodes, found, calls = self._index.categorize(x, k, self.max_init_search)
            nodes, found, calls = nodes.cpu().numpy(), found.cpu().numpy(), calls.cpu().numpy()
        else:   # a host embedding (the harness's numpy query): host memory in and out, one call
            nodes, found, calls = self._index.categorize_host(np.asarray(emb, np.float32).reshape(1, -1), k,
                                                              self.max_init_search)
        nf = int(found[0])
        # the reference's search draws one random() per heap push (one per log_prob call)
        # and one per retrieval (CobwebTorchTree.py:243,268,285) from the global stream
        # that ifit also draws from; advance it by as many, before the IndexError too
        advance_random(int(calls[0]) + nf)
        if nf < k:
            raise IndexError("list index out of range")
        results = []
        for nid in nodes[0].tolist():
            sid_lst = self._nodes[nid].sentence_id
            random.shuffle(sid_lst)      # CobwebWrapper.py:456, mutating the leaf's list
            for sid in sid_lst:
                if sid is None or sid >= len(self.sentences):
                    continue
                results.append(sid if return_ids else self.sentences[sid])
        return results

    # batched extensions (the benchmark's unit of work)
    def sentence_masks_by_label(self, label_of_sentence):
        """One SentenceMask per distinct label (tenant, ACL group, date bucket, ...) of an integer
        label per sentence -> (masks, values), `values` the distinct labels sorted and masks[j]
        the sentences labelled values[j].  For a batch whose query i may see label
        label_of_query[i] only:

            masks, values = w.sentence_masks_by_label(label_of_sentence)
            set_of_query = torch.searchsorted(values, label_of_query)   # every query label must be in values
            ids, scores = w.cobweb_predict_batch(Q, k, allowed_sets=masks, set_of_query=set_of_query)

        A mask takes 1 B per leaf-class row + 4 B per live row + 1 bit per sentence of device
        memory, whatever its size: 1,000 masks over 1M sentences are about 1.1 GB.
        The masks belong to the current prediction index, like sentence_mask's; close them when
        done."""
        self.build_prediction_index()
        lab = torch.as_tensor(label_of_sentence).reshape(-1)
        if lab.dtype.is_floating_point or lab.dtype.is_complex or lab.dtype == torch.bool:
            raise ValueError("label_of_sentence must be integers")
        if lab.numel() != self._index.n_sent:
            raise ValueError(f"label_of_sentence must have one entry per sentence: got {lab.numel()}, the index has "
                             f"{self._index.n_sent}")
        # one sort of the labels, then each mask from its own run of sentence ids: the work
        # is O(n log n) in all, not one pass over the sentences per label
        values, counts = torch.unique(lab, sorted=True, return_counts=True)
        runs = torch.split(torch.argsort(lab, stable=True), counts.tolist())
        masks = []
        try:
            for ids in runs:
                masks.append(self._index.sentence_mask(ids))
        except Exception:
            for m in masks:   # a failed build leaks no mask
                m.close()
            raise
        return masks, values

    def cobweb_predict_batch(self, queries, k=5, allowed=None, allowed_sets=None, set_of_query=None):
        """[Q, D] queries -> (ids [Q, k] int64 tensor, scores [Q, k] float32), Fast path.
        allowed: as in cobweb_predict_indexed, one set for the whole block (-1 / -inf past the
        allowed sentences).
        allowed_sets with set_of_query (no reference counterpart): a sequence of sets -- each a
        SentenceMask, a bool mask or sentence ids -- and one index into it per query; query i
        is ranked over allowed_sets[set_of_query[i]] only, in one call.  (A keyword of its own:
        allowed=[1, 2, 3] already means sentence ids.)  Not together with allowed=."""
        if allowed_sets is not None and allowed is not None:
            raise ValueError("pass allowed= or allowed_sets=, not both")
        if (allowed_sets is None) != (set_of_query is None):
            raise ValueError("allowed_sets= and set_of_query= go together")
        self.build_prediction_index()
        if allowed_sets is not None:
            made = []
            try:
                for a in allowed_sets:
                    made.append(self._mask_for(a))
                return self._index.score_topk(queries, k, masks=[m for m, _ in made], mask_of_query=set_of_query)
            finally:
                for m, mine in made:
                    if mine:
                        m.close()
        if allowed is None:
            return self._index.score_topk(queries, k)
        mask, mine = self._mask_for(allowed)
        try:
            return self._index.score_topk(queries, k, mask=mask)
        finally:
            if mine:
                mask.close()

    def cobweb_categorize_batch(self, queries, k=5, max_nodes=None):
        """[Q, D] queries -> (node ids [Q, k] BFS order, n_found [Q], log_prob calls [Q])."""
        self.build_prediction_index()
        return self._index.categorize(queries, k, self.max_init_search if max_nodes is None else max_nodes)

    # -------------------------------------------------------------- persistence
    def dump_json(self, save_path=None):
        """CobwebWrapper.py:484-497."""
        state = {"tree": json.loads(self.tree.dump_json()), "sentences": self.sentences,
                 "embedding_dim": self.tree.shape[0]}
        if save_path:
            with open(save_path, "w") as f:
                json.dump(state, f, indent=2)
        return json.dumps(state, indent=2)

    @staticmethod
    def load_json(json_data, encode_func=lambda x: x, device=None, resident=False):
        """CobwebWrapper.py:500-555, without its two bugs (identity encoder has no
        .shape; list sentence ids are unhashable): the tree shape comes from the
        JSON and every sentence id of a node maps to that node."""
        data = json.loads(json_data) if isinstance(json_data, str) else json_data
        w = CobwebWrapper.__new__(CobwebWrapper)
        CobwebWrapper.__init__(w, encode_func=encode_func, device=device)
        w.tree = CobwebTree.from_json(data["tree"])
        w.sentences = data.get("sentences", [])
        w.max_init_search = data.get("max_init_search", MAX_INIT_SEARCH)
        stack = [w.tree.root]
        while stack:
            n = stack.pop()
            for s in n.sentence_id or []:
                w.sentence_to_node[s] = n
            stack.extend(n.children)
        return _as_resident(w) if resident else w

    def save_binary(self, path):
        """Binary counterpart of dump_json (F2): the tree's BFS arrays plus the
        sentences (UTF-8 JSON bytes) in one .npz, readable with allow_pickle=False."""
        sent = np.frombuffer(json.dumps(list(self.sentences)).encode(), np.uint8)
        self.tree.save_binary(path, extra={"sentences": sent,
                                           "max_init_search": np.asarray([self.max_init_search], np.int64)})

    @staticmethod
    def load_binary(path, encode_func=lambda x: x, device=None, resident=False):
        head, a = CobwebTree.read_binary(path)
        sentences = json.loads(bytes(a.pop("sentences")).decode()) if "sentences" in a else []
        mis = int(a.pop("max_init_search")[0]) if "max_init_search" in a else MAX_INIT_SEARCH
        t = CobwebTree.from_arrays(a["parent"], a["count"], a["mean"], a["meanSq"], a["sid_ptr"], a["sid_list"],
                                   prior_var=head["prior_var"])
        t.use_info, t.acuity_cutoff, t.use_kl, t.alpha = (head["use_info"], head["acuity_cutoff"], head["use_kl"],
                                                          head["alpha"])
        w = CobwebWrapper.from_tree(t, sentences, device=device)
        w.encode_func = encode_func
        w.max_init_search = mis
        return _as_resident(w) if resident else w

    @classmethod
    def from_tree(cls, tree, sentences, device=None, resident=False):
        """Wrap an existing CobwebTree (e.g. CobwebTree.from_arrays / from_json)."""
        if resident:
            return _as_resident(CobwebWrapper.from_tree(tree, sentences, device=device))
        w = cls(device=device)
        w.tree = tree
        w.sentences = list(sentences)
        stack = [tree.root]
        while stack:
            n = stack.pop()
            for s in n.sentence_id or []:
                w.sentence_to_node[s] = n
            stack.extend(n.children)
        return w

    @classmethod
    def from_index(cls, index, sentences, encode_func=lambda x: x, node_of_sentence=None):
        """A query-only wrapper over a prebuilt CobwebIndex (e.g. a flat-synth tree at C3/C4
        scale, where the host keeps no node objects): the Fast / rank-score / batch entry
        points work; the add path needs the node tree.  With node_of_sentence (the BFS node
        of every sentence, as given to the index) Basic (cobweb_predict) works too: its id
        expansion reads per-node sentence lists made on first use (_NodeSentences)."""
        w = cls(device=index.device, encode_func=encode_func)
        w.sentences = sentences          # any sequence (len + indexing); not copied
        w._index = index
        w._prediction_index_valid = True
        if node_of_sentence is not None:
            w._nodes = _NodeSentences(node_of_sentence, index.n_nodes)
        return w

    def __len__(self):
        return len(self.sentences)


def _as_resident(w):
    """The resident counterpart of a default wrapper that was just loaded from a host tree."""
    from .resident import ResidentCobwebWrapper
    return ResidentCobwebWrapper._adopt(w)


class _NodeSentences:
    """nodes[i].sentence_id for a wrapper without host Node objects: the sentence ids of
    BFS node i (ascending), made on first access and kept, so the in-place random.shuffle
    of Basic's id expansion (CobwebWrapper.py:456) persists across calls as on the
    reference's node lists."""

    class _Ref:
        __slots__ = ("sentence_id",)

        def __init__(self, ids):
            self.sentence_id = ids

    def __init__(self, node_of_sentence, n_nodes):
        nos = np.asarray(node_of_sentence, np.int64)
        order = np.argsort(nos, kind="stable")
        self._ids = order
        self._ptr = np.searchsorted(nos[order], np.arange(n_nodes + 1))
        self._made = {}

    def __len__(self):
        return len(self._ptr) - 1

    def __getitem__(self, i):
        r = self._made.get(i)
        if r is None:
            r = self._Ref([int(v) for v in self._ids[self._ptr[i]:self._ptr[i + 1]]])
            self._made[i] = r
        return r
