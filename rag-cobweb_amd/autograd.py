"""Autograd through the sentence scores (CobwebWrapper.py:267-294, "Differentiable: return
raw scores for all leaves"; the query-encoder training loss of
src/training/cobweb_query_train.py:104-126 backpropagates through them).

Forward is `CobwebIndex.rank_scores` (cwq_rank_scores), backward is
`CobwebIndex.rank_scores_backward` (cwq_rank_scores_backward): both run in
libcwq on torch's current stream.  The backward needs only the queries, the upstream
gradient and the index, so nothing of the forward is stored.

Both functions also take the level weights as a differentiable input (`level_weights`,
cwq_rank_scores_w / cwq_rank_scores_backward_w / cwq_rank_ce_w): the scores
are evaluated under that vector instead of the weights baked into the index, and its .grad is
the per-query weight gradient summed over the batch.
"""
import torch
from torch.autograd.function import once_differentiable


class _Pin:
    """Keeps a CobwebIndex's device handle alive for a pending backward: the wrapper closes
    its index when sentences are added (add_sentences rebuilds it), and a graph built on the
    old tree must still differentiate the old tree.  Released with the graph."""

    def __init__(self, index):
        self.index = index
        index._pin()

    def __del__(self):
        try:
            self.index._unpin()
        except Exception:
            pass


class RankScores(torch.autograd.Function):
    """scores = index.rank_scores(q, w) for q float32 [nq, dim] and w (None, or float32 [n_w])
    on the index device."""

    @staticmethod
    def forward(ctx, q, index, w=None):
        ctx.index = index
        ctx.pin = _Pin(index)
        ctx.has_w = w is not None
        ctx.save_for_backward(*((q, w) if ctx.has_w else (q,)))
        return index.rank_scores(q.detach()) if w is None else index.rank_scores(q.detach(), w.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q = ctx.saved_tensors[0]
        w = ctx.saved_tensors[1] if ctx.has_w else None
        need_q = ctx.needs_input_grad[0]
        need_w = ctx.has_w and ctx.needs_input_grad[2]
        if not ctx.has_w:
            return ctx.index.rank_scores_backward(q, grad_out), None, None
        if not need_w:
            return ctx.index.rank_scores_backward(q, grad_out, w), None, None
        gq, gw = ctx.index.rank_scores_backward(q, grad_out, w, weight_grad=True, query_grad=need_q)
        return gq, None, gw.sum(0)


class RankCE(torch.autograd.Function):
    """(loss [nq], target_score [nq], rank [nq]) = index.rank_ce(q, target, T, w) for q float32
    [nq, dim] on the index device (cwq_rank_ce).  The forward computes
    d loss / d q (and d loss / d w per query) with the loss where they are needed and saves
    them: the backward is torch arithmetic, no library call, so the index needs no pin."""

    @staticmethod
    def forward(ctx, q, index, target, temperature, need, w=None, need_w=False, mask=None):
        if mask is not None:
            loss, gq, tscore, rank, *gw = index.rank_ce(q.detach(), target, temperature, grad=need, mask=mask)
        elif w is None:
            loss, gq, tscore, rank, *gw = index.rank_ce(q.detach(), target, temperature, grad=need)
        else:
            loss, gq, tscore, rank, *gw = index.rank_ce(q.detach(), target, temperature, grad=need,
                                                        level_weights=w.detach(), weight_grad=need_w)
        ctx.need, ctx.need_w = need, need_w
        ctx.save_for_backward(*([gq] if need else []), *gw)
        ctx.mark_non_differentiable(tscore, rank)
        return loss, tscore, rank

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _gs, _gr):
        saved = list(ctx.saved_tensors)
        gq = saved.pop(0) * grad_loss[:, None] if ctx.need else None
        gw = (saved.pop(0) * grad_loss[:, None]).sum(0) if ctx.need_w else None
        return gq, None, None, None, None, gw, None, None


def _weights(index, w):
    """The level weights on the index device as float32 [n_w], by torch ops (a CPU or float64
    parameter gets its .grad on its own device and dtype)."""
    if w is None:
        return None
    w = torch.as_tensor(w)
    if w.dim() != 1 or w.shape[0] > 64:
        raise ValueError("level_weights must be a vector of at most 64 values")
    return w.to(index.device, torch.float32).contiguous()


def rank_ce_autograd(index, q, target, temperature=1.0, level_weights=None, mask=None):
    """Differentiable per-query loss of index.rank_ce, with the target's score and rank: the
    device move, the cast and the reshape in front are torch ops, as in rank_scores_autograd.
    Under torch.no_grad(), or for inputs that do not require grad, no gradient pass runs.
    mask: the loss over a SentenceMask's allowed sentences (index.rank_ce(mask=...)); not
    together with level_weights."""
    if mask is not None and level_weights is not None:
        raise ValueError("mask and level_weights do not go together (call-time weights are not masked)")
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != index.dim:
        raise ValueError(f"queries must be [nq, {index.dim}]")
    q = q.to(index.device, torch.float32).contiguous()
    w = _weights(index, level_weights)
    # decided here: grad mode is always off inside a Function's forward
    on = torch.is_grad_enabled()
    need = bool(q.requires_grad and on)
    return RankCE.apply(q, index, target, temperature, need, w, bool(w is not None and w.requires_grad and on), mask)


def rank_scores_autograd(index, q, level_weights=None):
    """Differentiable index.rank_scores(q): the move to the index device, the cast and the
    [dim] -> [1, dim] reshape are torch ops, so a CPU leaf gets its .grad on the CPU."""
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != index.dim:
        raise ValueError(f"queries must be [nq, {index.dim}]")
    q = q.to(index.device, torch.float32).contiguous()
    w = _weights(index, level_weights)
    return RankScores.apply(q, index, w)


class TopKScores(torch.autograd.Function):
    """(ids, scores) = index.score_topk(q, k, ...) with the scores differentiable in q (DESIGN.md
    §4.18): the backward is cwq_score_pairs_backward over the returned ids, whose padded (-1 /
    -inf) entries contribute nothing.  Plain, mask= and masks= calls alike."""

    @staticmethod
    def forward(ctx, q, index, k, mask, masks, mask_of_query):
        ctx.index = index
        ctx.pin = _Pin(index)
        ids, scores = index.score_topk(q.detach(), k, mask=mask, masks=masks, mask_of_query=mask_of_query)
        ctx.save_for_backward(q, ids)
        ctx.mark_non_differentiable(ids)
        return ids, scores

    @staticmethod
    @once_differentiable
    def backward(ctx, _gi, grad_scores):
        q, ids = ctx.saved_tensors
        return ctx.index.score_pairs_backward(q, ids, grad_scores), None, None, None, None, None


class PairScores(torch.autograd.Function):
    """scores = index.score_pairs(q, ids); backward cwq_score_pairs_backward."""

    @staticmethod
    def forward(ctx, q, index, ids):
        ctx.index = index
        ctx.pin = _Pin(index)
        ctx.save_for_backward(q, ids)
        return index.score_pairs(q.detach(), ids)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_scores):
        q, ids = ctx.saved_tensors
        return ctx.index.score_pairs_backward(q, ids, grad_scores), None, None


class RankCETopK(torch.autograd.Function):
    """(loss, target_score, rank, tail_bound, cand_ids) = index.rank_ce_topk(q, target, K, T).
    Like RankCE the forward computes d loss / d q where it is needed and saves it, so the
    backward is torch arithmetic; the index is pinned all the same, as RankScores pins it."""

    @staticmethod
    def forward(ctx, q, index, target, K, temperature, need, mask=None, masks=None, mask_of_query=None):
        ctx.pin = _Pin(index)
        loss, gq, tscore, rank, bound, cand = index.rank_ce_topk(q.detach(), target, K, temperature, grad=need,
                                                                 mask=mask, masks=masks, mask_of_query=mask_of_query)
        ctx.need = need
        ctx.save_for_backward(*([gq] if need else []))
        ctx.mark_non_differentiable(tscore, rank, bound, cand)
        return loss, tscore, rank, bound, cand

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *_):
        gq = ctx.saved_tensors[0] * grad_loss[:, None] if ctx.need else None
        return gq, None, None, None, None, None, None, None, None


def _queries_autograd(index, q):
    """The move to the index device, the cast and the [dim] -> [1, dim] reshape as torch ops: a
    CPU leaf gets its gradient on the CPU."""
    q = torch.as_tensor(q)
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != index.dim:
        raise ValueError(f"queries must be [nq, {index.dim}]")
    return q.to(index.device, torch.float32).contiguous()


def topk_scores_autograd(index, q, k, mask=None, masks=None, mask_of_query=None):
    if int(k) > 4096:   # cwq_score_pairs_backward's entry limit: fail here, not in a later backward()
        raise ValueError("score_topk with a query that requires grad takes k <= 4096 (the sparse backward's limit): "
                         "detach the query, or differentiate rank_scores")
    return TopKScores.apply(_queries_autograd(index, q), index, int(k), mask, masks, mask_of_query)


def pair_scores_autograd(index, q, ids):
    q = _queries_autograd(index, q)
    return PairScores.apply(q, index, index._pair_ids(ids, q.shape[0]))


def rank_ce_topk_autograd(index, q, target, K, temperature=1.0, mask=None, masks=None, mask_of_query=None):
    """Differentiable per-query loss of index.rank_ce_topk with the target's score, its rank, the
    tail bound and the candidate ids (all non-differentiable).  Under torch.no_grad(), or for a
    q that does not require grad, no gradient pass runs."""
    q = _queries_autograd(index, q)
    need = bool(q.requires_grad and torch.is_grad_enabled())
    return RankCETopK.apply(q, index, target, int(K), float(temperature), need, mask, masks, mask_of_query)
