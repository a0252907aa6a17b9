"""Autograd through the sentence scores (CobwebWrapper.py:267-294, "Differentiable: return
raw scores for all leaves"; the query-encoder training loss of
src/training/cobweb_query_train.py:104-126 backpropagates through them).

Forward is `CobwebIndex.rank_scores` (cwq_rank_scores), backward is
`CobwebIndex.rank_scores_backward` (cwq_rank_scores_backward): both run in
libcwq on torch's current stream.  The backward needs only the queries, the upstream
gradient and the index, so nothing of the forward is stored.
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
    """scores = index.rank_scores(q) for q float32 [nq, dim] on the index device."""

    @staticmethod
    def forward(ctx, q, index):
        ctx.index = index
        ctx.pin = _Pin(index)
        ctx.save_for_backward(q)
        return index.rank_scores(q.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (q,) = ctx.saved_tensors
        return ctx.index.rank_scores_backward(q, grad_out), None


class RankCE(torch.autograd.Function):
    """(loss [nq], target_score [nq], rank [nq]) = index.rank_ce(q, target, T) for q float32
    [nq, dim] on the index device (cwq_rank_ce).  The forward computes
    d loss / d q with the loss when q requires grad and saves it: the backward is a torch
    multiply, no library call, so the index needs no pin."""

    @staticmethod
    def forward(ctx, q, index, target, temperature, need):
        loss, gq, tscore, rank = index.rank_ce(q.detach(), target, temperature, grad=need)
        if need:
            ctx.save_for_backward(gq)
        ctx.mark_non_differentiable(tscore, rank)
        return loss, tscore, rank

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _gs, _gr):
        (gq,) = ctx.saved_tensors
        return gq * grad_loss[:, None], None, None, None, None


def rank_ce_autograd(index, q, target, temperature=1.0):
    """Differentiable per-query loss of index.rank_ce, with the target's score and rank: the
    device move, the cast and the reshape in front are torch ops, as in rank_scores_autograd.
    Under torch.no_grad(), or for a q that does not require grad, no gradient pass runs."""
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != index.dim:
        raise ValueError(f"queries must be [nq, {index.dim}]")
    q = q.to(index.device, torch.float32).contiguous()
    # decided here: grad mode is always off inside a Function's forward
    return RankCE.apply(q, index, target, temperature, bool(q.requires_grad and torch.is_grad_enabled()))


def rank_scores_autograd(index, q):
    """Differentiable index.rank_scores(q): the move to the index device, the cast and the
    [dim] -> [1, dim] reshape are torch ops, so a CPU leaf gets its .grad on the CPU."""
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != index.dim:
        raise ValueError(f"queries must be [nq, {index.dim}]")
    q = q.to(index.device, torch.float32).contiguous()
    return RankScores.apply(q, index)
