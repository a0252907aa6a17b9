"""Yardsticks of the fused ranking-loss tests (tests/test_gpu_rank_ce.py), beside
grad_yardstick.py: the cross-entropy of FixedDocsRankingLoss (src/training/
cobweb_query_train.py:116-126) restated in fp64 -- on given fp32 scores (the loss and the
softmax alone) and through the dense scorer with autograd (the whole chain) -- and the exact
rank of a target under cwq_score_topk's documented order.
"""
import numpy as np
import torch

import grad_yardstick as Y


def targets_and_temps(d64, Xq):
    """grad_yardstick.upstreams' choice: per query the third-ranked sentence of the fp64 scores
    and T = their standard deviation, rounded to float32 (the C ABI's type: every party then
    uses the same T).  Returns (targets int64 [nq], temps fp64 [nq], S64 [nq, n_sent])."""
    S = torch.stack([d64.scores(torch.tensor(x, dtype=torch.float64)) for x in Xq])
    tg = torch.argsort(-S, dim=1, stable=True)[:, 2]
    return tg.numpy().astype(np.int64), f32(S.std(dim=1, unbiased=False).numpy()), S.numpy()


def f32(t):
    """A temperature (array) rounded to float32, as fp64."""
    return np.asarray(t, np.float64).astype(np.float32).astype(np.float64)


def loss_on_scores(S32, targets, temps):
    """fp64 logsumexp(s / T) - s_t / T per query on fp32 scores (-inf columns add nothing)."""
    S = torch.as_tensor(np.asarray(S32), dtype=torch.float64)
    T = torch.as_tensor(np.broadcast_to(np.asarray(temps, np.float64), (S.shape[0],)).copy())
    t = torch.as_tensor(np.asarray(targets, np.int64))
    Z = S / T[:, None]
    return (torch.logsumexp(Z, dim=1) - Z[torch.arange(S.shape[0]), t]).numpy()


def softmax_grad_on_scores(S32, targets, temps):
    """fp64 d loss / d scores = (softmax(s / T) - onehot(t)) / T on fp32 scores, [nq, n_sent]."""
    S = torch.as_tensor(np.asarray(S32), dtype=torch.float64)
    T = torch.as_tensor(np.broadcast_to(np.asarray(temps, np.float64), (S.shape[0],)).copy())
    G = torch.softmax(S / T[:, None], dim=1)
    G[torch.arange(S.shape[0]), torch.as_tensor(np.asarray(targets, np.int64))] -= 1.0
    return (G / T[:, None]).numpy()


def torch_ce_fp32(S32, targets, temps):
    """torch.nn.functional.cross_entropy in fp32 on the same scores, per query (for the table)."""
    S = torch.as_tensor(np.asarray(S32), dtype=torch.float32)
    t = torch.as_tensor(np.asarray(targets, np.int64))
    T = np.broadcast_to(np.asarray(temps, np.float64), (S.shape[0],))
    return np.array([float(torch.nn.functional.cross_entropy(S[i:i + 1] / float(T[i]), t[i:i + 1]))
                     for i in range(S.shape[0])])


def ce_through(dense, Xq, targets, temps):
    """(loss [nq], d loss / d x [nq, D]) of CrossEntropyLoss(scores(x) / T, target) by autograd
    through the dense scorer, in the scorer's own dtype: fp64 is the yardstick, fp32 the
    reference's own arithmetic (E_ref)."""
    dt = dense.M.dtype
    T = np.broadcast_to(np.asarray(temps, np.float64), (len(Xq),))
    ce = torch.nn.CrossEntropyLoss()
    L, G = [], []
    for qi in range(len(Xq)):
        x = torch.tensor(Xq[qi], dtype=dt, requires_grad=True)
        loss = ce(dense.scores(x).unsqueeze(0) / float(T[qi]), torch.tensor([int(targets[qi])]))
        (gx,) = torch.autograd.grad(loss, [x])
        L.append(float(loss.detach()))
        G.append(gx.numpy())
    return np.array(L, np.float64), np.stack(G)


def rank_of_targets(S, targets, node_of_sentence):
    """1 + the sentences before the target: higher score, then lower node index, then lower
    sentence id.  S [nq, n_sent] (any device), exact integer count."""
    S = torch.as_tensor(S)
    dev = S.device
    t = torch.as_tensor(np.asarray(targets, np.int64), device=dev)
    node = torch.as_tensor(np.asarray(node_of_sentence, np.int64), device=dev)
    sid = torch.arange(S.shape[1], device=dev)
    st = S.gather(1, t[:, None])
    nt = node[t][:, None]
    tie = (S == st) & ((node[None, :] < nt) | ((node[None, :] == nt) & (sid[None, :] < t[:, None])))
    return 1 + ((S > st) | tie).sum(1)


def rule(e_ref):
    """The end-to-end limit: the fused path differentiates fp32 scores, as the reference does,
    so its error follows E_ref; the factor 4 is for the other summation order."""
    return max(Y.LIMIT, 4.0 * float(np.max(e_ref)))
