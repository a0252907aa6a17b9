"""Yardsticks of the sparse differentiable scores, beside grad_yardstick.py and
ce_yardstick.py: in fp64, on given scores,

  * the candidate set C of a query under cwq_score_topk's documented order (higher score, then
    lower node index, then lower sentence id; sentences outside the tree never) -- the top K plus
    the target when it is not among them,
  * the truncated loss (m - s_t)/T + log z over C, its gradient with respect to the scores
    (softmax - one-hot restricted to C, zero elsewhere) and the rank capped at K + 1,
  * the bound log1p((n_tree - |C|) exp((s_K - m)/T) / z) on what the truncation leaves out,

and the gathered form of the backward: grad_x of sum_j g_j score(ids_j) from the listed
sentences' paths alone.
"""
import numpy as np

import grad_yardstick as Y


def order(s_row, nos):
    """Sentence ids of the tree in cwq_score_topk's order for one query's scores."""
    nos = np.asarray(nos, np.int64)
    sid = np.arange(len(nos))
    o = np.lexsort((sid, nos, -np.asarray(s_row, np.float64)))
    return o[nos[o] >= 0]


def truncated(S, nos, targets, temps, K):
    """Per query over scores S [nq, n_sent] (any float dtype; evaluated in fp64): dict of
    cand (list of id arrays: the top K in order), loss [nq], G [nq, n_sent] = d loss / d scores,
    bound [nq], rank [nq] (exact inside the top K, else K + 1; -1 for an invalid target)."""
    S = np.asarray(S, np.float64)
    nos = np.asarray(nos, np.int64)
    nq, ns = S.shape
    T = np.broadcast_to(np.asarray(temps, np.float64), (nq,))
    n_tree = int((nos >= 0).sum())
    out = {"cand": [], "loss": np.zeros(nq), "G": np.zeros((nq, ns)), "bound": np.zeros(nq),
           "rank": np.zeros(nq, np.int64)}
    for q in range(nq):
        top = order(S[q], nos)[:K]
        out["cand"].append(top)
        t = int(targets[q])
        if t < 0 or t >= ns or nos[t] < 0:
            out["loss"][q], out["rank"][q] = np.inf, -1
            continue
        inside = np.nonzero(top == t)[0]
        C = top if len(inside) else np.r_[top, t]
        s = S[q, C]
        m = s.max()
        e = np.exp((s - m) / T[q])
        z = e.sum()
        out["loss"][q] = (m - S[q, t]) / T[q] + np.log(z)
        g = e / z
        g[np.nonzero(C == t)[0][0]] -= 1.0
        out["G"][q, C] = g / T[q]
        out["rank"][q] = inside[0] + 1 if len(inside) else K + 1
        if n_tree >= K:
            out["bound"][q] = np.log1p((n_tree - len(C)) * np.exp((S[q, top[K - 1]] - m) / T[q]) / z)
    return out


def gathered_grad(mean, var, parent, nos, x, ids, g, weights=None):
    """grad_x of sum_j g[j] score(ids[j]) in fp64 from the listed sentences' paths: the
    coefficient weight[depth] / len(path) g[j] summed per node, then -sum coef (x - mu) / v over
    the distinct nodes.  Entries without a node are skipped; duplicates add."""
    w = Y.DEFAULT_W if weights is None else list(weights)
    coef = {}
    for sid, gj in zip(ids, g):
        sid = int(sid)
        if sid < 0 or sid >= len(nos) or nos[sid] < 0:
            continue
        path, j = [], int(nos[sid])
        while j >= 0:
            path.append(j)
            j = int(parent[j])
        path = path[::-1]
        for d, node in enumerate(path):
            coef[node] = coef.get(node, 0.0) + (w[d] if d < len(w) else 1.0) / len(path) * float(gj)
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    for node, c in coef.items():
        out -= c * (x - mean[node].astype(np.float64)) / var[node].astype(np.float64)
    return out
