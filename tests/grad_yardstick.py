"""The yardstick of the gradient tests: torch autograd on the CPU through a dense restatement
of the reference's score expression (CobwebWrapper.py:283-292), written out from a golden's
tree arrays with the path matrix weight[depth] / len(path) (CobwebWrapper.py:160-169).

fp64 is the yardstick; the same restatement in fp32 is what the reference itself computes,
and its error against fp64 (E_ref) is printed beside the kernel's.
"""
import numpy as np
import torch

from oracle import cobweb_oracle as O

LIMIT = 1e-5   # the project's RTOL for scores
DEFAULT_W = [1.0] * 6


def tree_arrays(g):
    """(mean fp32, var fp32, parent, node_of_sentence) of a golden's tree export."""
    var = O.compute_var(g["meanSq"], g["count"][:, None])
    var[g["count"] == 0] = O.PRIOR_VAR
    nos = np.full(int(g["n_sent"]), -1, np.int64)
    for i in range(len(g["parent"])):
        for s in g["sid_list"][g["sid_ptr"][i]:g["sid_ptr"][i + 1]]:
            nos[s] = i
    return g["mean"].astype(np.float32), var.astype(np.float32), g["parent"].astype(np.int64), nos


def path_matrix(parent, nos, weights=None, sparse=False):
    """Dense [n_sent, n_nodes] fp64: weight[depth] / len(path) on every node of a sentence's
    root-to-node path (weight 1.0 past the list); a sentence outside the tree has a zero row.
    sparse=True: the same matrix as a torch sparse tensor (the large synthetic trees)."""
    w = DEFAULT_W if weights is None else list(weights)
    if sparse:
        par = np.asarray(parent)
        depth = np.zeros(len(par), np.int64)
        for i in range(1, len(par)):
            depth[i] = depth[par[i]] + 1
        rows, cols, vals = [], [], []
        for s, n in enumerate(nos):
            j, L = int(n), int(depth[n]) + 1 if n >= 0 else 0
            while j >= 0:
                d = int(depth[j])
                rows.append(s)
                cols.append(j)
                vals.append((w[d] if d < len(w) else 1.0) / L)
                j = int(par[j])
        return torch.sparse_coo_tensor(torch.tensor([rows, cols]), torch.tensor(vals, dtype=torch.float64),
                                       (len(nos), len(par))).coalesce()
    P = np.zeros((len(nos), len(parent)), np.float64)
    for s, n in enumerate(nos):
        path, j = [], int(n)
        while j >= 0:
            path.append(j)
            j = int(parent[j])
        path = path[::-1]
        for d, node in enumerate(path):
            P[s, node] = (w[d] if d < len(w) else 1.0) / len(path)
    return P


class Dense:
    """The restated scorer in one dtype."""

    def __init__(self, mean, var, P, dtype):
        self.M = torch.tensor(mean, dtype=dtype)
        self.V = torch.tensor(var, dtype=dtype)
        self.P = P.to(dtype) if torch.is_tensor(P) else torch.tensor(P, dtype=dtype)
        self.logdet = torch.log(self.V).sum(dim=1)

    def scores(self, x):
        """x [D] -> [n_sent] (CobwebWrapper.py:283-292)."""
        diff_sq = (x.unsqueeze(0) - self.M) ** 2
        lp = -0.5 * (self.logdet + (diff_sq / self.V).sum(dim=1))
        if self.P.is_sparse:
            return torch.sparse.mm(self.P, lp.unsqueeze(1)).squeeze(1)
        return (self.P @ lp.unsqueeze(1)).squeeze(1)


def upstreams(d64, Xq, seed=0, targets=None, temps=None):
    """Per query the fp64 scores and the three upstream cases.  Returns (S [nq, n_sent] fp64,
    cases): cases[name] = (G [nq, n_sent] fp64 = dloss/dscores, grad_x [nq, D] fp64).
    ce: CrossEntropyLoss on scores / T with a target that is not the top-1 (the third-ranked
    sentence) and T the standard deviation of the query's fp64 scores, unless given."""
    nq, ns = len(Xq), d64.P.shape[0]
    W = torch.tensor(np.random.default_rng(seed).standard_normal((nq, ns)))
    ce = torch.nn.CrossEntropyLoss()
    out = {k: ([], []) for k in ("sum", "wsum", "ce")}
    S = []
    for qi in range(nq):
        for name in out:
            x = torch.tensor(Xq[qi], dtype=torch.float64, requires_grad=True)
            s = d64.scores(x)
            if name == "sum":
                S.append(s.detach().numpy().copy())
                loss = s.sum()
            elif name == "wsum":
                loss = (W[qi] * s).sum()
            else:
                sd = s.detach()
                tgt = int(torch.argsort(-sd, stable=True)[2]) if targets is None else int(targets[qi])
                T = float(sd.std(unbiased=False)) if temps is None else float(temps[qi])
                loss = ce(s.unsqueeze(0) / T, torch.tensor([tgt]))
            G, gx = torch.autograd.grad(loss, [s, x])
            out[name][0].append(G.numpy())
            out[name][1].append(gx.numpy())
    return np.stack(S), {k: (np.stack(v[0]), np.stack(v[1])) for k, v in out.items()}


def grad_through(dense, Xq, G):
    """grad_x of sum(G * scores) by autograd in the scorer's own dtype (the reference's
    fp32 arithmetic when dense is fp32)."""
    out = []
    for qi in range(len(Xq)):
        x = torch.tensor(Xq[qi], dtype=dense.M.dtype, requires_grad=True)
        (gx,) = torch.autograd.grad((torch.tensor(G[qi], dtype=dense.M.dtype) * dense.scores(x)).sum(), [x])
        out.append(gx.numpy())
    return np.stack(out)


def rel_l2(g, g64):
    """Per query |g - g64|_2 / |g64|_2."""
    g = np.asarray(g, np.float64)
    g64 = np.asarray(g64, np.float64)
    return np.linalg.norm(g - g64, axis=1) / np.linalg.norm(g64, axis=1)
