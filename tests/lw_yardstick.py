"""Yardstick of the level-weight tests (tests/test_level_weights_cpu.py,
tests/test_gpu_level_weights.py), beside grad_yardstick.py and ce_yardstick.py: the dense
restatement of the reference's score expression (CobwebWrapper.py:283-292) with its path matrix
(CobwebWrapper.py:160-169) written as

    P(w) = sum_d w[d] A_d,    A_d[s, n] = 1 / L_s  if n is the depth-d node of s's path,

so that the level weights w are a torch leaf: loss, d/dx and d/dw come from autograd in a given
dtype.  fp64 is the yardstick; fp32 is the reference's own arithmetic and gives E_ref.  A depth
past the end of w weighs 1.0 (CobwebWrapper.py:166); a weight past the tree's depth is unused
and has a zero gradient.
"""
import numpy as np
import torch

import ce_yardstick as C
import grad_yardstick as Y

# The weight vectors of the tests: the defaults, a 3-vector (shorter than the depth-6 trees), a
# zero weight, and ten levels of exponential decay (longer than the flat and two-level trees).
WEIGHTS = {"default": list(Y.DEFAULT_W), "w3": [1.0, 2.0, 0.5], "zero": [1.0, 0.0, 1.0],
           "exp10": [0.5 ** i for i in range(10)]}


def depth_matrices(parent, nos):
    """The A_d stacked as one sparse fp64 matrix [n_levels * n_sent, n_nodes], row d * n_sent + s
    (n_levels = the tree's depth + 1); returns (n_levels, matrix)."""
    parent = np.asarray(parent)
    depth = np.zeros(len(parent), np.int64)
    for i in range(1, len(parent)):
        depth[i] = depth[parent[i]] + 1
    nl, ns = int(depth.max()) + 1, len(nos)
    rows, cols, vals = [], [], []
    for s, n in enumerate(nos):
        j, L = int(n), int(depth[n]) + 1 if n >= 0 else 0
        while j >= 0:
            rows.append(int(depth[j]) * ns + s)
            cols.append(j)
            vals.append(1.0 / L)
            j = int(parent[j])
    A = torch.sparse_coo_tensor(torch.tensor([rows, cols]), torch.tensor(vals, dtype=torch.float64),
                                (nl * ns, len(parent))).coalesce()
    return nl, A


class DenseW:
    """The restated scorer in one dtype, the level weights an argument."""

    def __init__(self, mean, var, A, dtype):
        self.dtype = dtype
        self.M = torch.tensor(mean, dtype=dtype)
        self.V = torch.tensor(var, dtype=dtype)
        self.nl, self.A = A[0], A[1].to(dtype)
        self.ns = self.A.shape[0] // self.nl
        self.logdet = torch.log(self.V).sum(dim=1)

    def full(self, w):
        """w cut or padded with ones to the tree's levels (torch ops: differentiable)."""
        if w.shape[0] >= self.nl:
            return w[:self.nl]
        return torch.cat([w, torch.ones(self.nl - w.shape[0], dtype=w.dtype)])

    def path_matrix(self, w):
        """sum_d w[d] A_d, dense [n_sent, n_nodes]."""
        return torch.tensordot(self.full(w), self.A.to_dense().view(self.nl, self.ns, -1), dims=1)

    def lp(self, x):
        return -0.5 * (self.logdet + (((x.unsqueeze(0) - self.M) ** 2) / self.V).sum(dim=1))

    def scores(self, x, w):
        """x [D], w [n_w] -> [n_sent]: (sum_d w[d] A_d) lp, the sum over d taken last."""
        B = torch.sparse.mm(self.A, self.lp(x).unsqueeze(1)).view(self.nl, self.ns)
        return self.full(w) @ B

    def fixed(self, w):
        """grad_yardstick.Dense under these weights (for targets_and_temps / upstreams)."""
        d = Y.Dense.__new__(Y.Dense)
        d.M, d.V, d.logdet = self.M, self.V, self.logdet
        d.P = self.path_matrix(torch.as_tensor(np.asarray(w, np.float64)).to(self.dtype)).detach()
        return d


def leaves(dense, x, w):
    return (torch.tensor(np.asarray(x), dtype=dense.dtype, requires_grad=True),
            torch.tensor(np.asarray(w, np.float64), dtype=dense.dtype, requires_grad=True))


def ce_through(dense, Xq, targets, temps, w):
    """(loss [nq], d loss / d x [nq, D], d loss / d w [nq, n_w]) of CrossEntropyLoss(scores(x, w)
    / T, target) per query by autograd in the scorer's dtype."""
    T = np.broadcast_to(np.asarray(temps, np.float64), (len(Xq),))
    ce = torch.nn.CrossEntropyLoss()
    L, GX, GW = [], [], []
    for qi in range(len(Xq)):
        x, wt = leaves(dense, Xq[qi], w)
        loss = ce(dense.scores(x, wt).unsqueeze(0) / float(T[qi]), torch.tensor([int(targets[qi])]))
        gx, gw = torch.autograd.grad(loss, [x, wt])
        L.append(float(loss.detach()))
        GX.append(gx.numpy())
        GW.append(gw.numpy())
    return np.array(L, np.float64), np.stack(GX), np.stack(GW)


def grad_through(dense, Xq, G, w):
    """(d/dx [nq, D], d/dw [nq, n_w]) of sum(G[q] * scores(x_q, w)) per query."""
    GX, GW = [], []
    for qi in range(len(Xq)):
        x, wt = leaves(dense, Xq[qi], w)
        gx, gw = torch.autograd.grad((torch.tensor(G[qi], dtype=dense.dtype) * dense.scores(x, wt)).sum(), [x, wt])
        GX.append(gx.numpy())
        GW.append(gw.numpy())
    return np.stack(GX), np.stack(GW)


def targets_and_temps(d64, Xq, w):
    """ce_yardstick.targets_and_temps under the weights in use."""
    return C.targets_and_temps(d64.fixed(w), Xq)


def upstreams(d64, Xq, w, targets, temps):
    """grad_yardstick.upstreams under the weights in use: cases[name] = G [nq, n_sent] fp64."""
    _, cases = Y.upstreams(d64.fixed(w), Xq, targets=targets, temps=temps)
    return {k: v[0] for k, v in cases.items()}
