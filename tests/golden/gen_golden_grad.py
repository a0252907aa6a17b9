"""Generate the gradient golden g10_grad_d24.npz by running the REAL reference
(Teachable-AI-Lab/RAG-Cobweb @ 2025-09-26, mounted read-only at /root/reference).

Run:  python tests/golden/gen_golden_grad.py            (seconds on CPU)

The reference documents cobweb_rank_scores as differentiable (CobwebWrapper.py:267-294)
and trains its query encoder through it (src/training/cobweb_query_train.py:104-126).  This
script builds a small reference CobwebWrapper by its own ifit -- 200 sentences, D = 24 (no
multiple of 16 or 32), some exact duplicates so that leaves hold several sentences -- and
records the reference's own x.grad of three losses over the scores, under the default level
weights and under [1.0, 2.0, 0.5]:

    sum     scores.sum()
    wsum    (W * scores).sum(), W a fixed random-normal weighting
    ce      CrossEntropyLoss()(scores[None] / T, target[None]) -- the training loss; the
            target is the query's third-ranked sentence and T the standard deviation of its
            scores, so the softmax is not one-hot and the gradient does not vanish

Only data leaves this script (same import shim as gen_golden.py:22-36): the inputs, the tree
export in gen_golden.py's format and the reference's outputs.
"""
import os
import random
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch

_g = types.ModuleType("graphviz")
_g.Digraph = object
sys.modules["graphviz"] = _g
sys.path.insert(0, REF)
from src.cobweb.CobwebWrapper import CobwebWrapper          # noqa: E402

torch.set_num_threads(8)
WEIGHTS = [1.0, 2.0, 0.5]


class _Quiet:
    def __enter__(self):
        self._o = sys.stdout
        sys.stdout = open(os.devnull, "w")

    def __exit__(self, *a):
        sys.stdout.close()
        sys.stdout = self._o


def bfs(root):
    out, q, h = [], [root], 0
    while h < len(q):
        n = q[h]
        h += 1
        out.append(n)
        q.extend(n.children)
    return out


def export_tree(root, n_sent):
    nodes = bfs(root)
    pos = {id(n): i for i, n in enumerate(nodes)}
    parent = np.array([-1 if n.parent is None else pos[id(n.parent)] for n in nodes], np.int64)
    count = np.array([float(n.count) for n in nodes], np.float32)
    mean = np.stack([n.mean.numpy() for n in nodes]).astype(np.float32)
    meanSq = np.stack([n.meanSq.numpy() for n in nodes]).astype(np.float32)
    sid_ptr, sid_list = [0], []
    for n in nodes:
        sid_list += list(n.sentence_id or [])
        sid_ptr.append(len(sid_list))
    return dict(parent=parent, count=count, mean=mean, meanSq=meanSq, sid_ptr=np.array(sid_ptr, np.int64),
                sid_list=np.array(sid_list, np.int64), n_sent=np.int64(n_sent))


def ref_grads(w, Xq, W, target, T):
    """The reference's scores and x.grad of the three losses, per query."""
    out = {"scores": [], "sum": [], "wsum": [], "ce": []}
    ce = torch.nn.CrossEntropyLoss()
    for qi, xq in enumerate(Xq):
        for name in ("sum", "wsum", "ce"):
            x = torch.tensor(xq, requires_grad=True)
            s = w.cobweb_rank_scores(x, is_embedding=True)
            if name == "sum":
                out["scores"].append(s.detach().numpy().copy())
                loss = s.sum()
            elif name == "wsum":
                loss = (torch.tensor(W[qi]) * s).sum()
            else:
                loss = ce(s.unsqueeze(0) / float(T[qi]), torch.tensor([int(target[qi])]))
            loss.backward()
            out[name].append(x.grad.numpy().copy())
    return {k: np.stack(v).astype(np.float32) for k, v in out.items()}


def main():
    N, D, NQ = 200, 24, 8
    rng = np.random.default_rng(10)
    C = rng.normal(0, 3.0, (6, D)).astype(np.float32)
    X = (C[rng.integers(0, 6, N)] + rng.normal(0, 1.0, (N, D))).astype(np.float32)
    dup = rng.choice(N, 12, replace=False)
    X[dup] = X[rng.integers(0, N, len(dup))]          # exact duplicates: leaves with several sentences
    pick = rng.choice(N, NQ // 2, replace=False)
    Xq = np.concatenate([X[pick] + 0.1 * rng.standard_normal((NQ // 2, D)),
                         C[rng.integers(0, 6, NQ - NQ // 2)] + rng.standard_normal((NQ - NQ // 2, D))]).astype(np.float32)
    W = rng.standard_normal((NQ, N)).astype(np.float32)
    random.seed(10)
    torch.manual_seed(10)
    with _Quiet():
        w = CobwebWrapper(corpus=[f"s{i}" for i in range(N)], corpus_embeddings=X)
        w.build_prediction_index()
    tree = export_tree(w.tree.root, N)
    data = dict(X=X, Xq=Xq, W=W, prior_var=np.float32(w.tree.prior_var), weights_w3=np.array(WEIGHTS, np.float64), **tree)
    for tag, weights in (("", None), ("_w3", WEIGHTS)):
        with _Quiet():
            if weights is not None:
                w.set_level_weights(weights)
            w.build_prediction_index()
            s0 = np.stack([w.cobweb_rank_scores(torch.tensor(x), is_embedding=True).numpy() for x in Xq])
        target = np.argsort(-s0, axis=1, kind="stable")[:, 2].astype(np.int64)
        T = s0.astype(np.float64).std(axis=1)
        with _Quiet():
            r = ref_grads(w, Xq, W, target, T)
        data["ce_target" + tag] = target
        data["ce_T" + tag] = T
        data["rank_scores" + tag] = r["scores"]
        for name in ("sum", "wsum", "ce"):
            data[f"grad_{name}{tag}"] = r[name]
    multi = int(np.sum(np.diff(tree["sid_ptr"]) > 1))
    np.savez_compressed(os.path.join(OUT, "g10_grad_d24.npz"), **data)
    print(f"[g10_grad_d24] N={N} D={D} nodes={len(tree['parent'])} multi-sentence nodes={multi} "
          f"depth={int(max(len(p) for p in w._leaf_to_path_indices))}")


if __name__ == "__main__":
    main()
