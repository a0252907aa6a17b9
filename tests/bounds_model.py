"""Adversarial rounding fixtures for the filters' certified bounds, and a numpy model of the
bound for judging them (never for comparison with GPU numbers).

The filters (cwq_mfma.hip, cwq_stream.hip) bound an isotropic row's Fast key from the dot
product of the operands' hi parts: x'.mu' - x_hi.mu_hi = x_hi.mu_lo + x_lo.mu_hi + x_lo.mu_lo,
each term bounded by Cauchy-Schwarz (fg_bounds2, cwq_internal.h).  On Gaussian data the
residuals x_lo, mu_lo have random signs, the real error is ~1/sqrt(D) of the bound, and a
bound that is too narrow by a large factor still returns the exact scan's answer.  The
fixtures here make one term at a time tight: residuals of one sign in every dimension,
aligned with the other operand, on rows whose true keys are placed so that a bound a few
percent too narrow drops a true top-k row.

The model: `split` restates the operand splits (bf16 round-to-nearest-even; the int8 split of
i8_split_wave), `model_bounds` is fg_bounds2 in fp64 for a flat tree with the real constants
(filt_consts, PRIOR_VAR, the level weights), with one factor per split term (with `consts` /
`cent`: another tree's leaves, group-centred rows, Basic's key), `model_filter` is the final
pass (T2 = k-th largest l, survivors u >= T2).  `flip_factor` is the largest
factor on a fixture's targeted term at which the model loses a true top-k row.

Fixture layout (flat tree, root mean exactly 0 -- the filter's centre -- root var 1, every
leaf PRIOR_VAR).  Per engineered group a query x, `kmax` "top" rows (the true top-kmax) and
`kmax` "bottom" rows (the next kmax), keys `GAP`*|score| apart in fp64.  A row is its role's
base value in every dimension (int8: in all but the last, which is 127 steps and pins the
scale), moved 1, 2, 4 or 8 lattice steps up in n_up dimensions and one down in n_dn others;
(n_up, n_dn) comes from a greedy walk over the lattice in order of distance from x.  bf16
values lie four steps inside their binade (a = 132 units), so no step or residual leaves it:
  upper   x = a.  top: victims a + t (t = 0.45 units, so mu_lo = t.1 is aligned with x_hi
          and the hi-only key is too low by 2|hs||x_hi||mu_lo|); bottom: anchors, exact.
  lower   top: anchors, exact; bottom: decoys a - t (the hi-only key is too high).
  qside   x = a + t.  Exact rows: victims 2a (large |mu_hi| aligned with x_lo), anchors 0
          (small |mu_hi|; the lattice moves some dimensions towards x).
  both    as qside with victims 2a + t: all three terms coherent at once.  The targeted
          factor scales all three: x_lo.mu_lo alone is below 2^-16 (bf16) of x.mu, always
          inside the slack term, so no fixture can detect a fault of that term alone.
int8 fixtures hold two groups whose scales differ by 2^6, rows interleaved and queries
adjacent, so that a scale read from the neighbouring query or row is off by 64.

Measured flip factors (model, D = 64, `python tests/bounds_model.py` prints the table; the
floor is the slack margin plus the kmax key gaps between the lost row and the threshold):

  fixture            term(s) scaled       bf16 k = 1 / 10 / 64    int8 k = 1 / 10 / 64
  upper              x_hi.mu_lo           0.92 / 0.92 / 0.92      0.91 / 0.91 / 0.91
  lower              x_hi.mu_lo           0.92 / 0.92 / 0.92      0.92 / 0.91 / 0.94
  qside              x_lo.mu_hi           0.94 / 0.89 / 0.67      0.84 / 0.81 / 0.56
  both               all three            0.97 / 0.95 / 0.83      0.88 / 0.86 / 0.80
  both               x_lo.mu_lo alone     0 (never lost)          0 (never lost)
  grouped upper      x_hi.M_lo            0.91 / 0.89 / -         -
  grouped lower      x_hi.M_lo            0.91 / 0.91 / -         -
  both, 10 over 64   all three, Basic key 0.80 (k = 10)           0.70 (k = 10)
qside at k = 64 stays below 0.75 (FLIP_MIN): its rows are |x| away from the query, |score| is
~|hs||x|^2, and 64 key gaps take up to 40% of the coherent error 4|hs||x_lo||mu_hi|.
"""
import math
import os
import sys

import numpy as np

if __name__ == "__main__":   # the table printer, run from anywhere
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cobweb_oracle as O

PRIOR_VAR = float(O.PRIOR_VAR)
DEFAULT_W = (1.0,) * 6      # index.DEFAULT_LEVEL_WEIGHTS
RTOL = 1e-5                 # the project's tolerance on scores
GAP = 1.2e-4                # fp64 key gap between consecutive engineered ranks, relative to |score| (> 1e-4)
UP = 1.0 + 2.0 ** -20       # up() of cwq_mfma.hip: norms are rounded up a little
FG_TILE = 256
MULTS = (1, 2, 4, 8)        # lattice: steps up
R_LO = 0.45                 # residual in units (below the half unit at which the split would round away)


def dpb(D):
    """fgemm_dpb: whole 64-wide stages, at least two."""
    return max((D + 63) // 64 * 64, 128)


def filt_consts(D, operand):
    """filt_consts (cwq_handle.h): gamma, eps_n, slack; the int8 dot is exact (gamma 0)."""
    return ((dpb(D) + 64) * 2.0 ** -23 if operand == "bf16" else 0.0, 2.0 ** -20, 2.0 ** -16)


def bf16_round(v):
    """Round-to-nearest-even to bf16, returned as float32."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split(v, operand):
    """hi, lo (fp64, hi + lo == v exactly) of each row of the fp32 array v [n, D]."""
    v = np.atleast_2d(np.asarray(v, np.float32))
    if operand == "bf16":
        hi = bf16_round(v).astype(np.float64)
        return hi, v.astype(np.float64) - hi
    s = (np.abs(v).max(axis=1) / np.float32(127.0)).astype(np.float32)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(s > 0, np.clip(np.rint(v / s), -127, 127), 0).astype(np.float64)
    hi = s.astype(np.float64) * q
    return hi, v.astype(np.float64) - hi


def flat_consts(x, D, weights=DEFAULT_W):
    """Flat tree, root N(0, 1): pi [nq] = w0 lp'(root) / 2, hs, hl of a depth-1 leaf."""
    w = list(weights) + [1.0] * 2
    pi = 0.5 * w[0] * (-0.5 * (np.asarray(x, np.float64) ** 2).sum(axis=-1))
    cw = 0.5 * w[1]
    return pi, -0.5 * cw / PRIOR_VAR, -0.5 * cw * D * math.log(PRIOR_VAR)


def two_level_consts(x, D, centres, cluster, cvar, weights=DEFAULT_W):
    """Root N(0, 1) -> clusters N(centre, cvar) -> leaves: pi [nq, n] = (w0 lp'(root) +
    w1 lp'(cluster of the row)) / 3, hs, hl of a depth-2 leaf."""
    w = list(weights) + [1.0] * 3
    x = np.atleast_2d(np.asarray(x, np.float64))
    c = np.asarray(centres, np.float64)
    lpr = -0.5 * (x * x).sum(1)
    dc = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * x @ c.T
    lpc = -0.5 * (D * math.log(cvar) + dc / cvar)
    cw = w[2] / 3.0
    return (w[0] * lpr[:, None] + w[1] * lpc[:, cluster]) / 3.0, -0.5 * cw / PRIOR_VAR, -0.5 * cw * D * math.log(PRIOR_VAR)


def true_keys(x, rows, weights=DEFAULT_W, consts=None):
    """fp64 Fast keys [nq, n] of the leaves (consts: (pi, hs, hl); default: a flat tree)."""
    x = np.atleast_2d(np.asarray(x, np.float32)).astype(np.float64)
    m = np.asarray(rows, np.float32).astype(np.float64)
    pi, hs, hl = consts if consts is not None else flat_consts(x, m.shape[1], weights)
    S = (x * x).sum(1)[:, None] + (m * m).sum(1)[None, :] - 2.0 * x @ m.T
    return (pi[:, None] if pi.ndim == 1 else pi) + hl + hs * S


def model_bounds(x, rows, operand, scale=(1, 1, 1), weights=DEFAULT_W, consts=None, cent=None):
    """fg_bounds2 in fp64: (u, l) [nq, n].  scale multiplies the split terms |x_hi||mu_lo|,
    |x_lo||mu_hi|, |x_lo||mu_lo| separately.  Default: a flat tree whose root mean is 0.
    consts = (pi, hs, hl): another tree's prefix term and leaf coefficients.  cent [n, D]:
    group-centred rows (cwq_group.hip; the root mean still 0): the row operand is M = fl(mu -
    cent), the term -2 x.cent moves into the prefix, and the fp32 rounding of M adds
    2^-23 |M| to both split norms."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    rows = np.asarray(rows, np.float32)
    D = rows.shape[1]
    gamma, eps_n, slack = filt_consts(D, operand)
    xh, xl = split(x, operand)
    M = rows if cent is None else (rows - np.asarray(cent, np.float32)).astype(np.float32)
    mh, ml = split(M, operand)
    norm = lambda v: np.sqrt((v * v).sum(1)) * UP
    a, c, d, b = norm(xh)[:, None], norm(xl)[:, None], norm(mh)[None, :], norm(ml)[None, :]
    ge = 0.0 if cent is None else 2.0 ** -23 * UP * norm(M.astype(np.float64))[None, :]
    pi, hs, hl = consts if consts is not None else flat_consts(x, D, weights)
    pi = pi[:, None] if pi.ndim == 1 else pi
    x64 = x.astype(np.float64)
    n2 = (x64 ** 2).sum(1)[:, None] + (rows.astype(np.float64) ** 2).sum(1)[None, :]
    dot = xh @ mh.T
    shift = 0.0 if cent is None else x64 @ np.asarray(cent, np.float64).T     # exact, in the prefix
    eextra = (2.0 ** -23 if operand == "bf16" else 2.0 ** -21) * np.abs(dot)
    kr = hs * (n2 - 2.0 * dot - 2.0 * shift) + hl
    ES = 2.0 * (scale[0] * a * (b + ge) + gamma * a * d + scale[1] * c * (d + ge) + scale[2] * c * b
                + eextra) + eps_n * n2
    err = abs(hs) * ES + slack * (np.abs(pi) + abs(hl) + 3.0 * abs(hs) * n2)
    return pi + kr + err, pi + kr - err


def basic_consts(x, D):
    """Basic's key on a flat tree's leaf (cwq_build.hip build_filter, cat): the full log-density
    lp = -(logdet + D log 2 pi) / 2 - iv S / 2, no prefix term.  The filter takes it min'ed
    with the root's lp, so it orders only rows whose lp is below that."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    return np.zeros(len(x)), -0.5 / PRIOR_VAR, -0.5 * D * (math.log(PRIOR_VAR) + math.log(2.0 * math.pi))


def fp64_topk(keys, k):
    """Ids of the k largest keys of one query, ties to the lower id (the project's order)."""
    return np.lexsort((np.arange(keys.size), -keys))[:k]


def final_pass(u, l, key, k):
    """Per query: T2 = k-th largest l, survivors u >= T2.  A list of dicts: T2, survivors
    (count), top (fp64 top-k ids), lost (the ids of the true top-k that do not survive),
    enclosed (l <= key <= u for every row)."""
    out = []
    for qi in range(u.shape[0]):
        T2 = np.partition(l[qi], -k)[-k]
        top = fp64_topk(key[qi], k)
        out.append(dict(T2=T2, survivors=int((u[qi] >= T2).sum()), top=top, lost=top[u[qi, top] < T2],
                        enclosed=bool(((l[qi] <= key[qi]) & (key[qi] <= u[qi])).all())))
    return out


def model_filter(x, rows, k, operand, scale=(1, 1, 1), weights=DEFAULT_W, consts=None, cent=None):
    """The final pass on the model's bounds: whether the true top-k (fp64 keys) survives."""
    u, l = model_bounds(x, rows, operand, scale, weights, consts, cent)
    return final_pass(u, l, true_keys(x, rows, weights, consts), k)


# ----------------------------------------------------------------------------------------
# engineered groups
# ----------------------------------------------------------------------------------------
KINDS = ("upper", "lower", "qside", "both")
TARGET = {"upper": (0,), "lower": (0,), "qside": (1,), "both": (0, 1, 2)}   # the scaled split terms


def target_scale(kind, f):
    return tuple(f if i in TARGET[kind] else 1.0 for i in range(3))


class Group:
    """One engineered query with its rows: x [D] fp32, rows [2 kmax, D] fp32 in rank order (the
    first kmax are the true top-kmax), unit (the split's step at the engineered values)."""

    def __init__(self, x, rows, kmax, unit):
        self.x, self.rows, self.kmax, self.unit = x, rows, kmax, unit


def _group(kind, operand, D, kmax, unit, weights=DEFAULT_W, gap_s=None, nbot=None):
    """unit: bf16: the ulp of the binade of the query's values a = 132 units; int8:
    the step s (a power of two; rows and query have one component 127 s, the last)."""
    i8 = operand == "int8"
    nd = D - 1 if i8 else D          # engineered dimensions
    t = R_LO * unit
    # bf16: four steps above the binade's edge, so that no lattice step or residual leaves it
    a = unit * ((64 if kind in ("upper", "lower") else 60) if i8 else 132)
    far = kind in ("qside", "both")
    xd = np.float32(a + (t if far else 0.0))       # the query's value in every engineered dimension

    # roles (top, bottom): base value, residual in units of the base's own step, lattice step,
    # share of the dimensions the lattice may move
    u2 = unit if i8 else 2 * unit                  # the step at 2a
    if kind == "upper":
        roles = ((a, t, unit, 2), (a, 0.0, unit, 2))
    elif kind == "lower":
        roles = ((a, 0.0, unit, 2), (a, -t, unit, 2))
    else:
        roles = ((2 * a, 0.0 if kind == "qside" else R_LO * u2, u2, 8), (0.0, 0.0, 4 * unit, 2))

    def row(base, lo, step, n_up, n_dn, mult=1):
        v = np.full(D, base + lo, np.float64)
        v[:n_up] += mult * step
        v[n_up:n_up + n_dn] -= step
        if i8:
            v[D - 1] = 127.0 * unit
        return v.astype(np.float32)

    def lattice(base, lo, step, share):
        """(S, n_up, n_dn, mult) ascending in S = |row - x|^2 (fp64, from the rows' fp32 values):
        n_up dimensions mult steps up, n_dn dimensions one step down."""
        c = lambda sh: (np.float64(np.float32(base + lo + sh)) - np.float64(xd)) ** 2
        n = np.arange(nd // share + 1)
        S = np.stack([nd * c(0.0) + n[:, None] * (c(m * step) - c(0.0)) + n[None, :] * (c(-step) - c(0.0))
                      for m in MULTS])
        S[1:, 0, :] = np.inf                        # n_up = 0: the same row for every mult
        order = np.argsort(S, axis=None)
        order = order[np.isfinite(S.flat[order])]
        mi, nu, ndn = np.unravel_index(order, S.shape)
        return zip(S.flat[order], nu, ndn, np.asarray(MULTS)[mi])

    x = np.full(D, xd, np.float32)
    if i8:
        x[D - 1] = 127.0 * unit
    _, hs, _ = flat_consts(x, D, weights)
    score = float(true_keys(x, row(*roles[0][:3], 0, 0)[None], weights)[0, 0])
    if gap_s is None:                              # (given: a tree whose keys are not the flat tree's)
        gap_s = GAP * abs(score) / abs(hs)
    rows, S_prev = [], -np.inf
    for (base, lo, step, share), count in zip(roles, (kmax, nbot or kmax)):
        picked = 0
        for S, n_up, n_dn, mult in lattice(base, lo, step, share):
            if S >= S_prev + gap_s:
                rows.append(row(base, lo, step, int(n_up), int(n_dn), int(mult)))
                S_prev, picked = S, picked + 1
                if picked == count:
                    break
        assert picked == count, "the lattice does not reach the rows before it"
    return Group(x, np.stack(rows), kmax, unit)


def groups(kind, operand, D, kmax, nbot=None):
    """The fixture's engineered groups: bf16: one, a ~ 2 (upper, lower: |score| is small
    there) or ~0.5 (qside, both: the rows are |x| away, and 0.5 keeps |score| low against the
    coherent error); int8: two, steps 2^-5 and 2^1 (upper, lower) or 2^-7 and 2^-1."""
    near = kind in ("upper", "lower")
    if operand == "bf16":
        return [_group(kind, operand, D, kmax, 2.0 ** -6 if near else 2.0 ** -8, nbot=nbot)]
    s = 2.0 ** -5 if near else 2.0 ** -7
    return [_group(kind, operand, D, kmax, s, nbot=nbot), _group(kind, operand, D, kmax, 64 * s, nbot=nbot)]


class Fixture:
    """rows [N, D] fp32 (filter row r = leaf node r + 1 = sentence r), the engineered queries
    xq [n_groups, D], per group the filter rows of its engineered rows in rank order."""

    def __init__(self, kind, operand, D, kmax, rows, xq, eng):
        self.kind, self.operand, self.D, self.kmax, self.rows, self.xq, self.eng = kind, operand, D, kmax, rows, xq, eng
        self.free = np.setdiff1d(np.arange(len(rows)), np.concatenate(eng))   # the background rows

    def model_args(self, x, idx):
        """model_bounds' consts / cent for the queries x and the rows idx (a flat tree: none)."""
        return {}

    def keys(self, weights=DEFAULT_W):
        """fp64 keys [n_groups, N] of the engineered queries."""
        return true_keys(self.xq, self.rows, weights, **{k: v for k, v in self.model_args(
            self.xq, np.arange(len(self.rows))).items() if k == "consts"})

    def model(self, k, scale=(1, 1, 1), idx=None):
        """model_filter of the engineered queries over the rows idx (default: all; those bounds
        are kept for the next k)."""
        if idx is None and scale == (1, 1, 1) and getattr(self, "_full", None) is not None:
            return final_pass(*self._full, k)
        rows = self.rows if idx is None else self.rows[idx]
        args = self.model_args(self.xq, np.arange(len(self.rows)) if idx is None else idx)
        u, l = model_bounds(self.xq, rows, self.operand, scale, **args)
        key = true_keys(self.xq, rows, consts=args.get("consts"))
        if idx is None and scale == (1, 1, 1):
            self._full = (u, l, key)
        return final_pass(u, l, key, k)

    def tree(self):
        """(mean, var, parent, node_of_sentence) for CobwebIndex."""
        N, D = self.rows.shape
        mean = np.concatenate([np.zeros((1, D), np.float32), self.rows])
        var = np.full((N + 1, D), np.float32(PRIOR_VAR), np.float32)
        var[0] = 1.0
        parent = np.zeros(N + 1, np.int64)
        parent[0] = -1
        return mean, var, parent, np.arange(1, N + 1, dtype=np.int64)

    def queries(self, nq, slots=(0,), seed=5):
        """[nq, D]: ordinary queries (perturbed background rows), with the engineered queries at
        slots s, s + 1, ... (one per group) for every s in slots."""
        rng = np.random.default_rng(seed)
        Q = self.rows[rng.choice(self.free, nq)] + 0.2 * rng.standard_normal((nq, self.D)).astype(np.float32)
        where = {}
        for s in slots:
            for g in range(len(self.xq)):
                if 0 <= s + g < nq:
                    where[s + g] = g          # a later slot overrides an earlier one
        for s, g in where.items():
            Q[s] = self.xq[g]
        return Q.astype(np.float32), sorted(where.items())


def sample_stride(N):
    """The stride of the filter's threshold sample (cwq_build.hip build_filter): rows 0, stride, ..."""
    return max(1, N // min(32768, max(FG_TILE, N // 128 // FG_TILE * FG_TILE)))


def positions(N, n_groups, kmax, place, nbot=None):
    """Filter rows of the engineered rows: per group an array in rank order (top rows first).
    The groups' rows are interleaved, so that neighbouring rows differ in scale.
    front: rows 0, 1, ..., a group's top and bottom rows in turn.
    tiles: the pretest reads a tile's beta_max / delta_max, and it drops a row only when the
    threshold is already tight as the row's tile is processed -- so the bottom rows come
    early (one per group in the threshold sample: row 0, of two groups the second's, and row
    `stride`; the others from row 1 on: candidates of the first launch), a group's best top
    row is the last row of tile 0 (of two groups: the second's, whose scale is the larger;
    the first's -- of one group: its second best -- is the first row of tile 1), and the other
    top rows are the last rows of the last row tile (N not a multiple of 256: the partial
    tile)."""
    n = 2 * kmax
    if place == "front" and nbot not in (None, kmax):      # (unequal counts: plainly in rank order)
        return [np.arange(g, n_groups * (kmax + nbot), n_groups) for g in range(n_groups)]
    if place == "front":
        turn = np.argsort(np.arange(n).reshape(2, kmax).T.ravel())
        return [np.arange(g, n_groups * n, n_groups)[turn] for g in range(n_groups)]
    assert place == "tiles" and n_groups * (kmax - 1) <= (N - 1) % FG_TILE + 1 and n_groups * kmax < sample_stride(N)
    out = []
    for g in range(n_groups):
        last = g == n_groups - 1
        top = np.concatenate([[255 if last else 256], N - n_groups * (kmax - 1) + g + n_groups * np.arange(kmax - 1)])
        if n_groups == 1:
            top[1] = 256
        bot = np.concatenate([[0 if last else sample_stride(N)], 1 + g + n_groups * np.arange(kmax - 1)])
        out.append(np.concatenate([top, bot]))
    return out


def fixture(kind, operand, D, kmax=64, N=16640, place="front", background="gauss", seed=3, nbot=None):
    """background rows 2 N(0, I) (gauss) or the same rounded to bf16 (exact: they add nothing to
    a tile's beta_max), far from every engineered query.  nbot: bottom rows per group, if
    not kmax (Basic's lists have 64 rows whatever k is)."""
    gs = groups(kind, operand, D, kmax, nbot)
    rng = np.random.default_rng(seed)
    rows = (2.0 * rng.standard_normal((N, D))).astype(np.float32)
    if background == "exact":
        rows = bf16_round(rows)
    eng = positions(N, len(gs), kmax, place, nbot)
    for g, p in zip(gs, eng):
        rows[p] = g.rows
    return Fixture(kind, operand, D, kmax, rows, np.stack([g.x for g in gs]), eng)


def gaps_ok(keys, k):
    """Condition (c) on one query's fp64 keys: consecutive ranks of the top k + 1 are more than
    1e-4 |score| apart."""
    s = np.sort(keys)[::-1][:k + 1]
    return bool((s[:-1] - s[1:] > 1e-4 * np.abs(s[:-1])).all())


def flip_factor(fx, k, only=None):
    """The largest factor f (to 1/64) on the fixture's targeted terms (or the terms `only`) at
    which model_filter loses a true top-k row of every engineered query; 0.0 if even the
    dropped term loses none (losing is monotone in f).  Over the engineered rows and 512
    background rows: the others are far below every threshold."""
    sc = lambda f: target_scale(fx.kind, f) if only is None else tuple(f if i in only else 1.0 for i in range(3))
    idx = np.concatenate(list(fx.eng) + [fx.free[:512]])
    lost = lambda f: all(len(r["lost"]) > 0 for r in fx.model(k, sc(f), idx))
    if not lost(0.0):
        return 0.0
    lo, hi = 0, 64
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lost(mid / 64) else (lo, mid)
    return lo / 64


class GroupedFixture(Fixture):
    """A two-level tree for the group-centred rows (cwq_group.hip): root N(0, 1) -> G clusters
    with bf16-exact means and variance 1 -> leaves.  Cluster 1 (its rows straddle the first
    row-tile boundary) has the centre 2.1 and holds an upper / lower group built around
    a ~ 2: row = centre + engineered row, so M = fl(row - centre) is the engineered row, its
    residual coherent relative to the group centre, and the query centre + x (bf16-exact) is
    aligned with it.  Every other row is its cluster's centre + 0.3 N(0, I)."""
    CVAR = 1.0

    def __init__(self, kind, D=64, kmax=10, G=64, N=16640, seed=7, weights=DEFAULT_W):
        rng = np.random.default_rng(seed)
        self.weights = weights
        self.centres = bf16_round((2.0 * rng.standard_normal((G, D))).astype(np.float32))
        self.centres[1] = 2.0
        size = np.full(G, (N - 250) // (G - 1))
        size[0] = 250
        size[-1] += N - size.sum()
        self.cluster = np.repeat(np.arange(G), size)
        rows = (self.centres[self.cluster] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
        x = np.full((1, D), 2.0 + 132 * 2.0 ** -6, np.float32)
        # the gap from this tree's own score and hs, at the query's distance from the rows (~0)
        pi, hs, hl = two_level_consts(x, D, self.centres, np.array([1]), self.CVAR, weights)
        gap_s = GAP * abs(float(pi[0, 0]) + hl) / abs(hs)
        g = _group(kind, "bf16", D, kmax, 2.0 ** -6, gap_s=gap_s)
        assert np.array_equal(g.x + np.float32(2.0), x[0])
        eng = 250 + np.arange(2 * kmax)
        rows[eng] = g.rows + np.float32(2.0)
        Fixture.__init__(self, kind, "bf16", D, kmax, rows, x, [eng])

    def model_args(self, x, idx):
        return dict(consts=two_level_consts(x, self.D, self.centres, self.cluster[idx], self.CVAR, self.weights),
                    cent=self.centres[self.cluster[idx]])

    def tree(self):
        N, D = self.rows.shape
        G = len(self.centres)
        mean = np.concatenate([np.zeros((1, D), np.float32), self.centres, self.rows])
        var = np.full((1 + G + N, D), np.float32(PRIOR_VAR), np.float32)
        var[:1 + G] = self.CVAR
        parent = np.concatenate([[-1], np.zeros(G, np.int64), 1 + self.cluster]).astype(np.int64)
        return mean, var, parent, np.arange(1 + G, 1 + G + N, dtype=np.int64)


#: (kind, operand, kmax, ks): the fixture set of the tests.  qside / both: the rows are |x| away
#: from the query, |score| is ~|hs||x|^2, and the kmax key gaps between the lost row and the
#: threshold are a large share of the coherent error: one fixture per k, and the kmax = 64
#: ones keep the factor they reach (FLIP_MIN).
CASES = [(kind, op, kmax, ks) for op in ("bf16", "int8") for kind in KINDS
         for kmax, ks in (((64, (1, 10, 64)),) if kind in ("upper", "lower") else ((1, (1,)), (10, (10,)), (64, (64,))))]
FLIP_MIN = {("qside", "bf16", 64): 0.65, ("qside", "int8", 64): 0.55}


def flip_min(kind, operand, kmax):
    return FLIP_MIN.get((kind, operand, kmax), 0.75)


if __name__ == "__main__":
    print("fixture  operand  kmax  k   flip factor (targeted terms)   x_lo.mu_lo alone")
    for kind, op, kmax, ks in CASES:
        fx = fixture(kind, op, 64, kmax)
        for k in ks:
            alone = f"{flip_factor(fx, k, only=(2,)):.3f}" if kind == "both" else "-"
            print(f"{kind:7s}  {op:5s}  {kmax:4d}  {k:2d}   {flip_factor(fx, k):.3f}   {alone}")
    for kind in ("upper", "lower"):
        fx = GroupedFixture(kind)
        for k in (1, 10):
            print(f"grouped {kind:7s}  bf16  {fx.kmax:4d}  {k:2d}   {flip_factor(fx, k):.3f}   -")
