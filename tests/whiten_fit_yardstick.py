"""The yardstick of the whitening-fit tests: numpy restatements of what the reference's
fits compute (src/whitening/pca_ica.py:55-76, zca.py:32-51, pca_zca.py:47-60), i.e.
scikit-learn's PCA (covariance form, its sign rule and its variance-fraction rule) and
its parallel logcosh FastICA with whiten="unit-variance".

fp64 (`heavy=np.float64`) is the yardstick.  `heavy=np.float32` gives the E_ref variants:
the row-proportional passes (column sums, Grams, the two GEMMs and tanh of an iteration)
in numpy float32, the small d x d algebra in fp64 -- the same split the product makes, so
its error against fp64 is the error the number format allows, and the GPU tests bound
the kernels by a multiple of it.

Comparing two ICA fits: only up to row permutation and sign (FastICA's own whitening
matrix is a rotation of a degenerate spectrum), and only on problems where pca_dim is
the number of sources (`match_rows`).
"""
import numpy as np

F64 = np.float64

# Per-row relative L2 difference of the fp64 restatement's unmixing rows from the real
# reference's (the fixture) at the default tol = 1e-3, as tests/test_whiten_fit_cpu.py
# measures it: both stop within tol of the fixed point.  The GPU fit is allowed twice this.
ICA_VS_FIXTURE = 2.9e-3


# ---------------------------------------------------------------- data
def sources(N, D, P, seed):
    """N rows of D dims mixed from P independent non-Gaussian sources: P/2 Laplace and
    P - P/2 uniform(-1.7, 1.7) columns, scaled by linspace(1, 3, P), mixed by a
    standard-normal [P, D] matrix, plus 0.05 N(0, 1) noise, plus 0.5; float32."""
    rng = np.random.default_rng(seed)
    S = np.concatenate([rng.laplace(size=(N, P // 2)), rng.uniform(-1.7, 1.7, size=(N, P - P // 2))], axis=1)
    S *= np.linspace(1.0, 3.0, P)
    A = rng.standard_normal((P, D))
    X = S @ A + 0.05 * rng.standard_normal((N, D)) + 0.5
    return X.astype(np.float32)


# ---------------------------------------------------------------- heavy passes
def col_sums(X, heavy=F64):
    """Column sums of X accumulated in `heavy`, returned as fp64."""
    return np.asarray(X, heavy).sum(axis=0, dtype=heavy).astype(F64)


def gram(A, B, ctr_a=None, ctr_b=None, heavy=F64):
    """sum_r (A[r] - ctr_a)^T (B[r] - ctr_b) with the subtraction and the product in `heavy`."""
    A = np.asarray(A, heavy)
    B = np.asarray(B, heavy)
    if ctr_a is not None:
        A = A - np.asarray(ctr_a, heavy)
    if ctr_b is not None:
        B = B - np.asarray(ctr_b, heavy)
    return (A.T @ B).astype(F64)


def ica_g(X1, W, heavy=F64):
    """G = tanh(X1 W^T) [n, p] and gsum[j] = sum_r (1 - G[r][j]^2), all in `heavy`."""
    G = np.tanh(np.asarray(X1, heavy) @ np.asarray(W, heavy).T)
    gsum = (heavy(1) - G * G).sum(axis=0, dtype=heavy)
    return G, gsum.astype(F64)


def ica_step(X1, W, heavy=F64):
    """One iteration's data pass: (M, gsum) with M = G^T X1 [p, p]."""
    G, gsum = ica_g(X1, W, heavy)
    return gram(G, X1, heavy=heavy), gsum


def whiten(X, mean, comps, denom, heavy=F64):
    """((X - mean) comps^T) / denom in `heavy` (the transform's first GEMM)."""
    Xc = np.asarray(X, heavy) - np.asarray(mean, heavy)
    return (Xc @ np.asarray(comps, heavy).T) / np.asarray(denom, heavy)


# ---------------------------------------------------------------- small algebra (always fp64)
def mean_cov(X, heavy=F64):
    """(mean, covariance with np.cov's n - 1 normalisation).  The data is centred with the
    mean rounded to `heavy`, as a pass in that format has to."""
    n = X.shape[0]
    mean = col_sums(X, heavy) / n
    mc = mean.astype(heavy)
    return mean, gram(X, X, mc, mc, heavy) / (n - 1)


def sign_rule(components):
    """scikit-learn's svd_flip on the rows: the entry of largest magnitude is positive."""
    idx = np.argmax(np.abs(components), axis=1)
    s = np.sign(components[np.arange(components.shape[0]), idx])
    s[s == 0] = 1.0
    return components * s[:, None]


def n_components_for(var_all, pca_dim):
    """int: that many.  float in (0, 1): PCA(n_components=frac)'s rule."""
    if isinstance(pca_dim, (int, np.integer)):
        return int(pca_dim)
    ratio = var_all / var_all.sum()
    return int(np.searchsorted(np.cumsum(ratio), pca_dim, side="right")) + 1


def pca_from_cov(cov, pca_dim):
    """(components [p, d], explained variance [p]) of a covariance: eigh, descending,
    clipped at 0, the sign rule, then the first n_components_for rows."""
    lam, vec = np.linalg.eigh(np.asarray(cov, F64))
    order = np.argsort(lam)[::-1]
    lam = np.clip(lam[order], 0.0, None)
    comps = sign_rule(vec[:, order].T)
    p = n_components_for(lam, pca_dim)
    return comps[:p], lam[:p]


def pca_fit(X, pca_dim, heavy=F64):
    """(mean, components, explained variance): the reference's mean + PCA (pca_ica.py:59-66)."""
    mean, cov = mean_cov(X, heavy)
    comps, var = pca_from_cov(cov, pca_dim)
    return mean, comps, var


def sym_decorrelation(W):
    """(W W^T)^(-1/2) W, the eigendecomposition form of scikit-learn's _sym_decorrelation."""
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(F64).tiny, None)
    return (u * (1.0 / np.sqrt(s))) @ u.T @ W


def ica_whitening(gram_c, n):
    """FastICA's K from the Gram of the centred data (scikit-learn takes the SVD of the
    data: d are its singular values, u its left vectors, u *= sign(u[0])).  Returns
    (u^T [p, p], d [p]): K = u^T / d[:, None]."""
    lam, u = np.linalg.eigh(np.asarray(gram_c, F64))
    order = np.argsort(lam)[::-1]
    lam, u = lam[order], u[:, order]
    lam = np.clip(lam, np.finfo(F64).eps * 10, None)
    sg = np.sign(u[0])
    sg[sg == 0] = 1.0
    return (u * sg).T, np.sqrt(lam)


def fastica(Xn, w_init, tol=1e-3, max_iter=5000, heavy=F64):
    """scikit-learn's FastICA(whiten="unit-variance", algorithm="parallel", fun="logcosh")
    on Xn [n, p] with p components.  Returns (components_ [p, p], n_iter)."""
    n, p = Xn.shape
    m2 = col_sums(Xn, heavy) / n
    m2h = m2.astype(heavy)
    C = gram(Xn, Xn, m2h, m2h, heavy)
    ut, d = ica_whitening(C, n)
    denom = (d / np.sqrt(n)).astype(heavy)
    uth = ut.astype(heavy)
    X1 = whiten(Xn, m2h, uth, denom, heavy)
    K = (uth.astype(F64) / denom.astype(F64)[:, None]) / np.sqrt(n)   # the K that X1 was made with
    W = sym_decorrelation(np.asarray(w_init, F64))
    n_iter = max_iter
    for it in range(max_iter):
        M, gsum = ica_step(X1, W.astype(heavy), heavy)
        W1 = sym_decorrelation(M / n - (gsum / n)[:, None] * W)
        lim = np.max(np.abs(np.abs(np.einsum("ij,ij->i", W1, W)) - 1.0))
        W = W1
        if lim < tol:
            n_iter = it + 1
            break
    WK = W @ K
    std = np.sqrt(np.einsum("ij,jk,ik->i", WK, C, WK) / n)   # np.std of the sources, from the Gram
    return WK / std[:, None], n_iter


def pcaica_fit(X, pca_dim, w_init, eps=1e-8, tol=1e-3, max_iter=5000, heavy=F64):
    """PCAICAWhiteningModel.fit (pca_ica.py:55-76).  Returns a dict of the model's arrays."""
    mean, comps, var = pca_fit(X, pca_dim, heavy)
    denom = np.sqrt(var.astype(heavy) + heavy(eps))
    Xn = whiten(X, mean.astype(heavy), comps.astype(heavy), denom, heavy)
    unmix, n_iter = fastica(Xn, w_init, tol, max_iter, heavy)
    return dict(mean=mean, pca_components=comps, pca_explained_var=var, ica_unmixing=unmix, n_iter=n_iter)


def zca_fit(X, eps=1e-8, heavy=F64):
    """ZCAWhiteningModel.fit (zca.py:32-51): (mean, U diag(1/sqrt(lam + eps)) U^T)."""
    mean, cov = mean_cov(X, heavy)
    lam, u = np.linalg.eigh(cov)
    return mean, (u * (1.0 / np.sqrt(lam + eps))) @ u.T


def pcazca_fit(X, pca_dim, heavy=F64):
    """PCAZCAWhiteningModel.fit (pca_zca.py:47-60)."""
    return pca_fit(X, pca_dim, heavy)


def pcaica_transform(X, mean, comps, var, unmix, eps=1e-8):
    return whiten(X, mean, comps, np.sqrt(np.asarray(var, F64) + eps)) @ np.asarray(unmix, F64).T


def zca_transform(X, mean, wm):
    return (np.asarray(X, F64) - mean) @ np.asarray(wm, F64).T


def pcazca_transform(X, mean, comps, var, eps=1e-8):
    comps = np.asarray(comps, F64)
    z = (comps.T / np.sqrt(np.asarray(var, F64) + eps)) @ comps
    return (np.asarray(X, F64) - mean) @ z


# ---------------------------------------------------------------- comparisons
def rel_max(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def match_rows(U, V):
    """Match the rows of U to the rows of V: assignment on |cosine|, then sign, then the
    per-row relative L2 difference.  Returns (min |cos| over the matched pairs, max
    relative L2 difference, U's rows permuted and signed to V's order)."""
    U, V = np.asarray(U, F64), np.asarray(V, F64)
    Un = U / np.linalg.norm(U, axis=1, keepdims=True)
    Vn = V / np.linalg.norm(V, axis=1, keepdims=True)
    cos = Vn @ Un.T                      # [row of V][row of U]
    try:
        from scipy.optimize import linear_sum_assignment
        vi, ui = linear_sum_assignment(-np.abs(cos))
    except ImportError:                  # greedy: the best remaining pair first
        c = np.abs(cos).copy()
        vi, ui = [], []
        for _ in range(c.shape[0]):
            a, b = np.unravel_index(np.argmax(c), c.shape)
            vi.append(a)
            ui.append(b)
            c[a, :] = -1
            c[:, b] = -1
        order = np.argsort(vi)
        vi, ui = np.asarray(vi)[order], np.asarray(ui)[order]
    picked = cos[vi, ui]
    Um = U[ui] * np.sign(picked)[:, None]
    rel = np.linalg.norm(Um - V[vi], axis=1) / np.linalg.norm(V[vi], axis=1)
    return float(np.min(np.abs(picked))), float(np.max(rel)), Um
