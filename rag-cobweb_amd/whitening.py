"""PCA + ICA whitening (F4), drop-in for src/whitening/pca_ica.py:PCAICAWhiteningModel.

Same constructor, attributes, `transform(x, is_ica=True)` semantics (single vector ->
1-D result, batch -> 2-D; numpy in -> numpy out) and `fit(X, pca_dim, eps,
ica_max_iter, ica_tol)` classmethod.  `transform` runs on the GPU through libcwq
`cwq_whiten` (fp32 MFMA GEMMs with the centring and the PCA scaling fused); torch
supplies the device buffers.  `fit` is offline training: by default, like the reference
(:55-76), it delegates to scikit-learn's PCA and FastICA on the host; `backend="gpu"`
runs the same algorithm with every pass over the rows on the GPU (libcwq cwq_col_sums,
cwq_gram_acc, cwq_ica_g: fp32 MFMA partials over fixed row slabs, combined in fp64) and
the small d x d algebra (eigh, FastICA's symmetric decorrelation) in fp64 on the host.
`save`/`load` use a pickle-free .npz (the reference pickles, :78-99).

ZCAWhiteningModel (src/whitening/zca.py) and PCAZCAWhiteningModel
(src/whitening/pca_zca.py) are the reference's other two whitening models: the same
`cwq_whiten` transform, and fits from the GPU covariance.
"""
import ctypes
import time

import numpy as np
import torch

from ._lib import check, lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _resolve_device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the row-proportional passes of the fits (include/cobweb_query.h, cwq_whitenfit.hip) ----
FIT_CHUNK = 1 << 20   # rows per upload / per G buffer


def _work(nbytes, device):
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def col_sums(x, acc=None):
    """acc[j] += sum_r x[r][j] (cwq_col_sums).  x: device fp32 [n, d]; acc: device fp64 [d]
    (a new zero array when None).  Returns acc."""
    n, d = x.shape
    if acc is None:
        acc = torch.zeros(d, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        work = _work(lib().cwq_col_sums_work_bytes(n, d), x.device)
        check(lib().cwq_col_sums(_ptr(x), n, d, _ptr(acc), _ptr(work), _stream(x.device)))
    return acc


def gram_acc(a, b, ctr_a=None, ctr_b=None, acc=None):
    """acc[i][j] += sum_r (a[r][i] - ctr_a[i]) (b[r][j] - ctr_b[j]) (cwq_gram_acc).
    a [n, da], b [n, db]: device fp32; centres device fp32 or None; acc device fp64 [da, db]."""
    n, da = a.shape
    db = b.shape[1]
    if b.shape[0] != n:
        raise ValueError("a and b must have the same number of rows")
    if acc is None:
        acc = torch.zeros((da, db), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        work = _work(lib().cwq_gram_acc_work_bytes(n, da, db), a.device)
        check(lib().cwq_gram_acc(_ptr(a), _ptr(b), n, da, db, _ptr(ctr_a), _ptr(ctr_b), _ptr(acc), _ptr(work),
                                 _stream(a.device)))
    return acc


def ica_g(x1, w, g=None, gsum=None):
    """g = tanh(x1 w^T) [n, p] fp32 and gsum[j] += sum_r (1 - g[r][j]^2) fp64 (cwq_ica_g).
    Returns (g, gsum)."""
    n, p = x1.shape
    if g is None:
        g = torch.empty((n, p), dtype=torch.float32, device=x1.device)
    if gsum is None:
        gsum = torch.zeros(p, dtype=torch.float64, device=x1.device)
    with torch.cuda.device(x1.device):
        work = _work(lib().cwq_ica_g_work_bytes(n, p), x1.device)
        check(lib().cwq_ica_g(_ptr(x1), n, p, _ptr(w), _ptr(g), _ptr(gsum), _ptr(work), _stream(x1.device)))
    return g, gsum


def _whiten_into(x, mean, comps, denom, out, unmix=None, work=None):
    """One cwq_whiten call on device tensors: out = ((x - mean) comps^T / denom) (unmix^T)."""
    n, d_in = x.shape
    with torch.cuda.device(x.device):
        check(lib().cwq_whiten(_ptr(x), n, d_in, _ptr(mean), _ptr(comps), comps.shape[0], _ptr(denom), _ptr(unmix),
                               out.shape[1], _ptr(out), _ptr(work), _stream(x.device)))


def _as_rows(X):
    """The fit input as a 2-D float32 numpy array or torch tensor (no copy when it already is)."""
    if isinstance(X, torch.Tensor):
        X = X.to(torch.float32)
    else:
        X = np.asarray(X, np.float32)
    if X.ndim != 2 or X.shape[0] < 2:
        raise ValueError("fit needs a 2-D array of at least two rows")
    return X


def _dev_chunks(X, device):
    """Row chunks of X as contiguous device fp32 tensors; numpy input is uploaded chunk by chunk."""
    rows = FIT_CHUNK
    for i in range(0, X.shape[0], rows):
        c = X[i:i + rows]
        if not isinstance(c, torch.Tensor):
            c = torch.from_numpy(np.ascontiguousarray(c))
        yield i, c.to(device).contiguous()


def _f32_dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _mean_gram(X, device):
    """(mean fp64, the mean as the device fp32 centre, scatter matrix sum_r (x - mean)(x - mean)^T
    fp64).  The rows are centred with the fp32-rounded mean c; the rank-one term n (mean - c)
    (mean - c)^T that this leaves in the Gram is removed in fp64."""
    n, d = X.shape
    acc = torch.zeros(d, dtype=torch.float64, device=device)
    for _, c in _dev_chunks(X, device):
        col_sums(c, acc)
    mean = acc.cpu().numpy() / n
    if not np.all(np.isfinite(mean)):
        raise ValueError("X contains NaN or infinity")
    ctr = _f32_dev(mean, device)
    g = torch.zeros((d, d), dtype=torch.float64, device=device)
    for _, c in _dev_chunks(X, device):
        gram_acc(c, c, ctr, ctr, g)
    delta = mean - ctr.cpu().numpy().astype(np.float64)
    return mean, ctr, g.cpu().numpy() - n * np.outer(delta, delta)


def _pca_from_cov(cov, pca_dim):
    """PCA of a covariance as scikit-learn reports it: eigenvalues descending and clipped at 0,
    in each component the entry of largest magnitude positive (svd_flip), and `pca_dim`
    components (int) or PCA(n_components=frac)'s count (float in (0, 1))."""
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(lam)[::-1]
    lam = np.clip(lam[order], 0.0, None)
    comps = vec[:, order].T
    sg = np.sign(comps[np.arange(comps.shape[0]), np.argmax(np.abs(comps), axis=1)])
    sg[sg == 0] = 1.0
    comps = comps * sg[:, None]
    if isinstance(pca_dim, (int, np.integer)):
        p = int(pca_dim)
        if not 1 <= p <= cov.shape[0]:
            raise ValueError(f"pca_dim must be in [1, {cov.shape[0]}], got {p}")
    else:
        if not 0.0 < pca_dim < 1.0:
            raise ValueError(f"a fractional pca_dim must be in (0, 1), got {pca_dim}")
        p = int(np.searchsorted(np.cumsum(lam / lam.sum()), pca_dim, side="right")) + 1
    return comps[:p], lam[:p]


def _pca_fit_gpu(X, pca_dim, device, timing=None):
    """(mean, components, explained variance) in fp64: the mean, np.cov's n - 1 normalisation and
    the PCA of pca_ica.py:59-66 / pca_zca.py:51-58, the passes over the rows on the GPU."""
    t0 = time.perf_counter()
    mean, _, scatter = _mean_gram(X, device)
    t1 = time.perf_counter()
    comps, var = _pca_from_cov(scatter / (X.shape[0] - 1), pca_dim)
    if timing is not None:
        timing["mean_cov_s"] = t1 - t0
        timing["pca_eigh_s"] = time.perf_counter() - t1
    return mean, comps, var


def sym_decorrelation(W):
    """(W W^T)^(-1/2) W: scikit-learn's _sym_decorrelation, fp64."""
    s, u = np.linalg.eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return (u * (1.0 / np.sqrt(s))) @ u.T @ W


def _normal_init(p, random_state):
    """check_random_state(random_state).normal(size=(p, p)) on numpy's generators."""
    if random_state is None:
        return np.random.normal(size=(p, p))          # numpy's global generator, as scikit-learn
    if isinstance(random_state, (int, np.integer)):
        return np.random.RandomState(int(random_state)).normal(size=(p, p))
    return random_state.normal(size=(p, p))           # a RandomState or a Generator


def _fastica_gpu(xn, w_init, tol, max_iter, timing):
    """scikit-learn's FastICA(whiten="unit-variance", algorithm="parallel", fun="logcosh") on the
    device array xn [n, p] (consumed).  Returns (components_ [p, p] fp64, n_iter)."""
    n, p = xn.shape
    dev = xn.device
    t0 = time.perf_counter()
    # FastICA's own whitening: K = (u / d)^T of the centred data's SVD, from the p x p Gram
    m2 = col_sums(xn).cpu().numpy() / n
    ctr = _f32_dev(m2, dev)
    delta = m2 - ctr.cpu().numpy().astype(np.float64)
    C = gram_acc(xn, xn, ctr, ctr).cpu().numpy() - n * np.outer(delta, delta)
    lam, u = np.linalg.eigh(C)
    order = np.argsort(lam)[::-1]
    lam, u = np.clip(lam[order], np.finfo(np.float64).eps * 10, None), u[:, order]
    sg = np.sign(u[0])
    sg[sg == 0] = 1.0
    ut = np.ascontiguousarray((u * sg).T, dtype=np.float32)
    denom = (np.sqrt(lam) / np.sqrt(n)).astype(np.float32)
    # X1 = K (xn - mean) sqrt(n): one cwq_whiten call with comps = u^T and denom = d / sqrt(n)
    x1 = torch.empty_like(xn)
    _whiten_into(xn, ctr, _f32_dev(ut, dev), _f32_dev(denom, dev), x1)
    del xn
    K = (ut.astype(np.float64) / denom.astype(np.float64)[:, None]) / np.sqrt(n)   # as X1 was made
    torch.cuda.synchronize(dev)
    timing["ica_whiten_s"] = time.perf_counter() - t0

    W = sym_decorrelation(np.asarray(w_init, np.float64))
    rows = min(n, FIT_CHUNK)
    g = torch.empty((rows, p), dtype=torch.float32, device=dev)
    M = torch.zeros((p, p), dtype=torch.float64, device=dev)
    gsum = torch.zeros(p, dtype=torch.float64, device=dev)
    timing["iter_s"], timing["symdec_s"] = [], []
    n_iter = max_iter
    for it in range(max_iter):
        t0 = time.perf_counter()
        wd = _f32_dev(W, dev)
        M.zero_()
        gsum.zero_()
        for i in range(0, n, rows):
            xc = x1[i:i + rows]
            gc = g[:xc.shape[0]]
            ica_g(xc, wd, gc, gsum)
            gram_acc(gc, xc, None, None, M)
        Mh, gh = M.cpu().numpy(), gsum.cpu().numpy()
        t1 = time.perf_counter()
        W1 = sym_decorrelation(Mh / n - (gh / n)[:, None] * W)
        lim = float(np.max(np.abs(np.abs(np.einsum("ij,ij->i", W1, W)) - 1.0)))
        W = W1
        t2 = time.perf_counter()
        timing["iter_s"].append(t2 - t0)
        timing["symdec_s"].append(t2 - t1)
        if lim < tol:
            n_iter = it + 1
            break
    else:
        import warnings
        warnings.warn("FastICA did not converge. Consider increasing tolerance or the maximum number of iterations.")
    # unit variance: np.std of the sources W K (xn - mean), from the Gram (no pass over the rows)
    WK = W @ K
    std = np.sqrt(np.einsum("ij,jk,ik->i", WK, C, WK) / n)
    return WK / std[:, None], n_iter


def _run_whiten(x, device, mean, comps, denom, unmix, batch):
    """transform() of the three models: numpy in -> numpy out, a single vector -> 1-D."""
    as_numpy = not isinstance(x, torch.Tensor)
    xt = torch.as_tensor(np.asarray(x, np.float32) if as_numpy else x, dtype=torch.float32)
    single = xt.dim() == 1
    if single:
        xt = xt[None, :]
    xt = xt.to(device).contiguous()
    n, d_in = xt.shape
    if d_in != comps.shape[1]:
        raise ValueError(f"expected inputs of dimension {comps.shape[1]}, got {d_in}")
    d_out = unmix.shape[0] if unmix is not None else comps.shape[0]
    out = torch.empty((n, d_out), dtype=torch.float32, device=device)
    work = (torch.empty((min(n, batch), comps.shape[0]), dtype=torch.float32, device=device)
            if unmix is not None else None)
    for i in range(0, n, batch):
        _whiten_into(xt[i:i + batch], mean, comps, denom, out[i:i + batch], unmix, work)
    if single:
        out = out[0]
    return out.cpu().numpy() if as_numpy else out


class PCAICAWhiteningModel:
    def __init__(self, mean, pca_components, ica_unmixing, pca_explained_var, eps=1e-8, device=None):
        self.mean = np.asarray(mean, np.float32)
        self.pca_components = np.asarray(pca_components, np.float32)
        self.pca_explained_var = np.asarray(pca_explained_var, np.float32)
        self.ica_unmixing = None if ica_unmixing is None else np.asarray(ica_unmixing, np.float32)
        self.eps = eps
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dev = None

    def __repr__(self):
        return (f"{self.__class__.__name__}(\n  mean.shape={self.mean.shape},\n"
                f"  pca_components.shape={self.pca_components.shape},\n"
                f"  pca_explained_var.shape={self.pca_explained_var.shape},\n"
                f"  ica_unmixing.shape={None if self.ica_unmixing is None else self.ica_unmixing.shape},\n"
                f"  eps={self.eps}\n)")

    def _device_params(self):
        if self._dev is None:
            # the divisor exactly as the reference computes it (fp32 add, fp32 sqrt), pca_ica.py:44
            denom = np.sqrt(self.pca_explained_var + np.float32(self.eps)).astype(np.float32)
            to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self._dev = (to(self.mean), to(self.pca_components), to(denom), to(self.ica_unmixing))
        return self._dev

    def transform(self, x, is_ica=True, batch=1 << 20):
        """PCAICAWhiteningModel.transform (pca_ica.py:30-51) on the GPU."""
        mean, comps, denom, unmix = self._device_params()
        return _run_whiten(x, self.device, mean, comps, denom, unmix if is_ica else None, batch)

    @classmethod
    def fit(cls, X, pca_dim=256, eps=1e-8, ica_max_iter=5000, ica_tol=1e-3, device=None, backend="sklearn",
            w_init=None, random_state=None):
        """pca_ica.py:55-76: PCA -> normalise -> FastICA.  backend="sklearn": on the host through
        scikit-learn, as the reference.  backend="gpu": the same algorithm with the passes over the
        rows on the GPU (X: numpy, uploaded in row chunks, or a device tensor).  `w_init` [p, p] and
        `random_state` are FastICA's.  The iteration count is left in `model.ica_n_iter_`."""
        if backend not in ("sklearn", "gpu"):
            raise ValueError(f"backend must be 'sklearn' or 'gpu', got {backend!r}")
        if w_init is not None:
            w_init = np.asarray(w_init, np.float64)
            if w_init.ndim != 2 or w_init.shape[0] != w_init.shape[1] or (
                    isinstance(pca_dim, (int, np.integer)) and w_init.shape[0] != pca_dim):
                raise ValueError(f"w_init has invalid shape {w_init.shape} -- should be (pca_dim, pca_dim)")
        if backend == "gpu":
            return cls._fit_gpu(X, pca_dim, eps, ica_max_iter, ica_tol, device, w_init, random_state)
        from sklearn.decomposition import PCA, FastICA
        X = np.asarray(X, np.float32)
        mean = X.mean(axis=0)
        X_centered = X - mean
        pca = PCA(n_components=pca_dim)
        X_pca = pca.fit_transform(X_centered)
        components = pca.components_
        explained_var = pca.explained_variance_
        X_pca_normalized = X_pca / np.sqrt(explained_var + eps)
        ica = FastICA(n_components=components.shape[0], whiten="unit-variance", max_iter=ica_max_iter, tol=ica_tol,
                      w_init=w_init, random_state=random_state)
        ica.fit_transform(X_pca_normalized)
        model = cls(mean, components, ica.components_, explained_var, eps, device=device)
        model.ica_n_iter_ = int(ica.n_iter_)
        return model

    @classmethod
    def _fit_gpu(cls, X, pca_dim, eps, ica_max_iter, ica_tol, device, w_init, random_state):
        device = _resolve_device(device)
        X = _as_rows(X)
        if not isinstance(X, torch.Tensor) and X.shape[0] <= FIT_CHUNK:
            X = torch.from_numpy(np.ascontiguousarray(X)).to(device)   # one upload for all passes
        n = X.shape[0]
        timing = {}
        mean, comps, var = _pca_fit_gpu(X, pca_dim, device, timing)
        p = comps.shape[0]
        if w_init is not None and w_init.shape != (p, p):
            raise ValueError(f"w_init has invalid shape {w_init.shape} -- should be {(p, p)}")
        model = cls(mean, comps, None, var, eps, device=device)
        t0 = time.perf_counter()
        dmean, dcomps, ddenom, _ = model._device_params()
        xn = torch.empty((n, p), dtype=torch.float32, device=device)      # the normalised PCA output
        for i, c in _dev_chunks(X, device):
            _whiten_into(c, dmean, dcomps, ddenom, xn[i:i + c.shape[0]])
        torch.cuda.synchronize(device)
        timing["pca_transform_s"] = time.perf_counter() - t0
        if w_init is None:
            w_init = _normal_init(p, random_state)
        unmix, n_iter = _fastica_gpu(xn, w_init, ica_tol, ica_max_iter, timing)
        model.ica_unmixing = np.asarray(unmix, np.float32)
        model._dev = None
        model.ica_n_iter_ = n_iter
        model.fit_timing_ = timing
        return model

    def save(self, filepath):
        with open(filepath, "wb") as f:
            np.savez(f, mean=self.mean, pca_components=self.pca_components, pca_explained_var=self.pca_explained_var,
                     ica_unmixing=self.ica_unmixing if self.ica_unmixing is not None else np.zeros((0, 0), np.float32),
                     eps=np.asarray([self.eps], np.float64))

    @classmethod
    def load(cls, filepath, device=None):
        with np.load(filepath, allow_pickle=False) as z:
            unmix = z["ica_unmixing"]
            return cls(z["mean"], z["pca_components"], None if unmix.size == 0 else unmix, z["pca_explained_var"],
                       float(z["eps"][0]), device=device)


class ZCAWhiteningModel:
    """src/whitening/zca.py:ZCAWhiteningModel: x -> (x - mean) @ whitening_matrix^T, on the GPU."""

    def __init__(self, mean, whitening_matrix, eps=1e-8, device=None):
        self.mean = np.asarray(mean, np.float32)
        self.whitening_matrix = np.asarray(whitening_matrix, np.float32)
        self.eps = eps
        self.device = _resolve_device(device)
        self._dev = None

    def __repr__(self):
        return (f"{self.__class__.__name__}(\n  mean.shape={self.mean.shape},\n"
                f"  whitening_matrix.shape={self.whitening_matrix.shape},\n  eps={self.eps}\n)")

    def transform(self, x, batch=1 << 20):
        """zca.py:15-29 through cwq_whiten with a unit divisor and no second product."""
        if self._dev is None:
            self._dev = (_f32_dev(self.mean, self.device), _f32_dev(self.whitening_matrix, self.device),
                         torch.ones(self.whitening_matrix.shape[0], dtype=torch.float32, device=self.device))
        mean, wm, ones = self._dev
        return _run_whiten(x, self.device, mean, wm, ones, None, batch)

    @classmethod
    def fit(cls, X, eps=1e-8, device=None):
        """zca.py:32-51 with the mean and the covariance (np.cov: n - 1) from the GPU passes."""
        device = _resolve_device(device)
        X = _as_rows(X)
        mean, _, scatter = _mean_gram(X, device)
        lam, u = np.linalg.eigh(scatter / (X.shape[0] - 1))
        return cls(mean, (u * (1.0 / np.sqrt(lam + eps))) @ u.T, eps, device=device)

    def save(self, filepath):
        with open(filepath, "wb") as f:
            np.savez(f, mean=self.mean, whitening_matrix=self.whitening_matrix, eps=np.asarray([self.eps], np.float64))

    @classmethod
    def load(cls, filepath, device=None):
        with np.load(filepath, allow_pickle=False) as z:
            return cls(z["mean"], z["whitening_matrix"], float(z["eps"][0]), device=device)


class PCAZCAWhiteningModel:
    """src/whitening/pca_zca.py:PCAZCAWhiteningModel: PCA whitening rotated back to the input basis."""

    def __init__(self, mean, pca_components, pca_explained_var, eps=1e-8, device=None):
        self.mean = np.asarray(mean, np.float32)
        self.pca_components = np.asarray(pca_components, np.float32)
        self.pca_explained_var = np.asarray(pca_explained_var, np.float32)
        self.eps = eps
        self.device = _resolve_device(device)
        self._dev = None

    def __repr__(self):
        return (f"{self.__class__.__name__}(\n  mean.shape={self.mean.shape},\n"
                f"  pca_components.shape={self.pca_components.shape},\n"
                f"  pca_explained_var.shape={self.pca_explained_var.shape},\n  eps={self.eps}\n)")

    def transform(self, x, batch=1 << 20):
        """pca_zca.py:23-44: ((x - mean) C^T / sqrt(var + eps)) C, cwq_whiten with unmix = C^T."""
        if self._dev is None:
            denom = np.sqrt(self.pca_explained_var + np.float32(self.eps)).astype(np.float32)
            self._dev = (_f32_dev(self.mean, self.device), _f32_dev(self.pca_components, self.device),
                         _f32_dev(denom, self.device), _f32_dev(self.pca_components.T, self.device))
        mean, comps, denom, back = self._dev
        return _run_whiten(x, self.device, mean, comps, denom, back, batch)

    @classmethod
    def fit(cls, X, pca_dim=256, eps=1e-8, device=None):
        """pca_zca.py:47-60 with the mean and the covariance from the GPU passes."""
        device = _resolve_device(device)
        mean, comps, var = _pca_fit_gpu(_as_rows(X), pca_dim, device)
        return cls(mean, comps, var, eps, device=device)

    def save(self, filepath):
        with open(filepath, "wb") as f:
            np.savez(f, mean=self.mean, pca_components=self.pca_components, pca_explained_var=self.pca_explained_var,
                     eps=np.asarray([self.eps], np.float64))

    @classmethod
    def load(cls, filepath, device=None):
        with np.load(filepath, allow_pickle=False) as z:
            return cls(z["mean"], z["pca_components"], z["pca_explained_var"], float(z["eps"][0]), device=device)


def encode_and_whiten_pcaica(sentences, st_model, whitening_model):
    """pca_ica.py:103-122: encode (if given strings) then whiten."""
    if isinstance(sentences[0], str):
        embeddings = st_model.encode(sentences, convert_to_numpy=True, batch_size=64, show_progress_bar=False)
    else:
        embeddings = sentences
    return whitening_model.transform(embeddings)


def encode_and_whiten_zca(obj, st_model, whitening_model):
    """zca.py:71-86 (which reads its two models from globals): encode (if given strings) then whiten."""
    embeddings = (st_model.encode(obj, convert_to_numpy=True, batch_size=64, show_progress_bar=False)
                  if isinstance(obj[0], str) else obj)
    return whitening_model.transform(embeddings)


def encode_and_whiten_pcazca(sentences, st_model, whitening_model):
    """pca_zca.py:82-100: encode (if given strings) then whiten."""
    embeddings = (st_model.encode(sentences, convert_to_numpy=True, batch_size=64, show_progress_bar=False)
                  if isinstance(sentences[0], str) else sentences)
    return whitening_model.transform(embeddings)
