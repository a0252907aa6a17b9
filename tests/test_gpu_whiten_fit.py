"""Whitening fits on the GPU: libcwq cwq_col_sums / cwq_gram_acc / cwq_ica_g against fp64, and
PCAICAWhiteningModel.fit(backend="gpu"), ZCAWhiteningModel.fit and PCAZCAWhiteningModel.fit
against the fp64 yardstick (tests/whiten_fit_yardstick.py) and the real reference's fits
(tests/golden/g11_whiten_fit.npz).

Tolerance: in every comparison against fp64 the bound is MARGIN x the error of the numpy
float32 variant (E_ref) on the same inputs against the same fp64 value; the margin covers the
different summation order and the device tanh.  Each test prints both errors before it
asserts.  ICA fits are compared through the row matcher (permutation and sign are free)."""
import numpy as np
import pytest

import whiten_fit_yardstick as Y
from conftest import load_golden

pytestmark = pytest.mark.gpu
MARGIN = 8.0
F32 = np.float32


@pytest.fixture(scope="module")
def torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def gold():
    g = load_golden("g11_whiten_fit")
    g["X64"] = g["X"].astype(np.float64)
    return g


def slab(pkg):
    return pkg.lib().cwq_whitenfit_slab()


def bound(name, got, eref):
    print(f"{name}: GPU error {got:.3e}, E_ref {eref:.3e}, ratio {got / max(eref, 1e-300):.2f}")
    assert got <= MARGIN * eref, name


def offset_data(rng, n, d):
    """Columns of spread sigma around a centre of about 50 sigma: a missing or misplaced
    centring shows at once."""
    sigma = rng.uniform(0.5, 2.0, d)
    centre = 50.0 * sigma * rng.choice([-1.0, 1.0], d)
    return (rng.standard_normal((n, d)) * sigma + centre).astype(F32)


# ---------------------------------------------------------------- cwq_col_sums, cwq_gram_acc
def gram_case(pkg, torch, n, da, db, same):
    wh = pkg.whitening
    rng = np.random.default_rng(1000 * n + da + db)
    A = offset_data(rng, n, da)
    B = A if same else offset_data(rng, n, db)
    ca = A.mean(0).astype(F32)
    cb = ca if same else (B.mean(0) * (1 + 1e-3)).astype(F32)     # near, not at, the mean
    At = torch.from_numpy(A).cuda()
    Bt = At if same else torch.from_numpy(B).cuda()
    cat = torch.from_numpy(ca).cuda()
    cbt = cat if same else torch.from_numpy(cb).cuda()

    # column sums
    s64 = Y.col_sums(A)
    s = wh.col_sums(At)
    bound(f"col_sums {n}x{da}", Y.rel_max(s.cpu().numpy(), s64), Y.rel_max(Y.col_sums(A, F32), s64))
    assert torch.equal(wh.col_sums(At), s)                         # bit-identical from run to run
    assert torch.equal(wh.col_sums(At, s.clone()), 2 * s)          # a second call accumulates

    # Gram
    g64 = Y.gram(A, B, ca, cb)
    g = wh.gram_acc(At, Bt, cat, cbt)
    bound(f"gram_acc {n}x{da}x{db}{' (A == B)' if same else ''}", Y.rel_max(g.cpu().numpy(), g64),
          Y.rel_max(Y.gram(A, B, ca, cb, F32), g64))
    assert torch.equal(wh.gram_acc(At, Bt, cat, cbt), g)
    assert torch.equal(wh.gram_acc(At, Bt, cat, cbt, g.clone()), 2 * g)
    if same:
        assert torch.equal(g, g.T)                                 # mirrored tiles: exactly symmetric
    # no centres
    g0 = wh.gram_acc(At, Bt)
    g064 = Y.gram(A, B)
    bound(f"gram_acc {n}x{da}x{db} no centres", Y.rel_max(g0.cpu().numpy(), g064), Y.rel_max(Y.gram(A, B, heavy=F32), g064))


@pytest.mark.parametrize("n,da,db", [(5, 3, 3), (1000, 37, 37), (4099, 160, 96)])
def test_gpu_col_sums_and_gram_two_operands(pkg, torch_gpu, n, da, db):
    gram_case(pkg, torch_gpu, n, da, db, same=False)


def test_gpu_gram_symmetric_768(pkg, torch_gpu):
    gram_case(pkg, torch_gpu, 3001, 768, 768, same=True)


def test_gpu_gram_three_slabs(pkg, torch_gpu):
    gram_case(pkg, torch_gpu, 2 * slab(pkg) + 1, 288, 288, same=True)


def test_gpu_gram_one_operand_centred(pkg, torch_gpu):
    """Only ctr_a given, A != B, several slabs: rows past n in the last slab contribute 0."""
    torch, wh = torch_gpu, pkg.whitening
    rng = np.random.default_rng(5)
    n = slab(pkg) + 17
    A, B = offset_data(rng, n, 40), offset_data(rng, n, 130)
    ca = A.mean(0).astype(F32)
    g = wh.gram_acc(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(ca).cuda(), None)
    g64 = Y.gram(A, B, ca, None)
    bound("gram_acc ctr_a only", Y.rel_max(g.cpu().numpy(), g64), Y.rel_max(Y.gram(A, B, ca, None, F32), g64))


# ---------------------------------------------------------------- cwq_ica_g
@pytest.mark.parametrize("n,p", [(1000, 8), (4099, 37), (4099, 160), (None, 288)])
def test_gpu_ica_g(pkg, torch_gpu, n, p):
    torch, wh = torch_gpu, pkg.whitening
    n = 2 * slab(pkg) + 1 if n is None else n
    rng = np.random.default_rng(n + p)
    X1 = rng.standard_normal((n, p)).astype(F32)
    W = (np.linalg.qr(rng.standard_normal((p, p)))[0] * rng.uniform(0.5, 2.0, p)[:, None]).astype(F32)
    G64, gs64 = Y.ica_g(X1, W)
    G32, gs32 = Y.ica_g(X1, W, F32)
    xt, wt = torch.from_numpy(X1).cuda(), torch.from_numpy(W).cuda()
    G, gs = wh.ica_g(xt, wt)
    bound(f"ica_g G {n}x{p}", float(np.abs(G.cpu().numpy() - G64).max()), float(np.abs(G32 - G64).max()))
    # rows past n and columns past p are masked out of gsum (a zero padding row would add 1)
    bound(f"ica_g gsum {n}x{p}", Y.rel_max(gs.cpu().numpy(), gs64), Y.rel_max(gs32, gs64))
    G2, gs2 = wh.ica_g(xt, wt)
    assert torch.equal(G2, G) and torch.equal(gs2, gs)
    assert torch.equal(wh.ica_g(xt, wt, gsum=gs.clone())[1], 2 * gs)
    # one iteration's data pass (M, gsum) as the fit runs it
    M = wh.gram_acc(G, xt)
    M64, _ = Y.ica_step(X1, W)
    bound(f"ica step M {n}x{p}", Y.rel_max(M.cpu().numpy(), M64), Y.rel_max(Y.ica_step(X1, W, F32)[0], M64))


# ---------------------------------------------------------------- end to end
def cov_dev(out):
    """max |cov - I| of a whitened output (np.std's 1/n normalisation, as FastICA scales)."""
    out = np.asarray(out, np.float64)
    c = np.cov(out.T, bias=True)
    return float(np.abs(c - np.eye(c.shape[0])).max())


def transform_f32(X, r, eps=1e-8):
    """The float32 pipeline of the transform on a yardstick model (what numpy float32 gives)."""
    var = r["pca_explained_var"].astype(F32)
    xp = Y.whiten(X, r["mean"].astype(F32), r["pca_components"].astype(F32), np.sqrt(var + F32(eps)), F32)
    return xp @ r["ica_unmixing"].astype(F32).T


@pytest.fixture(scope="module")
def problems(gold):
    """name -> (X float32, P, w_init, fp64 fit, float32-variant fit), computed once."""
    out = {}
    big = Y.sources(8192, 64, 32, 11)
    for name, X, P, w0 in (("fixture", gold["X"], 12, gold["w_init"]),
                           ("8192x64", big, 32, np.random.RandomState(3).normal(size=(32, 32)))):
        r64 = Y.pcaica_fit(X.astype(np.float64), P, w0, tol=1e-6)
        r32 = Y.pcaica_fit(X, P, w0, tol=1e-6, heavy=F32)
        out[name] = (X, P, w0, r64, r32)
    return out


@pytest.mark.parametrize("name", ["fixture", "8192x64"])
def test_gpu_fit_pcaica_matches_yardstick(pkg, torch_gpu, problems, name):
    X, P, w0, r64, r32 = problems[name]
    m = pkg.whitening.PCAICAWhiteningModel.fit(X, pca_dim=P, ica_tol=1e-6, w_init=w0, backend="gpu", device="cuda:0")
    assert m.ica_unmixing.shape == (P, P) and m.ica_unmixing.dtype == F32
    bound(f"{name} mean", Y.rel_max(m.mean, r64["mean"]), Y.rel_max(r32["mean"].astype(F32), r64["mean"]))
    bound(f"{name} components", float(np.abs(m.pca_components - r64["pca_components"]).max()),
          float(np.abs(r32["pca_components"].astype(F32) - r64["pca_components"]).max()))
    bound(f"{name} variances", Y.rel_max(m.pca_explained_var, r64["pca_explained_var"]),
          Y.rel_max(r32["pca_explained_var"].astype(F32), r64["pca_explained_var"]))
    mincos, rel, _ = Y.match_rows(m.ica_unmixing, r64["ica_unmixing"])
    mc32, rel32, _ = Y.match_rows(r32["ica_unmixing"], r64["ica_unmixing"])
    print(f"{name} unmixing rows vs fp64: GPU min|cos| {mincos:.9f} rel {rel:.3e}; float32 variant {mc32:.9f} "
          f"{rel32:.3e}; iterations GPU {m.ica_n_iter_}, fp64 {r64['n_iter']}, float32 variant {r32['n_iter']}")
    assert mincos >= 0.999
    bound(f"{name} transform: max |cov - I|", cov_dev(m.transform(X)), cov_dev(transform_f32(X, r32)))
    assert abs(m.ica_n_iter_ - r64["n_iter"]) <= 3
    share = sum(m.fit_timing_["symdec_s"]) / sum(m.fit_timing_["iter_s"])
    print(f"{name} host symdec share of the iteration time: {share:.2f}")


def test_gpu_fit_pcaica_default_tol_matches_reference_rows(pkg, torch_gpu, gold):
    """At the default tol both fits stop within tol of the fixed point: twice the distance the
    fp64 restatement keeps from the reference's rows (tests/test_whiten_fit_cpu.py)."""
    m = pkg.whitening.PCAICAWhiteningModel.fit(gold["X"], pca_dim=12, w_init=gold["w_init"], backend="gpu",
                                               device="cuda:0")
    mincos, rel, um = Y.match_rows(m.ica_unmixing, gold["ica_unmixing"])
    print(f"default tol vs the reference's rows: min|cos| {mincos:.9f} rel {rel:.3e} (bound {2 * Y.ICA_VS_FIXTURE}), "
          f"iterations {m.ica_n_iter_}")
    assert mincos >= 0.999 and rel <= 2 * Y.ICA_VS_FIXTURE
    # the reference's transform, through the same permutation and sign
    T = int(gold["T"][0])
    m.ica_unmixing = um.astype(F32)
    m._dev = None
    assert Y.rel_max(m.transform(gold["X"][:T]), gold["X_ica"]) <= 4 * Y.ICA_VS_FIXTURE
    assert Y.rel_max(m.transform(gold["X"][:T], is_ica=False), gold["X_pca"]) <= 1e-5


def test_gpu_fit_zca_and_pcazca_match_reference(pkg, torch_gpu, gold):
    wh = pkg.whitening
    X, X64, T = gold["X"], gold["X64"], int(gold["T"][0])
    z = wh.ZCAWhiteningModel.fit(X, device="cuda:0")
    m32, w32 = Y.zca_fit(X, heavy=F32)
    assert z.whitening_matrix.shape == (24, 24) and z.mean.dtype == F32
    bound("zca mean", Y.rel_max(z.mean, gold["zca_mean"]), Y.rel_max(m32.astype(F32), gold["zca_mean"]))
    bound("zca matrix", Y.rel_max(z.whitening_matrix, gold["zca_matrix"]), Y.rel_max(w32.astype(F32), gold["zca_matrix"]))
    ref32 = (X[:T] - m32.astype(F32)) @ w32.astype(F32).T
    bound("zca transform", Y.rel_max(z.transform(X[:T]), gold["X_zca"]), Y.rel_max(ref32, gold["X_zca"]))
    one = z.transform(X[0])
    assert one.shape == (24,) and np.array_equal(one, z.transform(X[:1])[0])

    pz = wh.PCAZCAWhiteningModel.fit(X, pca_dim=12, device="cuda:0")
    pm, pc, pv = Y.pcazca_fit(X, 12, heavy=F32)
    bound("pca-zca components", float(np.abs(pz.pca_components - gold["pz_components"]).max()),
          float(np.abs(pc.astype(F32) - gold["pz_components"]).max()))
    bound("pca-zca variances", Y.rel_max(pz.pca_explained_var, gold["pz_explained_var"]),
          Y.rel_max(pv.astype(F32), gold["pz_explained_var"]))
    pc32, den32 = pc.astype(F32), np.sqrt(pv.astype(F32) + F32(1e-8))
    ref32 = (((X[:T] - pm.astype(F32)) @ pc32.T) / den32) @ pc32
    bound("pca-zca transform", Y.rel_max(pz.transform(X[:T]), gold["X_pcazca"]), Y.rel_max(ref32, gold["X_pcazca"]))
    xt = torch_gpu.from_numpy(X[:T]).cuda()
    out = pz.transform(xt)
    assert isinstance(out, torch_gpu.Tensor) and out.is_cuda and out.shape == (T, 24)


def test_gpu_fit_fraction_rule(pkg, torch_gpu, gold):
    """pca_dim = 0.96 keeps the reference's component count (10 of 24)."""
    pz = pkg.whitening.PCAZCAWhiteningModel.fit(gold["X"], pca_dim=0.96, device="cuda:0")
    assert pz.pca_components.shape == (int(gold["n_comp_096"][0]), 24) == (10, 24)
    m = pkg.whitening.PCAICAWhiteningModel.fit(gold["X"], pca_dim=0.96, backend="gpu", random_state=0, device="cuda:0",
                                               ica_max_iter=20)
    assert m.pca_components.shape == (10, 24) and m.ica_unmixing.shape == (10, 10)
    with pytest.raises(ValueError, match="w_init"):
        pkg.whitening.PCAICAWhiteningModel.fit(gold["X"], pca_dim=0.96, backend="gpu", w_init=np.eye(12),
                                               device="cuda:0")


def test_gpu_fit_device_tensor_and_numpy_agree(pkg, torch_gpu, gold, monkeypatch):
    W = pkg.whitening.PCAICAWhiteningModel
    kw = dict(pca_dim=12, w_init=gold["w_init"], backend="gpu", device="cuda:0")
    a = W.fit(gold["X"], **kw)
    b = W.fit(torch_gpu.from_numpy(gold["X"]).cuda(), **kw)
    for attr in ("mean", "pca_components", "pca_explained_var", "ica_unmixing"):
        assert np.array_equal(getattr(a, attr), getattr(b, attr)), attr
    assert a.ica_n_iter_ == b.ica_n_iter_
    # random_state: scikit-learn's draw (an int seeds a RandomState)
    c = W.fit(gold["X"], pca_dim=12, random_state=0, backend="gpu", device="cuda:0")
    assert np.array_equal(c.ica_unmixing, a.ica_unmixing)          # the fixture's w_init is RandomState(0)'s
    # numpy input above the chunk size: uploaded and accumulated in row chunks
    monkeypatch.setattr(pkg.whitening, "FIT_CHUNK", 1500)
    d = W.fit(gold["X"], **kw)
    assert np.abs(d.mean - a.mean).max() <= 1e-6 * np.abs(a.mean).max()
    assert np.abs(d.pca_components - a.pca_components).max() <= 1e-5
    mincos, rel, _ = Y.match_rows(d.ica_unmixing, a.ica_unmixing)
    print(f"chunked vs one chunk at the default tol: min|cos| {mincos:.9f} rel {rel:.3e}")
    assert mincos >= 0.999 and rel <= 2 * Y.ICA_VS_FIXTURE
