"""Whitening fits, CPU side: the fp64 yardstick (tests/whiten_fit_yardstick.py) against the
real reference's fits (tests/golden/g11_whiten_fit.npz, made by tests/golden/gen_whiten_fit.py
on float64 input) and against scikit-learn, the variance-fraction rule, the argument checks
of PCAICAWhiteningModel.fit and the save/load round trips of the three models.

ICA fits are compared through the row matcher only (permutation and sign are free), on a
problem whose pca_dim equals the number of sources."""
import os
import warnings

import numpy as np
import pytest

import whiten_fit_yardstick as Y
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    g = load_golden("g11_whiten_fit")
    g["X64"] = g["X"].astype(np.float64)
    return g


def test_sources_recipe_is_the_fixture_input(gold):
    assert np.array_equal(Y.sources(4096, 24, 12, 11), gold["X"])
    assert np.array_equal(np.random.RandomState(0).normal(size=(12, 12)), gold["w_init"])


def test_yardstick_pca_matches_reference(gold):
    mean, comps, var = Y.pca_fit(gold["X64"], 12)
    print("pca vs reference: mean", Y.rel_max(mean, gold["mean"]), "components",
          np.abs(comps - gold["pca_components"]).max(), "variance", Y.rel_max(var, gold["pca_explained_var"]))
    assert Y.rel_max(mean, gold["mean"]) < 1e-12
    assert np.abs(comps - gold["pca_components"]).max() < 1e-6       # the issue measured 4e-7
    assert Y.rel_max(var, gold["pca_explained_var"]) < 1e-6          # 2e-7
    T = int(gold["T"][0])
    eps = float(gold["eps"][0])
    xp = Y.whiten(gold["X64"][:T], mean, comps, np.sqrt(var + eps))
    assert Y.rel_max(xp, gold["X_pca"]) < 1e-6


def test_yardstick_ica_matches_reference_rows(gold):
    r = Y.pcaica_fit(gold["X64"], 12, gold["w_init"])               # default tol, as the fixture
    mincos, rel, um = Y.match_rows(r["ica_unmixing"], gold["ica_unmixing"])
    print("ica vs reference rows: min|cos|", mincos, "max rel L2", rel, "iterations", r["n_iter"])
    assert mincos >= 0.99999
    assert rel <= 4.1e-3                                             # the issue's CPU measurement
    assert rel <= Y.ICA_VS_FIXTURE
    # the matched model transforms like the reference's, up to the same permutation and sign
    T = int(gold["T"][0])
    out = Y.pcaica_transform(gold["X64"][:T], r["mean"], r["pca_components"], r["pca_explained_var"], um)
    assert Y.rel_max(out, gold["X_ica"]) <= 2 * 4.1e-3


def test_yardstick_f32_variant_matches_f64(gold):
    """The E_ref variant (heavy passes in float32) lands on the fp64 fit's components."""
    a = Y.pcaica_fit(gold["X64"], 12, gold["w_init"], tol=1e-6)
    b = Y.pcaica_fit(gold["X"], 12, gold["w_init"], tol=1e-6, heavy=np.float32)
    mincos, rel, _ = Y.match_rows(b["ica_unmixing"], a["ica_unmixing"])
    print("float32 variant vs fp64: min|cos|", mincos, "rel", rel, "iterations", b["n_iter"], a["n_iter"])
    assert mincos >= 0.999 and rel <= 2.4e-4
    assert abs(a["n_iter"] - b["n_iter"]) <= 3


def test_yardstick_matches_sklearn_float64(gold):
    dec = pytest.importorskip("sklearn.decomposition")
    X = gold["X64"]
    pca = dec.PCA(n_components=12)
    xp = pca.fit_transform(X - X.mean(0))
    mean, comps, var = Y.pca_fit(X, 12)
    assert np.abs(comps - pca.components_).max() < 1e-6
    assert Y.rel_max(var, pca.explained_variance_) < 1e-6
    xn = xp / np.sqrt(pca.explained_variance_ + 1e-8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ica = dec.FastICA(n_components=12, whiten="unit-variance", max_iter=5000, tol=1e-6, w_init=gold["w_init"])
        ica.fit(xn)
    mine, n_iter = Y.fastica(xn, gold["w_init"], tol=1e-6)
    mincos, rel, _ = Y.match_rows(mine, ica.components_)
    print("fastica vs scikit-learn float64 at tol 1e-6: min|cos|", mincos, "rel", rel, "iterations", n_iter,
          ica.n_iter_)
    assert mincos >= 0.99999 and rel <= 2.4e-4    # both within tol of the fixed point, like float32 vs fp64


def test_fraction_rule(gold):
    """pca_dim = 0.96 keeps 10 components on this X, as the reference (PCA(n_components=0.96)) does."""
    assert int(gold["n_comp_096"][0]) == 10
    mean, comps, var = Y.pca_fit(gold["X64"], 0.96)
    assert comps.shape == (10, 24) and var.shape == (10,)
    full = Y.pca_fit(gold["X64"], 12)
    assert np.array_equal(comps, full[1][:10]) and np.array_equal(var, full[2][:10])


def test_yardstick_zca_and_pcazca_match_reference(gold):
    T = int(gold["T"][0])
    mean, wm = Y.zca_fit(gold["X64"])
    assert Y.rel_max(mean, gold["zca_mean"]) < 1e-12 and Y.rel_max(wm, gold["zca_matrix"]) < 1e-9
    assert Y.rel_max(Y.zca_transform(gold["X64"][:T], mean, wm), gold["X_zca"]) < 1e-9
    mean, comps, var = Y.pcazca_fit(gold["X64"], 12)
    assert np.abs(comps - gold["pz_components"]).max() < 1e-6
    assert Y.rel_max(var, gold["pz_explained_var"]) < 1e-6
    assert Y.rel_max(Y.pcazca_transform(gold["X64"][:T], mean, comps, var), gold["X_pcazca"]) < 1e-6


def test_match_rows_undoes_permutation_and_sign():
    rng = np.random.default_rng(0)
    V = rng.standard_normal((7, 7))
    perm = rng.permutation(7)
    sg = rng.choice([-1.0, 1.0], 7)
    mincos, rel, um = Y.match_rows((V * sg[:, None])[perm], V)
    assert mincos > 1 - 1e-12 and rel < 1e-12 and np.allclose(um, V)


def test_fit_argument_errors(pkg, gold):
    """Checked before any device work: no GPU here."""
    W = pkg.whitening.PCAICAWhiteningModel
    X = gold["X"][:64]
    with pytest.raises(ValueError, match="backend"):
        W.fit(X, pca_dim=4, backend="cuda")
    with pytest.raises(ValueError, match="w_init"):
        W.fit(X, pca_dim=4, backend="gpu", w_init=np.zeros((4, 3)))
    with pytest.raises(ValueError, match="w_init"):
        W.fit(X, pca_dim=4, backend="gpu", w_init=np.zeros((5, 5)))
    with pytest.raises(ValueError, match="w_init"):
        W.fit(X, pca_dim=4, backend="sklearn", w_init=np.zeros((5, 5)))


def test_fit_c_abi_argument_errors(pkg):
    """CWQ_ERR_ARG before any device work; n == 0 is a no-op."""
    import ctypes
    L, E = pkg.lib(), pkg._lib.CWQ_ERR_ARG
    p = ctypes.c_void_p(256)     # never dereferenced
    assert L.cwq_whitenfit_slab() >= 1024
    assert L.cwq_col_sums(None, 5, 3, p, p, None) == E and b"NULL" in L.cwq_last_error()
    assert L.cwq_col_sums(p, -1, 3, p, p, None) == E
    assert L.cwq_col_sums(p, 5, 0, p, p, None) == E
    assert L.cwq_col_sums(p, 5, 1025, p, p, None) == E
    assert L.cwq_col_sums(p, 0, 3, p, p, None) == 0
    assert L.cwq_gram_acc(p, None, 5, 3, 3, None, None, p, p, None) == E
    assert L.cwq_gram_acc(p, p, 5, 3, 1025, None, None, p, p, None) == E
    assert L.cwq_gram_acc(p, p, 5, 0, 3, None, None, p, p, None) == E
    assert L.cwq_gram_acc(p, p, -2, 3, 3, None, None, p, p, None) == E
    assert L.cwq_gram_acc(p, p, 5, 3, 3, None, None, p, None, None) == E
    assert L.cwq_gram_acc(p, p, 0, 3, 3, None, None, p, p, None) == 0
    assert L.cwq_ica_g(p, 5, 3, p, p, None, p, None) == E
    assert L.cwq_ica_g(p, 5, 2000, p, p, p, p, None) == E
    assert L.cwq_ica_g(p, -1, 3, p, p, p, p, None) == E
    assert L.cwq_ica_g(p, 0, 3, p, p, p, p, None) == 0
    slab = L.cwq_whitenfit_slab()
    assert L.cwq_col_sums_work_bytes(2 * slab + 1, 7) == 3 * 7 * 8
    assert L.cwq_gram_acc_work_bytes(2 * slab + 1, 7, 5) == 3 * 7 * 5 * 4
    assert L.cwq_ica_g_work_bytes(257, 9) == 3 * 9 * 8
    assert L.cwq_gram_acc_work_bytes(10, 7, 1025) == -1


def test_save_load_round_trips(pkg, gold, tmp_path):
    wh = pkg.whitening
    eps = float(gold["eps"][0])
    models = [
        (wh.PCAICAWhiteningModel(gold["mean"], gold["pca_components"], gold["ica_unmixing"],
                                 gold["pca_explained_var"], eps, device="cpu"),
         ("mean", "pca_components", "pca_explained_var", "ica_unmixing")),
        (wh.ZCAWhiteningModel(gold["zca_mean"], gold["zca_matrix"], eps, device="cpu"), ("mean", "whitening_matrix")),
        (wh.PCAZCAWhiteningModel(gold["pz_mean"], gold["pz_components"], gold["pz_explained_var"], eps, device="cpu"),
         ("mean", "pca_components", "pca_explained_var")),
    ]
    for i, (m, attrs) in enumerate(models):
        path = os.path.join(tmp_path, f"m{i}.npz")
        m.save(path)
        m2 = type(m).load(path, device="cpu")
        for a in attrs:
            assert getattr(m2, a).dtype == np.float32 and np.array_equal(getattr(m, a), getattr(m2, a)), a
        assert m2.eps == eps
        assert type(m).__name__ in repr(m2)
