"""Golden vectors for the whitening fits, made by running the REAL reference classes
(src/whitening/pca_ica.py, zca.py, pca_zca.py under /root/reference, read-only) in the
build container: their own fit (scikit-learn PCA + FastICA, numpy eigh) and transform.

Run:  python tests/golden/gen_whiten_fit.py        (seconds)

The input is whiten_fit_yardstick.sources(4096, 24, 12, 11) cast to float64: on float32
input scikit-learn 1.7.2's FastICA returns a poor unmixing, so the
yardstick is the reference algorithm in float64.  pca_dim equals the number of sources;
the 0.96 variance fraction contributes its component count only.

Only data leaves this script (tests/golden/g11_whiten_fit.npz, under 1 MB): the input,
the fitted model parameters, the reference's outputs on the first T rows (all 4096 rows
of the three transforms would not fit the size limit) and FastICA's initial matrix (the
first draw of numpy's global generator after np.random.seed(0)).  Bytecode writing is
disabled; the GPU box never runs this script.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

from src.whitening.pca_ica import PCAICAWhiteningModel   # noqa: E402
from src.whitening.pca_zca import PCAZCAWhiteningModel   # noqa: E402
from src.whitening.zca import ZCAWhiteningModel          # noqa: E402
from whiten_fit_yardstick import sources                 # noqa: E402

T = 512


def main():
    warnings.filterwarnings("ignore")
    N, D, P = 4096, 24, 12
    X = sources(N, D, P, 11)
    X64 = X.astype(np.float64)
    w_init = np.random.RandomState(0).normal(size=(P, P))
    np.random.seed(0)   # FastICA's default random_state draws from numpy's global RNG
    m = PCAICAWhiteningModel.fit(X64, pca_dim=P)
    np.random.seed(0)
    m96 = PCAICAWhiteningModel.fit(X64, pca_dim=0.96)
    z = ZCAWhiteningModel.fit(X64)
    pz = PCAZCAWhiteningModel.fit(X64, pca_dim=P)
    out = dict(X=X, w_init=w_init, T=np.asarray([T], np.int64),
               mean=m.mean, pca_components=m.pca_components, pca_explained_var=m.pca_explained_var,
               ica_unmixing=m.ica_unmixing, eps=np.asarray([m.eps], np.float64),
               X_ica=m.transform(X64[:T]), X_pca=m.transform(X64[:T], is_ica=False),
               n_comp_096=np.asarray([m96.pca_components.shape[0]], np.int64),
               zca_mean=z.mean, zca_matrix=z.whitening_matrix, X_zca=z.transform(X64[:T]),
               pz_mean=pz.mean, pz_components=pz.pca_components, pz_explained_var=pz.pca_explained_var,
               X_pcazca=pz.transform(X64[:T]))
    for k, v in out.items():
        print(k, np.asarray(v).dtype, np.asarray(v).shape)
    path = os.path.join(OUT, "g11_whiten_fit.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
