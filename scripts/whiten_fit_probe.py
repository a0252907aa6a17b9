"""Stage times of the GPU whitening fit (PCAICAWhiteningModel.fit(backend="gpu")) on one MI355X
at n x 768 -> 256 (the C5 shape): the column sums, the covariance Gram, the host eigh, the
PCA transform, FastICA's own whitening, and per iteration cwq_ica_g, the G^T X1 Gram and the
host symmetric decorrelation; the two GEMM kernels' TFLOP/s against the 157.3 TF fp32 matrix
peak; the iteration count; and the scikit-learn fit (the default backend) on this machine's
CPU at a size it finishes in about a minute.  GPU only; no time here is a pass/fail condition.

    python scripts/whiten_fit_probe.py --n 2000000 --out profiles/whitenfit_probe.log
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cobweb_pkg  # noqa: E402

PEAK = 157.3


def device_sources(n, d, p, seed, dev, rows=1 << 18):
    """The tests' data recipe (tests/whiten_fit_yardstick.py sources) generated on the device:
    p/2 Laplace and p - p/2 uniform(-1.7, 1.7) sources scaled by linspace(1, 3, p), mixed by a
    standard-normal [p, d] matrix, plus 0.05 N(0, 1) noise, plus 0.5."""
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randn((p, d), generator=g, device=dev)
    scale = torch.linspace(1.0, 3.0, p, device=dev)
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    h = p // 2
    for i in range(0, n, rows):
        m = min(rows, n - i)
        lap = torch.empty((m, h), device=dev).exponential_(generator=g)
        lap = torch.where(torch.rand((m, h), generator=g, device=dev) < 0.5, -lap, lap)
        uni = (torch.rand((m, p - h), generator=g, device=dev) * 2.0 - 1.0) * 1.7
        S = torch.cat([lap, uni], dim=1) * scale
        X[i:i + m] = S @ A + 0.05 * torch.randn((m, d), generator=g, device=dev) + 0.5
    return X


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--p", type=int, default=256)
    ap.add_argument("--cpu-n", type=int, default=250_000, help="rows of the scikit-learn fit (0: skip)")
    ap.add_argument("--cpu-max-iter", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "whitenfit_probe.log"))
    a = ap.parse_args()
    pkg = cobweb_pkg.load()
    wh = pkg.whitening
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, "w")

    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    n, d, p = a.n, a.d, a.p
    say(f"whitening fit probe: {n} x {d} -> {p} on {torch.cuda.get_device_name(0)}, "
        f"slab {pkg.lib().cwq_whitenfit_slab()} rows, chunk {wh.FIT_CHUNK} rows, build {pkg.lib().cwq_build_id().decode()}")
    X = device_sources(n, d, p, 11, dev)
    torch.cuda.synchronize()

    # the passes on their own, one chunk resident in HBM
    c = X[:min(n, wh.FIT_CHUNK)]
    m = c.shape[0]
    ctr = (wh.col_sums(c) / m).to(torch.float32)
    t = timed(lambda: wh.col_sums(c))
    say(f"cwq_col_sums  {m} x {d}: {t * 1e3:8.2f} ms  {4.0 * m * d / t / 1e9:7.0f} GB/s")
    t = timed(lambda: wh.gram_acc(c, c, ctr, ctr))
    tiles = (d + 127) // 128
    done = tiles * (tiles + 1) / 2 / (tiles * tiles)
    say(f"cwq_gram_acc  {m} x {d} x {d} (A == B, {done:.2f} of the tiles computed): {t * 1e3:8.2f} ms  "
        f"{2.0 * m * d * d / t / 1e12:6.1f} TFLOP/s of the full product, {2.0 * m * d * d * done / t / 1e12:6.1f} "
        f"executed = {2.0 * m * d * d * done / t / 1e12 / PEAK:.2f} of the {PEAK} TF fp32 matrix peak")
    x1 = torch.randn((m, p), device=dev)
    w = torch.from_numpy(np.linalg.qr(np.random.default_rng(0).standard_normal((p, p)))[0].astype(np.float32)).to(dev)
    g, _ = wh.ica_g(x1, w)
    t = timed(lambda: wh.ica_g(x1, w, g))
    say(f"cwq_ica_g     {m} x {p}: {t * 1e3:8.2f} ms  {2.0 * m * p * p / t / 1e12:6.1f} TFLOP/s = "
        f"{2.0 * m * p * p / t / 1e12 / PEAK:.2f} of peak")
    t = timed(lambda: wh.gram_acc(g, x1))
    say(f"cwq_gram_acc  {m} x {p} x {p} (G^T X1): {t * 1e3:8.2f} ms  {2.0 * m * p * p / t / 1e12:6.1f} TFLOP/s = "
        f"{2.0 * m * p * p / t / 1e12 / PEAK:.2f} of peak")
    del x1, g

    # the fit
    w0 = np.random.RandomState(0).normal(size=(p, p))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = wh.PCAICAWhiteningModel.fit(X, pca_dim=p, w_init=w0, backend="gpu", device=dev)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    tm = model.fit_timing_
    it, sd = np.asarray(tm["iter_s"]), np.asarray(tm["symdec_s"])
    say(f"fit(backend='gpu') {n} x {d} -> {p}, tol 1e-3: {total:.2f} s, {model.ica_n_iter_} iterations")
    say(f"  mean + covariance (sums, Gram over {-(-n // wh.FIT_CHUNK)} chunks): {tm['mean_cov_s'] * 1e3:9.1f} ms")
    say(f"  host eigh {d} x {d} + sign / fraction rules:           {tm['pca_eigh_s'] * 1e3:9.1f} ms")
    say(f"  PCA transform to [n, {p}] (cwq_whiten):                 {tm['pca_transform_s'] * 1e3:9.1f} ms")
    say(f"  FastICA whitening (sums, Gram, eigh {p}, X1):           {tm['ica_whiten_s'] * 1e3:9.1f} ms")
    say(f"  iterations: {it.sum() * 1e3:9.1f} ms in all, median {np.median(it) * 1e3:.1f} ms each, of which the host "
        f"symmetric decorrelation {np.median(sd) * 1e3:.1f} ms ({sd.sum() / it.sum():.2f} of the iteration time)")
    out = model.transform(X)
    mu = wh.col_sums(out) / n
    cov = wh.gram_acc(out, out) / n - torch.outer(mu, mu)
    say(f"  transform of all rows: max |cov - I| = {(cov - torch.eye(p, device=dev)).abs().max().item():.2e}, "
        f"max |mean| = {mu.abs().max().item():.2e}")
    del out

    # the default backend on this machine's CPU, and the GPU fit on the same rows
    if a.cpu_n > 0:
        Xc = X[:a.cpu_n].cpu().numpy()
        w0 = np.random.RandomState(0).normal(size=(p, p))
        t0 = time.perf_counter()
        mg = wh.PCAICAWhiteningModel.fit(Xc, pca_dim=p, w_init=w0, backend="gpu", device=dev, ica_max_iter=a.cpu_max_iter)
        tg = time.perf_counter() - t0
        say(f"fit(backend='gpu')     {a.cpu_n} x {d} -> {p}: {tg:7.2f} s, {mg.ica_n_iter_} iterations (numpy input)")
        try:
            import sklearn
        except ImportError:
            say("fit(backend='sklearn'): scikit-learn is not importable on this machine; not timed")
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                ms = wh.PCAICAWhiteningModel.fit(Xc, pca_dim=p, w_init=w0, backend="sklearn", device=dev,
                                                 ica_max_iter=a.cpu_max_iter)
                ts = time.perf_counter() - t0
            say(f"fit(backend='sklearn') {a.cpu_n} x {d} -> {p}: {ts:7.2f} s, {ms.ica_n_iter_} iterations of at most "
                f"{a.cpu_max_iter} (scikit-learn {sklearn.__version__}, float32 input as the reference passes, "
                f"{os.environ.get('OMP_NUM_THREADS', '?')} threads)")
    log.close()


if __name__ == "__main__":
    main()
