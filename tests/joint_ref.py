"""The joint TPE model restated in plain numpy (DESIGN.md "Joint TPE"), for the
joint tests: nothing here calls hyperopt_amd.joint or the native library."""
import numpy as np
from scipy.special import logsumexp, ndtr

LF = 25


def ref_sigmas(x, pmu, psig):
    """Bandwidth of each observation of the column x (tid order): stable sort,
    prior inserted at searchsorted (left), the larger neighbour gap (one-sided
    at the ends), clipped to [psig / min(100, n + 2), psig], un-permuted."""
    x = np.asarray(x, dtype=float)
    n = len(x)
    if n == 0:
        return np.zeros(0)
    order = np.argsort(x, kind='stable')
    srt = x[order]
    pos = int(np.searchsorted(srt, pmu, side='left'))
    mu = np.concatenate([srt[:pos], [pmu], srt[pos:]])
    sig = np.empty(n + 1)
    sig[0] = mu[1] - mu[0]
    sig[-1] = mu[-1] - mu[-2]
    sig[1:-1] = np.maximum(mu[1:-1] - mu[:-2], mu[2:] - mu[1:-1])
    if n == 1:                                       # (the reference's one-observation case)
        sig[:] = psig * 0.5
    sig = np.clip(sig, psig / min(100.0, n + 2.0), psig)
    sig = np.delete(sig, pos)                        # the observations, sorted
    out = np.empty(n)
    out[order] = sig
    return out


def ref_side(X, pmu, psig, prior_weight=1.0):
    """(w [n+1], mu [n+1, D], sigma [n+1, D]): row 0 the prior, row 1 + t trial t."""
    X = np.asarray(X, dtype=float).reshape(-1, len(pmu))
    n, D = X.shape
    w = np.ones(n + 1)
    w[0] = prior_weight
    if n > LF:
        w[1:] = np.concatenate([np.linspace(1.0 / n, 1.0, num=n - LF), np.ones(LF)])
    w = w / w.sum()
    mu = np.vstack([np.asarray(pmu, dtype=float)[None, :], X])
    sigma = np.vstack([np.asarray(psig, dtype=float)[None, :],
                       np.stack([ref_sigmas(X[:, d], pmu[d], psig[d]) for d in range(D)], axis=1).reshape(n, D)])
    return w, mu, sigma


def ref_logcoef(w, mu, sigma, low, high):
    mass = ndtr((np.asarray(high)[None, :] - mu) / sigma) - ndtr((np.asarray(low)[None, :] - mu) / sigma)
    return np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi) * mass), axis=1)


def ref_lpdf(z, side, low, high, block=2048):
    """float64 log-density of the product-kernel mixture at z [C, D]."""
    w, mu, sigma = side
    z = np.asarray(z, dtype=np.float64)
    lc = ref_logcoef(w, mu, sigma, low, high)
    out = np.empty(len(z))
    for lo in range(0, len(z), block):
        zz = z[lo:lo + block]
        q = ((zz[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2
        out[lo:lo + block] = logsumexp(lc[None, :] - 0.5 * q.sum(axis=2), axis=1)
    return out


def tie_set(l_ref, g_ref, tol=1e-5):
    """Indices within 4 lpdf bounds of the best float64 score (test_gpu_kernels._check_argmax)."""
    score = np.asarray(l_ref) - np.asarray(g_ref)
    eps = 4 * tol * max(1.0, float(np.max(np.abs(l_ref))), float(np.max(np.abs(g_ref))))
    return np.nonzero(score >= np.nanmax(score) - eps)[0], score


def check_lpdf(got, ref, what, tol=1e-5):
    """|got - ref| <= tol * max(1, |ref|) (test_gpu_kernels._check_lpdf); returns the worst ratio."""
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got)), what
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    print('%s: max err / tol = %.3f' % (what, float(err.max()) / tol))
    assert err.max() <= tol, (what, float(err.max()), int(np.argmax(err)))
    return float(err.max()) / tol


def seeded_case(D, n, seed, n_below=None):
    """A seeded joint case: D dimensions (even ones bounded to [-10, 10) with the
    uniform prior, odd ones unbounded with prior N(1, 4)), n trials split into
    below / above; returns (below side, above side, low, high, pmu, psig)."""
    rs = np.random.RandomState(seed)
    bounded = np.arange(D) % 2 == 0
    low = np.where(bounded, -10.0, -np.inf)
    high = np.where(bounded, 10.0, np.inf)
    pmu = np.where(bounded, 0.0, 1.0)
    psig = np.where(bounded, 20.0, 4.0)
    X = np.where(bounded[None, :], rs.uniform(-10, 10, (n, D)), rs.normal(1.0, 4.0, (n, D)))
    nb = n_below if n_below is not None else min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    loss = rs.uniform(size=n)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    return ref_side(X[m], pmu, psig), ref_side(X[~m], pmu, psig), low, high, pmu, psig
