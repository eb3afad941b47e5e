"""Host side of joint (multivariate) TPE: the product-kernel mixtures of a group
of continuous labels and their device rows (include/tpe_hip.h "Joint
(multivariate) TPE stage"; DESIGN.md "Joint TPE").

A side (below / above) with n trials has n + 1 components: row 0 is the prior,
row 1 + t is trial t (tid order).  Every per-dimension quantity is the
univariate adaptive Parzen fit's (parzen.fit_parzen), un-permuted from its
sorted order back to trial order, so the joint model's marginal on a dimension
is that label's univariate mixture up to how truncation is normalised.
"""
import math

import numpy as np
from scipy.special import erfc

from . import _native as N
from .parzen import A_SCALE, DEFAULT_LF, LOG2E, fit_coord, linear_forgetting_weights

JOINT_DISTS = ('uniform', 'loguniform', 'normal', 'lognormal')
LOG_DISTS = ('loguniform', 'lognormal')


def eligible(row):
    """Whether a ParamRow can be joined: unconditional and continuous."""
    return row.dist in JOINT_DISTS and all(p is None for p in row.parents) and row.depth == 0


def prior_and_bounds(dist, args):
    """(prior mu, prior sigma, low, high) of a joinable label in its fit
    coordinate, as parzen.fit_posterior derives them (+-inf: unbounded)."""
    if dist in ('uniform', 'loguniform'):
        low, high = float(args['low']), float(args['high'])
        return 0.5 * (args['high'] + args['low']), 1.0 * (args['high'] - args['low']), low, high
    return float(args['mu']), float(args['sigma']), -np.inf, np.inf


def trial_sigmas(x, prior_mu, prior_sigma, lf=DEFAULT_LF):
    """The bandwidth adaptive_parzen_normal gives each observation of the column
    ``x`` (tid order): the native univariate fit under a STABLE sort (equal
    values in tid order, the device fit's tie rule), un-permuted."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0)
    order = np.ascontiguousarray(np.argsort(x, kind='stable'), dtype=np.int64)
    w, mu, sigma = np.empty(n + 1), np.empty(n + 1), np.empty(n + 1)
    pos = N.load().tpe_host_fit_parzen(x.ctypes.data, n, order.ctypes.data if n >= 2 else None, 1.0, float(prior_mu),
                                       float(prior_sigma), int(lf or 0), w.ctypes.data, mu.ctypes.data,
                                       sigma.ctypes.data)
    if pos < 0:
        raise AssertionError('non-positive Parzen bandwidth (prior_sigma=%r)' % prior_sigma)
    j = np.arange(n)
    out = np.empty(n)
    out[order] = sigma[j + (j >= pos)]
    return out


def side_mixture(X, priors, prior_weight=1.0, lf=DEFAULT_LF):
    """(w [n+1], mu [n+1, D], sigma [n+1, D]) of one side: ``X`` [n, D] the
    trials' fit coordinates in tid order, ``priors`` D (mu, sigma) pairs."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, len(priors))
    n, D = X.shape
    w = np.empty(n + 1)
    w[0] = prior_weight
    w[1:] = linear_forgetting_weights(n, lf) if (lf and lf < n) else 1.0
    w /= w.sum()
    mu, sigma = np.empty((n + 1, D)), np.empty((n + 1, D))
    for d, (pmu, psig) in enumerate(priors):
        mu[0, d], sigma[0, d] = pmu, psig
        mu[1:, d] = X[:, d]
        sigma[1:, d] = trial_sigmas(X[:, d], pmu, psig, lf)
    return w, mu, sigma


def _std_bounds(mu, sigma, low, high):
    """Phi of the standardised bounds, mirrored where the interval lies right
    of 0 so both keep relative precision: (fa, fb, flip)."""
    za, zb = (low - mu) / sigma, (high - mu) / sigma
    flip = za > 0
    a, b = np.where(flip, -zb, za), np.where(flip, -za, zb)
    return 0.5 * erfc(-a / np.sqrt(2)), 0.5 * erfc(-b / np.sqrt(2)), flip


def density_rows(w, mu, sigma, low, high):
    """f32 (mu [K, D], a [K, D], c [K]) and the float64 base of one side."""
    fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low)[None, :], np.asarray(high)[None, :])
    with np.errstate(divide='ignore'):
        logc = np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)
    c = logc * LOG2E
    fin = np.isfinite(c)
    shift = float(np.max(c[fin])) if fin.any() else 0.0
    return (np.ascontiguousarray(mu, dtype=np.float32), np.ascontiguousarray(A_SCALE / sigma, dtype=np.float32),
            np.ascontiguousarray(c - shift, dtype=np.float32), shift * math.log(2.0))


def sampler_rows(w, mu, sigma, low, high):
    """(cum [K] float64, rows [K, D, 5] f32 {mu, sigma, fa, fb, flip}) of the
    below side: component k with probability w_k, then per dimension a normal
    truncated to the label's bounds, drawn by inversion."""
    fa, fb, flip = _std_bounds(mu, sigma, np.asarray(low)[None, :], np.asarray(high)[None, :])
    cum = np.cumsum(w) / np.sum(w)
    cum[-1] = 1.0
    rows = np.stack([mu, sigma, fa, fb, flip.astype(np.float64)], axis=2)
    return np.ascontiguousarray(cum, dtype=np.float64), np.ascontiguousarray(rows, dtype=np.float32)


def lpdf_numpy(z, w, mu, sigma, low, high, block=1 << 14):
    """The model's float64 log-density at ``z`` [C, D] (the specification the
    device stage is tested against; tools/joint_time.py's host route)."""
    z = np.asarray(z, dtype=np.float64)
    fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low)[None, :], np.asarray(high)[None, :])
    logc = np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)
    out = np.empty(len(z))
    step = max(1, block // max(1, len(w) // 64 + 1))
    for lo in range(0, len(z), step):
        zz = z[lo:lo + step]
        t = logc[None, :].repeat(len(zz), axis=0)
        for d in range(z.shape[1]):
            t -= 0.5 * ((zz[:, d, None] - mu[None, :, d]) / sigma[None, :, d]) ** 2
        m = t.max(axis=1)
        out[lo:lo + step] = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
    return out


class JointModel(object):
    """The two mixtures of a joint group: ``rows`` the joined ParamRows,
    ``below`` / ``above`` = (w, mu, sigma), ``low`` / ``high`` [D]."""
    __slots__ = ('rows', 'below', 'above', 'low', 'high')

    def __init__(self, rows, below, above, low, high):
        self.rows, self.below, self.above, self.low, self.high = list(rows), below, above, low, high

    def values(self, z):
        """Label values of coordinates z [.., D]: exp for the log families."""
        z = np.array(z, dtype=np.float64)
        for d, r in enumerate(self.rows):
            if r.dist in LOG_DISTS:
                z[..., d] = np.exp(z[..., d])
        return z


def fit_model(rows, hist, below_tids, prior_weight=1.0, lf=DEFAULT_LF):
    """JointModel of ``rows`` (eligible labels: every trial observes each of
    them) from a History and its below set."""
    pb = [prior_and_bounds(r.dist, r.args) for r in rows]
    tids = None
    cols = []
    for r in rows:
        otids, ovals = hist.obs[r.label]
        otids = np.asarray(otids, dtype=np.int64)
        if tids is None:
            tids = otids
        elif len(otids) != len(tids) or (otids != tids).any():
            raise ValueError('joint label %r is not observed in the same trials as %r' % (r.label, rows[0].label))
        cols.append(fit_coord(r.dist, r.args, ovals))
    X = np.stack(cols, axis=1)
    order = np.argsort(tids, kind='stable')
    X, tids = X[order], tids[order]
    m = np.isin(tids, np.asarray(below_tids, dtype=np.int64))
    priors = [(p[0], p[1]) for p in pb]
    return JointModel(rows, side_mixture(X[m], priors, prior_weight, lf), side_mixture(X[~m], priors, prior_weight, lf),
                      np.array([p[2] for p in pb]), np.array([p[3] for p in pb]))
