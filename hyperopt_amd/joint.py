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


# ------------------------------------------------------------ mixed groups
# A joint group may also hold discrete labels (randint / categorical): the
# kernel coordinates are the continuous labels in table order, then the discrete
# ones in table order (include/tpe_hip.h "Mixed joint stage").  Discrete
# dimension d has U_d categories with prior p_d; on a side with n trials and the
# smoothing mass s_d = prior_weight U_d / (n + 1) the component of a trial that
# observed x is P(v) = (1[v = x] + s_d p_d(v)) / (1 + s_d), and the prior row's
# is p_d.  A component's category -1 marks the prior row.
DISCRETE_DISTS = ('randint', 'categorical')


def discrete_reason(row, table):
    """Why ``row`` cannot be joined as a discrete dimension, or None if it can."""
    if not all(p is None for p in row.parents) or row.depth != 0:
        return 'conditional (%s)' % row.dist
    if row.dist.startswith('q'):
        return 'a quantised label (%s)' % row.dist
    if row.dist not in DISCRETE_DISTS:
        return 'not a randint or categorical label (%s)' % row.dist
    if row.label in table.parent_labels:
        return ('a gate: its value routes other labels, and a joint override would pick values for the wrong '
                'branch')
    if int(row.args['upper']) < 2:
        return '%d category, fewer than 2: nothing to choose' % int(row.args['upper'])
    if int(row.args['upper']) > N.JOINT_MAX_CATS:
        return '%d categories, more than %d' % (int(row.args['upper']), N.JOINT_MAX_CATS)
    if row.dist == 'categorical' and not (np.asarray(row.args['p'], dtype=np.float64) > 0).all():
        return 'a prior probability of 0'
    return None


def eligible_discrete(row, table):
    """Whether a ParamRow can be joined as a discrete dimension: unconditional
    randint / categorical, no label's parent, 2 to 256 categories, no prior
    probability 0."""
    return discrete_reason(row, table) is None


def cat_prior(dist, args):
    """p_d [U_d] of a joinable discrete label."""
    U = int(args['upper'])
    if dist == 'randint':
        return np.full(U, 1.0 / U)
    p = np.asarray(args['p'], dtype=np.float64)
    return p / p.sum()


def smoothing(prior_weight, U, n):
    """s_d of a side with n trials."""
    return prior_weight * U / (n + 1.0)


def mixed_side_mixture(X, priors, XC, prior_weight=1.0, lf=DEFAULT_LF):
    """(w, mu, sigma, xc) of one side: (w, mu, sigma) are side_mixture's over
    the continuous part ``X`` [n, Dc]; xc [n + 1, Dk] int64 the components'
    categories, row 0 (the prior) -1, row 1 + t trial t's ``XC`` [n, Dk]."""
    XC = np.asarray(XC, dtype=np.int64)
    if XC.ndim == 1:
        XC = XC[:, None]
    n = len(XC)
    if len(priors):
        w, mu, sigma = side_mixture(np.asarray(X, dtype=np.float64).reshape(n, len(priors)), priors, prior_weight, lf)
    else:                                        # an all-discrete group: side_mixture's weights alone
        w = np.empty(n + 1)
        w[0] = prior_weight
        w[1:] = linear_forgetting_weights(n, lf) if (lf and lf < n) else 1.0
        w /= w.sum()
        mu = sigma = np.zeros((n + 1, 0))
    xc = np.vstack([np.full((1, XC.shape[1]), -1, dtype=np.int64), XC])
    return w, mu, sigma, xc


def discrete_tables(p, s):
    """float64 (miss [U], bonus [U], corr) of one dimension on one side, log2:
    log2 P_kd(v) = miss[v] + bonus[v] 1[v = x_kd] for a trial's component and
    miss[v] + corr for the prior row."""
    p = np.asarray(p, dtype=np.float64)
    miss = (np.log(s * p) - np.log1p(s)) * LOG2E
    bonus = np.log1p(1.0 / (s * p)) * LOG2E
    corr = (np.log1p(s) - np.log(s)) * LOG2E
    return miss, bonus, corr


def mixed_density_rows(w, mu, sigma, low, high, xc, ps, s):
    """density_rows of a mixed side: f32 (mu [K, Dc], a [K, Dc], c [K]), the
    float64 base, f32 cat [K, Dk] and the flat f32 (miss, bonus) [sum U_d].
    c carries the prior rows' correction (category -1) before the shift."""
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low, dtype=np.float64)[None, :],
                            np.asarray(high, dtype=np.float64)[None, :])
    with np.errstate(divide='ignore'):
        logc = np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)
    c = logc * LOG2E
    miss, bonus = [], []
    for d, p in enumerate(ps):
        mi, bo, corr = discrete_tables(p, s[d])
        miss.append(mi)
        bonus.append(bo)
        c = c + np.where(xc[:, d] < 0, corr, 0.0)
    fin = np.isfinite(c)
    shift = float(np.max(c[fin])) if fin.any() else 0.0
    return (np.ascontiguousarray(mu, dtype=np.float32), np.ascontiguousarray(A_SCALE / sigma, dtype=np.float32),
            np.ascontiguousarray(c - shift, dtype=np.float32), shift * math.log(2.0),
            np.ascontiguousarray(xc, dtype=np.float32), np.concatenate(miss).astype(np.float32),
            np.concatenate(bonus).astype(np.float32))


def mixed_sampler_rows(w, mu, sigma, low, high, ps, s):
    """sampler_rows of the below side plus float64 (h [Dk], cat_cum [sum U_d]):
    h_d = 1 / (1 + s_d) the probability that a trial's component repeats its
    category, cat_cum the cumsum of each p_d with its last entry 1.  cum and
    rows do not depend on the discrete dimensions."""
    cum, rows = sampler_rows(w, np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64), low, high)
    h = 1.0 / (1.0 + np.asarray(s, dtype=np.float64))
    cc = []
    for p in ps:
        q = np.cumsum(np.asarray(p, dtype=np.float64))
        q[-1] = 1.0
        cc.append(q)
    return cum, rows, np.ascontiguousarray(h), np.concatenate(cc)


def mixed_lpdf_numpy(z, v, w, mu, sigma, low, high, xc, ps, s, block=1 << 14):
    """The mixed model's float64 log-density at continuous ``z`` [C, Dc] and
    categories ``v`` [C, Dk]."""
    v = np.asarray(v, dtype=np.int64)
    C = len(v)
    z = np.asarray(z, dtype=np.float64).reshape(C, mu.shape[1])
    fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low, dtype=np.float64)[None, :],
                            np.asarray(high, dtype=np.float64)[None, :])
    logc = np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)
    out = np.empty(C)
    step = max(1, block // max(1, len(w) // 64 + 1))
    for lo in range(0, C, step):
        zz, vv = z[lo:lo + step], v[lo:lo + step]
        t = logc[None, :].repeat(len(vv), axis=0)
        for d in range(z.shape[1]):
            t -= 0.5 * ((zz[:, d, None] - mu[None, :, d]) / sigma[None, :, d]) ** 2
        for d, p in enumerate(ps):
            p = np.asarray(p, dtype=np.float64)
            pv = p[vv[:, d]][:, None]
            hit = vv[:, d, None] == xc[None, :, d]
            t += np.log(np.where(xc[None, :, d] < 0, pv, (hit + s[d] * pv) / (1.0 + s[d])))
        m = t.max(axis=1)
        out[lo:lo + step] = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
    return out


class MixedModel(object):
    """The two mixtures of a mixed joint group: ``rows`` the continuous
    ParamRows, ``drows`` the discrete ones (kernel coordinate order: rows, then
    drows), ``below`` / ``above`` = (w, mu, sigma, xc), ``ps`` the priors and
    ``s_below`` / ``s_above`` [Dk] the smoothing masses."""
    __slots__ = ('rows', 'drows', 'below', 'above', 'low', 'high', 'ps', 's_below', 's_above')

    def __init__(self, rows, drows, below, above, low, high, ps, s_below, s_above):
        self.rows, self.drows, self.below, self.above = list(rows), list(drows), below, above
        self.low, self.high, self.ps, self.s_below, self.s_above = low, high, ps, s_below, s_above

    def cats(self):
        """The ``cats`` argument of Engine.run_joint_mixed."""
        return [(self.below[3][:, d], self.above[3][:, d], self.ps[d], self.s_below[d], self.s_above[d])
                for d in range(len(self.drows))]

    def values(self, z):
        """Label values of kernel coordinates z [.., Dc + Dk]."""
        z = np.array(z, dtype=np.float64)
        for d, r in enumerate(self.rows):
            if r.dist in LOG_DISTS:
                z[..., d] = np.exp(z[..., d])
        return z


def fit_mixed_model(rows, drows, hist, below_tids, prior_weight=1.0, lf=DEFAULT_LF):
    """MixedModel of the eligible continuous ``rows`` and discrete ``drows``
    from a History and its below set."""
    pb = [prior_and_bounds(r.dist, r.args) for r in rows]
    tids = None
    cols, ccols = [], []
    first = (list(rows) + list(drows))[0]
    for r in list(rows) + list(drows):
        otids, ovals = hist.obs[r.label]
        otids = np.asarray(otids, dtype=np.int64)
        if tids is None:
            tids = otids
        elif len(otids) != len(tids) or (otids != tids).any():
            raise ValueError('joint label %r is not observed in the same trials as %r' % (r.label, first.label))
        if r.dist in DISCRETE_DISTS:
            ovals = np.asarray(ovals, dtype=np.int64)
            if len(ovals) and (ovals.min() < 0 or ovals.max() >= int(r.args['upper'])):
                raise IndexError('categorical observation of %r out of range [0, %d)' % (r.label, int(r.args['upper'])))
            ccols.append(ovals)
        else:
            cols.append(fit_coord(r.dist, r.args, ovals))
    n = len(tids)
    X = np.stack(cols, axis=1) if cols else np.zeros((n, 0))
    XC = np.stack(ccols, axis=1) if ccols else np.zeros((n, 0), dtype=np.int64)
    order = np.argsort(tids, kind='stable')
    X, XC, tids = X[order], XC[order], tids[order]
    m = np.isin(tids, np.asarray(below_tids, dtype=np.int64))
    priors = [(p[0], p[1]) for p in pb]
    ps = [cat_prior(r.dist, r.args) for r in drows]
    nb, na = int(m.sum()), int((~m).sum())
    return MixedModel(rows, drows, mixed_side_mixture(X[m], priors, XC[m], prior_weight, lf),
                      mixed_side_mixture(X[~m], priors, XC[~m], prior_weight, lf),
                      np.array([p[2] for p in pb], dtype=np.float64), np.array([p[3] for p in pb], dtype=np.float64),
                      ps, np.array([smoothing(prior_weight, len(p), nb) for p in ps]),
                      np.array([smoothing(prior_weight, len(p), na) for p in ps]))
