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


def f32_bounds(low, high):
    """f32 (lo [D], hi [D]) the kernels clip a drawn coordinate to, as
    tpe_joint_run derives them: the smallest float >= low_d and the largest
    float < high_d (-inf / +inf where unbounded)."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    lo, hi = low.astype(np.float32), high.astype(np.float32)
    up = np.isfinite(low) & (lo.astype(np.float64) < low)
    lo[up] = np.nextafter(lo[up], np.float32(np.inf))
    for d in np.flatnonzero(np.isfinite(high)):
        while float(hi[d]) >= high[d]:
            hi[d] = np.nextafter(hi[d], np.float32(-np.inf))
    return lo, hi


def branch_stream_word(rows):
    """The Philox stream word of a branch group (DESIGN.md "Branch groups"):
    0xFFFFFFFE - the lowest table index among its labels (all of them: the
    discrete and quantised ones of a widened group too).  It depends on the
    space alone, differs between groups (a label is in one group), and is at
    least 2^31, so it equals no univariate label index and not N.JOINT_STREAM."""
    return 0xFFFFFFFE - min(r.index for r in rows)


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


def discrete_reason(row, table, conditional=False):
    """Why ``row`` cannot be joined as a discrete dimension, or None if it can.
    ``conditional``: the label may be conditional (a branch group's label,
    tpe.suggest_choices' ``joint_branches_mixed``); every other test holds."""
    if not conditional and (not all(p is None for p in row.parents) or row.depth != 0):
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


# -------------------------------------------------------- quantised groups
# A joint group may also hold quantised labels (quniform / qloguniform): the
# kernel coordinates are the continuous labels, the discrete ones, then the
# quantised ones, each in table order (include/tpe_hip.h "Quantised joint
# stage").  A quantised label is a continuous dimension of the model observed
# through bins: lattice index i stands for the value (m_lo + i) q and takes the
# component's mass on [e_i, e_{i+1}) over its mass on [low, high).
QUANT_DISTS = ('quniform', 'qloguniform')
SQRT1_2 = math.sqrt(0.5)
QUANT_TAIL_MAX = 26.5       # |e - mu| / (sigma sqrt 2) beyond which a tail (below 2^-1018) counts as exactly 0


def lattice_size(dist, args):
    """(m_lo, V, q) of a quniform / qloguniform label with q > 0: m_lo the
    smallest integer m with (m + 1/2) q > lo_v (not below 0 for qloguniform),
    m_hi the largest with (m - 1/2) q < hi_v, V = m_hi - m_lo + 1; lo_v, hi_v the
    bounds as values.  A value whose clipped bin would be empty is not in the
    lattice (quniform(0, 3.5, 1): V = 4)."""
    q = float(args['q'])
    lo, hi = float(args['low']), float(args['high'])
    if dist == 'qloguniform':
        lo, hi = math.exp(lo), math.exp(hi)
    m_lo = int(math.floor(lo / q - 0.5)) + 1
    while (m_lo - 1 + 0.5) * q > lo:
        m_lo -= 1
    while not (m_lo + 0.5) * q > lo:
        m_lo += 1
    m_hi = int(math.ceil(hi / q + 0.5)) - 1
    while (m_hi + 1 - 0.5) * q < hi:
        m_hi += 1
    while not (m_hi - 0.5) * q < hi:
        m_hi -= 1
    if dist == 'qloguniform':
        m_lo = max(m_lo, 0)
    return m_lo, m_hi - m_lo + 1, q


def quant_lattice(dist, args):
    """(m_lo, V, q, edges [V + 1]) of a joinable quantised label: the edges in
    the fit coordinate, e_0 = low, e_V = high, e_i = (m_lo + i - 1/2) q between
    (its log for qloguniform); strictly increasing."""
    m_lo, V, q = lattice_size(dist, args)
    inner = (m_lo + np.arange(1, V) - 0.5) * q
    if dist == 'qloguniform':
        inner = np.log(inner)
    edges = np.concatenate([[float(args['low'])], inner, [float(args['high'])]])
    assert (np.diff(edges) > 0).all(), (dist, args)
    return m_lo, V, q, edges


def quant_reason(row, table, conditional=False):
    """Why ``row`` cannot be joined as a quantised dimension, or None if it can
    (``conditional``: as in discrete_reason)."""
    if not conditional and (not all(p is None for p in row.parents) or row.depth != 0):
        return 'conditional (%s)' % row.dist
    if row.dist in ('qnormal', 'qlognormal'):
        return ('%s: its lattice is unbounded and data-dependent, so eligibility could not be decided before the fit'
                % row.dist)
    if row.dist not in QUANT_DISTS:
        return 'not a quniform or qloguniform label (%s)' % row.dist
    if not float(row.args['q']) > 0:
        return 'q = %r is not positive' % (row.args['q'],)
    if not float(row.args['high']) > float(row.args['low']):
        return 'an empty range'
    V = lattice_size(row.dist, row.args)[1]
    if V < 2:
        return '%d lattice value, fewer than 2: nothing to choose' % V
    if V > N.JOINT_MAX_LATTICE:
        return ('%d lattice values, more than TPE_JOINT_MAX_LATTICE = %d: such a label is close to continuous, model '
                'it as uniform / loguniform' % (V, N.JOINT_MAX_LATTICE))
    return None


def eligible_quant(row, table):
    """Whether a ParamRow can be joined as a quantised dimension: unconditional
    quniform / qloguniform, q > 0, 2 to 256 lattice values."""
    return quant_reason(row, table) is None


def quant_bin_masses(mu, sigma, edges):
    """(diff [K, V], mass [K]) of one quantised dimension: the components' float64
    normal masses on the bins [e_i, e_{i+1}) and on [e_0, e_V), every Phi
    difference between the two smaller tails (_std_bounds' mirroring, per bin):
    lower tails left of mu, upper tails right of it, 1 - upper - lower for the
    bin that holds mu.  A tail beyond QUANT_TAIL_MAX is exactly 0 (float64 would
    go subnormal there: the rule keeps the result independent of the libm), so a
    far bin's mass is exactly 0."""
    mu, sigma = np.asarray(mu, dtype=np.float64)[:, None], np.asarray(sigma, dtype=np.float64)[:, None]
    t = (np.asarray(edges, dtype=np.float64)[None, :] - mu) * (SQRT1_2 / sigma)
    s = np.where(np.abs(t) > QUANT_TAIL_MAX, 0.0, 0.5 * erfc(np.abs(t)))

    def mass(ta, sa, tb, sb):
        return np.where(tb <= 0, sb - sa, np.where(ta >= 0, sa - sb, 1.0 - sa - sb))
    return mass(t[:, :-1], s[:, :-1], t[:, 1:], s[:, 1:]), mass(t[:, 0], s[:, 0], t[:, -1], s[:, -1])


def quant_P(mu, sigma, edges):
    """P_kd(i) [K, V]: every row sums to 1."""
    diff, mass = quant_bin_masses(mu, sigma, edges)
    return diff / mass[:, None]


def quant_table(mu, sigma, edges):
    """float64 T [K, V] = log2 P_kd(i) as the device stores it: entries below
    TPE_JOINT_QFLOOR (-inf included) are TPE_JOINT_QFLOOR."""
    diff, mass = quant_bin_masses(mu, sigma, edges)
    with np.errstate(divide='ignore'):
        T = np.log2(diff) - np.log2(mass)[:, None]
    return np.where(T >= N.JOINT_QFLOOR, T, N.JOINT_QFLOOR)


def quant_lpdf_numpy(z, v, qi, w, mu, sigma, low, high, xc, ps, s, quants, block=1 << 14):
    """The quantised model's float64 log-density at continuous ``z`` [C, Dc],
    categories ``v`` [C, Dk] and lattice indices ``qi`` [C, Dq]: ``quants`` one
    (mu [K], sigma [K], edges [V + 1]) per quantised dimension of this side.
    log p = logsumexp_k [log w_k + the continuous terms + sum_d log P_kd(v_d) +
    sum_d log P_kd(i_d)]; a quantised dimension adds nothing to the coefficient."""
    qi = np.asarray(qi, dtype=np.int64)
    C = len(qi)
    v = np.asarray(v, dtype=np.int64).reshape(C, len(ps))
    z = np.asarray(z, dtype=np.float64).reshape(C, np.asarray(mu).shape[1])
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low, dtype=np.float64)[None, :],
                            np.asarray(high, dtype=np.float64)[None, :])
    logc = np.log(w) - np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)
    with np.errstate(divide='ignore'):
        logP = [np.log(quant_P(qm, qs, e)) for qm, qs, e in quants]              # [K, V] each
    out = np.empty(C)
    step = max(1, block // max(1, len(w) // 64 + 1))
    for lo in range(0, C, step):
        zz, vv, qq = z[lo:lo + step], v[lo:lo + step], qi[lo:lo + step]
        t = logc[None, :].repeat(len(qq), axis=0)
        for d in range(z.shape[1]):
            t -= 0.5 * ((zz[:, d, None] - mu[None, :, d]) / sigma[None, :, d]) ** 2
        for d, p in enumerate(ps):
            p = np.asarray(p, dtype=np.float64)
            pv = p[vv[:, d]][:, None]
            hit = vv[:, d, None] == xc[None, :, d]
            t += np.log(np.where(xc[None, :, d] < 0, pv, (hit + s[d] * pv) / (1.0 + s[d])))
        for d in range(len(quants)):
            t += logP[d][:, qq[:, d]].T
        m = t.max(axis=1)
        out[lo:lo + step] = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
    return out


class QuantModel(object):
    """The two mixtures of a joint group with quantised labels: ``rows`` the
    continuous ParamRows, ``drows`` the discrete and ``qrows`` the quantised
    ones (kernel coordinate order: rows, drows, qrows); ``below`` / ``above`` =
    (w, mu, sigma, xc, qmu, qsigma) with qmu / qsigma [K, Dq] the quantised
    dimensions' components; ``lattices`` one quant_lattice per quantised label."""
    __slots__ = ('rows', 'drows', 'qrows', 'below', 'above', 'low', 'high', 'ps', 's_below', 's_above', 'lattices')

    def __init__(self, rows, drows, qrows, below, above, low, high, ps, s_below, s_above, lattices):
        self.rows, self.drows, self.qrows, self.below, self.above = list(rows), list(drows), list(qrows), below, above
        self.low, self.high, self.ps, self.s_below, self.s_above = low, high, ps, s_below, s_above
        self.lattices = lattices

    def cats(self):
        """The ``cats`` argument of Engine.run_joint_quant."""
        return [(self.below[3][:, d], self.above[3][:, d], self.ps[d], self.s_below[d], self.s_above[d])
                for d in range(len(self.drows))]

    def quants(self):
        """The ``quants`` argument of Engine.run_joint_quant."""
        return [(self.below[4][:, d], self.below[5][:, d], self.above[4][:, d], self.above[5][:, d], lat[3])
                for d, lat in enumerate(self.lattices)]

    def centres(self):
        """The ``centres`` argument of Engine.run_joint_quant with ``liar``:
        per quantised label the fit coordinates of its lattice values."""
        return [quant_centres(r.dist, r.args) for r in self.qrows]

    def values(self, z):
        """Label values of kernel coordinates z [.., Dc + Dk + Dq]: exp for the
        log families, (m_lo + i) q for a lattice index i."""
        z = np.array(z, dtype=np.float64)
        for d, r in enumerate(self.rows):
            if r.dist in LOG_DISTS:
                z[..., d] = np.exp(z[..., d])
        o = len(self.rows) + len(self.drows)
        for d, (m_lo, V, q, _) in enumerate(self.lattices):
            z[..., o + d] = (m_lo + np.rint(z[..., o + d])) * q
        return z


def fit_quant_model(rows, drows, qrows, hist, below_tids, prior_weight=1.0, lf=DEFAULT_LF):
    """QuantModel of the eligible continuous ``rows``, discrete ``drows`` and
    quantised ``qrows`` from a History and its below set (fit_mixed_model with
    the quantised columns fitted as continuous ones in their fit coordinate)."""
    crow = list(rows) + list(qrows)
    pb = [prior_and_bounds('uniform' if r.dist in QUANT_DISTS else r.dist, r.args) for r in crow]
    tids = None
    cols, ccols = [], []
    every = crow + list(drows)
    for r in every:
        otids, ovals = hist.obs[r.label]
        otids = np.asarray(otids, dtype=np.int64)
        if tids is None:
            tids = otids
        elif len(otids) != len(tids) or (otids != tids).any():
            raise ValueError('joint label %r is not observed in the same trials as %r' % (r.label, every[0].label))
        if r.dist in DISCRETE_DISTS:
            ovals = np.asarray(ovals, dtype=np.int64)
            if len(ovals) and (ovals.min() < 0 or ovals.max() >= int(r.args['upper'])):
                raise IndexError('categorical observation of %r out of range [0, %d)' % (r.label, int(r.args['upper'])))
            ccols.append(ovals)
        else:
            cols.append(fit_coord(r.dist, r.args, ovals))
    n, Dc = len(tids), len(rows)
    X = np.stack(cols, axis=1) if cols else np.zeros((n, 0))
    XC = np.stack(ccols, axis=1) if ccols else np.zeros((n, 0), dtype=np.int64)
    order = np.argsort(tids, kind='stable')
    X, XC, tids = X[order], XC[order], tids[order]
    m = np.isin(tids, np.asarray(below_tids, dtype=np.int64))
    priors = [(p[0], p[1]) for p in pb]
    ps = [cat_prior(r.dist, r.args) for r in drows]
    nb, na = int(m.sum()), int((~m).sum())
    sides = []
    for sel in (m, ~m):
        w, mu, sigma, xc = mixed_side_mixture(X[sel], priors, XC[sel], prior_weight, lf)
        sides.append((w, mu[:, :Dc], sigma[:, :Dc], xc, mu[:, Dc:], sigma[:, Dc:]))
    return QuantModel(rows, drows, qrows, sides[0], sides[1],
                      np.array([p[2] for p in pb[:Dc]], dtype=np.float64),
                      np.array([p[3] for p in pb[:Dc]], dtype=np.float64),
                      ps, np.array([smoothing(prior_weight, len(p), nb) for p in ps]),
                      np.array([smoothing(prior_weight, len(p), na) for p in ps]),
                      [quant_lattice(r.dist, r.args) for r in qrows])


# ------------------------------------------------------- sharded joint stage
def empty_records(P, dtype=N.JOINT_RECORD_DTYPE):
    """[P] records of a part that holds no candidate: global_idx -1, the rest 0
    (what the merge kernels write for a problem without a winner)."""
    rec = np.zeros(int(P), dtype=dtype)
    rec['global_idx'] = -1
    return rec


def combine_records(stacked):
    """[world, P] winner records (N.JOINT_RECORD_DTYPE or
    N.JOINT_WIDE_RECORD_DTYPE) of the parts of a candidate-sharded joint stage
    -> [P]: per problem the record the unsharded stage returns.  The order is
    the device's (np.argmax over the float64 score l - g in candidate index
    order): a NaN score beats every number, then the larger score wins, then
    the lower global_idx; -0.0 ties with +0.0.  A record with global_idx < 0 is
    empty and never wins against one that is not."""
    stacked = np.asarray(stacked)
    if stacked.ndim == 1:
        return stacked.copy()
    out = stacked[0].copy()
    for r in range(1, stacked.shape[0]):
        new = stacked[r]
        with np.errstate(invalid='ignore'):
            s_out, s_new = out['l'] - out['g'], new['l'] - new['g']
            out_nan, new_nan = np.isnan(s_out), np.isnan(s_new)
            lower = new['global_idx'] < out['global_idx']
            better = (new_nan & (~out_nan | lower)) | \
                     (~new_nan & ~out_nan & ((s_new > s_out) | ((s_new == s_out) & lower)))
        out_empty, new_empty = out['global_idx'] < 0, new['global_idx'] < 0
        better = (better | out_empty) & ~new_empty
        out[better] = new[better]
    return out


# ------------------------------------------------- batch-aware joint suggests
# The ids of one batched call pick greedily (include/tpe_hip.h "Batch-aware
# joint suggests", DESIGN.md "Batch-aware joint suggests"; continuous groups:
# the block after this one takes discrete and quantised labels).  The above
# side is side_mixture's: n trial rows and the prior row,
# un-normalised weights w~ (prior_weight, then the linear-forgetting ramp or 1),
# W their sum.  Id j (step j, the order given) is scored under the above
# mixture extended by J = G + j "liars": the G given vectors, then the picks of
# the ids before it.  Liar i (its ordinal among all liars):
#   weight  1 un-normalised (the newest trial), so the weights are (w~, 1, .., 1) / (W + J)
#   mean    z, the f32 coordinates of the pick or given vector
#   sigma_d the adaptive-Parzen neighbour rule over P_d = the side's K f32 mu
#           values of dimension d and the z_d of the liars before it: with L =
#           max{p <= z_d} and U = min{p > z_d}, max(z_d - L, U - z_d) (a missing
#           side dropped), clipped to [psig_d / min(100, m + 2), psig_d], m = n +
#           i + 1; float64 on f32 values.
#   log g_j(z) = logaddexp(log g(z), logsumexp_i log k_i(z) - log W) - log1p(J / W)
#   log k_i(z) = -sum_d [log(sigma_id sqrt(2 pi) mass_id) + ((z_d - mu_id) / sigma_id)^2 / 2]
# l is unchanged, score_j = l - g_j, the winner in np.argmax order.  Deviation
# from B sequential asks: the existing components are not refitted (their
# bandwidths, the below / above split and the forgetting ramp stay).
def side_weight_sum(n, prior_weight=1.0, lf=DEFAULT_LF):
    """W: the sum of the un-normalised weights side_mixture gives n trials."""
    w = linear_forgetting_weights(n, lf) if (lf and lf < n) else np.ones(n)
    return float(prior_weight) + float(np.sum(w))


def liar_sigmas(points, z, psig, m):
    """sigma [D] of a liar at the f32 vector ``z``: ``points`` [P, D] f32 the
    side's mu rows followed by the earlier liars, m = n + i + 1."""
    pts = np.asarray(points, dtype=np.float32).astype(np.float64)
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    psig = np.asarray(psig, dtype=np.float64)
    out = np.empty(len(z))
    for d in range(len(z)):
        col = pts[:, d]
        le, gt = col[col <= z[d]], col[col > z[d]]
        gaps = ([z[d] - le.max()] if len(le) else []) + ([gt.min() - z[d]] if len(gt) else [])
        out[d] = max(gaps) if gaps else 0.0
    return np.minimum(np.maximum(out, psig / min(100.0, m + 2.0)), psig)


def liar_log_g(z, log_g, liar_mu, liar_sigma, W, low, high):
    """log g_J at ``z`` [C, D] from the base ``log_g`` [C] and J liars (mu,
    sigma [J, D]); J = 0: log_g."""
    J = len(liar_mu)
    if J == 0:
        return np.array(log_g, dtype=np.float64)
    lk = lpdf_numpy(z, np.ones(J), np.asarray(liar_mu, dtype=np.float64), np.asarray(liar_sigma, dtype=np.float64),
                    low, high)
    return np.logaddexp(log_g, lk - math.log(W)) - math.log1p(J / W)


# ------------------------- batch-aware picks over discrete and quantised labels
# The liar model above for a root group that also holds discrete and / or
# quantised labels (include/tpe_hip.h and DESIGN.md "Batch-aware picks over
# discrete and quantised labels").  A row is [z (f32) | category index | lattice
# index] in kernel order; steps, ordering, W and m = n + i + 1 are unchanged, as
# are the below side, l and the existing components (their smoothing masses
# included).  Liar i from a row r, un-normalised weight 1:
#   continuous d   the rule above, over above_mu[:, d] (f32) and the earlier liars
#   discrete d     the category x = r[Dc + d] and the factor of a trial component
#                  of the above side as the stage holds it, P(v) = (1[v = x] +
#                  s_d p_d(v)) / (1 + s_d) with s_d = s_above[d] unchanged (one
#                  more trial would make it prior_weight U / (n + 2)); float64
#                  tables from discrete_tables; no bandwidth
#   quantised d    centre: the fit coordinate of the picked lattice value,
#                  fit_coord(dist, args, (m_lo + i) q), what a trial that observed
#                  it gets as qmu (quant_centres, one table per call).  Bandwidth:
#                  the neighbour rule over the K values above_qmu[:, d] (float64,
#                  the prior row included) and the earlier liars' centres,
#                  clipped to [psig_d / min(100, m + 2), psig_d], psig_d =
#                  above_qsigma[0, d].  Factor: quant_P(centre, sigma, edges_d),
#                  not floored: a far bin's log is -inf.
#   log k_i(z, v, q) = the continuous term + sum_d log P_id(v_d) + sum_d log Q_id(q_d)
# and log g_j as above; where every liar's term is -inf, g_j = log g - log1p(J / W).
LN2 = math.log(2.0)


def quant_centres(dist, args):
    """float64 [V]: the fit coordinate of every lattice value of a joinable
    quantised label, (m_lo + i) q through parzen.fit_coord."""
    m_lo, V, q = lattice_size(dist, args)
    return np.ascontiguousarray(fit_coord(dist, args, (m_lo + np.arange(V)) * q), dtype=np.float64)


def liar_cat_tables(p, s):
    """float64 (miss [U], bonus [U]) of a liar's discrete factor in natural
    logarithms: log P(v) = miss[v] + bonus[v] 1[v = x]; discrete_tables' values."""
    miss, bonus, _ = discrete_tables(p, s)
    return miss * LN2, bonus * LN2


def liar_quant_sigmas(points, c, psig, m):
    """sigma [Dq] of a liar's quantised dimensions at the centres ``c``:
    ``points`` [P, Dq] float64 the side's qmu rows followed by the earlier
    liars' centres, m = n + i + 1.  Float64 subtractions, one division, max /
    min: bit for bit what the device computes."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    pts = np.asarray(points, dtype=np.float64)
    pts = pts.reshape(len(pts), len(c))
    psig = np.asarray(psig, dtype=np.float64)
    out = np.empty(len(c))
    for d in range(len(c)):
        col = pts[:, d]
        le, gt = col[col <= c[d]], col[col > c[d]]
        gaps = ([c[d] - le.max()] if len(le) else []) + ([gt.min() - c[d]] if len(gt) else [])
        out[d] = max(gaps) if gaps else 0.0
    return np.minimum(np.maximum(out, psig / min(100.0, m + 2.0)), psig)


def liar_mixed_log_g(z, v, qi, log_g, liars, W, low, high, cat_tabs=(), edges=()):
    """log g_J at continuous ``z`` [C, Dc], categories ``v`` [C, Dk] and lattice
    indices ``qi`` [C, Dq] from the base ``log_g`` [C]: ``liars`` = (mu [J, Dc],
    sigma [J, Dc], cat [J, Dk], centre [J, Dq], qsigma [J, Dq]), ``cat_tabs`` one
    liar_cat_tables per discrete dimension, ``edges`` one array per quantised
    one.  J = 0: log_g."""
    mu, sigma, cat, qc, qs = liars
    J = len(cat)
    if J == 0:
        return np.array(log_g, dtype=np.float64)
    C = len(log_g)
    mu, sigma = np.asarray(mu, dtype=np.float64).reshape(J, -1), np.asarray(sigma, dtype=np.float64).reshape(J, -1)
    Dc = mu.shape[1]
    z = np.asarray(z, dtype=np.float64).reshape(C, Dc)
    v = np.asarray(v, dtype=np.int64).reshape(C, len(cat_tabs))
    qi = np.asarray(qi, dtype=np.int64).reshape(C, len(edges))
    cat = np.asarray(cat, dtype=np.int64).reshape(J, len(cat_tabs))
    t = np.zeros((C, J))
    if Dc:
        fa, fb, _ = _std_bounds(mu, sigma, np.asarray(low, dtype=np.float64)[None, :],
                                np.asarray(high, dtype=np.float64)[None, :])
        t -= np.sum(np.log(sigma * np.sqrt(2 * np.pi)) + np.log(fb - fa), axis=1)[None, :]
        for d in range(Dc):
            t -= 0.5 * ((z[:, d, None] - mu[None, :, d]) / sigma[None, :, d]) ** 2
    for d, (miss, bonus) in enumerate(cat_tabs):
        t += miss[v[:, d]][:, None] + np.where(v[:, d, None] == cat[None, :, d], bonus[v[:, d]][:, None], 0.0)
    for d, e in enumerate(edges):
        with np.errstate(divide='ignore'):
            logQ = np.log(quant_P(np.asarray(qc, dtype=np.float64).reshape(J, -1)[:, d],
                                  np.asarray(qs, dtype=np.float64).reshape(J, -1)[:, d], e))
        t += logQ[:, qi[:, d]].T
    m = t.max(axis=1)
    m = np.where(np.isfinite(m), m, 0.0)                 # every term -inf: the sum is 0, its log -inf, no NaN
    with np.errstate(divide='ignore'):
        lk = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
    return np.logaddexp(log_g, lk - math.log(W)) - math.log1p(J / W)
