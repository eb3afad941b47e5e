"""The mixed joint TPE model (continuous and discrete labels in one group,
DESIGN.md "Joint TPE") restated in plain numpy, on top of tests/joint_ref.py:
nothing here calls hyperopt_amd.joint or the native library."""
import numpy as np
from scipy.special import logsumexp

from tests import joint_ref as R

PCHOICE = np.array([0.5, 0.2, 0.15, 0.1, 0.05])          # the one non-uniform prior of the tests ("5p")


def prior(u):
    """p_d of a category spec: an int U is the uniform prior of an hp.choice,
    '5p' the hp.pchoice prior above."""
    return PCHOICE.copy() if u == '5p' else np.full(int(u), 1.0 / int(u))


def smoothing(U, n, prior_weight=1.0):
    """s_d = prior_weight U_d / (n + 1) of a side with n trials."""
    return prior_weight * U / (n + 1.0)


def ref_P(xc, p, s):
    """P_kd(v) [K, U] of one dimension: row k the prior p where xc[k] = -1 (row
    0), else (1[v = xc[k]] + s p(v)) / (1 + s)."""
    xc = np.asarray(xc)
    p = np.asarray(p, dtype=float)
    hit = (np.arange(len(p))[None, :] == xc[:, None]).astype(float)
    return np.where(xc[:, None] < 0, p[None, :], (hit + s * p[None, :]) / (1.0 + s))


def ref_mixed_side(X, pmu, psig, XC, prior_weight=1.0):
    """(w, mu, sigma, xc): joint_ref.ref_side over the continuous columns X
    [n, Dc] and xc [n + 1, Dk] the components' categories, row 0 (prior) -1."""
    XC = np.asarray(XC, dtype=np.int64)
    if XC.ndim == 1:
        XC = XC[:, None]
    n = len(XC)
    Dc = len(pmu)
    if Dc:
        w, mu, sigma = R.ref_side(np.asarray(X, dtype=float).reshape(n, Dc), pmu, psig, prior_weight)
    else:                                             # an all-discrete group: ref_side's weights alone
        w = np.ones(n + 1)
        w[0] = prior_weight
        if n > R.LF:
            w[1:] = np.concatenate([np.linspace(1.0 / n, 1.0, num=n - R.LF), np.ones(R.LF)])
        w = w / w.sum()
        mu = sigma = np.zeros((n + 1, 0))
    return w, mu, sigma, np.vstack([np.full((1, XC.shape[1]), -1, dtype=np.int64), XC])


def ref_mixed_lpdf(z, v, side, low, high, ps, s, block=2048):
    """float64 log p(z, v) = logsumexp_k [log w_k + the continuous terms +
    sum_d log P_kd(v_d)] at z [C, Dc], v [C, Dk]."""
    w, mu, sigma, xc = side
    v = np.asarray(v, dtype=np.int64)
    C = len(v)
    z = np.asarray(z, dtype=np.float64).reshape(C, mu.shape[1])
    lc = R.ref_logcoef(w, mu, sigma, low, high) if mu.shape[1] else np.log(w)
    logP = [np.log(ref_P(xc[:, d], ps[d], s[d])) for d in range(len(ps))]        # [K, U] each
    out = np.empty(C)
    for lo in range(0, C, block):
        zz, vv = z[lo:lo + block], v[lo:lo + block]
        t = lc[None, :] - 0.5 * (((zz[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2).sum(axis=2)
        for d in range(len(ps)):
            t = t + logP[d][:, vv[:, d]].T
        out[lo:lo + block] = logsumexp(t, axis=1)
    return out


def marginal(side, d, p, s):
    """sum_k w_k P_kd(v) [U]: the sampler's marginal of discrete dimension d."""
    return (side[0][:, None] * ref_P(side[3][:, d], p, s)).sum(axis=0)


def seeded_mixed_case(Dc, us, n, seed=None):
    """joint_ref.seeded_case's recipe for the continuous part (the same
    RandomState draws in the same order), the trials' categories drawn from the
    priors after X; the loss draw and the split follow.  Returns (below, above,
    low, high, pmu, psig, ps, s_below, s_above, rs)."""
    Dk = len(us)
    rs = np.random.RandomState(1000 * Dc + 10 * Dk + n if seed is None else seed)
    bounded = np.arange(Dc) % 2 == 0
    low = np.where(bounded, -10.0, -np.inf)
    high = np.where(bounded, 10.0, np.inf)
    pmu = np.where(bounded, 0.0, 1.0)
    psig = np.where(bounded, 20.0, 4.0)
    X = np.where(bounded[None, :], rs.uniform(-10, 10, (n, Dc)), rs.normal(1.0, 4.0, (n, Dc)))
    ps = [prior(u) for u in us]
    XC = np.stack([rs.choice(len(p), size=n, p=p) for p in ps], axis=1)
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    loss = rs.uniform(size=n)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    below = ref_mixed_side(X[m], pmu, psig, XC[m])
    above = ref_mixed_side(X[~m], pmu, psig, XC[~m])
    s_below = np.array([smoothing(len(p), int(m.sum())) for p in ps])
    s_above = np.array([smoothing(len(p), int((~m).sum())) for p in ps])
    return below, above, low, high, pmu, psig, ps, s_below, s_above, rs


def cats_of(below, above, ps, s_below, s_above):
    """The ``cats`` argument of Engine.run_joint_mixed."""
    return [(below[3][:, d], above[3][:, d], ps[d], s_below[d], s_above[d]) for d in range(len(ps))]
