"""The joint TPE model with quantised labels (DESIGN.md "Quantised labels in the
joint stage") restated in plain numpy, on top of tests/joint_ref.py and
tests/joint_mixed_ref.py: nothing here calls hyperopt_amd.joint or the native
library.

A quantised label is a continuous dimension observed through bins: lattice
index i stands for the value (m_lo + i) q and takes the component's normal mass
on [e_i, e_{i+1}) over its mass on [low, high)."""
import math

import numpy as np
from scipy.special import logsumexp, ndtr

from tests import joint_mixed_ref as M
from tests import joint_ref as R

QFLOOR = -4096.0
TAIL_MAX = 26.5 * math.sqrt(2.0)        # standardised distance beyond which a tail (below 2^-1018) counts as 0

# (dist, low, high, q) -> (m_lo, V): the lattices the rule was worked out on
LATTICE_CASES = [
    (('quniform', 0.0, 10.0, 1.0), (0, 11)),
    (('quniform', 1.0, 8.0, 1.0), (1, 8)),
    (('quniform', 0.0, 3.5, 1.0), (0, 4)),           # 4 would have the empty bin [3.5, 3.5)
    (('quniform', 0.5, 2.5, 1.0), (1, 2)),           # 0 ([-0.5, 0.5)) and 3 ([2.5, 3.5)) clip to nothing
    (('quniform', -5.0, 5.0, 2.5), (-2, 5)),
    (('quniform', 16.0, 512.0, 16.0), (1, 32)),
    (('quniform', 0.0, 256.0, 1.0), (0, 257)),
    (('qloguniform', math.log(16.0), math.log(512.0), 16.0), (1, 32)),
    (('qloguniform', math.log(1e-3), math.log(10.0), 1.0), (0, 11)),     # the value 0 is in the lattice
]


def ref_lattice(dist, low, high, q):
    """(m_lo, V, edges [V + 1]) by a linear search from the definition: m_lo the
    smallest integer m with (m + 1/2) q > lo_v (not below 0 for qloguniform),
    m_hi the largest with (m - 1/2) q < hi_v; e_0 = low, e_V = high, e_i =
    (m_lo + i - 1/2) q (its log for qloguniform).  Asserts that the edges are
    strictly increasing, so that the bins [e_i, e_{i+1}) tile [low, high)."""
    log = dist == 'qloguniform'
    lo_v, hi_v = (math.exp(low), math.exp(high)) if log else (low, high)
    m = int(math.floor(lo_v / q)) - 2
    while not (m + 0.5) * q > lo_v:
        m += 1
    m_lo = max(m, 0) if log else m
    m = int(math.ceil(hi_v / q)) + 2
    while not (m - 0.5) * q < hi_v:
        m -= 1
    V = m - m_lo + 1
    inner = np.array([(m_lo + i - 0.5) * q for i in range(1, V)])
    edges = np.concatenate([[low], np.log(inner) if log else inner, [high]])
    assert V >= 1 and len(edges) == V + 1
    assert (np.diff(edges) > 0).all(), (dist, low, high, q, edges)
    return m_lo, V, edges


def ref_binP(mu, sigma, edges):
    """P_kd(i) [K, V] of one quantised dimension: Phi differences between the two
    smaller tails (lower tails for a bin left of mu, upper tails right of it,
    1 - upper - lower for the bin that holds mu), over the mass on [e_0, e_V).
    A tail more than TAIL_MAX standard deviations out is exactly 0 (the model's
    underflow rule: float64 would be subnormal there)."""
    mu, sigma = np.asarray(mu, dtype=float)[:, None], np.asarray(sigma, dtype=float)[:, None]
    t = (np.asarray(edges, dtype=float)[None, :] - mu) / sigma
    s = np.where(np.abs(t) > TAIL_MAX, 0.0, ndtr(-np.abs(t)))          # the smaller tail of every edge

    def mass(a, sa, b, sb):
        return np.where(b <= 0, sb - sa, np.where(a >= 0, sa - sb, 1.0 - sb - sa))
    return mass(t[:, :-1], s[:, :-1], t[:, 1:], s[:, 1:]) / mass(t[:, 0], s[:, 0], t[:, -1], s[:, -1])[:, None]


def ref_table(mu, sigma, edges):
    """log2 P_kd(i) [K, V] with everything below the floor (-inf included) at the floor."""
    with np.errstate(divide='ignore'):
        T = np.log2(ref_binP(mu, sigma, edges))
    return np.where(T >= QFLOOR, T, QFLOOR), T


def ref_quant_lpdf(z, v, qi, side, low, high, ps, s, edges, block=2048):
    """float64 log p(z, v, i) = logsumexp_k [log w_k + the continuous terms +
    sum_d log P_kd(v_d) + sum_d log P_kd(i_d)] at z [C, Dc], v [C, Dk], qi
    [C, Dq]; ``side`` = (w, mu, sigma, xc, qmu, qsigma), ``edges`` one array per
    quantised dimension.  A quantised dimension adds nothing to the coefficient."""
    w, mu, sigma, xc, qmu, qsig = side
    qi = np.asarray(qi, dtype=np.int64)
    C = len(qi)
    v = np.asarray(v, dtype=np.int64).reshape(C, len(ps))
    z = np.asarray(z, dtype=np.float64).reshape(C, mu.shape[1])
    lc = R.ref_logcoef(w, mu, sigma, low, high) if mu.shape[1] else np.log(w)
    logP = [np.log(M.ref_P(xc[:, d], ps[d], s[d])) for d in range(len(ps))]
    with np.errstate(divide='ignore'):
        logQ = [np.log(ref_binP(qmu[:, d], qsig[:, d], e)) for d, e in enumerate(edges)]
    out = np.empty(C)
    for lo in range(0, C, block):
        zz, vv, qq = z[lo:lo + block], v[lo:lo + block], qi[lo:lo + block]
        t = lc[None, :] - 0.5 * (((zz[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2).sum(axis=2)
        for d in range(len(ps)):
            t = t + logP[d][:, vv[:, d]].T
        for d in range(len(edges)):
            t = t + logQ[d][:, qq[:, d]].T
        out[lo:lo + block] = logsumexp(t, axis=1)
    return out


def marginal(side, d, edges):
    """sum_k w_k P_kd(i) [V]: the sampler's marginal of quantised dimension d."""
    return (side[0][:, None] * ref_binP(side[4][:, d], side[5][:, d], edges)).sum(axis=0)


def lattice_of(V):
    """The test lattice of V values: quniform(0, V - 1, 1), edges 0, 0.5, .., V - 1.5, V - 1."""
    m_lo, V2, edges = ref_lattice('quniform', 0.0, float(V - 1), 1.0)
    assert (m_lo, V2) == (0, V)
    return edges


def seeded_quant_case(Dc, us, Vs, n, seed=None):
    """joint_mixed_ref.seeded_mixed_case's recipe for the continuous and discrete
    parts, then the trials' lattice values of every quantised dimension
    (lattice_of(V), drawn as quniform draws them: a uniform draw, rounded); the
    loss draw and the split follow.
    Returns (below, above, low, high, ps, s_below, s_above, edges, rs), the
    sides as (w, mu, sigma, xc, qmu, qsigma)."""
    Dk, Dq = len(us), len(Vs)
    rs = np.random.RandomState(100000 * Dq + 1000 * Dc + 10 * Dk + n if seed is None else seed)
    bounded = np.arange(Dc) % 2 == 0
    low = np.where(bounded, -10.0, -np.inf)
    high = np.where(bounded, 10.0, np.inf)
    pmu = np.where(bounded, 0.0, 1.0)
    psig = np.where(bounded, 20.0, 4.0)
    X = np.where(bounded[None, :], rs.uniform(-10, 10, (n, Dc)), rs.normal(1.0, 4.0, (n, Dc)))
    ps = [M.prior(u) for u in us]
    XC = np.stack([rs.choice(len(p), size=n, p=p) for p in ps], axis=1) if ps else np.zeros((n, 0), dtype=np.int64)
    edges = [lattice_of(V) for V in Vs]
    XQ = np.stack([np.rint(rs.uniform(0.0, V - 1.0, n)) for V in Vs], axis=1)
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    loss = rs.uniform(size=n)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    qpmu = np.array([0.5 * (V - 1.0) for V in Vs])
    qpsig = np.array([V - 1.0 for V in Vs])
    sides = []
    for sel in (m, ~m):
        w, mu, sigma, xc = M.ref_mixed_side(X[sel], pmu, psig, XC[sel])
        _, qmu, qsig = R.ref_side(XQ[sel], qpmu, qpsig)
        sides.append((w, mu, sigma, xc, qmu, qsig))
    s_below = np.array([M.smoothing(len(p), int(m.sum())) for p in ps])
    s_above = np.array([M.smoothing(len(p), int((~m).sum())) for p in ps])
    return sides[0], sides[1], low, high, ps, s_below, s_above, edges, rs


def quants_of(below, above, edges):
    """The ``quants`` argument of Engine.run_joint_quant."""
    return [(below[4][:, d], below[5][:, d], above[4][:, d], above[5][:, d], e) for d, e in enumerate(edges)]


def lattice_components(case, n, seed=0, extra=()):
    """(mu [n + 1 + len(extra)], sigma) of the prior row and n observations of a
    LATTICE_CASES-style case (dist, low, high, q) in its fit coordinate, the
    values drawn as the label draws them (a uniform draw in the fit coordinate,
    rounded to the lattice) and ``extra`` values appended."""
    dist, low, high, q = case
    rs = np.random.RandomState(seed)
    u = rs.uniform(low, high, n)
    vals = np.concatenate([np.rint((np.exp(u) if dist == 'qloguniform' else u) / q) * q, np.asarray(extra, dtype=float)])
    x = np.log(np.maximum(vals, max(1e-12, math.exp(low)))) if dist == 'qloguniform' else vals
    _, mu, sigma = R.ref_side(x[:, None], np.array([0.5 * (low + high)]), np.array([high - low]))
    return mu[:, 0], sigma[:, 0]
