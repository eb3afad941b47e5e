"""Batch-aware picks over discrete and quantised labels restated in plain numpy
(DESIGN.md "Batch-aware picks over discrete and quantised labels"), on top of
tests/joint_liar_ref.py, tests/joint_mixed_ref.py and tests/joint_quant_ref.py:
nothing here calls hyperopt_amd.

A row is [z (f32, Dc) | category index (Dk) | lattice index (Dq)].  A side is
the 6-tuple (w, mu, sigma, xc, qmu, qsigma) of joint_quant_ref (a group without
quantised labels carries qmu = qsigma = [K, 0]).  Liar i, un-normalised weight 1:
  continuous d  joint_liar_ref's rule over the side's f32 mu and the earlier liars
  discrete d    the category x of the row; P(v) = (1[v = x] + s_d p_d(v)) / (1 + s_d)
                with the above side's s_d unchanged
  quantised d   centre c = centres[d][lattice index]; sigma by the neighbour rule
                over the K values qmu[:, d] (float64) and the earlier centres,
                clipped to [psig_d / min(100, m + 2), psig_d], psig_d = qsigma[0, d];
                Q(v) = the normal (c, sigma) on bin v over its mass on the lattice
                (joint_quant_ref.ref_binP, not floored)
  log g_j = logaddexp(log g, logsumexp_i log k_i - log W) - log1p(J / W)
"""
import numpy as np
from scipy.special import logsumexp

from tests import joint_liar_ref as LR
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R


def quant_sigma(points, c, psig, m):
    """sigma [Dq] (float64) of a liar's quantised dimensions at the centres c:
    points [P, Dq] float64."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    pts = np.asarray(points, dtype=np.float64)
    pts = pts.reshape(len(pts), len(c))
    out = np.zeros(len(c))
    for d in range(len(c)):
        col = pts[:, d]
        gaps = []
        if (col <= c[d]).any():
            gaps.append(c[d] - col[col <= c[d]].max())
        if (col > c[d]).any():
            gaps.append(col[col > c[d]].min() - c[d])
        out[d] = max(gaps) if gaps else 0.0
    psig = np.asarray(psig, dtype=np.float64)
    return np.clip(out, psig / min(100.0, m + 2.0), psig)


def centres_of(Vs):
    """The centres of joint_quant_ref.lattice_of(V): quniform(0, V - 1, 1), whose
    fit coordinate is the value itself."""
    return [np.arange(V, dtype=np.float64) for V in Vs]


class MixedChain(object):
    """The liars of one greedy batch over the above side ``above`` (6-tuple):
    ``add`` a row, ``log_g`` the extended density from the base one."""

    def __init__(self, above, psig, low, high, ps, s_above, edges, centres, W=None, given=None):
        self.points = np.asarray(above[1], dtype=np.float32)           # the continuous rows as the device holds them
        self.qpoints = np.asarray(above[4], dtype=np.float64)
        self.n = len(above[0]) - 1
        self.W = LR.weight_sum(self.n) if W is None else float(W)
        self.psig, self.low, self.high = np.asarray(psig, dtype=np.float64), np.asarray(low), np.asarray(high)
        self.qpsig = np.asarray(above[5], dtype=np.float64)[0]
        self.ps, self.s, self.edges, self.centres = ps, s_above, edges, centres
        self.Dc, self.Dk, self.Dq = self.points.shape[1], len(ps), len(edges)
        self.mu, self.sigma = np.zeros((0, self.Dc), dtype=np.float32), np.zeros((0, self.Dc))
        self.cat = np.zeros((0, self.Dk), dtype=np.int64)
        self.qc, self.qs = np.zeros((0, self.Dq)), np.zeros((0, self.Dq))
        D = self.Dc + self.Dk + self.Dq
        for row in (() if given is None else np.asarray(given, dtype=np.float32).reshape(-1, D)):
            self.add(row)

    def split(self, rows):
        rows = np.asarray(rows)
        a, b = self.Dc, self.Dc + self.Dk
        return rows[..., :a], rows[..., a:b].astype(np.int64), rows[..., b:].astype(np.int64)

    def add(self, row):
        """Liar i = len(self.cat) at the f32 row; returns its sigma [Dc + Dq]."""
        z, v, qi = self.split(np.asarray(row, dtype=np.float32))
        i = len(self.cat)
        m = self.n + i + 1
        s = LR.liar_sigma(np.vstack([self.points, self.mu]), z, self.psig, m) if self.Dc else np.zeros(0)
        c = np.array([self.centres[d][qi[d]] for d in range(self.Dq)], dtype=np.float64)
        qs = quant_sigma(np.vstack([self.qpoints, self.qc]), c, self.qpsig, m) if self.Dq else np.zeros(0)
        self.mu, self.sigma = np.vstack([self.mu, z[None, :]]), np.vstack([self.sigma, s[None, :]])
        self.cat = np.vstack([self.cat, v[None, :]])
        self.qc, self.qs = np.vstack([self.qc, c[None, :]]), np.vstack([self.qs, qs[None, :]])
        return np.concatenate([s, qs])

    @property
    def sigmas(self):
        """[J, Dc + Dq]: what liar_sigma holds."""
        return np.hstack([self.sigma, self.qs])

    def log_kernels(self, cand):
        """log k_i [C, J] at the rows cand [C, D]."""
        z, v, qi = self.split(cand)
        J = len(self.cat)
        t = LR.log_kernels(z, self.mu, self.sigma, self.low, self.high) if self.Dc else np.zeros((len(cand), J))
        for d in range(self.Dk):
            t = t + np.log(M.ref_P(self.cat[:, d], self.ps[d], self.s[d]))[:, v[:, d]].T
        for d in range(self.Dq):
            with np.errstate(divide='ignore'):
                t = t + np.log(Q.ref_binP(self.qc[:, d], self.qs[:, d], self.edges[d]))[:, qi[:, d]].T
        return t

    def log_g(self, cand, g_base):
        J = len(self.cat)
        if J == 0:
            return np.array(g_base, dtype=np.float64)
        with np.errstate(divide='ignore'):
            lk = logsumexp(self.log_kernels(cand), axis=1)
        return np.logaddexp(g_base, lk - np.log(self.W)) - np.log1p(J / self.W)

    def extended_side(self, above):
        """The above side with the liar rows appended: weights (w~, 1, .., 1) /
        (W + J), xc rows the picks' categories, qmu / qsigma rows the centres and
        bandwidths: what log_g must equal through joint_quant_ref.ref_quant_lpdf."""
        w, mu, sigma, xc, qmu, qsig = above
        J = len(self.cat)
        wt = np.concatenate([np.asarray(w) * self.W, np.ones(J)]) / (self.W + J)
        return (wt, np.vstack([mu, self.mu.astype(np.float64)]), np.vstack([sigma, self.sigma]),
                np.vstack([xc, self.cat]), np.vstack([qmu, self.qc]), np.vstack([qsig, self.qs]))


def seeded_case(Dc, us, Vs, n, seed=None):
    """(below, above, low, high, psig, ps, s_below, s_above, edges): the sides as
    6-tuples; joint_quant_ref.seeded_quant_case, or joint_mixed_ref's recipe for
    a group without quantised labels."""
    if Vs:
        below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, us, Vs, n, seed)
    else:
        below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, n, seed)
        below = below + (np.zeros((len(below[0]), 0)),) * 2
        above = above + (np.zeros((len(above[0]), 0)),) * 2
        edges = []
    psig = np.asarray(above[2], dtype=np.float64)[0]
    return below, above, low, high, psig, ps, sb, sa, edges


def base_lpdf(cand, side, low, high, ps, s, edges):
    """float64 log-density of a side at the rows cand [C, D]."""
    Dc, Dk = side[1].shape[1], len(ps)
    cand = np.asarray(cand)
    return Q.ref_quant_lpdf(cand[:, :Dc].astype(np.float64), cand[:, Dc:Dc + Dk].astype(np.int64),
                            cand[:, Dc + Dk:].astype(np.int64), side, low, high, ps, s, edges)


def candidates(below, low, high, ps, s_below, edges, C, seed):
    """C shared f32 rows [C, D] drawn around the below side's components from
    RandomState(seed + 1): the continuous part as joint_liar_ref.candidates, a
    category the component's with probability 1 / (1 + s) (the prior's for the
    prior row and otherwise), a lattice index the bin of a normal draw."""
    rs = np.random.RandomState(seed + 1)
    w, mu, sigma, xc, qmu, qsig = below
    Dc = mu.shape[1]
    k = rs.choice(len(w), C, p=w)
    cols = []
    if Dc:
        z = (mu[k] + sigma[k] * rs.standard_normal((C, Dc))).astype(np.float32)
        lo32 = np.asarray(low).astype(np.float32)
        hi32 = np.nextafter(np.asarray(high).astype(np.float32), np.float32(-np.inf))
        cols.append(np.clip(z, lo32[None, :], hi32[None, :]))
    for d, p in enumerate(ps):
        own = (rs.uniform(size=C) < 1.0 / (1.0 + s_below[d])) & (xc[k, d] >= 0)
        cols.append(np.where(own, xc[k, d], rs.choice(len(p), C, p=p)).astype(np.float32)[:, None])
    for d, e in enumerate(edges):
        x = qmu[k, d] + qsig[k, d] * rs.standard_normal(C)
        cols.append(np.clip(np.searchsorted(e[1:-1], x, side='right'), 0, len(e) - 2).astype(np.float32)[:, None])
    return np.ascontiguousarray(np.hstack(cols), dtype=np.float32)


def greedy(chain, cand, l, g, B, forced=None):
    """B greedy steps over shared rows cand [C, D] with base l, g [C]: per step
    (g_j [C], tie set, score, the pick).  ``forced`` [B, D]: the row that joins
    after step j (teacher forcing); None: the reference's own pick."""
    steps = []
    for j in range(B):
        gj = chain.log_g(cand, g)
        ties, score = R.tie_set(l, gj)
        pick = int(np.argmax(score))
        steps.append((gj, ties, score, pick))
        chain.add(cand[pick] if forced is None else forced[j])
    return steps


# (Dc, category counts, lattice sizes, n, seed): the GPU cases.  The seeds are
# chosen so that the reference alone picks 8 distinct candidates with at most 8
# near-ties a step (tests/test_joint_liar_mixed_host.py checks it); the
# all-discrete case is exempt: equal rows score equally, by construction.
CASES = [
    (2, (3,), (), 60, 1),                                   # narrow mixed
    (0, (4, 2), (), 40, 1),                                 # all-discrete, uncapped
    (1, (2,), (5,), 80, 5),                                 # quantised
    (0, (), (3, 256), 120, 5),                              # all-quantised, the largest lattice
    (8, (2, 3, 4, 256), (2, 2, 252, 256), 150, 1),          # every limit at once
    (19, (3, 2), (), 200, 1),                               # wide mixed, D = 21
    (1, (2,), (4,), 3013, 4),                               # K_above = 3000
]


def case_inputs(Dc, us, Vs, n, seed, C):
    """Everything a test needs of one case, the reference l and g included."""
    below, above, low, high, psig, ps, sb, sa, edges = seeded_case(Dc, us, Vs, n, seed)
    cand = candidates(below, low, high, ps, sb, edges, C, seed)
    return dict(below=below, above=above, low=low, high=high, psig=psig, ps=ps, sb=sb, sa=sa, edges=edges,
                centres=centres_of(Vs), cand=cand, l=base_lpdf(cand, below, low, high, ps, sb, edges),
                g=base_lpdf(cand, above, low, high, ps, sa, edges))


def chain_of(c, W=None, given=None):
    return MixedChain(c['above'], c['psig'], c['low'], c['high'], c['ps'], c['sa'], c['edges'], c['centres'], W=W,
                      given=given)


def far_bin_case(C=1024, seed=3):
    """One quantised label of 256 values, 110 above trials that include the
    lattice values 0 and 1: a given liar at index 0 has both neighbours within
    one bin, so its sigma is the floor psig / 100 = 2.55 and every bin beyond
    26.5 sqrt(2) sigma of 0 has mass exactly 0.  Candidate 0 sits at index 255."""
    rs = np.random.RandomState(seed)
    V = 256
    edges = [Q.lattice_of(V)]
    qpmu, qpsig = np.array([0.5 * (V - 1.0)]), np.array([V - 1.0])
    sides = []
    for n in (10, 110):
        xq = np.rint(rs.uniform(0.0, V - 1.0, n))
        xq[:2] = [0.0, 1.0]
        w, qmu, qsig = R.ref_side(xq[:, None], qpmu, qpsig)
        sides.append((w, np.zeros((n + 1, 0)), np.zeros((n + 1, 0)), np.zeros((n + 1, 0), dtype=np.int64), qmu, qsig))
    below, above = sides
    cand = np.rint(rs.uniform(0.0, V - 1.0, C)).astype(np.float32)[:, None]
    cand[0, 0] = V - 1.0
    low = high = np.zeros(0)
    return dict(below=below, above=above, low=low, high=high, psig=np.zeros(0), ps=[], sb=np.zeros(0), sa=np.zeros(0),
                edges=edges, centres=centres_of((V,)), cand=cand, l=base_lpdf(cand, below, low, high, [], [], edges),
                g=base_lpdf(cand, above, low, high, [], [], edges))
