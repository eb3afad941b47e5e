"""Batch-aware joint suggests restated in plain numpy (DESIGN.md "Batch-aware
joint suggests"), for the liar tests: nothing here calls hyperopt_amd.

The ids of a batch pick greedily.  The above side has n trial rows and the
prior row, un-normalised weights w~ with sum W.  Step j scores under the above
mixture extended by J liars (the given vectors, then the earlier picks), each of
un-normalised weight 1, mean z (f32) and, per dimension, the bandwidth of the
adaptive-Parzen neighbour rule over the side's f32 mu values and the earlier
liars, clipped to [psig / min(100, m + 2), psig] with m = n + i + 1:

    log g_j(z) = logaddexp(log g(z), logsumexp_i log k_i(z) - log W) - log1p(J / W)
    log k_i(z) = -sum_d [log(sigma_id sqrt(2 pi) mass_id) + ((z_d - mu_id) / sigma_id)^2 / 2]
"""
import numpy as np
from scipy.special import logsumexp, ndtr

from tests import joint_ref as R


def weight_sum(n, prior_weight=1.0):
    """W of joint_ref.ref_side's weights before they are normalised."""
    w = np.ones(n)
    if n > R.LF:
        w = np.concatenate([np.linspace(1.0 / n, 1.0, num=n - R.LF), np.ones(R.LF)])
    return float(prior_weight) + float(w.sum())


def liar_sigma(points, z, psig, m):
    """sigma [D] (float64) of a liar at the f32 vector z: points [P, D] f32."""
    pts = np.asarray(points, dtype=np.float32).astype(np.float64)
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    out = np.empty(len(z))
    for d in range(len(z)):
        col = pts[:, d]
        gaps = []
        if (col <= z[d]).any():
            gaps.append(z[d] - col[col <= z[d]].max())
        if (col > z[d]).any():
            gaps.append(col[col > z[d]].min() - z[d])
        out[d] = max(gaps)
    psig = np.asarray(psig, dtype=np.float64)
    return np.clip(out, psig / min(100.0, m + 2.0), psig)


def log_kernels(z, mu, sigma, low, high):
    """log k_i(z) [C, J] of liars (mu, sigma [J, D]) at z [C, D]."""
    z = np.asarray(z, dtype=np.float64)
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    mass = ndtr((np.asarray(high)[None, :] - mu) / sigma) - ndtr((np.asarray(low)[None, :] - mu) / sigma)
    coef = -np.sum(np.log(sigma * np.sqrt(2 * np.pi) * mass), axis=1)
    q = ((z[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2
    return coef[None, :] - 0.5 * q.sum(axis=2)


class Chain(object):
    """The liars of one greedy batch over the above side ``above`` = (w, mu,
    sigma) of joint_ref.ref_side: ``add`` a vector, ``log_g`` the extended
    density from the base one."""

    def __init__(self, above, psig, low, high, W=None, given=None):
        self.points = np.asarray(above[1], dtype=np.float32)          # the rows as the device holds them
        self.n = len(self.points) - 1
        self.W = weight_sum(self.n) if W is None else float(W)
        self.psig, self.low, self.high = np.asarray(psig, dtype=np.float64), np.asarray(low), np.asarray(high)
        D = self.points.shape[1]
        self.mu, self.sigma = np.zeros((0, D), dtype=np.float32), np.zeros((0, D))
        for z in (() if given is None else np.asarray(given, dtype=np.float32).reshape(-1, D)):
            self.add(z)

    def add(self, z):
        """Liar i = len(self.mu) at the f32 vector z; returns its sigma [D]."""
        z = np.asarray(z, dtype=np.float32)
        i = len(self.mu)
        s = liar_sigma(np.vstack([self.points, self.mu]), z, self.psig, self.n + i + 1)
        self.mu, self.sigma = np.vstack([self.mu, z[None, :]]), np.vstack([self.sigma, s[None, :]])
        return s

    def log_g(self, z, g_base):
        J = len(self.mu)
        if J == 0:
            return np.array(g_base, dtype=np.float64)
        lk = logsumexp(log_kernels(z, self.mu, self.sigma, self.low, self.high), axis=1)
        return np.logaddexp(g_base, lk - np.log(self.W)) - np.log1p(J / self.W)

    def extended_side(self, above):
        """The above side with the liar rows appended, weights (w~, 1, .., 1) /
        (W + J): what log_g must equal through joint_ref.ref_lpdf."""
        w, mu, sigma = above
        J = len(self.mu)
        wt = np.concatenate([np.asarray(w) * self.W, np.ones(J)]) / (self.W + J)
        return wt, np.vstack([mu, self.mu.astype(np.float64)]), np.vstack([sigma, self.sigma])


def candidates(below, low, high, C, seed):
    """C shared f32 candidates [C, D] drawn around the below side's components
    from RandomState(seed + 1), clipped to [low, the largest f32 below high]."""
    rs = np.random.RandomState(seed + 1)
    w, mu, sigma = below
    D = mu.shape[1]
    k = rs.choice(len(w), C, p=w)
    z = (mu[k] + sigma[k] * rs.standard_normal((C, D))).astype(np.float32)
    lo32 = np.asarray(low).astype(np.float32)
    hi32 = np.nextafter(np.asarray(high).astype(np.float32), np.float32(-np.inf))
    return np.clip(z, lo32[None, :], hi32[None, :])


def greedy(chain, cand, l, g, B, forced=None):
    """B greedy steps over shared candidates cand [C, D] with base l, g [C]: per
    step (g_j [C], tie set, score, the pick).  ``forced`` [B, D] f32: the vector
    that joins after step j (teacher forcing); None: the reference's own pick."""
    steps = []
    for j in range(B):
        gj = chain.log_g(cand.astype(np.float64), g)
        ties, score = R.tie_set(l, gj)
        pick = int(np.argmax(score))
        steps.append((gj, ties, score, pick))
        chain.add(cand[pick] if forced is None else forced[j])
    return steps
