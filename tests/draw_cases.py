"""The mixtures of tests/test_gpu_draws.py, built in plain numpy so that
tests/test_draw_ref_host.py checks the model on the same ones without a GPU.

A case is a dict: dist, family (draw_ref's numbering = the engine's), low,
high (sampling space), q, below / above = (w, mu, sigma) or (p,), upper.
"""
import numpy as np

from tests import draw_ref as R

SEED = 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF        # both 32-bit words non-zero
IDS = (1000003, -(1 << 63) + 0x1234ABCD9)             # the second: high bit set, low word 0x234ABCD9
LABEL_BIG = (1 << 31) - 5
C_A = 2 * 2048 + 37                                   # two tiles and a partial one, odd
LDS_ROWS = 1024                                       # TPE_SAMPLE_LDS_ROWS (include/tpe_hip.h)
KS = (1, 26, 64, 65, LDS_ROWS, LDS_ROWS + 1)

SPACES = {
    'uniform': dict(low=-2.0, high=3.0), 'loguniform': dict(low=-4.0, high=1.0),
    'normal': dict(mu=0.5, sigma=2.0), 'lognormal': dict(mu=0.0, sigma=1.0),
    'quniform': dict(low=0.0, high=10.0, q=0.5), 'qloguniform': dict(low=0.0, high=5.0, q=2.0),
    'qnormal': dict(mu=2.0, sigma=4.0, q=0.5), 'qlognormal': dict(mu=1.0, sigma=0.7, q=0.25),
}
CONTINUOUS = tuple(SPACES)
DISTS = CONTINUOUS + ('randint', 'categorical')


def case(dist, below, above, low=None, high=None, q=None, upper=0):
    return dict(dist=dist, family=R.FAMILY[dist], low=low, high=high, q=q, below=below, above=above, upper=upper)


def _above(lo, hi, psig):
    return (np.array([0.5, 0.3, 0.2]), lo + (hi - lo) * np.array([0.2, 0.55, 0.8]), psig * np.array([0.5, 1.0, 0.25]))


def continuous_case(dist, K):
    """K-component below mixture of `dist`.  From K = 26 on a bounded one holds:
    a component wholly outside the bounds (mass 0: cum repeats a value), a
    mirrored one (za > 0) with visible mass, one nearly all outside on each side
    (fb - fa about 1e-6, weighted up so that it is drawn), and sigma = psig / 100."""
    a = SPACES[dist]
    bounded = 'low' in a
    lo, hi = (a['low'], a['high']) if bounded else (a['mu'] - 2 * a['sigma'], a['mu'] + 2 * a['sigma'])
    psig = (hi - lo) if bounded else a['sigma']
    rs = np.random.RandomState(100 + K)
    mu = rs.uniform(lo, hi, K)
    sg = rs.uniform(psig / 50, psig, K)
    w = rs.uniform(0.5, 1.5, K)
    if K >= 26:
        sg[3] = psig / 100                                      # the fit's smallest bandwidth
        if bounded:
            mu[0], sg[0] = hi + 60 * psig / 100, psig / 100       # wholly outside
            mu[1], sg[1] = lo - 0.3 * psig / 10, psig / 10        # mirrored, most mass inside reach
            mu[2], sg[2], w[2] = lo - 4.75 * psig / 20, psig / 20, 2e3 * K    # ~1e-6 visible, mirrored
            mu[4], sg[4], w[4] = hi + 4.75 * psig / 20, psig / 20, 2e3 * K    # ~1e-6 visible, high side
    order = np.argsort(mu, kind='stable')
    w, mu, sg = w[order] / w.sum(), mu[order], sg[order]
    return case(dist, (w, mu, sg), _above(lo, hi, psig), a.get('low'), a.get('high'), a.get('q'))


def categorical_case(dist, K):
    rs = np.random.RandomState(200 + K)
    p = rs.uniform(0.2, 1.0, K)
    if K >= 3:
        p[K // 2] = 0.0                                           # never drawn: cum repeats a value
    pa = rs.uniform(0.2, 1.0, K)
    return case(dist, (p / p.sum(),), (pa / pa.sum(),), upper=K)


def cases_a(dist):
    """[(name, case)] of section A for one family."""
    if dist == 'randint':
        return [('randint%d' % K, categorical_case(dist, K)) for K in KS]
    if dist == 'categorical':
        return [('categorical%d' % K, categorical_case(dist, K)) for K in (3, 26)]
    return [('%s%d' % (dist, K), continuous_case(dist, K)) for K in KS]


def rows_of(c):
    if c['family'] == R.CATEGORICAL:
        return R.sampler_rows(c['family'], p=c['below'][0])
    return R.sampler_rows(c['family'], *c['below'], low=c['low'], high=c['high'])


# ---------------------------------------------------------------- B, C, D
# above mixture of the B / C cases: more than 64 components, so that the
# per-candidate path (TPE_TABLES=0) sorts and prunes (and pools several ids)
def _above_wide(lo, hi, sigma):
    n = 80
    rs = np.random.RandomState(7)
    return (np.full(n, 1.0 / n), np.sort(rs.uniform(lo, hi, n)), np.full(n, sigma))


def edge_weights(wstar, variant):
    """c of section B for the selection word wstar: (w* + 0.5) 2^-32, the next
    double above it, and c - 2^-33.  At most 34 significant bits each."""
    c = (wstar + 0.5) * 2.0 ** -32
    return (c, float(np.nextafter(c, 2.0)), c - 2.0 ** -33)[variant]


EDGE_EXPECT = (1, 0, 1)            # component of the candidate drawn from w*, per variant


def two_component_case(c):
    """Unbounded normal, components at -4 and 4 (sigma 0.5), weights (c, 1 - c)."""
    return case('normal', (np.array([c, 1.0 - c]), np.array([-4.0, 4.0]), np.array([0.5, 0.5])),
                _above_wide(-6.0, 6.0, 1.0))


SIX_MU = np.array([-7.5, -4.5, -1.5, 1.5, 4.5, 7.5])


def six_component_case(c, j):
    """Six components, four weights of 2^-20 in a row: cum = c0, c0 + 2^-20, ..,
    c0 + 4 2^-20, 1 with cum[j] = c — five edges inside one 1/256 slice of the
    CDF (the caller checks that), so a fast kernel's guide entry settles two and
    guided_more walks the rest."""
    e = 2.0 ** -20
    w = np.array([c - j * e, e, e, e, e, 1.0 - c - (4 - j) * e])
    return case('normal', (w, SIX_MU.copy(), np.full(6, 0.5)), _above_wide(-8.0, 8.0, 1.0))


def selection_word(label_ix, new_id, g, seed=SEED):
    """The 32-bit selection word of global index g (f32, non-categorical)."""
    return int(R.uniforms(R.GAUSS, seed, label_ix, new_id, np.array([g], dtype=np.uint64), 'fp32')[3][0])


EDGE_INDICES = (0, 1, 2047, 2048, C_A - 1)


def cases_b(new_id=IDS[0], n_cand=C_A, label0=40):
    """[(name, label_ix, case, index of the w* candidate, expected component)]:
    the two-component mixtures for every edge index and variant, then the
    six-component mixtures with w* = candidate 1's word on each of five edges."""
    out = []
    ix = label0
    for i in EDGE_INDICES:
        i = min(i, n_cand - 1)
        for v in range(3):
            ws = selection_word(ix, new_id, i)
            out.append(('two_i%d_v%d' % (i, v), ix, two_component_case(edge_weights(ws, v)), i, EDGE_EXPECT[v]))
            ix += 1
    for j in range(5):
        for v in range(3):
            ws = selection_word(ix, new_id, 1)
            c = edge_weights(ws, v)
            assert c - j * 2.0 ** -20 > 0 and c + (4 - j) * 2.0 ** -20 < 1, 'pick another label index'
            assert int((c - j * 2.0 ** -20) * 256) == int((c + (4 - j) * 2.0 ** -20) * 256), 'pick another label index'
            out.append(('six_e%d_v%d' % (j, v), ix, six_component_case(c, j), 1, j + EDGE_EXPECT[v]))
            ix += 1
    return out


def cases_c_extra(label0=90):
    """One bounded loguniform and one quniform for section C."""
    lg = case('loguniform', (np.array([0.3, 0.5, 0.2]), np.array([-3.0, -1.0, 0.5]), np.array([0.6, 0.8, 0.5])),
              _above_wide(-4.0, 1.0, 0.7), -4.0, 1.0)
    qu = case('quniform', (np.array([0.4, 0.6]), np.array([2.0, 7.0]), np.array([1.5, 1.0])),
              _above_wide(0.0, 10.0, 1.2), 0.0, 10.0, 0.5)
    return [('loguniform', label0, lg), ('quniform', label0 + 1, qu)]


def case_d_fast():
    """cand_base = 1, C = 2049: few enough cells to be tabulated at that size."""
    return case('normal', (np.array([0.4, 0.6]), np.array([-4.0, 4.0]), np.array([1.0, 1.0])), _above_wide(-6.0, 6.0, 1.5))


def posterior(c):
    """The case as a parzen.Posterior (the only use of the package here)."""
    from hyperopt_amd import parzen
    return parzen.Posterior(c['dist'], c['family'], c['low'], c['high'], c['q'], c['below'], c['above'], c['upper'])


def all_cases():
    """Every (name, case) the GPU file uses."""
    out = [nc for dist in DISTS for nc in cases_a(dist)]
    out += [(n, c) for n, _, c, _, _ in cases_b()]
    out += [(n, c) for n, _, c in cases_c_extra()]
    out.append(('d_fast', case_d_fast()))
    return out


# ------------------------------------------------------------ exact laws
def mixture_cdf(c, grid):
    """Exact CDF of the (truncated) below mixture in the kernel coordinate
    (test_philox_sampler_distribution's formula)."""
    from scipy.special import erf
    w, mu, sg = c['below']
    Phi = lambda z: 0.5 * (1 + erf(z / np.sqrt(2)))
    if c['low'] is None:
        return (w[None, :] * Phi((grid[:, None] - mu) / sg)).sum(1)
    mass = Phi((c['high'] - mu) / sg) - Phi((c['low'] - mu) / sg)
    return (w * (Phi((grid[:, None] - mu) / sg) - Phi((c['low'] - mu) / sg))).sum(1) / (w * mass).sum()


def lattice_masses(c, points):
    """Exact mass of each lattice value of a quantised case: the (truncated)
    mixture's mass of the coordinates that np.round(x / q) sends to it."""
    q = c['q']
    log = c['family'] == R.QLOGGAUSS
    lo_x, hi_x = (points - 0.5 * q, points + 0.5 * q)
    with np.errstate(divide='ignore'):
        lo_t, hi_t = (np.log(np.maximum(lo_x, 0.0)), np.log(hi_x)) if log else (lo_x, hi_x)
    if c['low'] is not None:
        lo_t, hi_t = np.clip(lo_t, c['low'], c['high']), np.clip(hi_t, c['low'], c['high'])
    big = np.where(np.isfinite(lo_t), lo_t, -1e300)
    return mixture_cdf(c, hi_t) - mixture_cdf(c, big)
