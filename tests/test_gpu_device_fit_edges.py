"""Edges of the device Parzen fit of the above mixture (tpe_fit_above: the
resident value order k_ord_chunks / k_ord_delta / k_ord_merge / k_ord_below,
then the rows k_fit_gather / k_fit_main / k_fit_combine / k_fit_wide) against
the oracle's adaptive_parzen_normal, where the index arithmetic can go wrong
and the large random histories of the other tests cannot show it:

  * K on and beside the edges of the build's chunks (kFitChunk = 2048),
  * the prior at position 0, at n, and on a chunk edge,
  * below observations at the head and tail of the order, 64 of them in one
    chunk's stretch, 64 consecutive tids (whole rank buckets),
  * tied observations (a degenerate grid included),
  * linear forgetting with lf around n (one ramped observation included),
  * the wide list: 15 / 16 components above a threshold, no level that
    qualifies (thr = inf), more candidates than the candidate list holds,
  * first sorts and merges at the sort's (8192) and the merge tile's (2048)
    sizes, and appended observations read in delta mode or merged.

Most cases use UNCLIPPED data: a normal(0, 1) prior (smin = 0.01 for K >= 99)
and sorted above observations whose consecutive gaps are smin * exp(U(log
1.25, log 8)), so every bandwidth but the prior's lies strictly inside the
clip [smin, smax] and a component that read a wrong neighbour gets a wrong
sigma.  (The random histories of the other tests sit at the clip.)  Each such
case asserts that on the oracle's own sigmas.

The injected candidates are float32 values: the kernels take a candidate's
coordinate in float32, so the reference is evaluated at the very point the
kernel sees (at coordinates of +-150 and bandwidths of 0.01 the rounding of
an arbitrary float64 candidate would be the sampler's error, not the fit's).

Measured on an MI355X, the worst of the file per check: means 1.8e-15
(relative), sigmas 6.0e-8, spread of c 1.3e-6 (the merge to 10241
observations), lpdf 8.7e-6 ('A lognormal K=4097': a tail candidate at t = -76
where the log-density and -ln x cancel to a reference of 0.03, so the relative
bound turns absolute while either term is 76; the normal case's same candidate
is at 1.2e-7).  Every normal and uniform case is under 2.4e-7, the other
lognormal ones under 2.5e-6.  The whole file runs in about 5 s.
"""
import numpy as np
import pytest

from oracle import tpe_oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 2048                     # kFitChunk: components per build workgroup
WIDE_CAP = 8192                  # kWideCap: wide candidates listed per job
PRUNE_WIDE = 16                  # kPruneWide: the wide list's length
N_THR = 5                        # kThr: wide thresholds smin * 2^(m+1), m < 5
A_SCALE = float(np.sqrt(0.5 / np.log(2.0)))      # a_k = A / max(sigma_k, EPS)
NORMAL = dict(mu=0.0, sigma=1.0)
SMIN = 0.01                      # of NORMAL at K >= 99


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _check_lpdf(got, ref, tol, what):
    """test_gpu_kernels._check_lpdf (the project's fp32 bound)."""
    ref = np.asarray(ref)
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)
    assert err.max() <= tol, (what, float(err.max()), int(np.argmax(err)))
    assert np.all((got[~fin] == ref[~fin]) | (got[~fin] < -700)), what


# ------------------------------------------------------------------ the oracle
def _prior(dist, args):
    if 'low' in args:
        return 0.5 * (args['low'] + args['high']), float(args['high'] - args['low'])
    return float(args['mu']), float(args['sigma'])


def _oracle(dist, args, obs, bidx, lf):
    """The oracle's above mixture of obs less obs[bidx] and what the checks
    derive from it.  The weights follow the observations in STABLE order (ties
    by tid, the device order's rule; np.argsort's default leaves tied
    observations in any order, which permutes the weights inside a tie)."""
    logf = dist in ('loguniform', 'lognormal')
    t = np.log(obs) if logf else np.asarray(obs, dtype=np.float64)
    m = np.zeros(len(obs), bool)
    m[bidx] = True
    ta = t[~m]
    n, K = len(ta), len(ta) + 1
    pmu, psig = _prior(dist, args)
    w_o, mu_o, sg_o = O.adaptive_parzen_normal(ta, 1.0, pmu, psig, lf)
    order = np.argsort(ta, kind='stable')
    pos = int(np.searchsorted(ta[order], pmu))
    assert len(mu_o) == K and mu_o[pos] == pmu and sg_o[pos] == psig
    if lf and lf < n:
        w = np.insert(O.linear_forgetting_weights(n, lf)[order], pos, 1.0)
    else:
        w = np.ones(K)
    w /= w.sum()
    if len(np.unique(ta)) == n:
        np.testing.assert_array_equal(w, w_o)                 # no ties: the oracle's own
    else:
        np.testing.assert_allclose(np.sort(w), np.sort(w_o), rtol=1e-14, atol=0)
    # the wide list by k_fit_combine's rule: the first level m < 5 with at most
    # 15 sigmas (the prior's apart) above smin * 2^(m+1); none: no wide list
    smin = psig / min(100.0, 1.0 + K)
    others = np.delete(sg_o, pos)
    thr = np.inf
    for lv in range(N_THR):
        if np.count_nonzero(others > smin * (2 << lv)) <= PRUNE_WIDE - 1:
            thr = smin * (2 << lv)
            break
    wide = [] if thr == np.inf else sorted(set(np.flatnonzero(sg_o > thr).tolist()) | {pos})
    # the wide candidates k_fit_main lists (sigma > 2 smin, and the prior) and
    # how many a job of K components lists at most (wide_cap: kWideCap, or what
    # its scratch segment of K - 1 entries holds after the header and the
    # chunks' statistics); with more, k_fit_wide examines every component
    n_cand = 1 + int(np.count_nonzero(others > 2 * smin))
    cand_cap = min(WIDE_CAP, K - 1 - (8 + 12 * ((K + CHUNK - 1) // CHUNK)))
    return dict(t=t, ta=ta, n=n, K=K, pmu=pmu, psig=psig, w=w, mu=mu_o, sigma=sg_o, pos=pos, smin=smin,
                others=others, thr=thr, wide=wide, n_cand=n_cand, cand_cap=cand_cap,
                logf=logf, low=args.get('low'), high=args.get('high'))


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _candidates(r):
    """A few hundred float32 points: each chunk-boundary mean mu[2048 k - 1],
    mu[2048 k] and the two ends, plus 0, +-0.5 and +-2 of the oracle's sigma
    there, and 200 points over [min(mu) - 3 psig, max(mu) + 3 psig] (clipped
    into [low, high) for a bounded prior); the log families' are exp of them."""
    mu, sg, K = r['mu'], r['sigma'], r['K']
    at = sorted({0, K - 1} | {i for k in range(1, K // CHUNK + 1) for i in (CHUNK * k - 1, CHUNK * k) if i < K})
    pts = [mu[i] + f * sg[i] for i in at for f in (0.0, 0.5, -0.5, 2.0, -2.0)]
    x = _f32(np.concatenate([pts, np.linspace(mu.min() - 3 * r['psig'], mu.max() + 3 * r['psig'], 200)]))
    if r['low'] is not None and not r['logf']:
        hi = float(np.nextafter(np.float32(r['high']), np.float32(r['low'])))
        x = np.clip(x, float(np.float32(r['low'])), hi)
        assert np.all(x >= r['low']) and np.all(x < r['high'])
    return np.exp(x) if r['logf'] else x


# ------------------------------------------------------------------ the helper
def fit_and_check(engine, dist, args, obs, bidx, lf, x=None, dev=None, unclipped=0, tag=''):
    """Fit the above mixture of ``obs`` less ``obs[bidx]`` on the device (as
    test_gpu_kernels._device_post, with ``lf`` and the History's ``dev`` dict so
    the value order stays resident between calls), score the injected ``x``
    (None: _candidates) and check rows, wide list, lpdf and the value order
    against the oracle.  ``unclipped``: at most that many of the oracle's
    sigmas (the prior's apart) may lie outside (1.2 smin, 0.9 smax) (None: not
    asserted).  Returns what the callers compare or assert further."""
    from hyperopt_amd import _native as N, devhist, history, parzen
    from hyperopt_amd.engine import LevelProblem
    obs = np.asarray(obs, dtype=np.float64)
    bidx = np.asarray(bidx, dtype=np.int32)
    n_obs, nb = len(obs), len(bidx)
    assert nb <= 64 and np.all(np.diff(bidx) > 0) and (nb == 0 or (bidx[0] >= 0 and bidx[-1] < n_obs))
    r = _oracle(dist, args, obs, bidx, lf)
    K, pos, smin, psig = r['K'], r['pos'], r['smin'], r['psig']
    assert K > 64
    if unclipped is not None:
        out = np.count_nonzero(~((r['others'] > 1.2 * smin) & (r['others'] < 0.9 * psig)))
        assert out <= unclipped, (tag, 'sigmas at the clip', out)
    if x is None:
        x = _candidates(r)
    lpdf = O.lgmm1_lpdf if r['logf'] else O.gmm1_lpdf
    ref = lpdf(x, r['w'], r['mu'], r['sigma'], low=r['low'], high=r['high'])
    assert np.all(np.isfinite(ref)), (tag, 'reference lpdf not finite')

    hist = history.History(np.arange(n_obs), np.zeros(n_obs), {'x': (np.arange(n_obs), obs)}, dev=dev)
    dc = devhist.columns(hist, engine.device)
    col = dc.column('x', r['t'])                                 # the kernel coordinate
    order = dc.order('x')
    n_in = order.n if order.n <= n_obs else 0
    n_new = n_obs - n_in
    delta = n_in > 0 and 0 < n_new <= N.FIT_DELTA_MAX
    post = parzen.fit_posterior(dist, args, obs[bidx], None, 1.0, lf=lf, above_dev=(col, n_obs, bidx, order))
    res, l, g = engine.run([LevelProblem(post, 0, [3], inject=x[None, :])], len(x), 1, want_lg=True)
    prob, comp32 = engine.device_tables()
    p = prob[0]

    # 1. the component count
    assert int(p['above_len']) == K, (tag, int(p['above_len']), K)
    rows = comp32[int(p['above_off']):int(p['above_off']) + K]
    rw = rows.astype(np.float64)
    # 2. means
    mu = rw[:, 0] + rw[:, 1]
    e2 = float(np.max(np.abs(mu - r['mu']) / np.maximum(np.abs(r['mu']), 1.0)))
    # 3. sigmas
    se = np.maximum(r['sigma'], O.EPS)
    e3 = float(np.max(np.abs(A_SCALE / rw[:, 2] - se) / se))
    # 4. c_k = log2(w_k / sigma_k) - shift: a constant offset from the oracle's
    lw = np.log2(r['w']) - np.log2(se)
    narrow = np.isfinite(rw[:, 3])
    assert narrow.any(), tag
    d = rw[narrow, 3] - lw[narrow]
    e4 = float(d.max() - d.min())
    # 6. the above lpdf at the injected candidates
    e6 = float(np.max(np.abs(g[0] - ref) / np.maximum(np.abs(ref), 1.0)))
    print('fit-edge %s: K %d pos %d nb %d wide %d | mean %.3g sigma %.3g c-spread %.3g lpdf %.3g'
          % (tag, K, pos, nb, len(r['wide']), e2, e3, e4, e6))       # (each figure before its assertion)
    np.testing.assert_allclose(mu, r['mu'], rtol=1e-12, atol=1e-12, err_msg=tag)
    np.testing.assert_allclose(A_SCALE / rw[:, 2], se, rtol=2e-7, err_msg=tag)
    assert e4 <= 4e-6, (tag, 'c', e4)
    # 5. the wide list: the oracle's set, in index order, each row a sorted row
    nw = int(p['wide_len'])
    assert len(r['wide']) <= PRUNE_WIDE
    assert nw == len(r['wide']) and np.flatnonzero(~narrow).tolist() == r['wide'], \
        (tag, nw, np.flatnonzero(~narrow).tolist()[:20], r['wide'])
    assert np.all(rw[~narrow, 3] == -np.inf), tag
    wide = comp32[int(p['wide_off']):int(p['wide_off']) + nw]
    for k, i in enumerate(r['wide']):
        np.testing.assert_array_equal(wide[k, :3].view(np.uint32), rows[i, :3].view(np.uint32), err_msg=tag)
        assert abs(float(wide[k, 3]) - lw[i] - np.median(d)) <= 4e-6, (tag, 'wide c', i, float(wide[k, 3]), lw[i])
    _check_lpdf(g[0], ref, 1e-5, (tag, 'g'))
    # 7. the resident value order: a stable argsort of the observations it holds
    held = order.n
    assert held == (n_in if delta else n_obs), (tag, held, n_in, n_obs, delta)
    keys, idx = order.host()
    want = np.argsort(r['t'][:held], kind='stable')
    np.testing.assert_array_equal(idx, want, err_msg=tag)
    np.testing.assert_array_equal(keys, r['t'][:held][want], err_msg=tag)
    return dict(r, rows=rows.copy(), wide_rows=wide.copy(), g=g[0].copy(), held=held, delta=delta)


# ------------------------------------------------------------------ the data
def _gaps(rs, m, lo=1.25, hi=8.0):
    """m consecutive gaps of the unclipped construction."""
    return SMIN * np.exp(rs.uniform(np.log(lo), np.log(hi), m))


def _sorted(gaps):
    return np.concatenate([[0.0], np.cumsum(gaps)])


def _center(a, b, pos):
    """a (sorted above values) and b (below values) shifted so the prior mean 0
    falls at index pos among a: strictly inside the gap (a[pos - 1], a[pos]),
    2 smin before a[0] (pos = 0) or after a[-1] (pos = n)."""
    n = len(a)
    if pos == 0:
        c = a[0] - 2 * SMIN
    elif pos == n:
        c = a[-1] + 2 * SMIN
    else:
        assert a[pos - 1] < a[pos]
        c = 0.5 * (a[pos - 1] + a[pos])
    return a - c, np.asarray(b, dtype=np.float64) - c


def _assemble(rs, a, b, below_tids=None, new_a=(), new_b=()):
    """Observations in tid order and the ascending below indices: a[i] are the
    above values, b[i] the below ones.  a[new_a] and b[new_b] take the last
    tids (the newest observations), b's others ``below_tids`` in the order
    given (None: random ones), the rest of a the remaining tids at random."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n, nb = len(a), len(b)
    new_a, new_b = list(new_a), list(new_b)
    k, total = len(new_a) + len(new_b), n + nb
    tid_a, tid_b = np.full(n, -1, dtype=np.int64), np.full(nb, -1, dtype=np.int64)
    newest = rs.permutation(np.arange(total - k, total))
    tid_a[new_a] = newest[:len(new_a)]
    tid_b[new_b] = newest[len(new_a):]
    old_b = np.flatnonzero(tid_b < 0)
    if below_tids is None:
        below_tids = rs.choice(total - k, len(old_b), replace=False)
    below_tids = np.asarray(below_tids, dtype=np.int64)
    assert len(below_tids) == len(old_b) and len(np.unique(below_tids)) == len(old_b)
    assert len(below_tids) == 0 or (below_tids.min() >= 0 and below_tids.max() < total - k)
    tid_b[old_b] = below_tids
    tid_a[tid_a < 0] = rs.permutation(np.setdiff1d(np.arange(total - k), below_tids))
    obs = np.empty(total)
    obs[tid_a] = a
    obs[tid_b] = b
    assert len(np.unique(np.concatenate([tid_a, tid_b]))) == total
    return obs, np.sort(tid_b).astype(np.int32)


def _standard(rs, n, nb, pos=None):
    """The unclipped construction: n above values, nb below values at random
    among them, the prior at index pos (None: mid-data)."""
    a = _sorted(_gaps(rs, n - 1))
    b = rs.uniform(a[0], a[-1], nb)
    return _center(a, b, n // 2 if pos is None else pos)


def _obs_of(dist, t):
    return np.exp(t) if dist == 'lognormal' else t


# ------------------------------------------------------------------ A: chunk edges
@pytest.mark.parametrize('dist', ['normal', 'lognormal'])
@pytest.mark.parametrize('K', [2047, 2048, 2049, 4096, 4097])
def test_chunk_edges(engine, dist, K):
    """K on and beside the build's chunk edges: the last chunk holds 2047,
    2048 or 1 components; 25 random below observations, the prior mid-data."""
    rs = np.random.RandomState(1000 + K)
    a, b = _standard(rs, K - 1, 25)
    t, bidx = _assemble(rs, a, b)
    fit_and_check(engine, dist, NORMAL, _obs_of(dist, t), bidx, 25, tag='A %s K=%d' % (dist, K))


# ------------------------------------------------------------------ B: the prior's position
@pytest.mark.parametrize('pos', [0, 2047, 2048, 2049, 'n'])
def test_prior_position(engine, pos):
    """K = 4100 with the prior first, last, and on / beside a chunk edge."""
    n = 4099
    rs = np.random.RandomState(2000 + (n if pos == 'n' else pos))
    a, b = _standard(rs, n, 25, n if pos == 'n' else pos)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='B pos=%s' % pos)
    assert r['pos'] == (n if pos == 'n' else pos)


def test_prior_position_ties_at_zero(engine):
    """pos = 0 through ties: three observations equal to prior_mu
    (np.searchsorted(side='left') puts the prior before them), the oldest of
    them a below observation, which follows three below observations under
    prior_mu at the head of the order — k_ord_below's n_under and head both
    count.  (One tied component's gaps are both 0: its sigma is at the clip.)"""
    n, nb = 4099, 25
    rs = np.random.RandomState(2100)
    a = np.concatenate([[0.0], _sorted(_gaps(rs, n - 2))])            # a[0] = a[1] = 0 = prior_mu
    b = np.concatenate([[0.0, -0.5, -1.0, -1.5], rs.uniform(a[2], a[-1], nb - 4)])
    tids = np.concatenate([[0], 1 + rs.choice(n + nb - 1, nb - 1, replace=False)])    # the tied below one: tid 0
    t, bidx = _assemble(rs, a, b, below_tids=tids)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, unclipped=1, tag='B ties at prior_mu')
    assert r['pos'] == 0 and r['mu'][1] == 0.0 and r['mu'][2] == 0.0
    assert bidx[0] == 0 and t[0] == 0.0 and np.count_nonzero(t == 0.0) == 3 and np.count_nonzero(t[bidx] < 0) == 3


# ------------------------------------------------------------------ C: the below list
def _below_case(rs, layout):
    n = 8236 if layout == 'tids_one_bucket' else 4099
    a = _sorted(_gaps(rs, n - 1))
    tids = None
    if layout in ('nb0', 'nb1'):
        b = rs.uniform(a[0], a[-1], int(layout[2:]))
    elif layout == 'head':                                     # the 64 smallest values: the order's head
        b = a[0] - SMIN * np.arange(1, 65)
    elif layout == 'tail':                                     # the 64 largest: its tail
        b = a[-1] + SMIN * np.arange(1, 65)
    elif layout == 'straddle':
        # 64 consecutive positions of the order between above observations 2047
        # and 2048 (components 2047 and 2048: the prior comes after them), so
        # the stretches of chunks 0 and 1 both hold all of them
        b = a[2047] + (a[2048] - a[2047]) * np.arange(1, 65) / 65.0
    else:
        b = rs.uniform(a[0], a[-1], 64)
        # 64 consecutive tids: two whole rank buckets (a bucket holds 32 tids at
        # 4163 observations), the first and the last bucket's (tid 0 and tid
        # n_obs - 1), or all of one bucket (64 tids each from 8193 observations)
        tids = {'tids': np.arange(1024, 1088), 'tids_one_bucket': np.arange(4096, 4160),
                'tids_ends': np.concatenate([np.arange(32), n + 64 - 32 + np.arange(32)])}[layout]
    a, b = _center(a, b, n // 2)
    return _assemble(rs, a, b, below_tids=tids)


@pytest.mark.parametrize('layout', ['nb0', 'nb1', 'head', 'tail', 'straddle', 'tids', 'tids_ends', 'tids_one_bucket'])
def test_below_list(engine, layout):
    """K = 4100 (8237 for 64 tids of one rank bucket) with no, one and 64 below
    observations; lf = 25, so the LF rank (tid less the older below
    observations) shows in every ramped row's c."""
    rs = np.random.RandomState(3000 + len(layout) + ord(layout[-1]))
    t, bidx = _below_case(rs, layout)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='C %s' % layout)
    if layout == 'tids_one_bucket':
        assert len(t) == 8300 and r['K'] == 8237 and np.all(bidx >> 6 == 64)
        return
    assert r['K'] == 4100 and r['pos'] == 2049
    o = np.argsort(t, kind='stable')
    at = np.flatnonzero(np.isin(o, bidx))                      # the below positions of the order
    if layout == 'head':
        assert at.tolist() == list(range(64))
    elif layout == 'tail':
        assert at.tolist() == list(range(len(t) - 64, len(t)))
    elif layout == 'straddle':
        assert at.tolist() == list(range(2048, 2048 + 64))
    elif layout == 'tids_ends':
        assert bidx[0] == 0 and bidx[-1] == len(t) - 1


# ------------------------------------------------------------------ D: ties
@pytest.mark.parametrize('n_obs', [300, 4200])
@pytest.mark.parametrize('value', [0.0, 1.0])
def test_all_equal(engine, n_obs, value):
    """Every observation equal, on a uniform(-5, 5) prior: 0.0 is prior_mu (pos
    = 0 and both grid bounds equal: a degenerate grid), 1.0 puts the whole run
    after the prior.  Weights attach in tid order."""
    rs = np.random.RandomState(4000 + n_obs)
    obs = np.full(n_obs, value)
    bidx = np.sort(rs.choice(n_obs, 25, replace=False)).astype(np.int32)
    r = fit_and_check(engine, 'uniform', dict(low=-5.0, high=5.0), obs, bidx, 25, unclipped=None,
                      tag='D all %.0f n_obs=%d' % (value, n_obs))
    assert r['pos'] == 0 and np.all(r['mu'][1:] == value)
    # the host packer builds the same grid for a host-fitted mixture: the same
    # candidates against the host fit's own mixture (np.argsort's tie order)
    from hyperopt_amd import parzen
    from hyperopt_amd.engine import LevelProblem
    m = np.zeros(n_obs, bool)
    m[bidx] = True
    host = parzen.fit_posterior('uniform', dict(low=-5.0, high=5.0), obs[m], obs[~m], 1.0)
    x = _candidates(r)
    res, l, g = engine.run([LevelProblem(host, 0, [3], inject=x[None, :])], len(x), 1, want_lg=True)
    ref = O.gmm1_lpdf(x, *host.above, low=-5.0, high=5.0)
    assert np.all(np.isfinite(ref))
    _check_lpdf(g[0], ref, 1e-5, ('D host fit', value, n_obs))


def test_tied_run_over_chunk_edge(engine):
    """300 equal values over components 1900 .. 2199 (straddling the chunk edge
    2048) inside otherwise unclipped data: the LF weights attach in tid order."""
    n = 4099
    rs = np.random.RandomState(4500)
    g = _gaps(rs, n - 1)
    g[1899:2198] = 0.0                                         # a[1899 .. 2198] equal
    a = _sorted(g)
    a, b = _center(a, rs.uniform(a[0], a[-1], 25), 1000)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, unclipped=None, tag='D tied run')
    assert r['pos'] == 1000 and np.all(r['mu'][1900:2200] == r['mu'][1900]) and r['mu'][1899] < r['mu'][1900] < r['mu'][2200]
    assert len(np.unique(r['w'][1900:2200])) > 250             # (ramped weights: the tie order shows)


# ------------------------------------------------------------------ E: linear forgetting
@pytest.mark.parametrize('oldest_wide', [False, True])
@pytest.mark.parametrize('lf', ['0', '25', 'n-2', 'n-1', 'n', 'n+1'])
def test_linear_forgetting(engine, lf, oldest_wide):
    """K = 2049 with lf around n = n_above.  lf = n - 1 leaves ONE ramped
    observation, the oldest: np.linspace(1 / n, 1, num=1) is [1 / n], not the
    endpoint 1.  The oldest above observation is a sorted row (k_fit_main's
    weight) or, between two gaps of 40 smin, a wide row (FitCtx::weight)."""
    n, nb = 2048, 25
    rs = np.random.RandomState(5000 + 2 * len(lf) + oldest_wide + ord(lf[-1]))
    g = _gaps(rs, n - 1)
    p0 = 500
    if oldest_wide:
        g[p0 - 1] = g[p0] = 40 * SMIN
    a = _sorted(g)
    a, b = _center(a, rs.uniform(a[0], a[-1], nb), n // 2)
    t, bidx = _assemble(rs, a, b)
    oldest = int(np.setdiff1d(np.arange(n + nb), bidx)[0])     # the oldest above observation
    j = int(np.flatnonzero(t == a[p0])[0])
    t[oldest], t[j] = t[j], t[oldest]                          # ... is the value a[p0]
    lf_n = {'0': 0, '25': 25, 'n-2': n - 2, 'n-1': n - 1, 'n': n, 'n+1': n + 1}[lf]
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, lf_n, tag='E lf=%s wide=%d' % (lf, oldest_wide))
    i0 = int(np.flatnonzero(r['mu'] == a[p0])[0])              # its component (p0 < pos)
    assert i0 == p0 and (i0 in r['wide']) == oldest_wide
    W = 1.0 / r['w'][r['pos']]                                  # (the prior weighs 1 before normalisation)
    if lf == 'n-1':
        assert abs(r['w'][i0] * W - 1.0 / n) < 1e-15 and np.count_nonzero(np.abs(r['w'] * W - 1.0) < 1e-12) == n
    elif lf in ('0', 'n', 'n+1'):
        assert np.all(np.abs(r['w'] * W - 1.0) < 1e-12)


# ------------------------------------------------------------------ F: the wide list
def _widened(rs, n, base, wide, at):
    """n above values with gaps of base * smin, the gaps ``at`` widened to wide * smin."""
    g = np.full(n - 1, base * SMIN)
    g[list(at)] = wide * SMIN
    a = _sorted(g)
    return _center(a, rs.uniform(a[0], a[-1], 25), 3000)


@pytest.mark.parametrize('count', [15, 16])
def test_wide_threshold_count(engine, count):
    """Exactly 15, then 16 sigmas above 2 smin (gaps of 1.5 smin, some widened
    to 3 smin: each lone widened gap gives two such sigmas, two adjacent ones
    three): 15 is the most the first level takes (thr = 2 smin, a full wide
    list with the prior); 16 moves to the next level, which none reaches."""
    rs = np.random.RandomState(6000 + count)
    lone = [10, 700, 2046, 2050, 2500, 4000] + ([3500, 4090] if count == 16 else [])
    a, b = _widened(rs, 4099, 1.5, 3.0, lone + ([1200, 1201] if count == 15 else []))
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='F %d over 2 smin' % count)
    assert np.count_nonzero(r['others'] > 2 * SMIN) == count and r['smin'] == SMIN
    assert r['thr'] == (2 * SMIN if count == 15 else 4 * SMIN) and len(r['wide']) == (16 if count == 15 else 1)


def test_wide_no_level(engine):
    """More than 15 sigmas above every threshold (20 of 80 smin > 64 smin):
    thr = inf, no wide list, the prior a sorted row."""
    rs = np.random.RandomState(6100)
    n = 4099
    g = _gaps(rs, n - 1)
    g[[5, 400, 900, 1500, 2047, 2300, 2800, 3300, 3700, 4090]] = 80 * SMIN
    a = _sorted(g)
    a, b = _center(a, rs.uniform(a[0], a[-1], 25), n // 2)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='F no level')
    assert np.count_nonzero(r['others'] > 64 * SMIN) >= 16 and r['thr'] == np.inf and r['wide'] == []


def test_wide_candidates_overflow(engine):
    """K = 10241 unclipped: more than kWideCap = 8192 components above 2 smin,
    so k_fit_wide examines every component through AboveSrc (64 below positions
    to skip) for the six of 40 smin and the prior."""
    rs = np.random.RandomState(6200)
    n = 10240
    g = _gaps(rs, n - 1)
    g[[300, 4095, 9000]] = 40 * SMIN
    a = _sorted(g)
    a, b = _center(a, rs.uniform(a[0], a[-1], 64), n // 2)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='F candidates overflow')
    assert r['n_cand'] >= WIDE_CAP + 1 and r['thr'] == 8 * SMIN and len(r['wide']) == 7


@pytest.mark.parametrize('nb', [0, 25])
def test_wide_candidates_outgrow_scratch(engine, nb):
    """K = 2049 with every gap above 2.5 smin: every component is a wide
    candidate, more than the job's scratch segment (K - 1 entries, the header
    and two chunks' statistics at its head) has room to list, though far fewer
    than kWideCap — k_fit_wide examines every component here too.  (Before
    wide_cap the list ran past the segment's end.)"""
    rs = np.random.RandomState(6300 + nb)
    n = 2048
    g = _gaps(rs, n - 1, lo=2.5)
    g[[300, 1500]] = 40 * SMIN
    a = _sorted(g)
    a, b = _center(a, rs.uniform(a[0], a[-1], nb), n // 2)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='F candidates outgrow scratch nb=%d' % nb)
    assert r['n_cand'] == r['K'] and r['cand_cap'] == 2048 - 32 < r['n_cand'] < WIDE_CAP
    assert r['thr'] == 8 * SMIN and len(r['wide']) == 5


# ------------------------------------------------------------------ G: first sort and merge sizes
@pytest.mark.parametrize('n_obs', [8191, 8192, 8193, 10239, 10241, 16384, 16385])
def test_first_sort_sizes(engine, n_obs):
    """A fresh order at the chunk sort's size (8192) and the merge tile's
    (2048) and one beside them."""
    rs = np.random.RandomState(7000 + n_obs)
    a, b = _standard(rs, n_obs - 25, 25)
    t, bidx = _assemble(rs, a, b)
    r = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, tag='G n_obs=%d' % n_obs)
    assert not r['delta'] and r['held'] == n_obs


# ------------------------------------------------------------------ H: incremental
def _incremental(engine, t, bidx, k, delta, tag):
    """A resident order of the first len(t) - k observations, then a call with
    all of them (delta mode: read beside the order; else merged), against a
    from-scratch fit: the same row bits, and each against the oracle."""
    from hyperopt_amd import _native as N
    assert N.FIT_DELTA_MAX == 16 and delta == (k <= N.FIT_DELTA_MAX)
    n0 = len(t) - k
    dev = {}
    r0 = fit_and_check(engine, 'normal', NORMAL, t[:n0], bidx[bidx < n0], 25, dev=dev, unclipped=None,
                       tag=tag + ' (resident)')
    assert r0['held'] == n0 and not r0['delta']
    r1 = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, dev=dev, tag=tag + ' (+%d)' % k)
    assert r1['delta'] == delta and r1['held'] == (n0 if delta else len(t))
    r2 = fit_and_check(engine, 'normal', NORMAL, t, bidx, 25, dev={}, tag=tag + ' (fresh)')
    assert not r2['delta'] and r2['held'] == len(t)
    for key in ('rows', 'wide_rows'):
        np.testing.assert_array_equal(r1[key].view(np.uint32), r2[key].view(np.uint32), err_msg=tag + ' ' + key)
    return r1


@pytest.mark.parametrize('layout', ['smallest', 'largest', 'equal', 'stretch', 'stretch_below64', 'two_below'])
def test_delta_mode(engine, layout):
    """16 new observations read beside a resident order (delta mode), K = 4100."""
    rs = np.random.RandomState(8000 + len(layout) + ord(layout[0]))
    n, nb = 4099, 64 if layout == 'stretch_below64' else 25
    new_b = ()
    if layout == 'equal':                                      # each new one equal to a resident one
        a0 = _sorted(_gaps(rs, n - 16 - 1))
        sel = np.sort(rs.choice(n - 16, 16, replace=False))
        a = np.sort(np.concatenate([a0, a0[sel]]))
        new_a = np.searchsorted(a, a0[sel], side='right') - 1  # (the newest of a tie sorts last)
    else:
        a = _sorted(_gaps(rs, n - 1))
        new_a = {'smallest': np.arange(16), 'largest': np.arange(n - 16, n),
                 'stretch': np.arange(2033, 2065, 2), 'stretch_below64': np.arange(2033, 2065, 2),
                 'two_below': np.sort(rs.choice(n, 14, replace=False))}[layout]
        new_b = (3, 11) if layout == 'two_below' else ()
    if layout == 'stretch_below64':                            # (test_below_list's 'straddle')
        b = a[2047] + (a[2048] - a[2047]) * np.arange(1, 65) / 65.0
    else:
        b = rs.uniform(a[0], a[-1], nb)
    pos = n // 2
    if layout == 'equal':                                      # (a gap between two distinct values)
        while not a[pos - 1] < a[pos]:
            pos += 1
    a, b = _center(a, b, pos)
    t, bidx = _assemble(rs, a, b, new_a=new_a, new_b=new_b)
    r = _incremental(engine, t, bidx, 16, True, 'H delta %s' % layout)
    assert r['K'] == 4100
    if layout == 'two_below':
        assert np.count_nonzero(bidx >= len(t) - 16) == 2
    if layout == 'equal':
        assert all(np.count_nonzero(t[:len(t) - 16] == v) == 1 for v in t[len(t) - 16:])


@pytest.mark.parametrize('n_obs', [8192, 8193, 10241])
def test_merge_17(engine, n_obs):
    """17 new observations (one more than delta mode takes) merged into the
    resident order, landing on the chunk sort's size, one past it, and one past
    a multiple of the merge tile."""
    rs = np.random.RandomState(8500 + n_obs)
    n = n_obs - 25
    a, b = _standard(rs, n, 25)
    t, bidx = _assemble(rs, a, b, new_a=np.sort(rs.choice(n, 17, replace=False)))
    _incremental(engine, t, bidx, 17, False, 'H merge n_obs=%d' % n_obs)


def test_delta_one_onto_chunk_edge(engine):
    """One new observation takes K from 2048 to 2049: a second chunk of one component."""
    rs = np.random.RandomState(8900)
    n = 2048
    a, b = _standard(rs, n, 25)
    t, bidx = _assemble(rs, a, b, new_a=[int(rs.randint(n))])
    r = _incremental(engine, t, bidx, 1, True, 'H delta 1')
    assert r['K'] == 2049
