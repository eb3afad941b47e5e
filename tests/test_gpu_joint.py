"""GPU tests of the joint TPE stage (tpe_joint_run through Engine.run_joint) and
of tpe.suggest(..., joint=...), against the float64 model restated in numpy
(tests/joint_ref.py).

Tolerances are the project's (tests/test_gpu_kernels.py): l and g within
1e-5 * max(1, |ref|); the winner inside the tie set score >= max - 4e-5 *
max(1, max|l|, max|g|) and equal to np.argmax when that set has one member;
Kolmogorov distance of the sampler below 6e-3 at 2^18 candidates.
"""
import numpy as np
import pytest
from scipy.special import ndtr

from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # a plateau of near-equal scores must not hide a wrong winner


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _candidates(below, low, high, psig, C, seed, n_far=32):
    """C f32 candidates [C, D]: one eighth drawn around the below mixture's
    components, the rest spread over the box / the prior; the last n_far sit 40
    prior sigmas beyond every observation in the first unbounded dimension.
    (Only an eighth near the peak: the far candidates' |l| of about 850 widens
    the tie window to 0.034, and a denser peak would sit inside it.)"""
    rs = np.random.RandomState(seed)
    w, mu, sigma = below
    D = mu.shape[1]
    n_near = C // 8
    k = rs.choice(len(w), size=n_near, p=w)
    near = mu[k] + sigma[k] * rs.standard_normal((n_near, D))
    bounded = np.isfinite(low)
    wide = np.where(bounded[None, :], rs.uniform(-10, 10, (C - n_near, D)), rs.normal(1.0, 4.0, (C - n_near, D)))
    z = np.vstack([near, wide])
    free = np.flatnonzero(~bounded)
    if len(free) and n_far:
        d = free[0]
        z[-n_far:, d] = mu[:, d].max() + 40.0 * psig[d] + rs.uniform(0, 1, n_far)
    z = z.astype(np.float32)
    lo32 = np.where(bounded, low, -np.inf).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, high, np.inf).astype(np.float32), np.float32(-np.inf))
    return np.clip(z, lo32[None, :], hi32[None, :])


def _check_winner(rec, cand, l_ref, g_ref, D, what, cap):
    ties, score = R.tie_set(l_ref, g_ref)
    idx = int(rec['global_idx'])
    print('%s: winner %d, argmax %d, %d ties' % (what, idx, int(np.argmax(score)), len(ties)))
    if cap:
        assert len(ties) <= MAX_TIES, (what, len(ties))
    assert idx in ties, (what, idx, int(np.argmax(score)), ties[:10])
    if len(ties) == 1:
        assert idx == int(np.argmax(score))
    np.testing.assert_array_equal(rec['z'][:D], cand[idx].astype(np.float64))
    assert (rec['z'][D:] == 0).all()


@pytest.mark.parametrize('D,n,n_below', [(3, 60, None), (8, 300, None), (16, 120, None), (1, 3013, None),
                                         (2, 3013, None)])
def test_scoring_of_injected_candidates(engine, D, n, n_below):
    """l, g and the winner of 4096 given candidates; (1, 3013) and (2, 3013)
    have 3000 above components, so the LDS tile loop wraps."""
    below, above, low, high, pmu, psig = R.seeded_case(D, n, 1000 * D + n, n_below)
    if n == 3013:
        assert len(above[0]) == 3000
    C = 4096
    cand = _candidates(below, low, high, psig, C, D)
    rec, l, g = engine.run_joint(below, above, low, high, [7], C, seed=3, inject=cand, want_lg=True)
    z64 = cand.astype(np.float64)
    l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
    assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(g[0]))          # the far candidates too: no -inf
    R.check_lpdf(l[0], l_ref, 'l D=%d n=%d' % (D, n))
    R.check_lpdf(g[0], g_ref, 'g D=%d n=%d' % (D, n))
    if D >= 2:
        far = slice(C - 32, C)
        assert np.all(g_ref[far] < -700) or np.all(l_ref[far] < -700)      # they are beyond a fixed shift's reach
    assert rec['l'][0] == l[0][int(rec['global_idx'][0])] and rec['g'][0] == g[0][int(rec['global_idx'][0])]
    _check_winner(rec[0], cand, l_ref, g_ref, D, 'D=%d n=%d' % (D, n), cap=D >= 3)


def test_sampling_follows_the_below_mixture(engine):
    """2^18 sampled vectors: in bounds, every marginal the exact mixture of
    truncated normals, and the returned l the density of the returned vectors."""
    D, C = 3, 1 << 18
    below, above, low, high, pmu, psig = R.seeded_case(D, 60, 11)
    rec, cand, l, g = engine.run_joint(below, above, low, high, [0], C, seed=99, return_cand=True, want_lg=True)
    z = cand[0].astype(np.float64)
    assert z.shape == (C, D) and np.all(np.isfinite(z))
    assert np.all(z >= low[None, :]) and np.all(z < high[None, :])
    w, mu, sigma = below
    for d in range(D):
        t = np.sort(z[:, d])
        grid = t[:: C // 512]
        za = (low[d] - mu[:, d]) / sigma[:, d]
        mass = ndtr((high[d] - mu[:, d]) / sigma[:, d]) - ndtr(za)
        F = (w[None, :] * (ndtr((grid[:, None] - mu[None, :, d]) / sigma[None, :, d]) - ndtr(za)[None, :])
             / mass[None, :]).sum(axis=1)
        Femp = (np.arange(0, C, C // 512) + 1) / C
        ks = float(np.max(np.abs(F - Femp)))
        print('dimension %d: Kolmogorov distance %.2e' % (d, ks))
        assert ks < 6e-3, (d, ks)
    sub = slice(0, C, 16)                      # (the density check on every 16th vector: 2^14 of them)
    R.check_lpdf(l[0][sub], R.ref_lpdf(z[sub], below, low, high), 'sampled l')
    R.check_lpdf(g[0][sub], R.ref_lpdf(z[sub], above, low, high), 'sampled g')
    i = int(rec['global_idx'][0])
    np.testing.assert_array_equal(rec['z'][0, :D], z[i])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    score = l[0] - g[0]
    assert i == int(np.argmax(score))          # the device's own scores: np.argmax order exactly


def test_one_component_per_vector(engine):
    """Two components of weight 1/2 at (-3, -3) and (3, 3), sigma 0.25: a vector
    comes from ONE component, so its coordinates share a sign.  A sampler that
    picked a component per dimension would put half the vectors off the diagonal."""
    C = 1 << 18
    w = np.array([0.5, 0.5])
    mu = np.array([[-3.0, -3.0], [3.0, 3.0]])
    sigma = np.full((2, 2), 0.25)
    above = (np.array([1.0]), np.zeros((1, 2)), np.full((1, 2), 5.0))
    inf = np.full(2, np.inf)
    rec, cand = engine.run_joint((w, mu, sigma), above, -inf, inf, [3], C, seed=5, return_cand=True)
    z = cand[0]
    assert not np.any(np.sign(z[:, 0]) != np.sign(z[:, 1]))
    frac = float(np.mean(z[:, 0] > 0))
    print('upper cluster: %.4f of the vectors' % frac)
    assert abs(frac - 0.5) <= 5e-3             # 5 binomial standard deviations at 2^18


def test_determinism_and_batching(engine):
    """The same call twice gives the same bytes; ids [5, 9, 12] in one call are
    three single calls; 4097 candidates leave a ragged last chunk."""
    C = 4096 + 1
    below, above, low, high, _, _ = R.seeded_case(4, 90, 21)
    ids = [5, 9, 12]
    a = engine.run_joint(below, above, low, high, ids, C, seed=17, return_cand=True, want_lg=True)
    b = engine.run_joint(below, above, low, high, ids, C, seed=17, return_cand=True, want_lg=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, 4) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    for j, new_id in enumerate(ids):
        s = engine.run_joint(below, above, low, high, [new_id], C, seed=17, return_cand=True, want_lg=True)
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    other = engine.run_joint(below, above, low, high, ids, C, seed=18, return_cand=True)
    assert other[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------ the public path
def _public_case():
    from hyperopt_amd import base, hp, rand
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.loguniform('y', -3, 2), 'z': hp.normal('z', 0, 2),
             'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, 2])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(80):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = (float(v['x']) * float(v['y']) - 2.0) ** 2 + 0.1 * float(v['z']) ** 2 + 0.05 * float(v['q']) \
            + 0.1 * int(v['c'])
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _model_from_trials(trials, labels):
    """The float64 joint model from the Trials alone: the gamma = 0.25 split
    (the ceil(0.25 sqrt(n)) best losses, at most 25), then per side the
    restated mixture over the labels' fit coordinates in tid order."""
    spec = {'x': (lambda v: v, 0.0, 10.0, -5.0, 5.0), 'y': (np.log, -0.5, 5.0, -3.0, 2.0),
            'z': (lambda v: v, 0.0, 2.0, -np.inf, np.inf)}
    docs = sorted(trials.trials, key=lambda d: d['tid'])
    loss = np.array([d['result']['loss'] for d in docs])
    assert len(np.unique(loss)) == len(loss)
    nb = min(int(np.ceil(0.25 * np.sqrt(len(loss)))), 25)
    m = np.zeros(len(loss), dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    X = np.stack([spec[k][0](np.array([float(d['misc']['vals'][k][0]) for d in docs])) for k in labels], axis=1)
    pmu = np.array([spec[k][1] for k in labels])
    psig = np.array([spec[k][2] for k in labels])
    low = np.array([spec[k][3] for k in labels])
    high = np.array([spec[k][4] for k in labels])
    return R.ref_side(X[m], pmu, psig), R.ref_side(X[~m], pmu, psig), low, high


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_joint_suggest():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import fit_coord
    domain, trials = _public_case()
    C, seed = 4096, 321
    plain = _vals(tpe.suggest([80], domain, trials, seed, n_EI_candidates=C)[0])
    doc = tpe.suggest([80], domain, trials, seed, n_EI_candidates=C, joint=True)[0]
    trials.assert_valid_trial(doc)
    got = _vals(doc)
    assert set(got) == set(plain)
    for k in ('q', 'c'):                       # not joined: the same bytes as without joint
        assert type(got[k]) is type(plain[k]) and got[k] == plain[k], k
    for k in ('x', 'y', 'z'):
        assert type(got[k]) is np.float64
    assert -5 <= got['x'] < 5 and np.exp(-3) <= got['y'] <= np.exp(2)

    def pool_check(labels, vals, cap):
        below, above, low, high = _model_from_trials(trials, labels)
        rec, cand, l, g = get_engine().run_joint(below, above, low, high, [80], C, seed, return_cand=True,
                                                 want_lg=True)
        args = {'x': ('uniform', {}), 'y': ('loguniform', {}), 'z': ('normal', {})}
        zc = np.array([fit_coord(args[k][0], args[k][1], vals[k]) for k in labels]).astype(np.float32)
        hit = np.flatnonzero((cand[0] == zc[None, :]).all(axis=1))
        assert len(hit) >= 1, (labels, zc)
        z64 = cand[0].astype(np.float64)
        l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
        R.check_lpdf(l[0], l_ref, 'public l %s' % (labels,))
        R.check_lpdf(g[0], g_ref, 'public g %s' % (labels,))
        ties, score = R.tie_set(l_ref, g_ref)
        print('%s: row %s, argmax %d, %d ties' % (labels, hit, int(np.argmax(score)), len(ties)))
        if cap:
            assert len(ties) <= MAX_TIES
        assert int(hit[0]) in ties and int(rec['global_idx'][0]) == int(hit[0])
        if len(ties) == 1:
            assert int(hit[0]) == int(np.argmax(score))
    pool_check(['x', 'y', 'z'], got, True)

    two = _vals(tpe.suggest([80], domain, trials, seed, n_EI_candidates=C, joint=['x', 'y'])[0])
    for k in ('z', 'q', 'c'):                  # z stays univariate
        assert type(two[k]) is type(plain[k]) and two[k] == plain[k], k
    pool_check(['x', 'y'], two, False)

    # batched ids equal single calls; the same call twice the same bytes; columns carry the joined labels
    ids = [80, 81, 82]
    batch = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=True)
    assert _vals(batch[0]) == got
    for j, new_id in enumerate(ids[1:], 1):
        assert _vals(tpe.suggest([new_id], domain, trials, seed, n_EI_candidates=C, joint=True)[0]) == _vals(batch[j])
    from hyperopt_amd import history
    hist = history.extract(domain, trials)
    cc = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=C, joint=True, columns=True)
    cc2 = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=C, joint=True, columns=True)
    assert cc.values.tobytes() == cc2.values.tobytes() and np.asarray(cc.active).all()
    for j in range(3):
        for lab, v in _vals(batch[j]).items():
            assert cc.values[j, cc.labels.index(lab)] == float(v), (j, lab)
