"""GPU tests of the wide joint stage (tpe_joint_wide_run through
Engine.run_joint_wide) and of tpe.suggest(..., joint=True, joint_wide=True),
against the float64 model restated in numpy (tests/joint_ref.py).

Tolerances are the project's, as in tests/test_gpu_joint.py: l and g within
1e-5 * max(1, |ref|); the winner inside the tie set score >= max - 4e-5 *
max(1, max|l|, max|g|) and equal to np.argmax when that set has one member;
Kolmogorov distance of the sampler below 6e-3 at 2^18 candidates.
"""
from functools import partial

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
    prior sigmas beyond every observation in the first unbounded dimension
    (tests/test_gpu_joint.py's recipe)."""
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


def _check_winner(rec, cand, l_ref, g_ref, D, what):
    ties, score = R.tie_set(l_ref, g_ref)
    idx = int(rec['global_idx'])
    print('%s: winner %d, argmax %d, %d ties' % (what, idx, int(np.argmax(score)), len(ties)))
    assert len(ties) <= MAX_TIES, (what, len(ties))
    assert idx in ties, (what, idx, int(np.argmax(score)), ties[:10])
    if len(ties) == 1:
        assert idx == int(np.argmax(score))
    np.testing.assert_array_equal(rec['z'][:D], cand[idx].astype(np.float64))
    assert (rec['z'][D:] == 0).all()


@pytest.mark.parametrize('D,n', [(17, 40), (17, 120), (20, 3013), (24, 300), (33, 60), (48, 120), (64, 26),
                                 (64, 300)])
def test_scoring_of_injected_candidates(engine, D, n):
    """l, g and the winner of 4096 given candidates.  (20, 3013) has 3000 above
    components, so the LDS tile loop wraps; 17 and 33 are padded to 20 and 48;
    64 is the full width."""
    from hyperopt_amd import _native as N
    below, above, low, high, pmu, psig = R.seeded_case(D, n, 1000 * D + n)
    if n == 3013:
        assert len(above[0]) == 3000
    C = 4096
    cand = _candidates(below, low, high, psig, C, D, n_far=32)
    rec, l, g = engine.run_joint_wide(below, above, low, high, [7], C, seed=3, inject=cand, want_lg=True)
    assert rec.dtype == N.JOINT_WIDE_RECORD_DTYPE and rec.shape == (1,) and l.shape == g.shape == (1, C)
    z64 = cand.astype(np.float64)
    l_ref, g_ref = R.ref_lpdf(z64, below, low, high, block=256), R.ref_lpdf(z64, above, low, high, block=256)
    assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(g[0]))          # the far candidates too: no -inf
    R.check_lpdf(l[0], l_ref, 'l D=%d n=%d' % (D, n))
    R.check_lpdf(g[0], g_ref, 'g D=%d n=%d' % (D, n))
    assert rec['l'][0] == l[0][int(rec['global_idx'][0])] and rec['g'][0] == g[0][int(rec['global_idx'][0])]
    _check_winner(rec[0], cand, l_ref, g_ref, D, 'D=%d n=%d' % (D, n))


def test_streams_continue_the_narrow_stage(engine):
    """The first 16 coordinates of a 20-wide run are the narrow stage's draw on
    the model cut to 16 dimensions, bit for bit; on one 16-dimension model the
    two stages draw the same candidates and agree on l, g and the winner."""
    below, above, low, high, _, _ = R.seeded_case(20, 60, 11)
    C, ids, seed = 4097, [5, 9], 41
    rec_w, cand_w = engine.run_joint_wide(below, above, low, high, ids, C, seed, return_cand=True)
    assert cand_w.shape == (2, C, 20) and cand_w.dtype == np.float32

    def cut(side):
        return side[0], np.ascontiguousarray(side[1][:, :16]), np.ascontiguousarray(side[2][:, :16])
    b16, a16, lo16, hi16 = cut(below), cut(above), low[:16], high[:16]
    rec_n, cand_n, l_n, g_n = engine.run_joint(b16, a16, lo16, hi16, ids, C, seed, return_cand=True, want_lg=True)
    assert np.ascontiguousarray(cand_w[:, :, :16]).tobytes() == cand_n.tobytes()

    rec_s, cand_s, l_s, g_s = engine.run_joint_wide(b16, a16, lo16, hi16, ids, C, seed, return_cand=True,
                                                    want_lg=True)
    assert cand_s.tobytes() == cand_n.tobytes()
    for j in range(2):
        z64 = cand_n[j].astype(np.float64)
        l_ref, g_ref = R.ref_lpdf(z64, b16, lo16, hi16, block=256), R.ref_lpdf(z64, a16, lo16, hi16, block=256)
        R.check_lpdf(l_s[j], l_ref, 'wide l at D=16, id %d' % j)
        R.check_lpdf(g_s[j], g_ref, 'wide g at D=16, id %d' % j)
        R.check_lpdf(l_n[j], l_ref, 'narrow l at D=16, id %d' % j)
        R.check_lpdf(g_n[j], g_ref, 'narrow g at D=16, id %d' % j)
        ties, score = R.tie_set(l_ref, g_ref)
        assert int(rec_s['global_idx'][j]) in ties and int(rec_n['global_idx'][j]) in ties
        if len(ties) == 1:
            assert int(rec_s['global_idx'][j]) == int(rec_n['global_idx'][j]) == int(np.argmax(score))
        i = int(rec_s['global_idx'][j])
        np.testing.assert_array_equal(rec_s['z'][j, :16], z64[i])
        assert (rec_s['z'][j, 16:] == 0).all()


def test_sampling_follows_the_below_mixture(engine):
    """2^18 sampled 20-vectors: in bounds, every marginal the exact mixture of
    truncated normals (dimensions 3, 7, 11, 15 and 19 are the first words of
    Philox blocks 1 to 5), and the returned l, g the densities of the returned
    vectors."""
    D, C = 20, 1 << 18
    below, above, low, high, pmu, psig = R.seeded_case(D, 60, 11)
    rec, cand, l, g = engine.run_joint_wide(below, above, low, high, [0], C, seed=99, return_cand=True, want_lg=True)
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
    R.check_lpdf(l[0][sub], R.ref_lpdf(z[sub], below, low, high, block=256), 'sampled l')
    R.check_lpdf(g[0][sub], R.ref_lpdf(z[sub], above, low, high, block=256), 'sampled g')
    i = int(rec['global_idx'][0])
    np.testing.assert_array_equal(rec['z'][0, :D], z[i])
    assert (rec['z'][0, D:] == 0).all()
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    assert i == int(np.argmax(l[0] - g[0]))    # the device's own scores: np.argmax order exactly


def test_one_component_per_vector(engine):
    """Two components of weight 1/2 at -3 * 1 and +3 * 1, sigma 0.25: a vector
    comes from ONE component, so its 20 coordinates share a sign."""
    D, C = 20, 1 << 18
    w = np.array([0.5, 0.5])
    mu = np.stack([np.full(D, -3.0), np.full(D, 3.0)])
    sigma = np.full((2, D), 0.25)
    above = (np.array([1.0]), np.zeros((1, D)), np.full((1, D), 5.0))
    inf = np.full(D, np.inf)
    rec, cand = engine.run_joint_wide((w, mu, sigma), above, -inf, inf, [3], C, seed=5, return_cand=True)
    s = np.sign(cand[0])
    assert not np.any(s == 0) and not np.any(s != s[:, :1])
    frac = float(np.mean(cand[0][:, 0] > 0))
    print('upper cluster: %.4f of the vectors' % frac)
    assert abs(frac - 0.5) <= 5e-3             # 5 binomial standard deviations at 2^18


def test_determinism_and_batching(engine):
    """The same call twice gives the same bytes; ids [5, 9, 12] in one call are
    three single calls; 4097 candidates leave a ragged last chunk (of 512 at
    this width, and of 256 in the sampler)."""
    D, C = 24, 4096 + 1
    below, above, low, high, _, _ = R.seeded_case(D, 90, 21)
    ids = [5, 9, 12]
    a = engine.run_joint_wide(below, above, low, high, ids, C, seed=17, return_cand=True, want_lg=True)
    b = engine.run_joint_wide(below, above, low, high, ids, C, seed=17, return_cand=True, want_lg=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, D) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    for j, new_id in enumerate(ids):
        s = engine.run_joint_wide(below, above, low, high, [new_id], C, seed=17, return_cand=True, want_lg=True)
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    other = engine.run_joint_wide(below, above, low, high, ids, C, seed=18, return_cand=True)
    assert other[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------ the public path
def _flat_case(extra=False):
    """bench.py config 4's space (20 labels of uniform(-5, 5)) with 40 completed trials."""
    from hyperopt_amd import base, hp, rand
    space = {'x%02d' % i: hp.uniform('x%02d' % i, -5, 5) for i in range(20)}
    if extra:
        space['q'] = hp.quniform('q', 0, 10, 1)
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items() if len(x)}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': sum((v['x%02d' % i] - 0.1 * i) ** 2 for i in range(20))
                             + 0.05 * v.get('q', 0.0)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_wide_suggest():
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    domain, trials = _flat_case()
    C, seed, ids = 4096, 321, [40, 41]
    docs = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=True, joint_wide=True)
    hist = history.extract(domain, trials)
    group = list(domain.table.rows)
    assert len(group) == 20
    model = J.fit_model(group, hist, history.split_below(hist, tpe._default_gamma), tpe._default_prior_weight,
                        tpe.DEFAULT_LF)
    rec = get_engine().run_joint_wide(model.below, model.above, model.low, model.high, ids, C, seed)
    assert (rec['global_idx'] >= 0).all() and (rec['z'][:, 20:] == 0).all()
    want = model.values(rec['z'][:, :20])
    for j, doc in enumerate(docs):
        trials.assert_valid_trial(doc)
        got = _vals(doc)
        assert set(got) == set(domain.table.labels)
        for d, r in enumerate(group):
            v = got[r.label]
            assert type(v) is np.float64 and -5 <= v < 5, (r.label, v)
            assert v == want[j, d], (j, r.label, v, want[j, d])
    again = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=True, joint_wide=True)
    assert [_vals(d) for d in again] == [_vals(d) for d in docs]
    cc = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=C, joint=True, joint_wide=True,
                             columns=True)
    for j in range(2):
        for lab, v in _vals(docs[j]).items():
            assert cc.values[j, cc.labels.index(lab)] == float(v), (j, lab)


def test_public_label_outside_the_group_is_unchanged():
    from hyperopt_amd import tpe
    domain, trials = _flat_case(extra=True)
    C, seed = 4096, 321
    plain = _vals(tpe.suggest([40], domain, trials, seed, n_EI_candidates=C)[0])
    got = _vals(tpe.suggest([40], domain, trials, seed, n_EI_candidates=C, joint=True, joint_wide=True)[0])
    assert set(got) == set(plain)
    assert type(got['q']) is type(plain['q']) and got['q'] == plain['q']
    assert any(got[k] != plain[k] for k in plain if k != 'q')      # the 20 joined labels took the joint winner


def test_fmin_runs_with_a_wide_group():
    from hyperopt_amd import fmin, hp, tpe
    space = {'x%02d' % i: hp.uniform('x%02d' % i, -5, 5) for i in range(20)}
    best = fmin(lambda v: sum(x * x for x in v.values()), space,
                algo=partial(tpe.suggest, joint=True, joint_wide=True), max_evals=30,
                rstate=np.random.RandomState(3))
    assert set(best) == set(space) and all(-5 <= v < 5 for v in best.values())
