"""GPU tests of the segmented joint stage (tpe_joint_seg_run through
Engine.run_joint_segments) and of tpe.suggest(..., joint=True,
joint_branches=True) on a tree space (DESIGN.md "Branch groups").

The stage's defining property is tested as bytes: problem (id, segment) equals
a tpe_joint_run over that segment alone with its stream word and ids = [id].
Against the float64 model restated in numpy (tests/joint_ref.py) the tolerances
are the project's (tests/test_gpu_joint.py): l and g within 1e-5 * max(1,
|ref|), the winner inside the tie set, and at most MAX_TIES members in it.
"""
import functools

import numpy as np
import pytest

from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # a plateau of near-equal scores must not hide a wrong winner
C = 4096 + 1          # 5 chunks, the last ragged
SEED = 17


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _segments():
    """(models, stream words): D = 2 with the prior alone above, D = 3, D = 5
    (DP 6: one padded dimension; 296 above components wrap the 128-row LDS
    tile), D = 16, and one segment no problem names."""
    cases = [R.seeded_case(2, 40, 202, n_below=40), R.seeded_case(3, 60, 203), R.seeded_case(5, 300, 205),
             R.seeded_case(16, 120, 216), R.seeded_case(4, 50, 204)]
    assert len(cases[0][1][0]) == 1 and len(cases[2][1][0]) == 296
    return [c[:4] for c in cases], [0xFFFFFFFE - 3 * s for s in range(len(cases))]


# (new id, segment): non-contiguous ids, id 9 in two segments, two ids in segments 0, 2 and 3, not sorted by segment
PROBLEMS = [(9, 2), (5, 0), (40, 3), (9, 1), (12, 2), (1000003, 0), (7, 3)]


def _single(engine, model, word, new_id, inject=None):
    """tpe_joint_run over one segment alone with its stream word."""
    below, above, low, high = model
    return engine.run_joint(below, above, low, high, [new_id], C, SEED, inject, True, True, stream_word=word)


@pytest.fixture(scope='module')
def seg_run(engine):
    """The segmented call over PROBLEMS (computed once, shared, not modified)."""
    models, words = _segments()
    ids, segs = [p[0] for p in PROBLEMS], [p[1] for p in PROBLEMS]
    out = engine.run_joint_segments(models, words, segs, ids, C, SEED, return_cand=True, want_lg=True)
    return models, words, out


def test_segmented_run_equals_single_runs_bytes(engine, seg_run):
    models, words, (rec, cand, l, g) = seg_run
    assert rec.shape == (7,) and l.shape == g.shape == (7, C) and len(cand) == 7
    for p, (new_id, s) in enumerate(PROBLEMS):
        D = len(models[s][2])
        assert cand[p].shape == (C, D) and cand[p].dtype == np.float32
        srec, scand, sl, sg = _single(engine, models[s], words[s], new_id)
        assert rec[p:p + 1].tobytes() == srec.tobytes(), (p, rec[p], srec)
        assert cand[p].tobytes() == scand[0].tobytes(), p
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes(), p
    # id 9 draws independently in its two segments; two ids of one segment differ
    assert cand[0][:, :3].tobytes() != cand[3].tobytes() and cand[0].tobytes() != cand[4].tobytes()
    # the stream word matters: the root group's word gives other candidates
    other = engine.run_joint(*models[1], [9], C, SEED, return_cand=True)
    assert other[1][0].tobytes() != cand[3].tobytes()


def test_twice_the_same_bytes_and_any_problem_order(engine, seg_run):
    models, words, first = seg_run
    ids, segs = [p[0] for p in PROBLEMS], [p[1] for p in PROBLEMS]
    again = engine.run_joint_segments(models, words, segs, ids, C, SEED, return_cand=True, want_lg=True)
    assert again[0].tobytes() == first[0].tobytes()
    assert again[2].tobytes() == first[2].tobytes() and again[3].tobytes() == first[3].tobytes()
    for x, y in zip(again[1], first[1]):
        assert x.tobytes() == y.tobytes()
    perm = [6, 2, 4, 0, 5, 1, 3]
    rec, cand, l, g = engine.run_joint_segments(models, words, [segs[p] for p in perm], [ids[p] for p in perm], C, SEED,
                                                return_cand=True, want_lg=True)
    for q, p in enumerate(perm):
        assert rec[q:q + 1].tobytes() == first[0][p:p + 1].tobytes(), (q, p)
        assert cand[q].tobytes() == first[1][p].tobytes()
        assert l[q].tobytes() == first[2][p].tobytes() and g[q].tobytes() == first[3][p].tobytes()
    # records alone: the same winners without the optional outputs
    assert engine.run_joint_segments(models, words, segs, ids, C, SEED).tobytes() == first[0].tobytes()


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


def test_against_the_float64_model(seg_run):
    """l, g and the winner of every problem of the sampled call."""
    models, words, (rec, cand, l, g) = seg_run
    for p, (new_id, s) in enumerate(PROBLEMS):
        below, above, low, high = models[s]
        D = len(low)
        z64 = cand[p].astype(np.float64)
        assert np.all(z64 >= low[None, :]) and np.all(z64 < high[None, :])
        l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
        what = 'problem %d (id %d, D=%d)' % (p, new_id, D)
        R.check_lpdf(l[p], l_ref, 'l ' + what)
        R.check_lpdf(g[p], g_ref, 'g ' + what)
        i = int(rec['global_idx'][p])
        assert rec['l'][p] == l[p][i] and rec['g'][p] == g[p][i]
        assert i == int(np.argmax(l[p] - g[p]))                  # the device's own scores: np.argmax order exactly
        _check_winner(rec[p], cand[p], l_ref, g_ref, D, what)


def _candidates(below, low, high, psig, seed, n_far=32):
    """C f32 candidates as tests/test_gpu_joint.py builds them: one eighth around
    the below mixture's components, the rest over the box / the prior, the last
    n_far 40 prior sigmas beyond every observation in the first unbounded
    dimension."""
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
    z[-n_far:, free[0]] = mu[:, free[0]].max() + 40.0 * psig[free[0]] + rs.uniform(0, 1, n_far)
    z = z.astype(np.float32)
    lo32 = np.where(bounded, low, -np.inf).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, high, np.inf).astype(np.float32), np.float32(-np.inf))
    return np.clip(z, lo32[None, :], hi32[None, :])


def test_injected_candidates_of_one_segment(engine):
    """The D = 5 segment scores given candidates (far ones included: no -inf);
    its two problems get the same l and g, equal to the single run's bytes."""
    models, words = _segments()
    below, above, low, high = models[2]
    psig = R.seeded_case(5, 300, 205)[5]
    inj = _candidates(below, low, high, psig, 5)
    z64 = inj.astype(np.float64)
    l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
    rec, cand, l, g = engine.run_joint_segments(models, words, [2, 2], [9, 12], C, SEED,
                                                inject=[None, None, inj, None, None], return_cand=True, want_lg=True)
    assert np.all(np.isfinite(l)) and np.all(np.isfinite(g))
    srec, scand, sl, sg = _single(engine, models[2], words[2], 9, inject=inj)
    for p in range(2):
        assert cand[p].tobytes() == inj.tobytes() == scand[0].tobytes()
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes()
        assert rec[p:p + 1].tobytes() == srec.tobytes()
        R.check_lpdf(l[p], l_ref, 'injected l')
        R.check_lpdf(g[p], g_ref, 'injected g')
        _check_winner(rec[p], inj, l_ref, g_ref, 5, 'injected problem %d' % p)
    with pytest.raises(ValueError, match='inject lacks'):
        engine.run_joint_segments(models, words, [2, 1], [9, 12], C, SEED, inject=[None, None, inj, None, None])


def test_unseen_branch_scores_exactly_zero(engine):
    """A branch nobody observed: both sides are the prior row alone, with
    identical device rows, so l - g is exactly 0 for every candidate and the
    winner is candidate 0, a vector inside the bounds."""
    low, high = np.array([1.0, -np.inf, -3.0]), np.array([20.0, np.inf, 3.0])
    side = (np.array([1.0]), np.array([[10.5, 0.0, 0.0]]), np.array([[19.0, 1.0, 6.0]]))
    rec, cand, l, g = engine.run_joint_segments([(side, side, low, high)], [0xFFFFFFFE - 4], [0, 0], [3, 11], C, SEED,
                                                return_cand=True, want_lg=True)
    for p in range(2):
        assert l[p].tobytes() == g[p].tobytes() and np.all(np.isfinite(l[p]))
        assert int(rec['global_idx'][p]) == 0
        z = rec['z'][p, :3]
        np.testing.assert_array_equal(z, cand[p][0].astype(np.float64))
        assert np.all(z >= low) and np.all(z < high)
        zz = cand[p].astype(np.float64)
        assert np.all(zz >= low[None, :]) and np.all(zz < high[None, :])
    assert cand[0].tobytes() != cand[1].tobytes()


# ------------------------------------------------------------ the public path
def _space():
    from hyperopt_amd import hp
    return {'clf': hp.choice('clf', [{'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
                                     {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.uniform('rf_split', 0, 1)}]),
            'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5)}


def _loss(v, rf_offset=0.3):
    """Couples the labels inside each branch (and x with y).  ``rf_offset``
    decides which branch the best trials take (checked on the CPU for the 80
    trials of _public_case): 0.3 the rf branch, 1.5 the svm branch, 0.6 two rf
    trials and one svm trial."""
    if 'svm_C' in v:
        inner = (np.log(v['svm_C']) + np.log(v['svm_gamma']) + 2.0) ** 2 + 0.05 * np.log(v['svm_C']) ** 2
    else:
        inner = (v['rf_depth'] * v['rf_split'] - 4.0) ** 2 / 16.0 + rf_offset
    return float(inner + 0.1 * (v['x'] * v['y'] - 2.0) ** 2)


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


@functools.lru_cache(maxsize=None)
def _public_case(rf_offset):
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, _space())
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(80):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok',
                             'loss': _loss({k: float(v) for k, v in _vals(docs[0]).items()}, rf_offset)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    best = sorted(trials.trials, key=lambda d: d['result']['loss'])[:3]
    return domain, trials, [int(_vals(d)['clf']) for d in best]


# label: (fit coordinate, prior mu, prior sigma, low, high)
SPEC = {'svm_C': (np.log, 0.0, 6.0, -3.0, 3.0), 'svm_gamma': (np.log, -3.0, 6.0, -6.0, 0.0),
        'rf_depth': (lambda v: v, 10.5, 19.0, 1.0, 20.0), 'rf_split': (lambda v: v, 0.5, 1.0, 0.0, 1.0),
        'x': (lambda v: v, 0.0, 10.0, -5.0, 5.0), 'y': (lambda v: v, 0.0, 10.0, -5.0, 5.0)}


def _model_from_trials(trials, labels):
    """The float64 joint model of a group from the Trials alone: the gamma = 0.25
    split over ALL trials (the ceil(0.25 sqrt(n)) best losses, at most 25), then
    per side the restated mixture over the trials that observed the group, in
    tid order."""
    docs = sorted(trials.trials, key=lambda d: d['tid'])
    loss = np.array([d['result']['loss'] for d in docs])
    assert len(np.unique(loss)) == len(loss)
    nb = min(int(np.ceil(0.25 * np.sqrt(len(loss)))), 25)
    m = np.zeros(len(loss), dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    obs = np.array([len(d['misc']['vals'][labels[0]]) > 0 for d in docs])
    X = np.stack([SPEC[k][0](np.array([float(d['misc']['vals'][k][0]) for d, o in zip(docs, obs) if o]))
                  for k in labels], axis=1)
    m = m[obs]
    pmu, psig = np.array([SPEC[k][1] for k in labels]), np.array([SPEC[k][2] for k in labels])
    low, high = np.array([SPEC[k][3] for k in labels]), np.array([SPEC[k][4] for k in labels])
    return R.ref_side(X[m], pmu, psig), R.ref_side(X[~m], pmu, psig), low, high


def _check_batch(domain, trials, ids, Cn, seed):
    """Every check of the public path on one batched suggest; returns the
    branches the ids took."""
    from hyperopt_amd import history, tpe
    from hyperopt_amd.engine import get_engine
    table = domain.table
    assert table.labels == ['clf', 'rf_depth', 'rf_split', 'svm_C', 'svm_gamma', 'x', 'y']
    kw = dict(n_EI_candidates=Cn, joint=True, joint_branches=True)
    plain = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=Cn)]
    docs = tpe.suggest(ids, domain, trials, seed, **kw)
    root = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=Cn, joint=True)]
    got = [_vals(d) for d in docs]
    branch = {0: ['svm_C', 'svm_gamma'], 1: ['rf_depth', 'rf_split']}
    models = {c: _model_from_trials(trials, labels) for c, labels in branch.items()}
    words = {0: 0xFFFFFFFE - 3, 1: 0xFFFFFFFE - 1}
    for j, new_id in enumerate(ids):
        trials.assert_valid_trial(docs[j])
        v, c = got[j], int(plain[j]['clf'])
        # the gate: the plain suggest's bytes; only the taken branch's labels are present
        assert type(v['clf']) is type(plain[j]['clf']) and v['clf'] == plain[j]['clf']
        assert set(v) == set(plain[j]) == {'clf', 'x', 'y'} | set(branch[c])
        # the root pair: what joint=True alone returns
        assert root[j]['clf'] == plain[j]['clf'] and set(root[j]) == set(v)
        for k in ('x', 'y'):
            assert type(v[k]) is np.float64 and v[k] == root[j][k], (j, k)
        for k in branch[c]:                      # without joint_branches a conditional label stays univariate
            assert root[j][k] == plain[j][k], (j, k)
        # the joined pair: the winner of run_joint over the branch's observers with the group's stream word
        below, above, low, high = models[c]
        rec = get_engine().run_joint(below, above, low, high, [new_id], Cn, seed, None, False, False,
                                     stream_word=words[c])
        z = rec['z'][0, :2]
        want = np.exp(z) if c == 0 else z
        for d, k in enumerate(branch[c]):
            assert type(v[k]) is np.float64 and v[k] == want[d], (j, k, v[k], want[d])
        assert low[0] <= z[0] < high[0] and low[1] <= z[1] < high[1]
    assert any(got[j][k] != plain[j][k] for j in range(len(ids)) for k in branch[int(plain[j]['clf'])])

    # batched ids equal single-id calls
    for j, new_id in enumerate(ids):
        assert _vals(tpe.suggest([new_id], domain, trials, seed, **kw)[0]) == got[j], j
    # the columns form carries the joined labels as active where their branch is taken
    hist = history.extract(domain, trials)
    cc = tpe.suggest_choices(table, hist, ids, seed, columns=True, **kw)
    cc2 = tpe.suggest_choices(table, hist, ids, seed, columns=True, **kw)
    assert cc.values.tobytes() == cc2.values.tobytes()
    for j in range(len(ids)):
        for lab in table.labels:
            i = cc.labels.index(lab)
            assert bool(cc.active[j, i]) == (lab in got[j]), (j, lab)
            if lab in got[j]:
                assert cc.values[j, i] == float(got[j][lab]), (j, lab)
    # a list of conditional labels: only those groups are joined
    some = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=Cn,
                                          joint=['rf_depth', 'rf_split'], joint_branches=True)]
    for j in range(len(ids)):
        c = int(plain[j]['clf'])
        assert some[j] == (plain[j] if c == 0 else dict(plain[j], rf_depth=got[j]['rf_depth'],
                                                        rf_split=got[j]['rf_split'])), j
    return [int(v['clf']) for v in plain]


@pytest.mark.parametrize('rf_offset,best,taken', [(0.3, [1, 1, 1], 1), (1.5, [0, 0, 0], 0)])
def test_public_branch_suggest(rf_offset, best, taken):
    """4096 candidates.  With that many the gate's argmax sees every category,
    so all ids of one history take the branch of its best trials: one history
    per branch."""
    domain, trials, top = _public_case(rf_offset)
    assert top == best
    assert _check_batch(domain, trials, [80, 81, 90, 1000], 4096, 321) == [taken] * 4


def test_public_branch_suggest_routes_each_id():
    """Both branches in ONE batched call.  The gate only varies between ids when
    an id may draw no candidate of the better category, so this batch uses
    n_EI_candidates = 2 on a history whose best trials are two rf and one svm
    (below P(svm) = 0.375: about one id in seven takes svm) and 32 ids."""
    domain, trials, top = _public_case(0.6)
    assert sorted(top) == [0, 1, 1]
    took = _check_batch(domain, trials, list(range(80, 112)), 2, 321)
    assert set(took) == {0, 1}, took


def test_fmin_with_branch_groups():
    from hyperopt_amd import fmin, tpe, Trials
    algo = functools.partial(tpe.suggest, joint=True, joint_branches=True, n_EI_candidates=1024)
    t = Trials()

    def objective(d):
        v = dict(x=d['x'], y=d['y'])
        v.update(dict(svm_C=d['clf']['C'], svm_gamma=d['clf']['gamma']) if 'C' in d['clf'] else
                 dict(rf_depth=d['clf']['depth'], rf_split=d['clf']['split']))
        return _loss(v, 0.9)
    fmin(objective, _space(), algo=algo, max_evals=40, trials=t, rstate=np.random.RandomState(0))
    assert len(t) == 40
    taken = set()
    for doc in t.trials:
        t.assert_valid_trial(doc)
        v = _vals(doc)
        taken.add(int(v['clf']))
        assert set(v) == {'clf', 'x', 'y'} | ({'svm_C', 'svm_gamma'} if int(v['clf']) == 0 else
                                             {'rf_depth', 'rf_split'})
        assert np.isfinite(doc['result']['loss'])
    assert taken == {0, 1}
