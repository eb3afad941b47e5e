"""GPU tests of the wide segmented joint stage (tpe_joint_wide_seg_run through
Engine.run_joint_wide_segments) and of tpe.suggest(..., joint=True,
joint_wide=True, joint_branches=True, joint_branches_wide=True) on a tree space
whose branch holds 20 continuous labels (DESIGN.md "Wide branch groups").

The stage's defining property is tested as bytes: problem (id, segment) equals
a tpe_joint_wide_run over that segment alone with its stream word and ids =
[id].  Against the float64 model restated in numpy (tests/joint_ref.py) the
tolerances are the project's (tests/test_gpu_joint.py): l and g within 1e-5 *
max(1, |ref|), the winner inside the tie set, and at most MAX_TIES members in it.
"""
import functools

import numpy as np
import pytest

from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # a plateau of near-equal scores must not hide a wrong winner
C = 2049              # 9 sampler blocks, the last ragged; 5 chunks at R = 2, 9 at R = 1
SEED = 17

# (D, n, n_below): DP 20 with three padded dimensions and K_above = 147 (wraps the 128-row tile); DP 20 with the
# prior row alone above and K_below = 41; DP 24 exactly; DP 48 (R = 1) with K_above = 98 (wraps the 80-row tile);
# DP 64 with K_above = 68 (wraps the 64-row tile); one segment no problem names
SEGMENTS = [(17, 150, None), (20, 40, 40), (24, 60, None), (33, 100, None), (64, 70, None), (21, 50, None)]


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


@functools.lru_cache(maxsize=None)
def _case(s):
    D, n, nb = SEGMENTS[s]
    return R.seeded_case(D, n, 1000 * D + n, n_below=nb)


def _segments():
    cases = [_case(s) for s in range(len(SEGMENTS))]
    assert [len(c[1][0]) for c in cases[:5]] == [147, 1, 59, 98, 68] and len(cases[1][0][0]) == 41
    return [c[:4] for c in cases], [0xFFFFFFFE - 3 * s for s in range(len(cases))]


# (new id, segment): non-contiguous ids, one above 2^20, id 9 in two segments, two ids in segment 0 (R = 2) and in
# segment 3 (R = 1), not sorted by segment
PROBLEMS = [(9, 3), (5, 0), (40, 4), (9, 1), (12, 3), (2 ** 20 + 3, 0), (7, 2), (31, 4)]


def _single(engine, model, word, new_id, inject=None):
    """tpe_joint_wide_run over one segment alone with its stream word."""
    below, above, low, high = model
    return engine.run_joint_wide(below, above, low, high, [new_id], C, SEED, inject, return_cand=True, want_lg=True,
                                 stream_word=word)


@pytest.fixture(scope='module')
def seg_run(engine):
    """The segmented call over PROBLEMS (computed once, shared, not modified)."""
    models, words = _segments()
    ids, segs = [p[0] for p in PROBLEMS], [p[1] for p in PROBLEMS]
    out = engine.run_joint_wide_segments(models, words, segs, ids, C, SEED, return_cand=True, want_lg=True)
    return models, words, out


def test_segmented_run_equals_single_runs_bytes(engine, seg_run):
    from hyperopt_amd import _native as N
    models, words, (rec, cand, l, g) = seg_run
    P = len(PROBLEMS)
    assert rec.shape == (P,) and rec.dtype == N.JOINT_WIDE_RECORD_DTYPE
    assert l.shape == g.shape == (P, C) and len(cand) == P
    for p, (new_id, s) in enumerate(PROBLEMS):
        D = len(models[s][2])
        assert cand[p].shape == (C, D) and cand[p].dtype == np.float32
        srec, scand, sl, sg = _single(engine, models[s], words[s], new_id)
        assert rec[p:p + 1].tobytes() == srec.tobytes(), (p, rec[p], srec)
        assert cand[p].tobytes() == scand[0].tobytes(), p
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes(), p
        i = int(rec['global_idx'][p])
        assert 0 <= i < C and i == int(np.argmax(l[p] - g[p]))
        np.testing.assert_array_equal(rec['z'][p, :D], cand[p][i].astype(np.float64))
        assert (rec['z'][p, D:] == 0).all()
        low, high = models[s][2], models[s][3]
        z64 = cand[p].astype(np.float64)
        assert np.all(z64 >= low[None, :]) and np.all(z64 < high[None, :])
    # id 9 draws independently in its two segments (D = 33 and D = 20); two ids of one segment differ
    assert cand[0][:, :20].tobytes() != cand[3].tobytes()
    assert cand[0].tobytes() != cand[4].tobytes() and cand[1].tobytes() != cand[5].tobytes()
    # the stream word matters: the root group's word gives other candidates
    other = engine.run_joint_wide(*models[1], [9], C, SEED, return_cand=True)
    assert other[1][0].tobytes() != cand[3].tobytes()


def test_twice_the_same_bytes_and_any_problem_order(engine, seg_run):
    models, words, first = seg_run
    ids, segs = [p[0] for p in PROBLEMS], [p[1] for p in PROBLEMS]
    again = engine.run_joint_wide_segments(models, words, segs, ids, C, SEED, return_cand=True, want_lg=True)
    assert again[0].tobytes() == first[0].tobytes()
    assert again[2].tobytes() == first[2].tobytes() and again[3].tobytes() == first[3].tobytes()
    for x, y in zip(again[1], first[1]):
        assert x.tobytes() == y.tobytes()
    perm = [6, 2, 7, 4, 0, 5, 1, 3]
    rec, cand, l, g = engine.run_joint_wide_segments(models, words, [segs[p] for p in perm], [ids[p] for p in perm], C,
                                                     SEED, return_cand=True, want_lg=True)
    for q, p in enumerate(perm):
        assert rec[q:q + 1].tobytes() == first[0][p:p + 1].tobytes(), (q, p)
        assert cand[q].tobytes() == first[1][p].tobytes()
        assert l[q].tobytes() == first[2][p].tobytes() and g[q].tobytes() == first[3][p].tobytes()
    # records alone: the same winners without the optional outputs
    assert engine.run_joint_wide_segments(models, words, segs, ids, C, SEED).tobytes() == first[0].tobytes()


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


def _candidates(below, low, high, psig, seed, n_far=32):
    """C f32 candidates as tests/test_gpu_joint_branch.py builds them: one eighth
    around the below mixture's components, the rest over the box / the prior,
    the last n_far 40 prior sigmas beyond every observation in the first
    unbounded dimension."""
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


def test_injected_candidates_of_every_class(engine):
    """One problem pair per DP class (segments 0 to 4) scores given candidates
    (far ones included: no -inf) in ONE call: cand is the injected bytes, l, g
    and the record are the solo run's bytes and agree with the float64 model.
    (The float64 reference gives a tie set of 1 for each of these inputs.)"""
    models, words = _segments()
    inj = [_candidates(_case(s)[0], _case(s)[2], _case(s)[3], _case(s)[5], SEGMENTS[s][0]) for s in range(5)] + [None]
    segs, ids = [0, 3, 1, 4, 2, 2, 4, 0, 3, 1], [9, 12, 9, 40, 7, 8, 31, 5, 9, 2 ** 20 + 3]
    rec, cand, l, g = engine.run_joint_wide_segments(models, words, segs, ids, C, SEED, inject=inj, return_cand=True,
                                                     want_lg=True)
    assert np.all(np.isfinite(l)) and np.all(np.isfinite(g))
    solo, ref = {}, {}
    for p, s in enumerate(segs):
        below, above, low, high = models[s]
        D = len(low)
        if s not in solo:
            solo[s] = _single(engine, models[s], words[s], ids[p], inject=inj[s])
            z64 = inj[s].astype(np.float64)
            ref[s] = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
        srec, scand, sl, sg = solo[s]
        assert cand[p].tobytes() == inj[s].tobytes() == scand[0].tobytes(), p
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes(), p
        assert rec[p:p + 1].tobytes() == srec.tobytes(), p
        R.check_lpdf(l[p], ref[s][0], 'injected l, D = %d' % D)
        R.check_lpdf(g[p], ref[s][1], 'injected g, D = %d' % D)
        _check_winner(rec[p], inj[s], ref[s][0], ref[s][1], D, 'injected problem %d (D = %d)' % (p, D))
    with pytest.raises(ValueError, match='inject lacks'):
        engine.run_joint_wide_segments(models, words, [2, 5], [9, 12], C, SEED, inject=inj)


def test_unseen_wide_branch_scores_exactly_zero(engine):
    """A wide branch nobody observed: both sides are the prior row alone, with
    identical device rows, so l - g is exactly 0 for every candidate and the
    winner is candidate 0, a vector inside the bounds."""
    D = 20
    bounded = np.arange(D) % 2 == 0
    low, high = np.where(bounded, -3.0, -np.inf), np.where(bounded, 3.0, np.inf)
    side = (np.array([1.0]), np.where(bounded, 0.0, 1.0)[None, :], np.where(bounded, 6.0, 4.0)[None, :])
    rec, cand, l, g = engine.run_joint_wide_segments([(side, side, low, high)], [0xFFFFFFFE - 4], [0, 0], [3, 11], C,
                                                     SEED, return_cand=True, want_lg=True)
    for p in range(2):
        assert l[p].tobytes() == g[p].tobytes() and np.all(np.isfinite(l[p]))
        assert int(rec['global_idx'][p]) == 0
        z = rec['z'][p, :D]
        np.testing.assert_array_equal(z, cand[p][0].astype(np.float64))
        assert np.all(z >= low) and np.all(z < high)
        zz = cand[p].astype(np.float64)
        assert np.all(zz >= low[None, :]) and np.all(zz < high[None, :])
    assert cand[0].tobytes() != cand[1].tobytes()


# ------------------------------------------------------------ the public path
WIDE = ['m%02d' % i for i in range(20)]         # the mlp branch: 20 continuous knobs, uniform and loguniform
KW = dict(n_EI_candidates=C, joint=True, joint_wide=True, joint_branches=True, joint_branches_wide=True)


def _space():
    from hyperopt_amd import hp
    mlp = {k: (hp.uniform(k, -2, 2) if i % 2 == 0 else hp.loguniform(k, -3, 1)) for i, k in enumerate(WIDE)}
    return {'arch': hp.choice('arch', [mlp, {'a': hp.uniform('s_a', 0, 1), 'b': hp.loguniform('s_b', -4, 0)}]),
            'x': hp.uniform('x', -5, 5)}


def _loss(v, small_offset):
    """Couples the labels inside each branch; ``small_offset`` decides which
    branch the best trials take."""
    if 's_a' in v:
        inner = (v['s_a'] + np.log(v['s_b']) / 4.0) ** 2 + small_offset
    else:
        u = np.array([v[k] if i % 2 == 0 else np.log(v[k]) + 1.0 for i, k in enumerate(WIDE)])
        inner = float(np.mean((u[:-1] + u[1:]) ** 2)) / 4.0
    return float(inner + 0.01 * v['x'] ** 2)


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


@functools.lru_cache(maxsize=None)
def _public_case(small_offset):
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, _space())
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok',
                             'loss': _loss({k: float(v) for k, v in _vals(docs[0]).items()}, small_offset)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    best = sorted(trials.trials, key=lambda d: d['result']['loss'])[:2]
    return domain, trials, [int(_vals(d)['arch']) for d in best]


def _wide_group(domain, trials):
    """(the wide branch group's rows, its model as the suggest fits it, its stream word)."""
    from hyperopt_amd import history, joint as J, tpe
    root, groups = tpe._joint_plan(domain.table, True, 'philox', 'fp32', (None,) * 4, wide=True,
                                   branches=tpe._branch_mode(True, True, True))
    assert root is None and [[r.label for r in g] for g in groups] == [WIDE, ['s_a', 's_b']]
    hist = history.extract(domain, trials)
    rows, model = tpe._fit_branch_model(groups[0], hist, history.split_below(hist, 0.25), 1.0)
    return rows, model, J.branch_stream_word(rows)


@pytest.mark.parametrize('small_offset,taken', [(2.0, 0), (-1.0, 1)])
def test_public_wide_branch_suggest(engine, small_offset, taken):
    """With 2049 candidates the gate's argmax sees both categories, so all ids
    of one history take the branch of its best trials: one history per branch."""
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    domain, trials, top = _public_case(small_offset)
    assert top == [taken, taken]
    ids, seed = [60, 61, 70, 2 ** 20 + 1], 321
    docs = tpe.suggest(ids, domain, trials, seed, **KW)
    got = [_vals(d) for d in docs]
    # without the keyword: the 20-label branch left out of the joined labels
    base = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=['s_a', 's_b'],
                                          joint_branches=True)]
    plain = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C)]
    rows, model, word = _wide_group(domain, trials)
    assert [r.label for r in rows] == WIDE
    for j, new_id in enumerate(ids):
        trials.assert_valid_trial(docs[j])
        v = got[j]
        assert int(v['arch']) == taken and set(v) == set(base[j]) == {'arch', 'x'} | set(WIDE if taken == 0 else
                                                                                        ['s_a', 's_b'])
        # the gate and the univariate label: the bytes of the call without the keyword
        for k in ('arch', 'x'):
            assert type(v[k]) is type(base[j][k]) and v[k] == base[j][k] == plain[j][k], (j, k)
        if taken == 1:                               # the 2-label branch: its plan, its stage and its bytes
            assert v['s_a'] == base[j]['s_a'] and v['s_b'] == base[j]['s_b']
            continue
        rec = get_engine().run_joint_wide(model.below, model.above, model.low, model.high, [new_id], C, seed,
                                          stream_word=word)
        want = model.values(rec['z'][:, :20])[0]
        for d, k in enumerate(WIDE):
            assert type(v[k]) is np.float64 and v[k] == want[d], (j, k, v[k], want[d])
            assert (-2 <= v[k] < 2) if d % 2 == 0 else (np.exp(-3) <= v[k] <= np.exp(1))
    if taken == 0:
        assert any(got[j][k] != plain[j][k] for j in range(len(ids)) for k in WIDE)
    # batched ids equal single-id calls
    for j in (0, 3):
        assert _vals(tpe.suggest([ids[j]], domain, trials, seed, **KW)[0]) == got[j], j


def _narrow_space():
    from hyperopt_amd import hp
    return {'clf': hp.choice('clf', [{'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
                                     {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.uniform('rf_split', 0, 1)}]),
            'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5)}


def test_keyword_changes_nothing_without_a_wide_branch():
    """Branch groups of at most 16 labels: the documents with and without the keyword are equal."""
    from hyperopt_amd import base, rand, tpe
    domain = base.Domain(lambda d: 0.0, _narrow_space())
    trials = base.Trials()
    rs = np.random.RandomState(3)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    kw = dict(n_EI_candidates=C, joint=True, joint_wide=True, joint_branches=True)
    ids = list(range(40, 56))
    without = [_vals(d) for d in tpe.suggest(ids, domain, trials, 5, **kw)]
    with_kw = [_vals(d) for d in tpe.suggest(ids, domain, trials, 5, joint_branches_wide=True, **kw)]
    assert with_kw == without
    assert len(set(int(v['clf']) for v in without)) >= 1


def test_report_of_a_wide_branch_group(engine):
    """joint_candidate_report returns the wide branch group: entry 0 is the
    vector the suggest joins, and n_top, the scores and the stats are those of
    the solo run's l and g."""
    from hyperopt_amd import tpe
    domain, trials, _ = _public_case(2.0)
    rows, model, word = _wide_group(domain, trials)
    new_id, seed, k = 60, 321, 8
    rep = tpe.joint_candidate_report(new_id, domain, trials, seed, k=k, **KW)
    assert [g.labels for g in rep] == [WIDE, ['s_a', 's_b']]
    assert [g.condition for g in rep] == [('arch', 0), ('arch', 1)]
    gr = rep[0]
    rec, cand, l, g = engine.run_joint_wide(model.below, model.above, model.low, model.high, [new_id], C, seed,
                                            return_cand=True, want_lg=True, stream_word=word)
    score = l[0] - g[0]
    assert gr.n_top == k and gr.vectors.shape == (k, 20)
    order = np.argsort(-score, kind='stable')[:k]
    np.testing.assert_array_equal(gr.top['index'], order)
    assert gr.top['l'].tobytes() == l[0][order].tobytes() and gr.top['g'].tobytes() == g[0][order].tobytes()
    np.testing.assert_array_equal(gr.top['score'], score[order])
    np.testing.assert_array_equal(gr.vectors, model.values(cand[0][order].astype(np.float64)))
    assert int(gr.top['index'][0]) == int(rec['global_idx'][0])
    np.testing.assert_array_equal(gr.vectors[0], model.values(rec['z'][:, :20])[0])
    st = gr.stats
    assert (int(st['n_finite']), int(st['n_nan']), int(st['n_posinf']), int(st['n_neginf'])) == (C, 0, 0, 0)
    assert float(st['min']) == score.min() and float(st['max']) == score.max()
    # the bounds of tests/test_gpu_joint_report.py: mean within 1e-10 mean|s|, m2 1e-9 relative
    assert abs(float(st['mean']) - score.mean()) <= 1e-10 * np.abs(score).mean()
    m2 = float(np.sum((score - score.mean()) ** 2))
    assert abs(float(st['m2']) - m2) <= 1e-9 * m2
    # the suggest joins entry 0
    v = _vals(tpe.suggest([new_id], domain, trials, seed, **KW)[0])
    assert [v[lab] for lab in WIDE] == list(gr.vectors[0])
    # the narrow group beside it: what the report gives without the keyword
    ref = tpe.joint_candidate_report(new_id, domain, trials, seed, k=k, n_EI_candidates=C, joint=['s_a', 's_b'],
                                     joint_branches=True)
    assert rep[1].top.tobytes() == ref[0].top.tobytes() and rep[1].vectors.tobytes() == ref[0].vectors.tobytes()


def test_fmin_with_a_wide_branch():
    from hyperopt_amd import fmin, tpe, Trials
    algo = functools.partial(tpe.suggest, joint=True, joint_wide=True, joint_branches=True, joint_branches_wide=True,
                             n_EI_candidates=C, n_startup_jobs=8)
    t = Trials()

    def objective(d):
        v = dict(x=d['x'])
        v.update(dict(s_a=d['arch']['a'], s_b=d['arch']['b']) if 'a' in d['arch'] else d['arch'])
        return _loss(v, 0.5)
    fmin(objective, _space(), algo=algo, max_evals=20, trials=t, rstate=np.random.RandomState(0))
    assert len(t) == 20
    for doc in t.trials:
        t.assert_valid_trial(doc)
        v = _vals(doc)
        assert set(v) == {'arch', 'x'} | (set(WIDE) if int(v['arch']) == 0 else {'s_a', 's_b'})
        assert np.isfinite(doc['result']['loss'])
