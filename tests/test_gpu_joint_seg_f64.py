"""The float64 segmented joint stage (Engine.run_joint_segments(precision='fp64'), joint_precision_branches) against
tests/joint_ref.py at the project's fp64 tolerance, 1e-9 * max(1, |ref|), the winner in that bound's tie set, and
against the solo float64 stage byte for byte."""
import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R
from tests.test_gpu_joint_f64 import MAX_TIES, TOL, _group, engine  # noqa: F401  (engine: the module's fixture)

pytestmark = pytest.mark.gpu

IDS, SEED = [3, 70000, 2 ** 33 + 5], 11


def G(D=4, na=300, nb=25, kind='plain', n_ids=1, word=None):
    """One group of a call.  word None: a case of tests/test_gpu_joint_f64.py (its group seed, ids, call seed and
    stream word), whose pool is known to stay within the tie cap; a branch word: no cap, the solo bytes decide."""
    return dict(D=D, na=na, nb=nb, kind=kind, n_ids=n_ids, word=N.JOINT_STREAM if word is None else word,
                cap=word is None and nb > 0)


SMALL = [G(n_ids=3), G(D=16, na=128), G(D=2, na=15, word=0xFFFFFFFE), G(D=3, nb=0, word=0xFFFFFFFD),
         G(D=5, na=127, nb=1, word=0xFFFFFFFC), G(D=8, n_ids=0)]
CALLS = {2500: [G(D=2), G(D=3, n_ids=3), G(D=5), G(D=16), G(na=14), G(na=15), G(na=16), G(na=126), G(na=127),
                G(na=128, n_ids=3), G(nb=0), G(nb=1), G(kind='off-centre'), G(kind='clustered'),
                G(D=8, word=0xFFFFFFFB), G(D=11), G(D=6, n_ids=0)], 1025: SMALL, 1: SMALL}


def _check_call(engine, specs, C, inject=None):
    """One segmented float64 call over ``specs`` in a shuffled problem order; every problem against the fp32 call's
    candidates, the reference, and the solo float64 run of its group."""
    groups = [_group(s['D'], s['na'], s['nb'], s['kind']) for s in specs]
    models, words = [g[:4] for g in groups], [s['word'] for s in specs]
    probs = [(i, pid) for i, s in enumerate(specs) for pid in IDS[:s['n_ids']]]
    probs = [probs[i] for i in np.random.RandomState(0).permutation(len(probs))]
    args = (models, words, [p[0] for p in probs], [p[1] for p in probs], C, SEED)
    kw = dict(inject=inject, return_cand=True, want_lg=True)
    rec, cand, l, g = engine.run_joint_segments(*args, precision='fp64', **kw)
    cand32 = engine.run_joint_segments(*args, **kw)[1]
    again = engine.run_joint_segments(*args, precision='fp64', **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((rec, l, g), (again[0], again[2], again[3])))
    for i, s in enumerate(specs):
        at = [p for p, (seg, _) in enumerate(probs) if seg == i]
        if not at:
            continue
        solo = engine.run_joint(*models[i], [probs[p][1] for p in at], C, SEED, stream_word=s['word'], precision='fp64',
                                inject=None if inject is None else inject[i], return_cand=True, want_lg=True)
        for j, p in enumerate(at):
            what = 'C %d group %d %r id %d' % (C, i, s, probs[p][1])
            assert cand[p].dtype == np.float32 and cand[p].tobytes() == cand32[p].tobytes(), what
            (below, above, low, high), D, z64 = models[i], s['D'], cand[p].astype(np.float64)
            l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
            R.check_lpdf(l[p], l_ref, what + ' l', tol=TOL)
            R.check_lpdf(g[p], g_ref, what + ' g', tol=TOL)
            ties, idx = R.tie_set(l_ref, g_ref, tol=TOL)[0], int(rec['global_idx'][p])
            assert (len(ties) <= MAX_TIES or not s['cap']) and idx in ties, (what, idx, ties[:8])
            assert idx == int(np.argmax(l[p] - g[p]))
            assert rec['l'][p].tobytes() == l[p, idx].tobytes() and rec['g'][p].tobytes() == g[p, idx].tobytes()
            assert (rec['z'][p, :D] == z64[idx]).all() and (rec['z'][p, D:] == 0).all()
            for got, want in zip((rec[p], cand[p], l[p], g[p]), (solo[0][j], solo[1][j], solo[2][j], solo[3][j])):
                assert got.tobytes() == want.tobytes(), what     # the defining property
    return l, g


@pytest.mark.parametrize('C', sorted(CALLS))
def test_drawn_candidates_of_many_groups_in_one_call(engine, C):
    _check_call(engine, CALLS[C], C)


def test_injected_points(engine):
    """tests/test_gpu_joint_f64.py's points (D = 3; 22 to 24: 30 prior sigmas out, every block votes to skip), two ids."""
    below, above, low, high, pmu, psig = _group(3, 300, 25)
    on = above[1][(7 * np.arange(20) + 1) % len(above[1])]
    edge = np.array([[-10.0, 1.0, -10.0], [np.nextafter(np.float32(10.0), np.float32(0.0)), 1.0, -10.0]])
    far = np.array([[0.0, 1.0 + 120.0, 0.0], [0.0, 1.0 - 120.0, 0.0], [9.5, 1.0 - 120.0, -9.5]])
    pts = np.vstack([on, edge, far, below[1][1:4]]).astype(np.float32)
    assert len(np.unique(pts, axis=0)) == len(pts) == 28
    l, g = _check_call(engine, [G(D=3, n_ids=2), G(D=2, n_ids=0)], len(pts), inject=[pts, None])
    assert np.isfinite(l).all() and np.isfinite(g).all() and l[:, 22:25].max() < -400


def test_public_suggest_with_float64_branch_groups():
    from hyperopt_amd import base, history, hp, joint as J, rand, tpe
    from hyperopt_amd.engine import get_engine
    u, n = hp.uniform, hp.normal
    space = {'x': u('x', -5, 5), 'y': n('y', 0, 2), 'c': hp.choice('c', [0, 1, 2]),
             'g1': hp.choice('g1', [{'a1': u('a1', 0, 1), 'a2': hp.loguniform('a2', -3, 1)},
                                    {'b1': n('b1', 0, 1), 'b2': u('b2', -1, 1), 'b3': hp.lognormal('b3', 0, 1)}]),
             'g2': hp.choice('g2', [dict(('d%d' % i, u('d%d' % i, -1, 1)) for i in range(5)),
                                    {'e1': n('e1', 1, 2), 'e2': u('e2', 0, 4)}])}
    domain, trials, rs = base.Domain(lambda d: 0.0, space), base.Trials(), np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items() if len(x)}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': sum((x - 0.3) ** 2 for x in v.values())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    ids, C, seed = [60, 61, 62], 4096, 321
    kw = dict(n_EI_candidates=C, joint=True, joint_branches=True)

    def vals(docs):
        return [dict((k, v[0]) for k, v in d['misc']['vals'].items() if len(v)) for d in docs]
    f64 = dict(kw, joint_precision='fp64', joint_precision_branches=True)
    got, f32 = vals(tpe.suggest(ids, domain, trials, seed, **f64)), vals(tpe.suggest(ids, domain, trials, seed, **kw))
    assert vals(tpe.suggest(ids, domain, trials, seed, **f64)) == got
    hist, engine = history.extract(domain, trials), get_engine()
    below_tids = history.split_below(hist, 0.25)
    root, branch_groups = tpe._joint_plan(domain.table, True, 'philox', 'fp32', (None,) * 4, False, False, False, True,
                                          False)
    assert sorted(len(rows) for rows in branch_groups) == [2, 2, 3, 5] and [r.label for r in root] == ['x', 'y']
    stages = [(root, J.fit_model(root, hist, below_tids, 1.0, tpe.DEFAULT_LF), None)] + [
        tpe._fit_branch_model(rows, hist, below_tids, 1.0) + (J.branch_stream_word(rows),) for rows in branch_groups]
    taken = 0
    for j, (a, b) in enumerate(zip(got, f32)):
        assert sorted(a) == sorted(b)
        for k in ('c', 'g1', 'g2'):
            assert type(a[k]) is type(b[k]) and a[k] == b[k], (j, k)
        for rows, model, word in stages:
            if rows[0].label not in a:
                continue
            taken += word is not None
            cand = engine.run_joint(model.below, model.above, model.low, model.high, [ids[j]], C, seed,
                                    stream_word=word, return_cand=True)[1][0]
            z64 = cand.astype(np.float64)
            ties = R.tie_set(R.ref_lpdf(z64, model.below[:3], model.low, model.high),
                             R.ref_lpdf(z64, model.above[:3], model.low, model.high), tol=TOL)[0]
            want = model.values(z64[ties])
            assert len(ties) <= MAX_TIES
            assert any(all(a[r.label] == want[i, d] for d, r in enumerate(rows)) for i in range(len(ties))), (j, rows)
    assert taken == 2 * len(ids)
