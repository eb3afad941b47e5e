"""The wide float64 joint stage (Engine.run_joint_wide(precision='fp64'), joint_precision_wide=True) against
tests/joint_ref.py at the project's fp64 tolerance (tests/test_gpu_kernels.py): 1e-9 * max(1, |ref|), the winner in
that bound's tie set; its candidates are the fp32 wide stage's bytes."""
import numpy as np
import pytest

from tests import joint_ref as R
from tests.test_gpu_joint_f64 import MAX_TIES, TOL, _group

pytestmark = pytest.mark.gpu

T = 128                            # kWF64Tile (csrc/tpe_joint.hip): the largest component tile, DP = 20 and 24
BASE = dict(D=20, na=300, nb=25, C=600, n_ids=3)
CASES = ([dict(BASE)] + [dict(BASE, D=D) for D in (17, 21, 24, 25, 32, 33, 48, 49, 64)]
         + [dict(BASE, na=na) for na in (0, 15, 16, 17, T - 1, T, T + 1)] + [dict(BASE, nb=nb) for nb in (0, 1)]
         + [dict(BASE, C=C) for C in (1, 255, 256, 257, 513)]
         + [dict(BASE, n_ids=1), dict(BASE, D=64, na=T + 1, C=513), dict(BASE, D=33, kind='off-centre'),
            dict(BASE, D=64, kind='clustered')])


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _check(engine, below, above, low, high, ids, C, what, inject=None, cap=True):
    kw = dict(seed=11, inject=inject, return_cand=True, want_lg=True)
    rec, cand, l, g = engine.run_joint_wide(below, above, low, high, ids, C, precision='fp64', **kw)
    cand32 = engine.run_joint_wide(below, above, low, high, ids, C, **kw)[1]
    assert cand.dtype == np.float32 and cand.tobytes() == cand32.tobytes(), what      # (a) the fp32 wide stage's pool
    D = len(low)
    for j in range(len(ids)):
        z64 = cand[j].astype(np.float64)
        l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
        R.check_lpdf(l[j], l_ref, '%s l id %d' % (what, j), tol=TOL)                  # (b)
        R.check_lpdf(g[j], g_ref, '%s g id %d' % (what, j), tol=TOL)
        ties = R.tie_set(l_ref, g_ref, tol=TOL)[0]                                    # (c)
        idx = int(rec['global_idx'][j])
        assert (len(ties) <= MAX_TIES or not cap) and idx in ties, (what, idx, ties[:8])
        assert idx == int(np.argmax(l[j] - g[j]))                                     # (d)
        assert rec['l'][j].tobytes() == l[j, idx].tobytes() and rec['g'][j].tobytes() == g[j, idx].tobytes()   # (e)
        np.testing.assert_array_equal(rec['z'][j, :D], z64[idx])
        assert (rec['z'][j, D:] == 0).all()
    return l, g


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join('%s%s' % kv for kv in sorted(c.items())))
def test_drawn_candidates_scored_in_float64(engine, case):
    below, above, low, high, _, _ = _group(case['D'], case['na'], case['nb'], case.get('kind', 'plain'))
    _check(engine, below, above, low, high, [3, 70000, 2 ** 33 + 5][:case['n_ids']], case['C'], str(case),
           cap=case['nb'] > 0)      # (nb = 0: without the tie cap, for the reason tests/test_gpu_joint_f64.py gives)


def test_injected_points(engine):
    """D = 33 (odd dimensions unbounded, prior N(1, 4^2)): on components' centres (every position of a 16 x 16 block and
    beyond), on low and just under high, and 120 prior sigmas out in dimension 1, where every block may vote to skip."""
    below, above, low, high, pmu, psig = _group(33, 300, 25)
    mu = above[1]
    on = mu[(7 * np.arange(20) + 1) % len(mu)]
    edge, far = np.tile(pmu, (2, 1)), np.tile(pmu, (3, 1))
    edge[:, 0], edge[1, 2] = -10.0, np.nextafter(np.float32(10.0), np.float32(0.0))
    far[:, 1], far[2, 0], far[2, 32] = 1.0 + 4.0 * np.array([120.0, -120.0, -120.0]), 9.5, -9.5
    pts = np.vstack([on, edge, far, below[1][1:4]]).astype(np.float32)
    assert len(np.unique(pts, axis=0)) == len(pts) == 28
    z64 = pts.astype(np.float64)                                  # the cap holds for the reference alone
    assert len(R.tie_set(R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high), tol=TOL)[0]) <= MAX_TIES
    l, g = _check(engine, below, above, low, high, [9], len(pts), 'inject', inject=pts)
    assert np.isfinite(l).all() and np.isfinite(g).all() and l[0, 22:25].max() < -400


def test_public_suggest_with_wide_float64_root_stage():
    from hyperopt_amd import base, history, hp, joint as J, rand, tpe
    from hyperopt_amd.engine import get_engine
    space = dict([('x%02d' % i, hp.uniform('x%02d' % i, -5, 5) if i % 2 == 0 else hp.normal('x%02d' % i, 0, 2))
                  for i in range(20)], c=hp.choice('c', [0, 1, 2]))
    domain, trials, rs = base.Domain(lambda d: 0.0, space), base.Trials(), np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items()}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': sum(v[k] ** 2 for k in v if k != 'c') + 0.1 * v['c']}
        trials.insert_trial_docs(docs)
    trials.refresh()
    ids, C, seed = [60, 61, 62], 4096, 321
    kw = dict(n_EI_candidates=C, joint=True, joint_wide=True)
    wide = dict(kw, joint_precision='fp64', joint_precision_wide=True)
    first = tpe.suggest(ids, domain, trials, seed, **wide)
    vals = [dict((k, v[0]) for k, v in d['misc']['vals'].items()) for d in first]
    again, f32 = tpe.suggest(ids, domain, trials, seed, **wide), tpe.suggest(ids, domain, trials, seed, **kw)
    hist = history.extract(domain, trials)
    rows = [r for r in domain.table.rows if r.label != 'c']
    model = J.fit_model(rows, hist, history.split_below(hist, 0.25), 1.0, tpe.DEFAULT_LF)
    cand = get_engine().run_joint_wide(model.below, model.above, model.low, model.high, ids, C, seed,
                                       return_cand=True)[1]
    for j, got in enumerate(vals):
        assert type(got['c']) is type(f32[j]['misc']['vals']['c'][0]) and got['c'] == f32[j]['misc']['vals']['c'][0]
        assert dict((k, v[0]) for k, v in again[j]['misc']['vals'].items()) == got
        z64 = cand[j].astype(np.float64)
        ties = R.tie_set(R.ref_lpdf(z64, model.below[:3], model.low, model.high),
                         R.ref_lpdf(z64, model.above[:3], model.low, model.high), tol=TOL)[0]
        want = model.values(z64[ties])
        assert len(ties) <= MAX_TIES
        assert any(all(got[r.label] == want[i, d] for d, r in enumerate(rows)) for i in range(len(ties))), (j, got)
