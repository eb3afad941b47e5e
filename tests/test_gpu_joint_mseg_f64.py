"""The float64 mixed segmented joint stage (Engine.run_joint_msegments_f64, joint_precision_branches_mixed=True):
every problem of a call against the fp32 mixed segmented stage's candidates (bytes), tests/joint_quant_ref.py /
joint_ref.py at the project's fp64 tolerance 1e-9 * max(1, |ref|), the winner in that bound's tie set, and the solo
float64 run of its group's kind (candidates and index in bytes, l and g in bytes too: DESIGN.md "Float64 mixed
branch groups")."""
import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R
from tests.test_gpu_joint_f64 import _group as _cont_group
from tests.test_gpu_joint_mq_f64 import CASES, MAX_TIES, TOL, _group, _run, engine  # noqa: F401  (engine: the fixture)

pytestmark = pytest.mark.gpu

IDS, SEED = [3, 70000, 2 ** 33 + 5], 11


def G(Dc=3, us=(4,), Vs=(5,), na=300, nb=25, n_ids=1, word=None):
    """One group of a call; us = Vs = (): a continuous group.  The tie cap goes with a group that repeats a case of
    tests/test_gpu_joint_mq_f64.py (its group seed, ids, call seed and stream word); a branch word or nb = 0: no cap."""
    same = [c for c in CASES if (c['Dc'], c['us'], c['Vs'], c['na'], c['nb']) == (Dc, us, Vs, na, nb)
            and c.get('kind', 'plain') == 'plain']
    return dict(Dc=Dc, us=us, Vs=Vs, na=na, nb=nb, n_ids=n_ids, word=N.JOINT_STREAM if word is None else word,
                cap=bool(same) and word is None and nb > 0)


SHAPES = [G(n_ids=3), G(0, (3,), (4,), word=0xFFFFFFFE), G(0, (2,), (), na=15), G(0, (), (5,), na=127, nb=1),
          G(1, (4,), (), na=16, nb=0), G(2, (), (5,), na=128), G(8, (3,) * 4, (4,) * 4), G(3, (256,), (), word=0xFFFFFFFD),
          G(3, (), (256, 256)), G(3, (), ()), G(16, (), (), na=129), G(2, (4,), (5,), n_ids=0)]
SMALL = [G(n_ids=3), G(0, (2,), (), na=14, word=0xFFFFFFFC), G(2, (), (5,), na=126, nb=0), G(8, (3,) * 4, (4,) * 4, na=16),
         G(16, (), ()), G(3, (), (), n_ids=2), G(0, (), (5,), n_ids=0)]
CALLS = {2500: SHAPES, 1025: SMALL, 1: SMALL}


def _model(s):
    """(the group as its generator returns it, the model tuple run_joint_msegments_f64 takes)"""
    if not s['us'] and not s['Vs']:
        g = _cont_group(s['Dc'], s['na'], s['nb'])
        return g, g[:4]
    g = _group(s['Dc'], s['us'], s['Vs'], s['na'], s['nb'])
    below, above, low, high, ps, sb, sa, edges = g
    return g, (below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges))


def _check_call(engine, specs, C, inject=None):
    """One call over ``specs`` in a shuffled problem order; returns l, g [P, C]."""
    groups, models = zip(*[_model(s) for s in specs])
    words = [s['word'] for s in specs]
    probs = [(i, pid) for i, s in enumerate(specs) for pid in IDS[:s['n_ids']]]
    probs = [probs[i] for i in np.random.RandomState(0).permutation(len(probs))]
    args = (list(models), words, [p[0] for p in probs], [p[1] for p in probs], C, SEED)
    kw = dict(inject=inject, return_cand=True, want_lg=True)
    rec, cand, l, g = engine.run_joint_msegments_f64(*args, **kw)
    cand32 = engine.run_joint_segments(*args, **kw)[1]
    again = engine.run_joint_msegments_f64(*args, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((rec, l, g), (again[0], again[2], again[3])))
    for i, s in enumerate(specs):
        at = [p for p, (seg, _) in enumerate(probs) if seg == i]
        if not at:
            continue
        skw = dict(seed=SEED, stream_word=s['word'], inject=None if inject is None else inject[i], return_cand=True,
                   want_lg=True)
        mixed, D = len(models[i]) == 6, s['Dc'] + len(s['us']) + len(s['Vs'])
        ids = [probs[p][1] for p in at]
        solo = (_run(engine, groups[i], ids, C, 'fp64', **skw) if mixed
                else engine.run_joint(*models[i], ids, C, precision='fp64', **skw))
        for j, p in enumerate(at):
            what = 'C %d group %d %r id %d' % (C, i, s, probs[p][1])
            assert cand[p].dtype == np.float32 and cand[p].tobytes() == cand32[p].tobytes(), what
            z64 = cand[p].astype(np.float64)
            if mixed:
                below, above, low, high, ps, sb, sa, edges = groups[i]
                Dc, Dk = s['Dc'], len(ps)
                z, v, qi = z64[:, :Dc], z64[:, Dc:Dc + Dk].astype(np.int64), z64[:, Dc + Dk:].astype(np.int64)
                l_ref = Q.ref_quant_lpdf(z, v, qi, below, low, high, ps, sb, edges)
                g_ref = Q.ref_quant_lpdf(z, v, qi, above, low, high, ps, sa, edges)
            else:
                below, above, low, high = models[i]
                l_ref, g_ref = R.ref_lpdf(z64, below, low, high), R.ref_lpdf(z64, above, low, high)
            R.check_lpdf(l[p], l_ref, what + ' l', tol=TOL)
            R.check_lpdf(g[p], g_ref, what + ' g', tol=TOL)
            ties, idx = R.tie_set(l_ref, g_ref, tol=TOL)[0], int(rec['global_idx'][p])
            distinct = len(np.unique(cand[p][ties], axis=0))
            assert (distinct <= MAX_TIES or not s['cap']) and idx in ties, (what, idx, ties[:8])
            assert idx == int(np.argmax(l[p] - g[p]))
            assert rec['l'][p].tobytes() == l[p, idx].tobytes() and rec['g'][p].tobytes() == g[p, idx].tobytes()
            assert (rec['z'][p, :D] == z64[idx]).all() and (rec['z'][p, D:] == 0).all()
            for got, want in zip((rec[p], cand[p], l[p], g[p]), (solo[0][j], solo[1][j], solo[2][j], solo[3][j])):
                assert got.tobytes() == want.tobytes(), what     # the defining property
    return l, g


@pytest.mark.parametrize('C', sorted(CALLS))
def test_drawn_candidates_of_many_groups_in_one_call(engine, C):
    _check_call(engine, CALLS[C], C)


def test_far_bins(engine):
    """Bandwidths of 1e-3 on a lattice of 64 values as one segment: most table entries are -inf; l, g stay finite."""
    s = G(2, (4,), (64,), na=40, nb=6, word=0xFFFFFFFB)
    g, model = _model(s)
    narrow = [tuple(x if i != 5 else np.vstack([x[:1], np.full_like(x[1:], 1e-3)]) for i, x in enumerate(side))
              for side in g[:2]]
    g = tuple(narrow) + g[2:]
    model = model[:5] + (Q.quants_of(g[0], g[1], g[7]),)
    rec, cand, l, g64 = engine.run_joint_msegments_f64([model], [s['word']], [0], [7], 1500, SEED, return_cand=True,
                                                       want_lg=True)
    solo = _run(engine, g, [7], 1500, 'fp64', seed=SEED, stream_word=s['word'], return_cand=True, want_lg=True)
    assert np.isfinite(l).all() and np.isfinite(g64).all()
    z64 = cand[0].astype(np.float64)
    z, v, qi = z64[:, :2], z64[:, 2:3].astype(np.int64), z64[:, 3:].astype(np.int64)
    R.check_lpdf(l[0], Q.ref_quant_lpdf(z, v, qi, g[0], g[2], g[3], g[4], g[5], g[7]), 'far bins l', tol=TOL)
    R.check_lpdf(g64[0], Q.ref_quant_lpdf(z, v, qi, g[1], g[2], g[3], g[4], g[6], g[7]), 'far bins g', tol=TOL)
    for got, want in zip((rec[0], cand[0], l[0], g64[0]), (solo[0][0], solo[1][0], solo[2][0], solo[3][0])):
        assert got.tobytes() == want.tobytes()


def test_injected_points(engine):
    """tests/test_gpu_joint_mq_f64.py's points: categories equal to component k's, k over a 16-block and beyond the
    first tile, every value of the lattice; a second group without candidates and without a problem."""
    s = G(3, (4, 3), (5,), n_ids=2)
    above = _model(s)[0][1]
    ks = np.concatenate([np.arange(1, 17), [130, 200]])
    pts = np.concatenate([above[1][ks], above[3][ks], (np.arange(len(ks)) % 5)[:, None]], axis=1).astype(np.float32)
    _check_call(engine, [s, G(2, (4,), (), n_ids=0)], len(pts), inject=[pts, None])


def test_public_suggest_with_float64_mixed_branch_groups():
    """The benchmark tree (rf_n_est x rf_crit, knn_k x knn_p): the keyword's picks are run_joint_msegments_f64's."""
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    from tests.test_gpu_joint_branch_mixed import GROUPS, KW, N_CAND, _public_case, _vals
    domain, trials = _public_case()
    ids = [66, 67, 70, 90, 91, 1000, 1001, 5000]
    f32 = tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND, **KW)
    with pytest.raises(ValueError, match='does not combine with branch groups'):
        tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND, joint_precision='fp64', **KW)
    docs = tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND, joint_precision='fp64',
                       joint_precision_branches=True, joint_precision_branches_mixed=True, **KW)
    hist = history.extract(domain, trials)
    below = history.split_below(hist, tpe._default_gamma)
    fitted = {b: tpe._fit_branch_model([domain.table.by_label[k] for k in labels], hist, below, tpe._default_prior_weight)
              for b, labels in GROUPS.items()}
    took = [int(_vals(d)['model']) for d in docs]
    order = [b for b in (2, 1) if b in took]         # the groups in the order of their first label (knn_k, then rf_crit)
    assert len(order) == 2, took
    probs = [(order.index(b), new_id) for b in order for new_id, t in zip(ids, took) if t == b]
    rec = get_engine().run_joint_msegments_f64([fitted[b][1] for b in order],
                                               [J.branch_stream_word(fitted[b][0]) for b in order],
                                               [p[0] for p in probs], [p[1] for p in probs], N_CAND, 321)
    for j, new_id in enumerate(ids):
        trials.assert_valid_trial(docs[j])
        v, w, joined = _vals(docs[j]), _vals(f32[j]), GROUPS.get(took[j], [])
        assert set(v) == set(w)
        for k in v:                                  # every label outside a group: the fp32 call's bytes
            assert type(v[k]) is type(w[k]) and (k in joined or v[k] == w[k]), (j, k)
        if joined:
            rows, model = fitted[took[j]]
            want = model.values(rec['z'][probs.index((order.index(took[j]), new_id))][None, :len(rows)])[0]
            assert all(float(v[r.label]) == want[d] for d, r in enumerate(rows)), (j, v, want)
