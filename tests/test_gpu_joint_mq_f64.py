"""The float64 mixed joint stage (Engine.run_joint_mixed / run_joint_quant(precision='fp64'),
joint_precision_mixed=True) against tests/joint_mixed_ref.py / joint_quant_ref.py (unfloored logs) at the project's
fp64 tolerance 1e-9 * max(1, |ref|), the winner in that bound's tie set (at most MAX_TIES distinct vectors)."""
import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

TOL, MAX_TIES = 1e-9, 4
BASE = dict(Dc=3, us=(4,), Vs=(5,), na=300, nb=25, C=2500, n_ids=3)
CASES = ([dict(BASE)]
         + [dict(BASE, Dc=Dc) for Dc in (0, 1, 2, 8)] + [dict(BASE, Dc=9, us=(3,) * 7, Vs=()),
                                                         dict(BASE, Dc=8, us=(3,) * 4, Vs=(4,) * 4)]
         + [dict(BASE, us=()), dict(BASE, Vs=()), dict(BASE, Dc=0, Vs=()), dict(BASE, Dc=0, us=())]
         # above components = na + 1 (the prior row): 15, 16, 17 and 127, 128, 129 around the 128-component tile ...
         + [dict(BASE, na=na) for na in (0, 14, 15, 16, 126, 127, 128)]
         + [dict(BASE, Dc=9, Vs=(), na=na) for na in (62, 63, 64)]          # ... 63, 64, 65 around Dc = 9's tile of 64
         + [dict(BASE, nb=nb) for nb in (0, 1)] + [dict(BASE, C=C) for C in (1, 17, 1025)]
         + [dict(BASE, us=(2,)), dict(BASE, us=(256,)), dict(BASE, us=('5p',))]
         + [dict(BASE, Vs=(2,)), dict(BASE, Vs=(256,)), dict(BASE, Vs=(256, 256))]
         + [dict(BASE, Vs=(), kind='off-centre')])


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _group(Dc, us, Vs, na, nb, kind='plain', seed=5):
    """test_gpu_joint_f64._group plus categories and lattice values: (below, above, low, high, ps, sb, sa, edges)."""
    rs = np.random.RandomState(1000 * Dc + na + 7 * nb + seed + 31 * len(us) + 57 * len(Vs))
    bounded = np.arange(Dc) % 2 == 0
    lo, hi, m, s = (1000.0, 1001.0, -500.0, 0.5) if kind == 'off-centre' else (-10.0, 10.0, 1.0, 4.0)
    low, high = np.where(bounded, lo, -np.inf), np.where(bounded, hi, np.inf)
    pmu, psig = np.where(bounded, 0.5 * (lo + hi), m), np.where(bounded, hi - lo, s)
    n = na + nb
    X = np.where(bounded[None, :], rs.uniform(lo, hi, (n, Dc)), rs.normal(m, s, (n, Dc)))
    X = X.astype(np.float32).astype(np.float64)
    ps = [M.prior(u) for u in us]
    XC = (np.stack([rs.choice(len(p), size=n, p=p) for p in ps], axis=1) if ps else np.zeros((n, 0), dtype=np.int64))
    edges = [Q.lattice_of(V) for V in Vs]
    XQ = (np.stack([np.rint(rs.uniform(0.0, V - 1.0, n)) for V in Vs], axis=1) if Vs else np.zeros((n, 0)))
    qpmu, qpsig = np.array([0.5 * (V - 1.0) for V in Vs]), np.array([V - 1.0 for V in Vs])
    sides = []
    for sel in (slice(0, nb), slice(nb, n)):
        w, mu, sigma, xc = M.ref_mixed_side(X[sel], pmu, psig, XC[sel])
        _, qmu, qsig = R.ref_side(XQ[sel], qpmu, qpsig) if Vs else (None, np.zeros((len(w), 0)), np.zeros((len(w), 0)))
        sides.append((w, mu, sigma, xc, qmu, qsig))
    s_below = np.array([M.smoothing(len(p), nb) for p in ps])
    s_above = np.array([M.smoothing(len(p), na) for p in ps])
    return sides[0], sides[1], low, high, ps, s_below, s_above, edges


def _run(engine, g, ids, C, precision, **kw):
    below, above, low, high, ps, sb, sa, edges = g
    cats = M.cats_of(below, above, ps, sb, sa)
    if edges:
        return engine.run_joint_quant(below[:3], above[:3], low, high, cats, Q.quants_of(below, above, edges), ids, C,
                                      precision=precision, **kw)
    return engine.run_joint_mixed(below[:3], above[:3], low, high, cats, ids, C, precision=precision, **kw)


def _check(engine, g, ids, C, what, inject=None, cap=True):
    below, above, low, high, ps, sb, sa, edges = g
    Dc, Dk, Dq = len(low), len(ps), len(edges)
    D = Dc + Dk + Dq
    kw = dict(seed=11, inject=inject, return_cand=True, want_lg=True)
    rec, cand, l, g64 = _run(engine, g, ids, C, 'fp64', **kw)
    cand32 = _run(engine, g, ids, C, 'fp32', **kw)[1]
    assert cand.dtype == np.float32 and cand.tobytes() == cand32.tobytes(), what      # (a) the fp32 stage's pool
    for j in range(len(ids)):
        z64 = cand[j].astype(np.float64)
        z, v, qi = z64[:, :Dc], z64[:, Dc:Dc + Dk].astype(np.int64), z64[:, Dc + Dk:].astype(np.int64)
        l_ref = Q.ref_quant_lpdf(z, v, qi, below, low, high, ps, sb, edges)
        g_ref = Q.ref_quant_lpdf(z, v, qi, above, low, high, ps, sa, edges)
        R.check_lpdf(l[j], l_ref, '%s l id %d' % (what, j), tol=TOL)                  # (b)
        R.check_lpdf(g64[j], g_ref, '%s g id %d' % (what, j), tol=TOL)
        ties, score = R.tie_set(l_ref, g_ref, tol=TOL)                                # (c)
        idx = int(rec['global_idx'][j])
        distinct = len(np.unique(cand[j][ties], axis=0))
        assert (distinct <= MAX_TIES or not cap) and idx in ties, (what, idx, ties[:8])
        assert idx == int(np.argmax(l[j] - g64[j]))                                   # np.argmax order: the lowest index
        assert rec['l'][j].tobytes() == l[j, idx].tobytes() and rec['g'][j].tobytes() == g64[j, idx].tobytes()
        np.testing.assert_array_equal(rec['z'][j, :D], z64[idx])
        assert (rec['z'][j, D:] == 0).all()
    return l, g64


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join('%s%s' % kv for kv in sorted(c.items())))
def test_drawn_candidates_scored_in_float64(engine, case):
    g = _group(case['Dc'], case['us'], case['Vs'], case['na'], case['nb'], case.get('kind', 'plain'))
    _check(engine, g, [3, 70000, 2 ** 33 + 5][:case['n_ids']], case['C'], str(case), cap=case['nb'] > 0)


def test_far_bins_and_float64_table(engine):
    """Bandwidths of 1e-3 on a lattice of 64 values: most masses are exactly 0 (-inf in the table); l, g stay finite."""
    below, above, low, high, ps, sb, sa, edges = _group(2, (4,), (64,), 40, 6)
    narrow = [tuple(x if i != 5 else np.vstack([x[:1], np.full_like(x[1:], 1e-3)]) for i, x in enumerate(side))
              for side in (below, above)]
    g = (narrow[0], narrow[1], low, high, ps, sb, sa, edges)
    l, g64 = _check(engine, g, [7], 1500, 'far bins')
    assert np.isfinite(l).all() and np.isfinite(g64).all()
    out = _run(engine, g, [7], 16, 'fp64', seed=11, return_table=True)
    for got, side in zip(out[-2:], narrow):
        ref = Q.ref_table(side[4][:, 0], side[5][:, 0], edges[0])[1]
        fin = np.isfinite(ref)
        assert got.dtype == np.float64 and (np.isneginf(got) == np.isneginf(ref)).all() and (~fin).sum() > 100
        assert (np.abs(got[fin] - ref[fin]) <= TOL * np.maximum(1.0, np.abs(ref[fin]))).all()


def test_injected_points(engine):
    """Categories equal to component k's, k over a 16-block and beyond the first tile; every value of the lattice."""
    g = _group(3, (4, 3), (5,), 300, 25)
    above = g[1]
    ks = np.concatenate([np.arange(1, 17), [130, 200]])
    pts = np.concatenate([above[1][ks], above[3][ks], (np.arange(len(ks)) % 5)[:, None]], axis=1).astype(np.float32)
    _check(engine, g, [9], len(pts), 'inject', inject=pts, cap=False)


def test_public_suggest_with_float64_mixed_root_stage():
    from hyperopt_amd import base, history, hp, joint as J, rand, tpe
    from hyperopt_amd.engine import get_engine as ge
    space = {'lr': hp.loguniform('lr', -7, 0), 'batch': hp.qloguniform('batch', np.log(16), np.log(512), 16),
             'layers': hp.quniform('layers', 1, 8, 1), 'opt': hp.choice('opt', ['sgd', 'adam', 'rms']),
             'u': hp.uniform('u', 0, 1)}
    domain, trials, rs = base.Domain(lambda d: 0.0, space), base.Trials(), np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items()}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': (np.log(v['lr']) + 3) ** 2 + 0.01 * v['batch'] / 16 + 0.1 * v['opt']
                             + 0.05 * v['layers'] + v['u']}
        trials.insert_trial_docs(docs)
    trials.refresh()
    ids, C, seed = [60, 61, 62], 4096, 321
    joined = ['lr', 'batch', 'layers', 'opt']
    kw = dict(n_EI_candidates=C, joint=joined, joint_discrete=True, joint_quantized=True)
    f64 = dict(kw, joint_precision='fp64', joint_precision_mixed=True)
    vals = [dict((k, v[0]) for k, v in d['misc']['vals'].items()) for d in tpe.suggest(ids, domain, trials, seed, **f64)]
    again = tpe.suggest(ids, domain, trials, seed, **f64)
    f32 = tpe.suggest(ids, domain, trials, seed, **kw)
    hist = history.extract(domain, trials)
    crows, drows, qrows = tpe._joint_kernel_order([r for r in domain.table.rows if r.label in joined])
    group = crows + drows + qrows
    model = J.fit_quant_model(crows, drows, qrows, hist, history.split_below(hist, 0.25), 1.0, tpe.DEFAULT_LF)
    args = (model.below[:3], model.above[:3], model.low, model.high, model.cats(), model.quants(), ids, C, seed)
    cand, l, g = ge().run_joint_quant(*args, return_cand=True, want_lg=True, precision='fp64')[1:]   # (_check (a): the fp32 pool)
    for j, got in enumerate(vals):
        assert got['u'] == f32[j]['misc']['vals']['u'][0]
        assert dict((k, v[0]) for k, v in again[j]['misc']['vals'].items()) == got
        z64 = cand[j].astype(np.float64)
        z, v, qi = z64[:, :1], z64[:, 1:2].astype(np.int64), z64[:, 2:].astype(np.int64)
        edges = [lat[3] for lat in model.lattices]
        lr = Q.ref_quant_lpdf(z, v, qi, model.below, model.low, model.high, model.ps, model.s_below, edges)
        gr = Q.ref_quant_lpdf(z, v, qi, model.above, model.low, model.high, model.ps, model.s_above, edges)
        R.check_lpdf(l[j], lr, 'suggest l', tol=TOL)
        R.check_lpdf(g[j], gr, 'suggest g', tol=TOL)
        ties = R.tie_set(lr, gr, tol=TOL)[0]
        want = model.values(z64[ties])
        assert len(np.unique(cand[j][ties], axis=0)) <= MAX_TIES
        assert any(all(got[r.label] == want[i, d] and type(got[r.label]) is type(f32[j]['misc']['vals'][r.label][0])
                       for d, r in enumerate(group)) for i in range(len(ties))), (j, got)
