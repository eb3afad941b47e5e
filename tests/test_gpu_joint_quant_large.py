"""GPU tests of the large-lattice joint stage (Engine.run_joint_quant_large) and
of tpe.suggest(..., joint_quantized='large'), against the table stage (the same
bytes) and the float64 model (tests/joint_quant_ref.py) at the project's
tolerances: l and g within 1e-5 * max(1, |ref|), the winner inside tie_set."""
import functools
import math

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R
from tests.test_gpu_joint_quant import check_quant_winner, quant_candidates

pytestmark = pytest.mark.gpu

C2 = 1024 + 37                      # one full chunk and a ragged one
QLOG = ('qloguniform', math.log(8.0), math.log(4096.0), 1.0)    # wide bins at the low end, narrow ones at the high end


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _args(case):
    below, above, low, high, ps, sb, sa, edges = case[:8]
    return (below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges))


@pytest.mark.parametrize('Dc,us,Vs', [(1, (), (5,)), (3, (), (17, 4)), (5, (), (256,)), (2, (3,), (17, 4))])
def test_same_entries_same_sums(engine, Dc, us, Vs):
    """Sampled candidates, record, l and g of a group both stages take: equal byte for byte."""
    case = Q.seeded_quant_case(Dc, list(us), list(Vs), 60)
    want = engine.run_joint_quant(*_args(case), [3, 11], C2, seed=5, return_cand=True, want_lg=True)
    got = engine.run_joint_quant_large(*_args(case), [3, 11], C2, seed=5, return_cand=True, want_lg=True)
    for a, b, what in zip(want, got, ('record', 'cand', 'l', 'g')):
        assert a.tobytes() == b.tobytes(), what


def _qlog_side(side, d, n, seed):                    # quantised dimension d's components: n QLOG observations
    mu, sg = Q.lattice_components(QLOG, n, seed=seed)
    qmu, qsig = side[4].copy(), side[5].copy()
    qmu[:, d], qsig[:, d] = mu, sg
    return side[:4] + (qmu, qsig)


# name -> (Dc, us, Vs, the dimension that is QLOG or None, how the candidates' lattice indices are set)
CASES = {
    'V257': (0, (), (257,), None, 'edges'),                 # the smallest lattice the table stage refuses
    'V1000_cont': (1, (), (1000,), None, 'edges'),
    'qlog': (0, (), (4089,), 0, 'edges'),
    'two_large': (0, (), (1500, 1100), None, 'edges'),      # 2049 mini-table rows at most: more than 64 KiB of LDS
    'large_small_choice': (0, (3,), (2000, 17), None, 'edges'),
    'one_bin': (1, (), (3000,), None, 'one'),               # the two ends of the compaction
    'distinct': (1, (), (3000,), None, 'distinct'),
}


@functools.lru_cache(maxsize=None)
def injected_case(name):
    Dc, us, Vs, qlog, how = CASES[name]
    below, above, low, high, ps, sb, sa, edges, rs = Q.seeded_quant_case(Dc, list(us), list(Vs), 60)
    if qlog is not None:
        m_lo, V, e = Q.ref_lattice(*QLOG)
        assert (m_lo, V) == (8, Vs[qlog])
        edges[qlog] = e
        below = _qlog_side(below, qlog, len(below[0]) - 1, 1)
        above = _qlog_side(above, qlog, len(above[0]) - 1, 2)
    cand = quant_candidates(below, low, high, ps, edges, C2, 7)
    q0 = Dc + len(us)
    for d, V in enumerate(Vs):
        col = cand[:, q0 + d]
        if how == 'one':
            col[:1024] = 1234.0                              # the first chunk: one mini-table row
        elif how == 'distinct':
            col[:1024] = rs.permutation(V)[:1024]            # the first chunk: 1,024 rows (V >= 1024: all distinct)
        else:
            k = int(np.argmax(np.bincount(np.rint(above[4][1:, d]).astype(np.int64).clip(0, V - 1))))
            # index 0, V - 1, a value many components share, far from every component
            far = int(np.argmax(np.abs(np.arange(V)[:, None] - above[4][None, :, d]).min(axis=1))) \
                if qlog is None else 0
            col[[0, 1, 2, 3, 1030, 1031]] = [0.0, V - 1.0, float(k), float(far), V - 1.0, 0.0]
    z64, v, qi = cand[:, :Dc].astype(np.float64), cand[:, Dc:q0].astype(np.int64), cand[:, q0:].astype(np.int64)
    l_ref = Q.ref_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges)
    g_ref = Q.ref_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges)
    return below, above, low, high, ps, sb, sa, edges, cand, l_ref, g_ref


@pytest.mark.parametrize('name', sorted(CASES))
def test_large_lattices_against_the_float64_model(engine, name):
    case = injected_case(name)
    cand, l_ref, g_ref = case[8:]
    rec, l, g = engine.run_joint_quant_large(*_args(case), [7], C2, seed=3, inject=cand, want_lg=True)
    R.check_lpdf(l[0], l_ref, 'l ' + name)
    R.check_lpdf(g[0], g_ref, 'g ' + name)
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_quant_winner(rec[0], cand, l_ref, g_ref, cand.shape[1], name)


def test_suggest_joins_a_large_lattice(engine):
    from hyperopt_amd import base, history, hp, joint as J, rand, tpe
    space = {'lr': hp.loguniform('lr', -7, 0), 'units': hp.quniform('units', 16, 1024, 1), 'k': hp.choice('k', [0, 1])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(0)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, rs.randint(2 ** 31 - 1))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if x}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': (math.log(v['lr']) + 3) ** 2 + abs(v['units'] - 300) / 100 + v['k']}
        trials.insert_trial_docs(docs)
    trials.refresh()
    kw = dict(n_startup_jobs=5, n_EI_candidates=C2)
    ids = [40, 41, 42]
    vals = [d['misc']['vals'] for d in tpe.suggest(ids, domain, trials, 9, joint=['lr', 'units'],
                                                   joint_quantized='large', **kw)]
    plain = [d['misc']['vals'] for d in tpe.suggest(ids, domain, trials, 9, **kw)]
    hist = history.extract(domain, trials)
    rows = [domain.table.by_label[x] for x in ('lr', 'units')]
    model = J.fit_quant_model(rows[:1], [], rows[1:], hist, history.split_below(hist, tpe._default_gamma), 1.0,
                              tpe.DEFAULT_LF)
    rec = engine.run_joint_quant_large(model.below[:3], model.above[:3], model.low, model.high, model.cats(),
                                       model.quants(), ids, C2, 9)
    want = model.values(rec['z'][:, :2])
    for j, i in enumerate(ids):
        u = vals[j]['units'][0]
        assert type(u) is np.float64 and u == np.rint(u) and 16 <= u <= 1024
        assert u == want[j, 1] and vals[j]['lr'][0] == want[j, 0]
        assert vals[j]['k'] == plain[j]['k']                 # the unjoined label: the bytes of the call without joint
        one = tpe.suggest([i], domain, trials, 9, joint=['lr', 'units'], joint_quantized='large', **kw)[0]
        assert one['misc']['vals'] == vals[j]                # batched ids equal the single-id calls
