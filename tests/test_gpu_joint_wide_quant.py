"""GPU tests of the wide quantised joint stage (tpe_joint_wide_quant_run through
Engine.run_joint_wide_quant) and of tpe.suggest(..., joint_wide_quantized=True),
against the float64 model restated in numpy (tests/joint_wide_quant_ref.py).

Tolerances are the project's (tests/test_gpu_kernels.py, tests/test_gpu_joint.py):
l and g within 1e-5 * max(1, |ref|).  The winner is checked against the
device's OWN l - g, exactly: np.argmax order (NaN first, the lower index on a
tie), the winner's z, l and g copied bit for bit.  The Philox streams are
checked bit for bit against the stages that draw the same words."""
import functools
import math

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R
from tests import joint_wide_quant_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


# (Dc, us, Vs, n trials, ids, C, qloguniform lattice).  Even continuous dimensions are bounded, odd ones
# unbounded (joint_quant_ref.seeded_quant_case).  The above side has n - nb + 1 components, nb = ceil(sqrt(n) / 4);
# the component tile of each instantiation is joint_wide_quant_ref.tile_of (asserted in the test):
#   (17, 0, 1) V = [2]         DP 24, KP 0, tile 128: 297 components = 128 + 128 + 41; C = 700: one ragged chunk
#   (9, 1, 1)  V = [11]        DP 16, at most 16 labels but past the narrow stage; one tile of 59
#   (20, 2, 2) V = [256, 256]  DP 24, sum V at the limit, tile 8: 68 components = 8 tiles of 8 and one of 4
#   (28, 8, 4) V = [2, 3, 5, 7]  DP 32, KP 8, QP 4, tile 128: 297 components = 128 + 128 + 41
#   (44, 3, 1) V = [37]        DP 48, R = 1, tile 80: 197 components = 80 + 80 + 37; the qloguniform lattice
#   (59, 1, 4) V = [4, 4, 4, 4]  DP 64, 64 coordinates, tile 64: 147 components = 64 + 64 + 19
SHAPES = [
    (17, (), (2,), 301, (3,), 700, False),
    (9, (3,), (11,), 60, (5, 9), 2 * 512 + 37, False),
    (20, (3, '5p'), (256, 256), 70, (7,), 2 * 512 + 37, False),
    (28, (2, 3, '5p', 4, 2, 3, 2, 6), (2, 3, 5, 7), 301, (1, 2, 4), 2 * 512 + 37, False),
    (44, (3, 2, 4), (37,), 200, (11, 12), 2 * 256 + 37, True),
    (59, (3,), (4, 4, 4, 4), 150, (8,), 2 * 256 + 37, False),
]
TILES = {17: (128, 297, 3), 9: (128, 59, 1), 20: (8, 68, 9), 28: (128, 297, 3), 44: (80, 197, 3), 59: (64, 147, 3)}


@functools.lru_cache(maxsize=None)
def case(Dc, us, Vs, n, qlog):
    below, above, low, high, ps, sb, sa, edges, _ = W.wide_quant_case(Dc, list(us), list(Vs), n, qlog=qlog)
    return below, above, low, high, ps, sb, sa, edges


def _split(cand, Dc, Dk):
    return cand[:, :Dc].astype(np.float64), cand[:, Dc:Dc + Dk].astype(np.int64), cand[:, Dc + Dk:].astype(np.int64)


def _check_records(rec, cand, l, g, D, what):
    """Each id's record is np.argmax of the device's own l - g (NaN first, the
    lower index on a tie), the winner's z, l and g bit for bit."""
    for j in range(len(rec)):
        with np.errstate(invalid='ignore'):
            i = int(np.argmax(l[j] - g[j]))
        assert int(rec['global_idx'][j]) == i, (what, j, int(rec['global_idx'][j]), i)
        assert rec['l'][j].tobytes() == l[j][i].tobytes() and rec['g'][j].tobytes() == g[j][i].tobytes()
        assert rec['z'][j, :D].tobytes() == cand[j][i].astype(np.float64).tobytes()
        assert (rec['z'][j, D:] == 0).all()


@pytest.mark.parametrize('Dc,us,Vs,n,ids,C,qlog', SHAPES)
def test_wide_quant_stage(engine, Dc, us, Vs, n, ids, C, qlog):
    below, above, low, high, ps, sb, sa, edges = case(Dc, us, Vs, n, qlog)
    Dk, Dq = len(us), len(Vs)
    D = Dc + Dk + Dq
    assert W.takes_wide_stage(Dc, Dk, Dq)
    tile, ka, n_tiles = TILES[Dc]
    assert W.tile_of(Dc, sum(Vs)) == tile and len(above[0]) == ka and -(-ka // tile) == n_tiles
    assert n_tiles == 1 or ka % tile != 0                       # a ragged last tile
    assert np.isfinite(low).any() and (Dc < 2 or np.isinf(low).any())
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    what = 'Dc=%d Dk=%d Vs=%s' % (Dc, Dk, Vs)

    def run(ids, seed=23):
        return engine.run_joint_wide_quant(below[:3], above[:3], low, high, cats, quants, list(ids), C, seed,
                                           return_cand=True, want_lg=True)
    rec, cand, l, g = run(ids)
    assert cand.shape == (len(ids), C, D) and l.shape == g.shape == (len(ids), C)
    assert rec.dtype == N.JOINT_WIDE_RECORD_DTYPE
    # (i) l and g of every returned candidate against the float64 model
    for j in range(len(ids)):
        z64, v, qi = _split(cand[j], Dc, Dk)
        for d, e in enumerate(edges):
            assert (cand[j][:, Dc + Dk + d] == qi[:, d]).all() and qi[:, d].min() >= 0 and qi[:, d].max() < len(e) - 1
        for d, p in enumerate(ps):
            assert (cand[j][:, Dc + d] == v[:, d]).all() and v[:, d].min() >= 0 and v[:, d].max() < len(p)
        bounded = np.isfinite(low)
        assert (z64[:, bounded] >= low[bounded]).all() and (z64[:, bounded] < high[bounded]).all()
        R.check_lpdf(l[j], W.ref_wide_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges), 'l %s id %d' % (what, j))
        R.check_lpdf(g[j], W.ref_wide_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges), 'g %s id %d' % (what, j))
    # (ii) the records
    _check_records(rec, cand, l, g, D, what)
    # (iii) the continuous and discrete coordinates are those of the stage without the quantised labels
    if Dk:
        _, other = engine.run_joint_wide_mixed(below[:3], above[:3], low, high, cats, list(ids), C, 23, return_cand=True)
    else:
        _, other = engine.run_joint_wide(below[:3], above[:3], low, high, list(ids), C, 23, return_cand=True)
    assert other.shape == (len(ids), C, Dc + Dk)
    assert np.ascontiguousarray(cand[:, :, :Dc + Dk]).tobytes() == other.tobytes()
    # (iv) the same call twice; a batched call against the single-id calls
    again = run(ids)
    for x, y in zip((rec, cand, l, g), again):
        assert x.tobytes() == y.tobytes()
    if len(ids) > 1:
        assert len({cand[j].tobytes() for j in range(len(ids))}) == len(ids)   # every id its own stream
        for j, new_id in enumerate(ids):
            s = run([new_id])
            assert s[0].tobytes() == rec[j:j + 1].tobytes()
            for k, whole in ((1, cand), (2, l), (3, g)):
                assert s[k][0].tobytes() == whole[j].tobytes()


@pytest.mark.parametrize('Dc,us,Vs', [(5, (3, '5p'), (11, 4)), (8, (2, 3, '5p', 4), (3, 64, 17, 10)), (3, (), (32,))])
def test_a_narrow_shape_draws_the_quantised_stage_s_candidates_and_tables(engine, Dc, us, Vs):
    """A shape both stages take: every coordinate, and both sides' tables as the
    device built them, equal run_joint_quant's byte for byte."""
    C = 2 * 512 + 37
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, list(us), list(Vs), 60)
    assert not W.takes_wide_stage(Dc, len(us), len(Vs))
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    kw = dict(return_cand=True, want_lg=True, return_table=True)
    wrec, wcand, wl, wg, wtb, wta = engine.run_joint_wide_quant(below[:3], above[:3], low, high, cats, quants, [11, 12],
                                                                C, 42, **kw)
    _, ncand, _, _, ntb, nta = engine.run_joint_quant(below[:3], above[:3], low, high, cats, quants, [11, 12], C,
                                                 42, **kw)
    assert wcand.shape == ncand.shape == (2, C, Dc + len(us) + len(Vs))
    assert wcand.tobytes() == ncand.tobytes()
    assert wtb.shape == (len(below[0]), sum(Vs)) and wta.shape == (len(above[0]), sum(Vs))
    assert wtb.tobytes() == ntb.tobytes() and wta.tobytes() == nta.tobytes()
    for j in range(2):
        z64, v, qi = _split(wcand[j], Dc, len(us))
        R.check_lpdf(wl[j], W.ref_wide_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges), 'l narrow %d' % j)
        R.check_lpdf(wg[j], W.ref_wide_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges), 'g narrow %d' % j)
    _check_records(wrec, wcand, wl, wg, Dc + len(us) + len(Vs), 'narrow')


def test_injected_rows_on_lattice_ends_and_in_far_bins(engine):
    """Injected candidates whose lattice indices sit on the two ends of a
    256-value lattice and in bins whose mass under most above components is
    exactly 0 (table entries at TPE_JOINT_QFLOOR): l and g stay within the tolerance, and
    every id scores the same rows."""
    Dc, us, Vs, n, C = 20, (3, '5p'), (256, 256), 70, 2 * 512 + 37
    below, above, low, high, ps, sb, sa, edges = case(Dc, us, Vs, n, False)
    Dk, Dq = len(us), len(Vs)
    # (asserted on the reference) the above side's tables hold bins of mass exactly 0
    for d in range(Dq):
        _, raw = Q.ref_table(above[4][:, d], above[5][:, d], edges[d])
        assert (raw < Q.QFLOOR).sum() > 0 and np.isneginf(raw).any()
    rs = np.random.RandomState(5)
    bounded = np.isfinite(low)
    z = np.where(bounded[None, :], rs.uniform(-10, 10, (C, Dc)), rs.normal(1.0, 4.0, (C, Dc))).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, high, np.inf).astype(np.float32), np.float32(-np.inf))
    z = np.clip(z, np.where(bounded, low, -np.inf).astype(np.float32)[None, :], hi32[None, :])
    k = rs.choice(len(below[0]), size=C // 4, p=below[0])       # a quarter near below components
    z[:C // 4] = np.clip((below[1][k] + below[2][k] * rs.standard_normal((C // 4, Dc))).astype(np.float32),
                         np.where(bounded, low, -np.inf).astype(np.float32)[None, :], hi32[None, :])
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1)
    qi = np.stack([rs.randint(V, size=C) for V in Vs], axis=1)
    qi[0::8, 0], qi[1::8, 0], qi[2::8, 1], qi[3::8, 1] = 0, 255, 0, 255          # the lattice ends
    # far bins: the bin farthest from every trial component of the side (the prior row alone reaches it)
    for d in range(Dq):
        centre = np.concatenate([below[4][1:, d], above[4][1:, d]])
        dist = np.abs(np.arange(256)[:, None] - centre[None, :]).min(axis=1)
        qi[4 + d::8, d] = int(np.argmax(dist))
    cand = np.hstack([z, v.astype(np.float32), qi.astype(np.float32)])
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    rec, back, l, g = engine.run_joint_wide_quant(below[:3], above[:3], low, high, cats, quants, [4, 6], C, 3,
                                                  inject=cand, return_cand=True, want_lg=True)
    assert back.shape == (2, C, Dc + Dk + Dq) and back[0].tobytes() == cand.tobytes() == back[1].tobytes()
    z64, vv, qq = _split(cand, Dc, Dk)
    l_ref = W.ref_wide_quant_lpdf(z64, vv, qq, below, low, high, ps, sb, edges)
    g_ref = W.ref_wide_quant_lpdf(z64, vv, qq, above, low, high, ps, sa, edges)
    R.check_lpdf(l[0], l_ref, 'injected l')
    R.check_lpdf(g[0], g_ref, 'injected g')
    assert l[0].tobytes() == l[1].tobytes() and g[0].tobytes() == g[1].tobytes()
    _check_records(rec, back, l, g, Dc + Dk + Dq, 'injected')


# ------------------------------------------------------------ the public path
LOW_B, HIGH_B = math.log(16.0), math.log(512.0)
ALL = dict(joint=True, joint_wide=True, joint_discrete=True, joint_quantized=True, joint_wide_quantized=True)


@functools.lru_cache(maxsize=None)
def _public_case():
    """A network space: 20 continuous knobs, batch = qloguniform, layers =
    quniform(q = 2), an optimizer choice; beside them labels that no joint
    keyword joins (a qnormal, a gate and its branch)."""
    from hyperopt_amd import base, hp, rand
    space = {'k%02d' % i: (hp.loguniform('k%02d' % i, -6, 0) if i % 3 == 0 else hp.uniform('k%02d' % i, -1, 1))
             for i in range(20)}
    space.update({'batch': hp.qloguniform('batch', LOW_B, HIGH_B, 16), 'layers': hp.quniform('layers', 2, 12, 2),
                  'opt': hp.choice('opt', ['sgd', 'adam', 'rmsprop']), 'qn': hp.qnormal('qn', 0, 3, 1),
                  'reg': hp.choice('reg', [0, {'k': hp.uniform('l2', 0, 1)}])})
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(48):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = (math.log(float(v['k00'])) - math.log(float(v['batch']) / 256.0) + 4.0) ** 2 \
            + 0.3 * (float(v['layers']) - 6.0) ** 2 + 0.2 * int(v['opt']) + float(v['k01']) ** 2 + 1e-3 * rs.uniform()
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


JOINED = ['k%02d' % i for i in range(20)] + ['batch', 'layers', 'opt']


def test_public_joint_wide_quantized_suggest():
    from hyperopt_amd import history, tpe
    domain, trials = _public_case()
    C, seed, ids = 2048, 321, [48, 49]
    # without the keyword the space raises, as it always has
    with pytest.raises(ValueError, match='continuous labels only'):
        tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=True, joint_wide=True, joint_discrete=True,
                    joint_quantized=True)
    plain = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C)
    docs = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, **ALL)
    hist = history.extract(domain, trials)
    dicts = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=C, **ALL)
    for doc, pdoc, d in zip(docs, plain, dicts):
        trials.assert_valid_trial(doc)
        got, was = _vals(doc), _vals(pdoc)
        assert set(got) == set(was)
        for k in got:
            if k not in JOINED:               # not joined: the same bytes and types as without joint
                assert type(got[k]) is type(was[k]) and np.asarray(got[k]).tobytes() == np.asarray(was[k]).tobytes(), k
        assert any(got[k] != was[k] for k in JOINED)
        for k, q, lo, hi in (('batch', 16.0, 16.0, 512.0), ('layers', 2.0, 2.0, 12.0)):
            assert type(d[k]) is np.float64 and d[k] == got[k]
            assert got[k] == np.rint(got[k] / q) * q and lo <= got[k] <= hi, (k, got[k])
        assert type(d['opt']) is np.int64 and 0 <= d['opt'] < 3 and int(got['opt']) == d['opt']
        for i in range(20):
            k = 'k%02d' % i
            assert type(d[k]) is np.float64 and d[k] == got[k]
            assert (math.exp(-6) <= got[k] <= 1.0) if i % 3 == 0 else (-1 <= got[k] < 1)
    # a batched call gives the single-id calls' documents
    for j, new_id in enumerate(ids):
        assert _vals(tpe.suggest([new_id], domain, trials, seed, n_EI_candidates=C, **ALL)[0]) == _vals(docs[j])
    # a list names a group of 12 knobs and one quantised label (13 labels: past the narrow stage's 8 continuous)
    some = ['k%02d' % i for i in range(12)] + ['batch']
    two = _vals(tpe.suggest([48], domain, trials, seed, n_EI_candidates=C, joint=some, joint_wide=True,
                            joint_quantized=True, joint_wide_quantized=True)[0])
    was = _vals(plain[0])
    for k in was:
        if k not in some:
            assert type(two[k]) is type(was[k]) and np.asarray(two[k]).tobytes() == np.asarray(was[k]).tobytes(), k
    assert two['batch'] == np.rint(two['batch'] / 16.0) * 16.0 and 16.0 <= two['batch'] <= 512.0
    with pytest.raises(ValueError, match='at most 8 continuous labels beside a quantised one'):
        tpe.suggest([48], domain, trials, seed, n_EI_candidates=C, joint=some, joint_wide=True, joint_quantized=True)


def test_the_report_s_entry_0_is_the_vector_suggest_joins():
    from hyperopt_amd import tpe
    domain, trials = _public_case()
    C, seed = 2048, 321
    got = _vals(tpe.suggest([48], domain, trials, seed, n_EI_candidates=C, **ALL)[0])
    rep = tpe.joint_candidate_report(48, domain, trials, seed, k=4, n_EI_candidates=C, **ALL)
    assert len(rep) == 1
    gr = rep[0]
    assert gr.condition is None and sorted(gr.labels) == sorted(JOINED) and gr.labels[-3:] == ['opt'] + [
        r.label for r in domain.table.rows if r.label in ('batch', 'layers')]
    assert gr.n_top == 4 and gr.vectors.shape == (4, 23)
    for lab, val in zip(gr.labels, gr.vectors[0]):
        assert float(got[lab]) == float(val), lab
    assert (np.diff(gr.top['score']) <= 0).all() and len(np.unique(gr.vectors, axis=0)) == 4
