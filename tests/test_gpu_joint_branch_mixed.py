"""GPU tests of the mixed segmented joint stage (tpe_joint_mseg_run through
Engine.run_joint_segments) and of tpe.suggest(..., joint_branches_mixed=True) on
the benchmark tree (DESIGN.md "Discrete and quantised labels in branch groups").

The stage's defining property is tested as bytes: problem (id, segment) equals
the solo run over that segment alone (tpe_joint_quant_run, tpe_joint_mixed_run
or tpe_joint_run by the segment's kind) with its stream word and ids = [id].
Against the float64 models restated in numpy (tests/joint_*_ref.py) the
tolerances are the project's (tests/test_gpu_joint_quant.py): l and g within
1e-5 * max(1, |ref|), the winner inside the tie set, and at most MAX_TIES
distinct vectors in it."""
import functools

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # distinct vectors: a plateau of near-equal scores must not hide a wrong winner
C = 4096 + 1          # 5 chunks, the last ragged
SEED = 17


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


class Seg(object):
    """One segment: ``model`` as run_joint_segments takes it and the parts the
    float64 references need."""

    def __init__(self, kind, below, above, low, high, ps=(), sb=(), sa=(), edges=()):
        self.kind, self.below, self.above, self.low, self.high = kind, below, above, low, high
        self.ps, self.sb, self.sa, self.edges = list(ps), sb, sa, list(edges)
        self.Dc, self.Dk, self.Dq = len(low), len(self.ps), len(self.edges)
        self.D = self.Dc + self.Dk + self.Dq
        cats = M.cats_of(below, above, self.ps, sb, sa) if self.Dk else []
        if kind == 'quant':
            self.model = (below[:3], above[:3], low, high, cats, Q.quants_of(below, above, self.edges))
        elif kind == 'mixed':
            self.model = (below[:3], above[:3], low, high, cats)
        else:
            self.model = (below, above, low, high)

    def solo(self, engine, word, new_id, inject=None, **kw):
        """The solo run of this segment's kind with the stream word ``word``."""
        kw = dict(dict(return_cand=True, want_lg=True), **kw)
        if self.kind == 'quant':
            return engine.run_joint_quant(*self.model, [new_id], C, SEED, inject=inject, stream_word=word, **kw)
        if self.kind == 'mixed':
            return engine.run_joint_mixed(*self.model, [new_id], C, SEED, inject=inject, stream_word=word, **kw)
        return engine.run_joint(*self.model, [new_id], C, SEED, inject, kw['return_cand'], kw['want_lg'],
                                stream_word=word)

    def ref(self, cand):
        """float64 (l, g) of kernel rows ``cand`` [C, D]."""
        z = cand[:, :self.Dc].astype(np.float64)
        v = cand[:, self.Dc:self.Dc + self.Dk].astype(np.int64)
        qi = cand[:, self.Dc + self.Dk:].astype(np.int64)
        if self.kind == 'quant':
            return (Q.ref_quant_lpdf(z, v, qi, self.below, self.low, self.high, self.ps, self.sb, self.edges),
                    Q.ref_quant_lpdf(z, v, qi, self.above, self.low, self.high, self.ps, self.sa, self.edges))
        if self.kind == 'mixed':
            return (M.ref_mixed_lpdf(z, v, self.below, self.low, self.high, self.ps, self.sb),
                    M.ref_mixed_lpdf(z, v, self.above, self.low, self.high, self.ps, self.sa))
        return R.ref_lpdf(z, self.below, self.low, self.high), R.ref_lpdf(z, self.above, self.low, self.high)


def _quant_seg(Dc, us, Vs, n, seed=None, prior_above=False):
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, list(us), list(Vs), n, seed)
    if prior_above:                                  # the above side: the prior row alone
        above = (np.array([1.0]),) + tuple(a[:1] for a in above[1:])
    return Seg('quant', below, above, low, high, ps, sb, sa, edges)


@functools.lru_cache(maxsize=None)
def _segments():
    """S0: 2 continuous + 1 discrete (U = 3), 40 trials.  S1: 0 continuous, 1
    discrete (U = 2), 1 quantised (V = 50): the rf shape, no continuous rows.
    S2: 1 continuous + 1 quantised (V = 50), above the prior row alone: the knn
    shape.  S3: 3 continuous + 2 discrete + 2 quantised (V = 200, 56), 300
    trials: the above side wraps the 128-row tile and the table needs several
    tiles.  S4: S3's class with V = 2, 3: another tile and stride in the same
    launch.  S5: 5 continuous only.  S6: a segment no problem names."""
    b, a, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(2, [3], 40)
    s3 = _quant_seg(3, (3, '5p'), (200, 56), 300)
    assert len(s3.above[0]) == 296
    s2 = _quant_seg(1, (), (50,), 40, prior_above=True)
    assert len(s2.above[0]) == 1 and len(s2.below[0]) == 3
    segs = [Seg('mixed', b, a, low, high, ps, sb, sa), _quant_seg(0, (2,), (50,), 60), s2, s3,
            _quant_seg(3, (2, 4), (2, 3), 80), Seg('cont', *R.seeded_case(5, 300, 205)[:4]),
            _quant_seg(2, (3,), (5,), 30)]
    return segs, [0xFFFFFFFE - 3 * s for s in range(len(segs))]


# (new id, segment): non-contiguous ids, id 9 in two segments, unsorted, S3 and S4 interleaved
PROBLEMS = [(9, 3), (5, 0), (40, 4), (9, 1), (12, 3), (1000003, 2), (7, 4), (33, 5), (2, 1)]


@pytest.fixture(scope='module')
def seg_run(engine):
    """The segmented call over PROBLEMS (computed once, shared, not modified)."""
    segs, words = _segments()
    out = engine.run_joint_segments([s.model for s in segs], words, [p[1] for p in PROBLEMS],
                                    [p[0] for p in PROBLEMS], C, SEED, return_cand=True, want_lg=True)
    return segs, words, out


def test_segmented_run_equals_solo_runs_bytes(engine, seg_run):
    segs, words, (rec, cand, l, g) = seg_run
    P = len(PROBLEMS)
    assert rec.shape == (P,) and l.shape == g.shape == (P, C) and len(cand) == P
    for p, (new_id, s) in enumerate(PROBLEMS):
        assert cand[p].shape == (C, segs[s].D) and cand[p].dtype == np.float32
        srec, scand, sl, sg = segs[s].solo(engine, words[s], new_id)
        assert rec[p:p + 1].tobytes() == srec.tobytes(), (p, rec[p], srec)
        assert cand[p].tobytes() == scand[0].tobytes(), p
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes(), p
    # two ids of one segment differ; the stream word matters
    assert cand[0].tobytes() != cand[4].tobytes()
    other = segs[1].solo(engine, None, 9)
    assert other[1][0].tobytes() != cand[3].tobytes()


def test_twice_the_same_bytes_any_order_and_records_alone(engine, seg_run):
    segs, words, first = seg_run
    models = [s.model for s in segs]
    ids, sg = [p[0] for p in PROBLEMS], [p[1] for p in PROBLEMS]
    again = engine.run_joint_segments(models, words, sg, ids, C, SEED, return_cand=True, want_lg=True)
    assert again[0].tobytes() == first[0].tobytes()
    assert again[2].tobytes() == first[2].tobytes() and again[3].tobytes() == first[3].tobytes()
    for x, y in zip(again[1], first[1]):
        assert x.tobytes() == y.tobytes()
    perm = [6, 2, 8, 4, 0, 5, 1, 7, 3]
    rec, cand, l, g = engine.run_joint_segments(models, words, [sg[p] for p in perm], [ids[p] for p in perm], C, SEED,
                                                return_cand=True, want_lg=True)
    for q, p in enumerate(perm):
        assert rec[q:q + 1].tobytes() == first[0][p:p + 1].tobytes(), (q, p)
        assert cand[q].tobytes() == first[1][p].tobytes()
        assert l[q].tobytes() == first[2][p].tobytes() and g[q].tobytes() == first[3][p].tobytes()
    assert engine.run_joint_segments(models, words, sg, ids, C, SEED).tobytes() == first[0].tobytes()


def test_all_continuous_list_is_the_segmented_stage_of_today(engine, monkeypatch):
    """Continuous models only: the native function reached is
    tpe_joint_seg_run, never tpe_joint_mseg_run or its table size query."""
    cases = [R.seeded_case(2, 40, 202)[:4], R.seeded_case(5, 300, 205)[:4]]
    words = [0xFFFFFFFE - 1, 0xFFFFFFFE - 4]
    probs, ids = [1, 0, 1], [9, 9, 12]
    want = [engine.run_joint(*cases[s], [i], C, SEED, None, True, True, stream_word=words[s])
            for s, i in zip(probs, ids)]
    reached, native, lib = [], engine._joint_native, engine.lib
    monkeypatch.setattr(engine, '_joint_native', lambda fn, *a: (reached.append(fn), native(fn, *a))[1])

    class Lib(object):                                # the library, its mixed segmented entry points barred
        def __getattr__(self, name):
            assert not name.startswith('tpe_joint_mseg'), name
            return getattr(lib, name)
    monkeypatch.setattr(engine, 'lib', Lib())
    rec, cand, l, g = engine.run_joint_segments(cases, words, probs, ids, C, SEED, return_cand=True, want_lg=True)
    assert reached == ['tpe_joint_seg_run']
    for p, w in enumerate(want):
        assert rec[p:p + 1].tobytes() == w[0].tobytes() and cand[p].tobytes() == w[1][0].tobytes()
        assert l[p].tobytes() == w[2][0].tobytes() and g[p].tobytes() == w[3][0].tobytes()


def _check_winner(rec, cand, l_ref, g_ref, D, what):
    """The winner's vector is in the tie set (at most MAX_TIES distinct
    vectors) and its index the lowest one holding that vector."""
    ties, score = R.tie_set(l_ref, g_ref)
    idx = int(rec['global_idx'])
    distinct = np.unique(cand[ties], axis=0)
    print('%s: winner %d, argmax %d, %d ties, %d distinct' % (what, idx, int(np.argmax(score)), len(ties),
                                                             len(distinct)))
    assert len(distinct) <= MAX_TIES, (what, len(distinct))
    same = np.flatnonzero((cand == cand[idx][None, :]).all(axis=1))
    assert np.isin(same, ties).any(), (what, idx, int(np.argmax(score)), ties[:10])
    assert idx == int(same[0]), (what, idx, same[:10])
    np.testing.assert_array_equal(rec['z'][:D], cand[idx].astype(np.float64))
    assert (rec['z'][D:] == 0).all()


def test_against_the_float64_models(seg_run):
    segs, words, (rec, cand, l, g) = seg_run
    for p, (new_id, s) in enumerate(PROBLEMS):
        sg = segs[s]
        z64 = cand[p][:, :sg.Dc].astype(np.float64)
        assert np.all(z64 >= sg.low[None, :]) and np.all(z64 < sg.high[None, :])
        for d, pr in enumerate(sg.ps):
            v = cand[p][:, sg.Dc + d]
            assert np.all(v == np.rint(v)) and v.min() >= 0 and v.max() < len(pr)
        for d, e in enumerate(sg.edges):
            v = cand[p][:, sg.Dc + sg.Dk + d]
            assert np.all(v == np.rint(v)) and v.min() >= 0 and v.max() < len(e) - 1
        l_ref, g_ref = sg.ref(cand[p])
        what = 'problem %d (id %d, S%d)' % (p, new_id, s)
        R.check_lpdf(l[p], l_ref, 'l ' + what)
        R.check_lpdf(g[p], g_ref, 'g ' + what)
        i = int(rec['global_idx'][p])
        assert rec['l'][p] == l[p][i] and rec['g'][p] == g[p][i]
        assert i == int(np.argmax(l[p] - g[p]))                  # the device's own scores: np.argmax order exactly
        _check_winner(rec[p], cand[p], l_ref, g_ref, sg.D, what)


def _candidates(sg, seed):
    """C kernel rows of a segment: the continuous part over the box / the prior,
    categories and lattice indices uniform; one eighth around the below
    components."""
    rs = np.random.RandomState(seed)
    w = sg.below[0]
    k = rs.choice(len(w), size=C // 8, p=w)
    bounded = np.isfinite(sg.low)
    z = np.where(bounded[None, :], rs.uniform(-10, 10, (C, sg.Dc)), rs.normal(1.0, 4.0, (C, sg.Dc)))
    if sg.Dc:
        z[:C // 8] = sg.below[1][k] + sg.below[2][k] * rs.standard_normal((C // 8, sg.Dc))
    z = z.astype(np.float32)
    lo32 = np.where(bounded, sg.low, -np.inf).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, sg.high, np.inf).astype(np.float32), np.float32(-np.inf))
    z = np.clip(z, lo32[None, :], hi32[None, :])
    cols = [rs.randint(len(p), size=C) for p in sg.ps] + [rs.randint(len(e) - 1, size=C) for e in sg.edges]
    return np.hstack([z] + [c[:, None].astype(np.float32) for c in cols])


def test_injected_candidates(engine):
    """One call with injected candidates for S1, S3 and S5, equal to the solo
    injected runs and to the float64 models."""
    segs, words = _segments()
    inj = [None] * len(segs)
    for s in (1, 3, 5):
        inj[s] = _candidates(segs[s], 50 + s)
    probs = [(9, 3), (4, 1), (12, 5), (77, 3)]
    rec, cand, l, g = engine.run_joint_segments([s.model for s in segs], words, [p[1] for p in probs],
                                                [p[0] for p in probs], C, SEED, inject=inj, return_cand=True,
                                                want_lg=True)
    for p, (new_id, s) in enumerate(probs):
        srec, scand, sl, sg = segs[s].solo(engine, words[s], new_id, inject=inj[s])
        assert cand[p].tobytes() == inj[s].tobytes() == scand[0].tobytes()
        assert l[p].tobytes() == sl[0].tobytes() and g[p].tobytes() == sg[0].tobytes()
        assert rec[p:p + 1].tobytes() == srec.tobytes()
        l_ref, g_ref = segs[s].ref(inj[s])
        R.check_lpdf(l[p], l_ref, 'injected l S%d' % s)
        R.check_lpdf(g[p], g_ref, 'injected g S%d' % s)
        _check_winner(rec[p], inj[s], l_ref, g_ref, segs[s].D, 'injected S%d' % s)
    assert l[0].tobytes() == l[3].tobytes()                       # the id does not enter an injected score
    with pytest.raises(ValueError, match='inject lacks'):
        engine.run_joint_segments([s.model for s in segs], words, [3, 0], [9, 12], C, SEED, inject=inj)


# ------------------------------------------------------------ the public path
KW = dict(joint=True, joint_discrete=True, joint_quantized=True, joint_branches=True, joint_branches_mixed=True)
N_CAND = 24


def _space():
    """bench.py's benchmark tree, restated."""
    from hyperopt_amd import hp
    return {'model': hp.choice('model', [
        {'name': 'svm', 'C': hp.loguniform('svm_C', -5, 5),
         'kernel': hp.choice('svm_kernel', [{'gamma': hp.loguniform('svm_rbf_gamma', -5, 2)},
                                            {'degree': hp.quniform('svm_poly_degree', 2, 5, 1)}])},
        {'name': 'rf', 'n_est': hp.quniform('rf_n_est', 10, 500, 10),
         'depth': hp.choice('rf_depth', [None, hp.quniform('rf_depth_n', 2, 30, 1)]),
         'crit': hp.choice('rf_crit', ['gini', 'entropy'])},
        {'name': 'knn', 'k': hp.quniform('knn_k', 1, 50, 1), 'p': hp.uniform('knn_p', 1, 3)}])}


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


@functools.lru_cache(maxsize=None)
def _public_case():
    """66 random trials (gamma = 0.25: the 3 best are the below set), each drawn
    by rand.suggest until it takes the branch its tid is meant to take: tids 0,
    1, 2 (svm, rf, knn) get the best losses, so every branch has a below
    observer; tids 3 .. 40 take svm; the last 25 tids take rf and knn 12 times
    each and svm once.  Linear forgetting weighs the newest 25 above trials
    with exactly 1, so rf and knn have exactly equal posteriors on both sides
    of the gate: they tie for its argmax at every precision, the first rf or
    knn candidate of an id decides, and a batch of ids spreads over both
    branches."""
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, _space())
    trials = base.Trials()
    rs = np.random.RandomState(8)
    want = [0, 1, 2] + [0] * 38 + [1, 2] * 12 + [0]
    for tid, branch in enumerate(want):
        while True:
            docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
            if int(_vals(docs[0])['model']) == branch:
                break
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform()) - (2.0 if tid < 3 else 0.0)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    assert len(trials) == 66
    return domain, trials


GROUPS = {1: ['rf_crit', 'rf_n_est'], 2: ['knn_k', 'knn_p']}      # branch: its group's labels


def test_public_suggest_on_the_benchmark_tree():
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    domain, trials = _public_case()
    table = domain.table
    ids = [66, 67, 70, 90, 91, 1000, 1001, 5000]
    plain = [_vals(d) for d in tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND)]
    docs = tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND, **KW)
    got = [_vals(d) for d in docs]
    took = [int(v['model']) for v in plain]
    print('branches taken:', took)
    assert len(set(took)) >= 2, took
    hist = history.extract(domain, trials)
    below = history.split_below(hist, tpe._default_gamma)
    assert sorted(int(t) for t in below) == [0, 1, 2]
    for j, new_id in enumerate(ids):
        trials.assert_valid_trial(docs[j])
        v, b = got[j], took[j]
        assert set(v) == set(plain[j])
        joined = GROUPS.get(b, [])
        for k in v:                                  # every label outside a group: the plain suggest's bytes
            if k not in joined:
                assert type(v[k]) is type(plain[j][k]) and v[k] == plain[j][k], (j, k)
        if not joined:
            continue
        rows, model = tpe._fit_branch_model([table.by_label[k] for k in joined], hist, below, tpe._default_prior_weight)
        assert isinstance(model, J.QuantModel)
        word = J.branch_stream_word(rows)
        rec = get_engine().run_joint_quant(model.below[:3], model.above[:3], model.low, model.high, model.cats(),
                                           model.quants(), [new_id], N_CAND, 321, stream_word=word)
        want = model.values(rec['z'][:, :len(rows)])[0]
        for d, r in enumerate(rows):
            assert float(v[r.label]) == want[d], (j, r.label, v[r.label], want[d])
        if b == 2:
            assert type(v['knn_k']) is np.float64 and v['knn_k'] == np.rint(v['knn_k']) and 1 <= v['knn_k'] <= 50
            assert type(v['knn_p']) is np.float64 and 1 <= v['knn_p'] < 3
        else:
            assert type(v['rf_n_est']) is np.float64 and v['rf_n_est'] == 10 * np.rint(v['rf_n_est'] / 10)
            assert 10 <= v['rf_n_est'] <= 500
            assert type(v['rf_crit']) is type(plain[j]['rf_crit']) and v['rf_crit'] in (0, 1)
    # batched ids equal single-id calls
    for j in (0, len(ids) - 1):
        assert _vals(tpe.suggest([ids[j]], domain, trials, 321, n_EI_candidates=N_CAND, **KW)[0]) == got[j]


def test_joint_candidate_report_of_both_groups():
    from hyperopt_amd import tpe
    domain, trials = _public_case()
    ids = [66, 67, 70, 90, 91, 1000, 1001, 5000]
    got = [_vals(d) for d in tpe.suggest(ids, domain, trials, 321, n_EI_candidates=N_CAND, **KW)]
    seen = set()
    for j, new_id in enumerate(ids):
        b = int(got[j]['model'])
        if b not in GROUPS or b in seen:
            continue
        seen.add(b)
        rep = tpe.joint_candidate_report(new_id, domain, trials, 321, k=4, n_EI_candidates=N_CAND, **KW)
        assert [(gr.labels, gr.condition) for gr in rep] == [(['knn_p', 'knn_k'], ('model', 2)),
                                                            (['rf_crit', 'rf_n_est'], ('model', 1))]
        gr = rep[0 if b == 2 else 1]                 # entry 0 of the taken branch's group: the vector the suggest joins
        assert gr.n_top >= 1
        for d, lab in enumerate(gr.labels):
            assert gr.vectors[0, d] == float(got[j][lab]), (j, lab)
        for gr in rep:
            assert (np.diff(gr.top['score']) <= 0).all()
        assert (rep[1].vectors[:, 0] == np.rint(rep[1].vectors[:, 0])).all()          # a category
        assert (rep[1].vectors[:, 1] % 10 == 0).all() and (rep[0].vectors[:, 1] % 1 == 0).all()
    assert seen == {1, 2}


def test_fmin_with_the_keywords():
    from hyperopt_amd import fmin, tpe, Trials
    algo = functools.partial(tpe.suggest, n_EI_candidates=256, **KW)
    t = Trials()

    def objective(d):
        m = d['model']
        if m['name'] == 'knn':
            return (m['k'] - 7.0) ** 2 / 50.0 + (m['p'] - 2.0) ** 2
        if m['name'] == 'rf':
            return 0.2 + abs(m['n_est'] - 200.0) / 500.0 + (0.1 if m['crit'] == 'gini' else 0.0)
        return 0.6 + 0.01 * abs(np.log(m['C']))
    fmin(objective, _space(), algo=algo, max_evals=30, trials=t, rstate=np.random.RandomState(0))
    assert len(t) == 30
    for doc in t.trials:
        t.assert_valid_trial(doc)
        v = _vals(doc)
        assert np.isfinite(doc['result']['loss'])
        if int(v['model']) == 2:
            assert v['knn_k'] == np.rint(v['knn_k']) and 1 <= v['knn_k'] <= 50 and 1 <= v['knn_p'] <= 3
        if int(v['model']) == 1:
            assert v['rf_n_est'] % 10 == 0 and 10 <= v['rf_n_est'] <= 500 and v['rf_crit'] in (0, 1)
