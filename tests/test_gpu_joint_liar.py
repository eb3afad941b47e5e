"""GPU tests of batch-aware joint suggests (tpe_joint_liar through
Engine.run_joint / run_joint_wide with ``liar``, and tpe.suggest(...,
joint_liar=True)) against the model restated in numpy (tests/joint_liar_ref.py).

Tolerances are the project's (tests/joint_ref.py): g_j within 1e-5 * max(1,
|ref|); the winner inside the tie set (4 of those bounds) and equal to np.argmax
when that set has one member; liar_sigma bit for bit.  Every winner check is
teacher-forced: step j's reference is built from the device's own earlier picks.
"""
import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_liar_ref as LR
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8
B = 8
C = 4096
CASES = [(3, 60, 11), (2, 3013, 5), (16, 120, 7), (20, 200, 9)]


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


_CASES = {}


def _case(D, n, seed, C=C):
    """(below, above, low, high, psig, cand, l_ref, g_ref), computed once."""
    key = (D, n, seed, C)
    if key not in _CASES:
        below, above, low, high, pmu, psig = R.seeded_case(D, n, seed)
        cand = LR.candidates(below, low, high, C, seed)
        z = cand.astype(np.float64)
        _CASES[key] = (below, above, low, high, psig, cand, R.ref_lpdf(z, below, low, high),
                       R.ref_lpdf(z, above, low, high))
    return _CASES[key]


def _runner(engine, D):
    return engine.run_joint_wide if D > N.JOINT_MAX_DIMS else engine.run_joint


def _check_chain(what, rec, sig, cands, l_refs, g_refs, above, psig, low, high, given=None, cap=False, W=None):
    """Teacher-forced check of one liar call: ``cands`` / ``l_refs`` / ``g_refs``
    one entry per id (the same object for shared candidates).  Returns the
    picked indices and the worst g_j error over tolerance."""
    chain = LR.Chain(above, psig, low, high, W=W, given=given)
    G = len(chain.mu)
    D = cands[0].shape[1]
    if G:
        assert sig[:G].tobytes() == chain.sigma.tobytes(), (what, 'given sigma')
    worst, picks = 0.0, []
    for j in range(len(rec)):
        cand, l_ref = cands[j], l_refs[j]
        gj = chain.log_g(cand.astype(np.float64), g_refs[j])
        idx = int(rec['global_idx'][j])
        assert 0 <= idx < len(cand), (what, j, idx)
        worst = max(worst, R.check_lpdf(np.array([rec['g'][j]]), gj[idx:idx + 1], '%s g_%d' % (what, j)))
        R.check_lpdf(np.array([rec['l'][j]]), l_ref[idx:idx + 1], '%s l_%d' % (what, j))
        ties, score = R.tie_set(l_ref, gj)
        print('%s step %d: winner %d, argmax %d, %d ties' % (what, j, idx, int(np.argmax(score)), len(ties)))
        if cap:
            assert len(ties) <= MAX_TIES, (what, j, len(ties))
        assert idx in ties, (what, j, idx, int(np.argmax(score)), ties[:10])
        if len(ties) == 1:
            assert idx == int(np.argmax(score)), (what, j)
        assert rec['z'][j, :D].tobytes() == cand[idx].astype(np.float64).tobytes(), (what, j)
        assert (rec['z'][j, D:] == 0).all()
        s = chain.add(cand[idx])                              # the device's own pick joins: teacher forcing
        assert sig[G + j].tobytes() == s.tobytes(), (what, j, sig[G + j], s)
        picks.append(idx)
    print('%s: worst g_j err / tol = %.3f' % (what, worst))
    return picks, worst


# ------------------------------------------------- 1, 2: the four cases, B = 8
@pytest.mark.parametrize('D,n,seed', CASES)
def test_greedy_batch_of_injected_candidates(engine, D, n, seed):
    """8 ids over 4096 shared candidates: g_j, the tie set with its cap, distinct
    picks, liar_sigma bit for bit; without ``liar`` one index for all ids, and
    pick 0 is that record's bytes.  (2, 3013, 5): K_above = 3000, the neighbour
    scan and the base stage's tile loop wrap."""
    below, above, low, high, psig, cand, l_ref, g_ref = _case(D, n, seed)
    if n == 3013:
        assert len(above[0]) == 3000
    run, ids = _runner(engine, D), np.arange(100, 100 + B)
    rec, l, g, sig = run(below, above, low, high, ids, C, seed=3, inject=cand, want_lg=True, liar=True,
                         return_sigma=True)
    base, l0, g0 = run(below, above, low, high, ids, C, seed=3, inject=cand, want_lg=True)
    assert len(set(int(i) for i in base['global_idx'])) == 1            # the problem: B copies of one point
    assert rec[:1].tobytes() == base[:1].tobytes()                      # pick 0: the solo record, byte for byte
    assert l.tobytes() == l0.tobytes() and g.tobytes() == g0.tobytes()  # want_lg: the base l and g
    assert sig.shape == (B, D) and sig.dtype == np.float64
    picks, _ = _check_chain('D=%d n=%d' % (D, n), rec, sig, [cand] * B, [l_ref] * B, [g_ref] * B, above, psig, low,
                            high, cap=True)
    assert len(set(picks)) == B, picks


def test_one_dimension_with_wide_plateaus(engine):
    """(1, 300, 3): picks may repeat and the tie sets are large; g_j, tie-set
    membership and liar_sigma only."""
    below, above, low, high, psig, cand, l_ref, g_ref = _case(1, 300, 3)
    rec, sig = engine.run_joint(below, above, low, high, np.arange(B), C, seed=3, inject=cand, liar=True,
                                return_sigma=True)
    _check_chain('D=1 n=300', rec, sig, [cand] * B, [l_ref] * B, [g_ref] * B, above, psig, low, high)


# ------------------------------------------------------- 3: given rows at edges
def _given_case(n=60):
    return _case(2, n, 11, 2048)        # dimension 0 bounded to [-10, 10), dimension 1 unbounded


def _run_given(engine, given, n=60, W=None):
    below, above, low, high, psig, cand, l_ref, g_ref = _given_case(n)
    given = np.asarray(given, dtype=np.float32).reshape(-1, 2)
    rec, sig = engine.run_joint(below, above, low, high, [1, 2], len(cand), seed=3, inject=cand,
                                liar=True if W is None else W, given=given, return_sigma=True)
    assert sig.shape == (len(given) + 2, 2)
    _check_chain('given %s' % (given.tolist(),), rec, sig, [cand] * 2, [l_ref] * 2, [g_ref] * 2, above, psig, low, high,
                 given=given, W=W)
    return sig, np.asarray(above[1], dtype=np.float32), psig


def test_given_equal_to_an_existing_mu(engine):
    mu32 = np.asarray(_given_case()[1][1], dtype=np.float32)
    sig, _, _ = _run_given(engine, [mu32[5]])
    assert (sig[0] > 0).all()


def test_given_below_every_point(engine):
    mu32 = np.asarray(_given_case()[1][1], dtype=np.float32)
    z = np.array([max(-10.0, float(mu32[:, 0].min()) - 0.25), float(mu32[:, 1].min()) - 3.0], dtype=np.float32)
    assert (z < mu32.min(axis=0)).all()
    _run_given(engine, [z])


def test_given_above_every_point(engine):
    mu32 = np.asarray(_given_case()[1][1], dtype=np.float32)
    top = np.nextafter(np.float32(10.0), np.float32(-np.inf))
    z = np.array([min(float(top), float(mu32[:, 0].max()) + 0.25), float(mu32[:, 1].max()) + 3.0], dtype=np.float32)
    assert (z > mu32.max(axis=0)).all()
    _run_given(engine, [z])


def test_given_on_the_f32_lower_bound(engine):
    _run_given(engine, [[-10.0, 0.5]])


def test_given_equal_to_an_earlier_given_row(engine):
    _run_given(engine, [[1.25, -0.75], [1.25, -0.75], [1.25, -0.75]])      # the twin sees its twin as L = z


def test_given_with_few_trials(engine):
    """n small enough that m + 2 < 100: the floor of the clip moves with every liar."""
    below, above = _given_case(20)[:2]
    n = len(above[0]) - 1
    assert n + 4 + 2 < 100
    mu32 = np.asarray(above[1], dtype=np.float32)
    _run_given(engine, [mu32[1], mu32[1], [0.0, 1.0]], n=20, W=LR.weight_sum(n))


# ----------------------------------------------------------------- 4: loop edges
def test_ragged_second_chunk(engine):
    """C = 1025: the second chunk holds one candidate."""
    below, above, low, high, psig, cand, l_ref, g_ref = _case(2, 60, 11, 1025)
    rec, sig = engine.run_joint(below, above, low, high, [0, 1, 2, 3], 1025, seed=3, inject=cand, liar=True,
                                return_sigma=True)
    _check_chain('C=1025', rec, sig, [cand] * 4, [l_ref] * 4, [g_ref] * 4, above, psig, low, high)
    # the candidate alone in the second chunk must be able to win: move the winner's row there
    w, worst = int(rec['global_idx'][0]), int(np.argmin(l_ref - g_ref))
    cand2, l2, g2 = cand.copy(), l_ref.copy(), g_ref.copy()
    for arr in (cand2, l2, g2):
        arr[-1], arr[w] = arr[w].copy(), arr[worst].copy()
    assert 1024 in R.tie_set(l2, g2)[0]
    rec2, sig2 = engine.run_joint(below, above, low, high, [0, 1], 1025, seed=3, inject=cand2, liar=True,
                                  return_sigma=True)
    picks, _ = _check_chain('C=1025, last row best', rec2, sig2, [cand2] * 2, [l2] * 2, [g2] * 2, above, psig, low, high)
    assert picks[0] == 1024 or len(R.tie_set(l2, g2)[0]) > 1


def test_liar_tile_wraps(engine):
    """B = TPE_JOINT_LIAR_TILE + 2 ids: the last steps stream two tiles of liars."""
    Bw = N.JOINT_LIAR_TILE + 2
    below, above, low, high, psig, cand, l_ref, g_ref = _case(2, 60, 11, 1025)
    rec, sig = engine.run_joint(below, above, low, high, np.arange(Bw), 1025, seed=3, inject=cand, liar=True,
                                return_sigma=True)
    _check_chain('B=%d' % Bw, rec, sig, [cand] * Bw, [l_ref] * Bw, [g_ref] * Bw, above, psig, low, high)


def test_neighbour_scan_loops(engine):
    """K_above = 3000 with D = 2: every scanning thread sweeps the rows 23 times."""
    below, above, low, high, psig, cand, l_ref, g_ref = _case(2, 3013, 5, 1025)
    assert len(above[0]) == 3000
    rec, sig = engine.run_joint(below, above, low, high, [4, 5, 6], 1025, seed=3, inject=cand, liar=True,
                                return_sigma=True)
    _check_chain('K=3000', rec, sig, [cand] * 3, [l_ref] * 3, [g_ref] * 3, above, psig, low, high)


# ------------------------------------------------------------- 5: a sampled run
def test_sampled_run(engine):
    """ids [5, 9, 12] draw their own 4097 candidates: teacher-forced against the
    device's candidates; the same call twice the same bytes; one id is the
    record without the keyword."""
    below, above, low, high, pmu, psig = R.seeded_case(3, 60, 11)
    ids, Cs = [5, 9, 12], 4097
    kw = dict(return_cand=True, want_lg=True, liar=True, return_sigma=True)
    out = engine.run_joint(below, above, low, high, ids, Cs, seed=17, **kw)
    again = engine.run_joint(below, above, low, high, ids, Cs, seed=17, **kw)
    for x, y in zip(out, again):
        assert x.tobytes() == y.tobytes()
    rec, cand, l, g, sig = out
    plain = engine.run_joint(below, above, low, high, ids, Cs, seed=17, return_cand=True, want_lg=True)
    assert cand.tobytes() == plain[1].tobytes() and l.tobytes() == plain[2].tobytes()
    assert g.tobytes() == plain[3].tobytes() and rec[:1].tobytes() == plain[0][:1].tobytes()
    zs = [cand[j].astype(np.float64) for j in range(3)]
    _check_chain('sampled', rec, sig, [cand[j] for j in range(3)], [R.ref_lpdf(z, below, low, high) for z in zs],
                 [R.ref_lpdf(z, above, low, high) for z in zs], above, psig, low, high)
    for j in range(3):
        assert rec['l'][j] == l[j][int(rec['global_idx'][j])]
    one = engine.run_joint(below, above, low, high, [9], Cs, seed=17, liar=True)
    assert one.tobytes() == engine.run_joint(below, above, low, high, [9], Cs, seed=17).tobytes()


# ----------------------------------------------------------- 6: the public path
def _public_case(n_cont):
    from hyperopt_amd import base, hp, rand
    space = {'c': hp.choice('c', [0, 1, 2])}
    kinds = (lambda k: hp.uniform(k, -5, 5), lambda k: hp.loguniform(k, -3, 2), lambda k: hp.normal(k, 0, 2))
    for i in range(n_cont):
        space['x%02d' % i] = kinds[i % 3]('x%02d' % i)
    if n_cont > 3:
        space['q'] = hp.quniform('q', 0, 10, 1)
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = (float(v['x00']) - 1.0) ** 2 + 0.1 * float(v['x02']) ** 2 + 0.1 * int(v['c']) + 1e-3 * tid
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


@pytest.mark.parametrize('n_cont,kw', [(3, {}), (18, {'joint_wide': True})])
def test_public_suggest(n_cont, kw):
    """3 joined labels and a choice (4 labels), then 18 joined labels, a choice
    and a quniform (20 labels, the wide stage)."""
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF
    domain, trials = _public_case(n_cont)
    assert len(domain.table.rows) == (4 if n_cont == 3 else 20)
    Cp, seed, ids = 2048, 321, list(range(40, 48))
    joined = ['x%02d' % i for i in range(n_cont)]
    plain = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=Cp, joint=True, **kw)
    docs = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=Cp, joint=True, joint_liar=True, **kw)
    assert _vals(docs[0]) == _vals(plain[0])                             # id 0 picks as without the keyword
    for doc, ref in zip(docs, plain):
        trials.assert_valid_trial(doc)
        got, want = _vals(doc), _vals(ref)
        assert set(got) == set(want)
        for k in want:
            if k not in joined:                                          # not joined: the same bytes
                assert type(got[k]) is type(want[k]) and got[k] == want[k], k
    assert len(set(tuple(_vals(d)[k] for k in joined) for d in docs)) > 1
    one = tpe.suggest(ids[:1], domain, trials, seed, n_EI_candidates=Cp, joint=True, joint_liar=True, **kw)
    assert _vals(one[0]) == _vals(tpe.suggest(ids[:1], domain, trials, seed, n_EI_candidates=Cp, joint=True, **kw)[0])

    # the joined values are the engine-level picks
    hist = history.extract(domain, trials)
    rows = [domain.table.by_label[k] for k in joined]
    rows.sort(key=lambda r: r.index)
    model = J.fit_model(rows, hist, history.split_below(hist, 0.25), 1.0, DEFAULT_LF)
    engine = get_engine()
    run = engine.run_joint_wide if n_cont > N.JOINT_MAX_DIMS else engine.run_joint
    W = J.side_weight_sum(len(model.above[0]) - 1, 1.0, DEFAULT_LF)
    rec = run(model.below, model.above, model.low, model.high, ids, Cp, seed, liar=W)
    vals = model.values(rec['z'][:, :n_cont])
    for j, doc in enumerate(docs):
        got = _vals(doc)
        for d, r in enumerate(rows):
            assert got[r.label] == vals[j, d], (j, r.label)
    cc = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=Cp, joint=True, joint_liar=True,
                             columns=True, **kw)
    for j, doc in enumerate(docs):
        for lab, v in _vals(doc).items():
            assert cc.values[j, cc.labels.index(lab)] == float(v), (j, lab)
