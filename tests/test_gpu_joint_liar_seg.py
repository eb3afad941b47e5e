"""GPU tests of batch-aware picks in branch groups (tpe_joint_liar_seg through
Engine.run_joint_segments_liar, and tpe.suggest(..., joint_liar='branches')).

The defining property is byte equality: the picks, rows and bandwidths of a
group are those of Engine.run_joint(..., liar=W_s, stream_word=word_s) over that
group's problems, which tests/test_gpu_joint_liar.py checks against the numpy
model.  One test restates that teacher-forced check here (tolerances of
tests/joint_ref.py: g_j within 1e-5 * max(1, |ref|), the winner inside the tie
set, liar_sigma bit for bit)."""
import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_liar_ref as LR
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8
C = 4096
SEED = 3
NARROW = [(3, 60, 11), (2, 3013, 5), (16, 120, 7)]
WORDS = [0x1001, 0x2002, 0x3003, 0x4004]


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


_CASES = {}


def _case(D, n, seed, Cn=C):
    """(below, above, low, high, psig, cand, W), computed once."""
    key = (D, n, seed, Cn)
    if key not in _CASES:
        below, above, low, high, pmu, psig = R.seeded_case(D, n, seed)
        _CASES[key] = (below, above, low, high, psig, LR.candidates(below, low, high, Cn, seed),
                       LR.weight_sum(len(above[0]) - 1))
    return _CASES[key]


_REFS = {}


def _refs(D, n, seed):
    """(l_ref, g_ref) of the case's candidates, computed once."""
    key = (D, n, seed)
    if key not in _REFS:
        below, above, low, high, psig, cand, W = _case(D, n, seed)
        z = cand.astype(np.float64)
        _REFS[key] = R.ref_lpdf(z, below, low, high), R.ref_lpdf(z, above, low, high)
    return _REFS[key]


def _solo(engine, case, word, ids, Cn, seed, inject=True, **kw):
    below, above, low, high, psig, cand, W = case
    return engine.run_joint(below, above, low, high, ids, Cn, seed, liar=W, stream_word=word,
                            inject=cand if inject else None, return_sigma=True, **kw)


def _assert_group_is_the_solo_call(what, rec, sig, ps, D, solo):
    srec, ssig = solo
    for f in ('global_idx', 'l', 'g'):
        assert rec[f][ps].tobytes() == srec[f].tobytes(), (what, f, rec[f][ps], srec[f])
    assert np.ascontiguousarray(rec['z'][ps][:, :D]).tobytes() == np.ascontiguousarray(srec['z'][:, :D]).tobytes(), what
    assert (rec['z'][ps][:, D:] == 0).all(), what
    assert sig.dtype == np.float64 and sig.shape == (len(ps), D), (what, sig.shape)
    assert sig.tobytes() == ssig.tobytes(), (what, sig, ssig)


def _mixed_call():
    """Three groups with chains of 8, 3 and 1 problems, interleaved, and a
    fourth group without a problem."""
    cases = [_case(*c) for c in NARROW] + [_case(2, 30, 1)]
    prob_seg = np.array([0, 1, 0, 2, 0, 1, 0, 0, 1, 0, 0, 0], dtype=np.int32)
    prob_id = np.arange(100, 100 + len(prob_seg))
    models = [c[:4] for c in cases]
    return cases, models, prob_seg, prob_id, [c[5] for c in cases[:3]] + [None], [c[6] for c in cases]


@pytest.fixture(scope='module')
def mixed_run(engine):
    cases, models, prob_seg, prob_id, inject, W = _mixed_call()
    return engine.run_joint_segments_liar(models, WORDS, prob_seg, prob_id, C, SEED, liar=W, inject=inject,
                                          return_sigma=True)


# ------------------------------------------- 1: bit equality, injected candidates
def test_groups_equal_the_solo_liar_stage_bit_for_bit(engine, mixed_run):
    cases, models, prob_seg, prob_id, inject, W = _mixed_call()
    rec, sigs = mixed_run
    assert len(rec) == len(prob_seg) and len(sigs) == 4
    base = engine.run_joint_segments(models, WORDS, prob_seg, prob_id, C, SEED, inject=inject)
    for s in range(3):
        ps = np.flatnonzero(prob_seg == s)
        D = NARROW[s][0]
        _assert_group_is_the_solo_call('group %d' % s, rec, sigs[s], ps, D,
                                       _solo(engine, cases[s], WORDS[s], prob_id[ps], C, SEED))
        assert rec[ps[:1]].tobytes() == base[ps[:1]].tobytes()      # step 0: no liar yet, the stage's own record
    assert len(np.flatnonzero(prob_seg == 2)) == 1                  # the chain of one
    assert sigs[3].shape == (0, 2) and sigs[3].dtype == np.float64  # the group without a problem
    again = engine.run_joint_segments_liar(models, WORDS, prob_seg, prob_id, C, SEED, liar=W, inject=inject,
                                           return_sigma=True)
    assert again[0].tobytes() == rec.tobytes()
    for x, y in zip(again[1], sigs):
        assert x.tobytes() == y.tobytes()
    # liar=True (W_s = 1 / w[-1] of the above side): step 0 of every chain does not read W
    auto = engine.run_joint_segments_liar(models, WORDS, prob_seg, prob_id, C, SEED, inject=inject)
    first = [int(np.flatnonzero(prob_seg == s)[0]) for s in range(3)]
    assert auto[first].tobytes() == base[first].tobytes()


# ------------------------------------------------ 2: the host model, teacher-forced
def _check_chain(what, rec, sig, cand, l_ref, g_ref, above, psig, low, high, W, cap):
    """tests/test_gpu_joint_liar.py's teacher-forced check of one chain over
    shared candidates: step j's reference is built from the device's own
    earlier picks.  Returns the picked indices."""
    chain = LR.Chain(above, psig, low, high, W=W)
    D = cand.shape[1]
    worst, picks = 0.0, []
    for j in range(len(rec)):
        gj = chain.log_g(cand.astype(np.float64), g_ref)
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
        assert sig[j].tobytes() == s.tobytes(), (what, j, sig[j], s)
        picks.append(idx)
    print('%s: worst g_j err / tol = %.3f' % (what, worst))
    return picks


def test_chains_follow_the_host_model(engine, mixed_run):
    """The 8-id chain of the first call, then (3, 60, 11) and (2, 3013, 5) as
    two interleaved 8-id chains of a second call, against tests/joint_liar_ref.
    The cap of MAX_TIES near-ties a step holds for these inputs in
    tests/test_gpu_joint_liar.py, and by the bit equality above the chain here
    is that chain; it cannot be checked on the CPU because every step's
    reference is built from the device's own earlier picks."""
    cases, models, prob_seg, prob_id, inject, W = _mixed_call()
    rec, sigs = mixed_run
    ps = np.flatnonzero(prob_seg == 0)
    below, above, low, high, psig, cand, W0 = cases[0]
    l_ref, g_ref = _refs(*NARROW[0])
    picks = _check_chain('first call, group 0', rec[ps], sigs[0], cand, l_ref, g_ref, above, psig, low, high, W0, True)
    assert len(set(picks)) == 8, picks

    seg2 = np.array([0, 1] * 8, dtype=np.int32)
    ids2 = np.arange(200, 216)
    rec2, sigs2 = engine.run_joint_segments_liar(models[:2], WORDS[:2], seg2, ids2, C, SEED, liar=W[:2],
                                                 inject=inject[:2], return_sigma=True)
    base = engine.run_joint_segments(models[:2], WORDS[:2], seg2, ids2, C, SEED, inject=inject[:2])
    for s in range(2):
        ps = np.flatnonzero(seg2 == s)
        below, above, low, high, psig, cand, Ws = cases[s]
        l_ref, g_ref = _refs(*NARROW[s])
        picks = _check_chain('second call, group %d' % s, rec2[ps], sigs2[s], cand, l_ref, g_ref, above, psig, low,
                             high, Ws, True)
        assert len(set(picks)) == 8, picks
        assert len(set(int(i) for i in base['global_idx'][ps])) == 1    # without the stage: 8 copies of one point


# ---------------------------------------------- 3: sampled candidates, ragged shapes
def test_sampled_candidates_ragged_shapes(engine):
    """C = 1500 (two chunks, the second partial), D = 1, 2, 5, chains of 34 (two
    LDS tiles of liars), 2 and 5, every problem drawing its own candidates: bit
    equality with the solo calls; nothing is checked against the host model."""
    Cs = 1500
    shapes = [(1, 300, 3), (2, 60, 11), (5, 80, 4)]
    cases = [_case(*c, Cn=8) for c in shapes]
    lens = (N.JOINT_LIAR_TILE + 2, 2, 5)
    rs = np.random.RandomState(5)
    prob_seg = rs.permutation(np.repeat(np.arange(3), lens)).astype(np.int32)
    prob_id = 1000 + rs.permutation(len(prob_seg))
    W = [c[6] for c in cases]
    rec, sigs = engine.run_joint_segments_liar([c[:4] for c in cases], WORDS[:3], prob_seg, prob_id, Cs, 17, liar=W,
                                               return_sigma=True)
    for s in range(3):
        ps = np.flatnonzero(prob_seg == s)
        assert len(ps) == lens[s]
        _assert_group_is_the_solo_call('sampled group %d' % s, rec, sigs[s], ps, shapes[s][0],
                                       _solo(engine, cases[s], WORDS[s], prob_id[ps], Cs, 17, inject=False))
    assert (rec['global_idx'] >= 0).all() and (rec['global_idx'] < Cs).all()


# ------------------------------------------------------- 4: want_lg / return_cand
def test_want_lg_and_return_cand_are_the_base_stage(engine):
    cases = [_case(*c, Cn=8) for c in ((2, 60, 11), (3, 60, 11))]
    models = [c[:4] for c in cases]
    prob_seg, prob_id = [1, 0, 1, 1], [4, 5, 6, 7]
    rec, cand, l, g, sigs = engine.run_joint_segments_liar(models, WORDS[:2], prob_seg, prob_id, 1500, 17,
                                                           return_cand=True, want_lg=True, return_sigma=True)
    brec, bcand, bl, bg = engine.run_joint_segments(models, WORDS[:2], prob_seg, prob_id, 1500, 17, return_cand=True,
                                                    want_lg=True)
    assert l.tobytes() == bl.tobytes() and g.tobytes() == bg.tobytes()
    assert len(cand) == len(bcand) == 4
    for x, y in zip(cand, bcand):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    plain = engine.run_joint_segments_liar(models, WORDS[:2], prob_seg, prob_id, 1500, 17)
    assert plain.tobytes() == rec.tobytes()
    assert rec[[1, 0]].tobytes() == brec[[1, 0]].tobytes()           # the first problem of each chain
    for p in range(4):
        i = int(rec['global_idx'][p])
        assert rec['l'][p] == l[p, i] and rec['z'][p, :cand[p].shape[1]].tobytes() == \
            cand[p][i].astype(np.float64).tobytes()


# ----------------------------------------------------------------- 5: public path
def _public_case(branches=True):
    from hyperopt_amd import base, hp, rand
    if branches:
        space = {'clf': hp.choice('classifier', [
            {'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
            {'depth': hp.uniform('rf_depth', 1, 20), 'min_split': hp.uniform('rf_min_split', 0, 1)}]),
            'x': hp.uniform('x', -5, 5)}
    else:
        space = {'c': hp.choice('c', [0, 1, 2]), 'x00': hp.uniform('x00', -5, 5), 'x01': hp.loguniform('x01', -3, 2),
                 'x02': hp.normal('x02', 0, 2)}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = sum((i + 1) * 0.1 * abs(v[k] - 0.5) for i, k in enumerate(sorted(v))) + 1e-3 * tid
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def _same(got, want, keys=None):
    assert set(got) == set(want)
    for k in (want if keys is None else keys):
        assert type(got[k]) is type(want[k]) and got[k] == want[k], (k, got[k], want[k])


def test_public_suggest():
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF
    domain, trials = _public_case()
    Cp, seed, ids = 2048, 321, list(range(40, 48))
    kw = dict(n_EI_candidates=Cp, joint=True, joint_branches=True)
    root, groups = tpe._joint_plan(domain.table, True, 'philox', 'fp32', (None,) * 4, branches=True)
    assert root is None and sorted(sorted(r.label for r in rows) for rows in groups) == \
        [['rf_depth', 'rf_min_split'], ['svm_C', 'svm_gamma']]
    joined = set(r.label for rows in groups for r in rows)
    plain = tpe.suggest(ids, domain, trials, seed, **kw)
    docs = tpe.suggest(ids, domain, trials, seed, joint_liar='branches', **kw)
    hist = history.extract(domain, trials)
    engine = get_engine()
    shared = 0
    for rows in groups:
        labels = [r.label for r in rows]
        js = [j for j, d in enumerate(plain) if labels[0] in _vals(d)]
        assert js == [j for j, d in enumerate(docs) if labels[0] in _vals(d)]      # the gate is univariate
        if not js:
            continue
        _same(_vals(docs[js[0]]), _vals(plain[js[0]]))                # the first id on a branch; an id alone on it
        if len(js) < 2:
            continue
        shared += 1
        rows, model = tpe._fit_branch_model(rows, hist, history.split_below(hist, 0.25), 1.0)
        W = J.side_weight_sum(len(model.above[0]) - 1, 1.0, DEFAULT_LF)
        rec = engine.run_joint(model.below, model.above, model.low, model.high, [ids[j] for j in js], Cp, seed, liar=W,
                               stream_word=J.branch_stream_word(rows))
        vals = model.values(rec['z'][:, :len(rows)])
        for i, j in enumerate(js):
            got = _vals(docs[j])
            for d, r in enumerate(rows):
                assert got[r.label] == vals[i, d], (j, r.label)
        # (every id draws its own candidates, so the plain call's values differ in their bytes too: the values
        # above, not this count, are the check)
        assert len(set(tuple(_vals(docs[j])[k] for k in labels) for j in js)) >= 2
    assert shared >= 1                                               # 8 ids, 2 branches
    for doc, ref in zip(docs, plain):
        trials.assert_valid_trial(doc)
        got, want = _vals(doc), _vals(ref)
        _same(got, want, [k for k in want if k not in joined])       # outside the branch groups: the same bytes
    one = tpe.suggest(ids[:1], domain, trials, seed, joint_liar='branches', **kw)
    _same(_vals(one[0]), _vals(tpe.suggest(ids[:1], domain, trials, seed, **kw)[0]))


def test_public_suggest_without_branch_groups_is_mixed():
    from hyperopt_amd import tpe
    domain, trials = _public_case(branches=False)
    ids = list(range(40, 46))
    kw = dict(n_EI_candidates=2048, joint=True, joint_branches=True)
    a = tpe.suggest(ids, domain, trials, 321, joint_liar='branches', **kw)
    b = tpe.suggest(ids, domain, trials, 321, joint_liar='mixed', **kw)
    for x, y in zip(a, b):
        _same(_vals(x), _vals(y))
    assert len(set(_vals(d)['x00'] for d in a)) > 1
