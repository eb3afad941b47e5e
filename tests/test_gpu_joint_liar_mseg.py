"""GPU tests of batch-aware picks in mixed branch groups (tpe_joint_liar_mseg
through Engine.run_joint_msegments_liar, and tpe.suggest(...,
joint_liar='branches_mixed')).

The defining property is byte equality: the picks, rows and bandwidths of a
group are those of Engine.run_joint_liar_mixed(..., liar=W_s, stream_word=word_s,
centres=centres_s) over that group's problems (a continuous group:
Engine.run_joint), which tests/test_gpu_joint_liar_mixed.py and
tests/test_gpu_joint_liar.py check against the numpy model.  One test restates
the teacher-forced check here (tolerances of tests/joint_ref.py: g_j within 1e-5
* max(1, |ref|), the winner inside the tie set with at most MAX_TIES members,
liar_sigma bit for bit); tests/test_joint_liar_mseg_host.py shows on the CPU that
the reference's own chains keep that cap.  The cases are those of
tests/joint_liar_mixed_ref.py and tests/joint_ref.py: no new reference math."""
import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_liar_mixed_ref as X
from tests import joint_liar_ref as LR
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8
C = 4096
SEED = 3
CONT = (3, 60, 11)                                       # joint_ref.seeded_case: a continuous group
NARROW, DISCRETE, QUANT, ALLQ, LIMITS = X.CASES[:5]
GROUPS = [CONT, NARROW, QUANT, ALLQ, LIMITS, DISCRETE]
WORDS = [0x1001, 0x2002, 0x3003, 0x4004, 0x5005, 0x6006]
# interleaved chains of 2 (continuous), 3 (narrow mixed), 8 (quantised), 1 (all-quantised: a chain of one) and
# 2 (every limit); the all-discrete group has no problem here (it has in the edge tests)
PROB_SEG = np.array([2, 1, 2, 0, 4, 2, 1, 2, 3, 2, 4, 2, 0, 2, 1, 2], dtype=np.int32)
PROB_ID = np.arange(100, 100 + len(PROB_SEG))
CAPPED = ((QUANT, 8), (NARROW, 3))                       # (case, chain length) of the teacher-forced check


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


_CASES = {}


def _case(case, Cn=C, refs=False):
    """One group, computed once: model (what run_joint_segments takes), cand
    [Cn, D], W, centres and, for a mixed case with ``refs``, the dict of
    joint_liar_mixed_ref.case_inputs (its reference l and g)."""
    key = (tuple(case), Cn, refs)
    if key in _CASES:
        return _CASES[key]
    if len(case) == 3:                                   # continuous
        below, above, low, high, pmu, psig = R.seeded_case(*case)
        out = dict(model=(below, above, low, high), cand=LR.candidates(below, low, high, Cn, case[2]), centres=None,
                   W=LR.weight_sum(len(above[0]) - 1), D=case[0], n_sigma=case[0], quants=None)
    else:
        Dc, us, Vs, n, seed = case
        if refs:
            c = X.case_inputs(*case, C=Cn)
        else:
            below, above, low, high, psig, ps, sb, sa, edges = X.seeded_case(*case)
            c = dict(below=below, above=above, low=low, high=high, psig=psig, ps=ps, sb=sb, sa=sa, edges=edges,
                     centres=X.centres_of(Vs), cand=X.candidates(below, low, high, ps, sb, edges, Cn, seed))
        cats = M.cats_of(c['below'], c['above'], c['ps'], c['sb'], c['sa'])
        quants = Q.quants_of(c['below'], c['above'], c['edges'])
        out = dict(model=(c['below'][:3], c['above'][:3], c['low'], c['high'], cats, quants), cand=c['cand'],
                   centres=c['centres'] or None, W=LR.weight_sum(len(c['above'][0]) - 1), D=Dc + len(us) + len(Vs),
                   n_sigma=Dc + len(Vs), quants=quants, c=c)
    _CASES[key] = out
    return out


def _solo(engine, g, word, ids, Cn, seed, inject=True):
    """The defining property's right-hand side: (records, liar_sigma)."""
    cand = g['cand'] if inject else None
    if g['quants'] is None:
        return engine.run_joint(*g['model'], ids, Cn, seed, liar=g['W'], stream_word=word, inject=cand,
                                return_sigma=True)
    return engine.run_joint_liar_mixed(*g['model'], ids, Cn, seed, liar=g['W'], stream_word=word,
                                       centres=g['centres'], inject=cand, return_sigma=True)


def _call(engine, groups, words, prob_seg, prob_id, Cn, seed, inject=True, **kw):
    return engine.run_joint_msegments_liar(
        [g['model'] for g in groups], words, prob_seg, prob_id, Cn, seed, liar=[g['W'] for g in groups],
        centres=[g['centres'] for g in groups], inject=[g['cand'] for g in groups] if inject else None,
        return_sigma=True, **kw)


def _assert_group_is_the_solo_call(what, rec, sig, ps, g, solo):
    srec, ssig = solo
    D = g['D']
    for f in ('global_idx', 'l', 'g'):
        assert rec[f][ps].tobytes() == srec[f].tobytes(), (what, f, rec[f][ps], srec[f])
    assert np.ascontiguousarray(rec['z'][ps][:, :D]).tobytes() == np.ascontiguousarray(srec['z'][:, :D]).tobytes(), what
    assert (rec['z'][ps][:, D:] == 0).all(), what
    assert sig.dtype == np.float64 and sig.shape == (len(ps), g['n_sigma']), (what, sig.shape)
    assert sig.tobytes() == ssig.tobytes(), (what, sig, ssig)


def _assert_all_groups(what, engine, groups, words, prob_seg, prob_id, Cn, seed, rec, sigs, inject=True):
    prob_seg, prob_id = np.asarray(prob_seg), np.asarray(prob_id)
    for s, g in enumerate(groups):
        ps = np.flatnonzero(prob_seg == s)
        if len(ps) == 0:
            assert sigs[s].shape == (0, g['n_sigma']) and sigs[s].dtype == np.float64
            continue
        _assert_group_is_the_solo_call('%s, group %d' % (what, s), rec, sigs[s], ps, g,
                                       _solo(engine, g, words[s], prob_id[ps], Cn, seed, inject))


def _main_groups():
    return [_case(c, refs=any(c == k for k, _ in CAPPED)) for c in GROUPS]


@pytest.fixture(scope='module')
def main_run(engine):
    return _call(engine, _main_groups(), WORDS, PROB_SEG, PROB_ID, C, SEED)


# ------------------------------------------- 1: byte equality, injected candidates
def test_groups_equal_the_solo_liar_stages_byte_for_byte(engine, main_run):
    groups = _main_groups()
    rec, sigs = main_run
    assert len(rec) == len(PROB_SEG) and len(sigs) == len(GROUPS)
    assert np.bincount(PROB_SEG, minlength=6).tolist() == [2, 3, 8, 1, 2, 0]
    _assert_all_groups('main', engine, groups, WORDS, PROB_SEG, PROB_ID, C, SEED, rec, sigs)
    base = engine.run_joint_segments([g['model'] for g in groups], WORDS, PROB_SEG, PROB_ID, C, SEED,
                                     inject=[g['cand'] for g in groups])
    first = [int(np.flatnonzero(PROB_SEG == s)[0]) for s in range(5)]
    assert rec[first].tobytes() == base[first].tobytes()             # step 0: no liar yet, the stage's own record
    again = _call(engine, groups, WORDS, PROB_SEG, PROB_ID, C, SEED)
    assert again[0].tobytes() == rec.tobytes()
    for x, y in zip(again[1], sigs):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------ 2: the host model, teacher-forced
def _check_chain(what, c, rec, sig, W):
    """tests/test_gpu_joint_liar_mixed.py's teacher-forced check of one chain over
    shared candidates, with the cap: step j's reference is built from the
    device's own earlier picks.  Returns the picked indices."""
    chain = X.chain_of(c, W=W)
    cand, l_ref, g_ref = c['cand'], c['l'], c['g']
    D = cand.shape[1]
    assert sig.shape == (len(rec), chain.Dc + chain.Dq) and sig.dtype == np.float64
    worst, picks = 0.0, []
    for j in range(len(rec)):
        gj = chain.log_g(cand, g_ref)
        idx = int(rec['global_idx'][j])
        assert 0 <= idx < len(cand), (what, j, idx)
        worst = max(worst, R.check_lpdf(np.array([rec['g'][j]]), gj[idx:idx + 1], '%s g_%d' % (what, j)))
        R.check_lpdf(np.array([rec['l'][j]]), l_ref[idx:idx + 1], '%s l_%d' % (what, j))
        ties, score = R.tie_set(l_ref, gj)
        print('%s step %d: winner %d, argmax %d, %d ties' % (what, j, idx, int(np.argmax(score)), len(ties)))
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


def test_chains_follow_the_host_model(main_run):
    groups = _main_groups()
    rec, sigs = main_run
    for case, L in CAPPED:
        s = GROUPS.index(case)
        ps = np.flatnonzero(PROB_SEG == s)
        assert len(ps) == L
        picks = _check_chain(str(case), groups[s]['c'], rec[ps], sigs[s], groups[s]['W'])
        assert len(set(picks)) == L, picks


# ---------------------------------------------------------------------- 3: edges
def test_ragged_second_chunk(engine):
    """C = 1025: the second chunk holds one candidate."""
    groups = [_case(QUANT, 1025), _case(CONT, 1025), _case(DISCRETE, 1025)]
    prob_seg, prob_id = [0, 1, 0, 2, 0, 1, 0, 2], np.arange(8)
    rec, sigs = _call(engine, groups, WORDS[:3], prob_seg, prob_id, 1025, SEED)
    _assert_all_groups('C=1025', engine, groups, WORDS[:3], prob_seg, prob_id, 1025, SEED, rec, sigs)


def test_liar_tile_wraps(engine):
    """A chain of 40 over C = 1024: its last steps stream two tiles of liars,
    while the chain of 2 beside it has long ended."""
    Lw = 40
    assert Lw > N.JOINT_LIAR_TILE
    groups = [_case(DISCRETE, 1024), _case(QUANT, 1024)]
    prob_seg = np.array([1] * 5 + [0] + [1] * 20 + [0] + [1] * 15, dtype=np.int32)
    prob_id = np.arange(len(prob_seg))
    rec, sigs = _call(engine, groups, WORDS[:2], prob_seg, prob_id, 1024, SEED)
    assert sigs[1].shape == (Lw, 2) and sigs[0].shape == (2, 0)
    _assert_all_groups('chain of 40', engine, groups, WORDS[:2], prob_seg, prob_id, 1024, SEED, rec, sigs)


def test_a_candidate_every_liar_term_leaves_at_minus_infinity(engine):
    """joint_liar_mixed_ref.far_bin_case as a chain of 2 over two injected rows:
    the row at lattice index 0 wins step 0 by a wide margin, its liar has
    both neighbours within one bin, so sigma is the floor psig / 100 = 2.55
    and the bin of the row at index 255 has mass exactly 0: that row is pick 1
    with g_1 = g - log1p(1 / W), finite."""
    c = X.far_bin_case()
    cand = np.array([[0.0], [255.0]], dtype=np.float32)
    l = X.base_lpdf(cand, c['below'], c['low'], c['high'], [], [], c['edges'])
    g = X.base_lpdf(cand, c['above'], c['low'], c['high'], [], [], c['edges'])
    W = LR.weight_sum(len(c['above'][0]) - 1)
    chain = X.chain_of(c, W=W)
    steps = X.greedy(chain, cand, l, g, 2)
    assert [s[3] for s in steps] == [0, 1] and all(len(s[1]) == 1 for s in steps)       # the reference alone
    assert np.isneginf(chain.log_kernels(cand)[1, 0])
    model = (c['below'][:3], c['above'][:3], c['low'], c['high'], [], Q.quants_of(c['below'], c['above'], c['edges']))
    rec, sigs = engine.run_joint_msegments_liar([model], [0x77], [0, 0], [7, 8], 2, SEED, liar=[W],
                                                centres=[c['centres']], inject=[cand], return_sigma=True)
    assert rec['global_idx'].tolist() == [0, 1] and np.isfinite(rec['g']).all() and np.isfinite(rec['l']).all()
    R.check_lpdf(rec['g'][1:], np.array([g[1] - np.log1p(1.0 / W)]), 'far bin g_1')
    assert sigs[0][0].tolist() == [2.55]


def test_only_continuous_groups_are_run_joint_segments_liar(engine):
    groups = [_case(CONT, 1025), _case((2, 60, 11), 1025)]
    prob_seg, prob_id = [1, 0, 1, 1, 0], [4, 5, 6, 7, 8]
    rec, sigs = _call(engine, groups, WORDS[:2], prob_seg, prob_id, 1025, SEED)
    ref, rsigs = engine.run_joint_segments_liar([g['model'] for g in groups], WORDS[:2], prob_seg, prob_id, 1025, SEED,
                                                liar=[g['W'] for g in groups], inject=[g['cand'] for g in groups],
                                                return_sigma=True)
    assert rec.tobytes() == ref.tobytes()
    for x, y in zip(sigs, rsigs):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


# ------------------------------------------------------------------ 4: sampled run
def test_sampled_run(engine):
    """No inject: every problem draws its own 4097 candidates."""
    Cs = 4097
    groups = [_case(QUANT, 8), _case(NARROW, 8), _case(CONT, 8), _case(ALLQ, 8)]
    prob_seg, prob_id = [0, 1, 2, 0, 3, 1, 0, 2], [5, 9, 12, 40, 41, 42, 43, 1000]
    rec, sigs = _call(engine, groups, WORDS[:4], prob_seg, prob_id, Cs, 17, inject=False)
    assert (rec['global_idx'] >= 0).all() and (rec['global_idx'] < Cs).all()
    _assert_all_groups('sampled', engine, groups, WORDS[:4], prob_seg, prob_id, Cs, 17, rec, sigs, inject=False)
    plain = engine.run_joint_msegments_liar([g['model'] for g in groups], WORDS[:4], prob_seg, prob_id, Cs, 17,
                                            liar=[g['W'] for g in groups], centres=[g['centres'] for g in groups])
    assert plain.tobytes() == rec.tobytes()


# ----------------------------------------------------------------- 5: public path
KW = dict(n_EI_candidates=4096, joint=True, joint_discrete=True, joint_quantized=True, joint_branches=True,
          joint_branches_mixed=True)


def _public_case(mixed=True):
    from hyperopt_amd import base, hp, rand
    if mixed:                                            # README's rf / knn tree
        space = {'model': hp.choice('model', [
            {'name': 'rf', 'n_est': hp.quniform('rf_n_est', 10, 500, 10),
             'crit': hp.choice('rf_crit', ['gini', 'entropy'])},
            {'name': 'knn', 'k': hp.quniform('knn_k', 1, 50, 1), 'p': hp.uniform('knn_p', 1, 3)}])}
    else:
        space = {'clf': hp.choice('classifier', [
            {'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
            {'depth': hp.uniform('rf_depth', 1, 20), 'min_split': hp.uniform('rf_min_split', 0, 1)}]),
            'x': hp.uniform('x', -5, 5)}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: float(x[0]) for k, x in docs[0]['misc']['vals'].items() if len(x)}
        if mixed:
            loss = (abs(v['rf_n_est'] - 200.0) / 500.0 + 0.1 * v['rf_crit'] if 'rf_n_est' in v
                    else (v['knn_k'] - 7.0) ** 2 / 500.0 + 0.2 * (v['knn_p'] - 2.0) ** 2) + 1e-3 * tid
        else:
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


def test_public_suggest_on_the_readme_tree():
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF
    domain, trials = _public_case()
    seed, ids = 321, list(range(60, 68))
    root, groups = tpe._joint_plan(domain.table, True, 'philox', 'fp32', (None,) * 4, True, True, branches=True,
                                   branch_mixed=True)
    assert root is None and sorted(sorted(r.label for r in rows) for rows in groups) == \
        [['knn_k', 'knn_p'], ['rf_crit', 'rf_n_est']]
    joined = set(r.label for rows in groups for r in rows)
    plain = tpe.suggest(ids, domain, trials, seed, **KW)
    docs = tpe.suggest(ids, domain, trials, seed, joint_liar='branches_mixed', **KW)
    with pytest.raises(ValueError, match='discrete or quantised'):
        tpe.suggest(ids, domain, trials, seed, joint_liar='branches', **KW)
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
        assert isinstance(model, J.QuantModel)
        W = J.side_weight_sum(len(model.above[0]) - 1, 1.0, DEFAULT_LF)
        rec = engine.run_joint_liar_mixed(model.below[:3], model.above[:3], model.low, model.high, model.cats(),
                                          model.quants(), [ids[j] for j in js], KW['n_EI_candidates'], seed, liar=W,
                                          centres=model.centres(), stream_word=J.branch_stream_word(rows))
        vals = model.values(rec['z'][:, :len(rows)])
        for i, j in enumerate(js):
            got = _vals(docs[j])
            for d, r in enumerate(rows):
                assert got[r.label] == vals[i, d], (j, r.label)
        with_kw = [tuple(_vals(docs[j])[k] for k in labels) for j in js]
        without = [tuple(_vals(plain[j])[k] for k in labels) for j in js]
        print('%s: %d ids, %d distinct vectors with the keyword, %d without' % (labels, len(js), len(set(with_kw)),
                                                                              len(set(without))))
        assert len(set(with_kw)) == len(js), with_kw                  # pairwise distinct group vectors
    assert shared >= 1                                               # 8 ids, 2 branches
    for doc, ref in zip(docs, plain):
        trials.assert_valid_trial(doc)
        got, want = _vals(doc), _vals(ref)
        _same(got, want, [k for k in want if k not in joined])       # outside the branch groups: the same bytes
    one = tpe.suggest(ids[:1], domain, trials, seed, joint_liar='branches_mixed', **KW)
    _same(_vals(one[0]), _vals(tpe.suggest(ids[:1], domain, trials, seed, **KW)[0]))


def test_public_suggest_on_a_continuous_tree_is_branches():
    from hyperopt_amd import tpe
    domain, trials = _public_case(mixed=False)
    ids = list(range(60, 68))
    kw = dict(n_EI_candidates=2048, joint=True, joint_branches=True)
    a = tpe.suggest(ids, domain, trials, 321, joint_liar='branches_mixed', **kw)
    b = tpe.suggest(ids, domain, trials, 321, joint_liar='branches', **kw)
    for x, y in zip(a, b):
        _same(_vals(x), _vals(y))
