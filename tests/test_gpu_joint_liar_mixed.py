"""GPU tests of batch-aware picks over discrete and quantised labels
(tpe_joint_liar_mixed through Engine.run_joint_liar_mixed after the narrow mixed,
wide mixed or quantised stage, and tpe.suggest(..., joint_liar='mixed')) against
the model restated in numpy (tests/joint_liar_mixed_ref.py).

Tolerances are the project's (tests/joint_ref.py): g_j and l within 1e-5 *
max(1, |ref|); the winner inside the tie set (4 of those bounds) and equal to
np.argmax when that set has one member; the winner's row and liar_sigma bit for
bit.  Every winner check is teacher-forced: step j's reference is built from
the device's own earlier picks.  The all-discrete group's rows repeat, and
equal rows score equally by construction: it is exempt from the tie cap and
from distinct picks, and is checked for tie-set membership only.
"""
import ctypes

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
B = 8
C = 4096
QUANT = X.CASES[2]                                       # (1, (2,), (5,), 80): a row is [z, category, lattice index]


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


_CASES = {}


def _case(case, C=C):
    key = tuple(case) + (C,)
    if key not in _CASES:
        _CASES[key] = X.case_inputs(*case, C=C)
    return _CASES[key]


def _run(engine, c, ids, n_cand, **kw):
    """With ``liar``: Engine.run_joint_liar_mixed; without: the stage the group
    goes to (quantised, wide mixed or narrow mixed)."""
    cats = M.cats_of(c['below'], c['above'], c['ps'], c['sb'], c['sa'])
    quants = Q.quants_of(c['below'], c['above'], c['edges'])
    D = c['above'][1].shape[1] + len(c['ps']) + len(c['edges'])
    kw.setdefault('seed', 3)
    seed = kw.pop('seed')
    head = (c['below'][:3], c['above'][:3], c['low'], c['high'], cats)
    if kw.get('liar', False) is not False:
        return engine.run_joint_liar_mixed(*head, quants, ids, n_cand, seed, centres=c['centres'] or None, **kw)
    if c['edges']:
        return engine.run_joint_quant(*head, quants, ids, n_cand, seed, **kw)
    run = engine.run_joint_wide_mixed if D > N.JOINT_MAX_DIMS else engine.run_joint_mixed
    return run(*head, ids, n_cand, seed, **kw)


def _check_chain(what, c, rec, sig, cands, l_refs, g_refs, given=None, cap=False, W=None):
    """Teacher-forced check of one liar call: ``cands`` / ``l_refs`` / ``g_refs``
    one entry per id (the same object for shared candidates).  Returns the
    picked indices and the worst g_j error over tolerance."""
    chain = X.chain_of(c, W=W, given=given)
    G = len(chain.cat)
    D = cands[0].shape[1]
    assert sig.shape == (G + len(rec), chain.Dc + chain.Dq) and sig.dtype == np.float64
    if G:
        assert sig[:G].tobytes() == chain.sigmas.tobytes(), (what, 'given sigma')
    worst, picks = 0.0, []
    for j in range(len(rec)):
        cand, l_ref = cands[j], l_refs[j]
        gj = chain.log_g(cand, g_refs[j])
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


# ------------------------------------------------------- the seven cases, B = 8
@pytest.mark.parametrize('case', X.CASES)
def test_greedy_batch_of_injected_candidates(engine, case):
    """8 ids over 4096 shared candidates: g_j, the tie set with its cap, distinct
    picks, the winner's row and liar_sigma bit for bit; without ``liar`` one
    index for all ids, pick 0 is that record's bytes, and want_lg returns the
    base l and g.  The all-discrete group: tie-set membership only."""
    c = _case(case)
    all_discrete = case[0] == 0 and not case[2]
    if case[3] == 3013:
        assert len(c['above'][0]) == 3000
    ids = np.arange(100, 100 + B)
    rec, l, g, sig = _run(engine, c, ids, C, inject=c['cand'], want_lg=True, liar=True, return_sigma=True)
    base, l0, g0 = _run(engine, c, ids, C, inject=c['cand'], want_lg=True)
    assert len(set(int(i) for i in base['global_idx'])) == 1            # the problem: B copies of one point
    assert rec[:1].tobytes() == base[:1].tobytes()                      # pick 0: the solo record, byte for byte
    assert l.tobytes() == l0.tobytes() and g.tobytes() == g0.tobytes()  # want_lg: the base l and g
    picks, _ = _check_chain(str(case), c, rec, sig, [c['cand']] * B, [c['l']] * B, [c['g']] * B, cap=not all_discrete)
    if not all_discrete:
        assert len(set(picks)) == B, picks


# ------------------------------------------------------------------ given rows
def _run_given(engine, given, case=QUANT, W=None):
    c = _case(case, 2048)
    given = np.asarray(given, dtype=np.float32).reshape(-1, c['cand'].shape[1])
    rec, sig = _run(engine, c, [1, 2], 2048, inject=c['cand'], liar=True if W is None else W, given=given,
                    return_sigma=True)
    _check_chain('given %s' % (given.tolist(),), c, rec, sig, [c['cand']] * 2, [c['l']] * 2, [c['g']] * 2, given=given,
                 W=W)
    return sig, c


def test_given_first_and_last_category_and_lattice_index(engine):
    """Categories 0 and U - 1, lattice indices 0 and V - 1."""
    _run_given(engine, [[0.5, 0, 0], [-1.5, 1, 4]])


def test_given_centre_equal_to_an_existing_qmu(engine):
    c = _case(QUANT, 2048)
    assert 2.0 in c['above'][4][:, 0]                     # a trial of the above side observed lattice value 2
    sig, _ = _run_given(engine, [[0.25, 1, 2]])
    assert (sig[0] > 0).all()


def test_given_equal_to_an_earlier_given_row(engine):
    _run_given(engine, [[1.25, 0, 3], [1.25, 0, 3], [1.25, 0, 3]])       # the twin sees its twin as L = c


def test_given_with_few_trials(engine):
    """One trial on the above side: m + 2 < 100, the floor of the clip moves with every liar."""
    case = (1, (2,), (5,), 2, 1)
    c = _case(case, 2048)
    assert len(c['above'][0]) - 1 == 1
    _run_given(engine, [[0.5, 1, 1], [0.5, 1, 1], [0.0, 0, 4]], case=case, W=LR.weight_sum(1))


# ------------------------------------------------------------------ loop edges
def test_ragged_second_chunk(engine):
    """C = 1025: the second chunk holds one candidate."""
    c = _case(QUANT, 1025)
    rec, sig = _run(engine, c, [0, 1, 2, 3], 1025, inject=c['cand'], liar=True, return_sigma=True)
    _check_chain('C=1025', c, rec, sig, [c['cand']] * 4, [c['l']] * 4, [c['g']] * 4)
    # the candidate alone in the second chunk must be able to win: move the winner's row there
    w, worst = int(rec['global_idx'][0]), int(np.argmin(c['l'] - c['g']))
    cand2, l2, g2 = c['cand'].copy(), c['l'].copy(), c['g'].copy()
    for arr in (cand2, l2, g2):
        arr[-1], arr[w] = arr[w].copy(), arr[worst].copy()
    assert 1024 in R.tie_set(l2, g2)[0]
    rec2, sig2 = _run(engine, c, [0, 1], 1025, inject=cand2, liar=True, return_sigma=True)
    picks, _ = _check_chain('C=1025, last row best', c, rec2, sig2, [cand2] * 2, [l2] * 2, [g2] * 2)
    assert picks[0] == 1024 or len(R.tie_set(l2, g2)[0]) > 1


def test_liar_tile_wraps(engine):
    """B = 40 ids over C = 1024: the last steps stream two tiles of liars."""
    Bw = 40
    assert Bw > N.JOINT_LIAR_TILE
    c = _case(QUANT, 1024)
    rec, sig = _run(engine, c, np.arange(Bw), 1024, inject=c['cand'], liar=True, return_sigma=True)
    _check_chain('B=%d' % Bw, c, rec, sig, [c['cand']] * Bw, [c['l']] * Bw, [c['g']] * Bw)


def test_a_candidate_every_liar_term_leaves_at_minus_infinity(engine):
    """tests/test_joint_liar_mixed_host.py's far bin on the device: candidate 0
    (lattice index 255) under the given liar at index 0 of sigma psig / 100.
    Alone in the pool it is the pick, and its g_1 = g - log1p(1 / W): finite."""
    c = X.far_bin_case()
    given = np.zeros((1, 1), dtype=np.float32)
    chain = X.chain_of(c, given=given)
    assert np.isneginf(chain.log_kernels(c['cand'])[0]).all()
    rec, sig = _run(engine, c, [7], 1, inject=c['cand'][:1], liar=True, given=given, return_sigma=True)
    assert int(rec['global_idx'][0]) == 0 and np.isfinite(rec['g'][0]) and np.isfinite(rec['l'][0])
    R.check_lpdf(rec['g'][:1], np.array([c['g'][0] - np.log1p(1.0 / chain.W)]), 'far bin g_1')
    assert sig[0].tolist() == [2.55]
    n = len(c['cand'])
    rec, sig = _run(engine, c, [7, 8, 9], n, inject=c['cand'], liar=True, given=given, return_sigma=True)
    assert np.isfinite(rec['g']).all()
    _check_chain('far bin', c, rec, sig, [c['cand']] * 3, [c['l']] * 3, [c['g']] * 3, given=given)


# --------------------------------------------------------------- a sampled run
def test_sampled_run(engine):
    """ids [5, 9, 12] draw their own 4097 candidates: teacher-forced against the
    device's candidates; the same call twice the same bytes; one id is the
    record without the keyword."""
    c = _case(QUANT, 64)
    ids, Cs = [5, 9, 12], 4097
    kw = dict(return_cand=True, want_lg=True, liar=True, return_sigma=True, seed=17)
    out = _run(engine, c, ids, Cs, **dict(kw))
    again = _run(engine, c, ids, Cs, **dict(kw))
    for x, y in zip(out, again):
        assert x.tobytes() == y.tobytes()
    rec, cand, l, g, sig = out
    plain = _run(engine, c, ids, Cs, return_cand=True, want_lg=True, seed=17)
    assert cand.tobytes() == plain[1].tobytes() and l.tobytes() == plain[2].tobytes()
    assert g.tobytes() == plain[3].tobytes() and rec[:1].tobytes() == plain[0][:1].tobytes()
    l_refs = [X.base_lpdf(cand[j], c['below'], c['low'], c['high'], c['ps'], c['sb'], c['edges']) for j in range(3)]
    g_refs = [X.base_lpdf(cand[j], c['above'], c['low'], c['high'], c['ps'], c['sa'], c['edges']) for j in range(3)]
    _check_chain('sampled', c, rec, sig, [cand[j] for j in range(3)], l_refs, g_refs)
    for j in range(3):
        assert rec['l'][j] == l[j][int(rec['global_idx'][j])]
    one = _run(engine, c, [9], Cs, liar=True, seed=17)
    assert one.tobytes() == _run(engine, c, [9], Cs, seed=17).tobytes()


# ------------------------------------------ no discrete or quantised label at all
def test_continuous_group_through_the_new_entry_is_tpe_joint_liar(engine):
    """n_cat = n_quant = 0: tpe_joint_liar_mixed over the buffers of a continuous
    stage gives the bytes of tpe_joint_liar, which are run_joint(..., liar=True)'s."""
    import torch
    D, Cn, P = 3, 2048, 4
    below, above, low, high, pmu, psig = R.seeded_case(D, 60, 11)
    cand = LR.candidates(below, low, high, Cn, 11)
    W = LR.weight_sum(len(above[0]) - 1)
    rec, l, g, sig = engine.run_joint(below, above, low, high, np.arange(P), Cn, seed=3, inject=cand, want_lg=True,
                                      liar=W, return_sigma=True)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
           (np.tile(cand[None], (P, 1, 1)), l, g, np.asarray(above[1], dtype=np.float32))]
    lib = N.load()
    outs = []
    for fn, struct in ((lib.tpe_joint_liar, N.JointLiarArgs), (lib.tpe_joint_liar_mixed, N.JointLiarMixedArgs)):
        a = struct()
        a.n_dims, a.n_cand, a.n_ids, a.n_given = D, Cn, P, 0
        a.k_above, a.n_trials, a.w_sum = len(above[0]), len(above[0]) - 1, W
        a.cand, a.l_out, a.g_out, a.above_mu = (t.data_ptr() for t in dev)
        for d in range(D):
            a.psig[d], a.low[d], a.high[d] = psig[d], low[d], high[d]
        nb = ctypes.c_uint64(0)
        assert lib.tpe_joint_liar_scratch_bytes(P, Cn, D, 0, ctypes.byref(nb)) == 0
        scr = torch.zeros((nb.value + 7) // 8, dtype=torch.float64, device='cuda')
        picks = torch.zeros(P * 3, dtype=torch.float64, device='cuda')
        z = torch.zeros(P * D, dtype=torch.float32, device='cuda')
        s = torch.zeros(P * D, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        N.check(fn(ctypes.byref(a), picks.data_ptr(), z.data_ptr(), s.data_ptr(), scr.data_ptr(), scr.numel() * 8,
                   None), lib, 'liar entry')
        torch.cuda.synchronize()
        outs.append((picks.cpu().numpy().tobytes(), z.cpu().numpy().tobytes(), s.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    picks = np.frombuffer(outs[1][0], dtype=N.JOINT_PICK_DTYPE)
    assert (picks['idx'] == rec['global_idx']).all() and picks['l'].tobytes() == rec['l'].tobytes()
    assert picks['g'].tobytes() == rec['g'].tobytes() and outs[1][2] == sig.tobytes()


# ------------------------------------------------------------- the public path
def _public_case():
    from hyperopt_amd import base, hp, rand
    space = {'x00': hp.uniform('x00', -5, 5), 'x01': hp.loguniform('x01', -3, 2), 'x02': hp.normal('x02', 0, 2),
             'c': hp.choice('c', [0, 1, 2]), 'q': hp.quniform('q', 0, 10, 2),
             'g': hp.choice('g', [{'a': hp.uniform('a', 0, 1)}, {'u': hp.normal('u', 0, 1), 'k': hp.randint('k', 4)}])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = ((float(v['x00']) - 1.0) ** 2 + 0.1 * float(v['x02']) ** 2 + 0.1 * int(v['c']) + 0.02 * float(v['q'])
                + 1e-3 * tid)
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_suggest():
    """3 continuous labels, a choice and a quniform joined; a conditional subtree
    outside the group."""
    from hyperopt_amd import tpe
    domain, trials = _public_case()
    Cp, seed, ids = 2048, 321, list(range(40, 48))
    joined = ['x00', 'x01', 'x02', 'c', 'q']
    kw = dict(n_EI_candidates=Cp, joint=True, joint_discrete=True, joint_quantized=True)
    plain = tpe.suggest(ids, domain, trials, seed, **kw)
    docs = tpe.suggest(ids, domain, trials, seed, joint_liar='mixed', **kw)
    assert _vals(docs[0]) == _vals(plain[0])                             # id 0 picks as without the keyword
    for a, b in _vals(docs[0]).items():
        assert type(b) is type(_vals(plain[0])[a])
    for doc, ref in zip(docs, plain):
        trials.assert_valid_trial(doc)
        got, want = _vals(doc), _vals(ref)
        assert set(got) == set(want)
        for k in want:
            if k not in joined:                                          # not joined: the same bytes
                assert type(got[k]) is type(want[k]) and got[k] == want[k], k
        assert isinstance(got['c'], np.int64) and 0 <= got['c'] < 3
        assert got['q'] in (0.0, 2.0, 4.0, 6.0, 8.0, 10.0)               # a multiple of q
    assert len(set(tuple(_vals(d)[k] for k in joined) for d in docs)) == len(ids)
    one = tpe.suggest(ids[:1], domain, trials, seed, joint_liar='mixed', **kw)
    ref = tpe.suggest(ids[:1], domain, trials, seed, **kw)
    assert _vals(one[0]) == _vals(ref[0]) and [type(v) for v in _vals(one[0]).values()] == \
        [type(v) for v in _vals(ref[0]).values()]
    with pytest.raises(ValueError, match='discrete or quantised'):
        tpe.suggest(ids, domain, trials, seed, joint_liar=True, **kw)


def test_public_suggest_on_a_continuous_group_is_true():
    """On a root group of continuous labels only 'mixed' is True, byte for byte."""
    from hyperopt_amd import tpe
    domain, trials = _public_case()
    kw = dict(n_EI_candidates=1024, joint=['x00', 'x01', 'x02'])
    a = tpe.suggest(list(range(40, 44)), domain, trials, 5, joint_liar=True, **kw)
    b = tpe.suggest(list(range(40, 44)), domain, trials, 5, joint_liar='mixed', **kw)
    for x, y in zip(a, b):
        assert _vals(x) == _vals(y) and [type(v) for v in _vals(x).values()] == [type(v) for v in _vals(y).values()]
