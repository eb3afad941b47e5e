"""GPU tests of the large-lattice joint stage (Engine.run_joint_quant_large) at
the limits of its sizes, tiles and draws: lattices of 65,536 values, three and
four quantised labels, above sides of 296 components and of one, candidate
counts 1 / 1024 / 1025, exact ties, the sampler above 256 values, and the
public path.  References and tolerances are the project's: the float64 model
(tests/joint_quant_ref.py), l and g within 1e-5 * max(1, |ref|) (joint_ref.
check_lpdf), the winner inside joint_ref.tie_set with at most MAX_TIES distinct
vectors (check_quant_winner).  Every builder asserts the tie cap and the
finiteness of its references from the float64 model alone, before a device is
used."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R
from tests.test_gpu_joint_quant import MAX_TIES, check_quant_winner, quant_candidates
from tests.test_gpu_joint_quant_large import QLOG, _args, _qlog_side

pytestmark = pytest.mark.gpu

C3 = 2048 + 37                      # two full chunks and a ragged one


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _refs(case, cand, what):
    """(l_ref, g_ref) of cand [C, Dc + Dk + Dq] under the float64 model, with the
    conditions on the inputs: finite references, at most MAX_TIES distinct tied vectors."""
    below, above, low, high, ps, sb, sa, edges = case[:8]
    Dc, q0 = below[1].shape[1], below[1].shape[1] + len(ps)
    z64, v, qi = cand[:, :Dc].astype(np.float64), cand[:, Dc:q0].astype(np.int64), cand[:, q0:].astype(np.int64)
    l_ref = Q.ref_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges)
    g_ref = Q.ref_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges)
    assert np.isfinite(l_ref).all() and np.isfinite(g_ref).all(), what
    ties, _ = R.tie_set(l_ref, g_ref)
    assert len(np.unique(cand[ties], axis=0)) <= MAX_TIES, (what, len(ties))
    return l_ref, g_ref


# ------------------------------------------- injected candidates, float64 model
# name -> (Dc, us, Vs, n trials, how the candidates' lattice indices are set, cut the above side to its prior row)
EDGE_CASES = {
    # indices 0, 32767, 32768 and 65535 as uint16 in the chunk's index list; the key 65535 << 10
    'V65536': (1, (), (65536,), 60, 'ends', False),
    # the second chunk holds 4 x 1,024 distinct rows: n_total = 4096 -> tile 4, stride 8, 139,312 B of dynamic LDS;
    # the wave carry of the run numbering crosses all four waves in every dimension
    'four_large_distinct': (0, (), (65536, 3000, 1500, 1100), 60, 'distinct', False),
    # Dq = 3 in the QP = 4 instantiation (the padded slot reads the zero row), a large and two small lattices beside a
    # choice and two continuous labels; ka = 296: a chunk's tile loop wraps and ends on a tail of nk % 4 != 0
    'three_padded': (2, (3,), (2000, 300, 17), 300, None, False),
    # the second chunk has one mini-table row: tile 128, segs = 2, tiles of 128, 128 and 40 components (segs = 6)
    'K300_one_bin': (1, (), (3000,), 300, 'one', False),
    # three_padded with the above side cut to its prior row: K = 1, nk4 = 4, segs = 64, three padded components
    'one_above': (2, (3,), (2000, 300, 17), 300, None, True),
}


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(below, above, low, high, ps, s_below, s_above, edges, cand, l_ref, g_ref), computed once."""
    Dc, us, Vs, n, how, cut = EDGE_CASES[name]
    below, above, low, high, ps, sb, sa, edges, rs = Q.seeded_quant_case(Dc, list(us), list(Vs), n)
    if cut:
        above = (np.ones(1),) + tuple(x[:1] for x in above[1:])
    cand = quant_candidates(below, low, high, ps, edges, C3, 7)
    q0 = Dc + len(us)
    for d, V in enumerate(Vs):
        col = cand[:, q0 + d]
        if how == 'ends':
            col[[0, 1, 2, 3, 1030, 1031]] = [0.0, V - 1.0, 32767.0, 32768.0, V - 1.0, 0.0]
        elif how == 'distinct':
            col[1024:2048] = rs.permutation(V)[:1024]
        elif how == 'one':
            col[1024:2048] = 1234.0
    case = (below, above, low, high, ps, sb, sa, edges)
    return case + (cand,) + _refs(case, cand, name)


def check_edge_case_shape(name):
    """The branch the case is there for, read from its inputs alone."""
    case = edge_case(name)
    Dc, us, Vs, n, how, cut = EDGE_CASES[name]
    above, cand, q0 = case[1], case[8], Dc + len(us)
    assert cand.shape == (C3, q0 + len(Vs))
    if cut or n == 300:
        assert len(above[0]) == (1 if cut else 296)
    if how == 'ends':
        assert set([0.0, 32767.0, 32768.0, 65535.0]) <= set(cand[:1024, q0]) and cand[:, q0].max() == 65535.0
    if how == 'distinct':
        for d in range(len(Vs)):
            assert len(np.unique(cand[1024:2048, q0 + d])) == 1024
    if how == 'one':
        assert len(np.unique(cand[1024:2048, q0])) == 1


@pytest.mark.parametrize('name', sorted(EDGE_CASES))
def test_edge_cases_against_the_float64_model(engine, name):
    check_edge_case_shape(name)
    case = edge_case(name)
    cand, l_ref, g_ref = case[8:]
    if name == 'four_large_distinct':
        from hyperopt_amd import _native as N
        nb = ctypes.c_uint64(0)
        assert N.load().tpe_joint_quant_large_lds_bytes((ctypes.c_int32 * 4)(65536, 3000, 1500, 1100), 4,
                                                        ctypes.byref(nb)) == 0
        assert nb.value == 4097 * 32 + 8208 == 139312
    rec, l, g = engine.run_joint_quant_large(*_args(case), [7], C3, seed=3, inject=cand, want_lg=True)
    assert l.shape == g.shape == (1, C3)
    R.check_lpdf(l[0], l_ref, 'l ' + name)
    R.check_lpdf(g[0], g_ref, 'g ' + name)
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_quant_winner(rec[0], cand, l_ref, g_ref, cand.shape[1], name)


# ------------------------------------------------------- candidate-count edges
@functools.lru_cache(maxsize=None)
def count_case():
    case = Q.seeded_quant_case(1, [], [3000], 60)[:8]
    cand = quant_candidates(case[0], case[2], case[3], case[4], case[7], 1025, 7)
    refs = _refs(case, cand, 'counts')
    for C in (1, 1024):                                  # every prefix a run takes holds the conditions too
        _refs(case, cand[:C], 'counts C=%d' % C)
    return case + (cand,) + refs


def test_candidate_count_edges(engine):
    """C = 1: every sort key but one is ~0, one mini-table row, the record's
    index is 0.  C = 1024: one full chunk, no ragged one.  C = 1025: the second
    chunk holds one candidate, n_total = Dq = 1 and the longest tile.  The
    first min(C, 1024) rows are the same bytes in all three runs."""
    case = count_case()
    cand, l_ref, g_ref = case[8:]
    runs = {}
    for C in (1, 1024, 1025):
        rec, back, l, g = engine.run_joint_quant_large(*_args(case), [7], C, seed=3, inject=cand[:C], return_cand=True,
                                                       want_lg=True)
        assert back.shape == (1, C, 2) and l.shape == g.shape == (1, C)
        assert back[0].tobytes() == cand[:C].tobytes()
        R.check_lpdf(l[0], l_ref[:C], 'l C=%d' % C)
        R.check_lpdf(g[0], g_ref[:C], 'g C=%d' % C)
        i = int(rec['global_idx'][0])
        assert i == int(np.argmax(l[0] - g[0])), C       # the device's own scores, compared exactly
        assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
        np.testing.assert_array_equal(rec['z'][0, :2], cand[i].astype(np.float64))
        runs[C] = (rec, back, l, g)
    assert int(runs[1][0]['global_idx'][0]) == 0
    for C in (1, 1024):
        for k in (1, 2, 3):
            assert runs[C][k][0][:C].tobytes() == runs[1025][k][0][:C].tobytes(), (C, k)


# ------------------------------------------------------------------ exact ties
TIE_AT = (1024 + 700, 1024 + 5, 1024 + 300, 2048 + 1, 1024 + 64)


@functools.lru_cache(maxsize=None)
def tie_case(V):
    """(case, four [3072, 3] candidate arrays, the indices that must win): a
    pool of distinct poor rows and one best row b whose float64 score exceeds
    every other's by more than tie_set's window, written at TIE_AT; then also
    twice more in the lowest copy's lane; then also at index 3; then everywhere."""
    case = Q.seeded_quant_case(1, [3], [V], 60)[:8]
    pool = quant_candidates(case[0], case[2], case[3], case[4], case[7], 4096, 7)
    # (candidates clipped to a bound may repeat: the first of each vector, in the order drawn)
    pool = pool[np.sort(np.unique(pool, axis=0, return_index=True)[1])]
    l_ref, g_ref = _refs(case, pool, 'tie pool V=%d' % V)
    ties, score = R.tie_set(l_ref, g_ref)
    ib = int(np.argmax(score))
    keep = np.ones(len(pool), dtype=bool)                # the poor rows: outside the window of the best one
    keep[ties] = False
    sel = np.r_[ib, np.flatnonzero(keep)[:3 * 1024]]
    b, poor = pool[ib], pool[sel[1:]]
    ties, _ = R.tie_set(l_ref[sel], g_ref[sel])
    assert list(ties) == [0]                             # b beats every poor row by more than the window
    assert len(np.unique(pool[sel], axis=0)) == len(sel) == 3 * 1024 + 1 and min(TIE_AT) == 1029
    one = poor.copy()
    one[list(TIE_AT)] = b
    lane = one.copy()                                    # lane 5 of the second chunk holds b in three r slots
    lane[[1029 + 256, 1029 + 512]] = b
    two = one.copy()
    two[3] = b
    every = np.tile(b, (len(poor), 1))
    return case, (one, lane, two, every), (1029, 1029, 3, 0)


@pytest.mark.parametrize('stage,V', [('large', 3000), ('table', 200)])
def test_an_exact_tie_goes_to_the_lowest_index(engine, stage, V):
    """Duplicate rows score the same bytes, so the rule needs no tolerance.  The
    copies of the best row sit in two chunks (k_joint_merge); within the second
    chunk in r slots 0, 1 and 2, in two lanes of wave 0 (wave_best) and in waves
    1 and 2 (the four-slot reduce).  Then three copies in one lane (the lane's
    key > best.key), then a copy in the first chunk, then every row: index 0.
    'table': the same construction through run_joint_quant, which shares
    quant_chunk_body."""
    case, arrays, wins = tie_case(V)
    run = engine.run_joint_quant_large if stage == 'large' else engine.run_joint_quant
    for cand, win in zip(arrays, wins):
        rec, l, g = run(*_args(case), [7], len(cand), seed=3, inject=cand, want_lg=True)
        d = l[0] - g[0]
        assert len(set(d[i].tobytes() for i in TIE_AT)) == 1         # the precondition: equal bytes
        assert d[TIE_AT[0]] == d.max()
        assert int(rec['global_idx'][0]) == win, (stage, win)
        assert rec['l'][0] == l[0][win] and rec['g'][0] == g[0][win]
        np.testing.assert_array_equal(rec['z'][0, :3], cand[win].astype(np.float64))


# ------------------------------------------------- the sampler above 256 values
def _sampler_case(Dc, Vs, qlog):
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, [], list(Vs), 60)
    if qlog:                                             # the non-uniform lattice, as test_gpu_joint_quant_large's 'qlog'
        m_lo, V, e = Q.ref_lattice(*QLOG)
        assert (m_lo, V) == (8, Vs[0])
        edges[0] = e
        below = _qlog_side(below, 0, len(below[0]) - 1, 1)
        above = _qlog_side(above, 0, len(above[0]) - 1, 2)
    return below, above, low, high, ps, sb, sa, edges


@pytest.mark.parametrize('Dc,Vs,qlog', [(2, (1000,), False), (5, (65536, 300), False), (0, (4089,), True)])
def test_large_indices_are_the_binned_continuous_draws(engine, Dc, Vs, qlog):
    """test_quantised_indices_are_the_binned_continuous_draws above 256 values:
    the interior-edge binary search over V - 1 edges.  (5, [65536, 300]): words
    6 and 7, the second Philox block, and indices above 32,767.  (0, [4089]):
    qloguniform edges, wide bins at the low end and narrow ones at the high end."""
    C = 4096
    case = _sampler_case(Dc, Vs, qlog)
    below, above, low, high, ps, sb, sa, edges = case
    rec, cand, l, g = engine.run_joint_quant_large(*_args(case), [11], C, seed=42, return_cand=True, want_lg=True)
    assert cand.shape == (1, C, Dc + len(Vs))
    wide = [(s[0], np.hstack([s[1], s[4]]), np.hstack([s[2], s[5]])) for s in (below, above)]
    lo = np.concatenate([low, [e[0] for e in edges]])
    hi = np.concatenate([high, [e[-1] for e in edges]])
    _, full = engine.run_joint(wide[0], wide[1], lo, hi, [11], C, seed=42, return_cand=True)
    if Dc:
        _, cont = engine.run_joint(below[:3], above[:3], low, high, [11], C, seed=42, return_cand=True)
        assert np.ascontiguousarray(cand[0][:, :Dc]).tobytes() == cont[0].tobytes()
        assert np.ascontiguousarray(full[0][:, :Dc]).tobytes() == cont[0].tobytes()
    for d, e in enumerate(edges):
        zq = full[0][:, Dc + d].astype(np.float64)
        assert zq.min() >= e[0] and zq.max() < e[-1]
        want = np.searchsorted(e[1:-1], zq, 'right')
        np.testing.assert_array_equal(cand[0][:, Dc + d], want.astype(np.float32))
        if d == 0:
            assert want.max() > 255                          # draws beyond the table stage's lattices
    if Vs[0] == 65536:
        assert (cand[0][:, Dc] > 32767).sum() > 0
    qi = cand[0][:, Dc:].astype(np.int64)
    z64 = cand[0][:, :Dc].astype(np.float64)
    none = np.zeros((C, 0), dtype=np.int64)
    R.check_lpdf(l[0], Q.ref_quant_lpdf(z64, none, qi, below, low, high, [], sb, edges), 'l Dc=%d' % Dc)
    R.check_lpdf(g[0], Q.ref_quant_lpdf(z64, none, qi, above, low, high, [], sa, edges), 'g Dc=%d' % Dc)
    i = int(rec['global_idx'][0])
    assert i == int(np.argmax(l[0] - g[0]))
    np.testing.assert_array_equal(rec['z'][0, :Dc + len(Vs)], cand[0][i].astype(np.float64))


def test_large_determinism_and_batching(engine):
    """test_quant_determinism_and_batching with a 700-value label: the same
    call twice gives the same bytes; ids [5, 9, 12] in one call are three
    single calls; 1025 candidates leave a chunk of one."""
    C = 1025
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(3, [4], [700, 12], 90, seed=21)
    args = _args((below, above, low, high, ps, sb, sa, edges))
    ids = [5, 9, 12]

    def run(ids, seed=17):
        return engine.run_joint_quant_large(*args, ids, C, seed=seed, return_cand=True, want_lg=True)
    a, b = run(ids), run(ids)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, 6) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    assert a[1][:, :, 4].max() > 256
    for j, new_id in enumerate(ids):
        s = run([new_id])
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    assert run(ids, seed=18)[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------ the public path
def _trials(space, loss):
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(0)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, rs.randint(2 ** 31 - 1))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if x}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss(v)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def test_a_group_without_a_large_label_returns_the_table_stage_s_bytes():
    """joint_quantized='large' on a group whose quantised label has 11 values:
    the documents of joint_quantized=True (the routing, on device bytes)."""
    from hyperopt_amd import hp, tpe
    space = {'lr': hp.loguniform('lr', -7, 0), 'q': hp.quniform('q', 0, 10, 1), 'k': hp.choice('k', [0, 1])}
    domain, trials = _trials(space, lambda v: (math.log(v['lr']) + 3) ** 2 + abs(v['q'] - 4) + v['k'])
    kw = dict(n_startup_jobs=5, n_EI_candidates=1024 + 37, joint=['lr', 'q'])
    ids = [40, 41, 42]
    large = [d['misc']['vals'] for d in tpe.suggest(ids, domain, trials, 9, joint_quantized='large', **kw)]
    table = [d['misc']['vals'] for d in tpe.suggest(ids, domain, trials, 9, joint_quantized=True, **kw)]
    assert large == table
    for a, b in zip(large, table):
        assert set(a) == set(b) == {'lr', 'q', 'k'}
        for k in a:
            assert type(a[k][0]) is type(b[k][0])
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert type(a['q'][0]) is np.float64 and a['q'][0] == np.rint(a['q'][0]) and 0 <= a['q'][0] <= 10


def test_suggest_joins_a_large_qloguniform_beside_a_choice(engine):
    """joint=['lr', 'hidden', 'k'] with joint_discrete=True: a 4,089-value
    qloguniform label (non-uniform edges) and a joined choice in one group."""
    from hyperopt_amd import history, hp, joint as J, tpe
    C = 1024 + 37
    space = {'lr': hp.loguniform('lr', -7, 0), 'hidden': hp.qloguniform('hidden', math.log(8), math.log(4096), 1),
             'k': hp.choice('k', [0, 1])}
    domain, trials = _trials(space, lambda v: (math.log(v['lr']) + 3) ** 2 + abs(math.log(v['hidden']) - 5) + v['k'])
    kw = dict(n_EI_candidates=C, joint=['lr', 'hidden', 'k'], joint_discrete=True, joint_quantized='large')
    ids = [40, 41, 42]
    vals = [d['misc']['vals'] for d in tpe.suggest(ids, domain, trials, 9, n_startup_jobs=5, **kw)]
    hist = history.extract(domain, trials)
    row = domain.table.by_label
    model = J.fit_quant_model([row['lr']], [row['k']], [row['hidden']], hist,
                              history.split_below(hist, tpe._default_gamma), 1.0, tpe.DEFAULT_LF)
    assert [la[1] for la in model.lattices] == [4089]
    rec = engine.run_joint_quant_large(model.below[:3], model.above[:3], model.low, model.high, model.cats(),
                                       model.quants(), ids, C, 9)
    want = model.values(rec['z'][:, :3])                     # kernel coordinate order: lr, k, hidden
    cc = tpe.suggest_choices(domain.table, hist, ids, 9, columns=True, **kw)
    for j, i in enumerate(ids):
        h = vals[j]['hidden'][0]
        assert type(h) is np.float64 and h == np.rint(h) and 8 <= h <= 4096
        assert vals[j]['lr'][0] == want[j, 0] and vals[j]['k'][0] == want[j, 1] and h == want[j, 2]
        assert vals[j]['k'][0] in (0, 1)
        one = tpe.suggest([i], domain, trials, 9, n_startup_jobs=5, **kw)[0]
        assert one['misc']['vals'] == vals[j]                # batched ids equal the single-id calls
        for lab, val in vals[j].items():
            assert cc.values[j, cc.labels.index(lab)] == float(val[0]), (j, lab)
