"""Resident levels on the device (include/tpe_hip.h "Resident levels"): a
suggest against the same finished trials as the previous one keeps the fits,
the packed level and the score tables and only patches the seed and the new
ids into the device problem rows.  Every comparison is exact; the reference is
the same call with the feature off (tpe_level_resident(0))."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers import doc_values

from hyperopt_amd import _native as N

pytestmark = pytest.mark.gpu

CANDS = (4096, 1 << 20)       # lattice / per-candidate paths; the svm labels' cell tables


@pytest.fixture(scope='module')
def hists():
    import bench
    return {('svm', 600): bench.make_history(600, 0), ('svm', 2000): bench.make_history(2000, 0),
            ('rf', 2000): bench.make_history(2000, 0, loss=bench.rf_loss)}


@pytest.fixture(autouse=True)
def _resident_on():
    if not N.level_resident(1)[0]:
        pytest.skip('TPE_RESIDENT_LEVEL=0')
    yield
    N.level_resident(1)


def _stats():
    return N.level_resident(-1)[1]


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _off(fn):
    N.level_resident(0)
    try:
        return fn()
    finally:
        N.level_resident(1)


def _suggest(domain, trials, ids, seed, C, **kw):
    from hyperopt_amd import tpe
    return [doc_values([d]) for d in tpe.suggest(list(ids), domain, trials, seed, n_EI_candidates=C, **kw)]


@pytest.mark.parametrize('which', [('svm', 600), ('svm', 2000), ('rf', 2000)])
@pytest.mark.parametrize('C', CANDS)
def test_seeds_and_ids_hit_and_equal_off(hists, which, C):
    domain, trials = hists[which]
    n = which[1]
    seeds = (3, 4, 5, 6, 7)
    batches = ([n], [n, n + 1, n + 2], [n + 7, n + 8, n + 9])
    ref = _off(lambda: [[_suggest(domain, trials, ids, s, C) for s in seeds] for ids in batches])
    s0 = _stats()
    got = [_suggest(domain, trials, batches[0], s, C) for s in seeds]
    d = _delta(s0, _stats())
    assert got == ref[0]
    assert d['hits'] >= 4 and d['misses'] == 1, d
    # three ids: another level (a miss), then other ids on it (hits, another ctr3)
    s1 = _stats()
    got = [_suggest(domain, trials, batches[1], s, C) for s in seeds]
    d1 = _delta(s1, _stats())
    got2 = [_suggest(domain, trials, batches[2], s, C) for s in seeds]
    d2 = _delta(s1, _stats())
    assert got == ref[1] and got2 == ref[2]
    assert d1['misses'] == 1 and d1['hits'] >= 4, d1
    assert d2['misses'] == 1 and d2['hits'] >= 9, d2


def _flat_case():
    from hyperopt_amd import base, hp, rand
    domain = base.Domain(lambda d: 0.0, {'a': hp.uniform('a', -1, 1), 'b': hp.uniform('b', 0, 3),
                                         'c': hp.normal('c', 0, 1)})
    trials = base.Trials()
    rs = np.random.RandomState(0)
    for tid in range(60):
        d = rand.suggest([tid], domain, trials, rs.randint(2 ** 31 - 1))[0]
        d['state'] = base.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs([d])
    trials.refresh()
    return domain, trials


@pytest.mark.parametrize('C', CANDS)
def test_other_work_on_the_engine_invalidates(hists, C):
    from hyperopt_amd import tpe
    domain, trials = hists[('svm', 2000)]
    other = hists[('svm', 600)]
    flat = _flat_case()
    n = 2000

    def general():
        tpe.NATIVE_TREE = False
        try:
            _suggest(domain, trials, [n], 40, C)
        finally:
            tpe.NATIVE_TREE = True
    between = [
        ('another history', lambda: _suggest(other[0], other[1], [600], 41, C)),
        ('candidate_report', lambda: tpe.candidate_report(n, domain, trials, 42, k=4, n_EI_candidates=4096)),
        ('joint suggest', lambda: _suggest(flat[0], flat[1], [60], 43, 4096, joint=True)),
        ('another n_EI_candidates', lambda: _suggest(domain, trials, [n], 44, 2 * C if C < 1 << 20 else C // 2)),
        ('general path', general),
    ]
    seeds = [100 + i for i in range(3 * len(between))]
    ref = _off(lambda: [_suggest(domain, trials, [n], s, C) for s in seeds])
    for fn in (f for _, f in between):        # (every pool at its final size before the counts)
        fn()
    for k, (name, fn) in enumerate(between):
        a, b, c = seeds[3 * k:3 * k + 3]
        r_a = _suggest(domain, trials, [n], a, C)
        s0 = _stats()
        r_b = _suggest(domain, trials, [n], b, C)
        d = _delta(s0, _stats())
        assert d['hits'] == 1 and d['misses'] == 0, (name, d)
        fn()
        s1 = _stats()
        r_c = _suggest(domain, trials, [n], c, C)
        d = _delta(s1, _stats())
        assert d['hits'] == 0 and d['misses'] >= 1, (name, d)
        assert [r_a, r_b, r_c] == ref[3 * k:3 * k + 3], name


def _own_records(table, hist, eng):
    """The tree's label records with private copies of every tids / values
    array (so that a test may overwrite them in place), the arrays by label."""
    from hyperopt_amd import tpe
    arr = tpe._tree_labels(table, hist, eng)[0].copy()
    cols = {}
    for r in table.rows:
        i = r.index
        nobs = int(arr[i]['n_obs'])
        if nobs <= 0 or not arr[i]['tids'] or not arr[i]['values']:
            continue
        t = np.ctypeslib.as_array(ctypes.cast(int(arr[i]['tids']), ctypes.POINTER(ctypes.c_int64)), (nobs,)).copy()
        v = np.ctypeslib.as_array(ctypes.cast(int(arr[i]['values']), ctypes.POINTER(ctypes.c_int64)), (nobs,)).copy()
        arr[i]['tids'], arr[i]['values'] = t.ctypes.data, v.ctypes.data
        cols[r.label] = (t, v)
    return arr, cols


def _tree(eng, arr, below, ids, C, seed, prior_weight=1.0, lf=25):
    values, active = eng.suggest_tree(arr, below, prior_weight, lf, np.asarray(ids, dtype=np.int64), C, seed, 64.0)
    assert values is not None
    return values.copy(), active.copy()


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('C', CANDS)
def test_same_addresses_other_content(hists, C):
    """Engine.suggest_tree on hand-held records: content overwritten in place,
    at unchanged addresses, is never taken for the resident level's."""
    from hyperopt_amd import history as H
    from hyperopt_amd.engine import Engine
    domain, trials = hists[('svm', 2000)]
    hist = H.extract(domain, trials)
    table = domain.table
    eng, fresh = Engine(), Engine()
    arr, cols = _own_records(table, hist, eng)
    below = np.sort(H.split_below(hist, 0.25)).astype(np.int64)
    bset = set(below.tolist())
    st = dict(C=C, pw=1.0, lf=25, seed=500)

    def run(e):
        st['seed'] += 1
        return _tree(e, arr, below, [2000], st['C'], st['seed'], st['pw'], st['lf'])

    def ref():
        return _off(lambda: _tree(fresh, arr, below, [2000], st['C'], st['seed'], st['pw'], st['lf']))
    mt, mv = cols['model']                    # the root gate: every trial, categories 0..2
    ct, cv = cols['svm_C']                    # a continuous label of the svm branch (tids with gaps)

    def bump_cat(i):
        mv[i] = (mv[i] + 1) % 3

    def tids_pair():
        # an observation of the below set moved to the free tid after it (now above),
        # and its neighbour too where that tid is free
        for i in range(len(ct) - 2):
            if int(ct[i]) in bset and ct[i] + 1 < ct[i + 1] and int(ct[i]) + 1 not in bset:
                ct[i] += 1
                if ct[i + 1] + 1 < ct[i + 2]:
                    ct[i + 1] += 1
                return
        raise AssertionError('no below observation of svm_C with a free tid after it')

    def below_tid():
        free = [t for t in range(2000) if t not in bset]
        below[len(below) // 2] = free[len(free) // 2]
        below.sort()
    changes = [
        ('values[0]', lambda: bump_cat(0)), ('values[mid]', lambda: bump_cat(len(mv) // 2)),
        ('values[-1]', lambda: bump_cat(len(mv) - 1)), ('tids pair', tids_pair), ('below tid', below_tid),
        ('prior_weight', lambda: st.update(pw=0.5)), ('lf', lambda: st.update(lf=40)),
        ('n_cand', lambda: st.update(C=C // 2)),
    ]
    run(eng)
    for name, change in changes:
        run(eng)
        s0 = _stats()
        run(eng)
        d = _delta(s0, _stats())
        assert d['hits'] == 1 and d['misses'] == 0, (name, d)
        change()
        s1 = _stats()
        got = run(eng)
        d = _delta(s1, _stats())
        assert d['hits'] == 0 and d['misses'] >= 1, (name, d)
        assert _same(got, ref()), name


def _appended_flow(C, steer):
    """20 steps of insert - evaluate - refresh - suggest (bench.py's appending
    loop) with the feature off and on: (off results, on results, stats delta)."""
    import bench
    from hyperopt_amd import tpe

    def flow():
        domain, trials = bench.make_history(600, 3, loss=bench.rf_loss if steer == 'rf' else None)
        out, tid = [], 600
        for i in range(20):
            docs = tpe.suggest([tid], domain, trials, 900 + i, n_EI_candidates=C)
            out.append(doc_values(docs))
            trials.insert_trial_docs(docs)
            trials.refresh()
            bench.evaluate(domain, trials, trials.trials[-1])
            tid += 1
        return out
    ref = _off(flow)
    s0 = _stats()
    got = flow()
    d = _delta(s0, _stats())
    print('appended flow', steer, C, d)
    return ref, got, d


@pytest.mark.parametrize('C', CANDS)
def test_appended_flow_equals_off(C):
    """A sequential fmin on the rf-steered tree: every call misses, the results
    are the same, and fits are reused.  This tree's quantized labels are fitted
    through the hand-back to the caller (a refused native call, then one with
    the caller's sorts), whose second call finds the first call's fits under
    unchanged keys; and its nested rf_depth gate leaves rf_depth_n without a
    new observation whenever the finished trial took the shallow option.
    Measured on MI355X, both candidate counts: 20 misses, 0 hits, fit_reuses > 0."""
    ref, got, d = _appended_flow(C, 'rf')
    assert got == ref
    assert d['fit_reuses'] > 0 and d['misses'] >= 19, d


@pytest.mark.parametrize('C', CANDS)
def test_appended_flow_on_the_predicted_branch(C):
    """The same flow on the svm-steered tree.  Every suggestion lies on the
    branch the gates predicted, so the finished trial adds an observation to
    every label the next suggest fits: no key can match (measured: 20 misses,
    0 hits, 0 fit reuses, both candidate counts).  The results are the same."""
    ref, got, d = _appended_flow(C, 'svm')
    assert got == ref
    assert d['hits'] == 0 and d['misses'] >= 19, d


def test_pool_growth_is_a_miss(hists):
    from hyperopt_amd import history as H
    from hyperopt_amd.engine import Engine
    domain, trials = hists[('svm', 2000)]
    hist = H.extract(domain, trials)
    eng, fresh = Engine(), Engine()
    arr, cols = _own_records(domain.table, hist, eng)
    below = np.sort(H.split_below(hist, 0.25)).astype(np.int64)
    _tree(eng, arr, below, [2000], 4096, 1)
    s0 = _stats()
    _tree(eng, arr, below, [2000], 4096, 2)
    assert _delta(s0, _stats())['hits'] == 1
    blob0 = eng._bufs['blob'].data_ptr(), eng._bufs['tab'].numel()
    _tree(eng, arr, below, [2000], 1 << 20, 3)                 # (returns through _grow)
    assert (eng._bufs['blob'].data_ptr(), eng._bufs['tab'].numel()) != blob0
    s1 = _stats()
    got = _tree(eng, arr, below, [2000], 4096, 4)
    d = _delta(s1, _stats())
    assert d['hits'] == 0 and d['misses'] >= 1, d
    assert _same(got, _off(lambda: _tree(fresh, arr, below, [2000], 4096, 4)))


@pytest.mark.parametrize('C', CANDS)
def test_level_by_level_equals_off(hists, C):
    from hyperopt_amd import tpe
    domain, trials = hists[('svm', 600)]
    tpe.SPECULATE = False
    try:
        ref = _off(lambda: [_suggest(domain, trials, [600], s, C) for s in (70, 71, 72)])
        got = [_suggest(domain, trials, [600], s, C) for s in (70, 71, 72)]
    finally:
        tpe.SPECULATE = True
    assert got == ref


def _exchange_worker(port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        import bench
        from hyperopt_amd import dist as D, tpe
        from hyperopt_amd.engine import get_engine
        domain, trials = bench.make_history(600, 0)

        def run(s, c, **kw):
            return {k: float(v) for k, v in
                    doc_values(tpe.suggest([600], domain, trials, s, n_EI_candidates=c, **kw)).items()}
        cases = [(s, c) for c in CANDS for s in (81, 82, 83)]
        N.level_resident(0)
        ref = [run(*a) for a in cases]
        N.level_resident(1)
        D.EXCHANGE_ALWAYS = True
        got = {}
        for force in ('0', '1'):
            os.environ['TPE_FORCE_COMBINE'] = force
            got[force] = [run(*a, shard=(0, 1)) for a in cases]
        os.environ['TPE_FORCE_COMBINE'] = '0'
        plain = [run(*a) for a in cases]             # (and unsharded again, after the exchanged levels)
        D.exchange_for(get_engine()).close()
        q.put((ref, got, plain, None))
    except Exception:
        import traceback
        q.put((None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_forced_one_rank_exchange_equals_off():
    """The exchange forced on one rank (and its N-rank combine,
    TPE_FORCE_COMBINE=1): exchanged levels stay on the miss path; their results,
    and the unsharded suggests after them, equal the feature-off ones."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_exchange_worker, args=(port, q))
    p.start()
    ref, got, plain, err = q.get(timeout=240)
    p.join(timeout=60)
    assert err is None, err
    assert got['0'] == ref and got['1'] == ref and plain == ref
