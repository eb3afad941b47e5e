"""Joint candidate report on the GPU (include/tpe_hip.h "Joint candidate
report"): the k best distinct candidate rows and the score statistics per
problem, against the numpy statement of the semantics (tests/joint_report_ref.py) —

  1. synthetic (rows, l, g) arrays straight through the C-ABI,
  2. through the five Engine.run_joint* methods on the arrays the same call returns,
  3. the public tpe.joint_candidate_report against tpe.suggest and the engine.

Ranking, rows, l, g, indices, n_top, counts, min and max are compared exactly.
mean: |gpu - numpy| <= 1e-10 mean|s|; m2: 1e-9 relative — the bounds of
tests/test_gpu_report.py, which hold for n <= 2^16 candidates (two float64
summations of that many terms differ by at most about 1.5e-11 mean|s|).
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as J
from tests import joint_report_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 4096


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


# ------------------------------------------------------- 1. through the ABI
DECIMALS = (0, 1, 2)           # rounding of the problems' l and g: heavy ties


def _synthetic(C, widths, seed=0):
    """Three problems of C candidates (tests/test_gpu_report.py's recipe for l
    and g: rounded, 2 % of each -inf, from C = 100 one position shared — a NaN
    score).  Rows: problem 0 draws from 5 rows (fewer than k = 8 distinct),
    problem 1 from one base row changed in exactly one coordinate — the first,
    the middle and the last in turn — to one of 50 values, problem 2 from a
    lattice that holds -0.0 and +0.0."""
    rs = np.random.RandomState(2000 + C + 7 * sum(widths) + seed)
    rows, l, g = [], np.zeros((3, C)), np.zeros((3, C))
    n_inf = int(round(0.02 * C))
    for p, W in enumerate(widths):
        if p == 0:
            pool = rs.normal(0.0, 2.0, (5, W)).astype(np.float32)
            x = pool[rs.randint(0, 5, C)]
        elif p == 1:
            x = np.repeat(rs.normal(0.0, 2.0, (1, W)).astype(np.float32), C, axis=0)
            pos = np.array([0, W // 2, W - 1])[np.arange(C) % 3]
            x[np.arange(C), pos] = (rs.randint(0, 50, C) * 0.25 - 3.0).astype(np.float32)
        else:
            x = (rs.randint(0, 4, (C, W)) * 0.5).astype(np.float32)
            x[(x == 0) & (rs.uniform(size=(C, W)) < 0.5)] = np.float32(-0.0)
        rows.append(np.ascontiguousarray(x))
        l[p] = np.round(rs.normal(-2.0, 3.0, C), DECIMALS[p])
        g[p] = np.round(rs.normal(-2.5, 3.0, C), DECIMALS[p])
        if n_inf:
            li, gi = rs.choice(C, n_inf, replace=False), rs.choice(C, n_inf, replace=False)
            if C >= 100:
                gi[0] = li[0]
            l[p, li] = -np.inf
            g[p, gi] = -np.inf
    return rows, l, g


def _run_abi(engine, rows, l, g, k, layout):
    """tpe_joint_report over three problems.  ``layout``: 'packed' (one width,
    cand_off NULL), 'offsets' (one width, the problems in reverse order with
    odd gaps: rows not 16-byte aligned) or 'widths' (per-problem widths and
    offsets).  Runs twice with the outputs overwritten between; returns (top
    [3, k], z [3, k, z_stride], n_top, stats)."""
    import torch
    from hyperopt_amd import _native as N
    lib, dev = engine.lib, engine.device
    C = l.shape[1]
    widths = np.array([r.shape[1] for r in rows], dtype=np.int32)
    zs = int(widths.max()) + (3 if layout != 'packed' else 0)
    a = N.JointReportArgs()
    a.n_probs, a.n_cand, a.width, a.z_stride = 3, C, int(widths[0]), zs
    if layout == 'packed':
        assert len(set(widths)) == 1
        flat = np.concatenate([r.reshape(-1) for r in rows])
    else:
        off, n = np.zeros(3, dtype=np.int64), 1
        for p in (2, 1, 0):
            off[p] = n
            n += rows[p].size + 3
        flat = np.full(n, 77.0, dtype=np.float32)
        for p in range(3):
            flat[off[p]:off[p] + rows[p].size] = rows[p].reshape(-1)
        d_off = torch.from_numpy(off).to(dev)
        a.cand_off = d_off.data_ptr()
        if layout == 'widths':
            d_w = torch.from_numpy(widths).to(dev)
            a.widths, a.host_widths, a.width = d_w.data_ptr(), widths.ctypes.data, 0
    d_cand = torch.from_numpy(flat).to(dev)
    d_l, d_g = (torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(dev) for x in (l, g))
    a.cand, a.l_out, a.g_out = d_cand.data_ptr(), d_l.data_ptr(), d_g.data_ptr()
    nb = ctypes.c_uint64(0)
    N.check(lib.tpe_joint_report_scratch_bytes(3, C, k, ctypes.byref(nb)), lib, 'scratch_bytes')
    d_scr = torch.zeros(nb.value // 8 + 1, dtype=torch.float64, device=dev)
    d_top = torch.zeros(3 * k * 4, dtype=torch.float64, device=dev)
    d_z = torch.zeros(3 * k * zs, dtype=torch.float32, device=dev)
    d_ntop = torch.zeros(3, dtype=torch.int32, device=dev)
    d_stats = torch.zeros(3 * 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = []
    for _ in range(2):
        N.check(lib.tpe_joint_report(ctypes.byref(a), k, d_top.data_ptr(), d_z.data_ptr(), d_ntop.data_ptr(),
                                     d_stats.data_ptr(), d_scr.data_ptr(), nb.value, ctypes.c_void_p(stream)), lib,
                'tpe_joint_report')
        outs.append(tuple(t.cpu().numpy().tobytes() for t in (d_top, d_z, d_ntop, d_stats)))
        d_top.fill_(7.0)            # the second call must write everything again
        d_z.fill_(7.0)
        d_ntop.fill_(7)
        d_stats.fill_(7.0)
    assert outs[0] == outs[1], 'a second call gives different bytes'
    top = np.frombuffer(outs[0][0], dtype=N.JOINT_TOP_ENTRY_DTYPE).reshape(3, k)
    z = np.frombuffer(outs[0][1], dtype=np.float32).reshape(3, k, zs)
    return top, z, np.frombuffer(outs[0][2], dtype=np.int32), np.frombuffer(outs[0][3], dtype=N.SCORE_STATS_DTYPE)


# every C and every W of the issue, each k at several of them; 'offsets' rows
# are not 16-byte aligned, so W = 16 and 64 take both load paths
ABI_CASES = [(1, 1, 1, 'packed'), (1, 64, 8, 'packed'), (63, 2, 8, 'packed'), (63, 17, 64, 'offsets'),
             (65, 3, 1, 'offsets'), (65, 5, 64, 'packed'), (CHUNK - 1, 16, 8, 'packed'), (CHUNK, 17, 8, 'packed'),
             (CHUNK, 64, 1, 'offsets'), (CHUNK + 1, 64, 8, 'packed'), (CHUNK + 1, 1, 64, 'packed'),
             (3 * CHUNK + 17, 2, 1, 'packed'), (3 * CHUNK + 17, 3, 8, 'packed'), (3 * CHUNK + 17, 5, 8, 'offsets'),
             (3 * CHUNK + 17, 16, 64, 'offsets'), (3 * CHUNK + 17, 16, 8, 'packed'), (3 * CHUNK + 17, 64, 64, 'packed'),
             (3 * CHUNK + 17, 1, 8, 'packed')]


@pytest.mark.parametrize('C,W,k,layout', ABI_CASES)
def test_report_of_synthetic_rows(engine, C, W, k, layout):
    rows, l, g = _synthetic(C, (W, W, W))
    top, z, n_top, stats = _run_abi(engine, rows, l, g, k, layout)
    for p in range(3):
        R.check_report(rows[p], l[p], g[p], k, top[p], z[p], n_top[p], stats[p], (C, W, k, layout, p))
        if C >= CHUNK - 1:      # the case keeps its point: NaN, +inf and -inf scores are all there
            assert stats[p]['n_nan'] > 0 and stats[p]['n_posinf'] > 0 and stats[p]['n_neginf'] > 0, (C, p)
    if C >= 63:
        assert n_top[0] == min(k, 5)                     # fewer distinct rows than k = 8 or 64
        if W >= 3 and k > 1:                             # rows that differ in one coordinate are distinct
            assert n_top[1] == min(k, R.n_distinct_rows(rows[1])) > 1
    if C >= CHUNK and W >= 2:
        assert (rows[2] == 0).any() and np.signbit(rows[2][rows[2] == 0]).any()


def test_report_of_rows_of_several_widths(engine):
    C, k = CHUNK + 1, 8
    rows, l, g = _synthetic(C, (2, 5, 16))
    top, z, n_top, stats = _run_abi(engine, rows, l, g, k, 'widths')
    assert z.shape == (3, k, 19)
    for p in range(3):
        R.check_report(rows[p], l[p], g[p], k, top[p], z[p], n_top[p], stats[p], ('widths', p))


def test_equal_rows_with_different_scores_and_nan_rows(engine):
    """The stage takes arbitrary l and g: of two equal rows the better-scored
    one is the entry, wherever the other lies; a row with a NaN coordinate
    equals nothing, not even its copy."""
    C, W, k = 2 * CHUNK + 5, 3, 8
    rs = np.random.RandomState(5)
    x = rs.normal(size=(C, W)).astype(np.float32)
    x[CHUNK + 9] = x[3]                     # copies across chunks
    x[2 * CHUNK + 1] = x[3]
    x[100] = x[200] = (np.nan, 1.0, 2.0)
    l, g = rs.normal(size=C), np.zeros(C)
    l[[3, CHUNK + 9, 2 * CHUNK + 1]] = 50.0, 60.0, 55.0
    l[[100, 200]] = 58.0, 57.0
    rows = [x, x[::-1].copy(), x]
    ll = np.stack([l, l[::-1], l])
    top, z, n_top, stats = _run_abi(engine, rows, ll, np.stack([g, g, g]), k, 'packed')
    for p in range(3):
        R.check_report(rows[p], ll[p], g, k, top[p], z[p], n_top[p], stats[p], ('copies', p))
    assert top[0]['idx'][:3].tolist() == [CHUNK + 9, 100, 200] and 3 not in top[0]['idx']


# ------------------------------------------------------ 2. through the engine
C_ENGINE = 2 * CHUNK + 5
K_ENGINE = 8


def _check_engine(out, P, widths, what, n_head=1):
    """(rec, cand, l, g, top, top_z, n_top, stats) of one engine call: the
    report equals the reference applied to the arrays the call returned, entry 0
    is the stage's own winner record."""
    rec, cand, l, g, top, z, n_top, stats = out
    assert len(rec) == P and top.shape == (P, K_ENGINE) and len(z) == P and n_top.shape == (P,) and stats.shape == (P,)
    for p in range(P):
        W = widths[p]
        assert cand[p].shape == (C_ENGINE, W) and z[p].shape == (K_ENGINE, W) and z[p].dtype == np.float32
        R.check_report(cand[p], l[p], g[p], K_ENGINE, top[p], z[p], n_top[p], stats[p], (what, p))
        assert rec['global_idx'][p] == top['idx'][p, 0], (what, p)
        assert rec['l'][p] == top['l'][p, 0] and rec['g'][p] == top['g'][p, 0], (what, p)
        assert rec['z'][p, :W].tobytes() == z[p][0].astype(np.float64).tobytes(), (what, p)
    return n_top


def test_engine_run_joint(engine):
    below, above, low, high = J.seeded_case(3, 60, 203)[:4]
    out = engine.run_joint(below, above, low, high, [7, 11], C_ENGINE, 17, return_cand=True, want_lg=True,
                           report_k=K_ENGINE)
    n_top = _check_engine(out, 2, [3, 3], 'run_joint')
    assert (n_top == K_ENGINE).all()
    # without the per-candidate arrays: the same report; without report_k: what the call returned before
    only = engine.run_joint(below, above, low, high, [7, 11], C_ENGINE, 17, report_k=K_ENGINE)
    assert len(only) == 5
    for x, y in zip(only, (out[0],) + out[4:]):
        assert x.tobytes() == y.tobytes()
    plain = engine.run_joint(below, above, low, high, [7, 11], C_ENGINE, 17)
    assert isinstance(plain, np.ndarray) and plain.tobytes() == out[0].tobytes()
    lg = engine.run_joint(below, above, low, high, [7, 11], C_ENGINE, 17, want_lg=True, report_k=1)
    assert len(lg) == 7 and lg[1].tobytes() == out[2].tobytes() and lg[3].shape == (2, 1)
    assert lg[3].tobytes() == out[4][:, :1].tobytes()
    with pytest.raises(ValueError, match='report_k'):
        engine.run_joint(below, above, low, high, [7], C_ENGINE, 17, report_k=65)


def test_engine_run_joint_injected_duplicates(engine):
    below, above, low, high = J.seeded_case(3, 60, 203)[:4]
    rs = np.random.RandomState(9)
    pool = rs.uniform(-9, 9, (100, 3)).astype(np.float32)
    pool[:5] = pool[0]                                   # 96 distinct rows
    inj = pool[rs.randint(0, 100, C_ENGINE)]
    out = engine.run_joint(below, above, low, high, [7], C_ENGINE, 17, inject=inj, return_cand=True, want_lg=True,
                           report_k=K_ENGINE)
    assert out[1][0].tobytes() == inj.tobytes()
    _check_engine(out, 1, [3], 'inject')
    few = engine.run_joint(below, above, low, high, [7], C_ENGINE, 17, inject=pool[rs.randint(0, 5, C_ENGINE)],
                           report_k=K_ENGINE)                # one distinct row
    assert few[3].tolist() == [1] and (few[1]['idx'][0, 1:] == -1).all() and not few[2][0, 1:].any()


def test_engine_run_joint_mixed(engine):
    below, above, low, high, pmu, psig, ps, sb, sa, rs = M.seeded_mixed_case(2, [3, 4], 60)
    out = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [7, 11],
                                 C_ENGINE, 17, return_cand=True, want_lg=True, report_k=K_ENGINE)
    _check_engine(out, 2, [4, 4], 'run_joint_mixed')
    only = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [7, 11],
                                  C_ENGINE, 17, report_k=K_ENGINE)
    assert len(only) == 5 and only[1].tobytes() == out[4].tobytes() and only[2].tobytes() == out[5].tobytes()
    # discrete labels alone: 6 distinct rows among all the candidates
    below, above, low, high, pmu, psig, ps, sb, sa, rs = M.seeded_mixed_case(0, [2, 3], 60)
    out = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [7, 11],
                                 C_ENGINE, 17, return_cand=True, want_lg=True, report_k=K_ENGINE)
    assert _check_engine(out, 2, [2, 2], 'run_joint_mixed, discrete only').tolist() == [6, 6]


def test_engine_run_joint_quant(engine):
    below, above, low, high, ps, sb, sa, edges, rs = Q.seeded_quant_case(1, [3], [5], 60)
    out = engine.run_joint_quant(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                 Q.quants_of(below, above, edges), [7, 11], C_ENGINE, 17, return_cand=True,
                                 want_lg=True, report_k=K_ENGINE)
    _check_engine(out, 2, [3, 3], 'run_joint_quant')


def test_engine_run_joint_wide(engine):
    below, above, low, high = J.seeded_case(20, 60, 220)[:4]
    out = engine.run_joint_wide(below, above, low, high, [7, 11], C_ENGINE, 17, return_cand=True, want_lg=True,
                                report_k=K_ENGINE)
    _check_engine(out, 2, [20, 20], 'run_joint_wide')


def test_engine_run_joint_segments(engine):
    models = [J.seeded_case(2, 40, 202)[:4], J.seeded_case(3, 60, 203)[:4]]
    words = [0xFFFFFFFE, 0xFFFFFFFE - 3]
    segs, ids = [1, 0, 1], [9, 5, 12]
    out = engine.run_joint_segments(models, words, segs, ids, C_ENGINE, 17, return_cand=True, want_lg=True,
                                    report_k=K_ENGINE)
    _check_engine(out, 3, [3, 2, 3], 'run_joint_segments')
    plain = engine.run_joint_segments(models, words, segs, ids, C_ENGINE, 17, return_cand=True, want_lg=True)
    assert len(plain) == 4 and plain[0].tobytes() == out[0].tobytes()
    for x, y in zip(plain[1], out[1]):
        assert x.tobytes() == y.tobytes()
    assert plain[2].tobytes() == out[2].tobytes() and plain[3].tobytes() == out[3].tobytes()
    for kw in (dict(), dict(return_cand=True), dict(want_lg=True)):
        part = engine.run_joint_segments(models, words, segs, ids, C_ENGINE, 17, report_k=K_ENGINE, **kw)
        assert len(part) == 5 + (1 if 'return_cand' in kw else 0) + (2 if 'want_lg' in kw else 0)
        assert part[0].tobytes() == out[0].tobytes() and part[-4].tobytes() == out[4].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(part[-3], out[5]))
        assert part[-2].tobytes() == out[6].tobytes() and part[-1].tobytes() == out[7].tobytes()
        if 'return_cand' in kw:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(part[1], out[1]))
        if 'want_lg' in kw:
            assert part[1].tobytes() == out[2].tobytes() and part[2].tobytes() == out[3].tobytes()


# ------------------------------------------------------------ 3. the public path
C_PUBLIC = CHUNK + 5
SEED = 321


def _spaces():
    from hyperopt_amd import hp
    cont = {'x': hp.uniform('x', -5, 5), 'y': hp.lognormal('y', 0, 1), 'z': hp.normal('z', 0, 2)}
    disc = dict(cont, c=hp.choice('c', [0, 1, 2]), r=hp.randint('r', 4))
    quant = dict(disc, q=hp.quniform('q', 0, 10, 1), ql=hp.qloguniform('ql', 0, 3, 2))
    wide = dict(('u%02d' % i, hp.uniform('u%02d' % i, -1, 1)) for i in range(20))
    branch = {'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5), 'clf': hp.choice('clf', [
        {'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
        {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.uniform('rf_split', 0, 1), 'w': hp.normal('rf_w', 0, 1)}])}
    return dict(joint=(cont, dict(joint=True)), discrete=(disc, dict(joint=True, joint_discrete=True)),
                quantized=(quant, dict(joint=True, joint_discrete=True, joint_quantized=True)),
                wide=(wide, dict(joint=True, joint_wide=True)), branches=(branch, dict(joint=True, joint_branches=True)))


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


@functools.lru_cache(maxsize=None)
def _public_case(name):
    """The space of a README example with 40 random trials (computed once)."""
    from hyperopt_amd import base, rand
    space, kw = _spaces()[name]
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = np.array([float(x) for x in _vals(docs[0]).values()])
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(np.sum(np.sin(v)) + 0.01 * rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials, kw


def _check_group(gr, model, cand, l, g, top, what):
    """One group of the public report against the reference applied to the
    engine's arrays of the same pool."""
    from hyperopt_amd import tpe
    ref = R.top_distinct_rows(cand, l, g, K_ENGINE)
    assert gr.n_top == len(ref) == len(gr.top) == len(gr.vectors), what
    np.testing.assert_array_equal(gr.top['index'], ref, err_msg=str(what))
    assert gr.top['l'].tobytes() == l[ref].tobytes() and gr.top['g'].tobytes() == g[ref].tobytes(), what
    with np.errstate(invalid='ignore'):
        assert gr.top['score'].tobytes() == (l[ref] - g[ref]).tobytes(), what
    assert gr.vectors.tobytes() == model.values(cand[ref].astype(np.float64)).tobytes(), what
    assert gr.top.dtype == tpe.JOINT_REPORT_TOP_DTYPE
    want = R.score_stats(l, g)
    for f in ('n_finite', 'n_nan', 'n_posinf', 'n_neginf', 'min', 'max'):
        assert gr.stats[f] == want[f], (what, f)
    assert abs(gr.stats['mean'] - want['mean']) <= 1e-10 * want['mean_abs'], what
    assert abs(gr.stats['m2'] - want['m2']) <= 1e-9 * want['m2'], what


@pytest.mark.parametrize('name', ['joint', 'discrete', 'quantized', 'wide', 'branches'])
def test_public_joint_candidate_report(name):
    from hyperopt_amd import history, joint as JT, tpe
    from hyperopt_amd.engine import get_engine
    domain, trials, kw = _public_case(name)
    table, new_id = domain.table, 40
    rep = tpe.joint_candidate_report(new_id, domain, trials, SEED, k=K_ENGINE, n_EI_candidates=C_PUBLIC, **kw)
    got = _vals(tpe.suggest([new_id], domain, trials, SEED, n_EI_candidates=C_PUBLIC, **kw)[0])
    hist = history.extract(domain, trials)
    root, branch_groups = tpe._joint_plan(table, kw['joint'], 'philox', 'fp32', (None,) * 4,
                                          kw.get('joint_discrete', False), kw.get('joint_quantized', False),
                                          kw.get('joint_wide', False), kw.get('joint_branches', False))
    assert len(rep) == 1 + len(branch_groups) and rep[0].condition is None
    engine = get_engine()
    ids = np.array([new_id], dtype=np.int64)

    # the root group: entry 0 is what the suggest joins, byte for byte
    gr = rep[0]
    crows, drows, qrows = tpe._joint_kernel_order(root)
    assert gr.labels == [r.label for r in crows + drows + qrows] and len(gr.labels) == len(root)
    for d, lab in enumerate(gr.labels):
        assert np.float64(got[lab]).tobytes() == gr.vectors[0, d].tobytes(), (name, lab, got[lab], gr.vectors[0, d])
    group, model, (rec, cand, l, g) = tpe._run_root_group(engine, root, hist, ids, SEED, tpe._default_prior_weight,
                                                          C_PUBLIC, tpe._default_gamma, return_cand=True, want_lg=True)
    _check_group(gr, model, cand[0], l[0], g[0], gr.top, (name, 'root'))
    assert gr.top['index'][0] == rec['global_idx'][0]
    if name in ('discrete', 'quantized'):
        assert R.n_distinct_rows(cand[0]) <= C_PUBLIC
        for d, r in enumerate(group):
            if r.categorical or r.dist.startswith('q'):
                assert (gr.vectors[:, d] == np.rint(gr.vectors[:, d])).all(), (name, r.label)
    if name == 'wide':
        assert gr.vectors.shape == (K_ENGINE, 20)

    # the branch groups, as if active: the taken one equals the suggest, every
    # one equals the segmented stage called on its model, stream word and id
    below_tids = history.split_below(hist, tpe._default_gamma)
    taken = 0
    for gr, rows in zip(rep.groups[1:], branch_groups):
        assert gr.labels == [r.label for r in rows] and gr.condition == tpe._branch_key(rows[0])
        model = JT.fit_model(rows, hist, below_tids, tpe._default_prior_weight, tpe.DEFAULT_LF)
        rec, cand, l, g = engine.run_joint_segments([model], [JT.branch_stream_word(rows)], [0], ids, C_PUBLIC, SEED,
                                                    return_cand=True, want_lg=True)
        _check_group(gr, model, cand[0], l[0], g[0], gr.top, (name, gr.condition))
        assert gr.top['index'][0] == rec['global_idx'][0]
        assert gr.vectors[0].tobytes() == model.values(rec['z'][:1, :len(rows)])[0].tobytes()
        if int(got[gr.condition[0]]) == gr.condition[1]:
            taken += 1
            for d, lab in enumerate(gr.labels):
                assert np.float64(got[lab]).tobytes() == gr.vectors[0, d].tobytes(), (name, lab)
        else:
            assert not any(lab in got for lab in gr.labels)
    assert taken == (1 if name == 'branches' else 0)

    # the columns form and dicts()
    rep2 = tpe.joint_candidate_report_columns(table, hist, new_id, SEED, k=K_ENGINE, n_EI_candidates=C_PUBLIC, **kw)
    for a, b in zip(rep, rep2):
        assert a.labels == b.labels and a.vectors.tobytes() == b.vectors.tobytes() and a.top.tobytes() == b.top.tobytes()
        assert a.stats.tobytes() == b.stats.tobytes()
    dd = rep.dicts()
    assert len(dd) == len(rep) and dd[0]['top'][0]['vector'] == {lab: float(got[lab]) for lab in rep[0].labels}
