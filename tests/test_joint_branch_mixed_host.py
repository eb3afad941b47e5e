"""Discrete and quantised labels in branch groups (DESIGN.md "Discrete and
quantised labels in branch groups"), the parts that need no GPU: how
``joint_branches_mixed=True`` widens the branch groups, its argument errors,
the stream words, how the suggest builds the mixed segmented stage's problem
list and decodes its winners, the layout of the new structs, the size functions
and the checks tpe_joint_mseg_run makes before any launch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
NONE4 = (None,) * 4
ALL = dict(joint=True, joint_discrete=True, joint_quantized=True, joint_branches=True, joint_branches_mixed=True)


# ------------------------------------------------------------------- grouping
def bench_tree():
    """bench.py's benchmark tree, restated."""
    from hyperopt_amd import base, hp
    space = {'model': hp.choice('model', [
        {'name': 'svm', 'C': hp.loguniform('svm_C', -5, 5),
         'kernel': hp.choice('svm_kernel', [{'gamma': hp.loguniform('svm_rbf_gamma', -5, 2)},
                                            {'degree': hp.quniform('svm_poly_degree', 2, 5, 1)}])},
        {'name': 'rf', 'n_est': hp.quniform('rf_n_est', 10, 500, 10),
         'depth': hp.choice('rf_depth', [None, hp.quniform('rf_depth_n', 2, 30, 1)]),
         'crit': hp.choice('rf_crit', ['gini', 'entropy'])},
        {'name': 'knn', 'k': hp.quniform('knn_k', 1, 50, 1), 'p': hp.uniform('knn_p', 1, 3)}])}
    return base.Domain(lambda d: 0.0, space)


def _tree():
    """tests/test_joint_branch_host.py's tree, restated: two gates (clf, opt), a
    nested gate (svm_kernel under clf = 0), a label shared by both clf branches,
    a conditional quniform (rf_n), a conditional discrete label that gates
    nothing (sgd_sched) and two one-label branches (rbf_w, adam_lr)."""
    from hyperopt_amd import base, hp
    shared = hp.uniform('shared', 0, 1)
    space = {
        'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 2),
        'clf': hp.choice('clf', [
            {'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0), 'shared': shared,
             'kernel': hp.choice('svm_kernel', [{'a': hp.uniform('poly_a', 1, 5), 'b': hp.normal('poly_b', 0, 1)},
                                                {'w': hp.uniform('rbf_w', 0, 1)}])},
            {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.lognormal('rf_split', 0, 1),
             'n': hp.quniform('rf_n', 10, 100, 10), 'shared': shared}]),
        'opt': hp.choice('opt', [
            {'lr': hp.loguniform('sgd_lr', -9, 0), 'mom': hp.uniform('sgd_mom', 0, 1),
             'sched': hp.choice('sgd_sched', [0, 1])},
            {'lr': hp.loguniform('adam_lr', -9, 0)}]),
    }
    return base.Domain(lambda d: 0.0, space)


def _labels(groups):
    return [[r.label for r in g] for g in groups]


def test_groups_of_the_benchmark_tree():
    from hyperopt_amd import tpe
    t = bench_tree().table
    root, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, True)
    assert root is None and _labels(groups) == [['knn_k', 'knn_p'], ['rf_crit', 'rf_n_est']]
    c, d, q = tpe._joint_kernel_order(groups[0])
    assert [r.label for r in c + d + q] == ['knn_p', 'knn_k'] and (len(c), len(d), len(q)) == (1, 0, 1)
    c, d, q = tpe._joint_kernel_order(groups[1])
    assert [r.label for r in c + d + q] == ['rf_crit', 'rf_n_est'] and (len(c), len(d), len(q)) == (0, 1, 1)
    joined = set(r.label for g in groups for r in g)
    assert set(t.labels) - joined == {'rf_depth', 'svm_kernel', 'model', 'svm_C', 'svm_rbf_gamma', 'svm_poly_degree',
                                      'rf_depth_n'}
    assert [tpe._branch_condition(g[0]) for g in groups] == [('model', 2), ('model', 1)]
    # without the new keyword the tree joins nothing, as before
    with pytest.raises(ValueError, match='at least 2 labels to join in one group'):
        tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True)
    with pytest.raises(ValueError, match='at least 2 labels to join in one group'):
        tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, False)


def test_widened_groups_of_a_tree_space():
    from hyperopt_amd import tpe
    t = _tree().table
    today = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True)
    assert _labels(today[1]) == [['poly_a', 'poly_b'], ['rf_depth', 'rf_split'], ['sgd_lr', 'sgd_mom'],
                                 ['svm_C', 'svm_gamma']]
    assert tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, False) == today
    root, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, True)
    assert [r.label for r in root] == ['x', 'y']
    assert _labels(groups) == [['poly_a', 'poly_b'], ['rf_depth', 'rf_n', 'rf_split'],
                               ['sgd_lr', 'sgd_mom', 'sgd_sched'], ['svm_C', 'svm_gamma']]
    # joint_discrete alone: only sgd_sched joins; joint_quantized alone: only rf_n
    _, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, False, False, True, True)
    assert _labels(groups) == [['poly_a', 'poly_b'], ['rf_depth', 'rf_split'], ['sgd_lr', 'sgd_mom', 'sgd_sched'],
                               ['svm_C', 'svm_gamma']]
    _, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, False, True, False, True, True)
    assert _labels(groups) == [['poly_a', 'poly_b'], ['rf_depth', 'rf_n', 'rf_split'], ['sgd_lr', 'sgd_mom'],
                               ['svm_C', 'svm_gamma']]
    # neither: the keyword widens nothing
    assert tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, False, False, False, True, True) == \
        tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, branches=True)
    # gates, the shared label and the one-label branches stay univariate
    joined = set(r.label for g in tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, True)[1]
                 for r in g)
    assert not joined & {'clf', 'opt', 'svm_kernel', 'shared', 'rbf_w', 'adam_lr'}


def test_named_conditional_discrete_and_quantised_labels():
    from hyperopt_amd import tpe
    t = _tree().table
    root, groups = tpe._joint_plan(t, ['sgd_sched', 'rf_n', 'x', 'rf_depth', 'y', 'sgd_mom'], 'philox', 'fp32', NONE4,
                                   True, True, False, True, True)
    assert [r.label for r in root] == ['x', 'y']
    assert _labels(groups) == [['rf_depth', 'rf_n'], ['sgd_mom', 'sgd_sched']]
    # without the keyword a named conditional quantised label raises as it does today
    with pytest.raises(ValueError, match="'rf_n' is not eligible"):
        tpe._joint_plan(t, ['rf_n', 'rf_depth'], 'philox', 'fp32', NONE4, True, True, False, True)


def test_stream_words_of_the_widened_groups():
    from hyperopt_amd import joint as J, tpe
    for t in (bench_tree().table, _tree().table):
        _, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True, True)
        words = [J.branch_stream_word(g) for g in groups]
        assert words == [0xFFFFFFFE - min(r.index for r in g) for g in groups]
        assert len(set(words)) == len(words) and all(2 ** 31 <= w < N.JOINT_STREAM for w in words)
    # the word comes from ALL the labels: knn_k (quantised) has the lowest index of its group
    t = bench_tree().table
    words = [J.branch_stream_word(g) for g in tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False,
                                                              True, True)[1]]
    assert words[0] == 0xFFFFFFFE - t.by_label['knn_k'].index != 0xFFFFFFFE - t.by_label['knn_p'].index


# ------------------------------------------------------------ argument errors
def _wide_branch(n_cont=0, n_disc=0, lattices=()):
    from hyperopt_amd import base, hp
    opt = {}
    for i in range(n_cont):
        opt['u%d' % i] = hp.uniform('u%d' % i, 0, 1)
    for i in range(n_disc):
        opt['d%d' % i] = hp.choice('d%d' % i, [0, 1, 2])
    for i, hi in enumerate(lattices):
        opt['q%d' % i] = hp.quniform('q%d' % i, 0, hi, 1)
    return base.Domain(lambda d: 0.0, {'gate': hp.choice('gate', [{'only': hp.uniform('only', 0, 1)}, opt])})


def _odd_tree():
    """A qnormal under a branch and a quantised label shared by two branches."""
    from hyperopt_amd import base, hp
    both = hp.quniform('both', 0, 10, 1)
    return base.Domain(lambda d: 0.0, {'g': hp.choice('g', [
        {'a': hp.uniform('a', 0, 1), 'qn': hp.qnormal('qn', 0, 5, 1), 'both': both},
        {'b': hp.uniform('b', 0, 1), 'c': hp.uniform('c', 0, 1), 'both': both}])})


@pytest.mark.parametrize('domain,kw,match', [
    (_tree, dict(joint=True, joint_branches_mixed=True), 'joint_branches_mixed=True needs joint_branches=True'),
    (_tree, dict(joint_branches_mixed=True), 'joint_branches_mixed=True needs joint_branches=True'),
    (_tree, dict(ALL, joint=['svm_C', 'svm_gamma', 'svm_kernel']),
     "'svm_kernel' is not eligible with joint_branches_mixed=True: a gate"),
    (_odd_tree, dict(ALL, joint=['b', 'c', 'qn']),
     "'qn' is not eligible with joint_branches_mixed=True: qnormal: its lattice is unbounded"),
    (_odd_tree, dict(ALL, joint=['b', 'c', 'both']),
     "'both' is not eligible with joint_branches_mixed=True: it has 2 parents"),
    (lambda: _wide_branch(9, 0, (5,)), ALL,
     r"option 1 of gate 'gate' has 9 continuous labels beside a discrete or quantised one, more than 8.*joint=\["),
    (lambda: _wide_branch(1, 5), ALL, r"option 1 of gate 'gate' has 5 discrete labels, more than 4.*joint=\["),
    (lambda: _wide_branch(1, 0, (254, 255, 1)), ALL,
     r"option 1 of gate 'gate' has 513 lattice values in all, more than TPE_JOINT_MAX_LATTICE_TOTAL = 512.*joint=\["),
    (_tree, dict(ALL, joint=['x', 'y', 'sgd_sched']),
     "'sgd_sched' is the only label named under option 0 of gate 'opt'"),
])
def test_argument_errors(domain, kw, match):
    from hyperopt_amd import base, history, tpe
    d = domain()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)
    if kw.get('joint'):
        with pytest.raises(ValueError, match=match):
            tpe.joint_candidate_report(0, d, base.Trials(), 1, **kw)


def test_limits_hold_at_their_edges():
    from hyperopt_amd import tpe
    _, groups = tpe._joint_plan(_wide_branch(8, 4, (254, 255)).table, True, 'philox', 'fp32', NONE4, True, True, False,
                                True, True)
    assert len(groups) == 1 and len(groups[0]) == 14
    # a branch group of continuous labels only keeps its limit of 16
    _, groups = tpe._joint_plan(_wide_branch(16).table, True, 'philox', 'fp32', NONE4, True, True, False, True, True)
    assert len(groups[0]) == 16
    with pytest.raises(ValueError, match='17 labels'):
        tpe._joint_plan(_wide_branch(17).table, True, 'philox', 'fp32', NONE4, True, True, False, True, True)


# ------------------------------------------- the suggest's problem list, no GPU
def _trials(domain, n, loss):
    from hyperopt_amd import base, rand
    trials = base.Trials()
    rs = np.random.RandomState(3)
    for tid in range(n):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(loss(v, rs))}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return trials


class _Recorder(object):
    """Stands in for the Engine: records the calls; problem p's winner is the
    kernel vector (p + 1, p + 1.5, 1, 0, ...)."""

    def __init__(self):
        self.calls = []

    def run_joint(self, below, above, low, high, ids, n_cand, seed, **kw):
        self.calls.append(('run_joint', np.array(ids), n_cand, seed, kw))
        return np.zeros(len(ids), dtype=N.JOINT_RECORD_DTYPE)

    def run_joint_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, **kw):
        self.calls.append(('run_joint_segments', models, list(stream_words), list(prob_seg), list(prob_id), n_cand,
                           seed, kw))
        rec = np.zeros(len(prob_seg), dtype=N.JOINT_RECORD_DTYPE)
        rec['z'][:, 0] = np.arange(len(rec)) + 1.0
        rec['z'][:, 1] = np.arange(len(rec)) + 1.5
        rec['z'][:, 2] = 1.0
        return rec


def test_problem_list_models_and_decoded_winners(monkeypatch):
    from hyperopt_amd import history, joint as J, tpe
    d = _tree()
    t = d.table
    hist = history.extract(d, _trials(d, 40, lambda v, rs: rs.uniform()))
    ix = dict((k, t.by_label[k].index) for k in t.labels)
    ids = [40, 41, 42, 43]
    clf, opt = [1, 1, 1, 1], [0, 1, 0, 0]               # nobody takes the svm branch; id 41 takes adam
    base = np.full((4, len(t.rows)), np.nan)
    for j in range(4):
        for k in ('x', 'y', 'shared', 'rf_depth', 'rf_split'):
            base[j, ix[k]] = 0.25
        base[j, ix['clf']], base[j, ix['opt']], base[j, ix['rf_n']] = clf[j], opt[j], 30.0
        if opt[j] == 0:
            base[j, ix['sgd_lr']], base[j, ix['sgd_mom']], base[j, ix['sgd_sched']] = 0.1, 0.2, 0.0
        else:
            base[j, ix['adam_lr']] = 0.3
    act = ~np.isnan(base)
    rec = _Recorder()
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: rec)
    monkeypatch.setattr(tpe, '_suggest_local', lambda table, *a, **k: tpe.ChoiceColumns(table.labels, base.copy(),
                                                                                         act.copy()))
    cc = tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, columns=True, **ALL)
    assert [c[0] for c in rec.calls] == ['run_joint', 'run_joint_segments']
    _, models, words, prob_seg, prob_id, n_cand, seed, kw = rec.calls[1]
    # groups by their first label: (rf_depth, rf_n, rf_split), then (sgd_lr, sgd_mom, sgd_sched); the branches no id
    # takes (poly, svm) are not fitted
    assert [type(m) for m in models] == [J.QuantModel, J.MixedModel]
    q, m = models
    assert [r.label for r in q.rows + q.drows + q.qrows] == ['rf_depth', 'rf_split', 'rf_n']
    assert [r.label for r in m.rows + m.drows] == ['sgd_lr', 'sgd_mom', 'sgd_sched']
    assert words == [0xFFFFFFFE - ix['rf_depth'], 0xFFFFFFFE - ix['sgd_lr']]
    assert prob_seg == [0, 0, 0, 0, 1, 1, 1] and prob_id == [40, 41, 42, 43, 40, 42, 43]
    assert (n_cand, seed, kw) == (512, 77, {})
    below = history.split_below(hist, tpe._default_gamma)
    want = J.fit_quant_model(q.rows, q.drows, q.qrows, hist, below, tpe._default_prior_weight, tpe.DEFAULT_LF)
    for got, ref in zip(q.below + q.above, want.below + want.above):
        np.testing.assert_array_equal(got, ref)
    assert q.lattices[0][:3] == want.lattices[0][:3] == (1, 10, 10.0)
    want = J.fit_mixed_model(m.rows, m.drows, hist, below, tpe._default_prior_weight, tpe.DEFAULT_LF)
    for got, ref in zip(m.below + m.above, want.below + want.above):
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(m.s_below, want.s_below)
    # winners decoded through model.values into the taken branch's columns only
    np.testing.assert_array_equal(cc.active, act)
    v = cc.values
    assert v[:, ix['rf_depth']].tolist() == [1.0, 2.0, 3.0, 4.0]
    np.testing.assert_array_equal(v[:, ix['rf_split']], np.exp([1.5, 2.5, 3.5, 4.5]))
    assert v[:, ix['rf_n']].tolist() == [20.0] * 4                              # lattice index 1: (m_lo + 1) q
    np.testing.assert_array_equal(v[[0, 2, 3], ix['sgd_lr']], np.exp([5.0, 6.0, 7.0]))
    assert v[[0, 2, 3], ix['sgd_mom']].tolist() == [5.5, 6.5, 7.5]
    assert v[[0, 2, 3], ix['sgd_sched']].tolist() == [1.0, 1.0, 1.0]
    assert np.isnan(v[1, [ix['sgd_lr'], ix['sgd_mom'], ix['sgd_sched']]]).all() and v[1, ix['adam_lr']] == 0.3
    assert (v[:, ix['shared']] == 0.25).all() and v[:, ix['clf']].tolist() == clf and v[:, ix['opt']].tolist() == opt
    assert np.isnan(v[:, ix['svm_C']]).all()
    # a category is typed as the univariate path types it, a quantised value as the root group's
    docs = tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, **ALL)
    assert type(docs[0]['sgd_sched']) is type(tpe._value(t.by_label['sgd_sched'], 1.0)) is np.int64
    assert docs[0]['sgd_sched'] == 1 and docs[1]['sgd_sched'] is None
    assert type(docs[0]['rf_n']) is np.float64 and docs[0]['rf_n'] == 20.0


def test_branch_without_an_observer_gives_one_row_sides():
    from hyperopt_amd import base, history, hp, tpe
    opts = [{'a': hp.uniform('a', 0, 1)},
            {'n': hp.quniform('n', 1, 20, 1), 'c': hp.choice('c', [0, 1, 2]), 'u': hp.uniform('u', 0, 1)}]
    d = base.Domain(lambda d: 0.0, {'g': hp.pchoice('g', list(zip([1.0, 0.0], opts)))})
    hist = history.extract(d, _trials(d, 20, lambda v, rs: rs.uniform()))
    rows = [d.table.by_label[k] for k in ('c', 'n', 'u')]
    ordered, model = tpe._fit_branch_model(rows, hist, history.split_below(hist, 0.25), 1.0)
    assert [r.label for r in ordered] == ['u', 'c', 'n']
    for side in (model.below, model.above):
        w, mu, sigma, xc, qmu, qsig = side
        assert w.tolist() == [1.0] and mu.shape == (1, 1) and xc.tolist() == [[-1]] and qmu.shape == qsig.shape == (1, 1)


# ------------------------------------------------------------------------ ABI
def test_mseg_structs_match_c():
    lines = ['printf("tpe_joint_mseg %zu\\ntpe_joint_mseg_args %zu\\ntpe_joint_seg %zu\\n", sizeof(tpe_joint_mseg), '
             'sizeof(tpe_joint_mseg_args), sizeof(tpe_joint_seg));']
    for f, _ in N.JointMSeg._fields_:
        lines.append('printf("tpe_joint_mseg.%s %%zu\\n", offsetof(tpe_joint_mseg, %s));' % (f, f))
    for f, _ in N.JointMSegArgs._fields_:
        lines.append('printf("tpe_joint_mseg_args.%s %%zu\\n", offsetof(tpe_joint_mseg_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 's.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 's')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['tpe_joint_mseg'] == ctypes.sizeof(N.JointMSeg) == N.JOINT_MSEG_DTYPE.itemsize == 464
    assert lay['tpe_joint_mseg_args'] == ctypes.sizeof(N.JointMSegArgs)
    assert [f for f, _ in N.JointMSeg._fields_] == list(N.JOINT_MSEG_DTYPE.names)
    for f, _ in N.JointMSeg._fields_:
        assert getattr(N.JointMSeg, f).offset == N.JOINT_MSEG_DTYPE.fields[f][1] == lay['tpe_joint_mseg.' + f], f
    for f, _ in N.JointSeg._fields_:                                          # tpe_joint_seg's fields come first
        assert getattr(N.JointMSeg, f).offset == getattr(N.JointSeg, f).offset, f
    assert N.JointMSeg.n_cat.offset == lay['tpe_joint_seg']
    for f, _ in N.JointMSegArgs._fields_:
        assert getattr(N.JointMSegArgs, f).offset == lay['tpe_joint_mseg_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_mseg_scratch_bytes', 'tpe_joint_mseg_table_bytes', 'tpe_joint_mseg_run'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == N.ABI_VERSION == 24


C_HOST = 2048
# (n_dims, n_cat, n_quant, k_below, k_above, U, V) of the three segments of _host_args
SEGS = ((3, 0, 0, 4, 9, (), ()), (2, 1, 0, 3, 5, (3,), ()), (1, 1, 2, 2, 7, (2,), (5, 4)))


def _host_args(keep, probs=(0, 1, 2, 2), inject=False, **over):
    """Complete arguments whose 'device' pointers are host arrays: only good for
    calls that return before any launch (the scratch check is the last one and
    _run passes no scratch unless asked).  Every array of a segment lies in its
    pool behind the one before; the f32 pool ends with the last segment's
    quant_samp, the f64 pool with its above_qsigma, the table workspace with
    its table."""
    segs = np.zeros(len(SEGS), dtype=N.JOINT_MSEG_DTYPE)
    n32 = n64 = ntab = 0
    for s, (Dc, Dk, Dq, kb, ka, U, V) in enumerate(SEGS):
        g = segs[s]
        g['n_dims'], g['n_cat'], g['n_quant'], g['k_below'], g['k_above'] = Dc, Dk, Dq, kb, ka
        g['stream_word'], g['inject'] = 0xFFFFFFFE - s, -1
        ct, vt = sum(U), sum(V)
        for f, n in (('below_mu', kb * Dc), ('below_a', kb * Dc), ('below_c', kb), ('above_mu', ka * Dc),
                     ('above_a', ka * Dc), ('above_c', ka), ('samp', kb * Dc * 5), ('below_cat', kb * Dk),
                     ('above_cat', ka * Dk), ('below_miss', ct), ('below_bonus', ct), ('above_miss', ct),
                     ('above_bonus', ct), ('quant_samp', kb * Dq * 5)):
            g[f] = n32
            n32 += n
        g['n_edges'] = vt + Dq
        for f, n in (('samp_cum', kb), ('below_h', Dk), ('cat_cum', ct), ('quant_edges', vt + Dq),
                     ('below_qmu', kb * Dq), ('below_qsigma', kb * Dq), ('above_qmu', ka * Dq),
                     ('above_qsigma', ka * Dq)):
            g[f] = n64
            n64 += n
        g['cat_upper'][:Dk], g['cat_off'][:Dk] = U, np.cumsum((0,) + U[:-1])
        g['quant_v'][:Dq], g['quant_edge_off'][:Dq] = V, np.cumsum((0,) + tuple(v + 1 for v in V[:-1]))
        g['table'] = ntab
        ntab += (kb + ka) * vt
    prob_seg = np.array(probs, dtype=np.int32)
    pool = np.zeros(4096)
    keep.extend([segs, prob_seg, pool])
    a = N.JointMSegArgs()
    a.n_segs, a.n_probs, a.n_cand, a.flags, a.seed = len(segs), len(prob_seg), C_HOST, int(inject), 7
    a.segs = a.host_segs = segs.ctypes.data
    a.pool_f32 = a.pool_f64 = a.prob_id = a.quant_table = pool.ctypes.data
    a.pool_f32_len, a.pool_f64_len, a.quant_table_bytes = n32, n64, 4 * ntab
    a.prob_seg = a.host_prob_seg = prob_seg.ctypes.data
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, cand=False, scratch_bytes=0):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_mseg_run(ctypes.byref(a) if a is not None else None, p if records else None,
                                  p if cand else None, None, None, p if scratch_bytes else None, scratch_bytes, None)


def test_size_functions():
    lib, keep = N.load(), []
    nb = ctypes.c_uint64(0)
    # the order (int32 per problem, padded to 8 bytes), then one record per problem and chunk
    for n_probs, C, want in ((1, 1, 8 + 152), (2, 1024, 8 + 2 * 152), (7, 4097, 32 + 35 * 152)):
        assert lib.tpe_joint_mseg_scratch_bytes(n_probs, C, ctypes.byref(nb)) == 0 and nb.value == want
    assert lib.tpe_joint_mseg_scratch_bytes(0, 8, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_mseg_scratch_bytes(1, 8, None) == -1
    # (k_below + k_above) sum V floats per quantised segment: only the third of SEGS, (2 + 7) (5 + 4) = 81
    _host_args(keep)
    segs = keep[0]
    assert lib.tpe_joint_mseg_table_bytes(segs.ctypes.data, 3, ctypes.byref(nb)) == 0 and nb.value == 4 * 81
    assert lib.tpe_joint_mseg_table_bytes(segs.ctypes.data, 2, ctypes.byref(nb)) == 0 and nb.value == 0
    two = np.concatenate([segs[2:], segs[2:]])
    two[1]['k_below'], two[1]['quant_v'][:2] = 300, (256, 256)
    assert lib.tpe_joint_mseg_table_bytes(two.ctypes.data, 2, ctypes.byref(nb)) == 0
    assert nb.value == 4 * (81 + (300 + 7) * 512)
    two[1]['quant_v'][0] = 257
    assert lib.tpe_joint_mseg_table_bytes(two.ctypes.data, 2, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_mseg_table_bytes(None, 2, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_mseg_table_bytes(segs.ctypes.data, 0, ctypes.byref(nb)) == -1


def test_complete_arguments_reach_the_scratch_check():
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep), keep) == -1 and b'scratch too small' in lib.tpe_last_error()
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_mseg_scratch_bytes(4, C_HOST, ctypes.byref(need)) == 0
    assert _run(lib, _host_args(keep), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    # a segment with no problem is legal
    assert _run(lib, _host_args(keep, probs=(2,)), keep) == -1 and b'scratch too small' in lib.tpe_last_error()
    # under TPE_JOINT_INJECT only the segments that have a problem need candidates, [n_cand * (Dc + Dk + Dq)]
    k3 = []
    a = _host_args(k3, probs=(2, 2), inject=True)
    k3[0][2]['inject'] = 0
    a.pool_f32_len = max(a.pool_f32_len, C_HOST * 4)
    assert _run(lib, a, k3) == -1 and b'scratch too small' in lib.tpe_last_error()
    k3[0][2]['inject'] = a.pool_f32_len - C_HOST * 4 + 1
    assert _run(lib, a, k3) == -1 and b'leave its pool' in lib.tpe_last_error()


@pytest.mark.parametrize('over,msg', [
    (dict(n_segs=0), b'n_segs < 1'), (dict(n_segs=32768), b'more than 32767 segments'),
    (dict(n_probs=0), b'n_probs < 1'), (dict(n_cand=0), b'n_cand < 1'),
    (dict(segs=None), b'null segs'), (dict(host_segs=None), b'null segs / host_segs'),
    (dict(pool_f32=None), b'null pool'), (dict(pool_f64=None), b'null pool'),
    (dict(prob_seg=None), b'null prob_seg'), (dict(host_prob_seg=None), b'null prob_seg / host_prob_seg'),
    (dict(prob_id=None), b'prob_id'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(flags=N.JOINT_INJECT, pool_f64=None), b'null pool_f64 with a quantised segment'),
    (dict(quant_table=None), b'null table workspace with a quantised segment'),
    (dict(quant_table_bytes=4 * 81 - 1), b'table leaves the table workspace'),
    (dict(pool_f32_len=-1), b'leave its pool'), (dict(pool_f64_len=-1), b'leave its pool'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    a = _host_args(keep)
    for k in ('pool_f32_len', 'pool_f64_len'):                  # -1: one element short of what the segments need
        if over.get(k) == -1:
            over = dict(over, **{k: getattr(a, k) - 1})
    for k, v in over.items():
        setattr(a, k, v)
    assert _run(lib, a, keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def _edit(s, **fields):
    def edit(segs):
        for k, v in fields.items():
            if isinstance(v, tuple):
                segs[s][k][v[0]] = v[1]
            else:
                segs[s][k] = v
    return edit


@pytest.mark.parametrize('edit,msg', [
    (_edit(0, n_dims=0), b'n_dims outside [1, TPE_JOINT_MAX_DIMS]'), (_edit(0, n_dims=17), b'n_dims outside'),
    (_edit(1, n_dims=-1), b'n_dims < 0'),
    (_edit(1, n_dims=9), b'n_dims > 8 or n_cat > 4'), (_edit(2, n_dims=9), b'n_dims > 8 or n_cat > 4'),
    (_edit(1, n_cat=5), b'n_dims > 8 or n_cat > 4'), (_edit(1, n_cat=-1), b'n_cat outside'),
    (_edit(2, n_quant=5), b'n_quant outside [0, TPE_JOINT_MAX_QUANT]'), (_edit(2, n_quant=-1), b'n_quant outside'),
    (_edit(1, k_below=0), b'k_below < 1'), (_edit(2, k_above=0), b'k_below < 1 or k_above < 1'),
    (_edit(1, cat_upper=(0, 1)), b'categories of a label outside [2, TPE_JOINT_MAX_CATS]'),
    (_edit(1, cat_upper=(0, 257)), b'categories of a label outside'),
    (_edit(1, cat_off=(0, 1)), b'cat_off outside the tables'), (_edit(2, cat_off=(0, -1)), b'cat_off outside'),
    (_edit(2, quant_v=(1, 1)), b'lattice values of a label outside [2, TPE_JOINT_MAX_LATTICE]'),
    (_edit(2, quant_v=(0, 257)), b'lattice values of a label outside'),
    (_edit(2, quant_edge_off=(1, 7)), b'quant_edge_off outside the edge array'),
    (_edit(2, quant_edge_off=(0, -1)), b'quant_edge_off outside'),
    (_edit(0, below_mu=-1), b'leave its pool'), (_edit(1, above_cat=1 << 40), b'leave its pool'),
    (_edit(1, below_bonus=1 << 20), b'leave its pool'), (_edit(1, cat_cum=1 << 20), b'leave its pool'),
    (_edit(1, below_h=-1), b'leave its pool'), (_edit(2, quant_samp=1 << 20), b'leave its pool'),
    (_edit(2, quant_edges=1 << 20), b'leave its pool'), (_edit(2, n_edges=1 << 20), b'leave its pool'),
    (_edit(2, above_qsigma=1 << 20), b'leave its pool'), (_edit(2, below_qmu=-1), b'leave its pool'),
    (_edit(2, table=1), b'table leaves the table workspace'), (_edit(2, table=-1), b'table leaves'),
])
def test_bad_segments_are_rejected_without_a_device(edit, msg):
    lib, keep = N.load(), []
    a = _host_args(keep)
    edit(keep[0])
    assert _run(lib, a, keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_lattice_and_category_totals_null_outputs_and_bad_problems():
    lib, keep = N.load(), []
    a = _host_args(keep)
    keep[0][2]['n_quant'], keep[0][2]['quant_v'][:3] = 3, (256, 256, 2)
    assert _run(lib, a, keep) == -1 and b'more than TPE_JOINT_MAX_LATTICE_TOTAL' in lib.tpe_last_error()
    # (4 discrete coordinates of 256 categories are TPE_JOINT_MAX_CAT_TOTAL exactly: that total cannot be exceeded)
    assert _run(lib, None, keep) == -1 and b'null args' in lib.tpe_last_error()
    for bad in ((0, 3, 1), (0, -1), (5,)):
        k = []
        assert _run(lib, _host_args(k, probs=bad), k) == -1
        assert b'prob_seg outside [0, n_segs)' in lib.tpe_last_error()
    k = []
    assert _run(lib, _host_args(k), k, records=False) == -1 and b'null records' in lib.tpe_last_error()
    assert _run(lib, _host_args(k), k, cand=True) == -1 and b'cand without cand_off' in lib.tpe_last_error()
