"""Joint TPE on conditional branches (DESIGN.md "Branch groups"), the parts that
need no GPU: how ``joint_branches=True`` groups the labels of a tree space, its
argument errors, the joint model of a branch, the layout of the segmented
stage's structs, the checks tpe_joint_seg_run makes before any launch, and how
the suggest builds the stage's problem list."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
NONE4 = (None,) * 4


# ------------------------------------------------------------------- grouping
def _tree():
    """Two gates (clf, opt), a nested gate (svm_kernel under clf = 0), a label
    shared by both clf branches, a conditional quniform (rf_n), a conditional
    discrete label that gates nothing (sgd_sched) and two one-label branches
    (rbf_w, adam_lr)."""
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


def test_branch_groups_of_a_tree_space():
    from hyperopt_amd import joint as J, tpe
    t = _tree().table
    assert t.labels == ['adam_lr', 'clf', 'opt', 'poly_a', 'poly_b', 'rbf_w', 'rf_depth', 'rf_n', 'rf_split', 'sgd_lr',
                        'sgd_mom', 'sgd_sched', 'shared', 'svm_C', 'svm_gamma', 'svm_kernel', 'x', 'y']
    assert len(t.by_label['shared'].parents) == 2
    root, groups = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, branches=True)
    assert [r.label for r in root] == ['x', 'y']
    # ordered by their first label; a nested label grouped by its own direct parent
    assert [[r.label for r in g] for g in groups] == [['poly_a', 'poly_b'], ['rf_depth', 'rf_split'],
                                                      ['sgd_lr', 'sgd_mom'], ['svm_C', 'svm_gamma']]
    assert [tpe._branch_key(g[0]) for g in groups] == [('svm_kernel', 0), ('clf', 1), ('opt', 0), ('clf', 0)]
    words = [J.branch_stream_word(g) for g in groups]
    assert words == [0xFFFFFFFE - 3, 0xFFFFFFFE - 6, 0xFFFFFFFE - 9, 0xFFFFFFFE - 13]
    assert len(set(words)) == 4 and all(2 ** 31 <= w < N.JOINT_STREAM for w in words)
    joined = set(r.label for g in groups for r in g) | set(r.label for r in root)
    # gates, the shared label, the conditional quantised and discrete labels, the one-label branches: univariate
    assert set(t.labels) - joined == {'clf', 'opt', 'svm_kernel', 'shared', 'rf_n', 'sgd_sched', 'rbf_w', 'adam_lr'}
    # the other keywords widen the root group only
    root2, groups2 = tpe._joint_plan(t, True, 'philox', 'fp32', NONE4, True, True, False, True)
    assert [r.label for r in root2] == ['x', 'y'] and groups2 == groups
    # without the keyword: the root group alone, as before
    assert tpe._joint_plan(t, True, 'philox', 'fp32', NONE4) == (root, [])


def test_only_branch_groups_skips_the_root_stage():
    from hyperopt_amd import base, hp, tpe
    d = base.Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'g': hp.choice('g', [
        {'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)}, {'c': hp.uniform('c', 0, 1)}])})
    root, groups = tpe._joint_plan(d.table, True, 'philox', 'fp32', NONE4, branches=True)
    assert root is None and [[r.label for r in g] for g in groups] == [['a', 'b']]
    with pytest.raises(ValueError, match='at least 2'):                       # the keyword's absence: as before
        tpe._joint_plan(d.table, True, 'philox', 'fp32', NONE4)


def test_named_labels_are_partitioned_by_condition():
    from hyperopt_amd import tpe
    t = _tree().table
    root, groups = tpe._joint_plan(t, ['svm_gamma', 'y', 'rf_split', 'svm_C', 'x', 'rf_depth'], 'philox', 'fp32', NONE4,
                                   branches=True)
    assert [r.label for r in root] == ['x', 'y']
    assert [[r.label for r in g] for g in groups] == [['rf_depth', 'rf_split'], ['svm_C', 'svm_gamma']]
    root, groups = tpe._joint_plan(t, ['poly_a', 'poly_b'], 'philox', 'fp32', NONE4, branches=True)
    assert root is None and [[r.label for r in g] for g in groups] == [['poly_a', 'poly_b']]


@pytest.fixture
def no_device(monkeypatch):
    """Every way to the device fails the test."""
    from hyperopt_amd import engine, tpe

    def boom(*a, **kw):
        pytest.fail('the device was touched')
    monkeypatch.setattr(tpe, 'get_engine', boom)
    monkeypatch.setattr(engine, 'get_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)
    lib = N.load()
    for name in ('tpe_joint_run', 'tpe_joint_seg_run', 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


@pytest.mark.parametrize('kw,match', [
    (dict(joint_branches=True), 'joint_branches=True needs joint=True or joint='),
    (dict(joint=None, joint_branches=True), 'joint_branches=True needs joint=True or joint='),
    (dict(joint=['svm_C', 'x', 'y'], joint_branches=True), r"'svm_C' is the only label named under option 0 of gate 'clf'"),
    (dict(joint=['svm_C', 'svm_gamma', 'x'], joint_branches=True), "'x' is the only unconditional label named"),
    (dict(joint=['svm_C', 'rf_depth'], joint_branches=True), "'rf_depth' is the only label named under option 1"),
    (dict(joint=['svm_C', 'svm_gamma', 'shared'], joint_branches=True), "'shared' is not eligible"),
    (dict(joint=['svm_C', 'svm_gamma', 'rf_n'], joint_branches=True), "'rf_n' is not eligible"),
    (dict(joint=['svm_C', 'svm_gamma', 'sgd_sched'], joint_branches=True), "'sgd_sched' is not eligible"),
    (dict(joint=['svm_C', 'svm_gamma', 'svm_kernel'], joint_branches=True), "'svm_kernel' is not eligible"),
    (dict(joint=['svm_C', 'nope'], joint_branches=True), "'nope' is not a label"),
    (dict(joint=[], joint_branches=True), 'at least 2'),
    (dict(joint='svm_C', joint_branches=True), 'not the string'),
    # without the keyword a conditional label raises as before
    (dict(joint=['svm_C', 'svm_gamma']), r"label 'svm_C' is not eligible \(loguniform, conditional\): only unconditional"),
    (dict(joint=True, joint_branches=True, sampler='replay'), 'replay'),
    (dict(joint=True, joint_branches=True, precision='fp64'), 'fp64'),
    (dict(joint=True, joint_branches=True, shard=(0, 2)), 'shard'),
    (dict(joint=True, joint_branches=True, shard_ids=(0, 2)), 'shard'),
    (dict(joint=True, joint_branches=True, shard_labels=(0, 2)), 'shard'),
    (dict(joint=True, joint_branches=True, shard_grid=(0, 2)), 'shard'),
])
def test_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = _tree()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


def test_group_sizes(no_device):
    """A branch of one label raises nothing; of 17 labels a ValueError naming
    the gate and the option; no group of 2 anywhere: 'at least 2'."""
    from hyperopt_amd import base, hp, tpe
    big = base.Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'gate': hp.choice('gate', [
        {'only': hp.uniform('only', 0, 1)}, dict(('u%02d' % i, hp.uniform('u%02d' % i, 0, 1)) for i in range(17))])})
    with pytest.raises(ValueError, match=r"option 1 of gate 'gate' has 17 labels.*TPE_JOINT_MAX_DIMS = 16.*joint=\["):
        tpe.suggest([0], big, base.Trials(), 1, joint=True, joint_branches=True)
    sixteen = ['u%02d' % i for i in range(16)]
    root, groups = tpe._joint_plan(big.table, sixteen, 'philox', 'fp32', NONE4, branches=True)
    assert root is None and [r.label for r in groups[0]] == sixteen
    with pytest.raises(ValueError, match='17 labels'):
        tpe._joint_plan(big.table, sixteen + ['u16'], 'philox', 'fp32', NONE4, branches=True)
    small = base.Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'gate': hp.choice('gate', [
        {'only': hp.uniform('only', 0, 1)}, {'other': hp.uniform('other', 0, 1)}])})
    with pytest.raises(ValueError, match='at least 2'):
        tpe.suggest([0], small, base.Trials(), 1, joint=True, joint_branches=True)


# ------------------------------------------------------- the model of a branch
def _two_branch(p=None):
    from hyperopt_amd import base, hp
    opts = [{'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
            {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.uniform('rf_split', 0, 1)}]
    clf = hp.choice('clf', opts) if p is None else hp.pchoice('clf', list(zip(p, opts)))
    return base.Domain(lambda d: 0.0, {'clf': clf, 'x': hp.uniform('x', -5, 5), 'y': hp.uniform('y', -5, 5)})


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


def test_fit_model_on_a_branch_holds_its_observers_only():
    from hyperopt_amd import history, joint as J, tpe
    d = _two_branch()
    first = set()

    def loss(v, rs):                           # the first trial of each branch is its best: both branches have a below trial
        new = int(v['clf']) not in first
        first.add(int(v['clf']))
        return rs.uniform() - (2.0 if new else 0.0)
    trials = _trials(d, 60, loss)
    hist = history.extract(d, trials)
    below = np.asarray(history.split_below(hist, 0.25))
    assert len(below) == 2
    docs = sorted(trials.trials, key=lambda t: t['tid'])
    seen = 0
    for labels, logs in ((['svm_C', 'svm_gamma'], True), (['rf_depth', 'rf_split'], False)):
        rows = [d.table.by_label[k] for k in labels]
        model = J.fit_model(rows, hist, below, 1.0, tpe.DEFAULT_LF)
        obs = [t for t in docs if len(t['misc']['vals'][labels[0]])]
        X = np.array([[float(t['misc']['vals'][k][0]) for k in labels] for t in obs])
        X = np.log(X) if logs else X
        m = np.isin([t['tid'] for t in obs], below)
        assert 0 < len(obs) < 60 and m.any() and (~m).any()
        np.testing.assert_array_equal(model.below[1][1:], X[m])               # row 0: the prior
        np.testing.assert_array_equal(model.above[1][1:], X[~m])
        assert len(model.below[0]) == m.sum() + 1 and len(model.above[0]) == (~m).sum() + 1
        pb = [J.prior_and_bounds(r.dist, r.args) for r in rows]
        want = R.ref_side(X[m], np.array([p[0] for p in pb]), np.array([p[1] for p in pb]))
        for got, ref in zip(model.below, want):
            np.testing.assert_array_equal(got, ref)
        seen += len(obs)
    assert seen == 60                                                          # every trial took one branch


def test_unseen_branch_and_above_only_branch():
    """No observer: the prior row alone on both sides, and its device rows are
    finite with c = 0.  Observers only among the above trials: k_below = 1."""
    from hyperopt_amd import history, joint as J, tpe
    d = _two_branch(p=[1.0, 0.0])
    hist = history.extract(d, _trials(d, 30, lambda v, rs: rs.uniform()))
    rows = [d.table.by_label[k] for k in ('rf_depth', 'rf_split')]
    model = J.fit_model(rows, hist, history.split_below(hist, 0.25), 1.0, tpe.DEFAULT_LF)
    for side in (model.below, model.above):
        w, mu, sigma = side
        assert w.tolist() == [1.0] and mu.shape == sigma.shape == (1, 2)
        np.testing.assert_array_equal(mu[0], [10.5, 0.5])
        np.testing.assert_array_equal(sigma[0], [19.0, 1.0])
        m32, a32, c32, base = J.density_rows(w, mu, sigma, model.low, model.high)
        assert c32.tolist() == [0.0] and np.isfinite(base) and np.isfinite(a32).all()
    for x, y in zip(J.density_rows(*model.below, model.low, model.high),
                    J.density_rows(*model.above, model.low, model.high)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()              # so every score is exactly 0
    cum, samp = J.sampler_rows(*model.below, model.low, model.high)
    assert cum.tolist() == [1.0] and samp.shape == (1, 2, 5) and np.isfinite(samp).all()
    empty = J.side_mixture(np.zeros((0, 3)), [(0.0, 1.0)] * 3)
    assert empty[0].tolist() == [1.0] and empty[1].shape == (1, 3)

    d = _two_branch()
    hist = history.extract(d, _trials(d, 40, lambda v, rs: rs.uniform() + 10.0 * int(v['clf'])))
    below = history.split_below(hist, 0.25)
    model = J.fit_model(rows, hist, below, 1.0, tpe.DEFAULT_LF)               # the rf branch: clf = 1, every loss >= 10
    n_rf = len(hist.obs['rf_depth'][0])
    assert 0 < n_rf < 40 and len(model.below[0]) == 1 and len(model.above[0]) == n_rf + 1
    svm = J.fit_model([d.table.by_label[k] for k in ('svm_C', 'svm_gamma')], hist, below, 1.0, tpe.DEFAULT_LF)
    assert len(svm.below[0]) == len(below) + 1 and len(svm.above[0]) == 40 - n_rf - len(below) + 1


def test_f32_bounds_are_the_native_stage_s():
    from hyperopt_amd import joint as J
    low = np.array([-10.0, -np.inf, 0.1, np.exp(-3.0), -1e-300])
    high = np.array([10.0, np.inf, 0.3, np.exp(2.0), 16777217.0])
    lo, hi = J.f32_bounds(low, high)
    assert lo.dtype == hi.dtype == np.float32
    for d in range(len(low)):
        if np.isfinite(low[d]):
            assert float(lo[d]) >= low[d] and float(np.nextafter(lo[d], np.float32(-np.inf))) < low[d]
        else:
            assert lo[d] == -np.inf
        if np.isfinite(high[d]):
            assert float(hi[d]) < high[d] and float(np.nextafter(hi[d], np.float32(np.inf))) >= high[d]
        else:
            assert hi[d] == np.inf


# ------------------------------------------------------------------------ ABI
def test_segment_structs_match_c():
    lines = ['printf("TPE_ABI_VERSION %d\\n", TPE_ABI_VERSION);',
             'printf("tpe_joint_seg %zu\\ntpe_joint_seg_args %zu\\n", sizeof(tpe_joint_seg), sizeof(tpe_joint_seg_args));']
    for f, _ in N.JointSeg._fields_:
        lines.append('printf("tpe_joint_seg.%s %%zu\\n", offsetof(tpe_joint_seg, %s));' % (f, f))
    for f, _ in N.JointSegArgs._fields_:
        lines.append('printf("tpe_joint_seg_args.%s %%zu\\n", offsetof(tpe_joint_seg_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 's.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 's')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_seg'] == ctypes.sizeof(N.JointSeg) == N.JOINT_SEG_DTYPE.itemsize
    assert lay['tpe_joint_seg_args'] == ctypes.sizeof(N.JointSegArgs)
    assert [f for f, _ in N.JointSeg._fields_] == list(N.JOINT_SEG_DTYPE.names)
    for f, _ in N.JointSeg._fields_:
        assert getattr(N.JointSeg, f).offset == N.JOINT_SEG_DTYPE.fields[f][1] == lay['tpe_joint_seg.' + f], f
    for f, _ in N.JointSegArgs._fields_:
        assert getattr(N.JointSegArgs, f).offset == lay['tpe_joint_seg_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_seg_scratch_bytes', 'tpe_joint_seg_run'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ----------------------------------------------------- argument checks, no GPU
C_HOST = 2048


def _host_args(keep, probs=(0, 1, 1), inject=False, **over):
    """Complete arguments whose 'device' pointers are host arrays: only good for
    calls that return before any launch (the scratch check is the last one and
    _run passes no scratch unless asked)."""
    segs = np.zeros(2, dtype=N.JOINT_SEG_DTYPE)
    for s, (D, kb, ka) in enumerate(((3, 4, 9), (16, 1, 1))):
        g = segs[s]
        g['n_dims'], g['k_below'], g['k_above'], g['stream_word'] = D, kb, ka, 0xFFFFFFFE - s
        off = 1000 * s
        for f, n in (('below_mu', kb * D), ('below_a', kb * D), ('below_c', kb), ('above_mu', ka * D),
                     ('above_a', ka * D), ('above_c', ka), ('samp', kb * D * 5)):
            g[f] = off
            off += n
        g['samp_cum'], g['inject'] = 10 * s, -1
    prob_seg = np.array(probs, dtype=np.int32)
    pool = np.zeros(4096)
    keep.extend([segs, prob_seg, pool])
    a = N.JointSegArgs()
    a.n_segs, a.n_probs, a.n_cand, a.flags, a.seed = len(segs), len(prob_seg), C_HOST, int(inject), 7
    a.segs = a.host_segs = segs.ctypes.data
    a.pool_f32 = a.pool_f64 = a.prob_id = pool.ctypes.data
    a.pool_f32_len, a.pool_f64_len = 2000, 20
    a.prob_seg = a.host_prob_seg = prob_seg.ctypes.data
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, cand=False, scratch_bytes=0):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_seg_run(ctypes.byref(a) if a is not None else None, p if records else None,
                                 p if cand else None, None, None, p if scratch_bytes else None, scratch_bytes, None)


def _seg_edit(s, **fields):
    def edit(a, keep):
        segs = keep[0]
        for k, v in fields.items():
            segs[s][k] = v
    return edit


@pytest.mark.parametrize('over,msg', [
    (dict(n_segs=0), b'n_segs < 1'), (dict(n_probs=0), b'n_probs < 1'), (dict(n_cand=0), b'n_cand < 1'),
    (dict(segs=None), b'null segs'), (dict(host_segs=None), b'null segs / host_segs'),
    (dict(pool_f32=None), b'null pool'), (dict(pool_f64=None), b'null pool'),
    (dict(prob_seg=None), b'null prob_seg'), (dict(host_prob_seg=None), b'null prob_seg / host_prob_seg'),
    (dict(prob_id=None), b'prob_id'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(pool_f32_len=1145), b'leave its pool'), (dict(pool_f64_len=10), b'leave its pool'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


@pytest.mark.parametrize('edit,msg', [
    (_seg_edit(0, n_dims=0), b"n_dims outside"), (_seg_edit(1, n_dims=17), b"n_dims outside"),
    (_seg_edit(1, n_dims=-2), b"n_dims outside"),
    (_seg_edit(0, k_below=0), b'k_below < 1'), (_seg_edit(1, k_above=0), b'k_below < 1 or k_above < 1'),
    (_seg_edit(0, below_mu=-1), b'leave its pool'), (_seg_edit(1, above_c=2000), b'leave its pool'),
    (_seg_edit(0, samp_cum=17), b'leave its pool'), (_seg_edit(1, samp=1 << 40), b'leave its pool'),
])
def test_bad_segments_are_rejected_without_a_device(edit, msg):
    lib, keep = N.load(), []
    a = _host_args(keep)
    edit(a, keep)
    assert _run(lib, a, keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_bad_problems_null_outputs_and_small_scratch_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1 and b'null args' in lib.tpe_last_error()
    for bad in ((0, 2, 1), (0, -1), (5,)):
        assert _run(lib, _host_args(keep, probs=bad), keep) == -1
        assert b'prob_seg outside [0, n_segs)' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep), keep, records=False) == -1 and b'null records' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep), keep, cand=True) == -1 and b'cand without cand_off' in lib.tpe_last_error()
    # a segment with no problem is legal: the call gets as far as the scratch check
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_seg_scratch_bytes(3, C_HOST, ctypes.byref(need)) == 0
    assert need.value == 16 + 3 * 2 * N.JOINT_RECORD_DTYPE.itemsize            # the order (3 int32, padded), the chunks
    k2 = []
    assert _run(lib, _host_args(k2, probs=(1, 1, 1)), k2) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(k2), k2, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    # injected candidates: only the segments that have a problem need them
    k3 = []
    a = _host_args(k3, probs=(0, 0), inject=True)
    k3[0][0]['inject'] = 0
    a.pool_f32_len = C_HOST * 3
    assert _run(lib, a, k3) == -1 and b'scratch too small' in lib.tpe_last_error()
    a.pool_f32_len = C_HOST * 3 - 1
    assert _run(lib, a, k3) == -1 and b'leave its pool' in lib.tpe_last_error()
    nb = ctypes.c_uint64(0)
    for n_probs, C, want in ((1, 1, 8 + 152), (2, 1024, 8 + 2 * 152), (7, 4097, 32 + 35 * 152)):
        assert lib.tpe_joint_seg_scratch_bytes(n_probs, C, ctypes.byref(nb)) == 0 and nb.value == want
    assert lib.tpe_joint_seg_scratch_bytes(0, 8, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_seg_scratch_bytes(1, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_seg_scratch_bytes(1, 8, None) == -1


# ------------------------------------------- the suggest's problem list, no GPU
class _Recorder(object):
    """Stands in for the Engine in tpe._suggest_joint: records the calls;
    problem p's winner is the vector (p + 1, p + 1.5, 0, ...)."""

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
        return rec


def test_problem_list_follows_the_univariate_routing(monkeypatch):
    from hyperopt_amd import history, joint as J, tpe
    d = _two_branch()
    t = d.table
    hist = history.extract(d, _trials(d, 30, lambda v, rs: rs.uniform()))
    ix = dict((k, t.by_label[k].index) for k in t.labels)
    ids = [30, 31, 32, 33]
    clf = [1, 0, 1, 1]
    base = np.full((4, len(t.rows)), np.nan)
    act = np.zeros((4, len(t.rows)), dtype=bool)
    for j, c in enumerate(clf):
        base[j, ix['clf']], base[j, ix['x']], base[j, ix['y']] = c, 0.25, 0.5
        for k in (('svm_C', 'svm_gamma'), ('rf_depth', 'rf_split'))[c]:
            base[j, ix[k]] = 7.0
        act[j] = ~np.isnan(base[j])
    rec = _Recorder()
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: rec)
    monkeypatch.setattr(tpe, '_suggest_local', lambda table, *a, **k: tpe.ChoiceColumns(table.labels, base.copy(),
                                                                                         act.copy()))
    cc = tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, joint=True, joint_branches=True, columns=True)
    assert [c[0] for c in rec.calls] == ['run_joint', 'run_joint_segments']    # the root stage, then the segmented one
    assert rec.calls[0][1].tolist() == ids and rec.calls[0][2:] == (512, 77, {})
    _, models, words, prob_seg, prob_id, n_cand, seed, kw = rec.calls[1]
    # groups in table order: (rf_depth, rf_split) with ids 30, 32, 33, then (svm_C, svm_gamma) with id 31
    assert [[r.label for r in m.rows] for m in models] == [['rf_depth', 'rf_split'], ['svm_C', 'svm_gamma']]
    assert words == [0xFFFFFFFE - ix['rf_depth'], 0xFFFFFFFE - ix['svm_C']]
    assert prob_seg == [0, 0, 0, 1] and prob_id == [30, 32, 33, 31] and (n_cand, seed, kw) == (512, 77, {})
    want = J.fit_model(models[0].rows, hist, history.split_below(hist, tpe._default_gamma), tpe._default_prior_weight,
                       tpe.DEFAULT_LF)
    for got, ref in zip(models[0].below + models[0].above, want.below + want.above):
        np.testing.assert_array_equal(got, ref)
    # winners land in the taken branch's columns only; activity, the gate and the routing are the univariate pass's
    np.testing.assert_array_equal(cc.active, act)
    v = cc.values
    assert v[:, ix['clf']].tolist() == clf and (v[:, ix['x']] == 0).all() and (v[:, ix['y']] == 0).all()
    assert v[[0, 2, 3], ix['rf_depth']].tolist() == [1.0, 2.0, 3.0]
    assert v[[0, 2, 3], ix['rf_split']].tolist() == [1.5, 2.5, 3.5]
    assert v[1, ix['svm_C']] == np.exp(4.0) and v[1, ix['svm_gamma']] == np.exp(4.5)
    assert np.isnan(v[1, ix['rf_depth']]) and np.isnan(v[[0, 2, 3], ix['svm_C']]).all()

    # a branch no id takes is not fitted; only branch groups: no root stage
    rec.calls[:] = []
    act[:, ix['clf']] = True
    tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, joint=['rf_depth', 'rf_split', 'svm_C', 'svm_gamma'],
                        joint_branches=True)
    assert [c[0] for c in rec.calls] == ['run_joint_segments']
    base[1], act[1] = base[0], act[0]
    rec.calls[:] = []
    tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, joint=True, joint_branches=True)
    assert [[r.label for r in m.rows] for m in rec.calls[1][1]] == [['rf_depth', 'rf_split']]
    assert rec.calls[1][3] == [0, 0, 0, 0] and rec.calls[1][4] == ids
