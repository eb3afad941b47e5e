"""Joint candidate report (include/tpe_hip.h "Joint candidate report"), the
parts that need no GPU: the layout of its structs, the checks tpe_joint_report
makes before any launch, its scratch size, the numpy reference itself, and the
argument errors of tpe.joint_candidate_report."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_report_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')


# ------------------------------------------------------------------------ ABI
def test_report_structs_match_c():
    lines = ['printf("TPE_ABI_VERSION %d\\n", TPE_ABI_VERSION);',
             'printf("TPE_JOINT_REPORT_CHUNK %d\\n", TPE_JOINT_REPORT_CHUNK);',
             'printf("TPE_REPORT_MAX_K %d\\n", TPE_REPORT_MAX_K);',
             'printf("tpe_joint_top_entry %zu\\ntpe_joint_report_args %zu\\ntpe_score_stats %zu\\n", '
             'sizeof(tpe_joint_top_entry), sizeof(tpe_joint_report_args), sizeof(tpe_score_stats));']
    for f in N.JOINT_TOP_ENTRY_DTYPE.names:
        lines.append('printf("tpe_joint_top_entry.%s %%zu\\n", offsetof(tpe_joint_top_entry, %s));' % (f, f))
    for f, _ in N.JointReportArgs._fields_:
        lines.append('printf("tpe_joint_report_args.%s %%zu\\n", offsetof(tpe_joint_report_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 's.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 's')
        subprocess.check_call(['gcc', '-Wall', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['TPE_JOINT_REPORT_CHUNK'] == N.JOINT_REPORT_CHUNK == 4096
    assert lay['TPE_REPORT_MAX_K'] == N.REPORT_MAX_K
    assert lay['tpe_joint_top_entry'] == N.JOINT_TOP_ENTRY_DTYPE.itemsize == 32
    assert lay['tpe_score_stats'] == N.SCORE_STATS_DTYPE.itemsize
    assert lay['tpe_joint_report_args'] == ctypes.sizeof(N.JointReportArgs)
    for f in N.JOINT_TOP_ENTRY_DTYPE.names:
        assert N.JOINT_TOP_ENTRY_DTYPE.fields[f][1] == lay['tpe_joint_top_entry.' + f], f
    for f, _ in N.JointReportArgs._fields_:
        assert getattr(N.JointReportArgs, f).offset == lay['tpe_joint_report_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_report_scratch_bytes', 'tpe_joint_report', 'tpe_joint_report_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ----------------------------------------------------- argument checks, no GPU
P_HOST, C_HOST, K_HOST = 3, 5000, 8


def _host_args(keep, widths=None, **over):
    """Complete arguments whose 'device' pointers are host arrays: only good for
    calls that return before any launch (_run passes too little scratch)."""
    buf = np.zeros(1 << 12)
    keep.append(buf)
    a = N.JointReportArgs()
    a.n_probs, a.n_cand, a.width, a.z_stride = P_HOST, C_HOST, 3, 16
    a.cand = a.l_out = a.g_out = buf.ctypes.data
    if widths is not None:
        w = np.array(widths, dtype=np.int32)
        keep.append(w)
        a.widths = a.host_widths = a.cand_off = w.ctypes.data
        a.n_probs = len(w)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _run(lib, a, keep, k=K_HOST, scratch_bytes=0, outs=(True,) * 4):
    buf = np.zeros(1 << 12)
    keep.append(buf)
    p = buf.ctypes.data
    top, z, nt, st = (p if o else None for o in outs)
    return lib.tpe_joint_report(ctypes.byref(a) if a is not None else None, k, top, z, nt, st,
                                p if scratch_bytes else None, scratch_bytes, None)


@pytest.mark.parametrize('over,msg', [
    (dict(n_probs=0), b'n_probs / n_cand < 1'), (dict(n_probs=-3), b'n_probs / n_cand < 1'),
    (dict(n_cand=0), b'n_probs / n_cand < 1'),
    (dict(cand=None), b'null cand'), (dict(l_out=None), b'null cand / l_out'), (dict(g_out=None), b'null cand / l_out / g_out'),
    (dict(width=0), b'width outside [1, 64]'), (dict(width=65, z_stride=65), b'width outside [1, 64]'),
    (dict(width=-1), b'width outside [1, 64]'),
    (dict(z_stride=2), b'z_stride below the largest width'), (dict(width=64, z_stride=63), b'z_stride below'),
    (dict(n_probs=1 << 30, n_cand=4097), b'too many chunks'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_bad_k_widths_outputs_and_scratch_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1 and b'null args' in lib.tpe_last_error()
    for k in (0, -1, N.REPORT_MAX_K + 1):
        assert _run(lib, _host_args(keep), keep, k=k) == -1 and b'k outside [1, TPE_REPORT_MAX_K]' in lib.tpe_last_error()
    for i in range(4):
        outs = tuple(j != i for j in range(4))
        assert _run(lib, _host_args(keep), keep, outs=outs) == -1 and b'null outputs' in lib.tpe_last_error()
    # per-problem widths: the host copy is what is checked
    a = _host_args(keep, widths=(2, 5, 16))
    a.host_widths = None
    assert _run(lib, a, keep) == -1 and b'widths without host_widths' in lib.tpe_last_error()
    for bad in ((2, 0, 16), (2, 65, 16), (-1, 5, 16)):
        assert _run(lib, _host_args(keep, widths=bad, z_stride=128), keep) == -1
        assert b'a width outside [1, 64]' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, widths=(2, 5, 16), z_stride=15), keep) == -1
    assert b'z_stride below the largest width' in lib.tpe_last_error()
    # with widths given, `width` is not read
    assert _run(lib, _host_args(keep, widths=(2, 5, 16), width=0), keep) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    # complete arguments get as far as the scratch check, the last one
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_report_scratch_bytes(P_HOST, C_HOST, K_HOST, ctypes.byref(need)) == 0
    assert need.value == P_HOST * 2 * (80 + 32 * K_HOST)
    assert _run(lib, _host_args(keep), keep) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, width=64, z_stride=64), keep, k=64) == -1
    assert b'scratch too small' in lib.tpe_last_error()


def test_scratch_bytes():
    lib = N.load()
    nb = ctypes.c_uint64(0)

    def size(P, C, k):
        assert lib.tpe_joint_report_scratch_bytes(P, C, k, ctypes.byref(nb)) == 0, (P, C, k)
        return nb.value
    for P, C, k, want in ((1, 1, 1, 112), (1, 4096, 8, 80 + 256), (1, 4097, 8, 2 * (80 + 256)),
                          (7, 3 * 4096 + 17, 64, 7 * 4 * (80 + 2048))):
        assert size(P, C, k) == want
    # monotone in each argument
    for lo, hi in (((1, 5000, 8), (2, 5000, 8)), ((3, 4096, 8), (3, 4097, 8)), ((3, 5000, 8), (3, 5000, 9)),
                   ((3, 1, 1), (3, 2 ** 31 - 1, 1))):
        assert size(*lo) < size(*hi)
    for C in range(1, 3 * 4096, 511):
        assert size(2, C, 8) <= size(2, C + 511, 8)
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, -5, 8), (1, 8, 0), (1, 8, N.REPORT_MAX_K + 1),
                (1 << 30, 4097, 8)):
        assert lib.tpe_joint_report_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_report_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_report_scratch_bytes(1, 8, 8, None) == -1


# --------------------------------------------------------------- the reference
def test_reference_semantics():
    nz = np.float32(-0.0)
    cand = np.array([[1, 2], [1, 2], [0, nz], [nz, 0], [np.nan, 1], [np.nan, 1], [1, 3], [1, 2]], dtype=np.float32)
    l = np.array([1.0, 5.0, 3.0, 4.0, 0.0, 0.0, np.nan, np.inf])
    g = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, np.inf])
    # NaN scores first (6, then 7: inf - inf), then 5.0 (1), 4.0 (3), 3.0 (2: the twin of 3), 1.0 (0: a copy of 1),
    # then the two NaN rows: each distinct from everything
    assert R.rank_order(l, g).tolist() == [6, 7, 1, 3, 2, 0, 4, 5]
    assert R.top_distinct_rows(cand, l, g, 8).tolist() == [6, 7, 3, 4, 5]
    assert R.top_distinct_rows(cand, l, g, 2).tolist() == [6, 7]
    assert R.n_distinct_rows(cand) == 5
    # equal rows need not have equal scores: the copy with the better score is the entry
    assert R.top_distinct_rows(cand[:2], [1.0, 2.0], [0.0, 0.0], 4).tolist() == [1]
    st = R.score_stats(l, g)
    assert (st['n_finite'], st['n_nan'], st['n_posinf'], st['n_neginf']) == (6, 2, 0, 0)
    assert st['min'] == 0.0 and st['max'] == 5.0 and abs(st['mean'] - 13.0 / 6) < 1e-15
    st = R.score_stats([np.inf, -np.inf], [0.0, 0.0])
    assert (st['n_finite'], st['n_posinf'], st['n_neginf'], st['m2']) == (0, 1, 1, 0.0) and np.isnan(st['mean'])


# ------------------------------------------------ the public call's errors, no GPU
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
    for name in ('tpe_joint_run', 'tpe_joint_seg_run', 'tpe_joint_report', 'tpe_run_batch', 'tpe_level_run',
                 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def _domain():
    from hyperopt_amd import base, hp
    return base.Domain(lambda d: 0.0, {
        'x': hp.uniform('x', -5, 5), 'y': hp.lognormal('y', 0, 1), 'c': hp.choice('c', [0, 1, 2]),
        'q': hp.quniform('q', 0, 10, 1),
        'clf': hp.choice('clf', [{'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
                                 {'depth': hp.uniform('rf_depth', 1, 20)}])})


def _trials(domain, n):
    from hyperopt_amd import base, rand
    trials = base.Trials()
    rs = np.random.RandomState(3)
    for tid in range(n):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return trials


@pytest.mark.parametrize('kw,match', [
    (dict(k=0), r'k must be in \[1, 64\]'), (dict(k=65), r'k must be in \[1, 64\]'), (dict(k=-1), 'k must be in'),
    (dict(joint=False), 'needs joint=True or joint='), (dict(joint=None), 'needs joint=True or joint='),
    (dict(joint=['x']), 'at least 2 labels'), (dict(joint=['x', 'nope']), "'nope' is not a label"),
    (dict(joint='x'), 'not the string'),
    (dict(joint=['x', 'c']), "label 'c' is not eligible"),
    (dict(joint=['x', 'q'], joint_discrete=True), "'q' is not eligible"),
    (dict(joint=['x', 'svm_C']), r"label 'svm_C' is not eligible \(loguniform, conditional\)"),
    (dict(joint=['x', 'y', 'svm_C'], joint_branches=True), "'svm_C' is the only label named under option 0"),
    (dict(joint=['svm_C', 'svm_gamma', 'x'], joint_branches=True), "'x' is the only unconditional label named"),
])
def test_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import history, tpe
    d = _domain()
    trials = _trials(d, 12)
    with pytest.raises(ValueError, match=match):
        tpe.joint_candidate_report(12, d, trials, 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.joint_candidate_report_columns(d.table, history.extract(d, trials), 12, 1, **kw)


def test_an_empty_history_raises(no_device):
    from hyperopt_amd import base, history, tpe
    d = _domain()
    with pytest.raises(ValueError, match='needs a history'):
        tpe.joint_candidate_report(0, d, base.Trials(), 1)
    with pytest.raises(ValueError, match='needs a history'):
        tpe.joint_candidate_report_columns(d.table, history.extract(d, base.Trials()), 0, 1, joint=True,
                                           joint_branches=True)
    with pytest.raises(ValueError, match='n_EI_candidates out of range'):
        tpe.joint_candidate_report(12, d, _trials(d, 12), 1, n_EI_candidates=0)


class _Recorder(object):
    """Stands in for the Engine: records the calls, answers with report arrays
    whose entry r of problem p is the row (p + r, p + r + 0.5, ...)."""

    def __init__(self):
        self.calls = []

    def _rep(self, P, k, widths):
        top = np.zeros((P, k), dtype=N.JOINT_TOP_ENTRY_DTYPE)
        top['idx'] = np.arange(k)[None, :] + 10
        top['l'], top['g'] = 2.0, 0.5
        z = [np.arange(w, dtype=np.float32)[None, :] * 0.5 + (p + np.arange(k, dtype=np.float32))[:, None]
             for p, w in enumerate(widths)]
        return top, z, np.full(P, k - 1, dtype=np.int32), np.zeros(P, dtype=N.SCORE_STATS_DTYPE)

    def run_joint(self, below, above, low, high, ids, n_cand, seed, **kw):
        self.calls.append(('run_joint', np.array(ids).tolist(), n_cand, seed, kw))
        top, z, nt, st = self._rep(1, kw['report_k'], [len(low)])
        return np.zeros(1, dtype=N.JOINT_RECORD_DTYPE), top, np.stack(z), nt, st

    def run_joint_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, **kw):
        self.calls.append(('run_joint_segments', models, list(stream_words), list(prob_seg), list(prob_id), n_cand,
                           seed, kw))
        return (np.zeros(len(prob_seg), dtype=N.JOINT_RECORD_DTYPE),) + self._rep(len(prob_seg), kw['report_k'],
                                                                                   [len(m.low) for m in models])


def test_groups_calls_and_records(monkeypatch):
    """The root group first, then every branch group as if active through ONE
    segmented call with the branch stream words and the one id; split into
    several calls where P x C exceeds REPORT_MAX_RUN_CANDIDATES."""
    from hyperopt_amd import base, history, hp, joint as J, tpe
    d = base.Domain(lambda d: 0.0, {
        'x': hp.uniform('x', -5, 5), 'y': hp.lognormal('y', 0, 1),
        'clf': hp.choice('clf', [{'C': hp.loguniform('svm_C', -3, 3), 'gamma': hp.loguniform('svm_gamma', -6, 0)},
                                 {'depth': hp.uniform('rf_depth', 1, 20), 'split': hp.uniform('rf_split', 0, 1),
                                  'w': hp.normal('rf_w', 0, 1)}])})
    t = d.table
    hist = history.extract(d, _trials(d, 30))
    rec = _Recorder()
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: rec)
    rep = tpe.joint_candidate_report_columns(t, hist, 30, 77, k=4, joint=True, joint_branches=True,
                                             n_EI_candidates=512)
    assert [c[0] for c in rec.calls] == ['run_joint', 'run_joint_segments']
    assert rec.calls[0][1:] == ([30], 512, 77, dict(report_k=4))
    _, models, words, prob_seg, prob_id, n_cand, seed, kw = rec.calls[1]
    assert [[r.label for r in m.rows] for m in models] == [['rf_depth', 'rf_split', 'rf_w'], ['svm_C', 'svm_gamma']]
    assert words == [J.branch_stream_word(m.rows) for m in models]
    assert prob_seg == [0, 1] and prob_id == [30, 30] and (n_cand, seed, kw) == (512, 77, dict(report_k=4))
    assert len(rep) == 3 and [g.labels for g in rep] == [['x', 'y'], ['rf_depth', 'rf_split', 'rf_w'],
                                                         ['svm_C', 'svm_gamma']]
    assert [g.condition for g in rep] == [None, ('clf', 1), ('clf', 0)]
    for p, g in zip((0, 0, 1), rep):
        assert g.n_top == 3 and g.vectors.shape == (3, len(g.labels)) and g.vectors.dtype == np.float64
        assert g.top.dtype == tpe.JOINT_REPORT_TOP_DTYPE and len(g.top) == 3
        assert g.top['index'].tolist() == [10, 11, 12] and (g.top['score'] == 1.5).all()
    # values(): exp for the log families (y; svm_C, svm_gamma), the coordinate itself else
    assert rep[0].vectors[:, 0].tolist() == [0.0, 1.0, 2.0]
    np.testing.assert_array_equal(rep[0].vectors[:, 1], np.exp(np.array([0.5, 1.5, 2.5])))
    np.testing.assert_array_equal(rep[2].vectors, np.exp(np.array([[1.0, 1.5], [2.0, 2.5], [3.0, 3.5]])))
    assert rep[1].vectors[1].tolist() == [1.0, 1.5, 2.0]
    dd = rep.dicts()
    assert dd[2]['condition'] == ('clf', 0) and dd[2]['labels'] == ['svm_C', 'svm_gamma']
    assert dd[0]['top'][1] == dict(vector=dict(x=1.0, y=float(np.exp(1.5))), l=2.0, g=0.5, score=1.5, index=11)
    assert set(dd[0]['stats']) == set(N.SCORE_STATS_DTYPE.names)

    rec.calls[:] = []
    monkeypatch.setattr(tpe, 'REPORT_MAX_RUN_CANDIDATES', 600)
    rep2 = tpe.joint_candidate_report_columns(t, hist, 30, 77, k=4, joint=True, joint_branches=True,
                                              n_EI_candidates=512)
    assert [c[0] for c in rec.calls] == ['run_joint', 'run_joint_segments', 'run_joint_segments']
    assert [c[3] for c in rec.calls[1:]] == [[0], [0]] and [g.labels for g in rep2] == [g.labels for g in rep]
    # only branch groups: no root stage
    rec.calls[:] = []
    rep3 = tpe.joint_candidate_report_columns(t, hist, 30, 77, k=4, joint=['svm_C', 'svm_gamma'], joint_branches=True)
    assert [c[0] for c in rec.calls] == ['run_joint_segments'] and [g.condition for g in rep3] == [('clf', 0)]
