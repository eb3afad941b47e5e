"""Wide joint groups (DESIGN.md "Wide groups"), the parts that need no GPU: the
layout of the two new structs, the argument checks tpe_joint_wide_run makes
before any launch, the public interface's argument checks, and which Engine
method a group of a given size reaches."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')


# ------------------------------------------------------------------------ ABI
def test_wide_structs_match_c():
    lines = ['printf("TPE_JOINT_MAX_DIMS %d\\nTPE_JOINT_WIDE_MAX_DIMS %d\\nTPE_ABI_VERSION %d\\n", '
             'TPE_JOINT_MAX_DIMS, TPE_JOINT_WIDE_MAX_DIMS, TPE_ABI_VERSION);',
             'printf("tpe_joint_wide_record %zu\\ntpe_joint_wide_args %zu\\n", sizeof(tpe_joint_wide_record), '
             'sizeof(tpe_joint_wide_args));']
    for f in N.JOINT_WIDE_RECORD_DTYPE.names:
        lines.append('printf("tpe_joint_wide_record.%s %%zu\\n", offsetof(tpe_joint_wide_record, %s));' % (f, f))
    for f, _ in N.JointWideArgs._fields_:
        lines.append('printf("tpe_joint_wide_args.%s %%zu\\n", offsetof(tpe_joint_wide_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'w.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'w')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_JOINT_MAX_DIMS'] == N.JOINT_MAX_DIMS == 16
    assert lay['TPE_JOINT_WIDE_MAX_DIMS'] == N.JOINT_WIDE_MAX_DIMS == 64
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_wide_record'] == N.JOINT_WIDE_RECORD_DTYPE.itemsize == 24 + 8 * 64
    assert lay['tpe_joint_wide_args'] == ctypes.sizeof(N.JointWideArgs)
    for f in N.JOINT_WIDE_RECORD_DTYPE.names:
        assert N.JOINT_WIDE_RECORD_DTYPE.fields[f][1] == lay['tpe_joint_wide_record.' + f], f
    for f, _ in N.JointWideArgs._fields_:
        assert getattr(N.JointWideArgs, f).offset == lay['tpe_joint_wide_args.' + f], f
    # the fields of tpe_joint_args, in its order; only the two bound arrays are longer
    assert [f for f, _ in N.JointWideArgs._fields_] == [f for f, _ in N.JointArgs._fields_]
    for f, _ in N.JointArgs._fields_[:-2]:
        assert getattr(N.JointWideArgs, f).offset == getattr(N.JointArgs, f).offset, f
    assert N.JointWideArgs.low.size == N.JointWideArgs.high.size == 8 * 64


def test_library_exports_the_wide_symbols():
    lib = N.load()
    for name in ('tpe_joint_wide_scratch_bytes', 'tpe_joint_wide_run', 'tpe_joint_wide_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointWideArgs()
    a.n_dims, a.n_cand, a.n_ids, a.flags = 20, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids'):
        setattr(a, f, arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, scratch_bytes=0):
    """tpe_joint_wide_run with NO usable scratch unless asked: the scratch check
    is the last one, so every earlier rejection is reached and a call that were
    wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_wide_run(ctypes.byref(a) if a is not None else None, p if records else None, None, None,
                                  None, p if scratch_bytes else None, scratch_bytes, None)


def test_null_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert b'tpe_joint_wide_run: null args' in lib.tpe_last_error()


@pytest.mark.parametrize('over,msg', [
    (dict(n_dims=0), b'n_dims outside'), (dict(n_dims=-1), b'n_dims outside'), (dict(n_dims=65), b'n_dims outside'),
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    err = lib.tpe_last_error()
    assert err.startswith(b'tpe_joint_wide_run') and msg in err, err


@pytest.mark.parametrize('D', [1, 16, 17, 20, 33, 64])
def test_null_records_and_small_scratch_are_rejected(D):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, n_dims=D), keep, records=False) == -1
    assert b'null ids / records' in lib.tpe_last_error()
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_wide_scratch_bytes(1, 2048, D, ctypes.byref(need)) == 0
    # at least a record per 512 candidates and the f32 candidate block
    assert need.value >= 4 * 2048 * D + 4 * N.JOINT_WIDE_RECORD_DTYPE.itemsize
    assert _run(lib, _host_args(keep, n_dims=D), keep) == -1                       # no scratch at all
    assert b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, n_dims=D), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()


def test_scratch_bytes_arguments():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    last = 0
    for D in (1, 20, 32, 33, 64):                                           # grows with the width
        assert lib.tpe_joint_wide_scratch_bytes(3, 4097, D, ctypes.byref(nb)) == 0
        assert nb.value > last
        last = nb.value
    for bad in ((0, 8, 20), (1, 0, 20), (1, 8, 0), (1, 8, -1), (1, 8, 65)):
        assert lib.tpe_joint_wide_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_wide_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_wide_scratch_bytes(1, 8, 20, None) == -1


def test_wide_profile_has_nothing_to_read_before_a_profiled_call():
    lib = N.load()
    ms = ctypes.c_double(0)
    assert lib.tpe_joint_wide_profile(ctypes.byref(ms)) == -1
    assert b'tpe_joint_wide_profile' in lib.tpe_last_error()
    assert lib.tpe_joint_wide_profile(None) == -1


# ------------------------------------------------------- the public interface
def _flat(n, extra=None):
    """n labels of hp.uniform(-5, 5) (bench.py config 4's space at n = 20)."""
    from hyperopt_amd import base, hp
    s = {'x%02d' % i: hp.uniform('x%02d' % i, -5, 5) for i in range(n)}
    s.update(extra or {})
    return base.Domain(lambda d: 0.0, s)


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
    for name in ('tpe_joint_run', 'tpe_joint_wide_run', 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def _both(domain, match, **kw):
    from hyperopt_amd import base, history, tpe
    with pytest.raises(ValueError, match=match) as e:
        tpe.suggest([0], domain, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0], 1, **kw)
    return str(e.value)


def test_joint_wide_needs_joint(no_device):
    for joint in (False, None):
        msg = _both(_flat(20), 'joint_wide=True needs joint', joint=joint, joint_wide=True)
        assert 'it only widens what joint joins' in msg


def test_more_than_sixty_four_labels(no_device):
    d = _flat(65)
    msg = _both(d, r'TPE_JOINT_WIDE_MAX_DIMS = 64.*joint=\[', joint=True, joint_wide=True)
    assert '65' in msg
    _both(d, r'TPE_JOINT_WIDE_MAX_DIMS = 64.*joint=\[', joint=[r.label for r in d.table.rows], joint_wide=True)
    # without the keyword: today's message
    _both(d, r'TPE_JOINT_MAX_DIMS = 16.*joint=\[', joint=True)
    _both(_flat(17), r'TPE_JOINT_MAX_DIMS = 16.*joint=\[', joint=True, joint_wide=False)


def test_wide_groups_are_continuous_only(no_device):
    from hyperopt_amd import base, hp
    choices = base.Domain(lambda d: 0.0, {'c%02d' % i: hp.choice('c%02d' % i, [0, 1, 2]) for i in range(17)})
    msg = _both(choices, 'continuous labels only', joint=True, joint_discrete=True, joint_wide=True)
    assert '17' in msg and 'joint=[' in msg
    _both(choices, 'continuous labels only', joint=[r.label for r in choices.table.rows], joint_discrete=True,
          joint_wide=True)
    quant = _flat(17, {'q': hp.quniform('q', 0, 10, 1)})
    msg = _both(quant, 'continuous labels only', joint=True, joint_quantized=True, joint_wide=True)
    assert '18' in msg and '1 quantised' in msg and 'joint=[' in msg
    # 16 labels in all: the quantised stage's own limits speak, as without the keyword
    _both(_flat(15, {'q': hp.quniform('q', 0, 10, 1)}), 'beside a quantised one', joint=True, joint_quantized=True,
          joint_wide=True)


@pytest.mark.parametrize('kw,match', [
    (dict(sampler='replay'), 'replay'), (dict(precision='fp64'), 'fp64'),
    (dict(shard=(0, 2)), 'shard'), (dict(shard_ids=(0, 2)), 'shard'),
    (dict(shard_labels=(0, 2)), 'shard'), (dict(shard_grid=(0, 2)), 'shard'),
])
@pytest.mark.parametrize('n', [5, 20])
def test_replay_fp64_and_shards_keep_raising(kw, match, n, no_device):
    _both(_flat(n), match, joint=True, joint_wide=True, **kw)


def test_ineligible_named_label_is_still_refused(no_device):
    from hyperopt_amd import hp
    d = _flat(20, {'q': hp.quniform('q', 0, 10, 1)})
    _both(d, "'q'", joint=[r.label for r in d.table.rows], joint_wide=True)


def _with_trials(domain, n):
    from hyperopt_amd import base, rand
    trials = base.Trials()
    rs = np.random.RandomState(4)
    for tid in range(n):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return trials


class _Recorder(object):
    """Stands in for the Engine in tpe._suggest_joint: records the joint call
    and answers with candidate 0 at the origin."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, dtype, below, above, low, high, ids, n_cand, seed, **kw):
        self.calls.append((name, below, above, np.array(low), np.array(high), np.array(ids), n_cand, seed, kw))
        return np.zeros(len(ids), dtype=dtype)

    def run_joint(self, *a, **kw):
        return self._answer('run_joint', N.JOINT_RECORD_DTYPE, *a, **kw)

    def run_joint_wide(self, *a, **kw):
        return self._answer('run_joint_wide', N.JOINT_WIDE_RECORD_DTYPE, *a, **kw)


def _dispatch(monkeypatch, n, **kw):
    from hyperopt_amd import history, tpe
    domain = _flat(n)
    trials = _with_trials(domain, 30)
    hist = history.extract(domain, trials)
    rec = _Recorder()
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: rec)
    # the univariate part needs a device: every label inactive, and the joint stage fills its group
    L = len(domain.table.rows)

    def local(table, hist, new_ids, *a, **k):
        return tpe.ChoiceColumns(table.labels, np.full((len(new_ids), L), np.nan), np.zeros((len(new_ids), L), bool))
    monkeypatch.setattr(tpe, '_suggest_local', local)
    out = tpe.suggest_choices(domain.table, hist, [30, 31], 77, n_EI_candidates=512, **kw)
    return domain, hist, rec, out


def _same_call(a, b):
    assert a[0] == b[0] and a[6:] == b[6:]
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_array_equal(x, y)
    for k in (3, 4, 5):
        np.testing.assert_array_equal(a[k], b[k])


def test_small_group_takes_the_existing_stage(monkeypatch):
    _, _, plain, out0 = _dispatch(monkeypatch, 5, joint=True)
    _, _, wide, out1 = _dispatch(monkeypatch, 5, joint=True, joint_wide=True)
    assert [c[0] for c in plain.calls] == [c[0] for c in wide.calls] == ['run_joint']
    _same_call(plain.calls[0], wide.calls[0])
    assert out0 == out1
    _, _, sixteen, _ = _dispatch(monkeypatch, 16, joint=True, joint_wide=True)
    assert [c[0] for c in sixteen.calls] == ['run_joint']


@pytest.mark.parametrize('n', [17, 20, 64])
def test_wide_group_takes_the_wide_stage(monkeypatch, n):
    from hyperopt_amd import history, joint as J, tpe
    domain, hist, rec, out = _dispatch(monkeypatch, n, joint=True, joint_wide=True)
    assert [c[0] for c in rec.calls] == ['run_joint_wide']
    group = [r for r in domain.table.rows]
    model = J.fit_model(group, hist, history.split_below(hist, tpe._default_gamma), tpe._default_prior_weight,
                        tpe.DEFAULT_LF)
    want = ('run_joint_wide', model.below, model.above, np.array(model.low), np.array(model.high),
            np.array([30, 31]), 512, 77, {})
    _same_call(rec.calls[0], want)
    assert rec.calls[0][1][1].shape[1] == n
    # the record's z (all zero here) went through JointModel.values into every label
    assert len(out) == 2 and all(set(o) == set(domain.table.labels) for o in out)
    assert all(type(v) is np.float64 and v == 0.0 for o in out for v in o.values())


def test_startup_is_the_random_suggest(no_device):
    from hyperopt_amd import rand, tpe
    domain = _flat(20)
    trials = _with_trials(domain, 5)
    want = rand.suggest([5, 6], domain, trials, 99)
    got = tpe.suggest([5, 6], domain, trials, 99, joint=True, joint_wide=True)
    assert [d['misc']['vals'] for d in got] == [d['misc']['vals'] for d in want]
    for a, b in zip(got, want):
        for k, v in a['misc']['vals'].items():
            assert [float(x).hex() for x in v] == [float(x).hex() for x in b['misc']['vals'][k]]
