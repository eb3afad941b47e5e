"""Discrete labels in wide joint groups (DESIGN.md "Discrete labels in wide
groups"), the parts that need no GPU: the layout of tpe_joint_wide_mixed_args,
the argument checks tpe_joint_wide_mixed_run makes before any launch and their
order, the public keyword ``joint_wide_mixed`` with its own argument checks, and
which Engine method a group of a given size and make-up reaches."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
E = b'tpe_joint_wide_mixed_run: '


# ------------------------------------------------------------------------ ABI
def test_wide_mixed_args_match_c():
    lines = ['printf("TPE_JOINT_WIDE_MAX_CAT %d\\nTPE_JOINT_WIDE_MAX_DIMS %d\\nTPE_JOINT_MAX_CAT_TOTAL %d\\n'
             'TPE_ABI_VERSION %d\\n", TPE_JOINT_WIDE_MAX_CAT, TPE_JOINT_WIDE_MAX_DIMS, TPE_JOINT_MAX_CAT_TOTAL, '
             'TPE_ABI_VERSION);',
             'printf("tpe_joint_wide_mixed_args %zu\\ntpe_joint_wide_args %zu\\n", sizeof(tpe_joint_wide_mixed_args), '
             'sizeof(tpe_joint_wide_args));']
    for f, _ in N.JointWideMixedArgs._fields_:
        lines.append('printf("tpe_joint_wide_mixed_args.%s %%zu\\n", offsetof(tpe_joint_wide_mixed_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'wm.c')
        with open(c, 'w') as f:
            f.write(prog)
        exe = os.path.join(d, 'wm')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_JOINT_WIDE_MAX_CAT'] == N.JOINT_WIDE_MAX_CAT == 8
    assert lay['TPE_JOINT_WIDE_MAX_DIMS'] == N.JOINT_WIDE_MAX_DIMS == 64
    assert lay['TPE_JOINT_MAX_CAT_TOTAL'] == N.JOINT_MAX_CAT_TOTAL == 1024
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_wide_mixed_args'] == ctypes.sizeof(N.JointWideMixedArgs)
    for f, _ in N.JointWideMixedArgs._fields_:
        assert getattr(N.JointWideMixedArgs, f).offset == lay['tpe_joint_wide_mixed_args.' + f], f
    # it starts with tpe_joint_wide_args, field for field, the 64 bounds included
    names = [f for f, _ in N.JointWideMixedArgs._fields_]
    wide = [f for f, _ in N.JointWideArgs._fields_]
    assert names[:len(wide)] == wide
    for f in wide:
        assert getattr(N.JointWideMixedArgs, f).offset == getattr(N.JointWideArgs, f).offset, f
    assert N.JointWideMixedArgs.n_cat.offset == lay['tpe_joint_wide_args'] == ctypes.sizeof(N.JointWideArgs)
    # then n_cat, cat_upper[8], cat_off[8], then the mixed stage's tables in its order
    assert names[len(wide):] == ['n_cat', 'cat_upper', 'cat_off'] + [f for f, _ in N.JointMixedArgs._fields_[-8:]]
    assert N.JointWideMixedArgs.cat_upper.size == N.JointWideMixedArgs.cat_off.size == 4 * 8


def test_library_exports_the_wide_mixed_symbols():
    lib = N.load()
    for name in ('tpe_joint_wide_mixed_scratch_bytes', 'tpe_joint_wide_mixed_run', 'tpe_joint_wide_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24
    assert 'tpe_joint_wide_mixed_run' not in N.JOINT_STAGES          # not a stage tpe_joint_run_shard takes


POINTERS = ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids',
            'below_cat', 'above_cat', 'below_miss', 'below_bonus', 'above_miss', 'above_bonus', 'below_h', 'cat_cum')


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointWideMixedArgs()
    a.n_dims, a.n_cat, a.n_cand, a.n_ids, a.flags = 18, 2, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in POINTERS:
        setattr(a, f, arr.ctypes.data)
    a.cat_upper[0], a.cat_upper[1] = 3, 5
    a.cat_off[0], a.cat_off[1] = 0, 3
    for k, v in over.items():
        if k in ('cat_upper', 'cat_off'):
            for d, x in enumerate(v):
                getattr(a, k)[d] = x
        else:
            setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, scratch_bytes=0):
    """tpe_joint_wide_mixed_run with NO usable scratch unless asked: the scratch
    check is the last one, so every earlier rejection is reached and a call that
    were wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_wide_mixed_run(ctypes.byref(a) if a is not None else None, p if records else None, None,
                                        None, None, p if scratch_bytes else None, scratch_bytes, None)


def test_null_wide_mixed_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert lib.tpe_last_error() == E + b'null args'


@pytest.mark.parametrize('over,msg', [
    # n_cat outside [0, 8]
    (dict(n_cat=-1), b'n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]'),
    (dict(n_cat=9), b'n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]'),
    # a width outside [1, 64]; no continuous label
    (dict(n_dims=0), b'n_dims < 1 or n_dims + n_cat outside [1, TPE_JOINT_WIDE_MAX_DIMS]'),
    (dict(n_dims=-1), b'n_dims < 1 or n_dims + n_cat outside'), (dict(n_dims=63), b'n_dims + n_cat outside'),
    (dict(n_dims=57, n_cat=8, cat_upper=[2] * 8, cat_off=list(range(0, 16, 2))), b'n_dims + n_cat outside'),
    (dict(n_dims=65, n_cat=1), b'n_dims + n_cat outside'),
    # everything tpe_joint_wide_run checks
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids / records'),
    # a null table
    (dict(below_cat=None), b'null category tables'), (dict(above_cat=None), b'null category tables'),
    (dict(below_miss=None), b'null category tables'), (dict(below_bonus=None), b'null category tables'),
    (dict(above_miss=None), b'null category tables'), (dict(above_bonus=None), b'null category tables'),
    (dict(below_h=None), b'null category tables'), (dict(cat_cum=None), b'null category tables'),
    # a U_d outside [2, 256]
    (dict(cat_upper=[1, 5]), b'categories of a label outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[3, 0]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[257, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[3, -4]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    # more than 1024 categories in all
    (dict(n_cat=5, cat_upper=[256, 256, 256, 256, 2], cat_off=[0, 256, 512, 768, 1024]),
     b'more than TPE_JOINT_MAX_CAT_TOTAL categories'),
    # offsets that leave the tables
    (dict(cat_off=[0, 4]), b'cat_off outside the tables'), (dict(cat_off=[-1, 3]), b'cat_off outside the tables'),
    # no scratch
    (dict(), b'scratch too small'),
])
def test_bad_wide_mixed_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    err = lib.tpe_last_error()
    assert err.startswith(E) and msg in err, err


@pytest.mark.parametrize('first,then', [
    # (an earlier fault, a later one): the earlier one is reported
    (dict(n_cat=9), dict(n_dims=70)), (dict(n_dims=63), dict(n_cand=0)), (dict(n_cand=0), dict(n_ids=0)),
    (dict(n_ids=0), dict(k_below=0)), (dict(k_below=0), dict(below_c=None)), (dict(below_c=None), dict(samp=None)),
    (dict(samp=None), dict(ids=None)), (dict(ids=None), dict(below_cat=None)),
    (dict(below_cat=None), dict(cat_upper=[1, 5])), (dict(cat_upper=[1, 5]), dict(cat_off=[0, 4])),
    (dict(n_cat=5, cat_upper=[256, 256, 256, 256, 2]), dict(cat_off=[-1, 3])),
])
def test_the_order_of_the_checks(first, then):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **first), keep) == -1
    want = lib.tpe_last_error()
    both = dict(then)
    both.update(first)
    assert _run(lib, _host_args(keep, **both), keep) == -1
    assert lib.tpe_last_error() == want
    assert _run(lib, _host_args(keep, **then), keep) == -1
    assert lib.tpe_last_error() != want                     # (the later fault is one of its own)
    # the scratch check is the last: any fault beats it
    assert b'scratch too small' not in want


@pytest.mark.parametrize('Dc,Dk', [(1, 1), (8, 4), (15, 1), (16, 1), (9, 8), (18, 2), (32, 8), (33, 1), (56, 8),
                                   (63, 1)])
def test_accepted_wide_mixed_arguments_reach_the_scratch_check(Dc, Dk):
    lib, keep = N.load(), []
    over = dict(n_dims=Dc, n_cat=Dk, cat_upper=[2] * Dk, cat_off=list(range(0, 2 * Dk, 2)))
    assert _run(lib, _host_args(keep, **over), keep, records=False) == -1
    assert lib.tpe_last_error() == E + b'null ids / records'
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_wide_mixed_scratch_bytes(1, 2048, Dc, Dk, ctypes.byref(need)) == 0
    # at least a record per 512 candidates and the f32 candidate block over all coordinates
    assert need.value >= 4 * 2048 * (Dc + Dk) + 4 * N.JOINT_WIDE_RECORD_DTYPE.itemsize
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert lib.tpe_last_error() == E + b'scratch too small'
    assert _run(lib, _host_args(keep, **over), keep, scratch_bytes=need.value - 1) == -1
    assert lib.tpe_last_error() == E + b'scratch too small'
    # the 1024-category limit itself is accepted
    if Dk == 4:
        over.update(cat_upper=[256] * 4, cat_off=[0, 256, 512, 768])
        assert _run(lib, _host_args(keep, **over), keep) == -1
        assert lib.tpe_last_error() == E + b'scratch too small'


def test_scratch_bytes_arguments():
    lib = N.load()
    nb, wide = ctypes.c_uint64(0), ctypes.c_uint64(0)
    last = 0
    for Dc, Dk in ((1, 1), (16, 1), (18, 2), (30, 2), (33, 1), (56, 8)):          # grows with the width
        assert lib.tpe_joint_wide_mixed_scratch_bytes(3, 4097, Dc, Dk, ctypes.byref(nb)) == 0
        assert nb.value > last
        last = nb.value
        # the wide stage's records plus a candidate block that is Dk coordinates wider
        assert lib.tpe_joint_wide_scratch_bytes(3, 4097, Dc, ctypes.byref(wide)) == 0
        assert nb.value == wide.value + 3 * 17 * 256 * Dk * 4
    # n_cat = 0: the wide stage's size
    assert lib.tpe_joint_wide_mixed_scratch_bytes(3, 4097, 20, 0, ctypes.byref(nb)) == 0
    assert lib.tpe_joint_wide_scratch_bytes(3, 4097, 20, ctypes.byref(wide)) == 0
    assert nb.value == wide.value
    for bad in ((0, 8, 20, 1), (1, 0, 20, 1), (1, 8, 0, 1), (1, 8, -1, 1), (1, 8, 20, -1), (1, 8, 20, 9),
                (1, 8, 63, 2), (1, 8, 64, 1), (1, 8, 65, 0)):
        assert lib.tpe_joint_wide_mixed_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_wide_mixed_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_wide_mixed_scratch_bytes(1, 8, 20, 1, None) == -1


def test_no_discrete_label_reaches_the_wide_stage():
    """n_cat = 0 is tpe_joint_wide_run on the shared fields: its checks and its
    messages (the category tables are not looked at)."""
    lib, keep = N.load(), []
    none = dict((f, None) for f in POINTERS[9:])
    assert _run(lib, _host_args(keep, n_cat=0, **none), keep) == -1
    assert lib.tpe_last_error() == b'tpe_joint_wide_run: scratch too small'
    assert _run(lib, _host_args(keep, n_cat=0, below_mu=None), keep) == -1
    assert lib.tpe_last_error() == b'tpe_joint_wide_run: null density rows'
    assert _run(lib, _host_args(keep, n_cat=0, n_dims=65), keep) == -1
    assert lib.tpe_last_error() == b'tpe_joint_wide_run: n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]'
    assert _run(lib, _host_args(keep, n_cat=0, n_dims=64), keep) == -1
    assert lib.tpe_last_error() == b'tpe_joint_wide_run: scratch too small'


def test_the_shard_entry_does_not_take_the_stage():
    lib, keep = N.load(), []
    sh = N.JointShard()
    sh.cand_base, sh.n_cand_global = 0, 2048
    buf = np.zeros(1 << 16, dtype=np.uint8)
    a = _host_args(keep)
    assert lib.tpe_joint_run_shard(6, ctypes.byref(a), ctypes.byref(sh), buf.ctypes.data, None, None, None, None, 0,
                                   None) == -1
    assert b'stage outside' in lib.tpe_last_error()
    assert sorted(N.JOINT_STAGES.values()) == list(range(6))


# ------------------------------------------------------- the public interface
def _net(n_cont, choices=(), extra=None):
    """n_cont labels of hp.uniform(-5, 5) and one hp.choice of U options per entry of ``choices``."""
    from hyperopt_amd import base, hp
    s = {'x%02d' % i: hp.uniform('x%02d' % i, -5, 5) for i in range(n_cont)}
    s.update({'c%02d' % i: hp.choice('c%02d' % i, list(range(u))) for i, u in enumerate(choices)})
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
    for name in ('tpe_joint_run', 'tpe_joint_wide_run', 'tpe_joint_mixed_run', 'tpe_joint_wide_mixed_run',
                 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def _both(domain, match, **kw):
    from hyperopt_amd import base, history, tpe
    with pytest.raises(ValueError, match=match) as e:
        tpe.suggest([0], domain, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0], 1, **kw)
    return str(e.value)


ALL = dict(joint=True, joint_wide=True, joint_discrete=True, joint_wide_mixed=True)


def test_the_keyword_needs_joint_wide_and_joint_discrete(no_device):
    d = _net(18, [3, 2])
    msg = _both(d, 'joint_wide_mixed=True needs joint_wide=True', joint=True, joint_discrete=True,
                joint_wide_mixed=True)
    assert 'it only widens' in msg
    msg = _both(d, 'joint_wide_mixed=True needs joint_discrete=True', joint=True, joint_wide=True,
                joint_wide_mixed=True)
    assert 'it only' in msg
    _both(d, 'joint_wide_mixed=True needs joint_wide=True', joint_wide_mixed=True)
    for joint in (False, None):
        _both(d, 'needs joint=True', joint=joint, joint_wide=True, joint_discrete=True, joint_wide_mixed=True)


def test_nine_discrete_labels_in_a_wide_group(no_device):
    d = _net(10, [2] * 9)
    msg = _both(d, r'TPE_JOINT_WIDE_MAX_CAT = 8.*joint=\[', **ALL)
    assert 'not 9' in msg and 'its 19' in msg
    _both(d, r'TPE_JOINT_WIDE_MAX_CAT = 8.*joint=\[', **dict(ALL, joint=[r.label for r in d.table.rows]))
    # eight are taken: no error before the history is read (an empty history: the random suggest)
    from hyperopt_amd import base, tpe
    assert len(tpe.suggest([0], _net(10, [2] * 8), base.Trials(), 1, **ALL)) == 1


def test_more_than_1024_categories_in_a_wide_group(no_device):
    d = _net(14, [256, 256, 256, 256, 2])
    msg = _both(d, r'TPE_JOINT_MAX_CAT_TOTAL = 1024.*joint=\[', **ALL)
    assert '1026' in msg and 'its 19' in msg


def test_sixty_five_labels_under_the_keyword(no_device):
    msg = _both(_net(63, [3, 2]), r'TPE_JOINT_WIDE_MAX_DIMS = 64.*joint=\[', **ALL)
    assert '65' in msg


def test_a_quantised_label_in_a_wide_group_under_the_keyword(no_device):
    from hyperopt_amd import hp
    d = _net(17, [3], {'q': hp.quniform('q', 0, 10, 1)})
    msg = _both(d, r'no quantised label.*joint=\[', joint_quantized=True, **ALL)
    assert '1 quantised' in msg and 'its 19' in msg
    # 16 labels in all: the quantised stage's own limits speak, as without the keyword
    _both(_net(14, [3], {'q': hp.quniform('q', 0, 10, 1)}), 'beside a quantised one', joint_quantized=True, **ALL)


def test_the_keyword_does_not_combine_with_joint_shard(no_device):
    for d in (_net(18, [3, 2]), _net(5, [3])):
        msg = _both(d, 'joint_wide_mixed=True does not combine with joint_shard', joint_shard=(0, 1), **ALL)
        assert 'not sharded' in msg


def test_without_the_keyword_the_error_is_unchanged(no_device):
    d = _net(18, [3, 2])
    msg = _both(d, 'continuous labels only', joint=True, joint_discrete=True, joint_wide=True)
    assert 'TPE_JOINT_MAX_DIMS = 16' in msg and 'not 2 discrete and 0 quantised ones among its 20' in msg
    assert 'joint=[' in msg
    _both(d, 'continuous labels only', joint=True, joint_discrete=True, joint_wide=True, joint_wide_mixed=False)
    _both(d, r'TPE_JOINT_MAX_DIMS = 16.*joint=\[', joint=True, joint_discrete=True)


@pytest.mark.parametrize('kw,match', [
    (dict(sampler='replay'), 'replay'), (dict(precision='fp64'), 'fp64'),
    (dict(shard=(0, 2)), 'shard'), (dict(shard_ids=(0, 2)), 'shard'),
    (dict(shard_labels=(0, 2)), 'shard'), (dict(shard_grid=(0, 2)), 'shard'),
])
def test_replay_fp64_and_shards_keep_raising(kw, match, no_device):
    _both(_net(18, [3, 2]), match, **dict(ALL, **kw))


def test_report_takes_the_keyword_and_its_errors(no_device):
    from hyperopt_amd import base, tpe
    with pytest.raises(ValueError, match='TPE_JOINT_WIDE_MAX_CAT = 8'):
        tpe.joint_candidate_report(0, _net(10, [2] * 9), base.Trials(), 1, **ALL)
    with pytest.raises(ValueError, match='joint_wide_mixed=True needs joint_wide=True'):
        tpe.joint_candidate_report(0, _net(18, [3]), base.Trials(), 1, joint=True, joint_discrete=True,
                                   joint_wide_mixed=True)
    with pytest.raises(ValueError, match='needs a history'):                    # the plan itself is accepted
        tpe.joint_candidate_report(0, _net(18, [3]), base.Trials(), 1, **ALL)


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
    and answers with candidate 0 at the origin (category 0)."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, dtype, below, above, low, high, *rest, **kw):
        cats = rest[0] if len(rest) == 4 else None
        ids, n_cand, seed = rest[-3:]
        self.calls.append((name, below, above, np.array(low), np.array(high), np.array(ids), n_cand, seed, kw, cats))
        return np.zeros(len(ids), dtype=dtype)

    def run_joint(self, *a, **kw):
        return self._answer('run_joint', N.JOINT_RECORD_DTYPE, *a, **kw)

    def run_joint_wide(self, *a, **kw):
        return self._answer('run_joint_wide', N.JOINT_WIDE_RECORD_DTYPE, *a, **kw)

    def run_joint_mixed(self, *a, **kw):
        return self._answer('run_joint_mixed', N.JOINT_RECORD_DTYPE, *a, **kw)

    def run_joint_wide_mixed(self, *a, **kw):
        return self._answer('run_joint_wide_mixed', N.JOINT_WIDE_RECORD_DTYPE, *a, **kw)


def _dispatch(monkeypatch, domain, **kw):
    from hyperopt_amd import history, tpe
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
    return hist, rec, out


def _same_cats(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert len(a) == len(b)
        for ca, cb in zip(a, b):
            assert len(ca) == len(cb) == 5
            for x, y in zip(ca, cb):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def _same_call(a, b):
    assert a[0] == b[0] and a[6:9] == b[6:9]
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_array_equal(x, y)
    for k in (3, 4, 5):
        np.testing.assert_array_equal(a[k], b[k])
    _same_cats(a[9], b[9])


@pytest.mark.parametrize('n_cont,choices,name', [(5, [], 'run_joint'), (14, [3, 2], 'run_joint_mixed'),
                                                 (16, [], 'run_joint'), (3, [2, 4], 'run_joint_mixed')])
def test_small_group_takes_the_stage_it_takes_today(monkeypatch, n_cont, choices, name):
    d = _net(n_cont, choices)
    _, plain, out0 = _dispatch(monkeypatch, d, joint=True, joint_discrete=True)
    _, both, out1 = _dispatch(monkeypatch, d, **ALL)
    assert [c[0] for c in plain.calls] == [c[0] for c in both.calls] == [name]
    _same_call(plain.calls[0], both.calls[0])
    assert out0 == out1


@pytest.mark.parametrize('n', [17, 20, 64])
def test_wide_continuous_group_takes_the_wide_stage(monkeypatch, n):
    d = _net(n)
    _, wide, out0 = _dispatch(monkeypatch, d, joint=True, joint_wide=True)
    _, both, out1 = _dispatch(monkeypatch, d, **ALL)
    assert [c[0] for c in wide.calls] == [c[0] for c in both.calls] == ['run_joint_wide']
    _same_call(wide.calls[0], both.calls[0])
    assert out0 == out1


@pytest.mark.parametrize('n_cont,choices', [(18, [3, 2]), (16, [3]), (56, [2] * 8)])
def test_wide_group_with_discrete_labels_takes_the_new_stage(monkeypatch, n_cont, choices):
    from hyperopt_amd import history, joint as J, tpe
    d = _net(n_cont, choices)
    hist, rec, out = _dispatch(monkeypatch, d, **ALL)
    assert [c[0] for c in rec.calls] == ['run_joint_wide_mixed']
    # kernel coordinates: the continuous labels in table order, then the discrete ones in table order
    crows = [r for r in d.table.rows if not r.categorical]
    drows = [r for r in d.table.rows if r.categorical]
    assert len(crows) == n_cont and len(drows) == len(choices)
    model = J.fit_mixed_model(crows, drows, hist, history.split_below(hist, tpe._default_gamma),
                              tpe._default_prior_weight, tpe.DEFAULT_LF)
    want = ('run_joint_wide_mixed', model.below[:3], model.above[:3], np.array(model.low), np.array(model.high),
            np.array([30, 31]), 512, 77, {}, model.cats())
    _same_call(rec.calls[0], want)
    assert rec.calls[0][1][1].shape[1] == n_cont and len(rec.calls[0][9]) == len(choices)
    assert [len(c[2]) for c in rec.calls[0][9]] == [int(r.args['upper']) for r in drows]
    # the record's z (all zero here) went through MixedModel.values into every label, typed as today
    assert len(out) == 2 and all(set(o) == set(d.table.labels) for o in out)
    for o in out:
        for r in crows:
            assert type(o[r.label]) is np.float64 and o[r.label] == 0.0
        for r in drows:
            assert type(o[r.label]) is np.int64 and o[r.label] == 0


def test_a_list_names_the_wide_mixed_group(monkeypatch):
    d = _net(20, [3, 2, 4])
    labels = ['x%02d' % i for i in range(17)] + ['c00', 'c02']
    _, rec, out = _dispatch(monkeypatch, d, **dict(ALL, joint=labels))
    assert [c[0] for c in rec.calls] == ['run_joint_wide_mixed']
    assert rec.calls[0][1][1].shape[1] == 17 and [len(c[2]) for c in rec.calls[0][9]] == [3, 4]


# ------------------------------------------------------------------- packing
def test_wide_mixed_rows_are_the_mixed_rows():
    from hyperopt_amd import joint_pack as JP
    from tests import joint_mixed_ref as M
    below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(9, [2, '5p', 4], 60)
    cats = M.cats_of(below, above, ps, sb, sa)
    a = JP.group_rows(below[:3], above[:3], low, high, cats, entry='mixed')
    b = JP.group_rows(below[:3], above[:3], low, high, cats, entry='wide_mixed')
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k
    assert [row[0] for row in JP.group_rows_present(a)] == [row[0] for row in JP.group_rows_present(b)]


def test_wide_mixed_pack_limits():
    from hyperopt_amd import joint_pack as JP
    from tests import joint_mixed_ref as M

    def rows(Dc, us, **kw):
        below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, 20)
        return JP.group_rows(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), **kw)
    assert rows(56, [2] * 8, entry='wide_mixed')['Dk'] == 8
    assert rows(63, [5], entry='wide_mixed')['Dc'] == 63
    with pytest.raises(ValueError, match='1 to 8'):
        rows(10, [2] * 9, entry='wide_mixed')
    with pytest.raises(ValueError, match='65 dimensions, at most 64'):
        rows(63, [2, 2], entry='wide_mixed')
    below, above, low, high, _, _, _, _, _, _ = M.seeded_mixed_case(20, [2], 20)
    with pytest.raises(ValueError, match='1 to 8'):
        JP.group_rows(below[:3], above[:3], low, high, (), entry='wide_mixed')
    # the other entries keep their limits
    with pytest.raises(ValueError, match='17 dimensions, at most 16'):
        rows(16, [3], entry='mixed')


def test_engine_method_takes_no_shard():
    import inspect
    from hyperopt_amd.engine import Engine
    sig = inspect.signature(Engine.run_joint_wide_mixed)
    assert list(sig.parameters) == ['self', 'below', 'above', 'low', 'high', 'cats', 'ids', 'n_cand', 'seed',
                                    'inject', 'return_cand', 'want_lg', 'report_k', 'stream_word']
    assert Engine._JOINT_SOLO['wide_mixed'] == (N.JointWideMixedArgs, 'tpe_joint_wide_mixed_run')


# ------------------------------------------------------------------- startup
def test_startup_is_the_random_suggest(no_device):
    from hyperopt_amd import rand, tpe
    domain = _net(18, [3, 2])
    trials = _with_trials(domain, 5)
    want = rand.suggest([5, 6], domain, trials, 99)
    got = tpe.suggest([5, 6], domain, trials, 99, **ALL)
    assert [d['misc']['vals'] for d in got] == [d['misc']['vals'] for d in want]
    for a, b in zip(got, want):
        for k, v in a['misc']['vals'].items():
            assert [float(x).hex() for x in v] == [float(x).hex() for x in b['misc']['vals'][k]]
