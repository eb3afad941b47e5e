"""Quantised labels in wide joint groups (DESIGN.md "Quantised labels in wide
groups"), the parts that need no GPU: the layout of tpe_joint_wide_quant_args,
the argument checks tpe_joint_wide_quant_run makes before any launch, its
scratch size, the public keyword ``joint_wide_quantized`` with its own argument
checks, which Engine method a group of a given make-up reaches, the packer's
'wide_quant' entry, and the numpy restatement of the density against joint.py."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_wide_quant_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
E = b'tpe_joint_wide_quant_run: '


# ------------------------------------------------------------------------ ABI
def test_wide_quant_args_match_c():
    lines = ['printf("TPE_ABI_VERSION %d\\n", TPE_ABI_VERSION);',
             'printf("tpe_joint_wide_quant_args %zu\\ntpe_joint_wide_mixed_args %zu\\n", '
             'sizeof(tpe_joint_wide_quant_args), sizeof(tpe_joint_wide_mixed_args));']
    for f, _ in N.JointWideQuantArgs._fields_:
        lines.append('printf("a.%s %%zu\\n", offsetof(tpe_joint_wide_quant_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'wq.c')
        with open(c, 'w') as f:
            f.write(prog)
        exe = os.path.join(d, 'wq')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_wide_quant_args'] == ctypes.sizeof(N.JointWideQuantArgs)
    for f, _ in N.JointWideQuantArgs._fields_:
        assert getattr(N.JointWideQuantArgs, f).offset == lay['a.' + f], f
    # the fields of tpe_joint_wide_mixed_args at the same offsets, then the quantised fields of tpe_joint_quant_args
    names = [f for f, _ in N.JointWideQuantArgs._fields_]
    mixed = [f for f, _ in N.JointWideMixedArgs._fields_]
    assert names[:len(mixed)] == mixed
    for f in mixed:
        assert getattr(N.JointWideQuantArgs, f).offset == getattr(N.JointWideMixedArgs, f).offset, f
    assert N.JointWideQuantArgs.n_quant.offset == lay['tpe_joint_wide_mixed_args'] == ctypes.sizeof(N.JointWideMixedArgs)
    tail = [f for f, _ in N.JointQuantArgs._fields_[len(N.JointMixedArgs._fields_):]]
    assert names[len(mixed):] == tail and tail[0] == 'n_quant' and tail[-1] == 'quant_table_bytes'
    for f in tail:
        assert (getattr(N.JointWideQuantArgs, f).offset - N.JointWideQuantArgs.n_quant.offset ==
                getattr(N.JointQuantArgs, f).offset - N.JointQuantArgs.n_quant.offset), f


def test_library_exports_the_wide_quant_symbols():
    lib = N.load()
    for name in ('tpe_joint_wide_quant_scratch_bytes', 'tpe_joint_wide_quant_run', 'tpe_joint_wide_quant_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24
    assert 'tpe_joint_wide_quant_run' not in N.JOINT_STAGES          # not a stage tpe_joint_run_shard takes
    ms = ctypes.c_double(0)
    assert lib.tpe_joint_wide_quant_profile(ctypes.byref(ms)) == -1   # nothing profiled
    assert lib.tpe_last_error().startswith(b'tpe_joint_wide_quant_profile: ')


POINTERS = ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids',
            'below_cat', 'above_cat', 'below_miss', 'below_bonus', 'above_miss', 'above_bonus', 'below_h', 'cat_cum',
            'quant_edges', 'below_qmu', 'below_qsigma', 'above_qmu', 'above_qsigma', 'quant_samp', 'quant_table')
ARRAYS = ('cat_upper', 'cat_off', 'quant_v', 'quant_edge_off')


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointWideQuantArgs()
    a.n_dims, a.n_cat, a.n_quant, a.n_cand, a.n_ids, a.flags = 17, 2, 2, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in POINTERS:
        setattr(a, f, arr.ctypes.data)
    a.cat_upper[0], a.cat_upper[1] = 3, 5
    a.cat_off[0], a.cat_off[1] = 0, 3
    a.quant_v[0], a.quant_v[1] = 11, 4
    a.quant_edge_off[0], a.quant_edge_off[1] = 0, 12
    a.n_edges = 17
    a.quant_table_bytes = (4 + 9) * 15 * 4
    for k, v in over.items():
        if k in ARRAYS:
            for d, x in enumerate(v):
                getattr(a, k)[d] = x
        else:
            setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, scratch_bytes=0):
    """tpe_joint_wide_quant_run with NO usable scratch unless asked: the scratch
    check is the last one, so every earlier rejection is reached and a call
    that were wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_wide_quant_run(ctypes.byref(a) if a is not None else None, p if records else None, None,
                                        None, None, p if scratch_bytes else None, scratch_bytes, None)


def test_null_wide_quant_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert lib.tpe_last_error() == E + b'null args'


@pytest.mark.parametrize('over,msg', [
    # the counts: n_quant in [1, 4] (0 is NOT another stage here), n_cat in [0, 8], at least one continuous label,
    # at most 64 coordinates
    (dict(n_quant=0), b'n_quant outside [1, TPE_JOINT_MAX_QUANT]'),
    (dict(n_quant=-1), b'n_quant outside [1, TPE_JOINT_MAX_QUANT]'),
    (dict(n_quant=5), b'n_quant outside [1, TPE_JOINT_MAX_QUANT]'),
    (dict(n_cat=-1), b'n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]'),
    (dict(n_cat=9), b'n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]'),
    (dict(n_dims=0), b'n_dims < 1 or n_dims + n_cat + n_quant outside [2, TPE_JOINT_WIDE_MAX_DIMS]'),
    (dict(n_dims=-3), b'n_dims < 1 or'), (dict(n_dims=61), b'n_dims + n_cat + n_quant outside'),
    (dict(n_dims=64, n_cat=0, n_quant=1), b'n_dims + n_cat + n_quant outside'),
    (dict(n_dims=70, n_cat=0, n_quant=1), b'n_dims + n_cat + n_quant outside'),
    # everything tpe_joint_wide_run checks
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids / records'),
    # the category tables, as tpe_joint_wide_mixed_run
    (dict(below_cat=None), b'null category tables'), (dict(above_cat=None), b'null category tables'),
    (dict(below_miss=None), b'null category tables'), (dict(below_bonus=None), b'null category tables'),
    (dict(above_miss=None), b'null category tables'), (dict(above_bonus=None), b'null category tables'),
    (dict(below_h=None), b'null category tables'), (dict(cat_cum=None), b'null category tables'),
    (dict(cat_upper=[1, 5]), b'categories of a label outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[257, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(n_cat=5, cat_upper=[256, 256, 256, 256, 2], cat_off=[0, 256, 512, 768, 1024]),
     b'more than TPE_JOINT_MAX_CAT_TOTAL categories'),
    (dict(cat_off=[0, 4]), b'cat_off outside the tables'), (dict(cat_off=[-1, 3]), b'cat_off outside the tables'),
    # the lattices, the quantised rows and the table, as tpe_joint_quant_run
    (dict(quant_v=[1, 4]), b'lattice values of a label outside [2, TPE_JOINT_MAX_LATTICE]'),
    (dict(quant_v=[11, 257]), b'outside [2, TPE_JOINT_MAX_LATTICE]'),
    (dict(n_quant=3, quant_v=[256, 256, 2], quant_edge_off=[0, 257, 514], n_edges=517),
     b'more than TPE_JOINT_MAX_LATTICE_TOTAL lattice values'),
    (dict(quant_edge_off=[-1, 12]), b'quant_edge_off outside the edge array'),
    (dict(quant_edge_off=[0, 13]), b'quant_edge_off outside the edge array'),
    (dict(n_edges=16), b'quant_edge_off outside the edge array'),
    (dict(quant_edges=None), b'null quantised rows or table'), (dict(below_qmu=None), b'null quantised rows or table'),
    (dict(below_qsigma=None), b'null quantised rows or table'), (dict(above_qmu=None), b'null quantised rows or table'),
    (dict(above_qsigma=None), b'null quantised rows or table'), (dict(quant_samp=None), b'null quantised rows or table'),
    (dict(quant_table=None), b'null quantised rows or table'),
    (dict(quant_table_bytes=(4 + 9) * 15 * 4 - 1), b'table workspace too small'),
    # no scratch
    (dict(), b'scratch too small'),
])
def test_bad_wide_quant_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    err = lib.tpe_last_error()
    assert err.startswith(E) and msg in err, err


def test_no_discrete_label_is_this_stage_and_takes_null_tables():
    lib, keep = N.load(), []
    none = dict((f, None) for f in POINTERS[9:17])
    assert _run(lib, _host_args(keep, n_cat=0, **none), keep) == -1
    assert lib.tpe_last_error() == E + b'scratch too small'


@pytest.mark.parametrize('Dc,Dk,Dq', [(1, 0, 1), (3, 0, 1), (9, 1, 1), (17, 0, 1), (20, 2, 2), (28, 8, 4), (44, 3, 1),
                                      (59, 1, 4), (63, 0, 1), (52, 8, 4)])
def test_accepted_arguments_reach_the_scratch_check_and_the_size_is_the_formula(Dc, Dk, Dq):
    lib, keep = N.load(), []
    over = dict(n_dims=Dc, n_cat=Dk, n_quant=Dq, cat_upper=[2] * Dk, cat_off=list(range(0, 2 * Dk, 2)),
                quant_v=[2] * Dq, quant_edge_off=list(range(0, 3 * Dq, 3)), n_edges=3 * Dq)
    assert _run(lib, _host_args(keep, **over), keep, records=False) == -1
    assert lib.tpe_last_error() == E + b'null ids / records'
    need = ctypes.c_uint64(0)
    for n_ids, C in ((1, 2048), (3, 4097), (2, 1), (1, 700)):
        assert lib.tpe_joint_wide_quant_scratch_bytes(n_ids, C, Dc, Dk, Dq, ctypes.byref(need)) == 0
        assert need.value == W.scratch_bytes(n_ids, C, Dc, Dk, Dq)
    assert lib.tpe_joint_wide_quant_scratch_bytes(1, 2048, Dc, Dk, Dq, ctypes.byref(need)) == 0
    if Dk:
        mixed = ctypes.c_uint64(0)                       # the wide mixed stage's, Dq coordinates wider
        assert lib.tpe_joint_wide_mixed_scratch_bytes(1, 2048, Dc, Dk, ctypes.byref(mixed)) == 0
        assert need.value == mixed.value + 8 * 256 * Dq * 4
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert lib.tpe_last_error() == E + b'scratch too small'
    assert _run(lib, _host_args(keep, **over), keep, scratch_bytes=need.value - 1) == -1
    assert lib.tpe_last_error() == E + b'scratch too small'


def test_scratch_bytes_arguments():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    for bad in ((0, 8, 20, 1, 1), (1, 0, 20, 1, 1), (1, 8, 0, 1, 1), (1, 8, 20, -1, 1), (1, 8, 20, 9, 1),
                (1, 8, 20, 1, 0), (1, 8, 20, 1, 5), (1, 8, 62, 2, 1), (1, 8, 64, 0, 1)):
        assert lib.tpe_joint_wide_quant_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_wide_quant_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_wide_quant_scratch_bytes(1, 8, 20, 1, 1, None) == -1


def test_the_shard_entry_does_not_take_the_stage():
    lib, keep = N.load(), []
    sh = N.JointShard()
    sh.cand_base, sh.n_cand_global = 0, 2048
    buf = np.zeros(1 << 16, dtype=np.uint8)
    a = _host_args(keep)
    for stage in (6, 7):
        assert lib.tpe_joint_run_shard(stage, ctypes.byref(a), ctypes.byref(sh), buf.ctypes.data, None, None, None,
                                       None, 0, None) == -1
        assert b'stage outside [0, 5]' in lib.tpe_last_error()
    assert sorted(N.JOINT_STAGES.values()) == list(range(6))


def test_the_tile_rule_keeps_a_workgroup_under_64_kib():
    for Dc in (1, 16, 17, 24, 32, 33, 48, 49, 63):
        dp = W.dp_of(Dc)
        tk = 128 if dp <= 32 else (4096 // dp) & ~7
        for total in (2, 11, 100, 202, 512):
            t = W.tile_of(Dc, total)
            assert 8 <= t <= tk and t % 8 == 0
            static = 4 * (tk * 2 * dp + tk * 8 + tk) + 64
            assert static + (total + 1) * (t + 4) * 4 <= 64 * 1024
    assert W.tile_of(20, 512) == 8 and W.tile_of(17, 2) == 128 and W.tile_of(44, 37) == 80 and W.tile_of(59, 16) == 64


# ------------------------------------------------------- the public interface
def _net(n_cont, choices=(), quants=(), extra=None):
    """n_cont labels of hp.uniform(-5, 5), one hp.choice of U options per entry
    of ``choices`` and one hp.quniform(0, V - 1, 1) per entry V of ``quants``."""
    from hyperopt_amd import base, hp
    s = {'x%02d' % i: hp.uniform('x%02d' % i, -5, 5) for i in range(n_cont)}
    s.update({'c%02d' % i: hp.choice('c%02d' % i, list(range(u))) for i, u in enumerate(choices)})
    s.update({'q%02d' % i: hp.quniform('q%02d' % i, 0, v - 1, 1) for i, v in enumerate(quants)})
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
                 'tpe_joint_quant_run', 'tpe_joint_wide_quant_run', 'tpe_run_batch', 'tpe_level_run',
                 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


@pytest.fixture
def no_startup(monkeypatch):
    """The startup draw fails the test: the argument errors come first."""
    from hyperopt_amd import rand

    def boom(*a, **kw):
        pytest.fail('the startup draw was made')
    monkeypatch.setattr(rand, 'suggest', boom)


def _both(domain, match, **kw):
    from hyperopt_amd import base, history, tpe
    with pytest.raises(ValueError, match=match) as e:
        tpe.suggest([0], domain, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0], 1, **kw)
    return str(e.value)


ALL = dict(joint=True, joint_wide=True, joint_discrete=True, joint_quantized=True, joint_wide_quantized=True)


def test_the_keyword_needs_joint_joint_wide_and_joint_quantized(no_device, no_startup):
    d = _net(20, [3], [11, 4])
    msg = _both(d, 'joint_wide_quantized=True needs joint_wide=True', joint=True, joint_quantized=True,
                joint_wide_quantized=True)
    assert 'it only widens' in msg
    msg = _both(d, 'joint_wide_quantized=True needs joint_quantized=True', joint=True, joint_wide=True,
                joint_wide_quantized=True)
    assert 'it only admits' in msg
    _both(d, 'joint_wide_quantized=True needs joint_wide=True', joint_wide_quantized=True)
    for joint in (False, None):
        _both(d, 'joint_wide_quantized=True needs joint=True', joint=joint, joint_wide=True, joint_quantized=True,
              joint_wide_quantized=True)


def test_without_the_keyword_the_two_errors_are_unchanged(no_device, no_startup):
    d = _net(20, [3], [11, 4])
    msg = _both(d, 'continuous labels only', joint=True, joint_discrete=True, joint_quantized=True, joint_wide=True)
    assert 'not 1 discrete and 2 quantised ones among its 23' in msg and 'joint=[' in msg
    msg = _both(d, r'no quantised label.*joint=\[', joint=True, joint_discrete=True, joint_quantized=True,
                joint_wide=True, joint_wide_mixed=True)
    assert '2 quantised' in msg
    _both(d, 'continuous labels only', joint=True, joint_discrete=True, joint_quantized=True, joint_wide=True,
          joint_wide_quantized=False)
    # 13 labels: 12 continuous ones and one quniform
    msg = _both(_net(12, [], [11]), 'at most 8 continuous labels beside a quantised one', joint=True,
                joint_quantized=True)
    assert 'not 12' in msg
    _both(_net(12, [], [11]), 'at most 8 continuous labels beside a quantised one', joint=True, joint_quantized=True,
          joint_wide=True)
    _both(_net(3, [2] * 5, [11]), 'at most 4 discrete labels beside a quantised one', joint=True, joint_discrete=True,
          joint_quantized=True, joint_wide=True)


@pytest.mark.parametrize('make,match,parts', [
    (lambda: _net(62, [3], [4, 4]), r'TPE_JOINT_WIDE_MAX_DIMS = 64.*joint=\[', ('not 65', 'its 65')),
    (lambda: _net(0, [2] * 5, [4, 4]), r'at least 1 continuous label.*joint=\[', ('not 0', 'its 7')),
    (lambda: _net(14, [], [4] * 5), r'TPE_JOINT_MAX_QUANT = 4.*joint=\[', ('not 5', 'its 19')),
    (lambda: _net(14, [], [256, 256, 2]), r'TPE_JOINT_MAX_LATTICE_TOTAL = 512.*joint=\[', ('not 514', 'its 17')),
    (lambda: _net(10, [2] * 9, [4]), r'TPE_JOINT_WIDE_MAX_CAT = 8.*joint=\[', ('not 9', 'its 20')),
    (lambda: _net(10, [256, 256, 256, 256, 2], [4]), r'TPE_JOINT_MAX_CAT_TOTAL = 1024.*joint=\[',
     ('not 1026', 'its 16')),
])
def test_a_group_over_a_limit_of_the_new_stage(no_device, no_startup, make, match, parts):
    d = make()
    msg = _both(d, match, **ALL)
    assert msg.startswith('joint with joint_wide_quantized=True') and all(p in msg for p in parts), msg
    _both(d, match, **dict(ALL, joint=[r.label for r in d.table.rows]))


def test_the_limits_themselves_are_taken(no_device):
    from hyperopt_amd import base, tpe
    # an empty history: the plan is accepted and the random suggest answers
    for d in (_net(52, [2] * 8, [2] * 4), _net(1, [2] * 5, [256, 256]), _net(9, [256] * 4, [11]), _net(12, [], [11])):
        assert len(tpe.suggest([0], d, base.Trials(), 1, **ALL)) == 1


def test_the_keyword_does_not_combine_with_joint_shard(no_device, no_startup):
    for d in (_net(20, [3], [11, 4]), _net(5, [3], [4]), _net(5)):
        msg = _both(d, 'joint_wide_quantized=True does not combine with joint_shard', joint_shard=(0, 1), **ALL)
        assert 'not sharded' in msg


@pytest.mark.parametrize('liar', [True, 'mixed', 'branches', 'branches_mixed'])
def test_no_joint_liar_where_the_group_takes_the_new_stage(no_device, no_startup, liar):
    kw = dict(ALL, joint_liar=liar, joint_branches=liar in ('branches', 'branches_mixed'))
    for d in (_net(20, [3], [11, 4]), _net(12, [], [11]), _net(3, [2] * 5, [11])):
        if liar is True:
            _both(d, 'joint_liar=True needs a root group of continuous labels only', **kw)
        else:
            msg = _both(d, 'does not combine with a root group that takes the wide quantised stage', **kw)
            assert 'joint_liar=%r' % liar in msg


def test_joint_liar_stays_where_the_narrow_stage_takes_the_group(no_device):
    from hyperopt_amd import base, tpe
    assert len(tpe.suggest([0], _net(5, [3], [4]), base.Trials(), 1, **dict(ALL, joint_liar='mixed'))) == 1


@pytest.mark.parametrize('kw,match', [
    (dict(sampler='replay'), 'replay'), (dict(precision='fp64'), 'fp64'),
    (dict(shard=(0, 2)), 'shard'), (dict(shard_ids=(0, 2)), 'shard'),
    (dict(shard_labels=(0, 2)), 'shard'), (dict(shard_grid=(0, 2)), 'shard'),
])
def test_replay_fp64_and_shards_keep_raising(kw, match, no_device, no_startup):
    _both(_net(20, [3], [11, 4]), match, **dict(ALL, **kw))


def test_report_takes_the_keyword_and_its_errors(no_device):
    from hyperopt_amd import base, history, tpe
    d = _net(10, [2] * 9, [4])
    with pytest.raises(ValueError, match='TPE_JOINT_WIDE_MAX_CAT = 8'):
        tpe.joint_candidate_report(0, d, base.Trials(), 1, **ALL)
    with pytest.raises(ValueError, match='TPE_JOINT_WIDE_MAX_CAT = 8'):
        tpe.joint_candidate_report_columns(d.table, history.extract(d, base.Trials()), 0, 1, **ALL)
    d = _net(20, [3], [11, 4])
    with pytest.raises(ValueError, match='joint_wide_quantized=True needs joint_wide=True'):
        tpe.joint_candidate_report(0, d, base.Trials(), 1, joint=True, joint_quantized=True, joint_wide_quantized=True)
    with pytest.raises(ValueError, match='needs a history'):                    # the plan itself is accepted
        tpe.joint_candidate_report(0, d, base.Trials(), 1, **ALL)
    for fn in (tpe.joint_candidate_report, tpe.joint_candidate_report_columns):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ['joint_wide_mixed', 'joint_wide_quantized'] and 'joint_liar' not in names


def test_the_signatures():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import Engine
    for fn in (tpe.suggest, tpe.suggest_choices):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ['joint_wide_mixed', 'joint_wide_quantized', 'joint_liar']
        assert p['joint_wide_quantized'].default is False
    assert list(inspect.signature(tpe._joint_plan).parameters) == [
        'table', 'joint', 'sampler', 'precision', 'shards', 'discrete', 'quantized', 'wide', 'branches',
        'branch_mixed']
    p = inspect.signature(tpe._wide_mode).parameters
    assert list(p)[:2] == ['joint_wide', 'joint_wide_mixed'] and all(
        v.default is not inspect.Parameter.empty for v in list(p.values())[2:])
    assert tpe._wide_mode(True, False) is True and tpe._wide_mode(False, False) is False
    assert tpe._wide_mode(True, True) == tpe.WIDE_MIXED
    assert tpe._wide_mode(True, False, True) == tpe.WIDE_QUANT
    assert tpe._wide_mode(True, True, True) not in (True, tpe.WIDE_MIXED, tpe.WIDE_QUANT)
    assert list(inspect.signature(Engine.run_joint_wide_quant).parameters) == [
        'self', 'below', 'above', 'low', 'high', 'cats', 'quants', 'ids', 'n_cand', 'seed', 'inject', 'return_cand',
        'want_lg', 'return_table', 'report_k', 'stream_word']
    assert Engine._JOINT_SOLO['wide_quant'] == (N.JointWideQuantArgs, 'tpe_joint_wide_quant_run')


def test_the_plan_s_group_and_kernel_order(no_device):
    from hyperopt_amd import base, hp, tpe
    s = {'b': hp.quniform('b', 0, 10, 1), 'a': hp.choice('a', [0, 1, 2]), 'z': hp.uniform('z', 0, 1),
         'l': hp.qloguniform('l', np.log(16.0), np.log(512.0), 16)}
    s.update({'x%02d' % i: hp.loguniform('x%02d' % i, -3, 1) for i in range(20)})
    s['gate'] = hp.choice('gate', [{'u': hp.uniform('u', 0, 1)}, {'w': hp.uniform('w', 0, 1)}])
    d = base.Domain(lambda c: 0.0, s)
    wide = tpe._wide_mode(True, False, True)
    group, branches = tpe._joint_plan(d.table, True, 'philox', 'fp32', (None,) * 4, True, True, wide)
    assert branches == []
    want = [r.label for r in d.table.rows if r.label not in ('gate', 'u', 'w')]
    assert [r.label for r in group] == want and len(group) == 24          # table order
    assert tpe._takes_wide_quant(group)
    crows, drows, qrows = tpe._joint_kernel_order(group)
    assert [r.label for r in drows] == ['a'] and [r.label for r in qrows] == ['b', 'l']
    assert [r.label for r in crows] == [r.label for r in group if r.label not in ('a', 'b', 'l')]
    # a list names the group; the branch groups are untouched by the keyword
    named, _ = tpe._joint_plan(d.table, ['x%02d' % i for i in range(12)] + ['l'], 'philox', 'fp32', (None,) * 4, False,
                               True, wide)
    assert len(named) == 13 and tpe._takes_wide_quant(named)
    g2, br = tpe._joint_plan(d.table, True, 'philox', 'fp32', (None,) * 4, True, True, wide, True)
    assert [r.label for r in g2] == want and br == []                   # (one label a branch: no branch group)


# --------------------------------------------------- which stage a group takes
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
    and answers with candidate 0 at the origin (category 0, lattice index 0)."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, dtype, n_extra, below, above, low, high, *rest, **kw):
        extra = rest[:n_extra]
        ids, n_cand, seed = rest[n_extra:n_extra + 3]
        assert len(rest) == n_extra + 3
        self.calls.append((name, below, above, np.array(low), np.array(high), np.array(ids), n_cand, seed, kw, extra))
        return np.zeros(len(ids), dtype=dtype)

    def run_joint(self, *a, **kw):
        return self._answer('run_joint', N.JOINT_RECORD_DTYPE, 0, *a, **kw)

    def run_joint_wide(self, *a, **kw):
        return self._answer('run_joint_wide', N.JOINT_WIDE_RECORD_DTYPE, 0, *a, **kw)

    def run_joint_mixed(self, *a, **kw):
        return self._answer('run_joint_mixed', N.JOINT_RECORD_DTYPE, 1, *a, **kw)

    def run_joint_wide_mixed(self, *a, **kw):
        return self._answer('run_joint_wide_mixed', N.JOINT_WIDE_RECORD_DTYPE, 1, *a, **kw)

    def run_joint_quant(self, *a, **kw):
        return self._answer('run_joint_quant', N.JOINT_RECORD_DTYPE, 2, *a, **kw)

    def run_joint_wide_quant(self, *a, **kw):
        return self._answer('run_joint_wide_quant', N.JOINT_WIDE_RECORD_DTYPE, 2, *a, **kw)


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


def _same_parts(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb)
        for ta, tb in zip(pa, pb):
            assert len(ta) == len(tb)
            for x, y in zip(ta, tb):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def _same_call(a, b):
    assert a[0] == b[0] and a[6:9] == b[6:9]
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_array_equal(x, y)
    for k in (3, 4, 5):
        np.testing.assert_array_equal(a[k], b[k])
    _same_parts(a[9], b[9])


@pytest.mark.parametrize('n_cont,choices,quants,name,without', [
    # the narrow quantised stage's limits themselves: 8 continuous, 4 discrete, 16 in all
    (8, [3, 2, 2, 4], [11, 4, 2, 5], 'run_joint_quant', dict()),
    (3, [], [11], 'run_joint_quant', dict()),
    # no quantised label
    (18, [3, 2], [], 'run_joint_wide_mixed', dict(joint_wide_mixed=True)),
    (20, [], [], 'run_joint_wide', dict()),
    (5, [3], [], 'run_joint_mixed', dict()),
    (5, [], [], 'run_joint', dict()),
])
def test_the_fallbacks_take_the_stage_they_take_today(monkeypatch, n_cont, choices, quants, name, without):
    d = _net(n_cont, choices, quants)
    base_kw = dict(joint=True, joint_wide=True, joint_discrete=True, joint_quantized=True, **without)
    _, plain, out0 = _dispatch(monkeypatch, d, **base_kw)
    _, both, out1 = _dispatch(monkeypatch, d, joint_wide_quantized=True, **base_kw)
    assert [c[0] for c in plain.calls] == [c[0] for c in both.calls] == [name]
    _same_call(plain.calls[0], both.calls[0])
    assert out0 == out1


@pytest.mark.parametrize('n_cont,choices,quants', [(20, [3], [11, 4]), (12, [], [11]), (9, [2], [11]),
                                                   (3, [2] * 5, [4]), (52, [2] * 8, [2] * 4)])
def test_a_group_past_the_narrow_limits_takes_the_new_stage(monkeypatch, n_cont, choices, quants):
    from hyperopt_amd import history, joint as J, tpe
    d = _net(n_cont, choices, quants)
    hist, rec, out = _dispatch(monkeypatch, d, **ALL)
    assert [c[0] for c in rec.calls] == ['run_joint_wide_quant']
    crows = [r for r in d.table.rows if r.dist == 'uniform']
    drows = [r for r in d.table.rows if r.categorical]
    qrows = [r for r in d.table.rows if r.dist == 'quniform']
    assert (len(crows), len(drows), len(qrows)) == (n_cont, len(choices), len(quants))
    model = J.fit_quant_model(crows, drows, qrows, hist, history.split_below(hist, tpe._default_gamma),
                              tpe._default_prior_weight, tpe.DEFAULT_LF)
    want = ('run_joint_wide_quant', model.below[:3], model.above[:3], np.array(model.low), np.array(model.high),
            np.array([30, 31]), 512, 77, {}, (model.cats(), model.quants()))
    _same_call(rec.calls[0], want)
    assert [len(q[4]) - 1 for q in rec.calls[0][9][1]] == list(quants)
    # the record's z (all zero) went through QuantModel.values into every label, typed as today
    assert len(out) == 2 and all(set(o) == set(d.table.labels) for o in out)
    for o in out:
        for r in crows + qrows:
            assert type(o[r.label]) is np.float64 and o[r.label] == 0.0
        for r in drows:
            assert type(o[r.label]) is np.int64 and o[r.label] == 0


# ------------------------------------------------------------------- packing
def _assert_same(a, b, keys):
    for k in keys:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


QUANT_KEYS = ('below_qmu', 'below_qsigma', 'above_qmu', 'above_qsigma', 'quant_edges', 'quant_samp', 'quant_v',
              'quant_edge_off', 'n_lattice', 'qlow', 'qhigh')


def test_wide_quant_rows_are_the_quant_rows_and_the_wide_mixed_rows():
    from hyperopt_amd import joint_pack as JP
    # a shape both the quantised and the wide quantised entry take
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(8, [3, '5p'], [11, 4], 60)
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    a = JP.group_rows(below[:3], above[:3], low, high, cats, quants, entry='quant')
    b = JP.group_rows(below[:3], above[:3], low, high, cats, quants, entry='wide_quant')
    assert set(a) == set(b)
    _assert_same(a, b, sorted(a))
    assert [row[0] for row in JP.group_rows_present(a)] == [row[0] for row in JP.group_rows_present(b)]
    # a wide shape: the quant rows those of entry='quant' over the quantised part, the rest those of 'wide_mixed'
    below, above, low, high, ps, sb, sa, edges, _ = W.wide_quant_case(20, [3, 4], [11, 4], 60)
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    b = JP.group_rows(below[:3], above[:3], low, high, cats, quants, entry='wide_quant')
    m = JP.group_rows(below[:3], above[:3], low, high, cats, entry='wide_mixed')
    none = (below[0], np.zeros((len(below[0]), 0)), np.zeros((len(below[0]), 0))), \
        (above[0], np.zeros((len(above[0]), 0)), np.zeros((len(above[0]), 0)))
    q = JP.group_rows(none[0], none[1], [], [], (), quants, entry='quant')
    assert set(b) == set(m) | set(QUANT_KEYS) and set(QUANT_KEYS) <= set(q)
    _assert_same(m, b, sorted(k for k in m if k != 'Dq'))
    _assert_same(q, b, QUANT_KEYS)
    assert (b['Dc'], b['Dk'], b['Dq']) == (20, 2, 2)
    # no discrete label: the rest is the wide entry's
    b0 = JP.group_rows(below[:3], above[:3], low, high, (), quants, entry='wide_quant')
    w0 = JP.group_rows(below[:3], above[:3], low, high, entry='wide')
    _assert_same(w0, b0, sorted(k for k in w0 if k != 'Dq'))
    _assert_same(q, b0, QUANT_KEYS)


def test_wide_quant_pack_limits():
    from hyperopt_amd import joint_pack as JP

    def rows(Dc, us, Vs, **kw):
        below, above, low, high, ps, sb, sa, edges, _ = W.wide_quant_case(Dc, us, Vs, 20)
        return JP.group_rows(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                             Q.quants_of(below, above, edges), **kw)
    assert rows(52, [2] * 8, [2] * 4, entry='wide_quant')['Dq'] == 4
    assert rows(63, [], [5], entry='wide_quant')['Dc'] == 63
    assert rows(1, [], [5], entry='wide_quant')['Dc'] == 1
    with pytest.raises(ValueError, match='at most 8 discrete'):
        rows(10, [2] * 9, [4], entry='wide_quant')
    with pytest.raises(ValueError, match='65 dimensions, at most 64'):
        rows(62, [2], [4, 4], entry='wide_quant')
    with pytest.raises(ValueError, match='at least 1 continuous'):
        rows(0, [2], [4], entry='wide_quant')
    with pytest.raises(ValueError, match='5 quantised dimensions, at most 4'):
        rows(10, [], [2] * 5, entry='wide_quant')
    with pytest.raises(ValueError, match='514 lattice values in the group, at most 512'):
        rows(10, [], [256, 256, 2], entry='wide_quant')
    below, above, low, high, ps, sb, sa, _, _ = W.wide_quant_case(20, [2], [4], 20)
    with pytest.raises(ValueError, match='no quantised dimension'):
        JP.group_rows(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), (), entry='wide_quant')
    # the quantised entry keeps its limits
    with pytest.raises(ValueError, match='at most 8 continuous and 4 discrete'):
        rows(12, [], [11], entry='quant')


# --------------------------------------------------------------------- model
@pytest.mark.parametrize('Dc,us,Vs,n,qlog', [(5, [3, 4], [11, 4], 60, False), (44, [3, '5p', 2], [37], 90, True)])
def test_the_restated_density_is_joint_py_s(Dc, us, Vs, n, qlog):
    """joint.quant_lpdf_numpy is the restatement to 1e-12 at a narrow and at a
    wide shape (the second with the qloguniform lattice)."""
    from hyperopt_amd import joint as J
    below, above, low, high, ps, sb, sa, edges, rs = W.wide_quant_case(Dc, us, Vs, n, qlog=qlog)
    assert W.takes_wide_stage(Dc, len(us), len(Vs)) == (Dc > 8)
    C = 193
    z = np.where(np.isfinite(low)[None, :], rs.uniform(-9, 9, (C, Dc)), rs.normal(1.0, 4.0, (C, Dc)))
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1)
    qi = np.stack([rs.randint(len(e) - 1, size=C) for e in edges], axis=1)
    for side, s in ((below, sb), (above, sa)):
        w, mu, sigma, xc, qmu, qsig = side
        quants = [(qmu[:, d], qsig[:, d], e) for d, e in enumerate(edges)]
        got = J.quant_lpdf_numpy(z, v, qi, w, mu, sigma, low, high, xc, ps, s, quants)
        ref = W.ref_wide_quant_lpdf(z, v, qi, side, low, high, ps, s, edges)
        assert np.isfinite(ref).all()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))


# ------------------------------------------------------------------- startup
def test_startup_is_the_random_suggest(no_device):
    from hyperopt_amd import rand, tpe
    domain = _net(20, [3], [11, 4])
    trials = _with_trials(domain, 5)
    want = rand.suggest([5, 6], domain, trials, 99)
    got = tpe.suggest([5, 6], domain, trials, 99, **ALL)
    assert [d['misc']['vals'] for d in got] == [d['misc']['vals'] for d in want]
