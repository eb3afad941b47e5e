"""Sharded joint stage (DESIGN.md "Sharded joint stage"), the parts that need no
GPU: the additive export and its struct, the argument checks tpe_joint_run_shard
makes before any launch, joint.combine_records against a brute-force np.argmax,
the public keyword's own argument checks, and the unchanged path without it."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
STAGES = ('RUN', 'WIDE', 'MIXED', 'QUANT', 'SEG', 'MSEG')


# ------------------------------------------------------------------------ ABI
def test_abi_stays_24_and_the_shard_struct_matches_c():
    lines = ['printf("TPE_ABI_VERSION %d\\n", TPE_ABI_VERSION);',
             'printf("tpe_joint_shard %zu\\n", sizeof(tpe_joint_shard));']
    for f, _ in N.JointShard._fields_:
        lines.append('printf("tpe_joint_shard.%s %%zu\\n", offsetof(tpe_joint_shard, %s));' % (f, f))
    for s in STAGES:
        lines.append('printf("TPE_JOINT_STAGE_%s %%d\\n", TPE_JOINT_STAGE_%s);' % (s, s))
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
    assert lay['tpe_joint_shard'] == ctypes.sizeof(N.JointShard) == 16
    for f, _ in N.JointShard._fields_:
        assert getattr(N.JointShard, f).offset == lay['tpe_joint_shard.' + f], f
    for i, s in enumerate(STAGES):
        assert lay['TPE_JOINT_STAGE_' + s] == getattr(N, 'JOINT_STAGE_' + s) == i
    assert sorted(N.JOINT_STAGES.values()) == list(range(6))
    for fn in N.JOINT_STAGES:
        assert fn in N.EXPORTS


def test_library_exports_the_shard_call():
    lib = N.load()
    assert 'tpe_joint_run_shard' in N.EXPORTS and hasattr(lib, 'tpe_joint_run_shard')
    assert lib.tpe_abi_version() == 24


# ------------------------------------------------- tpe_joint_run_shard's checks
def _host_args(keep, cls=None, **over):
    """Complete tpe_joint_args (or the wide ones) whose pointers are host arrays:
    only good for calls that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = (cls or N.JointArgs)()
    a.n_dims, a.n_cand, a.n_ids, a.flags = 3, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids', 'inject'):
        setattr(a, f, arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _shard(base, total):
    sh = N.JointShard()
    sh.cand_base, sh.n_cand_global = base, total
    return sh


def _run(lib, stage, a, sh, keep):
    """tpe_joint_run_shard with NO scratch: the stage's scratch check is its last
    one, so every earlier rejection is reached and a call that were wrongly
    accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    return lib.tpe_joint_run_shard(stage, ctypes.byref(a) if a is not None else None,
                                   ctypes.byref(sh) if sh is not None else None, buf.ctypes.data, None, None, None,
                                   None, 0, None)


@pytest.mark.parametrize('stage,over,shard,msg', [
    (0, {}, None, b'null shard'),
    (-1, {}, (0, 2048), b'stage outside'),
    (6, {}, (0, 2048), b'stage outside'),
    (0, {}, (-1, 4096), b'cand_base < 0'),
    (0, {}, (1, 2048), b'cand_base + n_cand > n_cand_global'),
    (0, {}, (0, 2047), b'cand_base + n_cand > n_cand_global'),
    (0, {}, (2 ** 31 - 2048, 2 ** 31), b'n_cand_global >= 2^31'),
    (1, {}, (0, 2 ** 40), b'n_cand_global >= 2^31'),
    (0, dict(flags=N.JOINT_INJECT), (1, 4096), b'TPE_JOINT_INJECT with cand_base != 0'),
    (1, dict(flags=N.JOINT_INJECT), (5, 4096), b'TPE_JOINT_INJECT with cand_base != 0'),
    # what the stage's own entry point checks, through the new call
    (0, dict(n_dims=0), (7, 4096), b'tpe_joint_run: n_dims outside'),
    (0, dict(n_cand=0), (7, 4096), b'tpe_joint_run: n_cand < 1'),
    (0, dict(samp=None), (7, 4096), b'tpe_joint_run: null sampler rows'),
    (1, dict(n_dims=65), (7, 4096), b'tpe_joint_wide_run: n_dims outside'),
    (0, {}, (2 ** 31 - 1 - 2048, 2 ** 31 - 1), b'tpe_joint_run: scratch too small'),    # the largest legal base
    (0, dict(flags=N.JOINT_INJECT), (0, 2048), b'tpe_joint_run: scratch too small'),    # inject at base 0 is legal
])
def test_shard_arguments_are_rejected_without_a_device(stage, over, shard, msg):
    lib, keep = N.load(), []
    a = _host_args(keep, N.JointWideArgs if stage == 1 else N.JointArgs, **over)
    sh = _shard(*shard) if shard is not None else None
    assert _run(lib, stage, a, sh, keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_null_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, 0, None, _shard(0, 8), keep) == -1
    assert b'null args' in lib.tpe_last_error()


@pytest.mark.parametrize('stage,cls,msg', [
    (2, N.JointMixedArgs, b'tpe_joint_mixed_run'), (3, N.JointQuantArgs, b'tpe_joint_quant_run'),
    (4, N.JointSegArgs, b'tpe_joint_seg_run'), (5, N.JointMSegArgs, b'tpe_joint_mseg_run'),
])
def test_every_stage_reaches_its_own_checks(stage, cls, msg):
    """An all-zero args struct with n_cand = 8 passes the shard checks and is
    rejected by the named stage's own first check."""
    lib, keep = N.load(), []
    a = cls()
    a.n_cand = 8
    if stage == 3:
        a.n_quant = -1                               # (0 would hand the call on to the mixed stage)
    assert _run(lib, stage, a, _shard(3, 11), keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()
    assert _run(lib, stage, a, _shard(4, 11), keep) == -1
    assert b'cand_base + n_cand > n_cand_global' in lib.tpe_last_error()


# --------------------------------------------------------------- the combine
def _brute(stacked):
    """Per problem: np.argmax over the scores of the non-empty records in
    ascending global_idx order (an all-empty problem: the first rank's)."""
    world, P = stacked.shape
    out = stacked[0].copy()
    for p in range(P):
        col = stacked[:, p]
        full = col[col['global_idx'] >= 0]
        if len(full) == 0:
            continue
        full = full[np.argsort(full['global_idx'], kind='stable')]
        with np.errstate(invalid='ignore'):
            out[p] = full[np.argmax(full['l'] - full['g'])]
    return out


SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, 1e300, -1e300])


def _records(rs, world, P, dtype):
    """[world, P] records as the parts of a partition give them: rank r's
    global_idx inside its own range (ascending with the rank), scores from a
    small pool so that exact ties, NaN, +-inf and -0.0 / +0.0 meet, empty
    records on some ranks and, now and then, on all of them."""
    st = np.zeros((world, P), dtype=dtype)
    for p in range(P):
        mode = rs.randint(4)
        for r in range(world):
            rec = st[r, p]
            rec['global_idx'] = 1000 * r + rs.randint(1000)
            l = SPECIAL[rs.randint(len(SPECIAL))] if mode else rs.normal()
            g = rs.choice([0.0, -0.0, 1.5, np.inf, np.nan]) if mode == 1 else 0.0
            rec['l'], rec['g'] = l, g
            rec['z'][:] = rs.normal(size=rec['z'].shape)
            if rs.uniform() < (1.0 if mode == 3 and p % 7 == 0 else 0.2):
                rec['global_idx'], rec['l'], rec['g'] = -1, 0.0, 0.0
                rec['z'][:] = 0.0
    return st


@pytest.mark.parametrize('dtype', [N.JOINT_RECORD_DTYPE, N.JOINT_WIDE_RECORD_DTYPE], ids=['record', 'wide'])
def test_combine_records_is_np_argmax_over_the_concatenated_scores(dtype):
    from hyperopt_amd import joint as J
    seen = dict(nan=0, tie=0, zero=0, empty=0, all_empty=0)
    for case in range(100):                          # x 2 dtypes = 200 seeded cases
        rs = np.random.RandomState(7000 + case)
        world = (1, 2, 3, 8)[case % 4]
        st = _records(rs, world, 1 + rs.randint(12), dtype)
        got = J.combine_records(st)
        want = _brute(st)
        assert got.dtype == dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), case
        with np.errstate(invalid='ignore'):
            s = np.where(st['global_idx'] >= 0, st['l'] - st['g'], -np.inf)
        seen['nan'] += int(np.isnan(s).any())
        seen['tie'] += int(any(len(set(col.tolist())) < len(col) for col in s.T if world > 1))
        seen['zero'] += int(((st['l'] == 0) & np.signbit(st['l']) & (st['global_idx'] >= 0)).any())
        seen['empty'] += int((st['global_idx'] < 0).any())
        seen['all_empty'] += int((st['global_idx'] < 0).all(axis=0).any())
    assert all(v >= 5 for v in seen.values()), seen  # the generator reaches every kind of case


def test_combine_records_by_hand():
    from hyperopt_amd import joint as J

    def rec(idx, l, g=0.0):
        r = np.zeros(1, dtype=N.JOINT_RECORD_DTYPE)
        r['global_idx'], r['l'], r['g'], r['z'][0, 0] = idx, l, g, float(idx)
        return r

    def win(*parts):
        return int(J.combine_records(np.stack(parts))['global_idx'][0])
    assert win(rec(5, 1.0), rec(700, 2.0)) == 700                    # the larger score
    assert win(rec(5, 2.0), rec(700, 2.0)) == 5                      # a tie: the lower index
    assert win(rec(700, 2.0), rec(5, 2.0)) == 5                      # ... whatever the rank order
    assert win(rec(5, -0.0), rec(700, 0.0)) == 5 and win(rec(700, -0.0), rec(5, 0.0)) == 5    # -0 ties with +0
    assert win(rec(5, np.inf), rec(700, np.nan)) == 700              # NaN beats every number
    assert win(rec(5, np.nan), rec(700, np.nan)) == 5                # the first NaN
    assert win(rec(5, np.inf, np.inf), rec(700, 9.0)) == 5           # inf - inf is a NaN score
    assert win(rec(-1, 0.0), rec(700, -np.inf)) == 700               # an empty record never wins
    assert win(rec(700, -np.inf), rec(-1, 0.0)) == 700
    assert win(rec(-1, 0.0), rec(-1, 0.0)) == -1
    one = rec(3, 1.0)
    assert J.combine_records(one).tobytes() == one.tobytes()         # [P]: nothing to combine
    for dtype in (N.JOINT_RECORD_DTYPE, N.JOINT_WIDE_RECORD_DTYPE):
        e = J.empty_records(2, dtype)
        assert e.dtype == dtype and (e['global_idx'] == -1).all()
        e['global_idx'] = 0
        assert e.tobytes() == bytes(2 * dtype.itemsize)              # the rest: zeros


# ------------------------------------------------------- the public interface
def _space():
    from hyperopt_amd import base, hp
    s = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
         'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, {'k': hp.uniform('inner', 0, 1)}])}
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
    for name in ('tpe_joint_run', 'tpe_joint_run_shard', 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


@pytest.mark.parametrize('kw,match', [
    (dict(joint_shard=(0, 2)), 'joint_shard needs joint='),
    (dict(joint=False, joint_shard=(0, 2)), 'joint_shard needs joint='),
    (dict(joint=True, joint_shard=(2, 2)), 'pair of ints'),
    (dict(joint=True, joint_shard=(-1, 2)), 'pair of ints'),
    (dict(joint=True, joint_shard=(0, 0)), 'pair of ints'),
    (dict(joint=True, joint_shard=(0, 2, 1)), 'pair of ints'),
    (dict(joint=True, joint_shard=3), 'pair of ints'),
    (dict(joint=True, joint_shard=(0.0, 2)), 'pair of ints'),
    (dict(joint=True, joint_shard=(True, 2)), 'pair of ints'),
    (dict(joint=True, joint_shard='01'), 'pair of ints'),
    (dict(joint=True, joint_shard=(0, 2), sampler='replay'), 'replay'),
    (dict(joint=True, joint_shard=(0, 2), precision='fp64'), 'fp64'),
    (dict(joint=True, joint_shard=(0, 2), shard=(0, 2)), 'joint does not combine with a shard argument'),
    (dict(joint=True, joint_shard=(0, 2), shard_ids=(0, 2)), 'joint does not combine with a shard argument'),
    (dict(joint=True, joint_shard=(0, 2), shard_labels=(0, 2)), 'joint does not combine with a shard argument'),
    (dict(joint=True, joint_shard=(0, 2), shard_grid=(0, 2)), 'joint does not combine with a shard argument'),
    (dict(joint=['x', 'nope'], joint_shard=(0, 2)), "'nope'"),
])
def test_joint_shard_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = _space()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


def test_the_report_does_not_take_the_keyword():
    from hyperopt_amd import tpe
    for fn in (tpe.joint_candidate_report, tpe.joint_candidate_report_columns):
        assert 'joint_shard' not in inspect.signature(fn).parameters
    for fn in (tpe.suggest, tpe.suggest_choices):
        assert inspect.signature(fn).parameters['joint_shard'].default is None


def test_engine_shard_argument_errors():
    """Engine._joint_shard is pure: the range, the 2^31 limit, and no report or
    injected candidates at a non-zero base."""
    from hyperopt_amd.engine import Engine
    sh = Engine._joint_shard((695, 2085), 695)
    assert (sh.cand_base, sh.n_cand_global) == (695, 2085)
    assert Engine._joint_shard(None, 5) is None
    assert Engine._joint_shard((0, 8), 8, report_k=4, inject=np.zeros((8, 2))) is not None
    for shard, C, kw in (((-1, 8), 4, {}), ((5, 8), 4, {}), ((0, 2 ** 31), 4, {}), ((0,), 4, {}), (7, 4, {}),
                         ((1, 8), 4, dict(report_k=2)), ((1, 8), 4, dict(inject=np.zeros((4, 2))))):
        with pytest.raises(ValueError, match='shard'):
            Engine._joint_shard(shard, C, **kw)


def test_without_the_keyword_nothing_changes(golden, no_device):
    """joint_shard=None is the call without the keyword: the plan is formed by
    the same _joint_plan (its signature untouched), and the startup path gives
    the recorded document with or without a joint_shard."""
    import json
    from hyperopt_amd import base, rand, tpe
    assert list(inspect.signature(tpe._joint_plan).parameters) == [
        'table', 'joint', 'sampler', 'precision', 'shards', 'discrete', 'quantized', 'wide', 'branches',
        'branch_mixed']
    d = _space()
    none4 = (None, None, None, None)
    root, groups = tpe._joint_plan(d.table, True, 'philox', 'fp32', none4)
    assert [r.label for r in root] == ['x', 'y', 'z'] and groups == []
    assert tpe._joint_shard_pair(None, False) is None and tpe._joint_shard_pair((np.int64(1), 3), True) == (1, 3)
    g = golden('joint_startup_suggest.json')
    trials = base.Trials()
    for tid in range(5):
        docs = rand.suggest([tid], d, trials, 1000 + tid)
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(tid)}
        trials.insert_trial_docs(docs)
    trials.refresh()

    def plain(docs):
        return json.dumps([{k: [[type(x).__name__, float(x).hex()] for x in v]
                            for k, v in sorted(doc['misc']['vals'].items())} for doc in docs])
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint_shard=None)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True, joint_shard=None)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True, joint_shard=(1, 2))) == g['vals']
