"""Wide branch groups (DESIGN.md "Wide branch groups"), the parts that need no
GPU: how ``joint_branches_wide=True`` changes the plan, its argument errors, the
signatures, the packer's wide segments, the layout of the stage's structs, the
checks tpe_joint_wide_seg_run makes before any launch, and how the suggest
splits the branch groups over the two segmented stages."""
import ctypes
import inspect
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
WIDE_KW = dict(joint=True, joint_wide=True, joint_branches=True, joint_branches_wide=True)


# ------------------------------------------------------------------- the plan
def _labels(prefix, n, kind='uniform'):
    from hyperopt_amd import hp
    make = {'uniform': lambda k: hp.uniform(k, 0, 1), 'loguniform': lambda k: hp.loguniform(k, -3, 1)}[kind]
    return dict(('%s%02d' % (prefix, i), make('%s%02d' % (prefix, i))) for i in range(n))


def _space(n_a=17, n_b=64, extra_b=None):
    """gate 'arch': option 0 a branch of n_a labels, option 1 of n_b, option 2 a
    mixed branch (2 continuous, one discrete, one quantised label), option 3 a
    branch of 3 labels; x, y unconditional."""
    from hyperopt_amd import base, hp
    b = _labels('b', n_b)
    b.update(extra_b or {})
    return base.Domain(lambda d: 0.0, {
        'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 2),
        'arch': hp.choice('arch', [
            _labels('a', n_a, 'loguniform'), b,
            {'c0': hp.uniform('c0', 0, 1), 'c1': hp.uniform('c1', 0, 1), 'ck': hp.randint('ck', 4),
             'cq': hp.quniform('cq', 0, 10, 1)},
            _labels('d', 3)])})


def _plan(table, joint=True, wide_branches=True, **kw):
    from hyperopt_amd import tpe
    return tpe._joint_plan(table, joint, 'philox', 'fp32', NONE4, wide=True,
                           branches=tpe._branch_mode(True, wide_branches, True), **kw)


def test_wide_branches_form_groups():
    from hyperopt_amd import joint as J, tpe
    t = _space().table
    root, groups = _plan(t)
    assert [r.label for r in root] == ['x', 'y']
    assert [[r.label for r in g] for g in groups] == [
        ['a%02d' % i for i in range(17)], ['b%02d' % i for i in range(64)], ['c0', 'c1'], ['d00', 'd01', 'd02']]
    assert [tpe._branch_key(g[0]) for g in groups] == [('arch', 0), ('arch', 1), ('arch', 2), ('arch', 3)]
    assert [tpe._is_wide_branch(g) for g in groups] == [True, True, False, False]
    assert len(set(J.branch_stream_word(g) for g in groups)) == 4
    # without the keyword the 17 labels raise, with joint_wide too
    with pytest.raises(ValueError, match=r"option 0 of gate 'arch' has 17 labels.*TPE_JOINT_MAX_DIMS = 16"):
        _plan(t, wide_branches=False)
    # the sentinel is truthy and travels in `branches`
    assert tpe._branch_mode(True, True, True) == tpe.BRANCH_WIDE and tpe._branch_mode(True, False, True) is True
    assert tpe._branch_mode(False, False, False) is False


def test_narrow_and_mixed_groups_are_the_plan_s_without_the_keyword():
    """Groups of at most 16 labels and mixed groups: the same rows in the same
    order as without the keyword."""
    t = _space(n_a=16, n_b=9).table
    for kw in (dict(), dict(discrete=True, quantized=True, branch_mixed=True)):
        with_kw, without = _plan(t, **kw), _plan(t, wide_branches=False, **kw)
        assert with_kw[0] == without[0] and len(with_kw[1]) == len(without[1]) == 4
        for g, h in zip(with_kw[1], without[1]):
            assert len(g) == len(h) and all(r is q for r, q in zip(g, h))
    mixed = _plan(t, discrete=True, quantized=True, branch_mixed=True)[1]
    assert [r.label for r in mixed[2]] == ['c0', 'c1', 'ck', 'cq']
    # ... and beside a wide group the narrow and the mixed ones are still those
    t2 = _space(n_a=20, n_b=9).table
    with_kw = _plan(t2, discrete=True, quantized=True, branch_mixed=True)[1]
    assert [len(g) for g in with_kw] == [20, 9, 4, 3]
    only = _plan(t2, joint=['b%02d' % i for i in range(9)] + ['c0', 'c1', 'ck', 'cq', 'd00', 'd01', 'd02'],
                 wide_branches=False, discrete=True, quantized=True, branch_mixed=True)[1]
    for g, h in zip(with_kw[1:], only):
        assert all(r is q for r, q in zip(g, h))


def test_a_list_may_name_twenty_conditional_labels():
    t = _space(n_a=30).table
    named = ['a%02d' % i for i in range(5, 25)]
    root, groups = _plan(t, joint=named + ['x', 'y'])
    assert [r.label for r in root] == ['x', 'y'] and [[r.label for r in g] for g in groups] == [named]
    root, groups = _plan(t, joint=named)
    assert root is None and [[r.label for r in g] for g in groups] == [named]
    with pytest.raises(ValueError, match='20 labels'):
        _plan(t, joint=named, wide_branches=False)


# ----------------------------------------------------------------- the errors
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
    for name in ('tpe_joint_run', 'tpe_joint_seg_run', 'tpe_joint_wide_seg_run', 'tpe_run_batch', 'tpe_level_run',
                 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def _mixed17():
    from hyperopt_amd import hp
    return _space(n_a=2, n_b=16, extra_b={'bk': hp.randint('bk', 3)})


ERRORS = [
    (_space, dict(joint=True, joint_wide=True, joint_branches_wide=True),
     'joint_branches_wide=True needs joint_branches=True'),
    (_space, dict(joint=True, joint_branches=True, joint_branches_wide=True),
     'joint_branches_wide=True needs joint_wide=True'),
    (_space, dict(joint_wide=True, joint_branches=True, joint_branches_wide=True), 'needs joint=True or joint='),
    (lambda: _space(n_b=65), WIDE_KW, r"option 1 of gate 'arch' has 65 labels.*TPE_JOINT_WIDE_MAX_DIMS = 64.*joint=\["),
    (_mixed17, dict(WIDE_KW, joint_discrete=True, joint_branches_mixed=True),
     r"option 1 of gate 'arch' has 17 labels.*'bk' is discrete or quantised"),
    # without the keyword: 17 labels under a gate raise as before, joint_wide or not
    (_space, dict(joint=True, joint_wide=True, joint_branches=True),
     r"option 0 of gate 'arch' has 17 labels.*TPE_JOINT_MAX_DIMS = 16.*joint=\["),
]
SUGGEST_ERRORS = [
    (_space, dict(WIDE_KW, joint_shard=(0, 1)),
     r"joint_branches_wide=True does not combine with joint_shard.*option 0 of gate 'arch' has 17 labels"),
    (_space, dict(WIDE_KW, joint_liar='branches'),
     r"joint_liar='branches' does not combine with joint_branches_wide=True.*option 0 of gate 'arch'"),
    (_space, dict(WIDE_KW, joint_discrete=True, joint_quantized=True, joint_branches_mixed=True,
                  joint_liar='branches_mixed'),
     r"joint_liar='branches_mixed' does not combine with joint_branches_wide=True.*option 0 of gate 'arch'"),
    (_space, dict(WIDE_KW, joint_liar=True), 'does not combine with branch groups'),
    (_space, dict(WIDE_KW, joint_liar='mixed'), 'does not combine with branch groups'),
]


@pytest.mark.parametrize('space,kw,match', ERRORS + SUGGEST_ERRORS)
def test_suggest_errors_come_before_any_device_use(space, kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = space()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


@pytest.mark.parametrize('space,kw,match', ERRORS[:2] + ERRORS[3:])
def test_report_errors_come_before_any_device_use(space, kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = space()
    with pytest.raises(ValueError, match=match):
        tpe.joint_candidate_report(0, d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.joint_candidate_report_columns(d.table, history.extract(d, base.Trials()), 0, 1, **kw)


def test_shard_and_liar_keep_working_without_a_wide_group(no_device):
    """The two new errors need a wide branch group in the plan, not the keyword alone."""
    from hyperopt_amd import tpe
    plan = _plan(_space(n_a=16, n_b=9).table)
    tpe._branch_wide_check(plan, (0, 1), 'branches')
    with pytest.raises(ValueError, match='joint_shard'):
        tpe._branch_wide_check(_plan(_space().table), (0, 1), None)


def test_signatures():
    from hyperopt_amd import tpe
    for f in (tpe.suggest, tpe.suggest_choices, tpe.joint_candidate_report, tpe.joint_candidate_report_columns):
        ps = inspect.signature(f).parameters
        assert ps['joint_branches_wide'].default is False
        names = list(ps)
        assert names[names.index('joint_branches_wide') - 1] == 'joint_branches_mixed', f.__name__
    for f in (tpe.suggest, tpe.suggest_choices):
        assert list(inspect.signature(f).parameters)[-3:] == ['joint_wide_mixed', 'joint_wide_quantized', 'joint_liar']
    for f in (tpe.joint_candidate_report, tpe.joint_candidate_report_columns):
        assert list(inspect.signature(f).parameters)[-2:] == ['joint_wide_mixed', 'joint_wide_quantized']
    assert list(inspect.signature(tpe._joint_plan).parameters) == [
        'table', 'joint', 'sampler', 'precision', 'shards', 'discrete', 'quantized', 'wide', 'branches', 'branch_mixed']


# ----------------------------------------------------------------- the packer
def test_wide_segments_in_the_blob_are_the_solo_rows():
    from hyperopt_amd import joint as J, joint_pack as JP
    cases = [R.seeded_case(D, n, 1000 * D + n) for D, n in ((17, 30), (64, 20), (3, 25))]
    models, words = [c[:4] for c in cases], [0xFFFFFFFE - 5, 0xFFFFFFFE - 9, 0xFFFFFFFE - 11]
    C = 8
    inj = [None, np.arange(C * 64, dtype=np.float32).reshape(C, 64) / 64 - 3, None]
    for inject in (None, inj):
        prob_seg = [1, 1] if inject else [1, 0, 2, 1]
        b = JP.segment_blob(models, words, prob_seg, [7, 2 ** 20, 3, 9][:len(prob_seg)], C, inject,
                            N.JOINT_WIDE_SEG_DTYPE)
        assert b.segs.dtype == N.JOINT_WIDE_SEG_DTYPE and b.n_table == 0
        f32 = b.blob[b.offs[4]:b.offs[5]].view(np.float32)
        f64 = b.blob[b.offs[1]:b.offs[2]].view(np.float64)
        assert len(f32) == b.n32 and len(f64) == b.n64
        for s, m in enumerate(models):
            r = JP.group_rows(*m, entry='wide')
            g, D = b.segs[s], r['Dc']
            assert (g['n_dims'], g['k_below'], g['k_above'], g['stream_word']) == (D, r['k_below'], r['k_above'],
                                                                                   words[s])
            assert g['below_base'] == r['below_base'] and g['above_base'] == r['above_base']
            for key, field, _, dtype, _ in JP.group_rows_present(r):
                pool, want = (f32, np.float32) if dtype == np.float32 else (f64, np.float64)
                rows = np.ascontiguousarray(r[key], dtype=want).reshape(-1)
                off = int(g[field])
                assert 0 <= off and off + rows.size <= len(pool), (s, field)
                assert pool[off:off + rows.size].tobytes() == rows.tobytes(), (s, field)
            lo, hi = J.f32_bounds(r['low'], r['high'])
            assert g['lo'][:D].tobytes() == lo.tobytes() and g['hi'][:D].tobytes() == hi.tobytes()
            assert (g['lo'][D:] == -np.inf).all() and (g['hi'][D:] == np.inf).all() and g['lo'].shape == (64,)
            if inject and inject[s] is not None:
                off = int(g['inject'])
                assert f32[off:off + C * D].tobytes() == inject[s].tobytes() and off + C * D <= len(f32)
            else:
                assert g['inject'] == -1
        widths = [len(models[s][2]) for s in prob_seg]
        assert list(b.widths) == widths
        assert list(b.cand_off) == list(np.concatenate([[0], np.cumsum(C * np.array(widths))]))
    with pytest.raises(ValueError, match='65 dimensions, at most 64'):
        JP.segment_blob([R.seeded_case(65, 10, 1)[:4]], [1], [0], [0], C, None, N.JOINT_WIDE_SEG_DTYPE)
    with pytest.raises(ValueError, match='17 dimensions, at most 16'):          # the narrow descriptor keeps its limit
        JP.segment_blob(models[:1], words[:1], [0], [0], C, None, N.JOINT_SEG_DTYPE)
    cat = (np.array([0, 1]), np.array([1]), np.array([0.5, 0.5]), 1.0, 1.0)
    side = (np.array([0.5, 0.5]), np.zeros((2, 2)), np.ones((2, 2)))
    with pytest.raises(ValueError, match='a wide segment holds continuous dimensions only'):
        JP.segment_blob([(side, (np.array([1.0]), np.zeros((1, 2)), np.ones((1, 2))), [-1, -1], [1, 1], [cat])], [1],
                        [0], [0], C, None, N.JOINT_WIDE_SEG_DTYPE)


# ------------------------------------------------------------------------ ABI
def test_wide_segment_structs_match_c():
    lines = ['printf("TPE_ABI_VERSION %d\\n", TPE_ABI_VERSION);',
             'printf("tpe_joint_wide_seg %zu\\ntpe_joint_wide_seg_args %zu\\n", sizeof(tpe_joint_wide_seg), '
             'sizeof(tpe_joint_wide_seg_args));']
    for f, _ in N.JointWideSeg._fields_:
        lines.append('printf("tpe_joint_wide_seg.%s %%zu\\n", offsetof(tpe_joint_wide_seg, %s));' % (f, f))
    for f, _ in N.JointWideSegArgs._fields_:
        lines.append('printf("tpe_joint_wide_seg_args.%s %%zu\\n", offsetof(tpe_joint_wide_seg_args, %s));' % (f, f))
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
    assert lay['tpe_joint_wide_seg'] == ctypes.sizeof(N.JointWideSeg) == N.JOINT_WIDE_SEG_DTYPE.itemsize
    assert lay['tpe_joint_wide_seg_args'] == ctypes.sizeof(N.JointWideSegArgs) == ctypes.sizeof(N.JointSegArgs)
    assert [f for f, _ in N.JointWideSeg._fields_] == list(N.JOINT_WIDE_SEG_DTYPE.names)
    for f, _ in N.JointWideSeg._fields_:
        assert getattr(N.JointWideSeg, f).offset == N.JOINT_WIDE_SEG_DTYPE.fields[f][1] == lay['tpe_joint_wide_seg.' + f]
    for f, _ in N.JointWideSegArgs._fields_:
        assert getattr(N.JointWideSegArgs, f).offset == lay['tpe_joint_wide_seg_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_wide_seg_scratch_bytes', 'tpe_joint_wide_seg_run'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ----------------------------------------------------- argument checks, no GPU
C_HOST = 2049


def _host_args(keep, probs=(0, 1, 1), inject=False, **over):
    """Complete arguments whose 'device' pointers are host arrays: only good for
    calls that return before any launch (the scratch check is the last one and
    _run passes no scratch unless asked)."""
    segs = np.zeros(2, dtype=N.JOINT_WIDE_SEG_DTYPE)
    for s, (D, kb, ka) in enumerate(((17, 4, 9), (64, 1, 1))):
        g = segs[s]
        g['n_dims'], g['k_below'], g['k_above'], g['stream_word'] = D, kb, ka, 0xFFFFFFFE - s
        off = 1000 * s
        for f, n in (('below_mu', kb * D), ('below_a', kb * D), ('below_c', kb), ('above_mu', ka * D),
                     ('above_a', ka * D), ('above_c', ka), ('samp', kb * D * 5)):
            g[f] = off
            off += n
        g['samp_cum'], g['inject'] = 10 * s, -1
    assert off == 1000 + 64 * 9 + 2                       # the last row ends at 1578
    prob_seg = np.array(probs, dtype=np.int32)
    pool = np.zeros(4096)
    keep.extend([segs, prob_seg, pool])
    a = N.JointWideSegArgs()
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
    return lib.tpe_joint_wide_seg_run(ctypes.byref(a) if a is not None else None, p if records else None,
                                      p if cand else None, None, None, p if scratch_bytes else None, scratch_bytes,
                                      None)


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
    (dict(pool_f32_len=1577), b'leave its pool'), (dict(pool_f64_len=10), b'leave its pool'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    err = lib.tpe_last_error()
    assert msg in err and err.startswith(b'tpe_joint_wide_seg_run:'), err


@pytest.mark.parametrize('edit,msg', [
    (_seg_edit(0, n_dims=0), b'n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]'),
    (_seg_edit(1, n_dims=65), b'n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]'),
    (_seg_edit(1, n_dims=-2), b'n_dims outside'),
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
    # every segment as the narrow stage would refuse it (17 and 64 dimensions) gets as far as the scratch check;
    # a segment with no problem is legal
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_wide_seg_scratch_bytes(3, C_HOST, ctypes.byref(need)) == 0
    # the order (3 int32, padded), 9 chunk records a problem, 9 blocks of [64][256] floats a problem
    assert need.value == 16 + 3 * 9 * N.JOINT_WIDE_RECORD_DTYPE.itemsize + 3 * 9 * 256 * 64 * 4
    k2 = []
    assert _run(lib, _host_args(k2, probs=(1, 1, 1)), k2) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(k2), k2, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    # injected candidates: only the segments that have a problem need them
    k3 = []
    a = _host_args(k3, probs=(0, 0), inject=True)
    k3[0][0]['inject'] = 0
    a.pool_f32_len = C_HOST * 17
    assert _run(lib, a, k3) == -1 and b'scratch too small' in lib.tpe_last_error()
    a.pool_f32_len = C_HOST * 17 - 1
    assert _run(lib, a, k3) == -1 and b'leave its pool' in lib.tpe_last_error()
    a = _host_args(k3, probs=(0, 1), inject=True)
    k3[-3][0]['inject'] = 0                      # segment 1 has a problem and no candidates
    a.pool_f32_len = C_HOST * 17
    assert _run(lib, a, k3) == -1 and b'TPE_JOINT_INJECT without candidates' in lib.tpe_last_error()


def test_scratch_bytes():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    rec = N.JOINT_WIDE_RECORD_DTYPE.itemsize
    for n_probs, C, want in ((1, 1, 8 + rec + 65536), (2, 256, 8 + 2 * (rec + 65536)),
                             (7, 4097, 32 + 7 * 17 * (rec + 65536))):
        assert lib.tpe_joint_wide_seg_scratch_bytes(n_probs, C, ctypes.byref(nb)) == 0 and nb.value == want
    sizes = np.zeros((6, 6), dtype=np.uint64)
    for i, n_probs in enumerate((1, 2, 3, 8, 64, 1000)):
        for j, C in enumerate((1, 256, 257, 2049, 4096, 1 << 20)):
            assert lib.tpe_joint_wide_seg_scratch_bytes(n_probs, C, ctypes.byref(nb)) == 0
            sizes[i, j] = nb.value
            # at least what a solo wide run of every problem at 64 dimensions takes
            solo = ctypes.c_uint64(0)
            assert lib.tpe_joint_wide_scratch_bytes(n_probs, C, 64, ctypes.byref(solo)) == 0
            assert nb.value >= solo.value
    assert (np.diff(sizes.astype(np.float64), axis=0) > 0).all()         # monotone in n_probs ...
    assert (np.diff(sizes.astype(np.float64), axis=1) >= 0).all()        # ... and in n_cand
    assert lib.tpe_joint_wide_seg_scratch_bytes(0, 8, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_wide_seg_scratch_bytes(1, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_wide_seg_scratch_bytes(1, 8, None) == -1


# ------------------------------------- the suggest's two segmented calls, no GPU
class _Recorder(object):
    """Stands in for the Engine in tpe._suggest_joint: records the calls;
    problem p of a call wins with the vector (base + p, base + p + 0.5, 0, ...)."""

    def __init__(self):
        self.calls = []

    def run_joint(self, below, above, low, high, ids, n_cand, seed, **kw):
        self.calls.append(('run_joint', np.array(ids), n_cand, seed, kw))
        return np.zeros(len(ids), dtype=N.JOINT_RECORD_DTYPE)

    def _seg(self, name, dtype, base, models, stream_words, prob_seg, prob_id, n_cand, seed, kw):
        self.calls.append((name, models, list(stream_words), list(prob_seg), list(prob_id), n_cand, seed, kw))
        rec = np.zeros(len(prob_seg), dtype=dtype)
        rec['z'][:, 0] = np.arange(len(rec)) + base
        rec['z'][:, 1] = np.arange(len(rec)) + base + 0.5
        return rec

    def run_joint_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, **kw):
        return self._seg('run_joint_segments', N.JOINT_RECORD_DTYPE, 1.0, models, stream_words, prob_seg, prob_id,
                         n_cand, seed, kw)

    def run_joint_wide_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, **kw):
        return self._seg('run_joint_wide_segments', N.JOINT_WIDE_RECORD_DTYPE, 100.0, models, stream_words, prob_seg,
                         prob_id, n_cand, seed, kw)


def test_wide_groups_go_to_their_own_call(monkeypatch):
    from hyperopt_amd import base, history, rand, tpe
    d = _space(n_a=17, n_b=20)
    t = d.table
    trials = base.Trials()
    rs = np.random.RandomState(3)
    for tid in range(30):
        docs = rand.suggest([tid], d, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    hist = history.extract(d, trials)
    ix = dict((k, t.by_label[k].index) for k in t.labels)
    branch = {0: ['a%02d' % i for i in range(17)], 1: ['b%02d' % i for i in range(20)], 2: ['c0', 'c1', 'ck', 'cq'],
              3: ['d00', 'd01', 'd02']}
    ids = [30, 31, 32, 33, 34, 35]
    arch = [3, 1, 0, 2, 1, 3]
    vals = np.full((len(ids), len(t.rows)), np.nan)
    for j, c in enumerate(arch):
        vals[j, ix['arch']], vals[j, ix['x']], vals[j, ix['y']] = c, 0.25, 0.5
        for k in branch[c]:
            vals[j, ix[k]] = 0.5
    act = ~np.isnan(vals)
    rec = _Recorder()
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: rec)
    monkeypatch.setattr(tpe, '_suggest_local', lambda table, *a, **k: tpe.ChoiceColumns(table.labels, vals.copy(),
                                                                                         act.copy()))
    cc = tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, columns=True, **WIDE_KW)
    assert [c[0] for c in rec.calls] == ['run_joint', 'run_joint_segments', 'run_joint_wide_segments']
    _, models, words, prob_seg, prob_id, n_cand, seed, kw = rec.calls[1]
    assert [[r.label for r in m.rows] for m in models] == [['c0', 'c1'], branch[3]]
    assert words == [0xFFFFFFFE - ix['c0'], 0xFFFFFFFE - ix['d00']]
    assert prob_seg == [0, 1, 1] and prob_id == [33, 30, 35] and (n_cand, seed, kw) == (512, 77, {})
    _, models, words, prob_seg, prob_id, n_cand, seed, kw = rec.calls[2]
    assert [[r.label for r in m.rows] for m in models] == [branch[0], branch[1]]
    assert words == [0xFFFFFFFE - ix['a00'], 0xFFFFFFFE - ix['b00']]
    assert prob_seg == [0, 1, 1] and prob_id == [32, 31, 34] and (n_cand, seed, kw) == (512, 77, {})
    # the narrow call is the call of a suggest without the wide groups' labels
    first = rec.calls[1]
    rec.calls[:] = []
    tpe.suggest_choices(t, hist, ids, 77, n_EI_candidates=512, columns=True, joint_branches=True,
                        joint=['x', 'y', 'c0', 'c1'] + branch[3])
    assert rec.calls[1][2:] == first[2:]
    # winners land in the taken branch's columns only
    np.testing.assert_array_equal(cc.active, act)
    v = cc.values
    assert v[2, ix['a00']] == np.exp(100.0) and v[2, ix['a01']] == np.exp(100.5) and v[2, ix['a02']] == 1.0
    assert v[[1, 4], ix['b00']].tolist() == [101.0, 102.0] and v[[1, 4], ix['b01']].tolist() == [101.5, 102.5]
    assert v[3, ix['c0']] == 1.0 and v[3, ix['c1']] == 1.5 and v[3, ix['ck']] == 0.5
    assert v[[0, 5], ix['d00']].tolist() == [2.0, 3.0] and np.isnan(v[0, ix['b00']])
