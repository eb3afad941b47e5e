"""Host tests of joint_quantized='large' (DESIGN.md "Large lattices"): the plan, its ValueErrors, the packer's
record and the argument checks of tpe_joint_quant_large_run.  No device."""
import ctypes
import math

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests.test_joint_quant_host import _host_args, no_device  # noqa: F401


def _space():
    from hyperopt_amd import base, hp
    s = {'lr': hp.loguniform('lr', -7, 0), 'units': hp.quniform('units', 16, 1024, 1),
         'hidden': hp.qloguniform('hidden', math.log(8), math.log(4096), 1), 'q': hp.quniform('q', 0, 10, 1),
         'leaf': hp.choice('leaf', ['a', 'b', 'c']), 'huge': hp.quniform('huge', 0, 65536, 1),
         'c': hp.choice('c', [0, {'k': hp.uniform('inner', 0, 1), 'm': hp.quniform('cq', 0, 300, 1)}])}
    return base.Domain(lambda d: 0.0, s)


def test_the_plan_with_large(no_device):  # noqa: F811
    from hyperopt_amd import joint as J, tpe
    t = _space().table
    none = (None,) * 4
    order = [r.label for r in t.rows]
    assert [J.lattice_size(t.by_label[k].dist, t.by_label[k].args)[1] for k in ('units', 'hidden', 'huge')] == \
        [1009, 4089, 65537]
    got = tpe._joint_group(t, True, 'philox', 'fp32', none, True, 'large')
    assert [r.label for r in got] == [x for x in order if x in ('lr', 'units', 'hidden', 'q', 'leaf')]   # not 'huge'
    crows, drows, qrows = tpe._joint_kernel_order(got)
    assert [r.label for r in crows + drows] == ['lr', 'leaf']
    assert [r.label for r in qrows] == [x for x in order if x in ('units', 'hidden', 'q')]
    assert [r.label for r in tpe._large_rows(got)] == [x for x in order if x in ('units', 'hidden')]
    assert set(r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none, True, True)) == {'lr', 'q', 'leaf'}
    with pytest.raises(ValueError, match="'units' is not eligible with joint_quantized=True: 1009 lattice values, more "
                       'than TPE_JOINT_MAX_LATTICE = 256: such a label is close to continuous, model it as uniform'):
        tpe._joint_group(t, ['lr', 'units'], 'philox', 'fp32', none, False, True)
    from hyperopt_amd import base, hp                        # a large label does not count towards the total
    s = dict(('q%d' % i, hp.quniform('q%d' % i, 0, 255, 1)) for i in range(3))
    s['units'] = hp.quniform('units', 16, 1024, 1)
    with pytest.raises(ValueError, match='TPE_JOINT_MAX_LATTICE_TOTAL = 512 lattice values in all, not 768'):
        tpe._joint_group(base.Domain(lambda d: 0.0, s).table, True, 'philox', 'fp32', none, False, 'large')
    del s['q2']
    assert len(tpe._joint_group(base.Domain(lambda d: 0.0, s).table, True, 'philox', 'fp32', none, False, 'large')) == 3


HEAD = "joint_quantized='large' does not combine with "
TAIL = "'units' has 1009 lattice values, more than TPE_JOINT_MAX_LATTICE = 256, and the %s does not take large lattices"


@pytest.mark.parametrize('kw,match', [
    (dict(joint_wide=True, joint_wide_quantized=True), HEAD + 'joint_wide_quantized=True: ' + TAIL
     % 'wide quantised joint stage'),
    (dict(joint_liar='mixed'), HEAD + "joint_liar='mixed': " + TAIL % 'batch-aware liar stage'),
    (dict(joint_liar=True), HEAD + 'joint_liar=True: ' + TAIL % 'batch-aware liar stage'),
    (dict(joint_shard=(0, 2)), HEAD + 'joint_shard: ' + TAIL % 'sharded joint stage'),
    (dict(joint_precision='fp64', joint_precision_mixed=True), HEAD + "joint_precision='fp64': " + TAIL
     % 'float64 mixed joint stage'),
    (dict(joint=['lr', 'inner', 'cq'], joint_branches=True, joint_branches_mixed=True),
     HEAD + "joint_branches_mixed=True: 'cq' has 301 lattice values, more than TPE_JOINT_MAX_LATTICE = 256, and the "
     'mixed segmented joint stage does not take large lattices'),
    (dict(joint=['lr', 'huge']), "'huge' is not eligible with joint_quantized='large': 65537 lattice values, more than "
     'TPE_JOINT_MAX_LATTICE_LARGE = 65536'),
])
def test_large_argument_errors_come_before_any_device_use(kw, match, no_device):  # noqa: F811
    from hyperopt_amd import base, history, tpe
    d = _space()
    kw = dict(dict(joint=['lr', 'units'], joint_quantized='large'), **kw)
    with pytest.raises(ValueError, match=match.replace('(', r'\(').replace(')', r'\)')):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match.replace('(', r'\(').replace(')', r'\)')):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


def test_other_strings_and_the_report_raise(no_device):  # noqa: F811
    from hyperopt_amd import base, tpe
    d = _space()
    for fn in (lambda **kw: tpe.suggest([0], d, base.Trials(), 1, **kw),
               lambda **kw: tpe.joint_candidate_report(0, d, base.Trials(), 1, **kw)):
        with pytest.raises(ValueError, match="joint_quantized must be True or 'large' .or False.: 'huge'"):
            fn(joint=['lr', 'q'], joint_quantized='huge')
    with pytest.raises(ValueError, match=HEAD + 'joint_candidate_report: ' + TAIL % 'joint candidate report'):
        tpe.joint_candidate_report(0, d, base.Trials(), 1, joint=['lr', 'units'], joint_quantized='large')


def test_the_packer_s_record_of_a_large_label():
    from hyperopt_amd import joint_pack as JP
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(1, [3], [1000, 17], 60)
    args = (below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges))
    r = JP.group_rows(*args, entry='quant_large')
    assert r['quant_v'] == [1000, 17] and r['quant_edge_off'] == [0, 1001] and r['n_lattice'] == 1017
    np.testing.assert_array_equal(r['quant_edges'], np.concatenate(edges))
    assert not [k for k in r if 'table' in k]                # no table bytes: the stage has no table
    with pytest.raises(ValueError, match=r'joint stage: 1000 lattice values, outside \[2, 256\]'):
        JP.group_rows(*args, entry='quant')
    big = Q.quants_of(below, above, [Q.lattice_of(65537)])[:1]
    with pytest.raises(ValueError, match=r'joint stage: 65537 lattice values, outside \[2, 65536\]'):
        JP.group_rows(*args[:5], big, entry='quant_large')


def _run(lib, a, keep, scratch_bytes=0):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_quant_large_run(ctypes.byref(a), p, None, None, None, p if scratch_bytes else None,
                                         scratch_bytes, None)


@pytest.mark.parametrize('over,msg', [
    (dict(n_quant=0), b'n_quant outside [1, TPE_JOINT_MAX_QUANT]'), (dict(n_quant=5), b'n_quant outside [1, TPE_JOINT'),
    (dict(n_dims=9), b'n_dims > 8 or n_cat > 4'), (dict(quant_v=[1, 5]), b'outside [2, TPE_JOINT_MAX_LATTICE_LARGE]'),
    (dict(quant_v=[65537, 5], n_edges=1 << 17), b'outside [2, TPE_JOINT_MAX_LATTICE_LARGE]'),
    (dict(quant_v=[4096, 5], quant_edge_off=[0, 4097]), b'quant_edge_off outside'),
    (dict(below_qsigma=None), b'null quantised rows'),
    (dict(quant_v=[65536, 256], quant_edge_off=[0, 65537], n_edges=65537 + 257, quant_table=None,
          quant_table_bytes=0), b'scratch too small'),      # 65,536 values, no total, no table: accepted
])
def test_large_run_arguments_are_checked_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert b'tpe_joint_quant_large_run' in lib.tpe_last_error() and msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_lds_bytes():
    lib, nb = N.load(), ctypes.c_uint64(0)       # 40 KiB of mini-table, or 32 B a row a chunk may hold; 2 B a row of indices
    for vs, want in (([257], 40960 + 528), ([1500, 1100], 2049 * 32 + 4112), ([65536] * 4, 4097 * 32 + 8208)):
        assert lib.tpe_joint_quant_large_lds_bytes((ctypes.c_int32 * 4)(*vs), len(vs), ctypes.byref(nb)) == 0
        assert nb.value == want, (vs, nb.value)
    assert nb.value + 12 * 1024 <= 160 * 1024                # with the static rows: inside a CU's 160 KiB
