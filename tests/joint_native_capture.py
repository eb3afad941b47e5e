"""Capture what the native driver of the six joint stages (the host part of
hyperopt_amd/csrc/tpe_joint.hip) answers, so that a rewrite of it can be held
to the commit before.

``host``  plain ctypes, host arrays as 'device' pointers (as the _host_args of
          the test_joint_*_host.py files), nothing launches: for a table of
          faulty calls the return code and the whole tpe_last_error() text
          (every TPE_E_ARG message of the six runs, tpe_joint_run_shard, the
          size functions and the profile reads; doubly faulty calls pin the
          order of the checks), and every size function's value at the shapes
          the host tests use.
``gpu``   Engine.run_joint* on cuda:0: one sha256 per case over the bytes of
          records, cand, l and g.  Every chunk-kernel class of every stage once
          in sampling mode, per stage one inject case and one shard whose base
          is no multiple of the chunk.  3 ids, 3 below and 5 above components,
          one candidate more than two whole chunks.

``python -m tests.joint_native_capture host|gpu OUT.json`` writes (or replaces)
that section of OUT.json.  tests/golden/joint_native_parent.json was written
this way by the commit before the native driver was rewritten."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

from hyperopt_amd import _native as N
from tests import joint_pack_capture as P

U64 = ctypes.c_uint64
INJ = N.JOINT_INJECT


# ------------------------------------------------------------------ host mode
def solo_args(keep, cls, **over):
    """Complete arguments of a solo stage over host arrays: 3 continuous, 2
    discrete and 2 quantised labels, as far as ``cls`` has them."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = cls()
    a.n_dims, a.n_cand, a.n_ids, a.flags = 3, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f, t in cls._fields_:
        if t is ctypes.c_void_p and f != 'inject':
            setattr(a, f, arr.ctypes.data)
    if hasattr(a, 'n_cat'):
        a.n_cat = 2
        a.cat_upper[0], a.cat_upper[1], a.cat_off[0], a.cat_off[1] = 3, 5, 0, 3
    if hasattr(a, 'n_quant'):
        a.n_quant, a.n_edges, a.quant_table_bytes = 2, 18, 13 * 16 * 4
        a.quant_v[0], a.quant_v[1], a.quant_edge_off[0], a.quant_edge_off[1] = 11, 5, 0, 12
    for k, v in over.items():
        if not hasattr(cls, k):
            continue
        if isinstance(v, (list, tuple)):
            for d, x in enumerate(v):
                getattr(a, k)[d] = x
        else:
            setattr(a, k, arr.ctypes.data if v == 'ptr' else v)
    return a


def seg_args(keep, mixed, edit=None, **over):
    from tests import test_joint_branch_host as S
    from tests import test_joint_branch_mixed_host as MS
    k = []
    a = (MS if mixed else S)._host_args(k, **over)
    if edit:
        for (s, f), v in edit.items():
            if isinstance(v, tuple):
                k[0][s][f][v[0]] = v[1]
            else:
                k[0][s][f] = v
    keep.extend(k)
    return a


def call(lib, fn, a, keep, records=True, cand=False, scratch_bytes=0, shard=None, stage=None):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    rest = (p if records else None, p if cand else None, None, None, p if scratch_bytes else None, scratch_bytes, None)
    ref = ctypes.byref(a) if a is not None else None
    if stage is None:
        return getattr(lib, fn)(ref, *rest)
    sh = None
    if shard is not None:
        sh = N.JointShard()
        sh.cand_base, sh.n_cand_global = shard
    return lib.tpe_joint_run_shard(stage, ref, ctypes.byref(sh) if sh is not None else None, *rest)


SOLO = (('tpe_joint_run', N.JointArgs, 16), ('tpe_joint_wide_run', N.JointWideArgs, 64),
        ('tpe_joint_mixed_run', N.JointMixedArgs, 16), ('tpe_joint_quant_run', N.JointQuantArgs, 16))
HEAD_ROWS = ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c')
CAT_ROWS = ('below_cat', 'above_cat', 'below_miss', 'below_bonus', 'above_miss', 'above_bonus', 'below_h', 'cat_cum')
QUANT_ROWS = ('quant_edges', 'below_qmu', 'below_qsigma', 'above_qmu', 'above_qsigma', 'quant_samp', 'quant_table')


def host_table():
    """[(name, f(lib, keep) -> rc)]: the faulty calls."""
    t = []

    def solo(fn, cls, name, kw=None, **over):
        t.append(('%s/%s' % (fn, name), lambda lib, keep: call(lib, fn, solo_args(keep, cls, **over), keep, **(kw or {}))))

    for fn, cls, top in SOLO:
        t.append((fn + '/null_args', lambda lib, keep, fn=fn: call(lib, fn, None, keep)))
        for name, over in (
                ('n_dims_0', dict(n_dims=0, n_cat=0, n_quant=0) if fn != 'tpe_joint_quant_run' else dict(n_dims=-1)),
                ('n_dims_top', dict(n_dims=top + 1)), ('n_cand_0', dict(n_cand=0)), ('n_ids_0', dict(n_ids=0)),
                ('k_below_0', dict(k_below=0)), ('k_above_0', dict(k_above=0)),
                ('inject_null', dict(flags=INJ)), ('inject_ok', dict(flags=INJ, inject='ptr')),
                ('samp_cum_null', dict(samp_cum=None)), ('samp_null', dict(samp=None)), ('ids_null', dict(ids=None)),
                ('too_many', dict(n_cand=2 ** 31 - 1, n_ids=2 ** 22)), ('scratch_null', dict()),
                # two faults: the earlier check answers
                ('2_dims_cand', dict(n_dims=top + 1, n_cand=0)), ('2_cand_ids', dict(n_cand=0, n_ids=0)),
                ('2_ids_k', dict(n_ids=0, k_above=0)), ('2_k_rows', dict(k_below=0, below_c=None)),
                ('2_rows_inject', dict(above_c=None, flags=INJ)), ('2_inject_ids', dict(flags=INJ, ids=None)),
                ('2_samp_ids', dict(samp=None, ids=None)), ('2_ids_many', dict(ids=None, n_cand=2 ** 31 - 1, n_ids=2 ** 22)),
                ('2_inject_samp', dict(flags=INJ, inject='ptr', samp=None, samp_cum=None))):
            solo(fn, cls, name, **over)
        for f in HEAD_ROWS:
            solo(fn, cls, f + '_null', **{f: None})
        solo(fn, cls, 'records_null', dict(records=False))
        solo(fn, cls, '2_records_many', dict(records=False), n_cand=2 ** 31 - 1, n_ids=2 ** 22)
        solo(fn, cls, 'scratch_short', dict(scratch_bytes=151))
        solo(fn, cls, '2_many_scratch', dict(scratch_bytes=151), n_cand=2 ** 31 - 1, n_ids=2 ** 22)
    for fn, cls in (('tpe_joint_mixed_run', N.JointMixedArgs), ('tpe_joint_quant_run', N.JointQuantArgs)):
        none = dict((f, None) for f in ('below_mu', 'below_a', 'above_mu', 'above_a', 'samp'))
        for name, over in (
                ('n_cat_neg', dict(n_cat=-1)), ('dims_sum', dict(n_dims=13, n_cat=4)), ('n_dims_neg', dict(n_dims=-1)),
                ('n_cat_17', dict(n_dims=0, n_cat=17)),
                ('no_cont', dict(n_dims=0, **none)), ('no_cont_c_null', dict(n_dims=0, below_c=None)),
                ('no_cont_cum_null', dict(n_dims=0, samp_cum=None, **none)),
                ('cat_upper_1', dict(cat_upper=[1, 5])), ('cat_upper_257', dict(cat_upper=[3, 257])),
                ('cat_off_high', dict(cat_off=[0, 4])), ('cat_off_neg', dict(cat_off=[-1, 3])),
                ('2_neg_cat_dims', dict(n_cat=-1, n_dims=17)), ('2_neg_dims_cand', dict(n_dims=-1, n_cand=0)),
                ('2_ids_tables', dict(ids=None, below_cat=None)), ('2_tables_upper', dict(cat_cum=None, cat_upper=[1, 5])),
                ('2_upper_off', dict(cat_upper=[3, 0], cat_off=[-1, 3])),
                ('2_off_many', dict(cat_off=[0, 4], n_cand=2 ** 31 - 1, n_ids=2 ** 22))):
            solo(fn, cls, name, **over)
        for f in CAT_ROWS:
            solo(fn, cls, f + '_null', **{f: None})
        # n_cat = 0 (and n_quant = 0): the stage before, with its name
        z = dict(n_quant=0) if fn == 'tpe_joint_quant_run' else {}
        junk = dict(cat_upper=[0, 999], below_cat=None, cat_cum=None)
        for name, over in (('fwd_scratch', dict(n_cat=0, **junk)), ('fwd_n_cand', dict(n_cat=0, n_cand=0)),
                           ('fwd_rows', dict(n_cat=0, below_mu=None)), ('fwd_dims_0', dict(n_cat=0, n_dims=0)),
                           ('fwd_samp', dict(n_cat=0, samp=None))):
            solo(fn, cls, name, **dict(over, **z))
    fn, cls = 'tpe_joint_mixed_run', N.JointMixedArgs
    solo(fn, cls, 'cat_total', n_cat=5, cat_upper=[256] * 5, cat_off=[0, 256, 512, 768, 1024])
    solo(fn, cls, '2_total_off', n_cat=5, cat_upper=[256] * 5, cat_off=[-1, 256, 512, 768, 1024])
    solo(fn, cls, 'cat_16', n_dims=0, n_cat=16, cat_upper=[2] * 16, cat_off=list(range(0, 32, 2)))
    fn, cls = 'tpe_joint_quant_run', N.JointQuantArgs
    for name, over in (
            ('n_quant_neg', dict(n_quant=-1)), ('n_quant_5', dict(n_quant=5)),
            ('fwd_mixed_scratch', dict(n_quant=0, quant_v=[0, 999], quant_edges=None, quant_table_bytes=0)),
            ('fwd_mixed_upper', dict(n_quant=0, cat_upper=[1, 5])), ('fwd_mixed_cand', dict(n_quant=0, n_cand=0)),
            ('fwd_mixed_wide', dict(n_quant=0, n_dims=9, n_cat=5, cat_upper=[2] * 5, cat_off=[0, 2, 4, 6, 8])),
            ('dims_17', dict(n_dims=17)), ('sum_17', dict(n_dims=8, n_cat=4, n_quant=4, n_cand=0)),
            ('sum_over', dict(n_dims=13, n_cat=2)), ('n_dims_9', dict(n_dims=9)), ('n_cat_5', dict(n_dims=2, n_cat=5)),
            ('no_cat', dict(n_cat=0, below_cat=None, cat_cum=None, cat_upper=[0, 999])),
            ('quant_v_1', dict(quant_v=[1, 5])), ('quant_v_257', dict(quant_v=[11, 257])),
            ('lattice_total', dict(n_quant=3, quant_v=[256, 256, 2], quant_edge_off=[0, 257, 514], n_edges=517,
                                   quant_table_bytes=13 * 514 * 4)),
            ('edge_off_high', dict(quant_edge_off=[0, 13])), ('edge_off_neg', dict(quant_edge_off=[-1, 12])),
            ('n_edges_17', dict(n_edges=17)), ('table_short', dict(quant_table_bytes=13 * 16 * 4 - 1)),
            ('2_quant_null', dict(n_quant=5, n_cand=0)), ('2_dims_89', dict(n_dims=17, n_cat=5)),
            ('2_89_cand', dict(n_dims=9, n_cand=0)), ('2_off_lattice', dict(cat_off=[0, 4], quant_v=[1, 5])),
            ('2_v_total', dict(n_quant=3, quant_v=[256, 256, 1])),
            ('2_total_edge', dict(n_quant=3, quant_v=[256, 256, 2], quant_edge_off=[-1, 257, 514], n_edges=517)),
            ('2_edge_rows', dict(n_edges=17, quant_samp=None)), ('2_rows_table', dict(below_qmu=None, quant_table_bytes=0)),
            ('2_table_many', dict(quant_table_bytes=0, n_cand=2 ** 31 - 1, n_ids=2 ** 22))):
        solo(fn, cls, name, **over)
    for f in QUANT_ROWS:
        solo(fn, cls, f + '_null', **{f: None})

    def seg(mixed, name, kw=None, edit=None, **over):
        fn = 'tpe_joint_mseg_run' if mixed else 'tpe_joint_seg_run'
        t.append(('%s/%s' % (fn, name),
                  lambda lib, keep: call(lib, fn, seg_args(keep, mixed, edit, **over), keep, **(kw or {}))))

    for mixed in (False, True):
        fn = 'tpe_joint_mseg_run' if mixed else 'tpe_joint_seg_run'
        t.append((fn + '/null_args', lambda lib, keep, fn=fn: call(lib, fn, None, keep)))
        for name, over in (
                ('n_segs_0', dict(n_segs=0)), ('n_probs_0', dict(n_probs=0)),
                ('n_cand_0', dict(n_cand=0)), ('segs_null', dict(segs=None)), ('host_segs_null', dict(host_segs=None)),
                ('pool_f32_null', dict(pool_f32=None)), ('pool_f64_null', dict(pool_f64=None)),
                ('pool_f64_null_inject', dict(pool_f64=None, flags=INJ)),
                ('prob_seg_null', dict(prob_seg=None)), ('host_prob_seg_null', dict(host_prob_seg=None)),
                ('prob_id_null', dict(prob_id=None)), ('inject_none', dict(flags=INJ)),
                ('pool_f32_short', dict(pool_f32_len=1)), ('pool_f64_short', dict(pool_f64_len=1)),
                ('prob_low', dict(probs=(0, -1))), ('prob_high', dict(probs=(0, 7))), ('scratch_null', dict()),
                ('too_many', dict(n_cand=2 ** 31 - 1, probs=(0,) * 1024)),
                ('2_segs_probs', dict(n_segs=0, n_probs=0)), ('2_probs_cand', dict(n_probs=0, n_cand=0)),
                ('2_cand_segs', dict(n_cand=0, segs=None)), ('2_segs_pool', dict(host_segs=None, pool_f32=None)),
                ('2_pool_prob', dict(pool_f32=None, prob_id=None)), ('2_pool_prob_seg', dict(pool_f32_len=1, probs=(9,))),
                ('2_prob_inject', dict(probs=(0, 9), flags=INJ))):
            seg(mixed, name, **over)
        seg(mixed, 'records_null', dict(records=False))
        seg(mixed, 'cand_without_off', dict(cand=True))
        seg(mixed, '2_prob_id_records', dict(records=False), prob_id=None)
        seg(mixed, '2_records_cand', dict(records=False, cand=True))
        seg(mixed, '2_cand_segment', dict(cand=True), {(0, 'n_dims'): 0})
        seg(mixed, 'scratch_short', dict(scratch_bytes=159))
        for name, edit in (
                ('seg_dims_0', {(0, 'n_dims'): 0}), ('seg_dims_17', {(0, 'n_dims'): 17}),
                ('seg_k_below_0', {(0, 'k_below'): 0}), ('seg_k_above_0', {(1, 'k_above'): 0}),
                ('seg_mu_neg', {(0, 'below_mu'): -1}), ('seg_above_a_far', {(1, 'above_a'): 1 << 40}),
                ('seg_samp_far', {(0, 'samp'): 1 << 20}), ('seg_cum_far', {(0, 'samp_cum'): 1 << 20}),
                ('2_seg_dims_k', {(0, 'n_dims'): 0, (0, 'k_below'): 0}),
                ('2_seg_k_rows', {(0, 'k_above'): 0, (0, 'below_c'): -1}),
                ('2_seg0_seg1', {(0, 'below_c'): -1, (1, 'n_dims'): 0})):
            seg(mixed, name, edit=edit)
        seg(mixed, '2_rows_prob', edit={(1, 'above_c'): -1}, probs=(5,))
    for name, edit in (
            ('seg_n_cat_neg', {(1, 'n_cat'): -1}), ('seg_n_cat_17', {(1, 'n_cat'): 17}),
            ('seg_n_quant_neg', {(2, 'n_quant'): -1}), ('seg_n_quant_5', {(2, 'n_quant'): 5}),
            ('seg_dims_neg', {(1, 'n_dims'): -1}), ('seg_dims_9', {(2, 'n_dims'): 9}), ('seg_cat_5', {(1, 'n_cat'): 5}),
            ('seg_upper_1', {(1, 'cat_upper'): (0, 1)}), ('seg_upper_257', {(1, 'cat_upper'): (0, 257)}),
            ('seg_cat_off', {(1, 'cat_off'): (0, 1)}), ('seg_cat_off_neg', {(2, 'cat_off'): (0, -1)}),
            ('seg_v_1', {(2, 'quant_v'): (1, 1)}), ('seg_v_257', {(2, 'quant_v'): (0, 257)}),
            ('seg_edge_off', {(2, 'quant_edge_off'): (1, 7)}), ('seg_edge_off_neg', {(2, 'quant_edge_off'): (0, -1)}),
            ('seg_cat_far', {(1, 'above_cat'): 1 << 40}), ('seg_bonus_far', {(1, 'below_bonus'): 1 << 20}),
            ('seg_h_neg', {(1, 'below_h'): -1}), ('seg_qsamp_far', {(2, 'quant_samp'): 1 << 20}),
            ('seg_edges_far', {(2, 'quant_edges'): 1 << 20}), ('seg_n_edges_far', {(2, 'n_edges'): 1 << 20}),
            ('seg_qmu_neg', {(2, 'below_qmu'): -1}), ('seg_table_1', {(2, 'table'): 1}),
            ('seg_table_neg', {(2, 'table'): -1}),
            ('2_cat_quant', {(2, 'n_cat'): -1, (2, 'n_quant'): 5}), ('2_quant_dims', {(2, 'n_quant'): 5, (2, 'n_dims'): 9}),
            ('2_dims_k', {(1, 'n_dims'): 9, (1, 'k_below'): 0}), ('2_k_upper', {(1, 'k_below'): 0, (1, 'cat_upper'): (0, 1)}),
            ('2_upper_v', {(2, 'cat_upper'): (0, 1), (2, 'quant_v'): (0, 1)}),
            ('2_cat_off_v', {(2, 'cat_off'): (0, 1), (2, 'quant_v'): (0, 1)}),
            ('2_v_edge', {(2, 'quant_v'): (1, 300), (2, 'quant_edge_off'): (0, -1)}),
            ('2_edge_rows', {(2, 'quant_edge_off'): (0, -1), (2, 'below_c'): -1}),
            ('2_rows_table', {(2, 'below_c'): -1, (2, 'table'): -1})):
        seg(True, name, edit=edit)
    seg(True, 'n_segs_32768', n_segs=32768)               # (checked before the segments are read)
    seg(True, 'seg_lattice_total', edit={(2, 'n_quant'): 3, (2, 'quant_v'): (slice(0, 3), (256, 256, 2))})
    seg(True, '2_total_edge', edit={(2, 'n_quant'): 3, (2, 'quant_v'): (slice(0, 3), (256, 256, 2)),
                                    (2, 'quant_edge_off'): (0, -1)})
    seg(True, 'quant_pool_f64_null', pool_f64=None, flags=INJ)
    seg(True, 'quant_table_null', quant_table=None)
    seg(True, '2_edge_table_null', edit={(2, 'quant_edge_off'): (0, -1)}, quant_table=None)
    seg(True, 'table_short', quant_table_bytes=4 * 81 - 1)
    seg(True, '2_table_prob', quant_table_bytes=0, probs=(9,))

    def shard(name, stage, cls, sh, **over):
        t.append(('tpe_joint_run_shard/' + name, lambda lib, keep: call(
            lib, None, None if cls is None else solo_args(keep, cls, **over), keep, shard=sh, stage=stage)))
    shard('null_args', 0, None, (0, 8))
    shard('null_shard', 0, N.JointArgs, None)
    shard('2_args_shard', 0, None, None)
    shard('stage_neg', -1, N.JointArgs, (0, 2048))
    shard('stage_6', 6, N.JointArgs, (0, 2048))
    shard('2_shard_stage', 6, N.JointArgs, None)
    shard('base_neg', 0, N.JointArgs, (-1, 4096))
    shard('2_stage_base', 7, N.JointArgs, (-1, 4096))
    shard('global_2_31', 0, N.JointArgs, (2 ** 31 - 2048, 2 ** 31))
    shard('2_base_global', 1, N.JointWideArgs, (-1, 2 ** 40))
    shard('past_end', 0, N.JointArgs, (1, 2048))
    shard('short_global', 0, N.JointArgs, (0, 2047))
    shard('2_global_end', 0, N.JointArgs, (2 ** 31, 2 ** 31))
    shard('inject_base', 0, N.JointArgs, (1, 4096), flags=INJ, inject='ptr')
    shard('2_end_inject', 0, N.JointArgs, (1, 2048), flags=INJ)
    shard('inject_base_0', 0, N.JointArgs, (0, 2048), flags=INJ, inject='ptr')
    shard('largest_base', 0, N.JointArgs, (2 ** 31 - 1 - 2048, 2 ** 31 - 1))
    for stage, (fn, cls, top) in zip((0, 1, 2, 3), SOLO):
        shard('%s_dims' % fn, stage, cls, (7, 4096), n_dims=top + 1)
        shard('%s_scratch' % fn, stage, cls, (7, 4096))
        shard('%s_inject_base' % fn, stage, cls, (7, 4096), flags=INJ)
        shard('%s_past_end' % fn, stage, cls, (4, 2051), n_dims=top + 1)
    for stage, mixed in ((4, False), (5, True)):
        for name, sh, over in (('scratch', (3, 2051), {}), ('past_end', (4, 2051), {}), ('n_probs_0', (3, 2051), dict(n_probs=0)),
                               ('inject_base', (3, 2051), dict(flags=INJ))):
            t.append(('tpe_joint_run_shard/%s_%s' % ('mseg' if mixed else 'seg', name),
                      lambda lib, keep, stage=stage, mixed=mixed, sh=sh, over=over: call(
                          lib, None, seg_args(keep, mixed, **over), keep, shard=sh, stage=stage)))

    def prof(name, f):
        t.append((name, f))
    # (whether the process has profiled a run before is state: turning the profile off forgets the last run, and the
    # two companions are asked with a null pointer, which they answer the same way)
    prof('tpe_joint_profile/off', lambda lib, keep: lib.tpe_joint_profile(0, None))
    prof('tpe_joint_profile/read_without_run',
         lambda lib, keep: lib.tpe_joint_profile(0, None) or lib.tpe_joint_profile(0, keep_buf(keep)))
    prof('tpe_joint_quant_profile/null', lambda lib, keep: lib.tpe_joint_quant_profile(None))
    prof('tpe_joint_wide_profile/null', lambda lib, keep: lib.tpe_joint_wide_profile(None))
    return t


def keep_buf(keep):
    buf = np.zeros(8)
    keep.append(buf)
    return buf.ctypes.data


def size_table():
    """[(name, f(lib, keep) -> [rc, bytes])]: every size function at the shapes
    the host tests use, and its rejections."""
    t = []

    def add(fn, *args):
        def f(lib, keep):
            nb = U64(0)
            rc = getattr(lib, fn)(*args, ctypes.byref(nb))
            return [rc, int(nb.value) if rc == 0 else None]
        t.append(('%s%r' % (fn, args), f))

    def add_null(fn, *args):
        t.append(('%s%r/null' % (fn, args), lambda lib, keep: [getattr(lib, fn)(*args, None), None]))
    for fn in ('tpe_joint_scratch_bytes', 'tpe_joint_seg_scratch_bytes', 'tpe_joint_mseg_scratch_bytes'):
        for shape in ((1, 1), (1, 1024), (1, 1025), (1, 2048), (2, 1024), (3, 2048), (3, 4097), (4, 2048), (7, 4097),
                      (5, 100000), (2 ** 20, 2 ** 31 - 1), (0, 8), (1, 0), (-1, -1)):
            add(fn, *shape)
        add_null(fn, 1, 8)
    for D in (1, 16, 17, 20, 21, 24, 25, 32, 33, 48, 49, 64):
        for shape in ((1, 2048), (3, 4097), (1, 1), (3, 513)):
            add('tpe_joint_wide_scratch_bytes', *(shape + (D,)))
    for bad in ((0, 8, 20), (1, 0, 20), (1, 8, 0), (1, 8, 65)):
        add('tpe_joint_wide_scratch_bytes', *bad)
    add_null('tpe_joint_wide_scratch_bytes', 1, 8, 20)
    for shape in ((26, 9976, 32), (4, 9, 16), (1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 512), (0, 9, 32), (4, 0, 32), (4, 9, 0)):
        add('tpe_joint_quant_table_bytes', *shape)
    add_null('tpe_joint_quant_table_bytes', 4, 9, 32)

    def mseg_table(name, n, edit=None, null=False, null_out=False):
        def f(lib, keep):
            seg_args(keep, True)
            segs = keep[-3]
            if edit == 'two':
                segs = np.concatenate([segs[2:], segs[2:]])
                segs[1]['k_below'], segs[1]['quant_v'][:2] = 300, (256, 256)
            elif edit:
                for (s, fld), v in edit.items():
                    if isinstance(v, tuple):
                        segs[s][fld][v[0]] = v[1]
                    else:
                        segs[s][fld] = v
            keep.append(segs)
            nb = U64(0)
            rc = lib.tpe_joint_mseg_table_bytes(None if null else segs.ctypes.data, n, None if null_out else ctypes.byref(nb))
            return [rc, int(nb.value) if rc == 0 else None]
        t.append(('tpe_joint_mseg_table_bytes/' + name, f))
    mseg_table('three', 3)
    mseg_table('two_plain', 2)
    mseg_table('one', 1)
    mseg_table('two_large', 2, 'two')
    mseg_table('n_0', 0)
    mseg_table('null_segs', 2, null=True)
    mseg_table('null_out', 2, null_out=True)
    mseg_table('v_257', 3, {(2, 'quant_v'): (0, 257)})
    mseg_table('v_1', 3, {(2, 'quant_v'): (1, 1)})
    mseg_table('n_quant_5', 3, {(2, 'n_quant'): 5})
    mseg_table('n_quant_neg', 3, {(1, 'n_quant'): -1})
    mseg_table('k_below_0', 3, {(0, 'k_below'): 0})
    mseg_table('k_above_0', 3, {(1, 'k_above'): 0})
    mseg_table('2_quant_v', 3, {(2, 'n_quant'): 5, (2, 'quant_v'): (0, 257)})
    mseg_table('over_512', 3, {(2, 'n_quant'): 3, (2, 'quant_v'): (slice(0, 3), (256, 256, 2))})
    return t


def capture_host():
    lib = N.load()
    out = {'faults': {}, 'sizes': {}}
    for name, f in host_table():
        keep = []
        assert name not in out['faults'], name
        rc = f(lib, keep)
        out['faults'][name] = [int(rc), lib.tpe_last_error().decode() if rc != 0 else None]
    for name, f in size_table():
        keep = []
        assert name not in out['sizes'], name
        rc, nb = f(lib, keep)
        out['sizes'][name] = [int(rc), nb, lib.tpe_last_error().decode() if rc != 0 else None]
    return out


# ------------------------------------------------------------------- gpu mode
IDS3 = [3, 7, 11]
SEED = 1234
CHUNK = N.JOINT_CHUNK
N_CAND = 2 * CHUNK + 1
SHARD_BASE = 1500                       # no multiple of 256, 512 or 1024
KB, KA = 3, 5


def trim(group):
    """The group with its first KA above components (weights renormalised):
    cont_group & co. give 3 below and 39 above ones."""
    below, above = group[0], group[1]
    assert len(below[0]) == KB and len(above[0]) >= KA
    above = (above[0][:KA] / above[0][:KA].sum(),) + tuple(x[:KA] for x in above[1:])
    out = [below, above, group[2], group[3]]
    if len(group) > 4:
        out.append([(xb, xa[:KA], p, sb, sa) for xb, xa, p, sb, sa in group[4]])
    if len(group) > 5:
        out.append([(mb, sb, ma[:KA], sa[:KA], e) for mb, sb, ma, sa, e in group[5]])
    return tuple(out)


def inject_n(group, n, seed=5):
    """joint_pack_capture.inject_of over ``n`` candidates."""
    old = P.C
    P.C = n
    try:
        return P.inject_of(group, seed)
    finally:
        P.C = old


US = [2, 3, 4, '5p', 2, 3, 4, 2, 3]     # the category counts of up to 9 discrete labels
VS = [5, 50, 7]                         # the lattice sizes of up to 3 quantised labels
CONT_D = (1, 2, 3, 4, 5, 7, 9, 13)      # one D per padded width 1, 2, 3, 4, 6, 8, 12, 16
WIDE_D = (17, 21, 25, 33, 49)           # 20, 24, 32, 48, 64
MIXED_DC = (0, 1, 3, 5, 9)              # CP 0, 2, 4, 8, 16
MIXED_DK = (1, 2, 3, 5, 9)              # KP 1, 2, 4, 8, 16
QUANT_DC = (0, 1, 3, 5)                 # CP 0, 2, 4, 8
QUANT_DK = (0, 1, 2, 3)                 # KP 0, 1, 2, 4
QUANT_DQ = (1, 2, 3)                    # QP 1, 2, 4


def wide_cand(D):
    return 2 * 256 * (2 if D <= 32 else 1) + 1


def mseg_groups():
    """One group per class of the mixed segmented stage: 8 + 12 + 48."""
    g = [trim(P.cont_group(D)) for D in CONT_D]
    g += [trim(P.mixed_group(Dc, US[:Dk])) for Dc in QUANT_DC for Dk in (1, 2, 3)]
    g += [trim(P.quant_group(Dc, US[:Dk], VS[:Dq])) for Dc in QUANT_DC for Dk in QUANT_DK for Dq in QUANT_DQ]
    return g


def seg_problems(n_groups):
    """Every group scores id 0, every second one id 1 too, every third id 2, the
    groups in falling order so that the order kernel has work."""
    probs, pids = [], []
    for j, pid in enumerate(IDS3):
        for s in reversed(range(n_groups)):
            if s % (j + 1) == 0:
                probs.append(s)
                pids.append(pid)
    return probs, pids


def gpu_cases():
    """{name: f(engine) -> (records, cand, l, g)}."""
    out = {}
    kw = dict(return_cand=True, want_lg=True)

    def add(name, f):
        assert name not in out
        out[name] = f
    for D in CONT_D:
        add('run_D%d' % D, lambda e, D=D: e.run_joint(*trim(P.cont_group(D)), IDS3, N_CAND, SEED, **kw))
    for D in WIDE_D:
        add('wide_D%d' % D, lambda e, D=D: e.run_joint_wide(*trim(P.cont_group(D)), IDS3, wide_cand(D), SEED, **kw))
    for Dc in MIXED_DC:
        for Dk in MIXED_DK:
            if Dc + Dk <= N.JOINT_MAX_DIMS:                      # (all but 9 + 9: no <16, 16> kernel)
                add('mixed_%d_%d' % (Dc, Dk), lambda e, Dc=Dc, Dk=Dk: e.run_joint_mixed(
                    *trim(P.mixed_group(Dc, US[:Dk])), IDS3, N_CAND, SEED, **kw))
    for Dc in QUANT_DC:
        for Dk in QUANT_DK:
            for Dq in QUANT_DQ:
                add('quant_%d_%d_%d' % (Dc, Dk, Dq), lambda e, Dc=Dc, Dk=Dk, Dq=Dq: e.run_joint_quant(
                    *trim(P.quant_group(Dc, US[:Dk], VS[:Dq])), IDS3, N_CAND, SEED, **kw))

    def seg_case(groups, **more):
        def f(e):
            gs = groups()
            words = [0xFFFFFFFE - s for s in range(len(gs))]
            probs, pids = seg_problems(len(gs))
            return e.run_joint_segments(gs, words, probs, pids, N_CAND, SEED, **dict(kw, **more))
        return f
    add('seg_all', seg_case(lambda: [trim(P.cont_group(D)) for D in CONT_D]))
    add('mseg_all', seg_case(mseg_groups))

    g3, g21 = trim(P.cont_group(3)), trim(P.cont_group(21))
    m32, q312 = trim(P.mixed_group(3, US[:2])), trim(P.quant_group(3, US[:1], VS[:2]))
    sh = dict(shard=(SHARD_BASE, 8192))
    add('run_inject', lambda e: e.run_joint(*g3, IDS3, N_CAND, SEED, inject=inject_n(g3, N_CAND), **kw))
    add('run_shard', lambda e: e.run_joint(*g3, IDS3, N_CAND, SEED, **dict(kw, **sh)))
    add('wide_inject', lambda e: e.run_joint_wide(*g21, IDS3, wide_cand(21), SEED, inject=inject_n(g21, wide_cand(21)), **kw))
    add('wide_shard', lambda e: e.run_joint_wide(*g21, IDS3, wide_cand(21), SEED, **dict(kw, **sh)))
    add('mixed_inject', lambda e: e.run_joint_mixed(*m32, IDS3, N_CAND, SEED, inject=inject_n(m32, N_CAND), **kw))
    add('mixed_shard', lambda e: e.run_joint_mixed(*m32, IDS3, N_CAND, SEED, **dict(kw, **sh)))
    add('quant_inject', lambda e: e.run_joint_quant(*q312, IDS3, N_CAND, SEED, inject=inject_n(q312, N_CAND), **kw))
    add('quant_shard', lambda e: e.run_joint_quant(*q312, IDS3, N_CAND, SEED, **dict(kw, **sh)))
    few = [g3, trim(P.cont_group(7)), trim(P.cont_group(2))]
    mfew = [g3, m32, q312, trim(P.quant_group(0, [], VS[:1]))]
    for name, groups in (('seg', few), ('mseg', mfew)):
        add(name + '_inject', seg_case(lambda groups=groups: groups,
                                       inject=[inject_n(g, N_CAND, 7 + i) for i, g in enumerate(groups)]))
        add(name + '_shard', seg_case(lambda groups=groups: groups, **sh))
    return out


# the six stages' calls of the profiling test (tests/test_gpu_joint_native_parent.py)
STAGE_CASES = dict(run='run_D3', wide='wide_D21', mixed='mixed_3_2', quant='quant_3_1_2', seg='seg_all', mseg='mseg_all')


def digest(ret):
    """sha256 over the bytes of records, cand, l and g (lists: the segmented
    stages' per-problem arrays, in order)."""
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, (list, tuple)):
            for y in x:
                feed(y)
        else:
            h.update(np.ascontiguousarray(x).tobytes())
    feed(ret)
    return h.hexdigest()


def gpu_engine():
    import torch
    from hyperopt_amd.engine import get_engine
    return get_engine(torch.device('cuda', 0))


def capture_gpu(names=None):
    eng = gpu_engine()
    cases = gpu_cases()
    return dict((name, digest(cases[name](eng))) for name in (names or cases))


if __name__ == '__main__':
    mode, path = sys.argv[1], sys.argv[2]
    doc = json.load(open(path)) if os.path.exists(path) else {}
    commit = subprocess.check_output(['git', 'rev-parse', 'HEAD']).decode().strip() if os.path.isdir('.git') else None
    doc[mode] = dict(commit=commit or doc.get('host', {}).get('commit'),
                     data=capture_host() if mode == 'host' else capture_gpu())
    with open(path, 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write('\n')
