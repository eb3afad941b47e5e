"""The float64 segmented joint stage without a GPU: ValueErrors, routing, TPE_E_ARGs, scratch size, the blob's rows."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R

KW = dict(joint=True, joint_branches=True, joint_precision='fp64', joint_precision_branches=True)


def _space(kind='cont'):
    from hyperopt_amd import hp
    second = {'cont': {'u': hp.normal('u', 0, 1), 'v': hp.lognormal('v', 0, 1), 'w': hp.loguniform('w', -3, 1)},
              'disc': {'u': hp.normal('u', 0, 1), 'k': hp.choice('k', [0, 1, 2])},
              'quant': {'u': hp.normal('u', 0, 1), 'q': hp.quniform('q', 0, 10, 1)},
              'wide': dict(('w%02d' % i, hp.uniform('w%02d' % i, 0, 1)) for i in range(17))}[kind]
    return {'g': hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)}, second])}


@pytest.mark.parametrize('kind,kw,match', [
    ('cont', dict(joint_precision='fp32'), "joint_precision_branches=True needs joint_precision='fp64'.*scores in fp32"),
    ('cont', dict(joint_branches=False), 'joint_precision_branches=True needs joint_branches=True'),
    ('disc', dict(joint_discrete=True, joint_branches_mixed=True), 'discrete or quantised.*mixed segmented.*fp32 only'),
    ('quant', dict(joint_quantized=True, joint_branches_mixed=True), 'discrete or quantised.*mixed segmented.*fp32 only'),
    ('wide', dict(joint_wide=True, joint_branches_wide=True), 'at most 16 labels, not 17.*wide segmented.*fp32 only'),
    ('cont', dict(joint_shard=(0, 2)), 'joint_shard: the sharded joint stage'),
    ('cont', dict(joint_liar='branches'), 'joint_liar: the batch-aware liar stage'),
    ('cont', dict(joint_precision_branches=False), 'branch groups.*segmented joint stage scores in fp32 only'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(kind, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **k: pytest.fail('a startup draw was made'))
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    domain = base.Domain(lambda d: 0.0, _space(kind))
    kw = dict(KW, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, **kw)
    assert 'joint_precision_branches' not in tpe.joint_candidate_report.__code__.co_varnames


@pytest.mark.parametrize('gate,want', [(0, 1), (None, 0)])
def test_the_keyword_sends_the_branch_groups_through_one_float64_call(gate, want, monkeypatch):
    """A space whose only groups are branch groups; gate None: no id takes a branch with a group."""
    from hyperopt_amd import base, history, hp, rand, tpe
    space = _space() if gate is not None else {'g': hp.choice('g', [{'a': hp.uniform('a', 0, 1),
                                                                    'b': hp.uniform('b', 0, 1)}, {'c': 1}])}
    domain, trials = base.Domain(lambda d: 0.0, space), base.Trials()
    for tid in range(25):
        docs = rand.suggest([tid], domain, trials, tid)
        docs[0]['state'], docs[0]['result'] = base.JOB_STATE_DONE, {'status': 'ok', 'loss': float(tid % 7)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    hist, calls, ids, labels = history.extract(domain, trials), [], [25, 26], domain.table.labels

    class Eng(object):
        def __getattr__(self, name):
            def run(models, words, prob_seg, prob_id, *a, **k):
                calls.append((name, list(prob_id), k))
                rec = np.zeros(len(prob_seg), dtype=N.JOINT_RECORD_DTYPE)
                rec['z'][:, :2] = 0.5
                return rec
            return run

    values, active = np.zeros((2, len(labels))), np.zeros((2, len(labels)), dtype=bool)
    for i, name in enumerate(labels):
        active[:, i] = name == 'g' or (gate == 0 and name in ('a', 'b'))
    values[:, labels.index('g')] = 0 if gate == 0 else 1
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: Eng())
    monkeypatch.setattr(tpe, '_suggest_local', lambda table, *a, **k: tpe.ChoiceColumns(table.labels, values, active))
    out = tpe.suggest_choices(domain.table, hist, ids, 7, **KW)
    assert calls == [('run_joint_segments', ids, {'precision': 'fp64'})][:want]
    assert all(o['a'] == o['b'] == 0.5 for o in out) if want else all(o['a'] is None for o in out)


@pytest.mark.parametrize('kw,match', [(dict(report_k=4), 'report_k'), (dict(shard=(0, 100)), 'shard'),
                                      (dict(precision='fp16'), "'fp32' or 'fp64'"), (dict(cats=True), 'discrete or quant')])
def test_engine_rejects_what_the_float64_stage_does_not_take(kw, match, monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    below, above, low, high, _, _ = R.seeded_case(2, 30, 1)
    model = (below, above, low, high)
    if kw.pop('cats', False):
        model += ([(np.zeros(len(below[0]), dtype=int), np.zeros(len(above[0]), dtype=int), [0.5, 0.5], 1.0, 1.0)],)
    with pytest.raises(ValueError, match=match):
        Engine.__new__(Engine).run_joint_segments([model], [1], [0], [5], 8, 1, **dict(dict(precision='fp64'), **kw))


def _blob(n_cand=5000, inject=None):
    from hyperopt_amd import joint_pack as JP
    groups = [R.seeded_case(3, 40, 1)[:4], R.seeded_case(16, 300, 2)[:4], R.seeded_case(5, 20, 3, n_below=0)[:4]]
    args = (groups, [7, 8, 9], [1, 0, 1], [5, 6, 2 ** 33], n_cand, inject)
    return groups, JP.segment_blob(*args, N.JOINT_SEG_F64_DTYPE), JP.segment_blob(*args, N.JOINT_SEG_DTYPE)


def _psi_bytes(segs):
    return sum(((g['k_below'] + 15) // 16 + (g['k_above'] + 15) // 16) * N.f64_steps(g['n_dims']) * 512 for g in segs)


def test_a_groups_rows_in_the_float64_blob_are_its_solo_float64_rows():
    from hyperopt_amd import joint_pack as JP
    groups, b, b32 = _blob()
    pool64 = b.blob[b.offs[1]:b.offs[2]].view(np.float64)
    pool32, pool32_f32 = (x.blob[x.offs[4]:x.offs[5]].view(np.float32) for x in (b, b32))
    assert b.n64 == len(pool64) and [N.f64_steps(D) for D in (1, 2, 3, 4, 5, 8, 12, 16)] == [1, 2, 2, 3, 4, 5, 7, 9]
    psi = 0
    for s, group in enumerate(groups):
        r, g, g32 = JP.group_rows(*group, entry='f64'), b.segs[s], b32.segs[s]
        for key, field, buf, dtype, _ in JP.group_rows_present(r):
            at, pool = int(g[field + '64' if buf.endswith('64') else field]), pool64 if dtype is np.float64 else pool32
            assert pool[at:at + r[key].size].tobytes() == np.ascontiguousarray(r[key], dtype=dtype).tobytes(), key
        assert (g['centre'][:r['Dc']] == r['centre']).all() and (g['centre'][r['Dc']:] == 0).all()
        assert g['psi'] == psi and g['below_base'] == r['below_base'] and g['stream_word'] == 7 + s
        psi += _psi_bytes([g]) // 8
        # the sampler's rows: byte for byte the fp32 segment's, as are the bounds
        n = r['samp'].size
        assert pool32[int(g['samp']):int(g['samp']) + n].tobytes() == \
            pool32_f32[int(g32['samp']):int(g32['samp']) + n].tobytes() == r['samp'].tobytes()
        assert g['lo'].tobytes() == g32['lo'].tobytes() and g['hi'].tobytes() == g32['hi'].tobytes()
    assert (b.cand_off == b32.cand_off).all() and (b.widths == b32.widths).all()


def _run(lib, b, C=5000, short=0, **over):      # (host arrays: these calls return before any launch)
    a, nb, good = N.JointSegF64Args(), ctypes.c_uint64(0), _blob(C)[1].segs
    assert lib.tpe_joint_seg_f64_scratch_bytes(good.ctypes.data, len(good), len(b.prob_seg), C, ctypes.byref(nb)) == 0
    out = np.zeros(nb.value + 64, dtype=np.uint8)
    a.n_segs, a.n_probs, a.n_cand, a.seed = len(b.segs), len(b.prob_seg), C, 3
    for name, off in zip(('segs', 'pool_f64', 'prob_id', 'cand_off', 'pool_f32', 'prob_seg'), b.offs):
        setattr(a, name, b.blob.ctypes.data + int(off))
    a.host_segs, a.host_prob_seg, a.pool_f32_len, a.pool_f64_len = b.segs.ctypes.data, b.prob_seg.ctypes.data, b.n32, b.n64
    for k, v in over.items():
        setattr(a, k, v)
    p = out.ctypes.data + (-out.ctypes.data) % 16
    rc = lib.tpe_joint_seg_f64_run(ctypes.byref(a), p, None, None, None, p, nb.value + short, None)
    return rc, lib.tpe_last_error().decode(), nb.value


@pytest.mark.parametrize('n_cand', [5000, 1])
def test_scratch_bytes_are_the_documented_sum(n_cand):
    lib, seg = N.load(), ctypes.c_uint64(0)
    _, b, _ = _blob(n_cand)
    assert lib.tpe_joint_seg_scratch_bytes(3, n_cand, ctypes.byref(seg)) == 0
    assert seg.value == 16 + 3 * ((n_cand + 1023) // 1024) * N.JOINT_RECORD_DTYPE.itemsize
    # k_below + k_above = 3 + 39, 6 + 296, 1 + 21 components at D = 3, 16, 5 (NI = 2, 9, 4)
    assert _psi_bytes(b.segs) == ((1 + 3) * 2 + (1 + 19) * 9 + (1 + 2) * 4) * 512
    assert _run(lib, b, n_cand, pool_f64=None)[2] == (seg.value + 15) // 16 * 16 + _psi_bytes(b.segs)
    b.segs[2]['k_below'] = 0                     # (a descriptor the run refuses has no size)
    assert lib.tpe_joint_seg_f64_scratch_bytes(b.segs.ctypes.data, 3, 3, n_cand, ctypes.byref(seg)) == -1


@pytest.mark.parametrize('over,seg,msg', [
    (dict(pool_f64=None), {}, 'null pool_f64'), (dict(pool_f64=None, flags=N.JOINT_INJECT), {}, 'null pool_f64'),
    (dict(pool_f32=None), {}, 'null pool'), (dict(n_probs=0), {}, 'n_probs < 1'), (dict(n_cand=0), {}, 'n_cand < 1'),
    (dict(segs=None), {}, 'null segs / host_segs'), (dict(prob_id=None), {}, 'null prob_seg / host_prob_seg / prob_id'),
    ({}, dict(n_dims=17), "a segment's n_dims outside [1, TPE_JOINT_MAX_DIMS]"),
    ({}, dict(k_above=0), "a segment's k_below < 1 or k_above < 1"),
    ({}, dict(above_mu64=1 << 40), "a segment's rows leave its pool"), ({}, dict(below_c64=-1), "a segment's rows leave its pool"),
    ({}, dict(samp=1 << 40), "a segment's rows leave its pool"),
    (dict(flags=N.JOINT_INJECT), {}, 'TPE_JOINT_INJECT without candidates'),
    ({}, dict(centre=np.inf), "a segment's centre not finite"), (dict(short=-1), {}, 'scratch too small'),
    ({}, dict(psi=1 << 40), "a segment's psi range leaves scratch"), ({}, dict(psi=-1), "a segment's psi range leaves scratch"),
    ({}, dict(psi=4 * 2 * 64 - 1), "a segment's psi range overlaps another segment's"),
])
def test_bad_arguments_are_rejected_before_any_launch(over, seg, msg):
    _, b, _ = _blob()
    for k, v in seg.items():                     # (segment 1: D = 16, behind segment 0's 4 column blocks of 2 steps)
        b.segs[1][k] = v
    assert _run(N.load(), b, **over)[:2] == (-1, 'tpe_joint_seg_f64_run: ' + msg)
