"""The wide float64 joint stage without a GPU: the keyword's ValueErrors and routing, the entry's TPE_E_ARGs, the rows"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R


def _space(n, extra=None):
    from hyperopt_amd import hp
    more = {'disc': dict(c=hp.choice('c', [0, 1, 2])), 'quant': dict(q=hp.quniform('q', 0, 10, 1)),
            'branch': dict(g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                             {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}])), None: {}}
    return dict(dict(('w%02d' % i, hp.uniform('w%02d' % i, 0, 1)) for i in range(n)), **more[extra])


WIDE = dict(joint=True, joint_wide=True, joint_precision='fp64', joint_precision_wide=True)


@pytest.mark.parametrize('n,extra,kw,match', [
    (17, None, dict(joint_precision='fp32'), "joint_precision_wide=True needs joint_precision='fp64'"),
    (17, None, dict(joint_wide=False), 'joint_precision_wide=True needs joint_wide=True'),
    (17, 'disc', dict(joint_discrete=True, joint_wide_mixed=True), 'discrete or quantised.*score in fp32 only'),
    (17, 'quant', dict(joint_quantized=True, joint_wide_quantized=True), 'discrete or quantised.*score in fp32 only'),
    (65, None, dict(), 'at most TPE_JOINT_WIDE_MAX_DIMS = 64 labels, not 65'),
    (17, 'branch', dict(joint_branches=True), 'branch groups.*segmented joint stage'),
    (17, None, dict(joint_shard=(0, 2)), 'joint_shard: the sharded joint stage'),
    (17, None, dict(joint_liar=True), 'joint_liar: the batch-aware liar stage'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(n, extra, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **k: pytest.fail('a startup draw was made'))
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    domain = base.Domain(lambda d: 0.0, _space(n, extra))
    kw = dict(WIDE, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, **kw)
    assert 'joint_precision_wide' not in tpe.joint_candidate_report.__code__.co_varnames


@pytest.mark.parametrize('n,entry', [(16, 'run_joint'), (17, 'run_joint_wide')])
def test_the_keyword_routes_by_group_width(n, entry, monkeypatch):
    from hyperopt_amd import base, history, rand, tpe
    domain, trials = base.Domain(lambda d: 0.0, _space(n)), base.Trials()
    for tid in range(25):
        docs = rand.suggest([tid], domain, trials, tid)
        docs[0]['state'], docs[0]['result'] = base.JOB_STATE_DONE, {'status': 'ok', 'loss': float(tid % 7)}
        trials.insert_trial_docs(docs)
    trials.refresh()
    hist, calls, ids = history.extract(domain, trials), [], [25, 26]

    class Eng(object):
        def __getattr__(self, name):
            def run(*a, **k):
                calls.append((name, k))
                rec = np.zeros(len(ids), dtype=N.JOINT_WIDE_RECORD_DTYPE if n > 16 else N.JOINT_RECORD_DTYPE)
                rec['z'][:, :n] = 0.5
                return rec
            return run

    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: Eng())
    monkeypatch.setattr(tpe, '_suggest_local', lambda table, *a, **k: tpe.ChoiceColumns(
        table.labels, np.zeros((len(ids), n)), np.ones((len(ids), n), dtype=bool)))
    out = tpe.suggest_choices(domain.table, hist, ids, 7, **WIDE)
    assert calls == [(entry, {'precision': 'fp64'})] and all(v == 0.5 for v in out[0].values())


def _host_args(keep, **over):               # (over host arrays: only for calls that return before any launch)
    a, arr = N.JointWideF64Args(), np.zeros(256)
    keep.append(arr)
    a.n_dims, a.n_cand, a.n_ids, a.k_below, a.k_above = 20, 5000, 2, 4, 33
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids'):
        setattr(a, f, arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('over,msg', [
    (dict(below_mu=None), 'null density rows'), (dict(above_c=None), 'null density rows'),
    (dict(n_dims=0), 'n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]'),
    (dict(n_dims=65), 'n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]'),
    (dict(n_cand=0), 'n_cand < 1'), (dict(k_above=0), 'k_below < 1 or k_above < 1'),
    (dict(flags=N.JOINT_INJECT), 'TPE_JOINT_INJECT without candidates'), (dict(scratch_bytes=-1), 'scratch too small'),
    (dict(centre=19), 'centre not finite'),
])
def test_bad_arguments_are_rejected_before_any_launch(over, msg):
    lib, keep, nb, wide = N.load(), [], ctypes.c_uint64(0), ctypes.c_uint64(0)
    short, bad = over.pop('scratch_bytes', 0), over.pop('centre', None)
    a = _host_args(keep, **over)
    if bad is not None:
        a.centre[bad] = np.inf
    # the documented sum: the wide stage's scratch up to a multiple of 16, then both sides' column blocks of psi
    assert lib.tpe_joint_wide_f64_scratch_bytes(2, 5000, 20, 4, 33, ctypes.byref(nb)) == 0
    assert lib.tpe_joint_wide_scratch_bytes(2, 5000, 20, ctypes.byref(wide)) == 0
    assert wide.value == 2 * 10 * N.JOINT_WIDE_RECORD_DTYPE.itemsize + 2 * 20 * 256 * 20 * 4
    assert nb.value == (wide.value + 15) // 16 * 16 + (1 + 3) * (20 // 2 + 1) * 512
    out = np.zeros(1 << 12, dtype=np.uint8)
    p = out.ctypes.data + (-out.ctypes.data) % 16
    assert lib.tpe_joint_wide_f64_run(ctypes.byref(a), p, None, None, None, p, nb.value + short, None) == -1
    assert lib.tpe_last_error().decode() == 'tpe_joint_wide_f64_run: ' + msg


def test_packed_rows_are_the_wide_rows_before_their_rounding():
    from hyperopt_amd import joint_pack as JP
    below, above, low, high, pmu, psig = R.seeded_case(21, 120, 3)
    r, r32 = (JP.group_rows(below, above, low, high, entry=e) for e in ('wide_f64', 'wide'))
    for key in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c'):
        assert r[key].dtype == np.float64 and r32[key].tobytes() == r[key].astype(np.float32).tobytes()
    assert r['below_mu'].tobytes() == below[1].tobytes() and r['below_base'] == r32['below_base']
    assert r['samp'].tobytes() == r32['samp'].tobytes() and r['cum'].tobytes() == r32['cum'].tobytes()
    assert (r['centre'] == np.where(np.isfinite(low), 0.0, pmu)).all()
    assert JP.group_rows(*R.seeded_case(64, 30, 1)[:4], entry='wide_f64')['Dc'] == 64
    assert JP.group_rows(*R.seeded_case(1, 30, 1)[:4], entry='wide_f64')['Dc'] == 1
    for entry, top in (('wide_f64', 64), ('f64', 16)):
        with pytest.raises(ValueError, match='%d dimensions, at most %d' % (top + 1, top)):
            JP.group_rows(*R.seeded_case(top + 1, 30, 1)[:4], entry=entry)
