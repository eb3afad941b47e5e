"""The float64 joint stage without a GPU: the keyword's and the engine's ValueErrors, the entry's TPE_E_ARGs, the rows."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R


def _spaces():
    from hyperopt_amd import hp
    cont = {'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 2), 'lr': hp.loguniform('lr', -5, 0)}
    branch = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                          {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}]))
    return {'cont': cont, 'disc': dict(cont, c=hp.choice('c', [0, 1, 2])), 'quant': dict(cont, q=hp.quniform('q', 0, 10, 1)),
            'branch': branch, 'wide': dict(('w%02d' % i, hp.uniform('w%02d' % i, 0, 1)) for i in range(17))}


@pytest.mark.parametrize('space,kw,match', [
    ('cont', dict(), 'needs joint=True'),
    ('cont', dict(joint=True, joint_precision='fp16'), "must be 'fp32' or 'fp64'"),
    ('disc', dict(joint=True, joint_discrete=True), 'discrete or quantised.*mixed and quantised joint stages'),
    ('quant', dict(joint=True, joint_quantized=True), 'discrete or quantised.*mixed and quantised joint stages'),
    ('wide', dict(joint=True, joint_wide=True), 'at most 16 labels, not 17: the wide joint stage'),
    ('branch', dict(joint=True, joint_branches=True), 'branch groups.*segmented joint stage'),
    ('branch', dict(joint=['a', 'b'], joint_branches=True), 'branch groups.*segmented joint stage'),
    ('cont', dict(joint=True, joint_shard=(0, 2)), 'joint_shard: the sharded joint stage'),
    ('cont', dict(joint=True, joint_liar=True), 'joint_liar: the batch-aware liar stage'),
    ('cont', dict(joint=True, joint_precision='fp32', precision='fp64'), 'the joint stage scores in fp32'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(space, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **k: pytest.fail('a startup draw was made'))
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    domain = base.Domain(lambda d: 0.0, _spaces()[space])
    kw = dict(dict(joint_precision='fp64'), **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, **kw)
    assert 'joint_precision' not in tpe.joint_candidate_report.__code__.co_varnames


@pytest.mark.parametrize('kw,match', [(dict(report_k=4), 'report_k'), (dict(shard=(0, 100)), 'shard'),
                                      (dict(liar=True), 'liar'), (dict(precision='fp16'), "'fp32' or 'fp64'")])
def test_engine_rejects_what_the_float64_stage_does_not_take(kw, match, monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    below, above, low, high, _, _ = R.seeded_case(2, 30, 1)
    with pytest.raises(ValueError, match=match):
        Engine.__new__(Engine).run_joint(below, above, low, high, [0], 8, 1, **dict(dict(precision='fp64'), **kw))


def _host_args(keep, **over):               # (over host arrays: only for calls that return before any launch)
    a, arr = N.JointF64Args(), np.zeros(64)
    keep.append(arr)
    a.n_dims, a.n_cand, a.n_ids, a.k_below, a.k_above = 3, 5000, 2, 4, 9
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids'):
        setattr(a, f, arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('over,msg', [
    (dict(below_mu=None), 'null density rows'), (dict(above_c=None), 'null density rows'),
    (dict(n_dims=0), 'n_dims outside [1, TPE_JOINT_MAX_DIMS]'), (dict(n_dims=17), 'n_dims outside [1, TPE_JOINT_MAX_DIMS]'),
    (dict(n_cand=0), 'n_cand < 1'), (dict(k_above=0), 'k_below < 1 or k_above < 1'),
    (dict(flags=N.JOINT_INJECT), 'TPE_JOINT_INJECT without candidates'), (dict(scratch_bytes=-1), 'scratch too small'),
])
def test_bad_arguments_are_rejected_before_any_launch(over, msg):
    lib, keep, nb = N.load(), [], ctypes.c_uint64(0)
    short = over.pop('scratch_bytes', 0)
    a, out = _host_args(keep, **over), np.zeros(1 << 12, dtype=np.uint8)
    assert lib.tpe_joint_f64_scratch_bytes(2, 5000, ctypes.byref(nb)) == 0
    assert nb.value == 2 * 5 * N.JOINT_RECORD_DTYPE.itemsize
    p = out.ctypes.data
    assert lib.tpe_joint_f64_run(ctypes.byref(a), p, None, None, None, p, nb.value + short, None) == -1
    assert lib.tpe_last_error().decode() == 'tpe_joint_f64_run: ' + msg
    if short:                                    # ... and the size it names is enough: the checks pass, no device here
        a.centre[0] = np.nan
        assert lib.tpe_joint_f64_run(ctypes.byref(a), p, None, None, None, p, nb.value, None) == -1
        assert lib.tpe_last_error().decode() == 'tpe_joint_f64_run: centre not finite'


def test_packed_rows_are_the_header_formulas_in_float64():
    from hyperopt_amd import joint_pack as JP
    below, above, low, high, pmu, psig = R.seeded_case(5, 120, 3)
    r, r32 = JP.group_rows(below, above, low, high, entry='f64'), JP.group_rows(below, above, low, high, entry='run')
    for name, side in (('below', below), ('above', above)):
        w, mu, sigma = side
        c = R.ref_logcoef(w, mu, sigma, low, high) / np.log(2.0)
        assert r[name + '_mu'].dtype == np.float64 and r[name + '_mu'].tobytes() == mu.tobytes()
        np.testing.assert_allclose(r[name + '_a'], np.sqrt(np.log2(np.e) / 2) / sigma, rtol=1e-15, atol=0)
        np.testing.assert_allclose(r[name + '_c'], c - c.max(), rtol=0, atol=1e-12)
        assert r[name + '_c'].max() == 0.0 and abs(r[name + '_base'] - c.max() * np.log(2.0)) < 1e-12
        for f in ('_mu', '_a', '_c'):
            assert r32[name + f].dtype == np.float32 and r32[name + f].tobytes() == r[name + f].astype(np.float32).tobytes()
    up = dict((key, (buf, dt)) for key, _, buf, dt, _ in JP.group_rows_present(r))      # what the engine uploads
    assert all(up[s + f] == (s + f + '64', np.float64) for s in ('below', 'above') for f in ('_mu', '_a', '_c'))
    assert up['samp'] == ('samp', np.float32) and up == dict(up, **dict(
        (key, (buf, dt)) for key, _, buf, dt, _ in JP.group_rows_present(r32) if key in ('samp', 'cum')))
    assert (r['centre'] == np.where(np.isfinite(low), 0.0, pmu)).all()
    assert r['samp'].tobytes() == r32['samp'].tobytes() and r['cum'].tobytes() == r32['cum'].tobytes()
    with pytest.raises(ValueError, match='17 dimensions, at most 16'):
        JP.group_rows(*R.seeded_case(17, 30, 1)[:4], entry='f64')
