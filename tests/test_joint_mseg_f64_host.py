"""The float64 mixed segmented joint stage without a GPU: ValueErrors, TPE_E_ARGs, the size functions, the blob's rows."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R

KW = dict(joint=True, joint_discrete=True, joint_quantized=True, joint_branches=True, joint_branches_mixed=True,
          joint_precision='fp64', joint_precision_branches=True, joint_precision_branches_mixed=True)


def _space(wide=False):
    from hyperopt_amd import hp
    second = (dict(('w%02d' % i, hp.uniform('w%02d' % i, 0, 1)) for i in range(17)) if wide
              else {'u': hp.normal('u', 0, 1), 'k': hp.choice('k', [0, 1, 2]), 'q': hp.quniform('q', 0, 10, 1)})
    return {'g': hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)}, second])}


@pytest.mark.parametrize('wide,kw,match', [
    (False, dict(joint_precision='fp32'), "joint_precision_branches_mixed=True needs joint_precision='fp64'"),
    (False, dict(joint_branches=False), 'joint_precision_branches_mixed=True needs joint_branches=True'),
    (False, dict(joint_precision_branches=False), 'joint_precision_branches_mixed=True needs joint_precision_branches=True'),
    (False, dict(joint_branches_mixed=False), 'joint_precision_branches_mixed=True needs joint_branches_mixed=True'),
    (False, dict(joint_discrete=False, joint_quantized=False),
     'joint_precision_branches_mixed=True needs joint_discrete=True or joint_quantized=True'),
    (False, dict(joint_shard=(0, 2)), 'joint_shard: the sharded joint stage'),
    (False, dict(joint_liar='branches_mixed'), 'joint_liar: the batch-aware liar stage'),
    (True, dict(joint_wide=True, joint_branches_wide=True), 'at most 16 labels, not 17'),
    (False, dict(joint_precision_branches_mixed=False), 'discrete or quantised.*mixed segmented.*fp32 only'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(wide, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **k: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **k: pytest.fail('a startup draw was made'))
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    domain = base.Domain(lambda d: 0.0, _space(wide))
    kw = dict(KW, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, **kw)
    assert 'joint_precision_branches_mixed' not in tpe.joint_candidate_report.__code__.co_varnames


def _mixed(Dc, us, Vs, na, nb, seed):
    """A group (below, above, low, high, cats, quants) on top of joint_ref.seeded_case's continuous part."""
    below, above, low, high = R.seeded_case(max(Dc, 1), na, seed, n_below=nb)[:4]
    rs, sides = np.random.RandomState(seed), []
    for w, mu, sigma in (below[:3], above[:3]):
        sides.append((w, np.asarray(mu)[:, :Dc], np.asarray(sigma)[:, :Dc]))
    col = [lambda K, u=u: np.concatenate([[-1], rs.randint(0, u, K - 1)]) for u in us]
    cats = [(c(len(below[0])), c(len(above[0])), np.full(u, 1.0 / u), 1.0, 1.5) for c, u in zip(col, us)]
    quants = [tuple(x for K in (len(below[0]), len(above[0])) for x in (rs.uniform(0, V - 1, K), rs.uniform(0.5, 2.0, K)))
              + (np.arange(V + 1) - 0.5,) for V in Vs]
    return sides[0], sides[1], low[:Dc], high[:Dc], cats, quants


def _blob(n_cand=5000, groups=None):
    from hyperopt_amd import joint_pack as JP
    groups = groups or [_mixed(3, (4,), (5, 7), 40, 3, 1), R.seeded_case(16, 300, 2)[:4], _mixed(0, (2,), (), 20, 0, 3),
                        _mixed(5, (), (6,), 33, 2, 4)]
    args = (groups, [7, 8, 9, 10][:len(groups)], [1, 0, 3, 2, 1][:len(groups) + 1], [5, 6, 2 ** 33, 8, 9][:len(groups) + 1],
            n_cand, None)
    return groups, JP.segment_blob(*args, N.JOINT_MSEG_F64_DTYPE), JP.segment_blob(*args, N.JOINT_MSEG_DTYPE)


def _psi_bytes(segs):
    return sum(((g['k_below'] + 15) // 16 + (g['k_above'] + 15) // 16)
               * N.mseg_f64_steps(g['n_dims'], g['n_cat'], g['n_quant']) * 512 for g in segs)


def _table_bytes(segs):
    return sum(((g['k_below'] + 15) // 16 + (g['k_above'] + 15) // 16) * 16 * int(g['quant_v'][:g['n_quant']].sum()) * 8
               for g in segs)


def test_a_groups_rows_in_the_blob_are_its_solo_float64_rows():
    from hyperopt_amd import joint_pack as JP
    groups, b, b32 = _blob()
    pool64 = b.blob[b.offs[1]:b.offs[2]].view(np.float64)
    pool32 = b.blob[b.offs[4]:b.offs[5]].view(np.float32)
    assert b.n64 == len(pool64) and b.n32 == len(pool32)
    assert [N.mseg_f64_steps(D, 1, 0) for D in (0, 1, 2, 3, 4, 5, 8)] == [1, 1, 2, 3, 3, 5, 5]
    psi = table = 0
    for s, group in enumerate(groups):
        mixed = len(group) == 6
        r, g, g32 = JP.group_rows(*group, entry='mq_f64' if mixed else 'f64'), b.segs[s], b32.segs[s]
        for key, field, buf, dtype, _ in JP.group_rows_present(r):
            name = field if field.endswith('64') or not buf.endswith('64') else field + '64'
            at, pool = int(g[name]), pool64 if dtype is np.float64 else pool32
            assert pool[at:at + r[key].size].tobytes() == np.ascontiguousarray(r[key], dtype=dtype).tobytes(), key
        assert (g['centre'][:r['Dc']] == r['centre']).all() and (g['centre'][r['Dc']:] == 0).all()
        assert g['psi'] == psi and g['below_base'] == r['below_base'] and g['stream_word'] == 7 + s
        assert (g['n_dims'], g['n_cat'], g['n_quant']) == (r['Dc'], r['Dk'], r['Dq'])
        psi += _psi_bytes([g]) // 8
        if r['Dq']:
            assert g['table64'] == table
            table += _table_bytes([g]) // 8
        # what the sampler reads: the fp32 mixed segment's bytes
        for f in ('lo', 'hi', 'qlo', 'qhi', 'cat_upper', 'cat_off', 'quant_v', 'quant_edge_off', 'n_edges'):
            assert g[f].tobytes() == g32[f].tobytes(), f
    assert (b.cand_off == b32.cand_off).all() and (b.widths == b32.widths).all() and b.n_table == table


@pytest.mark.parametrize('group,match', [
    (lambda: _mixed(9, (3,), (), 20, 2, 1), 'at most 8 continuous and 4 discrete'),
    (lambda: _mixed(2, (3,) * 5, (), 20, 2, 1), 'at most 8 continuous and 4 discrete'),
    (lambda: _mixed(2, (), (4,) * 5, 20, 2, 1), '5 quantised dimensions, at most 4'),
    (lambda: _mixed(2, (), (256, 256, 2), 20, 2, 1), '514 lattice values in the group, at most 512'),
    (lambda: R.seeded_case(17, 20, 1)[:4], '17 dimensions, at most 16'),
])
def test_engine_rejects_groups_beyond_the_mixed_segments_limits(group, match, monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **k: pytest.fail('the library was loaded'))
    with pytest.raises(ValueError, match=match):
        Engine.__new__(Engine).run_joint_msegments_f64([group()], [1], [0], [5], 8, 1)
    assert not {'report_k', 'shard'} & set(Engine.run_joint_msegments_f64.__code__.co_varnames)


def _run(lib, b, C=5000, short=0, table_short=0, **over):      # (host arrays: these calls return before any launch)
    a, nb, tb, good = N.JointMSegF64Args(), ctypes.c_uint64(0), ctypes.c_uint64(0), _blob(C)[1].segs
    assert lib.tpe_joint_mseg_f64_scratch_bytes(good.ctypes.data, len(good), len(b.prob_seg), C, ctypes.byref(nb)) == 0
    assert lib.tpe_joint_mseg_f64_table_bytes(good.ctypes.data, len(good), ctypes.byref(tb)) == 0
    out, tab = np.zeros(nb.value + 64, dtype=np.uint8), np.zeros(tb.value // 8 + 1)
    a.n_segs, a.n_probs, a.n_cand, a.seed = len(b.segs), len(b.prob_seg), C, 3
    for name, off in zip(('segs', 'pool_f64', 'prob_id', 'cand_off', 'pool_f32', 'prob_seg'), b.offs):
        setattr(a, name, b.blob.ctypes.data + int(off))
    a.host_segs, a.host_prob_seg, a.pool_f32_len, a.pool_f64_len = b.segs.ctypes.data, b.prob_seg.ctypes.data, b.n32, b.n64
    a.quant_table64, a.quant_table64_bytes = tab.ctypes.data, tb.value + table_short
    for k, v in over.items():
        setattr(a, k, v)
    p = out.ctypes.data + (-out.ctypes.data) % 16
    rc = lib.tpe_joint_mseg_f64_run(ctypes.byref(a), p, None, None, None, p, nb.value + short, None)
    return rc, lib.tpe_last_error().decode(), nb.value, tb.value


@pytest.mark.parametrize('n_cand', [5000, 1])
def test_scratch_and_table_bytes_are_the_documented_sums(n_cand):
    lib, seg = N.load(), ctypes.c_uint64(0)
    _, b, _ = _blob(n_cand)
    assert lib.tpe_joint_mseg_scratch_bytes(5, n_cand, ctypes.byref(seg)) == 0
    # K = 4 + 38 (D 3 + 1 + 2: DP 4, NI 3), 6 + 296 (16: NI 9), 1 + 21 (0 + 1: DP 1, NI 1), 3 + 32 (5 + 0 + 1: DP 8, NI 5)
    assert _psi_bytes(b.segs) == ((1 + 3) * 3 + (1 + 19) * 9 + (1 + 2) * 1 + (1 + 2) * 5) * 512
    assert _table_bytes(b.segs) == ((1 + 3) * 16 * 12 + (1 + 2) * 16 * 6) * 8 == 8 * b.n_table
    got = _run(lib, b, n_cand, pool_f64=None)
    assert got[2:] == ((seg.value + 15) // 16 * 16 + _psi_bytes(b.segs), _table_bytes(b.segs))
    nb = ctypes.c_uint64(0)
    for field, value in (('k_below', 0), ('n_quant', 5), ('n_cat', 5), ('n_dims', 9)):   # (a refused descriptor has no size)
        bad = b.segs.copy()
        bad[0][field] = value
        assert lib.tpe_joint_mseg_f64_scratch_bytes(bad.ctypes.data, 4, 5, n_cand, ctypes.byref(nb)) == -1, field
    for field, value in (('k_above', 0), ('n_quant', -1), ('quant_v', 257)):
        bad = b.segs.copy()
        bad[0][field] = value
        assert lib.tpe_joint_mseg_f64_table_bytes(bad.ctypes.data, 4, ctypes.byref(nb)) == -1, field
    assert lib.tpe_joint_mseg_f64_table_bytes(None, 4, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_mseg_f64_table_bytes(b.segs.ctypes.data, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_mseg_f64_scratch_bytes(b.segs.ctypes.data, 4, 0, n_cand, ctypes.byref(nb)) == -1


S = "a segment's "


@pytest.mark.parametrize('over,seg,msg', [
    (dict(pool_f64=None), {}, 'null pool_f64'), (dict(pool_f64=None, flags=N.JOINT_INJECT), {}, 'null pool_f64'),
    (dict(pool_f32=None), {}, 'null pool'), (dict(n_probs=0), {}, 'n_probs < 1'), (dict(n_cand=0), {}, 'n_cand < 1'),
    (dict(n_segs=40000), {}, 'more than 32767 segments'),
    (dict(segs=None), {}, 'null segs / host_segs'), (dict(prob_id=None), {}, 'null prob_seg / host_prob_seg / prob_id'),
    ({}, dict(n_cat=17), S + 'n_cat outside [0, TPE_JOINT_MAX_DIMS]'),
    ({}, dict(n_quant=5), S + 'n_quant outside [0, TPE_JOINT_MAX_QUANT]'),
    ({}, dict(n_dims=9), 'n_dims > 8 or n_cat > 4 in a segment with a discrete or quantised label'),
    ({}, dict(n_dims=-1), S + 'n_dims < 0'), ({}, dict(k_above=0), S + 'k_below < 1 or k_above < 1'),
    ({}, dict(cat_upper=1), 'categories of a label outside [2, TPE_JOINT_MAX_CATS]'),
    ({}, dict(cat_off=3), 'cat_off outside the tables'),
    ({}, dict(quant_v=257), 'lattice values of a label outside [2, TPE_JOINT_MAX_LATTICE]'),
    ({}, dict(quant_edge_off=9), 'quant_edge_off outside the edge array'),
    (dict(quant_table64=None), {}, 'null table workspace with a quantised segment'),
    ({}, dict(above_mu64=1 << 40), S + 'rows leave its pool'), ({}, dict(below_c64=-1), S + 'rows leave its pool'),
    ({}, dict(samp=1 << 40), S + 'rows leave its pool'), ({}, dict(above_cat=1 << 40), S + 'rows leave its pool'),
    ({}, dict(below_bonus64=1 << 40), S + 'rows leave its pool'), ({}, dict(above_qsigma=-1), S + 'rows leave its pool'),
    ({}, dict(quant_samp=1 << 40), S + 'rows leave its pool'), ({}, dict(cat_cum=1 << 40), S + 'rows leave its pool'),
    (dict(flags=N.JOINT_INJECT), {}, 'TPE_JOINT_INJECT without candidates'),
    ({}, dict(centre=np.inf), S + 'centre not finite'), (dict(short=-1), {}, 'scratch too small'),
    ({}, dict(psi=1 << 40), S + 'psi range leaves scratch'), ({}, dict(psi=-1), S + 'psi range leaves scratch'),
    ({}, dict(psi=1), S + "psi range overlaps another segment's"),
    ({}, dict(table64=-1), S + 'table leaves the table workspace'),
    (dict(table_short=-8), {}, S + 'table leaves the table workspace'),
    ({}, dict(table64=(1 + 2) * 16 * 6 - 1), S + "table overlaps another segment's"),
])
def test_bad_arguments_are_rejected_before_any_launch(over, seg, msg):
    _, b, _ = _blob()
    for k, v in seg.items():                     # (segment 0: 3 + 1 + 2 coordinates, the first psi and table range)
        b.segs[0][k] = v
    assert _run(N.load(), b, **over)[:2] == (-1, 'tpe_joint_mseg_f64_run: ' + msg)
