"""Mixed joint TPE groups (continuous and discrete labels, DESIGN.md "Joint
TPE"), the parts that need no GPU: the host rows against the numpy restatement
(tests/joint_mixed_ref.py), the struct layout, the argument checks
tpe_joint_mixed_run makes before any launch, and the public keyword
``joint_discrete`` with its own argument checks."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_mixed_ref as M
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
LOG2E = 1.0 / np.log(2.0)
US = [2, 3, 7, 17, '5p']


# ------------------------------------------------------------------ host rows
@pytest.mark.parametrize('n', [0, 1, 25, 26, 90])
def test_mixed_side_matches_the_restated_model(n):
    """Weights, continuous rows and the components' categories (row 0: -1) of a
    side equal the restatement bit for bit; the smoothing mass is
    prior_weight U / (n + 1)."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(n)
    pmu, psig = rs.uniform(-1, 1, 2), rs.uniform(2, 20, 2)
    X = rs.uniform(-5, 5, (n, 2))
    ps = [M.prior(u) for u in US]
    XC = np.stack([rs.choice(len(p), size=n, p=p) for p in ps], axis=1).reshape(n, len(ps))
    w, mu, sigma, xc = J.mixed_side_mixture(X, list(zip(pmu, psig)), XC, 1.0)
    rw, rmu, rsig, rxc = M.ref_mixed_side(X, pmu, psig, XC, 1.0)
    np.testing.assert_array_equal(w, rw)
    np.testing.assert_array_equal(mu, rmu)
    np.testing.assert_array_equal(sigma, rsig)
    np.testing.assert_array_equal(xc, rxc)
    assert xc.shape == (n + 1, len(ps)) and (xc[0] == -1).all() and (xc[1:] >= 0).all()
    for p in ps:
        for pw in (1.0, 0.5):
            assert J.smoothing(pw, len(p), n) == M.smoothing(len(p), n, pw) == pw * len(p) / (n + 1.0)
    # an all-discrete side: the same weights, no continuous columns
    w0, mu0, sig0, xc0 = J.mixed_side_mixture(np.zeros((n, 0)), [], XC, 1.0)
    np.testing.assert_array_equal(w0, rw)
    np.testing.assert_array_equal(w0, M.ref_mixed_side(None, [], [], XC, 1.0)[0])
    assert mu0.shape == sig0.shape == (n + 1, 0)
    np.testing.assert_array_equal(xc0, rxc)


@pytest.mark.parametrize('n', [0, 1, 25, 26, 90])
@pytest.mark.parametrize('u', US)
def test_float64_tables_reproduce_log2_P(n, u):
    """miss + bonus 1[v = x] (a trial's row) and miss + corr (row 0) are
    log2 P_kd(v) to 1e-12 for every (k, v), and every row of P sums to 1."""
    from hyperopt_amd import joint as J
    p = M.prior(u)
    U = len(p)
    rs = np.random.RandomState(7 * n + U)
    xc = np.concatenate([[-1], rs.choice(U, size=n, p=p)])
    for pw in (1.0, 0.25):
        s = J.smoothing(pw, U, n)
        P = M.ref_P(xc, p, s)
        np.testing.assert_allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        miss, bonus, corr = J.discrete_tables(p, s)
        assert miss.dtype == bonus.dtype == np.float64 and miss.shape == bonus.shape == (U,)
        hit = np.arange(U)[None, :] == xc[:, None]
        got = miss[None, :] + np.where(hit, bonus[None, :], 0.0) + np.where(xc[:, None] < 0, corr, 0.0)
        np.testing.assert_allclose(got, np.log2(P), rtol=0, atol=1e-12)
        # the device form's definitions
        np.testing.assert_allclose(miss, np.log2(s * p / (1 + s)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(bonus, np.log2(1 + 1 / (s * p)), rtol=0, atol=1e-12)
        assert abs(corr - np.log2((1 + s) / s)) <= 1e-12


@pytest.mark.parametrize('Dc,us,n', [(2, [3], 60), (0, [3, '5p'], 40), (3, [2, '5p', 17], 90)])
def test_mixed_density_and_sampler_rows(Dc, us, n):
    """The f32 rows: mu / a as the continuous stage's, c with the prior row's
    correction before the shift to max 0, cat the categories as floats, miss /
    bonus flat in dimension order; the sampler's cum / rows are the continuous
    stage's, h = 1 / (1 + s), cat_cum the priors' cumsums ending in 1."""
    from hyperopt_amd import joint as J
    below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, n)
    for side, s in ((below, sb), (above, sa)):
        w, mu, sigma, xc = side
        m32, a32, c32, base, cat32, miss, bonus = J.mixed_density_rows(w, mu, sigma, low, high, xc, ps, s)
        assert m32.dtype == a32.dtype == c32.dtype == cat32.dtype == miss.dtype == bonus.dtype == np.float32
        assert m32.shape == a32.shape == (len(w), Dc) and cat32.shape == (len(w), len(ps))
        np.testing.assert_array_equal(cat32, xc.astype(np.float32))
        lc = (R.ref_logcoef(w, mu, sigma, low, high) if Dc else np.log(w)) * LOG2E
        lc[0] += sum(np.log2((1 + sd) / sd) for sd in s)
        assert c32.max() == 0.0
        assert abs(base - lc.max() * np.log(2.0)) <= 1e-12 * max(1.0, abs(base))
        np.testing.assert_allclose(c32, lc - lc.max(), rtol=0, atol=2.0 ** -17)
        want_miss = np.concatenate([np.log2(sd * p / (1 + sd)) for p, sd in zip(ps, s)])
        want_bonus = np.concatenate([np.log2(1 + 1 / (sd * p)) for p, sd in zip(ps, s)])
        np.testing.assert_allclose(miss, want_miss, rtol=2.0 ** -23, atol=0)      # (one f32 rounding)
        np.testing.assert_allclose(bonus, want_bonus, rtol=2.0 ** -23, atol=0)
        if Dc:
            rm, ra, _, _ = J.density_rows(w, mu, sigma, low, high)
            np.testing.assert_array_equal(m32, rm)
            np.testing.assert_array_equal(a32, ra)
    w, mu, sigma, xc = below
    cum, rows, h, cat_cum = J.mixed_sampler_rows(w, mu, sigma, low, high, ps, sb)
    assert cum.dtype == h.dtype == cat_cum.dtype == np.float64 and rows.dtype == np.float32
    np.testing.assert_allclose(cum, np.cumsum(w), rtol=1e-15)
    assert cum[-1] == 1.0 and rows.shape == (len(w), Dc, 5)
    if Dc:
        c0, r0 = J.sampler_rows(w, mu, sigma, low, high)
        assert cum.tobytes() == c0.tobytes() and rows.tobytes() == r0.tobytes()
    np.testing.assert_array_equal(h, 1.0 / (1.0 + sb))
    off = 0
    for p in ps:
        seg = cat_cum[off:off + len(p)]
        np.testing.assert_allclose(seg, np.cumsum(p), rtol=0, atol=1e-15)
        assert seg[-1] == 1.0 and (np.diff(seg) > 0).all()
        off += len(p)
    assert off == len(cat_cum)


@pytest.mark.parametrize('Dc,us,n', [(3, [2, '5p', 17], 60), (0, [3, '5p'], 40), (1, [7], 0)])
def test_mixed_lpdf_numpy_matches_the_restated_model(Dc, us, n):
    from hyperopt_amd import joint as J
    below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, n)
    rs = np.random.RandomState(1)
    z = rs.uniform(-9, 9, (257, Dc))
    v = np.stack([rs.randint(len(p), size=257) for p in ps], axis=1)
    for side, s in ((below, sb), (above, sa)):
        got = J.mixed_lpdf_numpy(z, v, side[0], side[1], side[2], low, high, side[3], ps, s)
        np.testing.assert_allclose(got, M.ref_mixed_lpdf(z, v, side, low, high, ps, s), rtol=0, atol=1e-12)


def test_the_device_form_in_float64_is_the_model():
    """c (corrected) - sum_cont + sum_d bonus 1[v = x] summed over k, plus the
    candidate's sum_d miss, is the model's density: the algebra of the kernel,
    evaluated in float64 from the float64 tables."""
    from hyperopt_amd import joint as J
    below, _, low, high, _, _, ps, sb, _, _ = M.seeded_mixed_case(2, [3, '5p'], 60)
    w, mu, sigma, xc = below
    rs = np.random.RandomState(3)
    z = rs.uniform(-9, 9, (64, 2))
    v = np.stack([rs.randint(len(p), size=64) for p in ps], axis=1)
    c = R.ref_logcoef(w, mu, sigma, low, high) * LOG2E
    tabs = [J.discrete_tables(p, s) for p, s in zip(ps, sb)]
    for d, (_, _, corr) in enumerate(tabs):
        c = c + np.where(xc[:, d] < 0, corr, 0.0)
    t = c[None, :] - 0.5 * LOG2E * (((z[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2).sum(axis=2)
    Mv = np.zeros(64)
    for d, (miss, bonus, _) in enumerate(tabs):
        t = t + np.where(v[:, d, None] == xc[None, :, d], bonus[v[:, d]][:, None], 0.0)
        Mv += miss[v[:, d]]
    got = (np.log2(np.exp2(t - t.max(axis=1)[:, None]).sum(axis=1)) + t.max(axis=1) + Mv) * np.log(2.0)
    np.testing.assert_allclose(got, M.ref_mixed_lpdf(z, v, below, low, high, ps, sb), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------ ABI
def test_mixed_args_match_c():
    lines = ['printf("TPE_JOINT_MAX_CATS %d\\nTPE_JOINT_MAX_CAT_TOTAL %d\\nTPE_JOINT_MAX_DIMS %d\\nTPE_ABI_VERSION %d\\n", '
             'TPE_JOINT_MAX_CATS, TPE_JOINT_MAX_CAT_TOTAL, TPE_JOINT_MAX_DIMS, TPE_ABI_VERSION);',
             'printf("tpe_joint_mixed_args %zu\\ntpe_joint_record %zu\\n", sizeof(tpe_joint_mixed_args), '
             'sizeof(tpe_joint_record));']
    for f, _ in N.JointMixedArgs._fields_:
        lines.append('printf("tpe_joint_mixed_args.%s %%zu\\n", offsetof(tpe_joint_mixed_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'm.c')
        with open(c, 'w') as f:
            f.write(prog)
        exe = os.path.join(d, 'm')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_JOINT_MAX_CATS'] == N.JOINT_MAX_CATS == 256
    assert lay['TPE_JOINT_MAX_CAT_TOTAL'] == N.JOINT_MAX_CAT_TOTAL == 1024
    assert lay['TPE_JOINT_MAX_DIMS'] == N.JOINT_MAX_DIMS == 16
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_record'] == N.JOINT_RECORD_DTYPE.itemsize
    assert lay['tpe_joint_mixed_args'] == ctypes.sizeof(N.JointMixedArgs)
    for f, _ in N.JointMixedArgs._fields_:
        assert getattr(N.JointMixedArgs, f).offset == lay['tpe_joint_mixed_args.' + f], f
    # the fields of tpe_joint_args, at the same places (n_cat where `reserved` was)
    for f, _ in N.JointArgs._fields_:
        g = 'n_cat' if f == 'reserved' else f
        assert getattr(N.JointMixedArgs, g).offset == getattr(N.JointArgs, f).offset, f


def test_library_exports_the_mixed_symbol_at_abi_24():
    lib = N.load()
    assert 'tpe_joint_mixed_run' in N.EXPORTS and hasattr(lib, 'tpe_joint_mixed_run')
    assert lib.tpe_abi_version() == 24


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointMixedArgs()
    a.n_dims, a.n_cat, a.n_cand, a.n_ids, a.flags = 3, 2, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids',
              'below_cat', 'above_cat', 'below_miss', 'below_bonus', 'above_miss', 'above_bonus', 'below_h', 'cat_cum'):
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
    """tpe_joint_mixed_run with NO usable scratch unless asked: the scratch
    check is the last one, so every earlier rejection is reached and a call that
    were wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_mixed_run(ctypes.byref(a) if a is not None else None, p if records else None, None, None,
                                   None, p if scratch_bytes else None, scratch_bytes, None)


def test_null_mixed_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert b'null args' in lib.tpe_last_error()


@pytest.mark.parametrize('over,msg', [
    # everything tpe_joint_run checks
    (dict(n_dims=-1), b'n_dims + n_cat outside'), (dict(n_dims=17), b'n_dims + n_cat outside'),
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids'),
    # n_dims + n_cat outside [1, 16]; n_cat < 0
    (dict(n_dims=0, n_cat=0), b'n_dims + n_cat outside'), (dict(n_dims=15, n_cat=2), b'n_dims + n_cat outside'),
    (dict(n_dims=0, n_cat=17), b'n_dims + n_cat outside'), (dict(n_dims=16, n_cat=1), b'n_dims + n_cat outside'),
    (dict(n_cat=-1), b'n_cat < 0'), (dict(n_dims=4, n_cat=-2), b'n_cat < 0'),
    # a null table while n_cat > 0
    (dict(below_cat=None), b'null category tables'), (dict(above_cat=None), b'null category tables'),
    (dict(below_miss=None), b'null category tables'), (dict(below_bonus=None), b'null category tables'),
    (dict(above_miss=None), b'null category tables'), (dict(above_bonus=None), b'null category tables'),
    (dict(below_h=None), b'null category tables'), (dict(cat_cum=None), b'null category tables'),
    # a U_d outside [2, 256]
    (dict(cat_upper=[1, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'), (dict(cat_upper=[3, 0]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[257, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'), (dict(cat_upper=[3, -4]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    # more than 1024 categories in all
    (dict(n_cat=5, cat_upper=[256, 256, 256, 256, 2], cat_off=[0, 256, 512, 768, 1024]),
     b'more than TPE_JOINT_MAX_CAT_TOTAL'),
    # offsets that leave the tables
    (dict(cat_off=[0, 4]), b'cat_off outside'), (dict(cat_off=[-1, 3]), b'cat_off outside'),
])
def test_bad_mixed_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_accepted_mixed_arguments_reach_the_scratch_check():
    """Good arguments (an all-discrete group without mu / a / samp rows and the
    1024-category limit included) pass every check up to the last one."""
    lib, keep = N.load(), []
    for over in (dict(), dict(n_dims=0, below_mu=None, below_a=None, above_mu=None, above_a=None, samp=None),
                 dict(n_dims=12, n_cat=4, cat_upper=[256] * 4, cat_off=[0, 256, 512, 768]),
                 dict(n_dims=0, n_cat=16, cat_upper=[2] * 16, cat_off=list(range(0, 32, 2)))):
        assert _run(lib, _host_args(keep, **over), keep) == -1
        assert b'scratch too small' in lib.tpe_last_error(), (over, lib.tpe_last_error())
    assert _run(lib, _host_args(keep), keep, records=False) == -1
    assert b'null ids / records' in lib.tpe_last_error()
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_scratch_bytes(1, 2048, ctypes.byref(need)) == 0
    assert _run(lib, _host_args(keep), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    # n_cat = 0 is tpe_joint_run, with its checks and its messages
    assert _run(lib, _host_args(keep, n_cat=0), keep) == -1
    assert b'tpe_joint_run: scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, n_cat=0, below_mu=None), keep) == -1
    assert b'tpe_joint_run: null density rows' in lib.tpe_last_error()


# ------------------------------------------------------- the public interface
def _space(extra=None):
    from hyperopt_amd import base, hp
    s = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
         'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, {'k': hp.uniform('inner', 0, 1)}])}
    s.update(extra or {})
    return base.Domain(lambda d: 0.0, s)


def _wide_space():
    from hyperopt_amd import hp
    return _space({'leaf': hp.choice('leaf', ['a', 'b', 'c']), 'pc': hp.pchoice('pc', [(0.7, 0), (0.3, 1)]),
                   'zero': hp.pchoice('zero', [(0.5, 0), (0.0, 1), (0.5, 2)]),
                   'big': hp.choice('big', list(range(257))),
                   'one': hp.choice('one', ['adam']), 'one_p': hp.pchoice('one_p', [(1.0, 'relu')]),
                   'g2': hp.pchoice('g2', [(0.5, 0), (0.5, {'k': hp.choice('deep', [0, 1])})])})


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
    for name in ('tpe_joint_run', 'tpe_joint_mixed_run', 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def test_eligible_discrete():
    from hyperopt_amd import joint as J
    t = _wide_space().table
    want = {'leaf': True, 'pc': True, 'zero': False, 'big': False, 'c': False, 'g2': False, 'deep': False,
            'one': False, 'one_p': False, 'x': False, 'q': False, 'inner': False}
    for label, ok in want.items():
        assert J.eligible_discrete(t.by_label[label], t) is ok, label
    assert 'prior probability' in J.discrete_reason(t.by_label['zero'], t)
    assert '257' in J.discrete_reason(t.by_label['big'], t)
    assert 'fewer than 2' in J.discrete_reason(t.by_label['one'], t)
    assert 'fewer than 2' in J.discrete_reason(t.by_label['one_p'], t)
    assert 'gate' in J.discrete_reason(t.by_label['c'], t) and 'gate' in J.discrete_reason(t.by_label['g2'], t)
    assert 'conditional' in J.discrete_reason(t.by_label['deep'], t)
    assert 'quantised' in J.discrete_reason(t.by_label['q'], t)


@pytest.mark.parametrize('kw,match', [
    (dict(joint=['x', 'c'], joint_discrete=True), "'c'.*gate"),
    (dict(joint=['x', 'g2'], joint_discrete=True), "'g2'.*gate"),
    (dict(joint=['x', 'inner'], joint_discrete=True), "'inner'.*conditional"),
    (dict(joint=['leaf', 'deep'], joint_discrete=True), "'deep'.*conditional"),
    (dict(joint=['x', 'q'], joint_discrete=True), "'q'.*quantised"),
    (dict(joint=['x', 'zero'], joint_discrete=True), "'zero'.*prior probability"),
    (dict(joint=['x', 'big'], joint_discrete=True), "'big'.*257 categories"),
    (dict(joint=['x', 'one'], joint_discrete=True), "'one'.*fewer than 2"),
    (dict(joint=['leaf', 'one_p'], joint_discrete=True), "'one_p'.*fewer than 2"),
    (dict(joint=['x', 'nope'], joint_discrete=True), "'nope'"),
    (dict(joint=['leaf'], joint_discrete=True), 'at least 2'),
    (dict(joint_discrete=True), 'joint_discrete=True needs joint'),
    (dict(joint=False, joint_discrete=True), 'joint_discrete=True needs joint'),
    (dict(joint=None, joint_discrete=True), 'joint_discrete=True needs joint'),
    (dict(joint=True, joint_discrete=True, sampler='replay'), 'replay'),
    (dict(joint=True, joint_discrete=True, precision='fp64'), 'fp64'),
    (dict(joint=True, joint_discrete=True, shard=(0, 2)), 'shard'),
    # without the keyword a discrete label is refused as before
    (dict(joint=['x', 'c']), "'c'"),
    (dict(joint=['x', 'leaf']), "'leaf'"),
    (dict(joint=['x', 'leaf'], joint_discrete=False), "'leaf'"),
])
def test_joint_discrete_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = _wide_space()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


def test_the_group_of_joint_discrete(no_device):
    """joint=True joins the eligible continuous and discrete labels and skips
    gates, conditional, quantised, zero-prior, one-option and oversized labels; a list may
    name discrete labels alone; 17 labels or more than 1024 categories raise."""
    from hyperopt_amd import base, hp, tpe
    t = _wide_space().table
    none = (None, None, None, None)
    got = [r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none, True)]
    assert got == ['leaf', 'pc', 'x', 'y', 'z']                      # table order
    assert [r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none)] == ['x', 'y', 'z']
    assert [r.label for r in tpe._joint_group(t, ['pc', 'leaf'], 'philox', 'fp32', none, True)] == ['leaf', 'pc']
    many = base.Domain(lambda d: 0.0, dict(('c%02d' % i, hp.choice('c%02d' % i, [0, 1])) for i in range(17)))
    with pytest.raises(ValueError, match='TPE_JOINT_MAX_DIMS = 16'):
        tpe.suggest([0], many, base.Trials(), 1, joint=True, joint_discrete=True)
    fat = base.Domain(lambda d: 0.0, dict(('c%d' % i, hp.choice('c%d' % i, list(range(256)))) for i in range(5)))
    with pytest.raises(ValueError, match='TPE_JOINT_MAX_CAT_TOTAL = 1024.*1280'):
        tpe.suggest([0], fat, base.Trials(), 1, joint=True, joint_discrete=True)


def test_startup_path_is_unchanged_by_joint_discrete(golden, no_device):
    """Below n_startup_jobs a suggest is rand.suggest, whatever joint_discrete
    says: the recorded document byte for byte."""
    from hyperopt_amd import base, hp, rand, tpe
    g = golden('joint_startup_suggest.json')
    s = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
         'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, {'k': hp.uniform('inner', 0, 1)}])}
    d = base.Domain(lambda d: 0.0, s)
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
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True, joint_discrete=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=['x', 'y'], joint_discrete=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint_discrete=False)) == g['vals']
