"""Joint TPE (DESIGN.md "Joint TPE"), the parts that need no GPU: the host rows
against the numpy restatement of the model (tests/joint_ref.py), the argument
checks tpe_joint_run makes before any launch, the public interface's own
argument checks, and the unchanged default path."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
LOG2E = 1.0 / np.log(2.0)


# ------------------------------------------------------------------ host rows
@pytest.mark.parametrize('D,n', [(1, 0), (2, 1), (3, 2), (3, 25), (4, 26), (5, 90)])
def test_side_mixture_matches_the_restated_model(D, n):
    """Weights (prior first, the forgetting ramp from 26 trials on), per-trial
    sigmas and means of a side equal the numpy restatement bit for bit."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(100 * D + n)
    pmu, psig = rs.uniform(-1, 1, D), rs.uniform(2, 20, D)
    X = rs.uniform(-5, 5, (n, D))
    w, mu, sigma = J.side_mixture(X, list(zip(pmu, psig)), 1.0)
    rw, rmu, rsig = R.ref_side(X, pmu, psig, 1.0)
    assert w.shape == (n + 1,) and mu.shape == sigma.shape == (n + 1, D)
    np.testing.assert_array_equal(w, rw)
    np.testing.assert_array_equal(mu, rmu)
    np.testing.assert_array_equal(sigma, rsig)
    assert abs(w.sum() - 1.0) < 1e-15 and (sigma[0] == psig).all() and (mu[0] == pmu).all()


def test_repeated_values_take_the_stable_tie_order():
    """Equal values sort in tid order: the later of two equal observations sits
    right of the earlier one, so their gaps differ as the stable order says."""
    from hyperopt_amd import joint as J
    x = np.array([3.0, -2.0, 3.0, 0.5, -2.0, 3.0, 7.0, 0.5])
    got = J.trial_sigmas(x, 0.25, 10.0)
    np.testing.assert_array_equal(got, R.ref_sigmas(x, 0.25, 10.0))
    # by hand, sorted with the prior (P = 0.25): -2a -2b P .5a .5b 3a 3b 3c 7; clip to [10/10, 10]
    want = {0: 2.5, 2: 1.0, 5: 4.0, 1: 1.0, 4: 2.25, 3: 1.0, 7: 2.5, 6: 4.0}
    for i, s in want.items():
        assert got[i] == s, (i, got[i], s)


@pytest.mark.parametrize('n', [2, 30, 200])
def test_unpermuted_rows_equal_the_univariate_fit(n):
    """On a tie-free column the side's (w, mu, sigma), sorted by mu with the
    prior at its searchsorted place, are parzen.fit_parzen_numpy's.  mu and sigma
    bit for bit; w to 1e-14 (the two normalise by the same n + 1 weights summed
    in a different order: at most a few ulp of the sum)."""
    from hyperopt_amd import joint as J, parzen
    rs = np.random.RandomState(n)
    x = rs.normal(0.5, 3.0, n)
    w, mu, sigma = J.side_mixture(x[:, None], [(0.5, 3.0)], 1.0)
    fw, fmu, fsig = parzen.fit_parzen_numpy(x, 1.0, 0.5, 3.0)
    order = np.argsort(x)
    pos = int(np.searchsorted(x[order], 0.5))
    perm = np.concatenate([1 + order[:pos], [0], 1 + order[pos:]])
    np.testing.assert_array_equal(mu[perm, 0], fmu)
    np.testing.assert_array_equal(sigma[perm, 0], fsig)
    np.testing.assert_allclose(w[perm], fw, rtol=1e-14, atol=0)


def test_density_and_sampler_rows():
    """mu, a = sqrt(log2e / 2) / sigma, c = log2 of w / prod(sigma sqrt(2 pi)
    mass) shifted to max 0 with the shift as the natural-log base; sampler rows
    {mu, sigma, fa, fb, flip} with the mirrored interval and cum = cumsum(w)."""
    from hyperopt_amd import joint as J
    below, above, low, high, _, _ = R.seeded_case(4, 80, 5)
    for w, mu, sigma in (below, above):
        m32, a32, c32, base = J.density_rows(w, mu, sigma, low, high)
        assert m32.dtype == a32.dtype == c32.dtype == np.float32
        np.testing.assert_array_equal(m32, mu.astype(np.float32))
        np.testing.assert_array_equal(a32, (np.sqrt(0.5 * LOG2E) / sigma).astype(np.float32))
        c = R.ref_logcoef(w, mu, sigma, low, high) * LOG2E
        assert c32.max() == 0.0
        assert abs(base - c.max() * np.log(2.0)) <= 1e-12 * max(1.0, abs(base))
        # (f32 rounding of values of magnitude <= 2^7: 2^-17 absolute)
        np.testing.assert_allclose(c32, c - c.max(), rtol=0, atol=2.0 ** -17)
        # the masses: 1 in the unbounded dimensions, Phi differences in the bounded ones
        mass = np.exp(-(R.ref_logcoef(w, mu, sigma, low, high) - np.log(w)
                        + np.sum(np.log(sigma * np.sqrt(2 * np.pi)), axis=1)))
        assert np.all(mass > 0) and np.all(mass <= 1.0 + 1e-12)
    w, mu, sigma = below
    cum, rows = J.sampler_rows(w, mu, sigma, low, high)
    assert cum.dtype == np.float64 and rows.dtype == np.float32 and rows.shape == (len(w), 4, 5)
    np.testing.assert_allclose(cum, np.cumsum(w), rtol=1e-15)
    assert cum[-1] == 1.0
    za, zb = (low[None, :] - mu) / sigma, (high[None, :] - mu) / sigma
    flip = za > 0
    np.testing.assert_array_equal(rows[:, :, 4] != 0, flip)
    from scipy.special import ndtr
    fa = np.where(flip, ndtr(-zb), ndtr(za))
    fb = np.where(flip, ndtr(-za), ndtr(zb))
    np.testing.assert_allclose(rows[:, :, 2], fa, rtol=1e-6, atol=1e-37)
    np.testing.assert_allclose(rows[:, :, 3], fb, rtol=1e-6)
    assert (rows[:, 1::2, 2] == 0).all() and (rows[:, 1::2, 3] == 1).all()       # unbounded dimensions


def test_lpdf_numpy_matches_the_restated_model():
    from hyperopt_amd import joint as J
    below, above, low, high, _, _ = R.seeded_case(3, 60, 9)
    z = np.random.RandomState(1).uniform(-9, 9, (257, 3))
    for side in (below, above):
        np.testing.assert_allclose(J.lpdf_numpy(z, side[0], side[1], side[2], low, high),
                                   R.ref_lpdf(z, side, low, high), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------ ABI
def test_joint_records_match_c():
    lines = ['printf("TPE_JOINT_MAX_DIMS %d\\nTPE_JOINT_CHUNK %d\\nTPE_JOINT_INJECT %d\\nTPE_ABI_VERSION %d\\n", '
             'TPE_JOINT_MAX_DIMS, TPE_JOINT_CHUNK, TPE_JOINT_INJECT, TPE_ABI_VERSION);',
             'printf("TPE_JOINT_STREAM %u\\n", TPE_JOINT_STREAM);',
             'printf("tpe_joint_record %zu\\ntpe_joint_args %zu\\n", sizeof(tpe_joint_record), sizeof(tpe_joint_args));']
    for f in N.JOINT_RECORD_DTYPE.names:
        lines.append('printf("tpe_joint_record.%s %%zu\\n", offsetof(tpe_joint_record, %s));' % (f, f))
    for f, _ in N.JointArgs._fields_:
        lines.append('printf("tpe_joint_args.%s %%zu\\n", offsetof(tpe_joint_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'j.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'j')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_JOINT_MAX_DIMS'] == N.JOINT_MAX_DIMS == 16
    assert lay['TPE_JOINT_CHUNK'] == N.JOINT_CHUNK
    assert lay['TPE_JOINT_INJECT'] == N.JOINT_INJECT
    assert lay['TPE_JOINT_STREAM'] == N.JOINT_STREAM and N.JOINT_STREAM > 2 ** 31 - 1    # no int32 label index
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_record'] == N.JOINT_RECORD_DTYPE.itemsize
    assert lay['tpe_joint_args'] == ctypes.sizeof(N.JointArgs)
    for f in N.JOINT_RECORD_DTYPE.names:
        assert N.JOINT_RECORD_DTYPE.fields[f][1] == lay['tpe_joint_record.' + f], f
    for f, _ in N.JointArgs._fields_:
        assert getattr(N.JointArgs, f).offset == lay['tpe_joint_args.' + f], f


def test_library_exports_the_joint_symbols():
    lib = N.load()
    for name in ('tpe_joint_scratch_bytes', 'tpe_joint_run', 'tpe_joint_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointArgs()
    a.n_dims, a.n_cand, a.n_ids, a.flags = 3, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids'):
        setattr(a, f, arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, scratch_bytes=0):
    """tpe_joint_run with NO usable scratch unless asked: the scratch check is
    the last one, so every earlier rejection is reached and a call that were
    wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_run(ctypes.byref(a) if a is not None else None, p if records else None, None, None, None,
                             p if scratch_bytes else None, scratch_bytes, None)


def test_null_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert b'null args' in lib.tpe_last_error()


@pytest.mark.parametrize('over,msg', [
    (dict(n_dims=0), b'n_dims outside'), (dict(n_dims=17), b'n_dims outside'), (dict(n_dims=-1), b'n_dims outside'),
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids'),
])
def test_bad_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_null_records_and_small_scratch_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep), keep, records=False) == -1
    assert b'null ids / records' in lib.tpe_last_error()
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_scratch_bytes(1, 2048, ctypes.byref(need)) == 0
    assert need.value == 2 * N.JOINT_RECORD_DTYPE.itemsize
    assert _run(lib, _host_args(keep), keep) == -1                       # no scratch at all
    assert b'scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()


def test_scratch_bytes():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    for n_ids, C, chunks in ((1, 1, 1), (1, 1024, 1), (1, 1025, 2), (3, 4097, 5), (2, 1 << 20, 1024)):
        assert lib.tpe_joint_scratch_bytes(n_ids, C, ctypes.byref(nb)) == 0
        assert nb.value == n_ids * chunks * 152
    assert lib.tpe_joint_scratch_bytes(0, 8, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_scratch_bytes(1, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_scratch_bytes(1, 8, None) == -1


def test_joint_profile_has_nothing_to_read_before_a_profiled_call():
    lib = N.load()
    ms = (ctypes.c_double * 2)()
    assert lib.tpe_joint_profile(0, ms) == -1
    assert b'tpe_joint_profile' in lib.tpe_last_error()
    assert lib.tpe_joint_profile(0, None) == 0


# ------------------------------------------------------- the public interface
def _space(n_cont=3):
    from hyperopt_amd import base, hp
    s = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
         'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, {'k': hp.uniform('inner', 0, 1)}])}
    for i in range(n_cont - 3):
        s['u%d' % i] = hp.lognormal('u%d' % i, 0, 1)
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
    for name in ('tpe_joint_run', 'tpe_run_batch', 'tpe_level_run', 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


@pytest.mark.parametrize('kw,match', [
    (dict(joint=['x', 'nope']), "'nope'"),
    (dict(joint=['x', 'q']), "'q'"),
    (dict(joint=['x', 'c']), "'c'"),
    (dict(joint=['x', 'inner']), "'inner'"),
    (dict(joint=['x']), 'at least 2'),
    (dict(joint=[]), 'at least 2'),
    (dict(joint=True, sampler='replay'), 'replay'),
    (dict(joint=True, precision='fp64'), 'fp64'),
    (dict(joint=True, shard=(0, 2)), 'shard'),
    (dict(joint=True, shard_ids=(0, 2)), 'shard'),
    (dict(joint=True, shard_labels=(0, 2)), 'shard'),
    (dict(joint=True, shard_grid=(0, 2)), 'shard'),
])
def test_joint_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = _space()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


def test_joint_true_needs_two_eligible_labels_and_at_most_sixteen(no_device):
    from hyperopt_amd import base, hp, tpe
    one = base.Domain(lambda d: 0.0, {'x': hp.uniform('x', 0, 1), 'q': hp.quniform('q', 0, 10, 1)})
    with pytest.raises(ValueError, match='at least 2'):
        tpe.suggest([0], one, base.Trials(), 1, joint=True)
    big = _space(17)
    with pytest.raises(ValueError, match=r'TPE_JOINT_MAX_DIMS = 16.*joint=\[') as e:
        tpe.suggest([0], big, base.Trials(), 1, joint=True)
    assert '17' in str(e.value)
    with pytest.raises(ValueError, match='TPE_JOINT_MAX_DIMS = 16'):
        tpe.suggest([0], big, base.Trials(), 1, joint=[r.label for r in big.table.rows if r.dist != 'quniform'
                                                       and r.label not in ('c', 'inner')])


def test_startup_path_and_default_are_unchanged(golden, no_device):
    """Below n_startup_jobs a suggest is rand.suggest, with or without joint;
    without joint the document is the recorded one byte for byte."""
    import json
    from hyperopt_amd import base, rand, tpe
    g = golden('joint_startup_suggest.json')
    d = _space()
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
    got = tpe.suggest([5, 6], d, trials, g['seed'])
    assert plain(got) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=False)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=['x', 'y'])) == g['vals']
