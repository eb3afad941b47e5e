"""Batch-aware joint suggests (DESIGN.md "Batch-aware joint suggests"), the
parts that need no GPU: the model's anchors in plain numpy (tests/joint_liar_ref),
the condition the GPU tests' inputs must meet, the package's own restatement,
the struct layouts, every ValueError of the public interface and the engine, and
every TPE_E_ARG tpe_joint_liar returns before any launch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_liar_ref as LR
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')

MAX_TIES = 8
B = 8
C = 4096
CASES = [(3, 60, 11), (2, 3013, 5), (16, 120, 7), (20, 200, 9)]


def _case(D, n, seed):
    below, above, low, high, pmu, psig = R.seeded_case(D, n, seed)
    cand = LR.candidates(below, low, high, C, seed)
    z = cand.astype(np.float64)
    return below, above, low, high, psig, cand, R.ref_lpdf(z, below, low, high), R.ref_lpdf(z, above, low, high)


@pytest.fixture(scope='module')
def cases():
    return dict((c, _case(*c)) for c in CASES)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize('case', CASES[:1] + CASES[2:])
def test_extended_density_is_a_mixture_with_more_components(cases, case):
    """g_j = joint_ref.ref_lpdf of the above side extended by the liar rows with
    weights (w~, 1, .., 1) / (W + J), at every step of a greedy chain."""
    below, above, low, high, psig, cand, l, g = cases[case]
    chain = LR.Chain(above, psig, low, high)
    z = cand[:512].astype(np.float64)
    for j in range(4):
        gj = chain.log_g(z, g[:512])
        ext = R.ref_lpdf(z, chain.extended_side(above), low, high)
        np.testing.assert_allclose(gj, ext, rtol=0, atol=1e-10 * max(1.0, float(np.abs(ext).max())))
        w = chain.extended_side(above)[0]
        assert abs(w.sum() - 1.0) < 1e-12 and len(w) == len(above[0]) + j
        chain.add(cand[int(np.argmax(l[:512] - gj))])


def test_weight_sum_undoes_the_normalisation():
    for n in (0, 1, 25, 26, 300):
        w = R.ref_side(np.zeros((n, 1)), [0.0], [1.0])[0]
        W = LR.weight_sum(n)
        assert abs(w[0] * W - 1.0) < 1e-12
        if n:
            assert abs(w[-1] * W - 1.0) < 1e-12           # the newest trial weighs 1: what liar=True relies on


def test_no_liar_is_the_base_density(cases):
    below, above, low, high, psig, cand, l, g = cases[CASES[0]]
    chain = LR.Chain(above, psig, low, high)
    assert chain.log_g(cand.astype(np.float64), g).tobytes() == g.tobytes()
    steps = LR.greedy(chain, cand, l, g, 1)
    assert steps[0][3] == int(np.argmax(l - g))


@pytest.mark.parametrize('case', CASES)
def test_inputs_give_distinct_picks_and_small_tie_sets(cases, case):
    """A condition on the GPU tests' inputs, not a measurement: the reference
    alone picks 8 distinct candidates, with at most MAX_TIES near-ties a step;
    without liars every step is step 0."""
    below, above, low, high, psig, cand, l, g = cases[case]
    steps = LR.greedy(LR.Chain(above, psig, low, high), cand, l, g, B)
    picks = [s[3] for s in steps]
    print(case, picks, [len(s[1]) for s in steps])
    assert len(set(picks)) == B
    assert max(len(s[1]) for s in steps) <= MAX_TIES


def test_sigma_rule_at_the_edges():
    pts = np.array([[0.0], [1.0], [4.0]], dtype=np.float32)
    psig = [20.0]
    lo = 20.0 / 6.0                                      # m = 4: psig / min(100, m + 2)
    assert LR.liar_sigma(pts, [2.0], psig, 4)[0] == max(2.0, lo)             # max(2 - 1, 4 - 2), then the floor
    assert LR.liar_sigma(pts, [1.0], psig, 4)[0] == max(3.0, lo)             # on a point: L = z, U = 4
    assert LR.liar_sigma(pts, [-9.0], psig, 4)[0] == 9.0                     # below every point: U alone
    assert LR.liar_sigma(pts, [30.0], psig, 4)[0] == 20.0                    # above: 26, clipped to psig
    assert LR.liar_sigma(pts, [4.0], psig, 200)[0] == 0.2                    # L = z alone: 0, floored at psig / 100


def test_package_model_equals_the_reference(cases):
    from hyperopt_amd import joint as J
    below, above, low, high, psig, cand, l, g = cases[CASES[0]]
    chain = LR.Chain(above, psig, low, high)
    n = len(above[0]) - 1
    assert J.side_weight_sum(n, 1.0, R.LF) == LR.weight_sum(n)
    assert J.side_weight_sum(300, 1.0, R.LF) == LR.weight_sum(300)
    for j in range(3):
        pts = np.vstack([np.asarray(above[1], dtype=np.float32), chain.mu])
        s = J.liar_sigmas(pts, cand[j], psig, n + j + 1)
        assert s.tobytes() == chain.add(cand[j]).tobytes()
    z = cand[:256].astype(np.float64)
    got = J.liar_log_g(z, g[:256], chain.mu, chain.sigma, chain.W, low, high)
    np.testing.assert_allclose(got, chain.log_g(z, g[:256]), rtol=0, atol=1e-10)
    assert J.liar_log_g(z, g[:256], chain.mu[:0], chain.sigma[:0], chain.W, low, high).tobytes() == g[:256].tobytes()


# -------------------------------------------------------------------- layouts
def test_structs_match_c_and_symbols_are_exported():
    lines = ['printf("TPE_JOINT_LIAR_TILE %d\\n", TPE_JOINT_LIAR_TILE);',
             'printf("tpe_joint_pick %zu\\ntpe_joint_liar_args %zu\\n", sizeof(tpe_joint_pick), '
             'sizeof(tpe_joint_liar_args));']
    for f in N.JOINT_PICK_DTYPE.names:
        lines.append('printf("tpe_joint_pick.%s %%zu\\n", offsetof(tpe_joint_pick, %s));' % (f, f))
    for f, _ in N.JointLiarArgs._fields_:
        lines.append('printf("tpe_joint_liar_args.%s %%zu\\n", offsetof(tpe_joint_liar_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'l.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'l')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['TPE_JOINT_LIAR_TILE'] == N.JOINT_LIAR_TILE
    assert lay['tpe_joint_pick'] == N.JOINT_PICK_DTYPE.itemsize == 24
    assert lay['tpe_joint_liar_args'] == ctypes.sizeof(N.JointLiarArgs)
    for f in N.JOINT_PICK_DTYPE.names:
        assert N.JOINT_PICK_DTYPE.fields[f][1] == lay['tpe_joint_pick.' + f], f
    for f, _ in N.JointLiarArgs._fields_:
        assert getattr(N.JointLiarArgs, f).offset == lay['tpe_joint_liar_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_liar_scratch_bytes', 'tpe_joint_liar'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ----------------------------------------------------- argument checks, no GPU
P_HOST, C_HOST, D_HOST, G_HOST = 3, 5000, 5, 2


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    a = N.JointLiarArgs()
    arr = np.zeros(64)
    keep.append(arr)
    a.n_dims, a.n_cand, a.n_ids, a.n_given = D_HOST, C_HOST, P_HOST, G_HOST
    a.k_above, a.n_trials, a.w_sum = 9, 8, 9.0
    a.cand = a.l_out = a.g_out = a.above_mu = a.given = arr.ctypes.data
    for d in range(64):
        a.psig[d], a.low[d], a.high[d] = 1.0, -np.inf, np.inf
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _need(lib, a):
    nb = ctypes.c_uint64(0)
    assert lib.tpe_joint_liar_scratch_bytes(a.n_ids, a.n_cand, a.n_dims, a.n_given, ctypes.byref(nb)) == 0
    return nb.value


def _call(lib, a, out, nbytes=None, picks=True, z=True, sigma=True, scratch=True):
    p = out.ctypes.data
    return lib.tpe_joint_liar(ctypes.byref(a) if a is not None else None, p if picks else None, p if z else None,
                              p if sigma else None, p if scratch else None, out.nbytes if nbytes is None else nbytes,
                              None)


def test_scratch_bytes_formula_and_its_checks():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    for P, Cn, D, G in ((1, 1, 1, 0), (8, 4096, 3, 0), (3, 5000, 5, 2), (64, 1 << 20, 64, 7)):
        assert lib.tpe_joint_liar_scratch_bytes(P, Cn, D, G, ctypes.byref(nb)) == 0
        assert nb.value == (G + P) * (2 * D + 1) * 8 + -(-Cn // N.JOINT_CHUNK) * 24
    for bad in ((0, 8, 3, 0), (1, 0, 3, 0), (1, 8, 0, 0), (1, 8, 65, 0), (1, 8, 3, -1)):
        assert lib.tpe_joint_liar_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_liar_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_liar_scratch_bytes(1, 8, 3, 0, None) == -1


@pytest.mark.parametrize('over,msg', [
    (dict(n_dims=0), b'n_dims'), (dict(n_dims=65), b'n_dims'),
    (dict(n_ids=0), b'< 1'), (dict(n_cand=0), b'< 1'), (dict(k_above=0), b'< 1'),
    (dict(n_given=-1), b'< 0'), (dict(n_trials=-1), b'< 0'),
    (dict(w_sum=0.0), b'w_sum'), (dict(w_sum=-1.0), b'w_sum'), (dict(w_sum=float('nan')), b'w_sum'),
    (dict(w_sum=float('inf')), b'w_sum'),
    (dict(cand=None), b'null cand'), (dict(l_out=None), b'null cand'), (dict(g_out=None), b'null cand'),
    (dict(above_mu=None), b'null cand'), (dict(given=None), b'without given'),
])
def test_bad_arguments_are_rejected_before_any_launch(over, msg):
    lib, keep = N.load(), []
    a = _host_args(keep, **over)
    out = np.zeros(1 << 16, dtype=np.uint8)
    assert _call(lib, a, out) == -1, over
    assert msg in lib.tpe_last_error(), (over, lib.tpe_last_error())


def test_null_outputs_psig_and_small_scratch_are_rejected():
    lib, keep = N.load(), []
    out = np.zeros(1 << 16, dtype=np.uint8)
    assert _call(lib, None, out) == -1 and b'null args' in lib.tpe_last_error()
    a = _host_args(keep)
    for kw in (dict(picks=False), dict(z=False), dict(sigma=False)):
        assert _call(lib, a, out, **kw) == -1, kw
        assert b'null outputs' in lib.tpe_last_error()
    need = _need(lib, a)
    assert need == (G_HOST + P_HOST) * (2 * D_HOST + 1) * 8 + 5 * 24
    assert _call(lib, a, out, nbytes=need - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert _call(lib, a, out, scratch=False) == -1 and b'scratch too small' in lib.tpe_last_error()
    a.psig[D_HOST - 1] = 0.0
    assert _call(lib, a, out) == -1 and b'prior sigma' in lib.tpe_last_error()
    a.psig[D_HOST - 1] = 1.0
    a.psig[D_HOST] = 0.0                                  # beyond n_dims: not read
    a.given, a.n_given = None, 0                          # no given liars: the pointer may be null
    assert _call(lib, a, out, nbytes=_need(lib, a) - 1) == -1 and b'scratch too small' in lib.tpe_last_error()


# ---------------------------------------------------------- ValueErrors, no GPU
def _no_device(monkeypatch):
    from hyperopt_amd import tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **kw: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **kw: pytest.fail('a startup draw was made'))
    monkeypatch.setattr(N, 'load', lambda *a, **kw: pytest.fail('the library was loaded'))


def _domain(space):
    from hyperopt_amd import base
    return base.Domain(lambda d: 0.0, space)


def _spaces():
    from hyperopt_amd import hp
    cont = {'x': hp.uniform('x', -5, 5), 'y': hp.normal('y', 0, 2), 'lr': hp.loguniform('lr', -5, 0)}
    disc = dict(cont, c=hp.choice('c', [0, 1, 2]))
    quant = dict(cont, q=hp.quniform('q', 0, 10, 1))
    branch = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                          {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}]))
    return cont, disc, quant, branch


@pytest.mark.parametrize('which,kw,match', [
    (0, dict(), 'needs joint'),
    (0, dict(joint=True, joint_shard=(0, 2)), 'joint_shard'),
    (1, dict(joint=True, joint_discrete=True), 'discrete or quantised'),
    (2, dict(joint=True, joint_quantized=True), 'discrete or quantised'),
    (3, dict(joint=True, joint_branches=True), 'branch groups'),
    (3, dict(joint=['a', 'b'], joint_branches=True), 'branch groups'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(which, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    _no_device(monkeypatch)
    domain = _domain(_spaces()[which])
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, joint_liar=True, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, joint_liar=True, **kw)


def test_joint_liar_is_the_last_keyword_and_the_plan_signature_stands():
    import inspect
    from hyperopt_amd import tpe
    for fn in (tpe.suggest, tpe.suggest_choices):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == 'joint_liar' and inspect.signature(fn).parameters['joint_liar'].default is False
    assert 'joint_liar' not in inspect.signature(tpe._joint_plan).parameters
    assert 'joint_liar' not in inspect.signature(tpe.joint_candidate_report).parameters


def test_engine_rejects_liar_with_shard_report_and_strays(monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **kw: pytest.fail('the library was loaded'))
    assert Engine._liar(False, None, False, 0, None) is None
    assert Engine._liar(True, None, True, 0, None) == {'W': None, 'given': None, 'sigma': True}
    assert Engine._liar(12.5, None, False, 0, None)['W'] == 12.5
    for args, match in (((True, None, False, 0, (0, 100)), 'shard'), ((True, None, False, 4, None), 'report_k'),
                        ((False, np.zeros((1, 2)), False, 0, None), 'need liar'),
                        ((False, None, True, 0, None), 'need liar'), ((0.0, None, False, 0, None), 'weight sum'),
                        ((float('nan'), None, False, 0, None), 'weight sum')):
        with pytest.raises(ValueError, match=match):
            Engine._liar(*args)
    below, above, low, high, pmu, psig = R.seeded_case(2, 30, 1)
    r = {'low': low, 'high': high}
    with pytest.raises(ValueError, match='continuous'):
        Engine._liar_model({'W': None, 'given': None, 'sigma': False}, 'mixed', above, r, 2)
    with pytest.raises(ValueError, match='given must be'):
        Engine._liar_model({'W': None, 'given': np.zeros((2, 3)), 'sigma': False}, 'run', above, r, 2)
    m = Engine._liar_model({'W': None, 'given': None, 'sigma': False}, 'run', above, r, 2)
    assert abs(m['W'] - LR.weight_sum(len(above[0]) - 1)) < 1e-9 and m['given'].shape == (0, 2)
    assert (m['psig'] == psig).all()
    for name in ('run_joint', 'run_joint_wide'):
        import inspect
        pars = inspect.signature(getattr(Engine, name)).parameters
        assert pars['liar'].default is False and pars['given'].default is None
    for name in ('run_joint_mixed', 'run_joint_quant', 'run_joint_wide_mixed', 'run_joint_segments'):
        assert 'liar' not in inspect.signature(getattr(Engine, name)).parameters
