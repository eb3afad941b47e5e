"""Batch-aware picks over discrete and quantised labels, the parts
that need no GPU: the mixture identity, the package's model against the numpy
restatement (tests/joint_liar_mixed_ref), the quantised bandwidth rule at its
edges, the candidate whose every liar term is -inf, the condition the GPU
tests' inputs must meet, the struct layout, every TPE_E_ARG of
tpe_joint_liar_mixed and every ValueError of the public interface."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_liar_mixed_ref as X
from tests import joint_liar_ref as LR
from tests import joint_quant_ref as Q
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')

MAX_TIES = 8
B = 8
C = 4096
MIXED, QUANT = X.CASES[0], X.CASES[2]


@pytest.fixture(scope='module')
def cases():
    return dict((c, X.case_inputs(*c, C=C)) for c in X.CASES)


def _tabs(c):
    from hyperopt_amd import joint as J
    return [J.liar_cat_tables(p, s) for p, s in zip(c['ps'], c['sa'])]


def _package_lpdf(c, side, s, rows):
    """joint.quant_lpdf_numpy / mixed_lpdf_numpy of a 6-tuple side at rows."""
    from hyperopt_amd import joint as J
    w, mu, sigma, xc, qmu, qsig = side
    Dc, Dk = mu.shape[1], len(c['ps'])
    z, v, qi = rows[:, :Dc].astype(np.float64), rows[:, Dc:Dc + Dk].astype(np.int64), rows[:, Dc + Dk:].astype(np.int64)
    if c['edges']:
        quants = [(qmu[:, d], qsig[:, d], e) for d, e in enumerate(c['edges'])]
        return J.quant_lpdf_numpy(z, v, qi, w, mu, sigma, c['low'], c['high'], xc, c['ps'], s, quants)
    return J.mixed_lpdf_numpy(z, v, w, mu, sigma, c['low'], c['high'], xc, c['ps'], s)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize('case', [MIXED, QUANT])
def test_extended_density_is_a_mixture_with_more_components(cases, case):
    """g_J = the package's lpdf of the above side with J components appended,
    weights (w~, 1, .., 1) / (W + J), xc rows the picks' categories, qmu / qsigma
    rows the centres and bandwidths; at J = 0 the bytes of the base g, then J = 1
    and 3.  The numpy restatement meets its own lpdf the same way."""
    from hyperopt_amd import joint as J
    c = cases[case]
    rows = c['cand'][:512]
    Dc, Dk = c['above'][1].shape[1], len(c['ps'])
    z, v, qi = rows[:, :Dc].astype(np.float64), rows[:, Dc:Dc + Dk].astype(np.int64), rows[:, Dc + Dk:].astype(np.int64)
    g = _package_lpdf(c, c['above'], c['sa'], rows)
    np.testing.assert_allclose(g, c['g'][:512], rtol=0, atol=1e-10 * max(1.0, float(np.abs(g).max())))
    chain = X.chain_of(c)
    for Jn in range(4):
        liars = (chain.mu, chain.sigma, chain.cat, chain.qc, chain.qs)
        gj = J.liar_mixed_log_g(z, v, qi, g, liars, chain.W, c['low'], c['high'], _tabs(c), c['edges'])
        if Jn == 0:
            assert gj.tobytes() == g.tobytes()
            assert chain.log_g(rows, c['g'][:512]).tobytes() == c['g'][:512].tobytes()
        if Jn in (1, 3):
            ext = chain.extended_side(c['above'])
            assert abs(ext[0].sum() - 1.0) < 1e-12 and len(ext[0]) == len(c['above'][0]) + Jn
            want = _package_lpdf(c, ext, c['sa'], rows)
            np.testing.assert_allclose(gj, want, rtol=0, atol=1e-10 * max(1.0, float(np.abs(want).max())))
            ref = X.base_lpdf(rows, ext, c['low'], c['high'], c['ps'], c['sa'], c['edges'])
            got = chain.log_g(rows, c['g'][:512])
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * max(1.0, float(np.abs(ref).max())))
        chain.add(rows[int(np.argmax(c['l'][:512] - gj))])


@pytest.mark.parametrize('case', [MIXED, QUANT, X.CASES[4]])
def test_package_model_equals_the_reference(cases, case):
    """joint.py against the numpy restatement: sigmas the same bytes, log g
    within 1e-10."""
    from hyperopt_amd import joint as J
    c = cases[case]
    chain = X.chain_of(c)
    n = len(c['above'][0]) - 1
    Dc, Dk = c['above'][1].shape[1], len(c['ps'])
    assert J.side_weight_sum(n, 1.0, R.LF) == chain.W
    for j in range(3):
        row = c['cand'][j]
        qi = row[Dc + Dk:].astype(np.int64)
        cen = np.array([c['centres'][d][qi[d]] for d in range(len(qi))])
        m = n + j + 1
        s = J.liar_sigmas(np.vstack([np.asarray(c['above'][1], dtype=np.float32), chain.mu]), row[:Dc], c['psig'], m) \
            if Dc else np.zeros(0)
        qs = J.liar_quant_sigmas(np.vstack([c['above'][4], chain.qc]), cen, c['above'][5][0], m)
        assert np.concatenate([s, qs]).tobytes() == chain.add(row).tobytes()
    rows = c['cand'][:256]
    z, v, qi = rows[:, :Dc].astype(np.float64), rows[:, Dc:Dc + Dk].astype(np.int64), rows[:, Dc + Dk:].astype(np.int64)
    got = J.liar_mixed_log_g(z, v, qi, c['g'][:256], (chain.mu, chain.sigma, chain.cat, chain.qc, chain.qs), chain.W,
                             c['low'], c['high'], _tabs(c), c['edges'])
    np.testing.assert_allclose(got, chain.log_g(rows, c['g'][:256]), rtol=0, atol=1e-10)


def test_quant_centres_are_the_fit_coordinates():
    from hyperopt_amd import joint as J
    from hyperopt_amd.parzen import fit_coord
    for (dist, low, high, q), (m_lo, V) in Q.LATTICE_CASES:
        if V > N.JOINT_MAX_LATTICE:
            continue
        args = {'low': low, 'high': high, 'q': q}
        cen = J.quant_centres(dist, args)
        assert cen.dtype == np.float64 and len(cen) == V
        assert cen.tobytes() == np.asarray(fit_coord(dist, args, (m_lo + np.arange(V)) * q), dtype=np.float64).tobytes()
        assert np.isfinite(cen).all() and (np.diff(cen) >= 0).all()
    assert J.quant_centres('quniform', {'low': 0.0, 'high': 10.0, 'q': 1.0}).tolist() == list(range(11))


def test_quant_sigma_rule_at_the_edges():
    from hyperopt_amd import joint as J
    pts = np.array([[0.0], [1.0], [4.0]])
    psig = [20.0]
    lo = 20.0 / 6.0                                      # m = 4: psig / min(100, m + 2)
    for fn in (X.quant_sigma, J.liar_quant_sigmas):
        assert fn(pts, [2.0], psig, 4)[0] == max(2.0, lo)              # max(2 - 1, 4 - 2), then the floor
        assert fn(pts, [1.0], psig, 4)[0] == max(3.0, lo)              # on an existing qmu: L = c, U = 4
        assert fn(pts, [-9.0], psig, 4)[0] == 9.0                      # below every point: U alone
        assert fn(pts, [30.0], psig, 4)[0] == 20.0                     # above every point: 26, clipped to psig
        assert fn(pts, [4.0], psig, 200)[0] == 0.2                     # L = c alone: 0, floored at psig / 100
        assert fn(np.zeros((0, 1)), [4.0], psig, 1)[0] == 20.0 / 3.0   # no point at all: 0, floored


def test_a_candidate_every_liar_term_leaves_at_minus_infinity():
    """V = 256, n = 110: the given liar at lattice index 0 has sigma psig / 100;
    the candidate at index 255 lies beyond the tail rule, its bin mass is exactly
    0, so g_1 = g - log1p(1 / W) exactly, finite, no NaN."""
    from hyperopt_amd import joint as J
    c = X.far_bin_case()
    assert len(c['above'][0]) - 1 >= 98
    chain = X.chain_of(c, given=[[0.0]])
    assert chain.sigmas.tolist() == [[255.0 / 100.0]]
    assert np.isneginf(chain.log_kernels(c['cand'])[0]).all()
    g1 = chain.log_g(c['cand'], c['g'])
    assert np.isfinite(g1).all()
    assert g1[0] == c['g'][0] - np.log1p(1.0 / chain.W)
    qi = c['cand'].astype(np.int64)
    z, v = np.zeros((len(qi), 0)), np.zeros((len(qi), 0), dtype=np.int64)
    got = J.liar_mixed_log_g(z, v, qi, c['g'], (chain.mu, chain.sigma, chain.cat, chain.qc, chain.qs), chain.W,
                             c['low'], c['high'], [], c['edges'])
    assert np.isfinite(got).all() and got[0] == c['g'][0] - np.log1p(1.0 / chain.W)
    np.testing.assert_allclose(got, g1, rtol=0, atol=1e-10)


@pytest.mark.parametrize('case', X.CASES)
def test_inputs_give_distinct_picks_and_small_tie_sets(cases, case):
    """A condition on the GPU tests' inputs, not a measurement: the reference
    alone picks 8 distinct candidates, with at most MAX_TIES near-ties a step.
    The all-discrete group is exempt from both: its rows repeat, and equal rows
    score equally by construction; the GPU test checks tie-set membership only."""
    c = cases[case]
    steps = X.greedy(X.chain_of(c), c['cand'], c['l'], c['g'], B)
    picks = [s[3] for s in steps]
    print(case, picks, [len(s[1]) for s in steps])
    if case[0] == 0 and not case[2]:
        return
    assert len(set(picks)) == B
    assert max(len(s[1]) for s in steps) <= MAX_TIES


# -------------------------------------------------------------------- layouts
def test_structs_match_c_and_symbols_are_exported():
    lines = ['printf("tpe_joint_liar_mixed_args %zu\\ntpe_joint_liar_args %zu\\n", sizeof(tpe_joint_liar_mixed_args), '
             'sizeof(tpe_joint_liar_args));']
    for f, _ in N.JointLiarMixedArgs._fields_:
        lines.append('printf("f.%s %%zu\\n", offsetof(tpe_joint_liar_mixed_args, %s));' % (f, f))
    for f, _ in N.JointLiarArgs._fields_:
        lines.append('printf("p.%s %%zu\\n", offsetof(tpe_joint_liar_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'l.c')
        open(src, 'w').write(prog)
        exe = os.path.join(d, 'l')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), src, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['tpe_joint_liar_mixed_args'] == ctypes.sizeof(N.JointLiarMixedArgs)
    assert lay['tpe_joint_liar_args'] == ctypes.sizeof(N.JointLiarArgs) == lay['f.n_cat']
    for f, _ in N.JointLiarMixedArgs._fields_:
        assert getattr(N.JointLiarMixedArgs, f).offset == lay['f.' + f], f
    for f, _ in N.JointLiarArgs._fields_:                  # the shared prefix: the same offsets
        assert lay['p.' + f] == lay['f.' + f], f
    lib = N.load()
    for name in ('tpe_joint_liar_mixed_scratch_bytes', 'tpe_joint_liar_mixed'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ----------------------------------------------------- argument checks, no GPU
P_HOST, C_HOST, G_HOST = 3, 5000, 2
DC_HOST, US_HOST, VS_HOST = 2, (3, 5), (4, 7)


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""
    a = N.JointLiarMixedArgs()
    arr = np.zeros(64)
    keep.append(arr)
    a.n_dims, a.n_cand, a.n_ids, a.n_given = DC_HOST, C_HOST, P_HOST, G_HOST
    a.k_above, a.n_trials, a.w_sum = 9, 8, 9.0
    for f in ('cand', 'l_out', 'g_out', 'above_mu', 'given', 'cat_miss', 'cat_bonus', 'quant_edges', 'quant_centre',
              'above_qmu'):
        setattr(a, f, arr.ctypes.data)
    for d in range(64):
        a.psig[d], a.low[d], a.high[d] = 1.0, -np.inf, np.inf
    a.n_cat, a.n_quant = len(US_HOST), len(VS_HOST)
    for d, U in enumerate(US_HOST):
        a.cat_upper[d], a.cat_off[d] = U, sum(US_HOST[:d])
    for d, V in enumerate(VS_HOST):
        a.quant_v[d], a.quant_edge_off[d] = V, sum(VS_HOST[:d]) + d
    a.n_edges = sum(VS_HOST) + len(VS_HOST)
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _need(lib, a):
    nb = ctypes.c_uint64(0)
    nl = sum(a.quant_v[d] for d in range(a.n_quant))
    assert lib.tpe_joint_liar_mixed_scratch_bytes(a.n_ids, a.n_cand, a.n_dims, a.n_cat, a.n_quant, nl, a.n_given,
                                                  ctypes.byref(nb)) == 0
    return nb.value


def _call(lib, a, out, nbytes=None, picks=True, z=True, sigma=True, scratch=True):
    p = out.ctypes.data
    return lib.tpe_joint_liar_mixed(ctypes.byref(a) if a is not None else None, p if picks else None,
                                    p if z else None, p if sigma else None, p if scratch else None,
                                    out.nbytes if nbytes is None else nbytes, None)


def test_scratch_bytes_formula_and_its_checks():
    lib = N.load()
    nb, nb0 = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for P, Cn, Dc, Dk, Dq, nl, G in ((1, 1, 0, 1, 0, 0, 0), (8, 4096, 2, 1, 0, 0, 0), (3, 5000, 2, 2, 2, 11, 2),
                                     (64, 1 << 20, 8, 4, 4, 512, 7), (8, 4096, 19, 2, 0, 0, 1)):
        assert lib.tpe_joint_liar_mixed_scratch_bytes(P, Cn, Dc, Dk, Dq, nl, G, ctypes.byref(nb)) == 0
        assert nb.value == (G + P) * (2 * Dc + 1 + Dk + Dq + nl) * 8 + -(-Cn // N.JOINT_CHUNK) * 24
    for P, Cn, D, G in ((8, 4096, 3, 0), (3, 5000, 64, 2)):                 # no discrete or quantised label: the liar's
        assert lib.tpe_joint_liar_mixed_scratch_bytes(P, Cn, D, 0, 0, 0, G, ctypes.byref(nb)) == 0
        assert lib.tpe_joint_liar_scratch_bytes(P, Cn, D, G, ctypes.byref(nb0)) == 0
        assert nb.value == nb0.value
    for bad in ((0, 8, 1, 1, 0, 0, 0), (1, 0, 1, 1, 0, 0, 0), (1, 8, 0, 0, 0, 0, 0), (1, 8, -1, 1, 0, 0, 0),
                (1, 8, 60, 5, 0, 0, 0), (1, 8, 1, 17, 0, 0, 0), (1, 8, 1, 0, 5, 10, 0), (1, 8, 1, 0, 1, 513, 0),
                (1, 8, 1, 0, 1, 0, 0), (1, 8, 1, 1, 0, 4, 0), (1, 8, 1, 1, 0, 0, -1)):
        assert lib.tpe_joint_liar_mixed_scratch_bytes(*bad, ctypes.byref(nb)) == -1, bad
        assert b'tpe_joint_liar_mixed_scratch_bytes' in lib.tpe_last_error()
    assert lib.tpe_joint_liar_mixed_scratch_bytes(1, 8, 1, 1, 0, 0, 0, None) == -1


@pytest.mark.parametrize('over,msg', [
    (dict(n_dims=-1), b'< 0'), (dict(n_cat=-1), b'< 0'), (dict(n_quant=-1), b'< 0'),
    (dict(n_cat=17), b'n_cat above'), (dict(n_quant=5), b'n_quant above'),
    (dict(n_dims=63, n_quant=0), b'row width'), (dict(n_dims=9), b'beside a quantised'),
    (dict(n_cat=5), b'beside a quantised'),
    (dict(n_ids=0), b'< 1'), (dict(n_cand=0), b'< 1'), (dict(k_above=0), b'< 1'),
    (dict(n_given=-1), b'< 0'), (dict(n_trials=-1), b'< 0'),
    (dict(w_sum=0.0), b'w_sum'), (dict(w_sum=float('nan')), b'w_sum'), (dict(w_sum=float('inf')), b'w_sum'),
    (dict(cand=None), b'null cand'), (dict(l_out=None), b'null cand'), (dict(g_out=None), b'null cand'),
    (dict(above_mu=None), b'null cand'), (dict(given=None), b'without given'),
    (dict(psig=(1, 0.0)), b'prior sigma'), (dict(psig=(DC_HOST + 1, -1.0)), b'prior sigma'),
    (dict(cat_miss=None), b'null category'), (dict(cat_bonus=None), b'null category'),
    (dict(cat_upper=(0, 1)), b'U_d'), (dict(cat_upper=(1, 257)), b'U_d'),
    (dict(cat_off=(1, 4)), b'cat_off'), (dict(cat_off=(0, -1)), b'cat_off'),
    (dict(quant_edges=None), b'null quant'), (dict(quant_centre=None), b'null quant'),
    (dict(above_qmu=None), b'null quant'),
    (dict(quant_v=(0, 1)), b'V_d'), (dict(quant_v=(1, 257)), b'V_d'),
    (dict(quant_edge_off=(1, 6)), b'quant_edge_off'), (dict(quant_edge_off=(0, -1)), b'quant_edge_off'),
    (dict(n_edges=12), b'quant_edge_off'),
])
def test_bad_arguments_are_rejected_before_any_launch(over, msg):
    lib, keep = N.load(), []
    a = _host_args(keep, **over)
    out = np.zeros(1 << 17, dtype=np.uint8)
    assert _call(lib, a, out) == -1, over
    assert msg in lib.tpe_last_error(), (over, lib.tpe_last_error())


def test_totals_null_outputs_and_small_scratch_are_rejected():
    lib, keep = N.load(), []
    out = np.zeros(1 << 17, dtype=np.uint8)
    assert _call(lib, None, out) == -1 and b'null args' in lib.tpe_last_error()
    a = _host_args(keep)
    for kw in (dict(picks=False), dict(z=False), dict(sigma=False)):
        assert _call(lib, a, out, **kw) == -1, kw
        assert b'null outputs' in lib.tpe_last_error()
    need = _need(lib, a)
    assert need == (G_HOST + P_HOST) * (2 * DC_HOST + 1 + 2 + 2 + 11) * 8 + 5 * 24
    assert _call(lib, a, out, nbytes=need - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert _call(lib, a, out, scratch=False) == -1 and b'scratch too small' in lib.tpe_last_error()
    a.psig[DC_HOST + 2] = 0.0                             # beyond the quantised dimensions: not read
    a.above_mu, a.n_dims = None, 0                        # no continuous label: the pointer may be null
    assert _call(lib, a, out, nbytes=_need(lib, a) - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    a = _host_args(keep, n_dims=0, n_quant=0, n_cat=5)    # more than TPE_JOINT_MAX_CAT_TOTAL categories
    for d in range(5):
        a.cat_upper[d], a.cat_off[d] = 256, 0
    assert _call(lib, a, out) == -1 and b'TPE_JOINT_MAX_CAT_TOTAL' in lib.tpe_last_error()
    a = _host_args(keep, n_quant=3, n_edges=1024)         # more than TPE_JOINT_MAX_LATTICE_TOTAL lattice values
    for d in range(3):
        a.quant_v[d], a.quant_edge_off[d] = 256, 0
    assert _call(lib, a, out) == -1 and b'TPE_JOINT_MAX_LATTICE_TOTAL' in lib.tpe_last_error()
    a = _host_args(keep, n_cat=0, n_quant=0)              # a continuous group: tpe_joint_liar's own checks
    a.w_sum = -1.0
    assert _call(lib, a, out) == -1 and b'tpe_joint_liar: w_sum' in lib.tpe_last_error()


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
    mixed = dict(cont, c=hp.choice('c', [0, 1, 2]), q=hp.quniform('q', 0, 10, 1))
    branch = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                          {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}]))
    return cont, mixed, branch


@pytest.mark.parametrize('which,liar,kw,match', [
    (1, 'mixed', dict(), 'needs joint'),
    (1, 'mixed', dict(joint=True, joint_discrete=True, joint_quantized=True, joint_shard=(0, 2)), 'joint_shard'),
    (2, 'mixed', dict(joint=True, joint_branches=True), 'branch groups'),
    (2, 'mixed', dict(joint=['a', 'b'], joint_branches=True), 'branch groups'),
    (1, 'other', dict(joint=True, joint_discrete=True), "True or 'mixed'"),
    (0, 'other', dict(joint=True), "True or 'mixed'"),
    (0, 1, dict(joint=True), "True or 'mixed'"),
    (0, 2.5, dict(joint=True), "True or 'mixed'"),
    (1, True, dict(joint=True, joint_discrete=True, joint_quantized=True), 'discrete or quantised'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(which, liar, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    _no_device(monkeypatch)
    domain = _domain(_spaces()[which])
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, joint_liar=liar, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234, joint_liar=liar, **kw)


def test_mixed_passes_the_checks_and_the_signature_facts_stand(monkeypatch):
    """'mixed' on a group with a choice and a quniform gets past every argument
    check (with no trials the startup draw is what comes next); False, None and
    np.bool_ stay what they were; joint_liar is still the last keyword."""
    from hyperopt_amd import base, tpe
    domain = _domain(_spaces()[1])
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **kw: pytest.fail('the engine was touched'))
    monkeypatch.setattr(tpe.rand, 'suggest', lambda *a, **kw: 'startup')
    kw = dict(joint=True, joint_discrete=True, joint_quantized=True)
    assert tpe.suggest([0, 1], domain, base.Trials(), 1234, joint_liar='mixed', **kw) == 'startup'
    assert tpe.suggest([0, 1], _domain(_spaces()[0]), base.Trials(), 1234, joint_liar='mixed', joint=True) == 'startup'
    assert tpe._joint_liar_mode(False) is None and tpe._joint_liar_mode(None) is None
    assert tpe._joint_liar_mode(np.bool_(False)) is None
    assert tpe._joint_liar_mode(True) is True and tpe._joint_liar_mode(np.bool_(True)) is True
    assert tpe._joint_liar_mode('mixed') == 'mixed'
    for fn in (tpe.suggest, tpe.suggest_choices):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == 'joint_liar' and inspect.signature(fn).parameters['joint_liar'].default is False
    assert 'joint_liar' not in inspect.signature(tpe._joint_plan).parameters
    assert 'joint_liar' not in inspect.signature(tpe.joint_candidate_report).parameters


def test_engine_keywords_and_given_rows(monkeypatch):
    """Engine.run_joint_liar_mixed with no device: liar with shard / report_k, a
    call without liar, and given rows that are non-integral or out of range."""
    from hyperopt_amd import joint_pack as JP
    from hyperopt_amd.engine import Engine
    from tests import joint_mixed_ref as M
    pars = inspect.signature(Engine.run_joint_liar_mixed).parameters
    assert pars['liar'].default is True and pars['given'].default is None and pars['return_sigma'].default is False
    for name in ('run_joint_mixed', 'run_joint_quant', 'run_joint_wide_mixed'):     # pinned by the existing tests
        assert 'liar' not in inspect.signature(getattr(Engine, name)).parameters
    e = Engine.__new__(Engine)
    monkeypatch.setattr(N, 'load', lambda *a, **kw: pytest.fail('the library was loaded'))
    args = ((), (), [], [], [], [], [0], 8, 1)
    for kw, match in ((dict(shard=(0, 100)), 'shard'), (dict(report_k=4), 'report_k'), (dict(liar=False), 'needs liar'),
                      (dict(liar=0.0), 'weight sum')):
        with pytest.raises(ValueError, match=match):
            e.run_joint_liar_mixed(*args, **kw)
    c = X.case_inputs(*X.CASES[2], C=64)                   # (1, (2,), (5,), 80): a row is [z, category, lattice index]
    cats = M.cats_of(c['below'], c['above'], c['ps'], c['sb'], c['sa'])
    quants = Q.quants_of(c['below'], c['above'], c['edges'])
    r = JP.group_rows(c['below'][:3], c['above'][:3], c['low'], c['high'], cats, quants, entry='quant')

    def model(given=None, centres=c['centres'], W=None):
        return Engine._liar_mixed_model({'W': W, 'given': given, 'sigma': False, 'mixed': True, 'centres': centres},
                                        c['above'][:3], r, cats, quants)
    m = model(given=[[0.5, 1, 4], [0.25, 0, 0]])
    assert m['given'].dtype == np.float32 and m['given'].shape == (2, 3) and m['n_sigma'] == 2
    assert abs(m['W'] - LR.weight_sum(len(c['above'][0]) - 1)) < 1e-9
    assert m['psig'].tolist() == [float(c['psig'][0]), float(c['above'][5][0, 0])]
    assert m['centre'].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and len(m['miss']) == len(m['bonus']) == 2
    for given, match in (([[0.5, 2, 0]], 'category'), ([[0.5, -1, 0]], 'category'), ([[0.5, 0.5, 0]], 'category'),
                         ([[0.5, 0, 5]], 'lattice index'), ([[0.5, 0, 1.5]], 'lattice index'),
                         ([[0.5, 0]], 'given must be')):
        with pytest.raises(ValueError, match=match):
            model(given=given)
    with pytest.raises(ValueError, match='needs centres'):
        model(centres=None)
    with pytest.raises(ValueError, match='one finite value per lattice value'):
        model(centres=[np.arange(4.0)])
