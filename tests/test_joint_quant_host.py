"""Quantised labels in the joint stage (DESIGN.md "Quantised labels in the joint
stage"), the parts that need no GPU: the lattice rule and the binned model
against the numpy restatement (tests/joint_quant_ref.py), the struct layout,
the argument checks tpe_joint_quant_run makes before any launch, and the public
keyword ``joint_quantized`` with its own argument checks."""
import ctypes
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from tests import joint_quant_ref as Q
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')
LOG2E = 1.0 / np.log(2.0)


def _args(case):
    dist, low, high, q = case
    return dist, {'low': low, 'high': high, 'q': q}


def _components(case, n=50, seed=0):
    """(mu, sigma, values) of the prior row and n observations of a lattice case
    in its fit coordinate, drawn as the label draws them."""
    dist, low, high, q = case
    rs = np.random.RandomState(seed)
    u = rs.uniform(low, high, n)
    vals = np.rint((np.exp(u) if dist == 'qloguniform' else u) / q) * q
    x = np.log(np.maximum(vals, max(1e-12, math.exp(low)))) if dist == 'qloguniform' else vals
    _, mu, sigma = R.ref_side(x[:, None], np.array([0.5 * (low + high)]), np.array([high - low]))
    return mu[:, 0], sigma[:, 0], vals


# ------------------------------------------------------------ lattice, model
@pytest.mark.parametrize('case,want', Q.LATTICE_CASES)
def test_lattice_and_edges(case, want):
    """V, m_lo and strictly increasing edges e_0 = low .. e_V = high; a value
    whose clipped bin is empty is not in the lattice."""
    from hyperopt_amd import joint as J
    dist, args = _args(case)
    m_lo, V, q, edges = J.quant_lattice(dist, args)
    assert (m_lo, V) == want == J.lattice_size(dist, args)[:2] and q == case[3]
    r_lo, r_V, r_edges = Q.ref_lattice(*case)
    assert (r_lo, r_V) == want
    np.testing.assert_array_equal(edges, r_edges)
    assert edges.dtype == np.float64 and len(edges) == V + 1
    assert edges[0] == case[1] and edges[-1] == case[2] and (np.diff(edges) > 0).all()
    if case[0] == 'qloguniform' and case[1] < math.log(0.5):
        assert m_lo == 0                                   # the value 0: its bin is [low, log(q / 2))


@pytest.mark.parametrize('case,want', Q.LATTICE_CASES)
def test_binning_rule_is_the_rounding_rule(case, want):
    """The number of interior edges <= z is rint(x / q) - m_lo on 2e5 uniform draws."""
    from hyperopt_amd import joint as J
    dist, args = _args(case)
    m_lo, V, q, edges = J.quant_lattice(dist, args)
    z = np.random.RandomState(want[1]).uniform(case[1], case[2], 200000)
    x = np.exp(z) if dist == 'qloguniform' else z
    i = np.searchsorted(edges[1:-1], z, 'right')
    assert i.min() == 0 and i.max() == V - 1
    np.testing.assert_array_equal(i, np.rint(x / q).astype(np.int64) - m_lo)


@pytest.mark.parametrize('case,want', Q.LATTICE_CASES)
def test_bin_masses_sum_to_one(case, want):
    """sum_i P_kd(i) = 1 to 1e-12 for every component (components outside the
    bounds included: the top value of qloguniform(log 16, log 512, 16) sits at
    `high`), the prior row's log2 P stays above -10, and the package's P is the
    restatement's."""
    from hyperopt_amd import joint as J
    dist, args = _args(case)
    edges = J.quant_lattice(dist, args)[3]
    mu, sigma, _ = _components(case)
    mu = np.concatenate([mu, [case[1] - 0.3 * (case[2] - case[1]), case[2] + 0.1 * (case[2] - case[1])]])
    sigma = np.concatenate([sigma, [0.05 * (case[2] - case[1]), 0.2 * (case[2] - case[1])]])
    P = J.quant_P(mu, sigma, edges)
    assert P.shape == (len(mu), want[1]) and (P >= 0).all()
    np.testing.assert_allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    ref = Q.ref_binP(mu, sigma, edges)
    np.testing.assert_allclose(ref.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(P, ref, rtol=1e-12, atol=1e-300)
    assert np.log2(P[0]).min() > -10.0


@pytest.mark.parametrize('n', [0, 1, 25, 26, 90])
def test_quant_lpdf_numpy_matches_the_restated_model(n):
    """joint.quant_lpdf_numpy is the restatement to 1e-12, and a quantised
    column (full of repeated values) gets the restatement's bandwidths bit for
    bit: the stable tie order."""
    from hyperopt_amd import joint as J
    below, above, low, high, ps, sb, sa, edges, rs = Q.seeded_quant_case(2, [3], [11, 5], n)
    C = 257
    z = rs.uniform(-9, 9, (C, 2))
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1)
    qi = np.stack([rs.randint(len(e) - 1, size=C) for e in edges], axis=1)
    for side, s in ((below, sb), (above, sa)):
        w, mu, sigma, xc, qmu, qsig = side
        quants = [(qmu[:, d], qsig[:, d], e) for d, e in enumerate(edges)]
        got = J.quant_lpdf_numpy(z, v, qi, w, mu, sigma, low, high, xc, ps, s, quants)
        np.testing.assert_allclose(got, Q.ref_quant_lpdf(z, v, qi, side, low, high, ps, s, edges), rtol=0, atol=1e-12)
        priors = [(0.5 * (e[0] + e[-1]), e[-1] - e[0]) for e in edges]
        jw, jmu, jsig = J.side_mixture(qmu[1:], priors)
        np.testing.assert_array_equal(jw, w)
        np.testing.assert_array_equal(jmu, qmu)
        np.testing.assert_array_equal(jsig, qsig)
    # an all-quantised group
    b0, a0, l0, h0, ps0, s0, _, e0, rs = Q.seeded_quant_case(0, [], [7], n)
    qi = rs.randint(7, size=(C, 1))
    got = J.quant_lpdf_numpy(np.zeros((C, 0)), np.zeros((C, 0)), qi, b0[0], b0[1], b0[2], l0, h0, b0[3], [], s0,
                             [(b0[4][:, 0], b0[5][:, 0], e0[0])])
    np.testing.assert_allclose(got, Q.ref_quant_lpdf(np.zeros((C, 0)), np.zeros((C, 0)), qi, b0, l0, h0, [], s0, e0),
                               rtol=0, atol=1e-12)


def test_the_device_form_in_float64_is_the_model():
    """c (without the quantised dimensions) - sum_cont + the categories' terms +
    sum_d T[k][d][i_d] summed over k is the model's density: the algebra of the
    kernel evaluated in float64 from the float64 table, floor included (this
    lattice of 256 values has entries at the floor, -inf among them)."""
    from hyperopt_amd import joint as J
    from tests import joint_mixed_ref as M
    _, below, low, high, ps, _, sb, edges, rs = Q.seeded_quant_case(2, [3], [256, 5], 60)     # (its above side: 59 rows)
    w, mu, sigma, xc, qmu, qsig = below
    C = 64
    z = rs.uniform(-9, 9, (C, 2))
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1)
    qi = np.stack([rs.randint(len(e) - 1, size=C) for e in edges], axis=1)
    c = R.ref_logcoef(w, mu, sigma, low, high) * LOG2E
    t = c[None, :] - 0.5 * LOG2E * (((z[:, None, :] - mu[None, :, :]) / sigma[None, :, :]) ** 2).sum(axis=2)
    t = t + np.log2(M.ref_P(xc[:, 0], ps[0], sb[0]))[:, v[:, 0]].T
    n_floor = n_inf = 0
    for d, e in enumerate(edges):
        T = J.quant_table(qmu[:, d], qsig[:, d], e)
        ref, raw = Q.ref_table(qmu[:, d], qsig[:, d], e)
        assert T.shape == (len(w), len(e) - 1) and T.dtype == np.float64 and T.min() >= N.JOINT_QFLOOR
        np.testing.assert_array_equal(T == N.JOINT_QFLOOR, ref == Q.QFLOOR)
        np.testing.assert_allclose(T, ref, rtol=1e-9, atol=1e-9)
        n_floor += int((raw < Q.QFLOOR).sum())
        n_inf += int(np.isneginf(raw).sum())
        t = t + T[:, qi[:, d]].T
    assert n_floor > 0 and n_inf > 0
    got = (np.log2(np.exp2(t - t.max(axis=1)[:, None]).sum(axis=1)) + t.max(axis=1)) * np.log(2.0)
    np.testing.assert_allclose(got, Q.ref_quant_lpdf(z, v, qi, below, low, high, ps, sb, edges), rtol=0, atol=1e-12)


def test_quniform_256_has_entries_at_the_floor():
    """quniform(0, 256, 1)'s neighbour in the limits, 256 values, 50 components:
    several hundred bin masses are exactly 0 in float64."""
    from hyperopt_amd import joint as J
    case = ('quniform', 0.0, 255.0, 1.0)
    mu, sigma, _ = _components(case, n=49)
    edges = J.quant_lattice(*_args(case))[3]
    diff, mass = J.quant_bin_masses(mu, sigma, edges)
    assert (mass > 0).all() and (diff >= 0).all()
    assert (diff == 0).sum() > 100
    T = J.quant_table(mu, sigma, edges)
    assert (T[diff == 0] == N.JOINT_QFLOOR).all() and np.isfinite(T).all()


# ------------------------------------------------------------------------ ABI
def test_quant_args_match_c():
    consts = ['TPE_JOINT_MAX_QUANT', 'TPE_JOINT_MAX_LATTICE', 'TPE_JOINT_MAX_LATTICE_TOTAL', 'TPE_JOINT_MAX_DIMS',
              'TPE_ABI_VERSION']
    lines = ['printf("%s %%d\\n", %s);' % (c, c) for c in consts]
    lines.append('printf("TPE_JOINT_QFLOOR %d\\n", (int)TPE_JOINT_QFLOOR);')
    lines.append('printf("tpe_joint_quant_args %zu\\ntpe_joint_mixed_args %zu\\n", sizeof(tpe_joint_quant_args), '
                 'sizeof(tpe_joint_mixed_args));')
    for f, _ in N.JointQuantArgs._fields_:
        lines.append('printf("tpe_joint_quant_args.%s %%zu\\n", offsetof(tpe_joint_quant_args, %s));' % (f, f))
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
    assert lay['TPE_JOINT_MAX_QUANT'] == N.JOINT_MAX_QUANT == 4
    assert lay['TPE_JOINT_MAX_LATTICE'] == N.JOINT_MAX_LATTICE == 256
    assert lay['TPE_JOINT_MAX_LATTICE_TOTAL'] == N.JOINT_MAX_LATTICE_TOTAL == 512
    assert lay['TPE_JOINT_QFLOOR'] == N.JOINT_QFLOOR == -4096
    assert lay['TPE_JOINT_MAX_DIMS'] == N.JOINT_MAX_DIMS == 16
    assert lay['TPE_ABI_VERSION'] == N.ABI_VERSION == 24
    assert lay['tpe_joint_quant_args'] == ctypes.sizeof(N.JointQuantArgs)
    for f, _ in N.JointQuantArgs._fields_:
        assert getattr(N.JointQuantArgs, f).offset == lay['tpe_joint_quant_args.' + f], f
    # the fields of tpe_joint_mixed_args, at the same places; the new ones follow
    for f, _ in N.JointMixedArgs._fields_:
        assert getattr(N.JointQuantArgs, f).offset == getattr(N.JointMixedArgs, f).offset, f
    assert N.JointQuantArgs.n_quant.offset == lay['tpe_joint_mixed_args'] == ctypes.sizeof(N.JointMixedArgs)


def test_library_exports_the_quant_symbols_at_abi_24():
    lib = N.load()
    for name in ('tpe_joint_quant_run', 'tpe_joint_quant_table_bytes', 'tpe_joint_quant_profile'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24
    nb = ctypes.c_uint64(0)
    assert lib.tpe_joint_quant_table_bytes(26, 9976, 32, ctypes.byref(nb)) == 0
    assert nb.value == (26 + 9976) * 32 * 4
    assert lib.tpe_joint_quant_table_bytes(0, 9, 32, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_quant_table_bytes(4, 9, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_joint_quant_table_bytes(4, 9, 32, None) == -1


TABLE_BYTES = (4 + 9) * (11 + 5) * 4


def _host_args(keep, **over):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch.  3 continuous, 2 discrete, 2 quantised labels."""
    arr = np.zeros(4096)
    keep.append(arr)
    a = N.JointQuantArgs()
    a.n_dims, a.n_cat, a.n_quant, a.n_cand, a.n_ids, a.flags = 3, 2, 2, 2048, 1, 0
    a.k_below, a.k_above, a.stream_word, a.seed = 4, 9, N.JOINT_STREAM, 7
    for f in ('below_mu', 'below_a', 'below_c', 'above_mu', 'above_a', 'above_c', 'samp_cum', 'samp', 'ids',
              'below_cat', 'above_cat', 'below_miss', 'below_bonus', 'above_miss', 'above_bonus', 'below_h', 'cat_cum',
              'quant_edges', 'below_qmu', 'below_qsigma', 'above_qmu', 'above_qsigma', 'quant_samp', 'quant_table'):
        setattr(a, f, arr.ctypes.data)
    a.cat_upper[0], a.cat_upper[1] = 3, 5
    a.cat_off[0], a.cat_off[1] = 0, 3
    a.quant_v[0], a.quant_v[1] = 11, 5
    a.quant_edge_off[0], a.quant_edge_off[1] = 0, 12
    a.n_edges, a.quant_table_bytes = 18, TABLE_BYTES
    for k, v in over.items():
        if k in ('cat_upper', 'cat_off', 'quant_v', 'quant_edge_off'):
            for d, x in enumerate(v):
                getattr(a, k)[d] = x
        else:
            setattr(a, k, v)
    return a


def _run(lib, a, keep, records=True, scratch_bytes=0):
    """tpe_joint_quant_run with NO usable scratch unless asked: the scratch
    check is the last one, so every earlier rejection is reached and a call that
    were wrongly accepted still could not launch."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    keep.append(buf)
    p = buf.ctypes.data
    return lib.tpe_joint_quant_run(ctypes.byref(a) if a is not None else None, p if records else None, None, None,
                                   None, p if scratch_bytes else None, scratch_bytes, None)


def test_null_quant_args_are_rejected():
    lib, keep = N.load(), []
    assert _run(lib, None, keep) == -1
    assert b'tpe_joint_quant_run: null args' in lib.tpe_last_error()


@pytest.mark.parametrize('over,msg', [
    # everything tpe_joint_mixed_run checks
    (dict(n_dims=-1), b'n_dims + n_cat + n_quant outside'), (dict(n_dims=17), b'n_dims + n_cat + n_quant outside'),
    (dict(n_cat=-1), b'n_cat < 0'),
    (dict(n_cand=0), b'n_cand < 1'), (dict(n_ids=0), b'n_ids < 1'),
    (dict(k_below=0), b'k_below < 1'), (dict(k_above=0), b'k_below < 1 or k_above < 1'),
    (dict(below_mu=None), b'null density rows'), (dict(below_a=None), b'null density rows'),
    (dict(below_c=None), b'null density rows'), (dict(above_mu=None), b'null density rows'),
    (dict(above_a=None), b'null density rows'), (dict(above_c=None), b'null density rows'),
    (dict(samp_cum=None), b'null sampler rows'), (dict(samp=None), b'null sampler rows'),
    (dict(flags=N.JOINT_INJECT), b'TPE_JOINT_INJECT without candidates'),
    (dict(ids=None), b'null ids'),
    (dict(below_cat=None), b'null category tables'), (dict(above_cat=None), b'null category tables'),
    (dict(below_miss=None), b'null category tables'), (dict(below_bonus=None), b'null category tables'),
    (dict(above_miss=None), b'null category tables'), (dict(above_bonus=None), b'null category tables'),
    (dict(below_h=None), b'null category tables'), (dict(cat_cum=None), b'null category tables'),
    (dict(cat_upper=[1, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_upper=[257, 5]), b'outside [2, TPE_JOINT_MAX_CATS]'),
    (dict(cat_off=[0, 4]), b'cat_off outside'), (dict(cat_off=[-1, 3]), b'cat_off outside'),
    # the coordinates in all, the quantised ones counted
    (dict(n_dims=8, n_cat=4, n_quant=4, n_cand=0), b'n_cand < 1'),            # (16 coordinates are allowed)
    (dict(n_dims=13, n_cat=2), b'n_dims + n_cat + n_quant outside'),
    # n_quant outside [0, 4]
    (dict(n_quant=-1), b'n_quant outside [0, TPE_JOINT_MAX_QUANT]'),
    (dict(n_quant=5), b'n_quant outside [0, TPE_JOINT_MAX_QUANT]'),
    # n_dims > 8 or n_cat > 4 beside a quantised label
    (dict(n_dims=9), b'n_dims > 8 or n_cat > 4'), (dict(n_dims=2, n_cat=5), b'n_dims > 8 or n_cat > 4'),
    # a V_d outside [2, 256]
    (dict(quant_v=[1, 5]), b'outside [2, TPE_JOINT_MAX_LATTICE]'),
    (dict(quant_v=[11, 0]), b'outside [2, TPE_JOINT_MAX_LATTICE]'),
    (dict(quant_v=[257, 5]), b'outside [2, TPE_JOINT_MAX_LATTICE]'),
    (dict(quant_v=[11, -3]), b'outside [2, TPE_JOINT_MAX_LATTICE]'),
    # more than 512 lattice values in all
    (dict(n_quant=3, quant_v=[256, 256, 2], quant_edge_off=[0, 257, 514], n_edges=517,
          quant_table_bytes=13 * 514 * 4), b'more than TPE_JOINT_MAX_LATTICE_TOTAL'),
    # an edge offset outside the edge array
    (dict(quant_edge_off=[0, 13]), b'quant_edge_off outside'), (dict(quant_edge_off=[-1, 12]), b'quant_edge_off outside'),
    (dict(n_edges=17), b'quant_edge_off outside'), (dict(quant_edge_off=[7, 12]), b'quant_edge_off outside'),
    # a null edge / mu / sigma / sampler / table pointer
    (dict(quant_edges=None), b'null quantised rows or table'), (dict(below_qmu=None), b'null quantised rows or table'),
    (dict(below_qsigma=None), b'null quantised rows or table'), (dict(above_qmu=None), b'null quantised rows or table'),
    (dict(above_qsigma=None), b'null quantised rows or table'), (dict(quant_samp=None), b'null quantised rows or table'),
    (dict(quant_table=None), b'null quantised rows or table'),
    # a table workspace smaller than tpe_joint_quant_table_bytes says
    (dict(quant_table_bytes=TABLE_BYTES - 1), b'table workspace too small'),
    (dict(quant_table_bytes=0), b'table workspace too small'),
])
def test_bad_quant_arguments_are_rejected_without_a_device(over, msg):
    lib, keep = N.load(), []
    assert _run(lib, _host_args(keep, **over), keep) == -1
    assert b'tpe_joint_quant_run' in lib.tpe_last_error() and msg in lib.tpe_last_error(), lib.tpe_last_error()


def test_accepted_quant_arguments_reach_the_scratch_check():
    """Good arguments (an all-quantised group without any other rows, and every
    limit at once) pass every check up to the last one."""
    lib, keep = N.load(), []
    nb = ctypes.c_uint64(0)
    assert lib.tpe_joint_quant_table_bytes(4, 9, 16, ctypes.byref(nb)) == 0 and nb.value == TABLE_BYTES
    none = dict(below_mu=None, below_a=None, above_mu=None, above_a=None, samp=None, below_cat=None, above_cat=None,
                below_miss=None, below_bonus=None, above_miss=None, above_bonus=None, below_h=None, cat_cum=None)
    for over in (dict(), dict(n_dims=0, n_cat=0, **none),
                 dict(n_dims=8, n_cat=4, n_quant=4, cat_upper=[256] * 4, cat_off=[0, 256, 512, 768],
                      quant_v=[256, 252, 2, 2], quant_edge_off=[0, 257, 510, 513], n_edges=516,
                      quant_table_bytes=13 * 512 * 4)):
        assert _run(lib, _host_args(keep, **over), keep) == -1
        assert b'tpe_joint_quant_run: scratch too small' in lib.tpe_last_error(), (over, lib.tpe_last_error())
    assert _run(lib, _host_args(keep), keep, records=False) == -1
    assert b'null ids / records' in lib.tpe_last_error()
    need = ctypes.c_uint64(0)
    assert lib.tpe_joint_scratch_bytes(1, 2048, ctypes.byref(need)) == 0
    assert _run(lib, _host_args(keep), keep, scratch_bytes=need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()


def test_n_quant_zero_forwards_to_the_mixed_stage():
    """n_quant = 0 is tpe_joint_mixed_run (and with n_cat = 0 too, tpe_joint_run),
    with its checks and its messages; the quantised fields are not looked at."""
    lib, keep = N.load(), []
    junk = dict(quant_v=[0, 999], quant_edges=None, quant_table=None, quant_table_bytes=0)
    assert _run(lib, _host_args(keep, n_quant=0, **junk), keep) == -1
    assert b'tpe_joint_mixed_run: scratch too small' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, n_quant=0, cat_upper=[1, 5]), keep) == -1
    assert b'tpe_joint_mixed_run: categories of a label outside' in lib.tpe_last_error()
    assert _run(lib, _host_args(keep, n_quant=0, n_cat=0, **junk), keep) == -1
    assert b'tpe_joint_run: scratch too small' in lib.tpe_last_error()
    over = dict(n_dims=9, n_cat=5, cat_upper=[2] * 5, cat_off=[0, 2, 4, 6, 8])        # (no quantised label: no 8 / 4 limit)
    assert _run(lib, _host_args(keep, n_quant=0, **over), keep) == -1
    assert b'tpe_joint_mixed_run: scratch too small' in lib.tpe_last_error()


# ------------------------------------------------------- the public interface
def _space(extra=None):
    from hyperopt_amd import base, hp
    s = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
         'q': hp.quniform('q', 0, 10, 1), 'b': hp.qloguniform('b', math.log(16), math.log(512), 16),
         'qn': hp.qnormal('qn', 0, 2, 1), 'qln': hp.qlognormal('qln', 0, 1, 1),
         'one': hp.quniform('one', 0, 0.4, 1), 'big': hp.quniform('big', 0, 256, 1),
         'leaf': hp.choice('leaf', ['a', 'b', 'c']),
         'c': hp.choice('c', [0, 1, {'k': hp.uniform('inner', 0, 1), 'm': hp.quniform('cq', 0, 5, 1)}])}
    s.update(extra or {})
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
    for name in ('tpe_joint_run', 'tpe_joint_mixed_run', 'tpe_joint_quant_run', 'tpe_run_batch', 'tpe_level_run',
                 'tpe_suggest_tree'):
        monkeypatch.setattr(lib, name, boom, raising=False)


def test_eligible_quant():
    from hyperopt_amd import joint as J
    t = _space().table
    want = {'q': True, 'b': True, 'qn': False, 'qln': False, 'one': False, 'big': False, 'cq': False, 'x': False,
            'leaf': False, 'c': False}
    for label, ok in want.items():
        assert J.eligible_quant(t.by_label[label], t) is ok, label
    assert 'conditional' in J.quant_reason(t.by_label['cq'], t)
    assert 'unbounded and data-dependent' in J.quant_reason(t.by_label['qn'], t)
    assert 'unbounded and data-dependent' in J.quant_reason(t.by_label['qln'], t)
    assert 'fewer than 2' in J.quant_reason(t.by_label['one'], t)
    why = J.quant_reason(t.by_label['big'], t)
    assert '257 lattice values' in why and 'TPE_JOINT_MAX_LATTICE = 256' in why and 'uniform' in why
    assert 'not a quniform or qloguniform' in J.quant_reason(t.by_label['x'], t)
    # the answers of the other two predicates are what they were
    assert 'quantised' in J.discrete_reason(t.by_label['q'], t) and not J.eligible_discrete(t.by_label['q'], t)
    assert not J.eligible(t.by_label['q']) and not J.eligible(t.by_label['b'])


def _many(n_cont, quants):
    from hyperopt_amd import base, hp
    s = dict(('x%02d' % i, hp.uniform('x%02d' % i, 0, 1)) for i in range(n_cont))
    s.update(dict(('q%d' % i, hp.quniform('q%d' % i, 0, hi, 1)) for i, hi in enumerate(quants)))
    return base.Domain(lambda d: 0.0, s)


@pytest.mark.parametrize('kw,match', [
    (dict(joint_quantized=True), 'joint_quantized=True needs joint'),
    (dict(joint=False, joint_quantized=True), 'joint_quantized=True needs joint'),
    (dict(joint=None, joint_quantized=True), 'joint_quantized=True needs joint'),
    (dict(joint=['x', 'cq'], joint_quantized=True), "'cq'.*conditional"),
    (dict(joint=['x', 'qn'], joint_quantized=True), "'qn'.*unbounded and data-dependent"),
    (dict(joint=['x', 'qln'], joint_quantized=True), "'qln'.*unbounded and data-dependent"),
    (dict(joint=['x', 'one'], joint_quantized=True), "'one'.*1 lattice value, fewer than 2"),
    (dict(joint=['x', 'big'], joint_quantized=True), "'big'.*257 lattice values.*uniform"),
    (dict(joint=['x', 'inner'], joint_quantized=True), "'inner'.*conditional"),
    (dict(joint=['x', 'nope'], joint_quantized=True), "'nope'"),
    (dict(joint=['q'], joint_quantized=True), 'at least 2'),
    # without joint_discrete a discrete label is refused as before
    (dict(joint=['q', 'leaf'], joint_quantized=True), "'leaf'"),
    (dict(joint=['q', 'c'], joint_quantized=True, joint_discrete=True), "'c'.*gate"),
    (dict(joint=True, joint_quantized=True, sampler='replay'), 'replay'),
    (dict(joint=True, joint_quantized=True, precision='fp64'), 'fp64'),
    (dict(joint=True, joint_quantized=True, shard=(0, 2)), 'shard'),
    (dict(joint=True, joint_quantized=True, shard_ids=(0, 2)), 'shard'),
    # keyword off: a quantised label is refused as before
    (dict(joint=['x', 'q']), "'q'.*quniform"),
    (dict(joint=['x', 'q'], joint_quantized=False), "'q'.*quniform"),
    (dict(joint=['x', 'q'], joint_discrete=True), "'q'.*quantised"),
])
def test_joint_quantized_argument_errors_come_before_any_device_use(kw, match, no_device):
    from hyperopt_amd import base, history, tpe
    d = _space()
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], d, base.Trials(), 1, **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(d.table, history.extract(d, base.Trials()), [0], 1, **kw)


@pytest.mark.parametrize('domain,match', [
    (lambda: _many(1, [3, 3, 3, 3, 3]), r'TPE_JOINT_MAX_QUANT = 4 quantised labels, not 5.*joint=\[\.\.\.\]'),
    (lambda: _many(1, [255, 255, 2]), r'TPE_JOINT_MAX_LATTICE_TOTAL = 512 lattice values in all, not 515.*joint=\['),
    (lambda: _many(9, [3]), r'at most 8 continuous labels beside a quantised one, not 9.*joint=\[\.\.\.\]'),
])
def test_group_limits_raise_under_joint_true(domain, match, no_device):
    from hyperopt_amd import base, tpe
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0], domain(), base.Trials(), 1, joint=True, joint_quantized=True)
    # without the keyword the same spaces join their continuous labels alone (or have too few of them)
    d = domain()
    labels = [r.label for r in d.table.rows if r.dist == 'uniform']
    if len(labels) >= 2:
        got = tpe._joint_group(d.table, True, 'philox', 'fp32', (None,) * 4)
        assert [r.label for r in got] == labels


def test_five_discrete_labels_beside_a_quantised_one(no_device):
    from hyperopt_amd import base, hp, tpe
    s = dict(('c%d' % i, hp.choice('c%d' % i, [0, 1])) for i in range(5))
    s['q'] = hp.quniform('q', 0, 3, 1)
    d = base.Domain(lambda d: 0.0, s)
    with pytest.raises(ValueError, match='at most 4 discrete labels beside a quantised one, not 5'):
        tpe.suggest([0], d, base.Trials(), 1, joint=True, joint_discrete=True, joint_quantized=True)


def test_the_group_of_joint_quantized(no_device):
    """joint=True joins the eligible quantised labels too and skips qnormal,
    qlognormal, conditional, one-value and oversized ones; the kernel order is
    continuous, discrete, quantised, each in table order."""
    from hyperopt_amd import tpe
    t = _space().table
    none = (None, None, None, None)
    order = [r.label for r in t.rows]
    got = tpe._joint_group(t, True, 'philox', 'fp32', none, True, True)
    assert set(r.label for r in got) == {'x', 'y', 'z', 'q', 'b', 'leaf'}
    assert [r.label for r in got] == [x for x in order if x in {'x', 'y', 'z', 'q', 'b', 'leaf'}]     # table order
    crows, drows, qrows = tpe._joint_kernel_order(got)
    assert [r.label for r in crows] == [x for x in order if x in 'xyz']
    assert [r.label for r in drows] == ['leaf']
    assert [r.label for r in qrows] == [x for x in order if x in 'qb']
    # without joint_discrete the discrete label stays out; without the keyword the quantised ones do
    assert set(r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none, False, True)) == set('xyzqb')
    assert set(r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none, True)) == {'x', 'y', 'z', 'leaf'}
    assert set(r.label for r in tpe._joint_group(t, True, 'philox', 'fp32', none)) == set('xyz')
    # a list may name quantised labels alone
    assert [r.label for r in tpe._joint_group(t, ['q', 'b'], 'philox', 'fp32', none, False, True)] == \
        [x for x in order if x in 'qb']


def test_joined_values_are_multiples_of_q():
    """QuantModel.values maps a lattice index i to (m_lo + i) q as float64."""
    from hyperopt_amd import joint as J
    t = _space().table
    rows = [t.by_label['y']], [t.by_label['leaf']], [t.by_label['q'], t.by_label['b']]
    lats = [J.quant_lattice(r.dist, r.args) for r in rows[2]]
    m = J.QuantModel(rows[0], rows[1], rows[2], None, None, None, None, None, None, None, lats)
    z = np.array([[0.5, 2.0, 10.0, 31.0], [-1.0, 0.0, 0.0, 0.0]])
    v = m.values(z)
    assert v.dtype == np.float64
    np.testing.assert_array_equal(v[:, 2:], [[10.0, 512.0], [0.0, 16.0]])
    np.testing.assert_array_equal(v[:, 0], np.exp(z[:, 0]))
    np.testing.assert_array_equal(v[:, 1], z[:, 1])


def test_startup_path_is_unchanged_by_joint_quantized(golden, no_device):
    """Below n_startup_jobs a suggest is rand.suggest, whatever joint_quantized
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
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True, joint_quantized=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=['x', 'q'], joint_quantized=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint=True, joint_discrete=True,
                             joint_quantized=True)) == g['vals']
    assert plain(tpe.suggest([5, 6], d, trials, g['seed'], joint_quantized=False)) == g['vals']
