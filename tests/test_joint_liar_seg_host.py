"""Batch-aware picks in branch groups (DESIGN.md of that name), the parts that
need no GPU: the layouts of the descriptor and the args struct against the C
header, the scratch formula, every TPE_E_ARG tpe_joint_liar_seg returns before
any launch, the chain packer (joint_pack.liar_chains) against a literal and a
brute-force restatement, and every ValueError of joint_liar='branches' and of
Engine.run_joint_segments_liar."""
import ctypes
import inspect
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from hyperopt_amd import joint_pack as JP
from tests import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')


# -------------------------------------------------------------------- layouts
def test_structs_match_c_and_symbols_are_exported():
    lines = ['printf("tpe_joint_liar_seg_desc %zu\\ntpe_joint_liar_seg_args %zu\\n", '
             'sizeof(tpe_joint_liar_seg_desc), sizeof(tpe_joint_liar_seg_args));']
    for f, _ in N.JointLiarSeg._fields_:
        lines.append('printf("tpe_joint_liar_seg_desc.%s %%zu\\n", offsetof(tpe_joint_liar_seg_desc, %s));' % (f, f))
    for f, _ in N.JointLiarSegArgs._fields_:
        lines.append('printf("tpe_joint_liar_seg_args.%s %%zu\\n", offsetof(tpe_joint_liar_seg_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'l.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'l')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['tpe_joint_liar_seg_desc'] == ctypes.sizeof(N.JointLiarSeg) == N.JOINT_LIAR_SEG_DTYPE.itemsize
    assert lay['tpe_joint_liar_seg_args'] == ctypes.sizeof(N.JointLiarSegArgs)
    assert [f for f, _ in N.JointLiarSeg._fields_] == list(N.JOINT_LIAR_SEG_DTYPE.names)
    for f, _ in N.JointLiarSeg._fields_:
        assert getattr(N.JointLiarSeg, f).offset == lay['tpe_joint_liar_seg_desc.' + f], f
        assert N.JOINT_LIAR_SEG_DTYPE.fields[f][1] == lay['tpe_joint_liar_seg_desc.' + f], f
    for f, _ in N.JointLiarSegArgs._fields_:
        assert getattr(N.JointLiarSegArgs, f).offset == lay['tpe_joint_liar_seg_args.' + f], f
    lib = N.load()
    for name in ('tpe_joint_liar_seg_scratch_bytes', 'tpe_joint_liar_seg'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# --------------------------------------------------------------------- chains
PROB_SEG = [2, 0, 2, 1, 2, 0]


def test_liar_chains_literal():
    ch = JP.liar_chains(PROB_SEG, 4)
    assert ch.order.tolist() == [2, 0, 1, 3]              # lengths 3, 2, 1, 0: descending, stable
    assert ch.first.tolist() == [3, 5, 0, 6]              # by group
    assert ch.chain.tolist() == [0, 2, 4, 1, 5, 3]        # slot -> problem, a group's problems in caller order
    assert ch.active.tolist() == [3, 2, 1]
    assert ch.order.dtype == ch.first.dtype == ch.chain.dtype == np.int32


@pytest.mark.parametrize('seed', range(6))
def test_liar_chains_brute_force(seed):
    rs = np.random.RandomState(seed)
    S = int(rs.randint(1, 7))
    prob_seg = rs.randint(0, S, size=int(rs.randint(1, 40)))
    ch = JP.liar_chains(prob_seg, S)
    chains = [[p for p, s in enumerate(prob_seg) if s == g] for g in range(S)]
    order = sorted(range(S), key=lambda g: (-len(chains[g]), g))
    assert ch.order.tolist() == order
    slot = 0
    for g in order:
        assert ch.first[g] == slot
        assert ch.chain[slot:slot + len(chains[g])].tolist() == chains[g]
        slot += len(chains[g])
    assert slot == len(prob_seg)
    longest = max(len(c) for c in chains)
    assert ch.active.tolist() == [sum(len(c) > r for c in chains) for r in range(longest)]
    for r, n in enumerate(ch.active):                     # the active groups of round r are a prefix of the order
        assert all(len(chains[g]) > r for g in order[:n]) and all(len(chains[g]) <= r for g in order[n:])


def test_liar_chains_rejects():
    for args in (([], 2), ([0], 0), ([0, 2], 2), ([-1], 2)):
        with pytest.raises(ValueError):
            JP.liar_chains(*args)


# ----------------------------------------------------- argument checks, no GPU
C_HOST = 5000
DIMS = (3, 2, 5, 4)


def _models():
    return [R.seeded_case(D, 20 + 3 * D, 1 + D)[:4] for D in DIMS]


class _Host(object):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""

    def __init__(self, prob_seg=PROB_SEG):
        models = _models()
        self.b = JP.segment_blob(models, [7, 8, 9, 10], prob_seg, np.arange(len(prob_seg)), C_HOST, None,
                                 N.JOINT_SEG_DTYPE)
        self.lb = JP.liar_segment_blob(models, self.b.segs, JP.liar_weight_sums(True, models), self.b.prob_seg)
        self.pool = np.zeros(self.b.n32, dtype=np.float32)
        self.out = np.zeros(1 << 16, dtype=np.uint8)
        a = self.a = N.JointLiarSegArgs()
        a.n_segs, a.n_probs, a.n_cand = len(models), len(prob_seg), C_HOST
        a.segs = a.host_segs = self.lb.segs.ctypes.data
        a.order = a.host_order = self.lb.order.ctypes.data
        a.chain = a.host_chain = self.lb.chain.ctypes.data
        a.log_norm = a.host_log_norm = self.lb.log_norm.ctypes.data
        a.host_prob_seg = self.b.prob_seg.ctypes.data
        a.cand = a.l_out = a.g_out = a.cand_off = a.pool_f32 = self.pool.ctypes.data
        a.pool_f32_len = self.b.n32

    def need(self, lib):
        nb = ctypes.c_uint64(0)
        assert lib.tpe_joint_liar_seg_scratch_bytes(self.lb.segs.ctypes.data, self.a.n_segs, self.a.n_cand,
                                                    ctypes.byref(nb)) == 0
        return nb.value

    def call(self, lib, nbytes=None, args=True, picks=True, z=True, sigma=True, scratch=True):
        p = self.out.ctypes.data
        return lib.tpe_joint_liar_seg(ctypes.byref(self.a) if args else None, p if picks else None, p if z else None,
                                      p if sigma else None, p if scratch else None,
                                      self.out.nbytes if nbytes is None else nbytes, None)


def test_the_packed_arguments_pass_every_check_but_the_scratch_size():
    """The packer's own output is what the library accepts: with one byte of
    scratch too few the call gets as far as the last check."""
    lib, h = N.load(), _Host()
    lens = [2, 1, 3, 0]
    need = h.need(lib)
    assert need == sum(L * (2 * D + 1) for L, D in zip(lens, DIMS)) * 8 + 3 * 5 * 24
    assert h.call(lib, nbytes=need - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert h.call(lib, scratch=False) == -1 and b'scratch too small' in lib.tpe_last_error()
    segs = h.lb.segs
    assert segs['chain_len'].tolist() == lens and segs['chain_first'].tolist() == [3, 5, 0, 6]
    assert segs['row_off'].tolist() == [3 * 11, 3 * 11 + 2 * 7, 0, 3 * 11 + 2 * 7 + 5]
    assert segs['sigma_off'].tolist() == [15, 21, 0, 23] and h.lb.n_sigma == 23
    assert (segs['above_mu'] == h.b.segs['above_mu']).all() and (segs['n_trials'] == segs['k_above'] - 1).all()
    for s in range(4):
        W = segs['w_sum'][s]
        assert segs['log_w'][s] == math.log(W)
        assert [h.lb.log_norm[segs['chain_first'][s] + j] for j in range(lens[s])] == \
            [math.log1p(j / W) for j in range(lens[s])]


def test_scratch_bytes_formula_and_its_checks():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    for lens, dims, Cn in (((1,), (1,), 1), ((8, 3, 1, 0), (3, 2, 16, 5), 4096), ((34, 2, 5), (1, 2, 5), 1500),
                           ((16, 16, 16, 16), (4, 4, 4, 4), 1 << 20), ((0, 0), (2, 2), 7)):
        segs = np.zeros(len(lens), dtype=N.JOINT_LIAR_SEG_DTYPE)
        segs['chain_len'], segs['n_dims'] = lens, dims
        assert lib.tpe_joint_liar_seg_scratch_bytes(segs.ctypes.data, len(lens), Cn, ctypes.byref(nb)) == 0
        active = sum(L > 0 for L in lens)
        assert nb.value == sum(L * (2 * D + 1) for L, D in zip(lens, dims)) * 8 + active * -(-Cn // N.JOINT_CHUNK) * 24
    segs = np.zeros(2, dtype=N.JOINT_LIAR_SEG_DTYPE)
    segs['chain_len'], segs['n_dims'] = 1, 2
    ok = (segs.ctypes.data, 2, 8, ctypes.byref(nb))
    assert lib.tpe_joint_liar_seg_scratch_bytes(*ok) == 0
    for i, v in ((0, None), (1, 0), (2, 0), (3, None)):
        bad = list(ok)
        bad[i] = v
        assert lib.tpe_joint_liar_seg_scratch_bytes(*bad) == -1, (i, v)
        assert b'tpe_joint_liar_seg_scratch_bytes' in lib.tpe_last_error()
    for field, v in (('n_dims', 0), ('n_dims', 17), ('chain_len', -1)):
        segs[field][1] = v
        assert lib.tpe_joint_liar_seg_scratch_bytes(*ok) == -1, (field, v)
        segs[field][1] = 1 if field == 'chain_len' else 2


@pytest.mark.parametrize('field,value,msg', [
    ('n_segs', 0, b'< 1'), ('n_probs', 0, b'< 1'), ('n_cand', 0, b'< 1'),
    ('segs', None, b'null segs'), ('host_segs', None, b'null segs'), ('order', None, b'null segs'),
    ('host_order', None, b'null segs'), ('chain', None, b'null segs'), ('host_chain', None, b'null segs'),
    ('log_norm', None, b'null segs'), ('host_log_norm', None, b'null segs'), ('host_prob_seg', None, b'null segs'),
    ('cand', None, b'null cand'), ('cand_off', None, b'null cand'), ('l_out', None, b'null cand'),
    ('g_out', None, b'null cand'), ('pool_f32', None, b'null cand'),
])
def test_bad_arguments_are_rejected_before_any_launch(field, value, msg):
    lib, h = N.load(), _Host()
    setattr(h.a, field, value)
    assert h.call(lib) == -1, field
    assert msg in lib.tpe_last_error(), (field, lib.tpe_last_error())


@pytest.mark.parametrize('field,seg,value,msg', [
    ('n_dims', 0, 0, b'n_dims'), ('n_dims', 3, 17, b'n_dims'), ('k_above', 1, 0, b'k_above'),
    ('n_trials', 2, -1, b'n_trials'), ('w_sum', 0, 0.0, b'w_sum'), ('w_sum', 0, -1.0, b'w_sum'),
    ('w_sum', 3, float('nan'), b'w_sum'), ('w_sum', 1, float('inf'), b'w_sum'),
    ('above_mu', 2, -1, b'above_mu'), ('above_mu', 3, 1 << 40, b'above_mu'),
    ('log_w', 0, 0.123, b'log_w'),
    ('chain_len', 2, 2, b'partition'), ('chain_len', 3, 1, b'partition'), ('chain_first', 0, 4, b'partition'),
    ('row_off', 0, 0, b'row_off'), ('sigma_off', 1, 0, b'row_off'),
])
def test_bad_descriptors_are_rejected_before_any_launch(field, seg, value, msg):
    lib, h = N.load(), _Host()
    h.lb.segs[field][seg] = value
    assert h.call(lib) == -1, (field, seg, value)
    assert msg in lib.tpe_last_error(), (field, lib.tpe_last_error())


def test_null_outputs_psig_pool_and_chain_tables_are_rejected():
    lib = N.load()
    h = _Host()
    assert h.call(lib, args=False) == -1 and b'null args' in lib.tpe_last_error()
    for kw in (dict(picks=False), dict(z=False), dict(sigma=False)):
        assert h.call(lib, **kw) == -1 and b'null outputs' in lib.tpe_last_error(), kw
    for v in (0.0, -1.0, float('nan')):
        h = _Host()
        h.lb.segs['psig'][1][DIMS[1] - 1] = v
        assert h.call(lib) == -1 and b'prior sigma' in lib.tpe_last_error()
    h = _Host()
    h.lb.segs['psig'][1][DIMS[1]] = 0.0                     # beyond n_dims: not read
    assert h.call(lib, nbytes=h.need(lib) - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    h = _Host()
    h.a.pool_f32_len = int((h.lb.segs['above_mu'] + h.lb.segs['k_above'] * h.lb.segs['n_dims']).max()) - 1
    assert h.call(lib) == -1 and b'above_mu' in lib.tpe_last_error()
    # the chain table: a swapped pair inside a chain, a problem in another group's chain, a repeated problem,
    # an entry out of range; the order: not by length, not a permutation; the problem list itself
    for edit in (lambda h: h.lb.chain.__setitem__(slice(0, 2), [2, 0]),
                 lambda h: h.lb.chain.__setitem__(slice(2, 4), [1, 4]),
                 lambda h: h.lb.chain.__setitem__(1, 0),
                 lambda h: h.lb.chain.__setitem__(5, 6),
                 lambda h: h.lb.order.__setitem__(slice(0, 2), [0, 2]),
                 lambda h: h.lb.order.__setitem__(3, 1),
                 lambda h: h.lb.order.__setitem__(3, 4),
                 lambda h: h.b.prob_seg.__setitem__(3, 0)):
        h = _Host()
        edit(h)
        assert h.call(lib) == -1 and b'partition' in lib.tpe_last_error(), lib.tpe_last_error()
    for v in (-1, 4):
        h = _Host()
        h.b.prob_seg[0] = v
        assert h.call(lib) == -1 and b'host_prob_seg entry' in lib.tpe_last_error()
    h = _Host()
    h.lb.log_norm[1] = np.nextafter(h.lb.log_norm[1], 1.0)  # the host's log1p, to the last bit
    assert h.call(lib) == -1 and b'log_norm' in lib.tpe_last_error()


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
    branch = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                          {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}]))
    branch_disc = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1),
                                                'k': hp.randint('k', 5)},
                                               {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1)}]))
    branch_quant = dict(cont, g=hp.choice('g', [{'a': hp.uniform('a', 0, 1), 'b': hp.uniform('b', 0, 1)},
                                                {'u': hp.normal('u', 0, 1), 'v': hp.normal('v', 0, 1),
                                                 'q': hp.quniform('q', 0, 10, 1)}]))
    return cont, branch, branch_disc, branch_quant


def test_the_mode():
    from hyperopt_amd import tpe
    assert tpe._joint_liar_mode('branches') == 'branches'
    assert tpe._joint_liar_mode('mixed') == 'mixed' and tpe._joint_liar_mode(True) is True
    assert tpe._joint_liar_mode(False) is None and tpe._joint_liar_mode(None) is None
    for bad in ('other', 'branch', 1, 2.5):
        with pytest.raises(ValueError, match="True or 'mixed'"):
            tpe._joint_liar_mode(bad)
    with pytest.raises(ValueError, match="'branches' with joint_branches"):
        tpe._joint_liar_mode('other')


@pytest.mark.parametrize('which,kw,match', [
    (1, dict(joint_branches=True), 'needs joint'),
    (1, dict(joint=True, joint_branches=True, joint_shard=(0, 2)), 'joint_shard'),
    (1, dict(joint=True), 'needs joint_branches=True'),
    (0, dict(joint=True), 'needs joint_branches=True'),
    (2, dict(joint=True, joint_branches=True, joint_discrete=True, joint_branches_mixed=True),
     'joint_branches_mixed.*discrete or quantised'),
    (3, dict(joint=True, joint_branches=True, joint_quantized=True, joint_branches_mixed=True),
     'joint_branches_mixed.*discrete or quantised'),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(which, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    _no_device(monkeypatch)
    domain = _domain(_spaces()[which])
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, joint_liar='branches', **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234,
                            joint_liar='branches', **kw)


@pytest.mark.parametrize('mode', [True, 'mixed'])
def test_true_and_mixed_still_refuse_branch_groups(mode, monkeypatch):
    from hyperopt_amd import base, tpe
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match='branch groups'):
        tpe.suggest([0, 1], _domain(_spaces()[1]), base.Trials(), 1234, joint=True, joint_branches=True,
                    joint_liar=mode)


class _Startup(Exception):
    pass


@pytest.mark.parametrize('which,kw', [
    (1, dict(joint=True, joint_branches=True)),                      # a root group and two branch groups
    (1, dict(joint=['a', 'b', 'u', 'v'], joint_branches=True)),      # no root group
    (2, dict(joint=True, joint_branches=True)),                      # the discrete label stays univariate
    (0, dict(joint=True, joint_branches=True)),                      # no branch group in the space: 'mixed'
])
def test_branches_gets_past_the_checks_to_the_startup_draw(which, kw, monkeypatch):
    from hyperopt_amd import base, tpe
    _no_device(monkeypatch)

    def startup(*a, **k):
        raise _Startup()
    monkeypatch.setattr(tpe.rand, 'suggest', startup)
    with pytest.raises(_Startup):
        tpe.suggest([0, 1], _domain(_spaces()[which]), base.Trials(), 1234, joint_liar='branches', **kw)


def test_signatures_stand():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import Engine
    for fn in (tpe.suggest, tpe.suggest_choices):
        pars = inspect.signature(fn).parameters
        assert list(pars)[-1] == 'joint_liar' and pars['joint_liar'].default is False
    assert 'joint_liar' not in inspect.signature(tpe._joint_plan).parameters
    assert 'joint_liar' not in inspect.signature(tpe.joint_candidate_report).parameters
    assert 'liar' not in inspect.signature(Engine.run_joint_segments).parameters
    pars = inspect.signature(Engine.run_joint_segments_liar).parameters
    assert list(pars) == ['self', 'models', 'stream_words', 'prob_seg', 'prob_id', 'n_cand', 'seed', 'liar', 'inject',
                          'return_cand', 'want_lg', 'return_sigma']
    assert pars['liar'].default is True and 'shard' not in pars and 'report_k' not in pars


def test_engine_rejects_mixed_models_and_bad_weight_sums(monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **kw: pytest.fail('the library was loaded'))
    eng = Engine.__new__(Engine)                             # no device, no library: the checks come first
    cont = [R.seeded_case(2, 30, 1)[:4], R.seeded_case(3, 30, 2)[:4]]
    K = len(cont[1][0][0]), len(cont[1][1][0])
    cat = (np.zeros(K[0], dtype=np.int64), np.zeros(K[1], dtype=np.int64), np.array([0.5, 0.5]), 1.0, 1.0)
    with pytest.raises(ValueError, match='group 1 holds a discrete or quantised'):
        eng.run_joint_segments_liar([cont[0], cont[1] + ([cat],)], [1, 2], [0, 1], [5, 6], 64, 3)
    for W in ([1.0, 0.0], [1.0, -2.0], [1.0, float('nan')], [1.0, float('inf')], [1.0], 3.5, False):
        with pytest.raises(ValueError, match='weight sum'):
            eng.run_joint_segments_liar(cont, [1, 2], [0, 1], [5, 6], 64, 3, liar=W)
    assert JP.liar_weight_sums(True, cont) == [1.0 / float(m[1][0][-1]) for m in cont]
    assert JP.liar_weight_sums([2.0, 3.5], cont) == [2.0, 3.5]
