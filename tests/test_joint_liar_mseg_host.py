"""Batch-aware picks in mixed branch groups (DESIGN.md of that name), the parts
that need no GPU: the layouts of the descriptor and the args struct against the
C header, the packer (joint_pack.liar_msegment_blob) on a four-group example,
the scratch formula, every TPE_E_ARG tpe_joint_liar_mseg returns before any
launch, the ValueErrors of joint_liar='branches_mixed', the signature of
Engine.run_joint_msegments_liar, and the tie cap of tests/test_gpu_joint_liar_mseg.py
on the numpy reference alone."""
import ctypes
import inspect
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N
from hyperopt_amd import joint as J
from hyperopt_amd import joint_pack as JP
from tests import joint_liar_mixed_ref as X
from tests import joint_liar_ref as LR
from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R
from tests import test_gpu_joint_liar_mseg as G
from tests import test_joint_liar_seg_host as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')


# -------------------------------------------------------------------- layouts
def test_structs_match_c_and_symbols_are_exported():
    lines = ['printf("tpe_joint_liar_mseg_desc %zu\\ntpe_joint_liar_mseg_args %zu\\n", '
             'sizeof(tpe_joint_liar_mseg_desc), sizeof(tpe_joint_liar_mseg_args));']
    for f, _ in N.JointLiarMSeg._fields_:
        lines.append('printf("tpe_joint_liar_mseg_desc.%s %%zu\\n", offsetof(tpe_joint_liar_mseg_desc, %s));' % (f, f))
    for f, _ in N.JointLiarMSegArgs._fields_:
        lines.append('printf("tpe_joint_liar_mseg_args.%s %%zu\\n", offsetof(tpe_joint_liar_mseg_args, %s));' % (f, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'l.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'l')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    lay = dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())
    assert lay['tpe_joint_liar_mseg_desc'] == ctypes.sizeof(N.JointLiarMSeg) == N.JOINT_LIAR_MSEG_DTYPE.itemsize
    assert lay['tpe_joint_liar_mseg_args'] == ctypes.sizeof(N.JointLiarMSegArgs)
    assert [f for f, _ in N.JointLiarMSeg._fields_] == list(N.JOINT_LIAR_MSEG_DTYPE.names)
    for f, _ in N.JointLiarMSeg._fields_:
        assert getattr(N.JointLiarMSeg, f).offset == lay['tpe_joint_liar_mseg_desc.' + f], f
        assert N.JOINT_LIAR_MSEG_DTYPE.fields[f][1] == lay['tpe_joint_liar_mseg_desc.' + f], f
    for f, _ in N.JointLiarMSegArgs._fields_:
        assert getattr(N.JointLiarMSegArgs, f).offset == lay['tpe_joint_liar_mseg_args.' + f], f
    for f, _ in N.JointLiarSeg._fields_:                   # the shared prefixes
        assert getattr(N.JointLiarMSeg, f).offset == getattr(N.JointLiarSeg, f).offset, f
    for f, _ in N.JointLiarSegArgs._fields_:
        assert getattr(N.JointLiarMSegArgs, f).offset == getattr(N.JointLiarSegArgs, f).offset, f
    lib = N.load()
    for name in ('tpe_joint_liar_mseg_scratch_bytes', 'tpe_joint_liar_mseg'):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert lib.tpe_abi_version() == 24


# ------------------------------------------------------- the four-group example
# continuous D = 3; narrow mixed (2 continuous + U = 3); quantised (1 continuous, U = 2, V = 5, 3, 4); all-discrete
CASES = [(3, 20, 4), (2, (3,), (), 30, 1), (1, (2,), (5, 3, 4), 40, 5), (0, (4, 2), (), 25, 1)]
PROB_SEG = [2, 0, 2, 1, 2, 0, 3, 3, 3, 3]
LENS = [2, 1, 3, 4]
ORDER = [3, 2, 0, 1]                                     # chain length descending
DC, DK, DQ, TOTV = [3, 2, 1, 0], [0, 1, 1, 2], [0, 0, 3, 0], [0, 0, 12, 0]
C_HOST = 5000


def _models():
    """(models, centres) of CASES."""
    models, centres = [], []
    for case in CASES:
        if len(case) == 3:
            models.append(R.seeded_case(*case)[:4])
            centres.append(None)
            continue
        below, above, low, high, psig, ps, sb, sa, edges = X.seeded_case(*case)
        models.append((below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                       Q.quants_of(below, above, edges)))
        centres.append(X.centres_of(case[2]) or None)
    return models, centres


def _blobs(prob_seg=PROB_SEG):
    models, centres = _models()
    b = JP.segment_blob(models, [7, 8, 9, 10], prob_seg, np.arange(len(prob_seg)), C_HOST, None, N.JOINT_MSEG_DTYPE)
    return models, centres, b, JP.liar_msegment_blob(models, b.segs, JP.liar_weight_sums(True, models), b.prob_seg,
                                                     centres)


def test_liar_msegment_blob_on_the_four_group_example():
    models, centres, b, lb = _blobs()
    segs = lb.segs
    assert segs.dtype == N.JOINT_LIAR_MSEG_DTYPE
    assert lb.order.tolist() == ORDER and segs['chain_len'].tolist() == LENS
    assert segs['chain_first'].tolist() == [7, 9, 4, 0]
    assert lb.chain.tolist() == [6, 7, 8, 9, 0, 2, 4, 1, 5, 3]      # slot -> problem, chain by chain in that order
    assert segs['n_dims'].tolist() == DC and segs['n_cat'].tolist() == DK and segs['n_quant'].tolist() == DQ
    assert segs['n_lattice'].tolist() == TOTV
    ls = [2 * dc + 1 + dk + dq for dc, dk, dq in zip(DC, DK, DQ)]   # doubles of a liar row: 7, 6, 7, 3
    row = tab = sig = 0
    for s in ORDER:                                                 # the running sums, in the order of the chains
        assert (segs['row_off'][s], segs['tab_off'][s], segs['sigma_off'][s]) == (row, tab, sig), s
        row, tab, sig = row + LENS[s] * ls[s], tab + LENS[s] * TOTV[s], sig + LENS[s] * (DC[s] + DQ[s])
    assert lb.n_sigma == sig == 2 * 3 + 1 * 2 + 3 * 4
    for f in ('above_mu', 'k_above'):
        assert (segs[f] == b.segs[f]).all(), f
    assert (segs['n_trials'] == segs['k_above'] - 1).all()
    for s in range(4):
        W = segs['w_sum'][s]
        assert W == JP.liar_weight_sums(True, models)[s] and segs['log_w'][s] == math.log(W)
        assert [lb.log_norm[segs['chain_first'][s] + j] for j in range(LENS[s])] == \
            [math.log1p(j / W) for j in range(LENS[s])]
        above, low, high, cats, quants = JP.seg_parts(models[s])[1:6]
        psig = list(np.asarray(above[2], dtype=np.float64).reshape(len(above[0]), DC[s])[0]) + \
            [float(q[3][0]) for q in quants]
        assert segs['psig'][s].tolist() == psig + [1.0] * (N.JOINT_MAX_DIMS - len(psig))
        assert segs['low'][s][:DC[s]].tolist() == list(low) and np.isneginf(segs['low'][s][DC[s]:]).all()
        assert segs['high'][s][:DC[s]].tolist() == list(high) and np.isposinf(segs['high'][s][DC[s]:]).all()
    # the f64 pool of this call: per group, in the order of the chains, miss, bonus, centres
    pool = lb.blob[lb.offs[2]:lb.offs[3]].view(np.float64)
    assert len(pool) == lb.n_pool == (4 + 2) * 2 + (2 * 2 + 12) + 3 * 2
    fill = 0
    for s in ORDER:
        cats = JP.seg_parts(models[s])[4]
        if cats:
            tabs = [J.liar_cat_tables(c[2], c[4]) for c in cats]
            for field, i in (('cat_miss', 0), ('cat_bonus', 1)):
                want = np.concatenate([t[i] for t in tabs])
                assert segs[field][s] == fill
                assert pool[fill:fill + len(want)].tobytes() == want.tobytes(), (s, field)
                fill += len(want)
            assert segs['cat_upper'][s].tolist() == b.segs['cat_upper'][s].tolist()
            assert segs['cat_off'][s].tolist() == b.segs['cat_off'][s].tolist()
        if DQ[s]:
            want = np.concatenate(centres[s])
            assert segs['quant_centre'][s] == fill and pool[fill:fill + len(want)].tobytes() == want.tobytes()
            fill += len(want)
            assert segs['quant_v'][s].tolist() == [5, 3, 4, 0] and segs['quant_tab_off'][s].tolist() == [0, 5, 8, 0]
            for f in ('quant_edge_off', 'n_edges', 'above_qmu', 'quant_edges'):
                assert np.array_equal(segs[f][s], b.segs[f][s]), f
    assert fill == lb.n_pool
    assert [int(o) for o in lb.offs] == [0, 4 * 592, 4 * 592 + 80, 4 * 592 + 80 + 8 * lb.n_pool,
                                         4 * 592 + 80 + 8 * lb.n_pool + 16, len(lb.blob)]
    assert len(JP.LIAR_MSECTIONS) == len(lb.offs) - 1


def test_liar_msegment_blob_rejects_bad_centres():
    models, centres, b, _ = _blobs()
    W = JP.liar_weight_sums(True, models)
    for bad, msg in ((None, 'needs centres'), (centres[:3], 'one entry per group'),
                     (centres[:2] + [centres[2][:2]] + [None], 'needs centres'),
                     (centres[:2] + [[np.arange(5.0), np.arange(3.0), np.arange(5.0)]] + [None], 'one finite value'),
                     (centres[:2] + [[np.arange(5.0), np.arange(3.0), np.array([0, 1, np.nan, 3])]] + [None],
                      'one finite value'),
                     ([[np.arange(3.0)]] + centres[1:], 'without a quantised')):
        with pytest.raises(ValueError, match=msg):
            JP.liar_msegment_blob(models, b.segs, W, b.prob_seg, bad)


# ----------------------------------------------------- argument checks, no GPU
class _Host(object):
    """Complete arguments whose pointers are host arrays: only good for calls
    that return before any launch."""

    def __init__(self, prob_seg=PROB_SEG):
        models, centres, self.b, self.lb = _blobs(prob_seg)
        self.pool = np.zeros(64, dtype=np.float64)
        self.out = np.zeros(1 << 16, dtype=np.uint8)
        a = self.a = N.JointLiarMSegArgs()
        a.n_segs, a.n_probs, a.n_cand = len(models), len(prob_seg), C_HOST
        a.segs = a.host_segs = self.lb.segs.ctypes.data
        a.order = a.host_order = self.lb.order.ctypes.data
        a.chain = a.host_chain = self.lb.chain.ctypes.data
        a.log_norm = a.host_log_norm = self.lb.log_norm.ctypes.data
        a.host_prob_seg = self.b.prob_seg.ctypes.data
        a.cand = a.l_out = a.g_out = a.cand_off = a.pool_f32 = a.pool_f64 = a.liar_pool = self.pool.ctypes.data
        a.pool_f32_len, a.pool_f64_len, a.liar_pool_len = self.b.n32, self.b.n64, self.lb.n_pool

    def need(self, lib):
        nb = ctypes.c_uint64(0)
        assert lib.tpe_joint_liar_mseg_scratch_bytes(self.lb.segs.ctypes.data, self.a.n_segs, self.a.n_cand,
                                                     ctypes.byref(nb)) == 0
        return nb.value

    def call(self, lib, nbytes=None, args=True, picks=True, z=True, sigma=True, scratch=True):
        p = self.out.ctypes.data
        return lib.tpe_joint_liar_mseg(ctypes.byref(self.a) if args else None, p if picks else None, p if z else None,
                                       p if sigma else None, p if scratch else None,
                                       self.out.nbytes if nbytes is None else nbytes, None)


def test_the_packed_arguments_pass_every_check_but_the_scratch_size():
    """The packer's own output is what the library accepts: with one byte of
    scratch too few the call gets as far as the last check."""
    lib, h = N.load(), _Host()
    need = h.need(lib)
    assert need == sum(L * (2 * dc + 1 + dk + dq + v) for L, dc, dk, dq, v in zip(LENS, DC, DK, DQ, TOTV)) * 8 + \
        4 * 5 * 24
    assert h.call(lib, nbytes=need - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert h.call(lib, scratch=False) == -1 and b'scratch too small' in lib.tpe_last_error()
    h = _Host([2, 0, 2])                                   # groups without a problem are legal
    assert h.call(lib, nbytes=h.need(lib) - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    assert h.need(lib) == (2 * (7 + 12) + 7) * 8 + 2 * 5 * 24


def test_scratch_bytes_formula_and_its_checks():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    for lens, dims, Cn in (((1,), ((1, 0, 0, 0),), 1),
                           ((8, 3, 1, 0, 2), ((3, 0, 0, 0), (2, 1, 0, 0), (0, 0, 2, 259), (16, 0, 0, 0), (8, 4, 4, 512)),
                            4096),
                           ((34, 2, 5), ((1, 1, 1, 5), (0, 2, 0, 0), (5, 0, 0, 0)), 1500),
                           ((16, 16, 16, 16), ((2, 1, 1, 32),) * 4, 1 << 20), ((0, 0), ((2, 0, 0, 0), (0, 1, 0, 0)), 7)):
        segs = np.zeros(len(lens), dtype=N.JOINT_LIAR_MSEG_DTYPE)
        segs['chain_len'] = lens
        for s, (dc, dk, dq, v) in enumerate(dims):
            segs['n_dims'][s], segs['n_cat'][s], segs['n_quant'][s], segs['n_lattice'][s] = dc, dk, dq, v
        assert lib.tpe_joint_liar_mseg_scratch_bytes(segs.ctypes.data, len(lens), Cn, ctypes.byref(nb)) == 0
        active = sum(L > 0 for L in lens)
        assert nb.value == sum(L * (2 * dc + 1 + dk + dq + v) for L, (dc, dk, dq, v) in zip(lens, dims)) * 8 + \
            active * -(-Cn // N.JOINT_CHUNK) * 24
    segs = np.zeros(2, dtype=N.JOINT_LIAR_MSEG_DTYPE)
    segs['chain_len'], segs['n_dims'] = 1, 2
    ok = (segs.ctypes.data, 2, 8, ctypes.byref(nb))
    assert lib.tpe_joint_liar_mseg_scratch_bytes(*ok) == 0
    for i, v in ((0, None), (1, 0), (2, 0), (3, None)):
        bad = list(ok)
        bad[i] = v
        assert lib.tpe_joint_liar_mseg_scratch_bytes(*bad) == -1, (i, v)
        assert b'tpe_joint_liar_mseg_scratch_bytes' in lib.tpe_last_error()
    for edit in (dict(n_dims=0), dict(n_dims=17), dict(chain_len=-1), dict(n_cat=-1), dict(n_quant=-1),
                 dict(n_cat=1, n_dims=9), dict(n_cat=5), dict(n_quant=5, n_lattice=10), dict(n_quant=1),
                 dict(n_lattice=4), dict(n_quant=2, n_lattice=513)):
        segs[1] = segs[0]
        for field, v in edit.items():
            segs[field][1] = v
        assert lib.tpe_joint_liar_mseg_scratch_bytes(*ok) == -1, edit
    segs[1] = segs[0]
    assert lib.tpe_joint_liar_mseg_scratch_bytes(*ok) == 0


@pytest.mark.parametrize('field,value,msg', [
    ('n_segs', 0, b'< 1'), ('n_probs', 0, b'< 1'), ('n_cand', 0, b'< 1'),
    ('segs', None, b'null segs'), ('host_segs', None, b'null segs'), ('order', None, b'null segs'),
    ('host_order', None, b'null segs'), ('chain', None, b'null segs'), ('host_chain', None, b'null segs'),
    ('log_norm', None, b'null segs'), ('host_log_norm', None, b'null segs'), ('host_prob_seg', None, b'null segs'),
    ('cand', None, b'null cand'), ('cand_off', None, b'null cand'), ('l_out', None, b'null cand'),
    ('g_out', None, b'null cand'), ('pool_f32', None, b'null cand'),
    ('pool_f64', None, b'leaves pool_f64'), ('pool_f64_len', 10, b'leaves pool_f64'),
    ('liar_pool', None, b'leaves liar_pool'), ('liar_pool_len', 3, b'leaves liar_pool'),
    ('pool_f32_len', 5, b'above_mu'),
])
def test_bad_arguments_are_rejected_before_any_launch(field, value, msg):
    lib, h = N.load(), _Host()
    setattr(h.a, field, value)
    assert h.call(lib) == -1, field
    assert msg in lib.tpe_last_error(), (field, lib.tpe_last_error())


@pytest.mark.parametrize('field,seg,value,msg', [
    ('n_dims', 0, 0, b'n_dims outside'), ('n_dims', 0, 17, b'n_dims outside'), ('n_dims', 1, -1, b'< 0'),
    ('n_cat', 0, -1, b'< 0'), ('n_quant', 3, -1, b'< 0'),
    ('n_dims', 1, 9, b'TPE_JOINT_MSEG_MAX_CONT'), ('n_cat', 3, 5, b'TPE_JOINT_MSEG_MAX_CAT'),
    ('n_quant', 2, 5, b'TPE_JOINT_MAX_QUANT'),
    ('k_above', 1, 0, b'k_above'), ('n_trials', 2, -1, b'n_trials'), ('w_sum', 0, 0.0, b'w_sum'),
    ('w_sum', 3, float('nan'), b'w_sum'), ('w_sum', 1, float('inf'), b'w_sum'),
    ('above_mu', 2, -1, b'above_mu'), ('above_mu', 0, 1 << 40, b'above_mu'),
    ('log_w', 2, 0.123, b'log_w'),
    ('cat_miss', 1, -1, b'cat_miss / cat_bonus'), ('cat_bonus', 3, 1 << 40, b'cat_miss / cat_bonus'),
    ('n_lattice', 2, 11, b'n_lattice'), ('n_lattice', 1, 2, b'n_lattice'),
    ('quant_edges', 2, -1, b'leaves pool_f64'), ('quant_edges', 2, 1 << 40, b'leaves pool_f64'),
    ('above_qmu', 2, -1, b'leaves pool_f64'), ('above_qmu', 2, 1 << 40, b'leaves pool_f64'),
    ('n_edges', 2, 14, b'quant_edge_off'),
    ('quant_centre', 2, -1, b'quant_centre'), ('quant_centre', 2, 1 << 40, b'quant_centre'),
    ('chain_len', 2, 2, b'partition'), ('chain_len', 1, 2, b'partition'), ('chain_first', 0, 4, b'partition'),
    ('row_off', 0, 0, b'running sum'), ('tab_off', 1, 0, b'running sum'), ('sigma_off', 0, 0, b'running sum'),
])
def test_bad_descriptors_are_rejected_before_any_launch(field, seg, value, msg):
    lib, h = N.load(), _Host()
    h.lb.segs[field][seg] = value
    assert h.call(lib) == -1, (field, seg, value)
    assert msg in lib.tpe_last_error(), (field, lib.tpe_last_error())


@pytest.mark.parametrize('field,seg,dim,value,msg', [
    ('psig', 0, 2, 0.0, b'prior sigma'), ('psig', 2, 0, -1.0, b'prior sigma'),
    ('psig', 2, 3, float('nan'), b'prior sigma'),            # quantised dimension 2 of group 2: psig[n_dims + 2]
    ('cat_upper', 1, 0, 1, b'U_d'), ('cat_upper', 3, 1, 257, b'U_d'),
    ('cat_off', 3, 1, -1, b'cat_off'), ('cat_off', 3, 1, 5, b'cat_off'),
    ('quant_v', 2, 1, 1, b'V_d'), ('quant_v', 2, 0, 257, b'V_d'),
    ('quant_tab_off', 2, 1, 4, b'quant_tab_off'), ('quant_tab_off', 2, 0, 1, b'quant_tab_off'),
    ('quant_edge_off', 2, 0, -1, b'quant_edge_off'), ('quant_edge_off', 2, 2, 11, b'quant_edge_off'),
])
def test_bad_per_dimension_entries_are_rejected_before_any_launch(field, seg, dim, value, msg):
    lib, h = N.load(), _Host()
    h.lb.segs[field][seg][dim] = value
    assert h.call(lib) == -1, (field, seg, dim, value)
    assert msg in lib.tpe_last_error(), (field, lib.tpe_last_error())


def test_null_outputs_lattice_total_chain_tables_and_entries_that_are_not_read():
    lib = N.load()
    h = _Host()
    assert h.call(lib, args=False) == -1 and b'null args' in lib.tpe_last_error()
    for kw in (dict(picks=False), dict(z=False), dict(sigma=False)):
        assert h.call(lib, **kw) == -1 and b'null outputs' in lib.tpe_last_error(), kw
    h = _Host()                                             # 256 + 256 + 4 lattice values
    h.lb.segs['quant_v'][2][:3], h.lb.segs['quant_tab_off'][2][:3] = [256, 256, 4], [0, 256, 512]
    assert h.call(lib) == -1 and b'TPE_JOINT_MAX_LATTICE_TOTAL' in lib.tpe_last_error()
    h = _Host()                                             # beyond the counts: not read
    h.lb.segs['psig'][2][4] = 0.0
    h.lb.segs['cat_upper'][1][1] = 999
    h.lb.segs['quant_v'][2][3] = 999
    h.lb.segs['quant_centre'][0] = h.lb.segs['cat_miss'][0] = h.lb.segs['above_qmu'][1] = -5
    assert h.call(lib, nbytes=h.need(lib) - 1) == -1 and b'scratch too small' in lib.tpe_last_error()
    for edit in (lambda h: h.lb.chain.__setitem__(slice(0, 2), [7, 6]),
                 lambda h: h.lb.chain.__setitem__(slice(3, 5), [0, 9]),
                 lambda h: h.lb.chain.__setitem__(1, 6),
                 lambda h: h.lb.chain.__setitem__(5, 10),
                 lambda h: h.lb.order.__setitem__(slice(0, 2), [2, 3]),
                 lambda h: h.lb.order.__setitem__(3, 0),
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
MIXED_KW = {2: dict(joint=True, joint_branches=True, joint_discrete=True, joint_branches_mixed=True),
            3: dict(joint=True, joint_branches=True, joint_quantized=True, joint_branches_mixed=True)}


def test_the_mode():
    from hyperopt_amd import tpe
    assert tpe._joint_liar_mode('branches_mixed') == 'branches_mixed'
    assert tpe._joint_liar_mode('branches') == 'branches' and tpe._joint_liar_mode('mixed') == 'mixed'
    assert tpe._joint_liar_mode(True) is True and tpe._joint_liar_mode(False) is None
    for bad in ('other', 'branch', 'branch_mixed', 'mixed_branches', 1, 2.5):
        with pytest.raises(ValueError, match="True or 'mixed'"):
            tpe._joint_liar_mode(bad)
    with pytest.raises(ValueError, match="'branches' with joint_branches"):
        tpe._joint_liar_mode('other')
    with pytest.raises(ValueError, match="'branches_mixed' with joint_branches"):
        tpe._joint_liar_mode('other')


@pytest.mark.parametrize('which,kw,match', [
    (2, dict(joint_branches=True, joint_discrete=True, joint_branches_mixed=True), 'needs joint'),
    (2, dict(MIXED_KW[2], joint_shard=(0, 2)), 'joint_shard'),
    (3, dict(MIXED_KW[3], joint_shard=(1, 2)), 'joint_shard'),
    (1, dict(joint=True), "joint_liar='branches_mixed' needs joint_branches=True"),
    (0, dict(joint=True), "joint_liar='branches_mixed' needs joint_branches=True"),
])
def test_suggest_rejects_before_any_device_use_or_startup_draw(which, kw, match, monkeypatch):
    from hyperopt_amd import base, history, tpe
    SH._no_device(monkeypatch)
    domain = SH._domain(SH._spaces()[which])
    with pytest.raises(ValueError, match=match):
        tpe.suggest([0, 1], domain, base.Trials(), 1234, joint_liar='branches_mixed', **kw)
    with pytest.raises(ValueError, match=match):
        tpe.suggest_choices(domain.table, history.extract(domain, base.Trials()), [0, 1], 1234,
                            joint_liar='branches_mixed', **kw)


@pytest.mark.parametrize('which', [2, 3])
def test_branches_still_refuses_mixed_branch_groups(which, monkeypatch):
    from hyperopt_amd import base, tpe
    SH._no_device(monkeypatch)
    with pytest.raises(ValueError, match='joint_branches_mixed.*discrete or quantised'):
        tpe.suggest([0, 1], SH._domain(SH._spaces()[which]), base.Trials(), 1234, joint_liar='branches',
                    **MIXED_KW[which])


@pytest.mark.parametrize('which,kw', [
    (2, MIXED_KW[2]),                                               # a branch group with a discrete label
    (3, MIXED_KW[3]),                                               # a branch group with a quantised label
    (1, dict(joint=True, joint_branches=True)),                     # continuous branch groups: 'branches'
    (1, dict(joint=['a', 'b', 'u', 'v'], joint_branches=True)),     # no root group
    (0, dict(joint=True, joint_branches=True)),                     # no branch group in the space: 'mixed'
])
def test_branches_mixed_gets_past_the_checks_to_the_startup_draw(which, kw, monkeypatch):
    from hyperopt_amd import base, tpe
    SH._no_device(monkeypatch)

    def startup(*a, **k):
        raise SH._Startup()
    monkeypatch.setattr(tpe.rand, 'suggest', startup)
    with pytest.raises(SH._Startup):
        tpe.suggest([0, 1], SH._domain(SH._spaces()[which]), base.Trials(), 1234, joint_liar='branches_mixed', **kw)


def test_signatures_stand():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import Engine
    for fn in (tpe.suggest, tpe.suggest_choices):
        pars = inspect.signature(fn).parameters
        assert list(pars)[-1] == 'joint_liar' and pars['joint_liar'].default is False
    pars = inspect.signature(Engine.run_joint_msegments_liar).parameters
    assert list(pars) == ['self', 'models', 'stream_words', 'prob_seg', 'prob_id', 'n_cand', 'seed', 'liar', 'centres',
                          'inject', 'return_cand', 'want_lg', 'return_sigma']
    assert pars['liar'].default is True and pars['centres'].default is None and pars['inject'].default is None
    assert all(pars[k].default is False for k in ('return_cand', 'want_lg', 'return_sigma'))
    assert 'shard' not in pars and 'report_k' not in pars
    assert list(inspect.signature(JP.liar_msegment_blob).parameters) == ['models', 'segs', 'weight_sums', 'prob_seg',
                                                                         'centres']


def test_engine_checks_come_before_any_device_use(monkeypatch):
    from hyperopt_amd.engine import Engine
    monkeypatch.setattr(N, 'load', lambda *a, **kw: pytest.fail('the library was loaded'))
    eng = Engine.__new__(Engine)                             # no device, no library: the checks come first
    models, centres = _models()
    for W in ([1.0, 0.0, 1.0, 1.0], [1.0], 3.5, False):
        with pytest.raises(ValueError, match='weight sum'):
            eng.run_joint_msegments_liar(models, [1, 2, 3, 4], [0, 1, 2, 3], [5, 6, 7, 8], 64, 3, liar=W,
                                         centres=centres)
    with pytest.raises(ValueError, match='needs centres'):
        eng.run_joint_msegments_liar(models, [1, 2, 3, 4], [0, 1, 2, 3], [5, 6, 7, 8], 64, 3)
    with pytest.raises(ValueError, match='centres without a quantised'):
        eng.run_joint_msegments_liar(models[:1], [1], [0, 0], [5, 6], 64, 3, centres=[[np.arange(3.0)]])


# ------------------------------------------- the tie cap, on the reference alone
@pytest.mark.parametrize('case,length', G.CAPPED)
def test_the_reference_chain_keeps_the_tie_cap(case, length):
    """What tests/test_gpu_joint_liar_mseg.py caps on the device holds for the
    numpy reference's own greedy chain: distinct picks, at most MAX_TIES
    near-ties a step, with the W the GPU test passes."""
    c = X.case_inputs(*case, C=G.C)
    W = LR.weight_sum(len(c['above'][0]) - 1)
    steps = X.greedy(X.chain_of(c, W=W), c['cand'], c['l'], c['g'], length)
    assert max(len(ties) for _, ties, _, _ in steps) <= G.MAX_TIES, [len(s[1]) for s in steps]
    assert len(set(pick for _, _, _, pick in steps)) == length
