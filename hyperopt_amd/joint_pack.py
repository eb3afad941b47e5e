"""Host-side packing of the joint stages (DESIGN.md "Joint TPE"): numpy only.

``group_rows`` validates one joint group and turns it into its device rows;
every stage goes through it, so a group's rows in a segmented blob are the
bytes of its solo run by construction.  ``segment_blob`` lays the groups of a
segmented stage out in one upload.  Engine.run_joint* upload what these return
and make the native call.

The dimension limits by entry point (``_check_dims``):
  'run'      run_joint             1 <= D <= JOINT_MAX_DIMS, continuous only
  'wide'     run_joint_wide        1 <= D <= JOINT_WIDE_MAX_DIMS, continuous only
  'mixed'    run_joint_mixed       Dk >= 1, Dc + Dk <= JOINT_MAX_DIMS
  'wide_mixed' run_joint_wide_mixed  1 <= Dk <= JOINT_WIDE_MAX_CAT, Dq = 0, 1 <= Dc + Dk <= JOINT_WIDE_MAX_DIMS
  'quant'    run_joint_quant       Dq >= 1, Dc <= JOINT_QUANT_MAX_CONT, Dk <= JOINT_QUANT_MAX_DISC
  'wide_quant' run_joint_wide_quant  Dq >= 1, Dc >= 1, Dk <= JOINT_WIDE_MAX_CAT, 2 <= Dc + Dk + Dq <= JOINT_WIDE_MAX_DIMS
  'segment'  run_joint_segments    a continuous group 1 <= Dc <= JOINT_MAX_DIMS; one with discrete or
                                   quantised parts Dc <= JOINT_MSEG_MAX_CONT, Dk <= JOINT_MSEG_MAX_CAT
  'wide_segment' run_joint_wide_segments  1 <= Dc <= JOINT_WIDE_MAX_DIMS, continuous only
and Dq <= JOINT_MAX_QUANT everywhere.
"""
import collections

import numpy as np

from . import _native as N
from . import joint as J

SIDES = ('below', 'above')

# The rows of a group in the order they go into the pools of a segmented stage:
# (key in group_rows' dict, field of the args struct / descriptor, name of the
# solo stages' buffer, dtype, the part of the group the row belongs to).
# Dk = 0 leaves the 'cat' rows out, Dq = 0 the 'quant' ones.  The 'cont' rows
# are empty arrays when Dc = 0: the pools and run_joint_mixed take them as they
# are, run_joint_quant leaves their pointers null (Engine._joint_solo).
ROWS = tuple((s + f, s + f, s + f, dt, part) for s in SIDES for f, dt, part in (
    ('_mu', np.float32, 'cont'), ('_a', np.float32, 'cont'), ('_c', np.float32, None),
    ('_cat', np.float32, 'cat'), ('_miss', np.float32, 'cat'), ('_bonus', np.float32, 'cat'),
    ('_qmu', np.float64, 'quant'), ('_qsigma', np.float64, 'quant'))) + (
    ('samp', 'samp', 'samp', np.float32, 'cont'), ('cum', 'samp_cum', 'cum', np.float64, None),
    ('below_h', 'below_h', 'cat_h', np.float64, 'cat'), ('cat_cum', 'cat_cum', 'cat_cum', np.float64, 'cat'),
    ('quant_edges', 'quant_edges', 'qedges', np.float64, 'quant'),
    ('quant_samp', 'quant_samp', 'qsamp', np.float32, 'quant'))


_PRESENT = {(cat, quant): tuple(row for row in ROWS if row[4] in (None, 'cont') + ('cat',) * cat + ('quant',) * quant)
            for cat in (False, True) for quant in (False, True)}


def group_rows_present(r):
    """ROWS without the parts the group ``r`` (group_rows) does not have."""
    return _PRESENT[r['Dk'] > 0, r['Dq'] > 0]


def seg_parts(m):
    """(below, above, low, high, cats, quants) of one group of
    run_joint_segments: a model object or a tuple of 4, 5 or 6 entries;
    below / above = (w, mu, sigma)."""
    if hasattr(m, 'below'):
        cats = m.cats() if hasattr(m, 'drows') else []
        quants = m.quants() if hasattr(m, 'qrows') else []
        return m.below[:3], m.above[:3], m.low, m.high, cats, quants
    m = tuple(m)
    return m[0][:3], m[1][:3], m[2], m[3], list(m[4]) if len(m) > 4 else [], list(m[5]) if len(m) > 5 else []


def _check_dims(entry, Dc, Dk, Dq):
    if entry == 'mixed' and Dk == 0:
        raise ValueError('joint stage: no discrete dimension, use run_joint')
    if entry == 'quant' and Dq == 0:
        raise ValueError('joint stage: no quantised dimension, use run_joint_mixed / run_joint')
    if Dq > N.JOINT_MAX_QUANT:
        raise ValueError('joint stage: %d quantised dimensions, at most %d' % (Dq, N.JOINT_MAX_QUANT))
    if entry == 'quant':
        if Dc > N.JOINT_QUANT_MAX_CONT or Dk > N.JOINT_QUANT_MAX_DISC:
            raise ValueError('joint stage: beside a quantised dimension at most %d continuous and %d discrete ones, '
                             'not %d and %d' % (N.JOINT_QUANT_MAX_CONT, N.JOINT_QUANT_MAX_DISC, Dc, Dk))
    elif entry == 'segment' and (Dk or Dq):
        if Dc > N.JOINT_MSEG_MAX_CONT or Dk > N.JOINT_MSEG_MAX_CAT:
            raise ValueError('joint stage: a segment with discrete or quantised dimensions holds at most %d continuous '
                             'and %d discrete ones, not %d and %d'
                             % (N.JOINT_MSEG_MAX_CONT, N.JOINT_MSEG_MAX_CAT, Dc, Dk))
    elif entry == 'wide_quant':
        if Dq == 0:
            raise ValueError('joint stage: no quantised dimension, use run_joint_wide_mixed / run_joint_wide')
        if Dc < 1:
            raise ValueError('joint stage: a wide group with quantised dimensions needs at least 1 continuous one')
        if Dk > N.JOINT_WIDE_MAX_CAT:
            raise ValueError('joint stage: a wide group with quantised dimensions holds at most %d discrete ones, '
                             'not %d' % (N.JOINT_WIDE_MAX_CAT, Dk))
        if Dc + Dk + Dq > N.JOINT_WIDE_MAX_DIMS:
            raise ValueError('joint stage: %d dimensions, at most %d' % (Dc + Dk + Dq, N.JOINT_WIDE_MAX_DIMS))
    elif entry == 'wide_mixed':
        if Dq or not 1 <= Dk <= N.JOINT_WIDE_MAX_CAT:
            raise ValueError('joint stage: a wide group with discrete dimensions holds 1 to %d of them and no '
                             'quantised one, not %d and %d' % (N.JOINT_WIDE_MAX_CAT, Dk, Dq))
        if not 1 <= Dc + Dk <= N.JOINT_WIDE_MAX_DIMS:
            raise ValueError('joint stage: %d dimensions, at most %d' % (Dc + Dk, N.JOINT_WIDE_MAX_DIMS))
    elif entry == 'wide_segment' and (Dk or Dq):
        raise ValueError('joint stage: a wide segment holds continuous dimensions only, not %d discrete and %d '
                         'quantised ones' % (Dk, Dq))
    else:
        top = N.JOINT_WIDE_MAX_DIMS if entry in ('wide', 'wide_segment') else N.JOINT_MAX_DIMS
        if not 1 <= Dc + Dk <= top:
            raise ValueError('joint stage: %d dimensions, at most %d' % (Dc + Dk, top))


def group_rows(below, above, low, high, cats=(), quants=(), entry='segment'):
    """Validate one joint group and make its device rows: ``below`` / ``above``
    = (w [K], mu [K, Dc], sigma [K, Dc]), ``low`` / ``high`` [Dc], ``cats`` and
    ``quants`` as Engine.run_joint_mixed / run_joint_quant take them; ``entry``
    names the limits (the module docstring).  Returns a dict: Dc, Dk, Dq,
    k_below, k_above, low, high, the rows of ROWS that the group has (the
    functions of joint.py give them), below_base / above_base, and with
    categories cat_upper / cat_off, with lattices quant_v / quant_edge_off,
    n_lattice (sum V) and the lattice ends qlow / qhigh."""
    low, high = np.asarray(low, dtype=np.float64).reshape(-1), np.asarray(high, dtype=np.float64).reshape(-1)
    Dc, Dk, Dq = len(low), len(cats), len(quants)
    _check_dims(entry, Dc, Dk, Dq)
    edges = [np.ascontiguousarray(q[4], dtype=np.float64).reshape(-1) for q in quants]
    vs = [len(e) - 1 for e in edges]
    for e in edges:
        if not 2 <= len(e) - 1 <= N.JOINT_MAX_LATTICE:
            raise ValueError('joint stage: %d lattice values, outside [2, %d]' % (len(e) - 1, N.JOINT_MAX_LATTICE))
        if not (np.isfinite(e).all() and (np.diff(e) > 0).all()):
            raise ValueError('joint stage: the lattice edges must be finite and strictly increasing')
    if sum(vs) > N.JOINT_MAX_LATTICE_TOTAL:
        raise ValueError('joint stage: %d lattice values in the group, at most %d'
                         % (sum(vs), N.JOINT_MAX_LATTICE_TOTAL))
    ps = [np.asarray(c[2], dtype=np.float64).reshape(-1) for c in cats]
    ups = [len(p) for p in ps]
    for p in ps:
        if not 2 <= len(p) <= N.JOINT_MAX_CATS:
            raise ValueError('joint stage: %d categories, outside [2, %d]' % (len(p), N.JOINT_MAX_CATS))
        if not (p > 0).all():
            raise ValueError('joint stage: a prior probability of 0')
    if sum(ups) > N.JOINT_MAX_CAT_TOTAL:
        raise ValueError('joint stage: %d categories in the group, at most %d' % (sum(ups), N.JOINT_MAX_CAT_TOTAL))
    s_side = [np.array([float(c[3 + i]) for c in cats]) for i in (0, 1)]
    if Dk and not all((s > 0).all() and np.isfinite(s).all() for s in s_side):
        raise ValueError('joint stage: the smoothing masses must be positive')
    r = dict(Dc=Dc, Dk=Dk, Dq=Dq, low=low, high=high)
    for i, (name, side) in enumerate(zip(SIDES, (below, above))):
        w = np.asarray(side[0], dtype=np.float64)
        mu = np.asarray(side[1], dtype=np.float64).reshape(len(w), -1)
        sigma = np.asarray(side[2], dtype=np.float64).reshape(len(w), -1)
        if mu.shape != (len(w), Dc) or sigma.shape != mu.shape:
            raise ValueError('joint stage: mixture shapes do not match %d dimensions' % Dc)
        cols = [np.asarray(c[i], dtype=np.int64).reshape(-1) for c in cats]
        qmu = [np.asarray(q[2 * i], dtype=np.float64).reshape(-1) for q in quants]
        qsig = [np.asarray(q[2 * i + 1], dtype=np.float64).reshape(-1) for q in quants]
        if any(len(col) != len(w) for col in cols + qmu + qsig):
            raise ValueError('joint stage: one category / (mu, sigma) per component and dimension')
        for col, U in zip(cols, ups):
            if col.min() < -1 or col.max() >= U:
                raise ValueError('joint stage: a component category outside [-1, %d)' % U)
        if Dk:
            (r[name + '_mu'], r[name + '_a'], r[name + '_c'], r[name + '_base'], r[name + '_cat'], r[name + '_miss'],
             r[name + '_bonus']) = J.mixed_density_rows(w, mu, sigma, low, high, np.stack(cols, axis=1), ps, s_side[i])
        else:
            r[name + '_mu'], r[name + '_a'], r[name + '_c'], r[name + '_base'] = J.density_rows(w, mu, sigma, low, high)
        if Dq:
            qsig = np.stack(qsig, axis=1)
            if not ((qsig > 0).all() and np.isfinite(qsig).all()):
                raise ValueError('joint stage: the quantised bandwidths must be positive')
            r[name + '_qmu'], r[name + '_qsigma'] = np.stack(qmu, axis=1), qsig
        r['k_' + name] = len(w)
        if i == 0:                                   # the sampler draws from the below side
            if Dk:
                r['cum'], r['samp'], r['below_h'], r['cat_cum'] = J.mixed_sampler_rows(w, mu, sigma, low, high, ps,
                                                                                       s_side[0])
            else:
                r['cum'], r['samp'] = J.sampler_rows(w, mu, sigma, low, high)
            if Dq:
                r['qlow'], r['qhigh'] = np.array([e[0] for e in edges]), np.array([e[-1] for e in edges])
                r['quant_samp'] = J.sampler_rows(w, r['below_qmu'], qsig, r['qlow'], r['qhigh'])[1]
    if Dk:
        r['cat_upper'], r['cat_off'] = ups, [int(x) for x in np.cumsum([0] + ups[:-1])]
    if Dq:
        r['quant_edges'], r['n_lattice'] = np.concatenate(edges), sum(vs)
        r['quant_v'], r['quant_edge_off'] = vs, [int(x) for x in np.cumsum([0] + [v + 1 for v in vs[:-1]])]
    return r


def inject_rows(inject, C, D):
    """The candidates to score instead of sampling, f32 [C, D]."""
    inj = np.ascontiguousarray(inject, dtype=np.float32)
    if inj.shape != (C, D):
        raise ValueError('joint stage: inject must be [n_cand, %d]' % D)
    return inj


# What segment_blob returns.  blob: the one upload (None for an empty part of a
# sharded stage, n_cand = 0); offs: where its sections start, in the order
# SECTIONS; segs: the descriptors on the host; prob_seg: the int32 problem list
# on the host; cand_off [P + 1]; widths [P]: D of every problem's group; n32 /
# n64: the pools' element counts; n_table: the f32 elements of the quantised
# tables.
SegmentBlob = collections.namedtuple('SegmentBlob', 'blob offs segs prob_seg cand_off widths n32 n64 n_table')
# one blob: the 8-byte items first, then the 4-byte ones
SECTIONS = ('segs', 'pool_f64', 'prob_id', 'cand_off', 'pool_f32', 'prob_seg')


def segment_blob(models, stream_words, prob_seg, prob_id, n_cand, inject, seg_dtype, empty_ok=False):
    """The upload of a segmented stage (Engine.run_joint_segments' arguments):
    per group its descriptor (``seg_dtype``: N.JOINT_SEG_DTYPE, continuous
    groups only, N.JOINT_WIDE_SEG_DTYPE, continuous groups of up to
    JOINT_WIDE_MAX_DIMS labels, or N.JOINT_MSEG_DTYPE) and its group_rows in the two pools,
    in the order of ROWS with the group's inject rows last; a continuous group
    is the case Dk = Dq = 0.  The descriptors carry the f32 bounds
    (joint.f32_bounds), padded with -+inf.  ``empty_ok``: n_cand = 0 is allowed
    (a sharded stage) and gives the widths alone."""
    S, C = len(models), int(n_cand)
    prob_seg = np.ascontiguousarray(prob_seg, dtype=np.int32).reshape(-1)
    prob_id = np.ascontiguousarray(prob_id, dtype=np.int64).reshape(-1)
    P = len(prob_seg)
    if S < 1 or len(stream_words) != S:
        raise ValueError('joint stage: one stream word per group, at least one group')
    if P < 1 or len(prob_id) != P or C < (0 if empty_ok else 1) or C >= 2 ** 31:
        raise ValueError('joint stage: n_cand / problems out of range')
    if prob_seg.min() < 0 or prob_seg.max() >= S:
        raise ValueError('joint stage: a problem names a group outside [0, %d)' % S)
    groups = [seg_parts(m) for m in models]
    if C == 0:                                   # an empty part of a sharded stage: nothing is packed or checked
        widths = [sum(len(x) for x in groups[s][3:]) for s in prob_seg]
        return SegmentBlob(None, None, None, prob_seg, None, widths, 0, 0, 0)
    if inject is not None and len(inject) != S:
        raise ValueError('joint stage: inject must hold one entry per group')
    mixed = 'n_cat' in seg_dtype.names
    entry = 'wide_segment' if seg_dtype['lo'].shape == (N.JOINT_WIDE_MAX_DIMS,) else 'segment'
    segs = np.zeros(S, dtype=seg_dtype)
    pools = {4: [], 8: []}
    fill = {4: 0, 8: 0}

    def put(arr, dtype):
        arr = np.ascontiguousarray(arr, dtype=dtype).reshape(-1)
        size = arr.dtype.itemsize
        pools[size].append(arr)
        fill[size] += arr.size
        return fill[size] - arr.size
    dims = np.empty(S, dtype=np.int64)
    n_table = 0
    for s, group in enumerate(groups):
        r = group_rows(*group, entry=entry)
        Dc, Dk, Dq = r['Dc'], r['Dk'], r['Dq']
        D = dims[s] = Dc + Dk + Dq
        g = segs[s]
        g['n_dims'], g['k_below'], g['k_above'] = Dc, r['k_below'], r['k_above']
        g['stream_word'] = int(stream_words[s])
        g['below_base'], g['above_base'] = r['below_base'], r['above_base']
        for key, field, _, dtype, _ in group_rows_present(r):
            g[field] = put(r[key], dtype)
        g['lo'], g['hi'] = np.float32(-np.inf), np.float32(np.inf)
        g['lo'][:Dc], g['hi'][:Dc] = J.f32_bounds(r['low'], r['high'])
        if mixed:
            g['n_cat'], g['n_quant'] = Dk, Dq
            g['qlo'], g['qhi'] = np.float32(-np.inf), np.float32(np.inf)
        if Dk:
            g['cat_upper'][:Dk], g['cat_off'][:Dk] = r['cat_upper'], r['cat_off']
        if Dq:
            g['quant_v'][:Dq], g['quant_edge_off'][:Dq] = r['quant_v'], r['quant_edge_off']
            g['n_edges'] = r['n_lattice'] + Dq
            g['qlo'][:Dq], g['qhi'][:Dq] = J.f32_bounds(r['qlow'], r['qhigh'])
            g['table'] = n_table
            n_table += (r['k_below'] + r['k_above']) * r['n_lattice']
        g['inject'] = -1
        if inject is not None and inject[s] is not None:
            g['inject'] = put(inject_rows(inject[s], C, D), np.float32)
    if inject is not None and any(inject[s] is None for s in np.unique(prob_seg)):
        raise ValueError('joint stage: inject lacks the candidates of a group that has a problem')
    widths = dims[prob_seg]
    cand_off = np.concatenate([[0], np.cumsum(C * widths)]).astype(np.int64)
    if P * C >= 2 ** 31 or cand_off[-1] >= 2 ** 31:
        raise ValueError('joint stage: %d problems x %d candidates do not fit one run' % (P, C))
    parts = [segs.view(np.uint8), np.concatenate(pools[8]).view(np.uint8), prob_id.view(np.uint8),
             cand_off[:P].view(np.uint8), np.concatenate(pools[4]).view(np.uint8), prob_seg.view(np.uint8)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    return SegmentBlob(np.concatenate(parts), offs, segs, prob_seg, cand_off, widths, fill[4], fill[8], n_table)


# What liar_chains returns.  order [S]: rank -> group, chain length descending,
# ties by group index; first [S]: BY GROUP, its first slot; chain [P]: slot ->
# problem, group after group in that order, a group's problems in the caller's
# order; active [longest chain]: the groups with more than r problems, which
# are order[:active[r]].
LiarChains = collections.namedtuple('LiarChains', 'order first chain active')


def liar_chains(prob_seg, n_segs):
    """The greedy chains of a segmented liar stage (include/tpe_hip.h
    "Batch-aware picks in branch groups"): the chain of group s is its problems
    in the caller's order.  Pure numpy; a group without a problem is legal."""
    prob_seg = np.ascontiguousarray(prob_seg, dtype=np.int32).reshape(-1)
    S = int(n_segs)
    if S < 1 or len(prob_seg) < 1:
        raise ValueError('joint stage: at least one group and one problem')
    if prob_seg.min() < 0 or prob_seg.max() >= S:
        raise ValueError('joint stage: a problem names a group outside [0, %d)' % S)
    lens = np.bincount(prob_seg, minlength=S)
    order = np.argsort(-lens, kind='stable').astype(np.int32)
    first = np.zeros(S, dtype=np.int32)
    first[order] = np.concatenate([[0], np.cumsum(lens[order])[:-1]])
    rank = np.empty(S, dtype=np.int64)
    rank[order] = np.arange(S)
    chain = np.argsort(rank[prob_seg], kind='stable').astype(np.int32)
    active = np.array([(lens > r).sum() for r in range(int(lens.max()))], dtype=np.int32)
    return LiarChains(order, first, chain, active)


# What liar_segment_blob returns.  blob: the one upload; offs: where its
# sections start, in the order LIAR_SECTIONS; segs / order / chain / log_norm:
# the host copies the library checks (segs['sigma_off'][s]: where group s's
# [L_s, D_s] rows start in liar_sigma); n_sigma: the doubles of liar_sigma.
LiarSegmentBlob = collections.namedtuple('LiarSegmentBlob', 'blob offs segs order chain log_norm n_sigma')
LIAR_SECTIONS = ('segs', 'log_norm', 'order', 'chain')


def liar_weight_sums(liar, models):
    """The un-normalised weight sum W_s of every group's above side: ``liar``
    True takes 1 / w[-1] (the newest trial weighs 1; a side without trials: 1),
    as Engine.run_joint does; a sequence gives one positive finite W_s per
    group.  ValueError for anything else."""
    S = len(models)
    if isinstance(liar, (bool, np.bool_)):
        if not liar:
            raise ValueError('joint stage: liar must be True or one positive weight sum W per group')
        out = []
        for m in models:
            w = np.asarray(seg_parts(m)[1][0], dtype=np.float64)
            out.append(1.0 / float(w[-1]) if len(w) > 1 else 1.0)
        return out
    try:
        out = [float(x) for x in liar]
    except TypeError:
        raise ValueError('joint stage: liar must be True or one positive weight sum W per group: %r' % (liar,))
    if len(out) != S or not all(x > 0 and np.isfinite(x) for x in out):
        raise ValueError('joint stage: liar must be True or one positive weight sum W per group: %r' % (liar,))
    return out


def liar_segment_blob(models, segs, weight_sums, prob_seg):
    """The upload of a segmented liar stage after a segmented stage over the
    same ``models`` and ``prob_seg``: per group its descriptor
    (N.JOINT_LIAR_SEG_DTYPE; ``segs``: that stage's descriptors, whose above_mu
    offsets it shares), the chains (liar_chains) and log1p(j / W_s) by slot.
    log W_s and log1p come from the C library (math), as tpe_joint_liar takes
    them; the library rejects any other bits."""
    import math
    S = len(models)
    ch = liar_chains(prob_seg, S)
    out = np.zeros(S, dtype=N.JOINT_LIAR_SEG_DTYPE)
    lens = np.bincount(np.asarray(prob_seg, dtype=np.int64), minlength=S)
    log_norm = np.zeros(len(ch.chain), dtype=np.float64)
    row = sig = 0
    for s in ch.order:
        above, low, high = seg_parts(models[s])[1:4]
        D, g, W = int(segs[s]['n_dims']), out[s], float(weight_sums[s])
        g['n_dims'], g['k_above'], g['n_trials'] = D, segs[s]['k_above'], segs[s]['k_above'] - 1
        g['chain_len'], g['chain_first'] = lens[s], ch.first[s]
        g['w_sum'], g['log_w'], g['above_mu'] = W, math.log(W), segs[s]['above_mu']
        g['row_off'], g['sigma_off'] = row, sig
        g['psig'], g['low'], g['high'] = 1.0, -np.inf, np.inf
        g['psig'][:D] = np.asarray(above[2], dtype=np.float64).reshape(-1, D)[0]
        g['low'][:D], g['high'][:D] = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
        for j in range(int(lens[s])):
            log_norm[ch.first[s] + j] = math.log1p(j / W)
        row += int(lens[s]) * (2 * D + 1)
        sig += int(lens[s]) * D
    parts = [out.view(np.uint8), log_norm.view(np.uint8), ch.order.view(np.uint8), ch.chain.view(np.uint8)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    return LiarSegmentBlob(np.concatenate(parts), offs, out, ch.order, ch.chain, log_norm, sig)


# What liar_msegment_blob returns: LiarSegmentBlob's fields (segs:
# N.JOINT_LIAR_MSEG_DTYPE; sections in the order LIAR_MSECTIONS) and n_pool, the
# doubles of the liar pool.
LiarMSegmentBlob = collections.namedtuple('LiarMSegmentBlob', 'blob offs segs order chain log_norm n_sigma n_pool')
LIAR_MSECTIONS = ('segs', 'log_norm', 'liar_pool', 'order', 'chain')


def liar_msegment_blob(models, segs, weight_sums, prob_seg, centres=None):
    """liar_segment_blob for the groups of a mixed segmented stage
    (include/tpe_hip.h "Batch-aware picks in mixed branch groups"): ``segs`` are
    that stage's descriptors (N.JOINT_MSEG_DTYPE), whose above_mu, above_qmu and
    quant_edges offsets and per-dimension sizes the liar descriptors
    (N.JOINT_LIAR_MSEG_DTYPE) share.  The float64 liar pool, uploaded in the
    same blob, holds per group the natural-log category tables of the above side
    (joint.liar_cat_tables: miss, then bonus) and the centres.  ``centres``: per
    group None or one float64 [V_d] array per quantised dimension
    (QuantModel.centres()); a group with a quantised label needs them."""
    import math
    S = len(models)
    if centres is None:
        centres = [None] * S
    if len(centres) != S:
        raise ValueError('joint stage: centres must hold one entry per group')
    ch = liar_chains(prob_seg, S)
    out = np.zeros(S, dtype=N.JOINT_LIAR_MSEG_DTYPE)
    lens = np.bincount(np.asarray(prob_seg, dtype=np.int64), minlength=S)
    log_norm = np.zeros(len(ch.chain), dtype=np.float64)
    pool, fill = [], 0
    row = tab = sig = 0
    for s in ch.order:
        above, low, high, cats, quants = seg_parts(models[s])[1:6]
        g, m, W, L = out[s], segs[s], float(weight_sums[s]), int(lens[s])
        Dc, Dk, Dq = int(m['n_dims']), int(m['n_cat']), int(m['n_quant'])
        g['n_dims'], g['n_cat'], g['n_quant'] = Dc, Dk, Dq
        g['k_above'], g['n_trials'] = m['k_above'], m['k_above'] - 1
        g['chain_len'], g['chain_first'] = L, ch.first[s]
        g['w_sum'], g['log_w'], g['above_mu'] = W, math.log(W), m['above_mu']
        g['psig'], g['low'], g['high'] = 1.0, -np.inf, np.inf
        if Dc:
            g['psig'][:Dc] = np.asarray(above[2], dtype=np.float64).reshape(-1, Dc)[0]
            g['low'][:Dc], g['high'][:Dc] = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
        vs =[int(v) for v in m['quant_v'][:Dq]]
        if Dk:
            g['cat_upper'], g['cat_off'] = m['cat_upper'], m['cat_off']
            tabs = [J.liar_cat_tables(c[2], c[4]) for c in cats]
            for field, i in (('cat_miss', 0), ('cat_bonus', 1)):
                g[field] = fill
                pool.extend(np.asarray(t[i], dtype=np.float64).reshape(-1) for t in tabs)
                fill += int(sum(m['cat_upper'][:Dk]))
        if Dq:
            cs = centres[s]
            if cs is None or len(cs) != Dq:
                raise ValueError('joint stage: liar with quantised labels needs centres, one array per quantised '
                                 'dimension (joint.quant_centres): group %d' % s)
            cs = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in cs]
            if any(len(c) != V or not np.isfinite(c).all() for c, V in zip(cs, vs)):
                raise ValueError('joint stage: centres must hold one finite value per lattice value')
            g['psig'][Dc:Dc + Dq] = [float(np.asarray(q[3], dtype=np.float64).reshape(-1)[0]) for q in quants]
            g['quant_v'], g['quant_edge_off'], g['n_edges'] = m['quant_v'], m['quant_edge_off'], m['n_edges']
            g['quant_tab_off'][:Dq] = np.cumsum([0] + vs[:-1])
            g['n_lattice'] = sum(vs)
            g['above_qmu'], g['quant_edges'] = m['above_qmu'], m['quant_edges']
            g['quant_centre'] = fill
            pool.extend(cs)
            fill += sum(vs)
        elif centres[s]:
            raise ValueError('joint stage: centres without a quantised dimension: group %d' % s)
        g['row_off'], g['tab_off'], g['sigma_off'] = row, tab, sig
        for j in range(L):
            log_norm[ch.first[s] + j] = math.log1p(j / W)
        row += L * (2 * Dc + 1 + Dk + Dq)
        tab += L * sum(vs)
        sig += L * (Dc + Dq)
    lpool = np.concatenate(pool) if pool else np.zeros(0)
    assert len(lpool) == fill
    parts = [out.view(np.uint8), log_norm.view(np.uint8), lpool.view(np.uint8), ch.order.view(np.uint8),
             ch.chain.view(np.uint8)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    return LiarMSegmentBlob(np.concatenate(parts), offs, out, ch.order, ch.chain, log_norm, sig, fill)
