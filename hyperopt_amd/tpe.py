"""Tree-structured Parzen Estimator suggest — MI355X engine behind the
reference's algorithm-plugin contract.

``suggest(new_ids, domain, trials, seed, prior_weight, n_startup_jobs,
n_EI_candidates, gamma, linear_forgetting)`` keeps the signature, defaults and
return value of the reference (tpe.py:762-772, 804-897): a list of new trial
documents, one per new id, with ``misc['idxs']/misc['vals']`` set for the
active hyperparameters.  ``fmin(algo=tpe.suggest)`` and
``functools.partial(tpe.suggest, n_EI_candidates=...)`` work unchanged.

Per call (the reference rebuilds and interprets a pyll posterior graph,
tpe.py:814-881; here):
  1. SoA history from the Trials cache (history.py)          tpe.py:820-842
  2. below set = the n_below best losses                     tpe.py:613-641
  3. Parzen fit of below/above per active hyperparameter     tpe.py:398-607
  4. per tree level, ONE batched device launch sequence over every
     (hyperparameter, new_id): sample C candidates from the below mixture,
     score l(x) - g(x), argmax                                tpe.py:62-301, 749-759
  5. trial documents                                          tpe.py:884-897

Extensions over the reference (keyword-only, defaults keep its behaviour):
  * ``len(new_ids) > 1``: one batched suggest (the reference asserts a single
    id).  Id j draws from Philox stream (seed, label, new_id j), so a batched
    call returns exactly what single-id calls with the same seed return.
  * ``sampler``: 'philox' (device sampling, default) or 'replay' (the
    reference's RandomState draws on the host, for exact trajectory parity).
  * ``precision``: 'fp32' (default) or 'fp64' for the continuous families.
  * ``shard=(rank, world)``: split every problem's candidates over ranks of
    the default ``torch.distributed`` group (see dist.py).
  * ``shard_ids=(rank, world)`` / ``shard_labels=(rank, world)``: split a
    batched suggest's new ids / its hyperparameters over the ranks; one
    all-gather of the chosen values after the suggest, every rank returns the
    whole result (include/tpe_hip.h "Shard axes").
  * ``joint=True`` / ``joint=[labels]``: the unconditional continuous labels
    (or the listed ones) are suggested as one vector — product-kernel
    mixtures over the group, whole-vector candidates, one argmax
    (joint.py, DESIGN.md "Joint TPE"); every other label as without it.
    ``joint_discrete=True`` lets the group also hold unconditional randint /
    categorical labels that gate no other label, ``joint_quantized=True``
    unconditional quniform / qloguniform labels of 2 to 256 lattice values,
    ``joint_wide=True`` 17 to 64 continuous labels instead of at most 16,
    ``joint_wide_mixed=True`` (with both) 1 to 8 discrete labels among them,
    ``joint_wide_quantized=True`` (with joint_wide and joint_quantized) 1 to
    4 quantised labels beside more than 8 continuous or 4 discrete ones.
    ``joint_branches=True`` also joins the continuous labels of every
    conditional branch, one group per (gate, option), each id under the model
    of the branch it takes (DESIGN.md "Branch groups");
    ``joint_branches_mixed=True`` lets joint_discrete / joint_quantized widen
    those branch groups too, ``joint_branches_wide=True`` lets joint_wide
    widen them to 17 to 64 continuous labels.

``linear_forgetting`` is accepted and, as in the reference, not used: the
forgetting window is fixed at DEFAULT_LF=25 (tpe.py:27-29).
"""
import logging
import os
import math
import time

import numpy as np

from . import _native as N
from . import devhist
from . import dist as _dist
from . import history as _history
from . import joint as _joint
from . import rand
from . import replay
from .engine import LevelProblem, get_engine
try:
    from . import _hostaddr          # (csrc/hostaddr.c, built with the library: hyperopt_amd.build)
except ImportError:                  # pragma: no cover - the package is importable before its build
    _hostaddr = None
from .parzen import _FAMILY, DEFAULT_LF, DEVICE_FIT_FAMILIES, cat_split, fit_coord, fit_posterior, fit_split

logger = logging.getLogger(__name__)

_default_prior_weight = 1.0
_default_n_EI_candidates = 24
_default_gamma = 0.25
_default_n_startup_jobs = 20
_default_linear_forgetting = DEFAULT_LF


class _Fits(object):
    """Lazily fitted posteriors of one suggest call (inactive labels are never
    fitted).  Large continuous above mixtures are left to the device fit when
    the engine computes in fp32 (Engine.device_fit_min)."""

    def __init__(self, table, hist, below_tids, prior_weight, engine=None):
        self.table, self.hist = table, hist
        self.below_tids, self.prior_weight = below_tids, prior_weight
        self.engine = engine
        self.below_sorted = None
        self.cache = {}

    def _below_sorted(self):
        if self.below_sorted is None:
            self.below_sorted = np.sort(np.asarray(self.below_tids, dtype=np.int64))
            self.below_addr = self.below_sorted.ctypes.data
        return self.below_sorted

    def get(self, row):
        post = self.cache.get(row.label)
        if post is None:
            otids, ovals = self.hist.obs[row.label]
            eng = self.engine
            f32 = eng is not None and eng.precision == 'fp32'
            bidx = None
            dmin = _dev_fit_min(eng)
            if dmin is not None and _FAMILY[row.dist] in DEVICE_FIT_FAMILIES and len(ovals) >= dmin:
                bidx = _history.below_index(otids, self.below_tids, self.hist.sorted_obs)
                if device_fits(len(ovals), len(bidx), dmin):
                    dc = devhist.columns(self.hist, eng.device)
                    # the kernel coordinate (numpy's log for the log families, as the host fits use)
                    logc = _FAMILY[row.dist] == N.FAM_LOGGAUSS
                    col = dc.column(row.label, self.hist.log_values(row.label) if logc else ovals)
                    post = fit_posterior(row.dist, row.args, ovals[bidx], None, self.prior_weight, DEFAULT_LF,
                                         above_dev=(col, len(ovals), bidx, dc.order(row.label)))
            if post is not None:
                pass
            elif row.categorical and self.hist.sorted_obs:
                # split + both pseudo-count posteriors in one native call (exact)
                bs = self._below_sorted()
                cols = self.hist.cat_columns(row.label)
                post = cat_split(row.dist, row.args, otids, ovals, bs, self.prior_weight, DEFAULT_LF,
                                 addrs=None if cols is None else cols + (self.below_addr,))
            elif (f32 and _FAMILY[row.dist] in DEVICE_FIT_FAMILIES and self.hist.sorted_obs
                  and self.hist.value_order(row.label) is not None):
                # fp32 device path: split + both fits in one native call
                logc = _FAMILY[row.dist] == N.FAM_LOGGAUSS
                bs = self._below_sorted()
                order = self.hist.value_order(row.label)
                cols = self.hist.native_columns(row.label, log=logc)
                post = fit_split(row.dist, row.args, otids, ovals, bs, order, self.prior_weight, DEFAULT_LF,
                                 coord=self.hist.log_values(row.label) if logc else None,
                                 addrs=None if cols is None else cols + (self.below_addr,))
            else:
                if bidx is None:
                    bidx = _history.below_index(otids, self.below_tids, self.hist.sorted_obs)
                m = np.zeros(len(ovals), dtype=bool)
                m[bidx] = True
                post = fit_posterior(row.dist, row.args, ovals[m], ovals[~m], self.prior_weight, DEFAULT_LF)
            self.cache[row.label] = post
        return post


def _value(row, v):
    """Reference value types: np.int64 for categorical draws, np.float64 else."""
    return np.int64(int(v)) if row.categorical else np.float64(v)


def _column(row, values):
    """_value over a float64 array of results (numpy scalars, one C loop)."""
    return list(values.astype(np.int64)) if row.categorical else list(np.asarray(values, dtype=np.float64))


def _run(engine, problems, C, seed, shard):
    if shard is None:
        return engine.run_level(problems, C, seed)
    rank, world = shard
    lo, hi = _dist.shard_range(C, rank, world)
    res = engine.run_level(problems, hi - lo, seed, cand_base=lo, n_cand_global=C)
    return _dist.allgather_results(res, device=engine.device)


# speculative level fusion (_choices_fused): on by default; a gating
# categorical's winner is predicted when the expected number of draws of the
# predicted category is at least SPECULATE_MIN_DRAWS
SPECULATE = True
SPECULATE_MIN_DRAWS = 64.0


def _predict_activity(table, fits, C):
    """Predicted {label: category or None} of a conditional space, or None.

    A switch index (categorical) scores every candidate by the same per-category
    value log p_below[c] - log p_above[c] (categorical_lpdf, tpe.py:50-57), so
    its argmax (broadcast_best, tpe.py:749-759) is the best category among the
    categories drawn — with C candidates, the best category of the fitted
    posteriors unless it goes undrawn (probability (1 - q)^C).  Labels that are
    not gates get a placeholder.  Any non-categorical gate: no prediction."""
    chosen = {}
    for level in table.levels():
        for row in level:
            if not table.active(row, chosen):
                chosen[row.label] = None
            elif row.label not in table.parent_labels:
                chosen[row.label] = -1
            elif not row.categorical:
                return None
            else:
                post = fits.get(row)
                pb = post.below[0].tolist()
                pa = post.above[0].tolist()
                tot = math.fsum(pb)
                if not tot > 0:
                    return None
                # np.argmax of log pb - log pa over the drawable categories (pb > 0)
                c, best = -1, None
                for k, (b, a) in enumerate(zip(pb, pa)):
                    if not b > 0:
                        continue
                    sc = math.log(b) - math.log(a) if a > 0 else math.inf
                    if best is None or sc > best or (sc != sc and best == best):
                        c, best = k, sc
                if c < 0 or C * pb[c] / tot < SPECULATE_MIN_DRAWS:
                    return None
                chosen[row.label] = c
    return chosen


def _choices_fused(table, fits, new_ids, seed, C, engine, shard, remote=()):
    """Every tree level in ONE device batch under the predicted activity; the
    gates' device winners are then checked against the prediction.  A problem's
    draws depend only on (seed, label, new_id) and its scores on the fits, so a
    verified batch chooses what the level-by-level evaluation chooses (up to
    the fp32 summation order of pruned above mixtures, which follows the batch
    layout).  Returns None on a misprediction (the caller then evaluates level
    by level)."""
    pred = _predict_activity(table, fits, C)
    if pred is None:
        return None
    ids = np.asarray(new_ids, dtype=np.int64)
    rows = [r for r in table.rows if pred[r.label] is not None and r.index not in remote]
    problems = [LevelProblem(fits.get(r), r.index, ids) for r in rows]
    res = _run(engine, problems, C, seed, shard)
    n = len(ids)
    order = table.level_order()
    chosen = [dict.fromkeys(order) for _ in new_ids]
    for r in table.rows:                     # active here, evaluated by another rank
        if r.index in remote and pred[r.label] is not None:
            for d in chosen:
                d[r.label] = np.nan
    idx = res['idx']
    for k, row in enumerate(rows):
        if (idx[k * n:(k + 1) * n] < 0).any():
            raise RuntimeError('no candidate selected for %r' % row.label)
        col = _column(row, res['value'][k * n:(k + 1) * n])
        if pred[row.label] >= 0 and any(int(v) != pred[row.label] for v in col):
            return None
        lab = row.label
        for d, v in zip(chosen, col):
            d[lab] = v
    return chosen


def _choices_philox(table, fits, new_ids, seed, C, engine, shard, remote=()):
    """Level by level over the tree (after the fused batch when it applies).
    ``remote``: label indices another rank evaluates (hyperparameter-axis
    shard, never a gate): active ones get NaN here."""
    if SPECULATE and table.n_levels > 1:
        fused = _choices_fused(table, fits, new_ids, seed, C, engine, shard, remote)
        if fused is not None:
            return fused
    ids = np.asarray(new_ids, dtype=np.int64)
    chosen = [dict.fromkeys(table.level_order()) for _ in new_ids]
    every = list(range(len(new_ids)))
    for level in table.levels():
        problems, rows, members = [], [], []
        for row in level:
            if row.parents == [None]:          # unconditional: active for every id
                act = every
            else:
                act = [i for i, c in enumerate(chosen) if table.active(row, c)]
            if not act:
                continue
            if row.index in remote:
                for i in act:
                    chosen[i][row.label] = np.nan
                continue
            problems.append(LevelProblem(fits.get(row), row.index, ids if act is every else ids[act]))
            rows.append(row)
            members.append(act)
        if not problems:
            continue
        res = _run(engine, problems, C, seed, shard)
        k = 0
        for row, act in zip(rows, members):
            if (res['idx'][k:k + len(act)] < 0).any():
                raise RuntimeError('no candidate selected for %r' % row.label)
            col = _column(row, res['value'][k:k + len(act)])
            k += len(act)
            lab = row.label
            for i, v in zip(act, col):
                chosen[i][lab] = v
    return chosen


# one native call per suggest (tpe_suggest_tree) for the spaces it covers;
# TPE_NATIVE_TREE=0 keeps every suggest on the general path (A/B, tests)
NATIVE_TREE = os.environ.get('TPE_NATIVE_TREE', '1') != '0'


def _tree_static(table):
    """TREE_LABEL_DTYPE records of a ParamTable's static fields (family,
    bounds, prior, gating structure), built once per table; None when the
    tree has a label with more parents than the record holds."""
    st = table.__dict__.get('_tree_static')
    if st is not None:
        return st if st[0] is not None else None
    arr = np.zeros(len(table.rows), dtype=N.TREE_LABEL_DTYPE)
    keep, meta = [], []
    for r in table.rows:
        rec = arr[r.index]
        fam = _FAMILY[r.dist]
        a = r.args
        rec['family'], rec['label_ix'] = fam, r.index
        if fam == N.FAM_CATEGORICAL:
            rec['upper'] = int(a['upper'])
            if r.dist != 'randint':
                p = np.ascontiguousarray(a['p'], dtype=np.float64)
                keep.append(p)
                rec['p_prior'] = p.ctypes.data
        elif r.dist in ('uniform', 'loguniform', 'quniform', 'qloguniform'):
            rec['flags'] = N.F_HAS_LOW | N.F_HAS_HIGH
            rec['low'], rec['high'] = float(a['low']), float(a['high'])
            rec['prior_mu'], rec['prior_sigma'] = 0.5 * (a['high'] + a['low']), 1.0 * (a['high'] - a['low'])
        else:
            rec['prior_mu'], rec['prior_sigma'] = float(a['mu']), float(a['sigma'])
        if a.get('q') is not None:
            rec['q'] = float(a['q'])
        rec['depth'] = r.depth
        ps = [p for p in r.parents if p is not None]
        if len(ps) > N.TREE_MAX_PARENTS:
            table._tree_static = (None, None, None)
            return None
        rec['n_parents'] = len(ps)
        for j, (pl, pc) in enumerate(ps):
            rec['parent'][j] = table.by_label[pl].index
            rec['parent_cat'][j] = int(pc)
        meta.append((r.label, r.index, fam))
    st = table._tree_static = (arr, keep, meta)
    return st


_I64, _F64 = np.dtype(np.int64).num, np.dtype(np.float64).num


def _tree_groups(table, meta):
    """The tree records' labels by kind, once per table: the categorical ones
    [(label, index)] and the continuous ones (labels, their record indices,
    which are log families) — the quantized ones take no columns."""
    g = table.__dict__.get('_tree_groups')
    if g is None:
        cats = [(label, ix) for label, ix, fam in meta if fam == N.FAM_CATEGORICAL]
        gm = [(label, ix, fam == N.FAM_LOGGAUSS) for label, ix, fam in meta if fam in (N.FAM_GAUSS, N.FAM_LOGGAUSS)]
        g = table._tree_groups = (cats, [m[0] for m in gm], np.array([m[1] for m in gm], dtype=np.int64),
                                  np.array([m[2] for m in gm], dtype=bool))
    return g


def _dev_fit_min(engine):
    """Observations from which a continuous label's above side is fitted on
    the device (Engine.device_fit_min, fp32 only), or None."""
    if engine is None or engine.precision != 'fp32' or engine.device_fit_min <= 0:
        return None
    return max(int(engine.device_fit_min), 64)


def device_fits(n_obs, n_below, dev_min):
    """Whether a continuous label's above side gets the device Parzen fit: the
    one predicate of both paths (tpe_suggest.cpp fit_label: n_obs >= dev_min,
    at most 64 below observations, more than 64 above components), so a
    suggest fits a label the same way whichever path takes it."""
    return dev_min is not None and n_obs >= dev_min and n_below <= 64 and n_obs - n_below + 1 > 64


_DENSE_FIELDS = ('n_obs', 'tids', 'values', 'order', 'dev_obs', 'ord_key_in', 'ord_idx_in', 'n_ord_in', 'ord_key_out',
                 'ord_idx_out')


def _tree_labels(table, hist, engine=None, remote=()):
    """The table's tree records with the history's observation columns filled
    in (tids, kernel coordinate, value order) and, for the continuous labels
    large enough for the device Parzen fit, the device column and resident
    value order (devhist) — memoised per (table object, document count) on the
    Trials cache, or on the History itself without one, while the device
    columns and orders stay put (DeviceColumns.version).  Quantized labels
    carry no columns: tpe_suggest_tree sends them to the caller whenever they
    need a fit.  Returns (records, keep-alive list, the device-fitted labels
    as (label indices, order slots, n_obs, devhist order group) or None, the
    records' address) or None.
    ``remote`` labels (another rank's, TPE_F_REMOTE) get no device column."""
    st = _tree_static(table)
    if st is None:
        return None
    arr0, _, meta = st
    dev_min = _dev_fit_min(engine)
    cache = hist._cache
    holder, n_docs = (cache, len(cache.docs)) if cache is not None else (hist, -1)
    dc = devhist.columns(hist, engine.device) if dev_min is not None else None
    # keyed on the table OBJECT (the memo keeps it alive, so a new table can
    # never reuse its id), the document count and the device state's version
    memo = getattr(holder, 'tree_memo', None)
    dver = dc.version if dc is not None else None
    mkey = (dev_min, remote)
    if memo is not None and memo[0] is table and memo[2] == mkey and memo[4] == dver:
        if memo[1] == n_docs:
            return memo[3]
        # documents appended (FMinIter: one per suggest), no device-fitted label:
        # the records are updated in place — only the labels that gained
        # observations, through the field views (no structured-scalar writes)
        if cache is not None and n_docs > memo[1] and memo[3][2] is None and _tree_refill(memo[5], meta, hist):
            holder.tree_memo = (table, n_docs, mkey, memo[3], dver, memo[5])
            return memo[3]
    keep = []
    cats, glab, gix, glogc = _tree_groups(table, meta)
    dense = hist.obs if isinstance(hist.obs, _history.DenseObs) else None
    dense_all = (bool(glab) and not cats and dense is not None and dev_min is not None and dense.n >= dev_min
                 and not remote and not glogc.any())
    # a dense history's views (FMinIter on columnar data: a new History per
    # appended trial, one device state shared in hist.dev): every record field
    # that moves is rewritten below, so the previous view's records are reused
    # — no copy of the table's records and no flag fix-ups per suggest
    prev = hist.dev.get('_dense_tree') if dense_all and cache is None else None
    if prev is not None and prev[0] is table and prev[1] == mkey:
        arr = prev[2]
    else:
        arr = arr0.view(np.uint8).copy().view(arr0.dtype)  # (a byte copy: the record dtype copies field by field)
    for label, ix in cats:
        otids, ovals = hist.obs[label]
        cols = hist.cat_columns(label)
        if cols is None:
            t, v = np.ascontiguousarray(otids, dtype=np.int64), np.ascontiguousarray(ovals, dtype=np.int64)
            keep += [t, v]
            cols = (t.ctypes.data, v.ctypes.data)
        rec = arr[ix]
        rec['tids'], rec['values'], rec['n_obs'] = cols[0], cols[1], len(otids)
    devs = None
    if glab and dense is not None and dev_min is not None and dense.n >= dev_min and not remote \
            and not glogc.any():
        # a dense history (every label in every trial, one matrix row each): the
        # device labels' records straight from the matrix, no per-label Python
        n = dense.n
        ri = dense.layout.row_index(glab)
        m = dense.matrix
        slots = dc.upload_rows(glab, m, ri, n)
        keep += [dense.tids, m, dc.store]
        ns = np.full(len(glab), n, dtype=np.int64)
        kin, iin, n_in, kout, iout = dc.orders.ptrs_many(slots, ns)
        ta = np.ascontiguousarray(dense.tids, dtype=np.int64)
        if ta is not dense.tids:
            keep.append(ta)
        # (the records' field views kept with the reused records; every label a
        # device label in table order — config 5 — writes whole fields)
        fvs = prev[3] if prev is not None and prev[2] is arr else None
        if fvs is None:
            whole = len(gix) == len(arr) and bool((gix == np.arange(len(arr))).all())
            fvs = {f: arr[f] for f in _DENSE_FIELDS}
            fvs[None] = slice(None) if whole else gix
        at = fvs[None]
        for f, v in (('n_obs', n), ('tids', ta.ctypes.data), ('values', m.ctypes.data + m.strides[0] * ri),
                     ('order', 0), ('dev_obs', dc.addresses(slots)), ('ord_key_in', kin), ('ord_idx_in', iin),
                     ('n_ord_in', n_in), ('ord_key_out', kout), ('ord_idx_out', iout)):
            fvs[f][at] = v
        devs = (gix, slots, ns, dc.orders)
        glab = ()
        if dense_all and cache is None:
            hist.dev['_dense_tree'] = (table, mkey, arr, fvs)
    if glab:
        obs = hist.obs
        pairs = [obs[k] for k in glab]
        tl = [p[0] for p in pairs]
        ns = np.fromiter(map(len, tl), dtype=np.int64, count=len(tl))
        arr['n_obs'][gix] = ns
        big = ns >= dev_min if dev_min is not None else np.zeros(len(ns), dtype=bool)
        host, dev = ~big, big
        if remote and big.any():                 # (another rank's labels: never fitted here)
            dev = big & ~np.isin(gix, np.asarray(remote, dtype=np.int64))
        for q in np.flatnonzero(host).tolist():
            label, ix, logc = glab[q], int(gix[q]), bool(glogc[q])
            otids, ovals = pairs[q]
            order = hist.value_order(label)
            cols = hist.native_columns(label, log=logc) if order is not None else None
            if cols is None:
                t = np.ascontiguousarray(otids, dtype=np.int64)
                x = np.ascontiguousarray(hist.log_values(label) if logc else ovals, dtype=np.float64)
                keep += [t, x]
                cols = (t.ctypes.data, x.ctypes.data, 0)
                if order is not None:
                    o = np.ascontiguousarray(order, dtype=np.int64)
                    keep.append(o)
                    cols = cols[:2] + (o.ctypes.data,)
            rec = arr[ix]
            rec['tids'], rec['values'], rec['order'] = cols
        if dev.any():
            # device fit of the above side: the device column (kernel coordinate)
            # and its resident order — every such label's new observations up in
            # one scatter, room for their orders made, then the addresses (a
            # re-layout moves them all); the host keeps the columns for the below side
            if _hostaddr is None:
                raise N.NativeUnavailable('hyperopt_amd._hostaddr is not built (python -m hyperopt_amd.build)')
            if dev.all():
                dq, dlab, dns, ixs = None, glab, ns, gix
            else:
                dq = np.flatnonzero(dev)
                dlab, dns, ixs = [glab[q] for q in dq.tolist()], ns[dq], gix[dq]
            sel = pairs if dq is None else [pairs[q] for q in dq.tolist()]
            dt = tl if dq is None else [p[0] for p in sel]
            if glogc.any():
                lg = glogc if dq is None else glogc[dq]
                dx = [hist.log_values(k) if l else p[1] for k, l, p in zip(dlab, lg.tolist(), sel)]
            else:
                dx = [p[1] for p in sel]
            try:
                ta = _hostaddr.addresses(dt, _I64)
            except TypeError:
                dt = [np.ascontiguousarray(a, dtype=np.int64) for a in dt]
                ta = _hostaddr.addresses(dt)
            try:
                xa = _hostaddr.addresses(dx, _F64)
            except TypeError:
                dx = [np.ascontiguousarray(a, dtype=np.float64) for a in dx]
                xa = _hostaddr.addresses(dx)
            slots = dc.upload(dlab, dx, dns)
            keep += [dt, dx, dc.store]
            kin, iin, n_in, kout, iout = dc.orders.ptrs_many(slots, dns)
            for f, v in (('tids', ta), ('values', xa), ('order', 0), ('dev_obs', dc.addresses(slots)),
                         ('ord_key_in', kin), ('ord_idx_in', iin), ('n_ord_in', n_in), ('ord_key_out', kout),
                         ('ord_idx_out', iout)):
                arr[f][ixs] = v
            devs = (ixs, slots, dns, dc.orders)
    out = (arr, keep, devs, arr.ctypes.data)
    fv = None
    if cache is not None and devs is None and not keep:
        fv = {f: arr[f] for f in ('tids', 'values', 'order', 'n_obs')}
        fv['n'] = arr['n_obs'].tolist()
    # (the version after the columns and orders above were looked up: that may move it)
    holder.tree_memo = (table, n_docs, mkey, out, dc.version if dc is not None else None, fv)
    return out


def _tree_refill(fv, meta, hist):
    """In-place update of memoised tree records (_tree_labels) after appended
    documents: the labels whose observation count changed get their columns'
    current addresses (a grown buffer moves) and merged value order.  False
    (nothing written that matters: the caller rebuilds) when the records were
    not built from the Trials cache or a value order is unavailable."""
    if fv is None:
        return False
    f_tids, f_vals, f_ord, f_n, last = fv['tids'], fv['values'], fv['order'], fv['n_obs'], fv['n']
    for label, ix, fam in meta:
        cat = fam == N.FAM_CATEGORICAL
        if not cat and fam != N.FAM_GAUSS and fam != N.FAM_LOGGAUSS:
            continue                         # (quantized labels carry no columns)
        n = len(hist.obs[label][0])
        if n == last[ix]:
            continue
        if cat:
            f_tids[ix], f_vals[ix] = hist.cat_columns(label)
        else:
            if hist.value_order(label) is None:
                return False
            f_tids[ix], f_vals[ix], f_ord[ix] = hist.native_columns(label, log=fam == N.FAM_LOGGAUSS)
        f_n[ix] = n
        last[ix] = n
    return True


def _choices_native(table, hist, below_tids, new_ids, seed, C, engine, prior_weight, shard=None, columns=False,
                    remote=(), borrow=False):
    """``_choices_philox`` in one native call (tpe_suggest_tree), or None when
    the space or history needs the general path.  Labels the native fits cannot
    reproduce (quantized ones, sides with repeated values: numpy's argsort tie
    order decides their weights) come back flagged; they are fitted here
    exactly as the general path fits them and handed to a second call.
    ``shard`` = (rank, world): candidate-sharded over the default process
    group, the level results exchanged inside the native call (dist.py).
    ``remote``: label indices another rank evaluates (TPE_F_REMOTE)."""
    out = _native_tree(table, hist, below_tids, new_ids, seed, C, engine, prior_weight, shard, columns, remote,
                       borrow)
    if out is None:
        table.native_fit_hint = ()             # the general path takes it: nothing to pre-fit next time
    return out


_GIVEN_FIELDS = ('tids', 'values', 'n_obs', 'side_order', 'side_n', 'host_k', 'host_w')


def _coord_fn(table, row):
    """The row's fit coordinate as an elementwise function (parzen.fit_coord),
    made once per table row."""
    fns = table.__dict__.setdefault('_coord_fns', {})
    f = fns.get(row.index)
    if f is None:
        a, dist = row.args, row.dist
        f = fns[row.index] = lambda v: fit_coord(dist, a, v)
    return f


def _below_positions(hist, label, otids, below_tids):
    """(positions of the below observations among a label's, history.below_index;
    the mask of the others), kept on the below set itself for the History and
    column length they were computed for."""
    memo = getattr(below_tids, 'positions', None)
    if memo is not None:
        p = memo.get(label)
        if p is not None and p[0] == len(otids) and p[1] is hist:
            return p[2], p[3]
    b = _history.below_index(otids, below_tids, hist.sorted_obs)
    above = np.ones(len(otids), dtype=bool)
    above[b] = False
    if memo is not None:
        memo[label] = (len(otids), hist, b, above)
    return b, above


def _side_orders(hist, label, otids, x, below_tids):
    """numpy's argsort of a label's below and above sides (the reference's tie
    order, tpe.py:427-428), kept on the below set beside the positions for the
    same History and column length (a History's columns are fixed): a suggest
    on an unchanged history and below set — the same inputs — reuses them."""
    bidx, above = _below_positions(hist, label, otids, below_tids)
    memo = getattr(below_tids, 'positions', None)
    key = ('orders', label)
    if memo is not None:
        p = memo.get(key)
        if p is not None and p[0] == len(otids) and p[1] is hist:
            return p[2], p[3]
    ob = np.argsort(x[bidx])
    oa = np.argsort(x[above])
    if memo is not None:
        memo[key] = (len(otids), hist, ob, oa)
    return ob, oa


def _native_tree(table, hist, below_tids, new_ids, seed, C, engine, prior_weight, shard, columns=False, remote=(),
                 borrow=False):
    if not hist.sorted_obs:
        return None
    tl = _tree_labels(table, hist, engine, remote)
    if tl is None:
        return None
    rm = getattr(table, '_remote_applied', None)
    if rm is None or rm[0] is not tl[0] or rm[1] != remote:
        fl = tl[0]['flags']
        fl &= ~N.F_REMOTE
        if remote:
            fl[list(remote)] |= N.F_REMOTE
        table._remote_applied = (tl[0], remote)
    ex = None
    if shard is not None:
        ex = _dist.exchange_for(engine)
    below = getattr(below_tids, 'sorted_view', None)
    if below is None:
        below = np.sort(np.asarray(below_tids, dtype=np.int64))
    # the labels the previous suggest used are fitted up front on the native
    # worker threads (TPE_F_PREFIT; the active branch seldom changes)
    hint = getattr(table, 'native_used', None)
    pf = getattr(table, '_prefit_applied', None)
    if hint is not None and (pf is None or pf[0] is not tl[0] or pf[1] != hint):
        fl = tl[0]['flags']
        fl &= ~N.F_PREFIT
        fl[list(hint)] |= N.F_PREFIT
        table._prefit_applied = (tl[0], hint)
    st = {'arr': tl[0], 'ptr': tl[3]}
    host = {}

    def give(ix):
        """Label ix for the native call with numpy's argsort of each of its
        sides (the reference's tie order, tpe.py:427-428): the fit coordinate
        in tid order and the two permutations (tpe_tree_label.side_order) —
        the native call then fits it.  (A categorical label: the general
        path's fit.)  False: the label needs the general path."""
        if not host and 'copied' not in st:
            # the call's records: a per-table copy of the memoised ones (the given
            # labels' fields point at this call's arrays), its field views and
            # address kept with it
            g = table.__dict__.get('_given')
            if g is None or g[0] is not tl[0]:
                arr2 = tl[0].copy()
                g = table._given = (tl[0], arr2, {f: arr2[f] for f in _GIVEN_FIELDS},
                                    arr2.__array_interface__['data'][0])
            else:
                np.copyto(g[1], tl[0])
            st['copied'] = True
            st['arr'], st['fv'], st['ptr'] = g[1], g[2], g[3]
        fv = st['fv']
        row = table.rows[ix]
        keep = host[ix] = []                   # (keeps the arrays alive for the call)
        otids, ovals = hist.obs[row.label]
        n = len(otids)
        if row.categorical:
            if 'fits' not in st:
                st['fits'] = _Fits(table, hist, below_tids, prior_weight, engine)
            post = st['fits'].get(row)
            for sd, side in enumerate((post.below, post.above)):
                c = np.ascontiguousarray(side[0], dtype=np.float64)
                keep.append(c)
                fv['host_k'][ix, sd] = len(c)
                fv['host_w'][ix, sd] = c.__array_interface__['data'][0]
            return True
        dmin = _dev_fit_min(engine)
        if dmin is not None and _FAMILY[row.dist] in DEVICE_FIT_FAMILIES and n >= dmin:
            return False                       # (device-fit sizes: the general path)
        x = hist.coord_values(row.label, row.dist, _coord_fn(table, row))
        ob, oa = _side_orders(hist, row.label, otids, x, below_tids)
        cols = hist.cat_columns(row.label)     # (the cache's column addresses: tids, raw values)
        if cols is None:
            t = np.ascontiguousarray(otids, dtype=np.int64)
            x = np.ascontiguousarray(x, dtype=np.float64)
            keep += [t, x]
            ta, xa_ = t.__array_interface__['data'][0], x.__array_interface__['data'][0]
        else:
            ta, xa_ = cols[0], hist.coord_addr(row.label, row.dist)
        keep += [ob, oa]
        fv['tids'][ix], fv['values'][ix], fv['n_obs'][ix] = ta, xa_, n
        so = fv['side_order']
        so[ix, 0], so[ix, 1] = ob.__array_interface__['data'][0], oa.__array_interface__['data'][0]
        sn = fv['side_n']
        sn[ix, 0], sn[ix, 1] = len(ob), len(oa)
        return True
    # the labels the previous call had to fit here are fitted up front (the active
    # branch seldom changes between suggests): no refused first call
    for ix in getattr(table, 'native_fit_hint', ()):
        if not give(ix):
            return None
    # (a level-by-level run learns a deeper level's needs only after the levels above it)
    for attempt in range(table.n_levels + 1):
        values, active = engine.suggest_tree(st['arr'], below, prior_weight, DEFAULT_LF, new_ids, C, seed,
                                             SPECULATE_MIN_DRAWS if SPECULATE else -1.0, shard=shard,
                                             exchange=ex, labels_ptr=st['ptr'])
        if values is not None:
            break
        need = np.flatnonzero(active)          # (need_fit on TPE_E_FALLBACK)
        if not len(need) or any(ix in host for ix in need.tolist()):
            return None
        for ix in need.tolist():
            if not give(ix):
                return None
    else:
        return None
    # (values / active: the engine's result buffers, consumed or copied here)
    # (only labels some id used: a branch switch drops the old branch's; a
    # batch's rows are not turned into Python lists — and a batch whose every
    # label is active, a flat space, is told by one contiguous pass)
    av = active.view(np.bool_)
    if len(values) == 1:
        used = av[0].tolist()
    elif av.all():
        used = [True] * av.shape[1]
    else:
        used = np.ascontiguousarray(av.T).any(axis=1).tolist()
    table.native_fit_hint = tuple(ix for ix in host if used[ix]) if host else ()
    if used != getattr(table, '_used_list', None):      # (the active branch seldom changes)
        table._used_list = used
        table.native_used = tuple(i for i, u in enumerate(used) if u)
    # the device-fitted labels that ran hold their merged value orders now (a
    # label the call took a host fit for, give(), did not run the device fit:
    # its order buffers were not written)
    # (a call on the same records, branch and host fits as the last committed one
    # finds every order already at its length: nothing to walk)
    done = getattr(table, '_committed', None)
    dv = tl[2]
    if dv is not None and (host or done is None or done[0] is not tl[0] or done[1] is not table._used_list):
        ok = np.asarray(used, dtype=bool)[dv[0]]
        if host:
            ok &= ~np.isin(dv[0], np.fromiter(host, dtype=np.int64, count=len(host)))
        dv[3].commit_many(dv[1][ok], dv[2][ok])
        table._committed = None if host else (tl[0], table._used_list)
    if columns:
        # (borrow: views of the engine's result buffers, consumed by the caller
        # before the engine's next suggest — the sharded paths' gathers)
        return ChoiceColumns(table.labels, values, av) if borrow else \
            ChoiceColumns(table.labels, values.copy(), av.copy())
    return _result_dicts(table, values, av)


def _result_dicts(table, values, active):
    """Per-id {label: value or None} dicts in level order from [n x L] values
    (float64) and activity (bool or int8), with the reference's value types —
    np.int64 categories, np.float64 values — for any id count, made natively
    (a 1000-dim space is 1000 scalars per suggest; 4096 x 20 in 5.9 ms on the
    build host against 8.2 for Python scalars column by column)."""
    order = table.level_order()
    tm = table.__dict__.get('_typed_meta')
    if tm is None:
        cat = {r.label: r.categorical for r in table.rows}
        tm = table._typed_meta = (tuple(order), np.array([table.by_label[k].index for k in order], dtype=np.int64),
                                  np.array([cat[k] for k in order], dtype=np.int8))
    values = np.ascontiguousarray(values, dtype=np.float64)
    act = np.ascontiguousarray(active)
    if act.dtype != np.int8 and act.dtype != np.bool_:
        act = act.astype(np.bool_)
    if _hostaddr is not None:
        return _hostaddr.typed_dicts(tm[0], tm[1], tm[2], values, act)
    out = []
    for a, v in zip(act.tolist(), values.tolist()):
        d = dict.fromkeys(order)
        for label, ix, c in zip(tm[0], tm[1].tolist(), tm[2].tolist()):
            if a[ix]:
                d[label] = np.int64(v[ix]) if c else np.float64(v[ix])
        out.append(d)
    return out


def _tree_static_meta(table):
    """(label, index, family) of every label, table order (the families the
    result dicts type values by)."""
    meta = table.__dict__.get('_result_meta')
    if meta is None:
        meta = table._result_meta = [(r.label, r.index, N.FAM_CATEGORICAL if r.categorical else N.FAM_GAUSS)
                                     for r in table.rows]
    return meta


def _choices_replay(table, fits, new_ids, seed, C, engine):
    """Reference RandomState order: labels descending, ancestors first.  Draws
    are made on the host in that order; a label whose parent is drawn but not
    yet scored forces a device flush of the pending draws first."""
    rng = np.random.RandomState(seed)
    out = []
    for new_id in new_ids:
        chosen, pending, pending_labels = {}, [], set()

        def flush():
            if not pending:
                return
            problems = [LevelProblem(fits.get(row), row.index, [new_id], inject=cand[None, :])
                        for row, cand in pending]
            res = engine.run(problems, C, seed)
            for (row, cand), r in zip(pending, res):
                chosen[row.label] = cand[int(r['idx'])]
            del pending[:]
            pending_labels.clear()

        for row in table.rng_order():
            if any(p is not None and p[0] in pending_labels for p in row.parents):
                flush()
            if table.active(row, chosen):
                pending.append((row, replay.draw(rng, fits.get(row), C)))
                pending_labels.add(row.label)
            else:
                chosen[row.label] = None
        flush()
        out.append(dict((k, (None if v is None else _value(table.by_label[k], v))) for k, v in chosen.items()))
    return out


def suggest(new_ids, domain, trials, seed,
            prior_weight=_default_prior_weight,
            n_startup_jobs=_default_n_startup_jobs,
            n_EI_candidates=_default_n_EI_candidates,
            gamma=_default_gamma,
            linear_forgetting=_default_linear_forgetting,
            sampler='philox', precision='fp32', device=None, shard=None, shard_ids=None, shard_labels=None,
            shard_grid=None, joint=False, joint_discrete=False, joint_quantized=False, joint_wide=False,
            joint_branches=False, joint_branches_mixed=False, joint_branches_wide=False, joint_shard=None,
            joint_wide_mixed=False, joint_wide_quantized=False, joint_liar=False):
    new_ids = list(new_ids)
    if not new_ids:
        return []
    if joint_shard is not None:                  # (argument errors first, as below; nothing on the default path)
        _joint_shard_pair(joint_shard, joint, joint_wide_mixed, joint_wide_quantized)
    liar_mode = _joint_liar_mode(joint_liar)
    if liar_mode:
        _joint_liar_check(joint, joint_shard, mode=liar_mode, joint_branches=joint_branches)
    if ((joint is not False and joint is not None) or joint_discrete or joint_quantized or joint_wide or joint_branches
            or joint_branches_mixed or joint_branches_wide or joint_wide_mixed or joint_wide_quantized):
        # (argument errors first: no device use, no startup draw)
        plan = _joint_plan(domain.table, joint, sampler, precision, (shard, shard_ids, shard_labels, shard_grid),
                           joint_discrete, joint_quantized,
                           _wide_mode(joint_wide, joint_wide_mixed, joint_wide_quantized),
                           _branch_mode(joint_branches, joint_branches_wide, joint_wide), joint_branches_mixed)
        _branch_wide_check(plan, joint_shard, liar_mode)
        if liar_mode:
            _joint_liar_check(joint, joint_shard, plan, liar_mode, joint_branches)
            _wide_quant_liar_check(plan[0], liar_mode)
    t0 = time.time()
    hist = _history.extract(domain, trials)
    if logger.isEnabledFor(logging.INFO):
        if len(hist):
            logger.info('TPE using %i/%i trials with best loss %f', len(hist), len(trials),
                        float(np.min(hist.losses)))
        else:
            logger.info('TPE using 0 trials')
    if len(hist) < n_startup_jobs:
        return rand.suggest(new_ids, domain, trials, seed)
    choices = suggest_choices(domain.table, hist, new_ids, seed, prior_weight=prior_weight,
                              n_EI_candidates=n_EI_candidates, gamma=gamma, sampler=sampler,
                              precision=precision, device=device, shard=shard, shard_ids=shard_ids,
                              shard_labels=shard_labels, shard_grid=shard_grid, joint=joint,
                              joint_discrete=joint_discrete, joint_quantized=joint_quantized, joint_wide=joint_wide,
                              joint_branches=joint_branches, joint_branches_mixed=joint_branches_mixed,
                              joint_branches_wide=joint_branches_wide, joint_shard=joint_shard,
                              joint_wide_mixed=joint_wide_mixed,
                              joint_wide_quantized=joint_wide_quantized, joint_liar=joint_liar)
    logger.info('tpe.suggest took %f seconds', time.time() - t0)
    return rand.docs_from_choices(new_ids, domain, trials, choices)


class ChoiceColumns(object):
    """Columnar result of a batched suggest (``suggest_choices(...,
    columns=True)``): ``labels`` in table order, ``values`` float64
    [n_ids x n_labels] (a categorical label's chosen index as a float, NaN
    where inactive) and ``active`` bool [n_ids x n_labels].  ``dicts()`` gives
    the per-id {label: value or None} dicts ``suggest_choices`` returns."""
    __slots__ = ('labels', 'values', 'active', '_cat')

    def __init__(self, labels, values, active, categorical=None):
        self.labels, self.values, self.active = list(labels), values, active
        self._cat = categorical

    def __len__(self):
        return len(self.values)

    def dicts(self, table):
        return _result_dicts(table, self.values, self.active)

    @classmethod
    def from_dicts(cls, table, dicts):
        n, L = len(dicts), len(table.rows)
        values = np.full((n, L), np.nan)
        active = np.zeros((n, L), dtype=bool)
        for j, d in enumerate(dicts):
            for r in table.rows:
                v = d.get(r.label)
                if v is not None:            # (NaN: active, evaluated by another rank)
                    values[j, r.index] = float(v)
                    active[j, r.index] = True
        return cls(table.labels, values, active)


def suggest_choices(table, hist, new_ids, seed, prior_weight=_default_prior_weight,
                    n_EI_candidates=_default_n_EI_candidates, gamma=_default_gamma,
                    sampler='philox', precision='fp32', device=None, shard=None, columns=False,
                    shard_ids=None, shard_labels=None, shard_grid=None, joint=False, joint_discrete=False,
                    joint_quantized=False, joint_wide=False, joint_branches=False, joint_branches_mixed=False,
                    joint_branches_wide=False, joint_shard=None, joint_wide_mixed=False, joint_wide_quantized=False,
                    joint_liar=False):
    """The suggest core on a structure-of-arrays history (``history.History``):
    per new id a {label: value or None} dict.  ``suggest`` wraps it with the
    Trials document layout; columnar callers (and bench.py's large configs)
    use it directly.  ``columns=True``: the same choices as one ChoiceColumns
    (SoA in, SoA out — no per-id Python objects for a batch of thousands).

    At most one shard axis (rank, world) over the default process group:
    ``shard`` splits every problem's candidates (one exchange per tree level),
    ``shard_ids`` the new ids (contiguous blocks), ``shard_labels`` the
    hyperparameters (dist.label_owners) and ``shard_grid`` both at once — the
    (label x new id) problem grid cut into label groups x id blocks
    (dist.grid_shape: every rank the same problem count where the grid
    divides) — those three exchange the chosen values once, after the
    suggest; every rank returns the whole result, equal to the unsharded
    suggest's (the candidates are keyed on seed, label, new id and global
    index).

    ``joint``: True joins every eligible label (unconditional ``uniform``,
    ``loguniform``, ``normal``, ``lognormal``), a list joins exactly those
    labels: their candidates are whole vectors scored under product-kernel
    mixtures, one argmax picks the vector (DESIGN.md "Joint TPE").  Every other
    label is suggested exactly as without ``joint``.

    ``joint_discrete=True`` (with ``joint``): the group may also hold discrete
    labels — unconditional ``randint`` / ``categorical`` labels (``hp.choice``,
    ``hp.pchoice``) that gate no other label, have 2 to 256 categories and
    no prior probability 0.  ``joint=True`` then joins every such label too and
    a list may name them; a named gate, conditional or quantised label raises
    ValueError.  A group that ends up with no discrete label is the continuous
    stage, byte for byte.

    ``joint_quantized=True`` (with ``joint``): the group may also hold
    unconditional ``quniform`` / ``qloguniform`` labels with q > 0 and 2 to 256
    lattice values — at most 4 of them with 512 lattice values in all, beside at
    most 8 continuous and 4 discrete labels (DESIGN.md "Quantised labels in the
    joint stage").  Their joined values are ``np.float64`` multiples of q.
    ``qnormal`` / ``qlognormal`` labels stay univariate.  A group that ends up
    with no quantised label is the stage without the keyword, byte for byte.

    ``joint_wide=True`` (with ``joint``): a group may hold 17 to
    TPE_JOINT_WIDE_MAX_DIMS = 64 labels, all of them continuous (the labels
    ``joint`` alone joins); it is scored by the wide stage (DESIGN.md "Wide
    groups"), whose candidates continue the same Philox streams.  A group of at
    most 16 labels takes exactly the path without the keyword, byte for byte.
    64 bounds the set of kernel instantiations; it is not a measured limit.

    ``joint_wide_mixed=True`` (with ``joint``, ``joint_wide`` and
    ``joint_discrete``): a group of 17 to 64 labels may hold 1 to
    TPE_JOINT_WIDE_MAX_CAT = 8 discrete labels (those ``joint_discrete``
    admits, at most 1024 categories in all) beside its continuous ones; it is
    scored by the wide mixed stage (DESIGN.md "Discrete labels in wide groups"):
    the mixed model, kernel coordinates continuous first, then discrete, the
    continuous coordinates drawn as the wide stage draws them.  A group of at
    most 16 labels, and a wide one without a discrete label, take exactly the
    path without the keyword, byte for byte.  A quantised label, more than 8
    discrete labels or more than 64 labels in such a group raise ValueError; 8
    bounds the set of kernel instantiations, it is not a measured limit.  It
    does not combine with ``joint_shard``.

    ``joint_wide_quantized=True`` (with ``joint``, ``joint_wide`` and
    ``joint_quantized``): a root group with 1 to 4 quantised labels that the
    quantised stage does not take (more than 16 labels, more than 8 continuous
    or more than 4 discrete ones) is scored by the wide quantised stage
    (DESIGN.md "Quantised labels in wide groups"): 2 to 64 labels in all, at
    least 1 continuous, at most 512 lattice values, 0 to 8 discrete labels
    (those ``joint_discrete`` admits; ``joint_wide_mixed`` is not needed for
    them) of at most 1024 categories in all; more raises ValueError.  The
    model is the quantised stage's, the kernel coordinates continuous, discrete,
    then quantised, and the continuous and discrete coordinates are drawn as
    the wide mixed stage draws them.  A group the quantised stage takes and a
    group without a quantised label take exactly the path without the keyword,
    byte for byte.  It does not combine with ``joint_shard``, nor with any
    ``joint_liar`` value where the root group takes the new stage.

    ``joint_branches=True`` (with ``joint``): conditional labels are joined
    too, one group per branch (DESIGN.md "Branch groups").  A branch group is
    the ``uniform`` / ``loguniform`` / ``normal`` / ``lognormal`` labels that
    share one condition (gate label, option) and have no other parent; a label
    nested below a conditional gate belongs to its own direct parent's group.
    ``joint=True`` joins every branch group of 2 to 16 labels (one label stays
    univariate, more than 16 raise ValueError) beside the unconditional group,
    which is formed and run exactly as without the keyword and which the other
    three keywords alone widen; it is skipped when fewer than 2 unconditional
    labels are eligible, and at least one group of 2 labels must exist.  A list
    may name conditional continuous labels: the named labels are partitioned by
    condition, and a part of one label raises ValueError.  Gates, labels with
    several parents and conditional discrete or quantised labels stay
    univariate.  Per new id a branch group's winner replaces its labels' values
    only where the branch is taken; every other value, the gates' included, is
    the same bytes as without ``joint``.  All branch groups of a suggest are
    scored by one segmented device stage (Engine.run_joint_segments).

    ``joint_branches_mixed=True`` (with ``joint_branches``): the other keywords
    widen the branch groups too (DESIGN.md "Discrete and quantised labels in
    branch groups").  ``joint_discrete`` then also admits a conditional
    ``randint`` / ``categorical`` label that has exactly one parent (gate,
    option), gates nothing, has 2 to 256 categories and no prior probability 0;
    ``joint_quantized`` a conditional ``quniform`` / ``qloguniform`` label with
    exactly one parent, q > 0 and 2 to 256 lattice values; a list may name such
    labels (each joins the part of its condition; an ineligible one raises
    ValueError).  A branch group that holds a discrete or quantised label takes
    at most 8 continuous, 4 discrete and 4 quantised labels, 1024 categories and
    512 lattice values in all (these bound the set of compiled kernels; they are
    not measurements; more raises ValueError); a group of continuous labels only
    keeps its limit of 16 and its path.  A group's kernel coordinates are its
    continuous, discrete, then quantised labels, and its Philox stream word
    comes from ALL its labels: a branch whose lowest-index label is discrete or
    quantised draws its continuous coordinates from another stream than without
    the keyword.  A joined category is typed as the univariate path types it, a
    quantised value is a multiple of q.  Without the keyword every plan and
    every output byte is what ``joint_branches`` alone gives.

    ``joint_branches_wide=True`` (with ``joint_branches`` and ``joint_wide``):
    ``joint_wide`` widens the branch groups too (DESIGN.md "Wide branch
    groups"): a branch group of continuous labels only may hold 2 to 64 labels
    (more raises ValueError).  The grouping, the model (fitted on the trials
    that took the branch), the ids a group applies to and its stream word are
    those of ``joint_branches``.  Groups of at most 16 labels and every group
    with a discrete or quantised label keep their plan, their stage and their
    bytes; the groups of 17 to 64 labels of a suggest are scored by one call of
    the wide segmented stage (Engine.run_joint_wide_segments), each (id, group)
    problem byte for byte as Engine.run_joint_wide scores it alone.  A branch
    group of more than 16 labels with a discrete or quantised one,
    ``joint_shard`` and ``joint_liar='branches'`` / ``'branches_mixed'`` on a
    plan that holds a wide branch group raise ValueError.  Without the keyword
    17 labels under a gate raise as before.

    ``joint_shard=(rank, world)`` (with ``joint`` and any of the keywords
    above): the candidates of every joint stage are split over the ranks of the
    default process group (DESIGN.md "Sharded joint stage").  The univariate
    pass runs whole on every rank; a rank scores the candidate indices
    dist.shard_range(n_EI_candidates, rank, world) of the root group's stage
    and of the branch stage, and one all-gather per stage brings every rank all
    winner records (joint.combine_records).  Every rank returns the whole
    result, byte for byte that of the same call without the keyword.
    n_EI_candidates < 2^31.  It does not combine with the four ``shard*``
    arguments, and joint_candidate_report does not take it.

    ``joint_liar=True`` (with ``joint``; the root group continuous, at most 16
    labels or, with ``joint_wide``, 17 to 64): the ids of one call pick the
    group's vector greedily, in the order given (DESIGN.md "Batch-aware joint
    suggests").  Id 0 picks as without the keyword; its vector then counts as
    one more bad trial of the above mixture (a "liar"), id 1 picks under that,
    and so on, on the device.  Without it every id of a batch finds the same
    mode.  Only the group's values change: every other label, and with one id
    the whole result, is the same bytes as without the keyword.  A root group
    with a discrete or quantised label, any branch group, ``joint_shard`` and
    the keyword without ``joint`` raise ValueError; joint_candidate_report does
    not take it.

    ``joint_liar='mixed'``: everything True does, and the root group may also
    hold discrete labels (``joint_discrete``), quantised labels
    (``joint_quantized``) or be a wide group with discrete labels
    (``joint_wide_mixed``): DESIGN.md "Batch-aware picks over discrete and
    quantised labels".  A picked category counts as one more trial component of
    the above side with that category, a picked lattice value as a binned
    normal at its fit coordinate.  On a continuous root group it is True byte
    for byte.  Branch groups, ``joint_shard`` and the keyword without ``joint``
    raise as under True; any other value raises ValueError.

    ``joint_liar='branches'`` (with ``joint_branches``): everything 'mixed'
    does on the root group, which need not exist, and every branch group is
    batch-aware too (DESIGN.md "Batch-aware picks in branch groups"): the ids
    that take one branch pick that group's vector greedily, in the order given,
    one chain per branch, all chains in one segmented device stage
    (Engine.run_joint_segments_liar).  Only the branch-group values of ids that
    share their branch with an earlier id change: every other label, a call
    with one id and a call whose ids all take different branches are the same
    bytes as without the keyword; without any branch group in the space it is
    'mixed' byte for byte.  A branch group with a discrete or quantised label
    (``joint_branches_mixed``), ``joint_shard``, and the value without
    ``joint`` or without ``joint_branches`` raise ValueError.  Univariate
    labels, the gates included, stay as they are.

    ``joint_liar='branches_mixed'`` (with ``joint_branches``): everything
    'branches' does, and a branch group may also hold discrete or quantised
    labels (``joint_branches_mixed``; DESIGN.md "Batch-aware picks in mixed
    branch groups"): one chain per branch, all chains in one segmented device
    stage (Engine.run_joint_msegments_liar), a picked category or lattice value
    counting as under 'mixed'.  On a space whose branch groups are all
    continuous, or without a branch group, it is 'branches' byte for byte; one
    id, or ids that all take different branches, are the same bytes as without
    the keyword.  ``joint_shard`` and the value without ``joint`` or without
    ``joint_branches`` raise ValueError."""
    if sampler not in ('philox', 'replay'):
        raise ValueError("sampler must be 'philox' or 'replay'")
    if joint_shard is not None:
        joint_shard = _joint_shard_pair(joint_shard, joint, joint_wide_mixed, joint_wide_quantized)
    liar_mode = _joint_liar_mode(joint_liar)
    if liar_mode:
        _joint_liar_check(joint, joint_shard, mode=liar_mode, joint_branches=joint_branches)
    group, branch_groups = None, []
    if ((joint is not False and joint is not None) or joint_discrete or joint_quantized or joint_wide or joint_branches
            or joint_branches_mixed or joint_branches_wide or joint_wide_mixed or joint_wide_quantized):
        group, branch_groups = _joint_plan(table, joint, sampler, precision,
                                           (shard, shard_ids, shard_labels, shard_grid), joint_discrete,
                                           joint_quantized,
                                           _wide_mode(joint_wide, joint_wide_mixed, joint_wide_quantized),
                                           _branch_mode(joint_branches, joint_branches_wide, joint_wide),
                                           joint_branches_mixed)
        _branch_wide_check((group, branch_groups), joint_shard, liar_mode)
        if liar_mode:
            _joint_liar_check(joint, joint_shard, (group, branch_groups), liar_mode, joint_branches)
            _wide_quant_liar_check(group, liar_mode)
    if sum(a is not None for a in (shard, shard_ids, shard_labels, shard_grid)) > 1:
        raise ValueError('shard, shard_ids, shard_labels and shard_grid are exclusive: one shard axis per suggest')
    if (shard_ids is not None or shard_labels is not None or shard_grid is not None) and sampler == 'replay':
        raise ValueError("sampler='replay' draws on the host from one RandomState stream; it does not shard")
    # (an id array stays one: list() of 4096 numpy ints is ~0.2 ms of objects)
    new_ids = new_ids.reshape(-1) if isinstance(new_ids, np.ndarray) else list(new_ids)
    if shard_ids is not None or shard_labels is not None or shard_grid is not None:
        return _suggest_sharded(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, precision, device,
                                columns, shard_ids, shard_labels, shard_grid)
    if group is not None or branch_groups:
        return _suggest_joint(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, device, columns, group,
                              branch_groups, joint_shard, liar_mode or False)
    return _suggest_local(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, sampler, precision,
                          device, shard, columns)


TPE_JOINT_MAX_DIMS = N.JOINT_MAX_DIMS
TPE_JOINT_WIDE_MAX_DIMS = N.JOINT_WIDE_MAX_DIMS
TPE_JOINT_WIDE_MAX_CAT = N.JOINT_WIDE_MAX_CAT


def _joint_liar_mode(joint_liar):
    """``joint_liar`` as None (off: False or None), True, 'mixed', 'branches' or
    'branches_mixed'; ValueError for anything else (another string, a number)."""
    if joint_liar is None or (isinstance(joint_liar, (bool, np.bool_)) and not joint_liar):
        return None
    if isinstance(joint_liar, (bool, np.bool_)):
        return True
    if isinstance(joint_liar, str) and joint_liar in ('mixed', 'branches', 'branches_mixed'):
        return joint_liar
    raise ValueError("joint_liar must be True or 'mixed', or 'branches' with joint_branches or 'branches_mixed' with "
                     'joint_branches (or False): %r' % (joint_liar,))


def _joint_liar_check(joint, joint_shard, plan=None, mode=True, joint_branches=False):
    """ValueError where ``joint_liar`` (``mode``: True, 'mixed', 'branches' or
    'branches_mixed') does not apply: without ``joint``, with ``joint_shard``,
    'branches' / 'branches_mixed' without ``joint_branches``, and (``plan`` =
    _joint_plan's result) for a root group that is missing or, under True,
    holds a discrete or quantised label, and for any branch group; under
    'branches' for a branch group that holds a discrete or quantised label
    ('branches_mixed' admits it), and under both without any branch group what
    'mixed' raises.  Touches no device."""
    if joint is False or joint is None:
        raise ValueError('joint_liar needs joint=True or joint=[labels]: it only changes how the joint stage picks')
    if joint_shard is not None:
        raise ValueError('joint_liar=%r does not combine with joint_shard' % (mode,))
    if mode in ('branches', 'branches_mixed') and not joint_branches:
        raise ValueError('joint_liar=%r needs joint_branches=True: the keyword that makes branch groups' % (mode,))
    if plan is None:
        return
    group, branch_groups = plan
    if mode == 'branches_mixed' and branch_groups:   # every kind of branch group
        return
    if mode == 'branches' and branch_groups:
        for rows in branch_groups:
            other = [r.label for r in rows if r.dist not in _joint.JOINT_DISTS]
            if other:
                raise ValueError("joint_liar='branches' needs branch groups of continuous labels only "
                                 '(joint_branches_mixed): %r is discrete or quantised' % other[0])
        return
    if mode in ('branches', 'branches_mixed'):   # no branch group in the space: 'mixed'
        mode = 'mixed'
    if branch_groups:
        raise ValueError('joint_liar=%r does not combine with branch groups (joint_branches)' % (mode,))
    if mode == 'mixed':
        if group is None:
            raise ValueError("joint_liar='mixed' needs a root group: there is none")
        return
    other = [r.label for r in (group or ()) if r.dist not in _joint.JOINT_DISTS]
    if group is None or other:
        raise ValueError('joint_liar=True needs a root group of continuous labels only: %s'
                         % ('there is no root group' if group is None else '%r is discrete or quantised' % other[0]))


def _joint_shard_pair(joint_shard, joint, wide_mixed=False, wide_quant=False):
    """(rank, world) of a ``joint_shard`` argument as ints, or None; ValueError
    without ``joint``, with ``joint_wide_mixed`` / ``joint_wide_quantized`` and for anything but a pair of
    ints with 0 <= rank < world.  Touches no device."""
    if joint_shard is None:
        return None
    if joint is False or joint is None:
        raise ValueError('joint_shard needs joint=True or joint=[labels]: it only shards the joint stages')
    if wide_mixed:
        raise ValueError('joint_wide_mixed=True does not combine with joint_shard: the wide mixed stage is not sharded')
    if wide_quant:
        raise ValueError('joint_wide_quantized=True does not combine with joint_shard: the wide quantised stage is '
                         'not sharded')
    ok = isinstance(joint_shard, (tuple, list)) and len(joint_shard) == 2 and \
        all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in joint_shard)
    if not ok or not 0 <= joint_shard[0] < joint_shard[1]:
        raise ValueError('joint_shard must be a pair of ints (rank, world) with 0 <= rank < world: %r' % (joint_shard,))
    return int(joint_shard[0]), int(joint_shard[1])


class _JointParts(object):
    """This rank's part of every joint stage of a ``joint_shard`` suggest: its
    candidate range [lo, hi) of ``C`` and the exchange of the winner records
    (None in a world of one rank, unless dist.EXCHANGE_ALWAYS)."""

    def __init__(self, engine, joint_shard, C):
        import torch.distributed as td
        rank, world = joint_shard
        self.C = int(C)
        if self.C >= 2 ** 31:
            raise ValueError('joint_shard: n_EI_candidates must be below 2^31')
        self.ex = None
        up = td.is_available() and td.is_initialized()
        g_rank, g_world = (td.get_rank(), td.get_world_size()) if up else (0, 1)
        if (g_rank, g_world) != (rank, world):
            raise ValueError('joint_shard (%d, %d) is not this process group (rank %d of %d)'
                             % (rank, world, g_rank, g_world))
        if up and (world > 1 or _dist.EXCHANGE_ALWAYS):
            self.ex = _dist.exchange_for(engine)     # (collective on the first sharded call)
        self.lo, self.hi = _dist.shard_range(self.C, rank, world)

    @property
    def n_cand(self):
        return self.hi - self.lo

    @property
    def shard(self):
        return self.lo, self.C

    def records(self, run, P, dtype):
        """``run()`` gives this rank's [P] records of one stage; all ranks'
        records, combined.  A rank whose stage failed still takes part in the
        gather (status word): every rank raises and none waits."""
        failed, err, rec = False, None, None
        try:
            rec = run()
        except Exception as e:
            failed, err = True, e
        if self.ex is None:
            if err is not None:
                raise err
            return rec
        try:
            stacked = _dist.gather_joint_records(self.ex, rec, P, dtype, failed)
        except RuntimeError:
            if err is not None:
                raise err
            raise
        return _joint.combine_records(stacked)


WIDE_MIXED = 'mixed'
WIDE_QUANT = 'quant'                  # joint_wide_quantized
WIDE_QUANT_MIXED = 'quant_mixed'      # ... together with joint_wide_mixed
_WIDE_QUANT_MODES = (WIDE_QUANT, WIDE_QUANT_MIXED)


def _is_wide_quant(wide):
    return isinstance(wide, str) and wide in _WIDE_QUANT_MODES


def _wide_base(wide):
    """``wide`` (_wide_mode) without ``joint_wide_quantized``: what governs a
    group that the wide quantised stage does not take."""
    if _is_wide_quant(wide):
        return WIDE_MIXED if wide == WIDE_QUANT_MIXED else True
    return wide


def _wide_mode(joint_wide, joint_wide_mixed, joint_wide_quantized=False):
    """The ``wide`` argument of _joint_plan and what it calls: ``joint_wide``
    as given, or WIDE_MIXED where ``joint_wide_mixed`` also admits discrete
    labels to the wide groups, or WIDE_QUANT (with ``joint_wide_mixed``:
    WIDE_QUANT_MIXED) where ``joint_wide_quantized`` admits quantised labels
    beyond the quantised stage's limits; ValueError for one of those keywords
    without ``joint_wide``."""
    if joint_wide_quantized and not joint_wide:
        raise ValueError('joint_wide_quantized=True needs joint_wide=True: it only widens the wide groups')
    if not joint_wide_mixed:
        return WIDE_QUANT if joint_wide_quantized else joint_wide
    if not joint_wide:
        raise ValueError('joint_wide_mixed=True needs joint_wide=True: it only widens the wide groups')
    return WIDE_QUANT_MIXED if joint_wide_quantized else WIDE_MIXED


BRANCH_WIDE = 'wide'                  # joint_branches_wide: the ``branches`` argument of _joint_plan


def _branch_mode(joint_branches, joint_branches_wide, joint_wide):
    """The ``branches`` argument of _joint_plan: ``joint_branches`` as given, or
    BRANCH_WIDE where ``joint_branches_wide`` lets ``joint_wide`` widen the
    branch groups too; ValueError for that keyword without one of the two."""
    if not joint_branches_wide:
        return joint_branches
    if not joint_branches:
        raise ValueError('joint_branches_wide=True needs joint_branches=True: it only widens the branch groups')
    if not joint_wide:
        raise ValueError('joint_branches_wide=True needs joint_wide=True: it lets that keyword widen the branch groups')
    return BRANCH_WIDE


def _is_wide_branch(rows):
    """A branch group that the wide segmented stage takes (it is continuous: _branch_limit)."""
    return len(rows) > TPE_JOINT_MAX_DIMS


def _branch_wide_check(plan, joint_shard, liar_mode):
    """ValueError where a plan that holds a wide branch group (joint_branches_wide)
    meets ``joint_shard`` or a ``joint_liar`` for branch groups: the wide
    segmented stage has neither.  Touches no device."""
    wide = [rows for rows in plan[1] if _is_wide_branch(rows)]
    if not wide:
        return
    key = _branch_condition(wide[0][0])
    where = 'the branch group under option %d of gate %r has %d labels' % (key[1], key[0], len(wide[0]))
    if joint_shard is not None:
        raise ValueError('joint_branches_wide=True does not combine with joint_shard: %s, and the wide segmented stage '
                         'is not sharded' % where)
    if liar_mode in ('branches', 'branches_mixed'):
        raise ValueError('joint_liar=%r does not combine with joint_branches_wide=True: %s, and the batch-aware picks '
                         'take branch groups of at most TPE_JOINT_MAX_DIMS = %d labels'
                         % (liar_mode, where, TPE_JOINT_MAX_DIMS))


def _branch_stages(engine, groups):
    """[(Engine call, indices into ``groups``)] of the segmented stages that
    serve the branch groups ``groups`` (each in kernel coordinate order): the
    groups of at most TPE_JOINT_MAX_DIMS labels and the mixed ones through
    Engine.run_joint_segments, the wide ones through
    Engine.run_joint_wide_segments; a part without groups is left out."""
    narrow = [i for i, rows in enumerate(groups) if not _is_wide_branch(rows)]
    wide = [i for i, rows in enumerate(groups) if _is_wide_branch(rows)]
    return ([(engine.run_joint_segments, narrow)] if narrow else []) + \
        ([(engine.run_joint_wide_segments, wide)] if wide else [])


def _joint_group(table, joint, sampler, precision, shards, discrete=False, quantized=False, wide=False):
    """The ParamRows a ``joint`` argument joins, in table order (``discrete`` /
    ``quantized``: the eligible discrete / quantised labels among them;
    ``wide``: more than TPE_JOINT_MAX_DIMS continuous labels allowed, as
    WIDE_MIXED up to TPE_JOINT_WIDE_MAX_CAT discrete ones among them);
    ValueError for every combination the joint stage does not take.  Touches no
    device."""
    _joint_restrictions(joint, sampler, precision, shards, discrete, quantized, wide)
    rows = _joint_rows(table, joint, discrete, quantized)
    if len(rows) < 2:
        raise ValueError('joint needs at least 2 labels to join, got %d' % len(rows))
    return _joint_limits(rows, wide)


def _joint_restrictions(joint, sampler, precision, shards, discrete=False, quantized=False, wide=False,
                        branches=False, branch_mixed=False):
    """ValueError for a keyword without ``joint`` (or without the keywords it
    widens) and for the sampler, precision and shard arguments the joint stage
    does not combine with."""
    if _is_wide_quant(wide):
        if joint is False or joint is None:
            raise ValueError('joint_wide_quantized=True needs joint=True or joint=[labels]: it only widens what joint '
                             'joins')
        if not quantized:
            raise ValueError('joint_wide_quantized=True needs joint_quantized=True: it only admits the quantised '
                             'labels that keyword joins to the wide groups')
    if _wide_base(wide) == WIDE_MIXED and not discrete:
        raise ValueError('joint_wide_mixed=True needs joint_discrete=True: it only admits the discrete labels that '
                         'keyword joins to the wide groups')
    if branch_mixed and not branches:
        raise ValueError('joint_branches_mixed=True needs joint_branches=True: it only widens the branch groups')
    if branches and (joint is False or joint is None):
        raise ValueError('joint_branches=True needs joint=True or joint=[labels]: it only widens what joint joins')
    if wide and (joint is False or joint is None):
        raise ValueError('joint_wide=True needs joint=True or joint=[labels]: it only widens what joint joins')
    if discrete and (joint is False or joint is None):
        raise ValueError('joint_discrete=True needs joint=True or joint=[labels]: it only widens what joint joins')
    if quantized and (joint is False or joint is None):
        raise ValueError('joint_quantized=True needs joint=True or joint=[labels]: it only widens what joint joins')
    if sampler == 'replay':
        raise ValueError("joint does not combine with sampler='replay': the joint candidates are Philox draws")
    if precision == 'fp64':
        raise ValueError("joint does not combine with precision='fp64': the joint stage scores in fp32")
    if any(a is not None for a in shards):
        raise ValueError('joint does not combine with a shard argument')


def _joint_rows(table, joint, discrete=False, quantized=False):
    """The unconditional rows ``joint`` (True or a list of labels) selects, in
    table order; ValueError for a listed label that cannot be joined."""
    if joint is True:
        rows = [r for r in table.rows if _joint.eligible(r) or (discrete and _joint.eligible_discrete(r, table))
                or (quantized and _joint.eligible_quant(r, table))]
    else:
        if isinstance(joint, str):
            raise ValueError('joint must be True or a list of labels, not the string %r' % joint)
        want = list(joint)
        for label in want:
            r = table.by_label.get(label)
            if r is None:
                raise ValueError('joint: %r is not a label of the space' % (label,))
            if quantized and r.dist.startswith('q'):
                why = _joint.quant_reason(r, table)
                if why is not None:
                    raise ValueError('joint: label %r is not eligible with joint_quantized=True: %s' % (label, why))
            elif discrete and not _joint.eligible(r):
                why = _joint.discrete_reason(r, table)
                if why is not None:
                    raise ValueError('joint: label %r is not eligible with joint_discrete=True: %s' % (label, why))
            elif not _joint.eligible(r):
                raise ValueError('joint: label %r is not eligible (%s%s): only unconditional uniform, loguniform, '
                                 'normal and lognormal labels are joined'
                                 % (label, r.dist, '' if all(p is None for p in r.parents) else ', conditional'))
        rows = [r for r in table.rows if r.label in set(want)]
    return rows


def _joint_limits(rows, wide=False):
    """``rows`` (at least 2), or ValueError where the group exceeds what one
    joint stage takes (``wide`` = WIDE_MIXED: a wide group may hold 1 to
    TPE_JOINT_WIDE_MAX_CAT discrete labels; WIDE_QUANT / WIDE_QUANT_MIXED: a
    group with a quantised label that the quantised stage does not take is held
    to the wide quantised stage's limits, every other group to those without
    ``joint_wide_quantized``)."""
    if _is_wide_quant(wide):
        if _takes_wide_quant(rows):
            return _wide_quant_limits(rows)
        wide = _wide_base(wide)
    if len(rows) > TPE_JOINT_MAX_DIMS:
        if not wide:
            raise ValueError('joint joins at most TPE_JOINT_MAX_DIMS = %d labels, not %d: pass the labels to join as '
                             'joint=[...]' % (TPE_JOINT_MAX_DIMS, len(rows)))
        if len(rows) > TPE_JOINT_WIDE_MAX_DIMS:
            raise ValueError('joint with joint_wide=True joins at most TPE_JOINT_WIDE_MAX_DIMS = %d labels, not %d: '
                             'pass the labels to join as joint=[...]' % (TPE_JOINT_WIDE_MAX_DIMS, len(rows)))
        n_disc = sum(1 for r in rows if r.categorical)
        n_quant = sum(1 for r in rows if r.dist in _joint.QUANT_DISTS)
        if wide == WIDE_MIXED:
            head = 'joint with joint_wide_mixed=True: a group of more than TPE_JOINT_MAX_DIMS = %d labels joins ' \
                % TPE_JOINT_MAX_DIMS
            tail = ' among its %d: pass the labels to join as joint=[...]' % len(rows)
            n_cats = sum(int(r.args['upper']) for r in rows if r.categorical)
            if n_quant:
                raise ValueError('%sno quantised label, not %d quantised and %d discrete ones%s'
                                 % (head, n_quant, n_disc, tail))
            if n_disc > TPE_JOINT_WIDE_MAX_CAT:
                raise ValueError('%sat most TPE_JOINT_WIDE_MAX_CAT = %d discrete labels, not %d%s'
                                 % (head, TPE_JOINT_WIDE_MAX_CAT, n_disc, tail))
            if n_cats > N.JOINT_MAX_CAT_TOTAL:
                raise ValueError('%sdiscrete labels of at most TPE_JOINT_MAX_CAT_TOTAL = %d categories in all, not %d%s'
                                 % (head, N.JOINT_MAX_CAT_TOTAL, n_cats, tail))
            return rows
        if n_disc or n_quant:
            raise ValueError('joint with joint_wide=True: a group of more than TPE_JOINT_MAX_DIMS = %d labels joins '
                             'continuous labels only, not %d discrete and %d quantised ones among its %d: pass the '
                             'labels to join as joint=[...]' % (TPE_JOINT_MAX_DIMS, n_disc, n_quant, len(rows)))
        return rows
    n_cats = sum(int(r.args['upper']) for r in rows if r.categorical)
    if n_cats > N.JOINT_MAX_CAT_TOTAL:
        raise ValueError('joint joins discrete labels of at most TPE_JOINT_MAX_CAT_TOTAL = %d categories in all, not '
                         '%d: pass the labels to join as joint=[...]' % (N.JOINT_MAX_CAT_TOTAL, n_cats))
    qrows = [r for r in rows if r.dist in _joint.QUANT_DISTS]
    if qrows:
        n_disc = sum(1 for r in rows if r.categorical)
        n_cont = len(rows) - len(qrows) - n_disc
        n_lat = sum(_joint.lattice_size(r.dist, r.args)[1] for r in qrows)
        tail = ': pass the labels to join as joint=[...]'
        if len(qrows) > N.JOINT_MAX_QUANT:
            raise ValueError('joint joins at most TPE_JOINT_MAX_QUANT = %d quantised labels, not %d%s'
                             % (N.JOINT_MAX_QUANT, len(qrows), tail))
        if n_lat > N.JOINT_MAX_LATTICE_TOTAL:
            raise ValueError('joint joins quantised labels of at most TPE_JOINT_MAX_LATTICE_TOTAL = %d lattice values '
                             'in all, not %d%s' % (N.JOINT_MAX_LATTICE_TOTAL, n_lat, tail))
        if n_cont > N.JOINT_QUANT_MAX_CONT:
            raise ValueError('joint joins at most %d continuous labels beside a quantised one, not %d%s'
                             % (N.JOINT_QUANT_MAX_CONT, n_cont, tail))
        if n_disc > N.JOINT_QUANT_MAX_DISC:
            raise ValueError('joint joins at most %d discrete labels beside a quantised one, not %d%s'
                             % (N.JOINT_QUANT_MAX_DISC, n_disc, tail))
    return rows


def _takes_wide_quant(rows):
    """Whether a root group holds a quantised label and does not fit the
    quantised stage (more than TPE_JOINT_MAX_DIMS labels, more than 8
    continuous or more than 4 discrete ones): under ``joint_wide_quantized``
    the wide quantised stage takes it."""
    n_quant = sum(1 for r in rows if r.dist in _joint.QUANT_DISTS)
    if not n_quant:
        return False
    n_disc = sum(1 for r in rows if r.categorical)
    return (len(rows) > TPE_JOINT_MAX_DIMS or len(rows) - n_quant - n_disc > N.JOINT_QUANT_MAX_CONT
            or n_disc > N.JOINT_QUANT_MAX_DISC)


def _wide_quant_limits(rows):
    """``rows`` of a group the wide quantised stage takes, or ValueError where
    it exceeds that stage's limits (they bound the set of compiled kernels)."""
    n_disc = sum(1 for r in rows if r.categorical)
    qrows = [r for r in rows if r.dist in _joint.QUANT_DISTS]
    n_cont = len(rows) - len(qrows) - n_disc
    n_cats = sum(int(r.args['upper']) for r in rows if r.categorical)
    n_lat = sum(_joint.lattice_size(r.dist, r.args)[1] for r in qrows)
    head = 'joint with joint_wide_quantized=True: a group with quantised labels beyond the quantised stage joins '
    tail = ' among its %d: pass the labels to join as joint=[...]' % len(rows)
    if len(rows) > TPE_JOINT_WIDE_MAX_DIMS:
        raise ValueError('%sat most TPE_JOINT_WIDE_MAX_DIMS = %d labels, not %d%s'
                         % (head, TPE_JOINT_WIDE_MAX_DIMS, len(rows), tail))
    if n_cont < 1:
        raise ValueError('%sat least 1 continuous label, not %d%s' % (head, n_cont, tail))
    if len(qrows) > N.JOINT_MAX_QUANT:
        raise ValueError('%sat most TPE_JOINT_MAX_QUANT = %d quantised labels, not %d%s'
                         % (head, N.JOINT_MAX_QUANT, len(qrows), tail))
    if n_lat > N.JOINT_MAX_LATTICE_TOTAL:
        raise ValueError('%squantised labels of at most TPE_JOINT_MAX_LATTICE_TOTAL = %d lattice values in all, not '
                         '%d%s' % (head, N.JOINT_MAX_LATTICE_TOTAL, n_lat, tail))
    if n_disc > TPE_JOINT_WIDE_MAX_CAT:
        raise ValueError('%sat most TPE_JOINT_WIDE_MAX_CAT = %d discrete labels, not %d%s'
                         % (head, TPE_JOINT_WIDE_MAX_CAT, n_disc, tail))
    if n_cats > N.JOINT_MAX_CAT_TOTAL:
        raise ValueError('%sdiscrete labels of at most TPE_JOINT_MAX_CAT_TOTAL = %d categories in all, not %d%s'
                         % (head, N.JOINT_MAX_CAT_TOTAL, n_cats, tail))
    return rows


def _wide_quant_liar_check(group, mode):
    """ValueError where ``joint_liar`` meets a root group that takes the wide
    quantised stage: tpe_joint_liar_mixed does not take such a group."""
    if group is not None and _takes_wide_quant(group):
        raise ValueError('joint_liar=%r does not combine with a root group that takes the wide quantised stage '
                         '(joint_wide_quantized): more than 8 continuous or 4 discrete labels beside a quantised one'
                         % (mode,))


def _joint_kernel_order(group):
    """(continuous, discrete, quantised) rows of a joint group, each in table
    order: concatenated, the kernel coordinate order."""
    drows = [r for r in group if r.categorical]
    qrows = [r for r in group if r.dist in _joint.QUANT_DISTS]
    return [r for r in group if not r.categorical and r.dist not in _joint.QUANT_DISTS], drows, qrows


def _branch_key(row):
    """(gate label, option) of a continuous label under exactly one condition
    (a label a branch group may hold), else None."""
    if row.dist in _joint.JOINT_DISTS and len(row.parents) == 1 and row.parents[0] is not None:
        return tuple(row.parents[0])
    return None


def _branch_condition(row):
    """(gate label, option) of a label under exactly one condition, else None."""
    if len(row.parents) == 1 and row.parents[0] is not None:
        return tuple(row.parents[0])
    return None


def _branch_mixed_reason(row, table, discrete, quantized):
    """Why a conditional ``row`` joins no branch group under
    ``joint_branches_mixed``, or None if it joins the group of its condition."""
    if _branch_key(row) is not None:
        return None
    if quantized and row.dist.startswith('q'):
        why = _joint.quant_reason(row, table, conditional=True)
    elif discrete and row.categorical:
        why = _joint.discrete_reason(row, table, conditional=True)
    else:
        return 'not a label that the joint keywords given admit to a branch group (%s)' % row.dist
    if why is None and _branch_condition(row) is None:
        why = ('it has %d parents: a label that several branches share belongs to no single branch group'
               % len(row.parents))
    return why


def _branch_mixed_limit(key, rows, wide=False):
    """``rows`` of the branch group under ``key``, or ValueError where it
    exceeds what the segmented stage takes: a group with a discrete or
    quantised label is bound by the quantised stage's limits (they bound the
    set of compiled kernels), a continuous one by _branch_limit.  ``wide``
    (joint_branches_wide) widens the continuous groups only."""
    crows, drows, qrows = _joint_kernel_order(rows)
    if not drows and not qrows:
        return _branch_limit(key, rows, wide)
    if wide and len(rows) > TPE_JOINT_MAX_DIMS:
        raise ValueError('joint with joint_branches_wide=True: the branch group under option %d of gate %r has %d '
                         'labels, more than TPE_JOINT_MAX_DIMS = %d, and %r is discrete or quantised: a wide branch '
                         'group holds continuous labels only: pass the labels to join as joint=[...]'
                         % (key[1], key[0], len(rows), TPE_JOINT_MAX_DIMS, (drows + qrows)[0].label))
    head = 'joint with joint_branches_mixed=True: the branch group under option %d of gate %r has ' % (key[1], key[0])
    tail = ': pass the labels to join as joint=[...]'
    n_cats = sum(int(r.args['upper']) for r in drows)
    n_lat = sum(_joint.lattice_size(r.dist, r.args)[1] for r in qrows)
    if len(crows) > N.JOINT_QUANT_MAX_CONT:
        raise ValueError('%s%d continuous labels beside a discrete or quantised one, more than %d%s'
                         % (head, len(crows), N.JOINT_QUANT_MAX_CONT, tail))
    if len(drows) > N.JOINT_QUANT_MAX_DISC:
        raise ValueError('%s%d discrete labels, more than %d%s' % (head, len(drows), N.JOINT_QUANT_MAX_DISC, tail))
    if len(qrows) > N.JOINT_MAX_QUANT:
        raise ValueError('%s%d quantised labels, more than TPE_JOINT_MAX_QUANT = %d%s'
                         % (head, len(qrows), N.JOINT_MAX_QUANT, tail))
    if n_cats > N.JOINT_MAX_CAT_TOTAL:
        raise ValueError('%s%d categories in all, more than TPE_JOINT_MAX_CAT_TOTAL = %d%s'
                         % (head, n_cats, N.JOINT_MAX_CAT_TOTAL, tail))
    if n_lat > N.JOINT_MAX_LATTICE_TOTAL:
        raise ValueError('%s%d lattice values in all, more than TPE_JOINT_MAX_LATTICE_TOTAL = %d%s'
                         % (head, n_lat, N.JOINT_MAX_LATTICE_TOTAL, tail))
    return rows


def _branch_limit(key, rows, wide=False):
    if wide and len(rows) > TPE_JOINT_WIDE_MAX_DIMS:
        raise ValueError('joint with joint_branches_wide=True: the branch group under option %d of gate %r has %d '
                         'labels, more than TPE_JOINT_WIDE_MAX_DIMS = %d: pass the labels to join as joint=[...]'
                         % (key[1], key[0], len(rows), TPE_JOINT_WIDE_MAX_DIMS))
    if not wide and len(rows) > TPE_JOINT_MAX_DIMS:
        raise ValueError('joint with joint_branches=True: the branch group under option %d of gate %r has %d labels, '
                         'more than TPE_JOINT_MAX_DIMS = %d: pass the labels to join as joint=[...]'
                         % (key[1], key[0], len(rows), TPE_JOINT_MAX_DIMS))
    return rows


def _joint_plan(table, joint, sampler, precision, shards, discrete=False, quantized=False, wide=False,
                branches=False, branch_mixed=False):
    """(root group or None, branch groups) of a ``joint`` argument.  Without
    ``branches``: (_joint_group(...), []).  With it (DESIGN.md "Branch
    groups"): the root group as _joint_group forms it, or None where fewer than
    2 unconditional labels are joined, and one list of ParamRows (table order)
    per condition with 2 to TPE_JOINT_MAX_DIMS joined labels, ordered by their
    first label.  ``branch_mixed``: ``discrete`` / ``quantized`` also admit
    conditional discrete / quantised labels with exactly one parent to the
    group of their condition (_branch_mixed_reason, _branch_mixed_limit).
    ``wide`` (_wide_mode, WIDE_QUANT among its values) widens the root group only (_joint_limits),
    unless ``branches`` is BRANCH_WIDE (_branch_mode): then a branch group of continuous
    labels holds up to TPE_JOINT_WIDE_MAX_DIMS of them.
    ValueError as _joint_group; touches no device."""
    if not branches:
        if branch_mixed:
            raise ValueError('joint_branches_mixed=True needs joint_branches=True: it only widens the branch groups')
        return _joint_group(table, joint, sampler, precision, shards, discrete, quantized, wide), []
    _joint_restrictions(joint, sampler, precision, shards, discrete, quantized, wide, True, branch_mixed)
    parts = {}
    branch_wide = isinstance(branches, str) and branches == BRANCH_WIDE

    def limit(key, rows):
        return (_branch_mixed_limit if branch_mixed else _branch_limit)(key, rows, branch_wide)

    def conditional(r):
        return any(p is not None for p in r.parents)
    if joint is True:
        root = _joint_rows(table, True, discrete, quantized)
        for r in table.rows:
            key = _branch_key(r)
            if key is None and branch_mixed and conditional(r) and \
                    _branch_mixed_reason(r, table, discrete, quantized) is None:
                key = _branch_condition(r)
            if key is not None:
                parts.setdefault(key, []).append(r)
        groups = [limit(key, rows) for key, rows in parts.items() if len(rows) >= 2]
        root = root if len(root) >= 2 else None
    else:
        if isinstance(joint, str):
            raise ValueError('joint must be True or a list of labels, not the string %r' % joint)
        want = list(joint)
        named = set(label for label in want if label in table.by_label and _branch_key(table.by_label[label]))
        if branch_mixed:
            for label in want:
                r = table.by_label.get(label)
                if r is None or label in named or not conditional(r):
                    continue
                if (quantized and r.dist.startswith('q')) or (discrete and r.categorical):
                    why = _branch_mixed_reason(r, table, discrete, quantized)
                    if why is not None:
                        raise ValueError('joint: label %r is not eligible with joint_branches_mixed=True: %s'
                                         % (label, why))
                    named.add(label)
        root = _joint_rows(table, [label for label in want if label not in named], discrete, quantized)
        if len(root) == 1:
            raise ValueError('joint with joint_branches=True: %r is the only unconditional label named: a group needs '
                             'at least 2 labels' % root[0].label)
        for r in table.rows:
            if r.label in named:
                parts.setdefault(_branch_condition(r), []).append(r)
        for key, rows in parts.items():
            if len(rows) == 1:
                raise ValueError('joint with joint_branches=True: %r is the only label named under option %d of gate '
                                 '%r: a group needs at least 2 labels' % (rows[0].label, key[1], key[0]))
        groups = [limit(key, rows) for key, rows in parts.items()]
        root = root or None
    if root is None and not groups:
        raise ValueError('joint needs at least 2 labels to join in one group (the unconditional labels, or the labels '
                         'of one branch), and there is none')
    return (None if root is None else _joint_limits(root, wide)), groups


def _run_root_group(engine, group, hist, ids, seed, prior_weight, n_EI_candidates, gamma, **kw):
    """Fit the root group's model and run its joint stage: (the group in kernel
    coordinate order, the model, what the engine call returned).  ``kw``: more
    keywords of the Engine.run_joint* call (report_k, return_cand, want_lg)."""
    crows, drows, qrows = _joint_kernel_order(group)
    if qrows:                                    # kernel coordinates: continuous, discrete, then quantised labels
        group = crows + drows + qrows
        model = _joint.fit_quant_model(crows, drows, qrows, hist, _history.split_below(hist, gamma), prior_weight,
                                       DEFAULT_LF)
        if kw.pop('liar', False):                # (joint_liar='mixed': W as below, the lattice values' fit coordinates)
            _wide_quant_liar_check(group, 'mixed')
            out = engine.run_joint_liar_mixed(
                model.below[:3], model.above[:3], model.low, model.high, model.cats(), model.quants(), ids,
                int(n_EI_candidates), seed, centres=model.centres(),
                liar=_joint.side_weight_sum(len(model.above[0]) - 1, prior_weight, DEFAULT_LF), **kw)
        else:
            # beyond the quantised stage's limits (joint_wide_quantized=True let the group through): the wide one
            run = engine.run_joint_wide_quant if _takes_wide_quant(group) else engine.run_joint_quant
            out = run(model.below[:3], model.above[:3], model.low, model.high, model.cats(), model.quants(), ids,
                      int(n_EI_candidates), seed, **kw)
    elif drows:                                  # kernel coordinates: the continuous labels, then the discrete ones
        group = [r for r in group if not r.categorical] + drows
        model = _joint.fit_mixed_model(group[:len(group) - len(drows)], drows, hist,
                                       _history.split_below(hist, gamma), prior_weight, DEFAULT_LF)
        # more than TPE_JOINT_MAX_DIMS labels (joint_wide_mixed=True let them through): the wide mixed stage
        run = engine.run_joint_wide_mixed if len(group) > TPE_JOINT_MAX_DIMS else engine.run_joint_mixed
        if kw.pop('liar', False):                # (the stage `run` names, then tpe_joint_liar_mixed)
            out = engine.run_joint_liar_mixed(
                model.below[:3], model.above[:3], model.low, model.high, model.cats(), (), ids, int(n_EI_candidates),
                seed, liar=_joint.side_weight_sum(len(model.above[0]) - 1, prior_weight, DEFAULT_LF), **kw)
        else:
            out = run(model.below[:3], model.above[:3], model.low, model.high, model.cats(), ids,
                      int(n_EI_candidates), seed, **kw)
    else:
        model = _joint.fit_model(group, hist, _history.split_below(hist, gamma), prior_weight, DEFAULT_LF)
        # more than TPE_JOINT_MAX_DIMS labels (joint_wide=True let them through): the wide stage
        run = engine.run_joint_wide if len(group) > TPE_JOINT_MAX_DIMS else engine.run_joint
        if kw.pop('liar', False):                # (joint_liar: W of the above side as side_mixture weighs it)
            kw['liar'] = _joint.side_weight_sum(len(model.above[0]) - 1, prior_weight, DEFAULT_LF)
        out = run(model.below, model.above, model.low, model.high, ids, int(n_EI_candidates), seed, **kw)
    return group, model, out


def _suggest_joint(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, device, columns, group,
                   branch_groups=(), joint_shard=None, joint_liar=False):
    """The univariate suggest of every label (the joined labels' univariate
    winners are discarded: each costs one problem of the level's batch, and the
    other labels' values are then the same bytes as without ``joint``), then
    one joint stage over the root group (if any), whose winner fills the
    group's columns, then one segmented stage over the branch groups: group g
    applies to the ids for which its labels are active, and its winners fill
    its columns for those ids only (a joined label gates nothing, so the
    routing is the univariate pass's).  ``joint_shard``: the two joint stages
    run over this rank's candidate range and exchange their records
    (_JointParts); the univariate pass is replicated.  ``joint_liar`` (False,
    True, 'mixed', 'branches' or 'branches_mixed'): the root group's ids pick
    greedily (Engine.run_joint's ``liar``); 'branches' / 'branches_mixed': so do
    the ids of every branch group (Engine.run_joint_segments_liar /
    run_joint_msegments_liar)."""
    cc = _suggest_local(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, 'philox', 'fp32', device,
                        None, True)
    if len(cc) == 0:
        return cc if columns else []
    engine = get_engine(device, 'fp32')
    ids = np.asarray(new_ids, dtype=np.int64).reshape(-1)
    values = np.array(cc.values, dtype=np.float64)
    active = np.array(cc.active, dtype=bool)
    parts = None if joint_shard is None else _JointParts(engine, joint_shard, n_EI_candidates)
    if group is not None and parts is not None:
        got = []

        def run():
            got[:] = _run_root_group(engine, group, hist, ids, seed, prior_weight, parts.n_cand, gamma,
                                     shard=parts.shard)
            return got[2]
        rec = parts.records(run, len(ids), N.JOINT_WIDE_RECORD_DTYPE if len(group) > TPE_JOINT_MAX_DIMS
                            else N.JOINT_RECORD_DTYPE)
        group, model = got[0], got[1]
    elif group is not None:
        group, model, rec = _run_root_group(engine, group, hist, ids, seed, prior_weight, n_EI_candidates, gamma,
                                            **({'liar': True} if joint_liar else {}))
    if group is not None:
        if (rec['global_idx'] < 0).any():
            raise RuntimeError('no joint candidate selected')
        vals = model.values(rec['z'][:, :len(group)])
        for d, r in enumerate(group):
            values[:, r.index] = vals[:, d]
            active[:, r.index] = True
    if branch_groups:
        _suggest_branches(engine, hist, ids, seed, prior_weight, n_EI_candidates, gamma, branch_groups,
                          np.asarray(cc.active, dtype=bool), values, parts,
                          joint_liar if joint_liar in ('branches', 'branches_mixed') else False)
    cc = ChoiceColumns(table.labels, values, active)
    return cc if columns else cc.dicts(table)


def _fit_branch_model(rows, hist, below_tids, prior_weight):
    """(the branch group in kernel coordinate order, its model): a JointModel
    for continuous labels, a MixedModel with discrete labels, a QuantModel with
    quantised ones — each fitted on the trials that took the branch."""
    crows, drows, qrows = _joint_kernel_order(rows)
    if qrows:
        return crows + drows + qrows, _joint.fit_quant_model(crows, drows, qrows, hist, below_tids, prior_weight,
                                                              DEFAULT_LF)
    if drows:
        return crows + drows, _joint.fit_mixed_model(crows, drows, hist, below_tids, prior_weight, DEFAULT_LF)
    return rows, _joint.fit_model(rows, hist, below_tids, prior_weight, DEFAULT_LF)


def _suggest_branches(engine, hist, ids, seed, prior_weight, n_EI_candidates, gamma, branch_groups, taken, values,
                      parts=None, liar=False):
    """The segmented joint stage of a suggest: one problem per (new id, branch
    group whose labels are active for it in ``taken`` [n_ids x n_labels]), all
    in one Engine.run_joint_segments call; the winners overwrite ``values``.
    ``parts`` (_JointParts): the call covers this rank's candidates, and the
    records of all ranks are combined.  ``liar`` (joint_liar='branches'): the ids
    that take one branch pick its vector greedily, in the order given
    (Engine.run_joint_segments_liar, W of every group's above side as
    side_mixture weighs it); 'branches_mixed': the same over groups that may
    hold discrete or quantised labels (Engine.run_joint_msegments_liar, with
    each model's centres())."""
    below_tids = _history.split_below(hist, gamma)
    models, words, prob_seg, prob_id, where = [], [], [], [], []
    for rows in branch_groups:
        on = taken[:, rows[0].index]
        for r in rows[1:]:
            assert (taken[:, r.index] == on).all(), ('labels of one branch group differ in activity', rows[0].label,
                                                     r.label)
        js = np.flatnonzero(on)
        if len(js) == 0:                             # no new id takes this branch
            continue
        prob_seg.extend([len(models)] * len(js))
        prob_id.extend(ids[js])
        rows, model = _fit_branch_model(rows, hist, below_tids, prior_weight)
        where.append((rows, js))
        models.append(model)
        words.append(_joint.branch_stream_word(rows))
    if not models:
        return
    if liar:
        assert parts is None, 'joint_liar does not combine with joint_shard'
        W = [_joint.side_weight_sum(len(m.above[0]) - 1, prior_weight, DEFAULT_LF) for m in models]
        if liar == 'branches_mixed':
            rec = engine.run_joint_msegments_liar(
                models, words, prob_seg, prob_id, int(n_EI_candidates), seed, liar=W,
                centres=[m.centres() if hasattr(m, 'centres') else None for m in models])
        else:
            rec = engine.run_joint_segments_liar(models, words, prob_seg, prob_id, int(n_EI_candidates), seed, liar=W)
    elif parts is None and not any(_is_wide_branch(w[0]) for w in where):
        rec = engine.run_joint_segments(models, words, prob_seg, prob_id, int(n_EI_candidates), seed)
    elif parts is None:
        # joint_branches_wide: the wide groups' problems in one call of their own, the others' in the call above
        rec = np.zeros(len(prob_seg), dtype=N.JOINT_WIDE_RECORD_DTYPE)
        seg = np.asarray(prob_seg)
        for run, sel in _branch_stages(engine, [w[0] for w in where]):
            local = np.full(len(models), -1)
            local[sel] = np.arange(len(sel))
            at = np.flatnonzero(local[seg] >= 0)
            got = run([models[i] for i in sel], [words[i] for i in sel], local[seg[at]],
                      np.asarray(prob_id, dtype=np.int64)[at], int(n_EI_candidates), seed)
            for f in ('global_idx', 'l', 'g'):
                rec[f][at] = got[f]
            rec['z'][at, :got['z'].shape[1]] = got['z']
    else:
        rec = parts.records(lambda: engine.run_joint_segments(models, words, prob_seg, prob_id, parts.n_cand, seed,
                                                              shard=parts.shard), len(prob_seg), N.JOINT_RECORD_DTYPE)
    if (rec['global_idx'] < 0).any():
        raise RuntimeError('no joint candidate selected')
    p = 0
    for (rows, js), model in zip(where, models):
        vals = model.values(rec['z'][p:p + len(js), :len(rows)])
        for d, r in enumerate(rows):
            values[js, r.index] = vals[:, d]
        p += len(js)


def _suggest_local(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, sampler, precision, device,
                   shard, columns, remote=(), borrow=False):
    engine = get_engine(device, precision)
    below_tids = _history.split_below(hist, gamma)
    C = int(n_EI_candidates)
    if sampler == 'philox' and NATIVE_TREE and precision == 'fp32':
        out = _choices_native(table, hist, below_tids, new_ids, seed, C, engine, prior_weight, shard,
                              columns, remote, borrow)
        if out is not None:
            return out
    fits = _Fits(table, hist, below_tids, prior_weight, engine)
    if sampler == 'philox':
        out = _choices_philox(table, fits, new_ids, seed, C, engine, shard, remote)
    elif shard is not None:
        raise ValueError("sampler='replay' draws on the host; it does not shard")
    else:
        out = _choices_replay(table, fits, new_ids, seed, C, engine)
    return ChoiceColumns.from_dicts(table, out) if columns else out


def _suggest_sharded(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, precision, device, columns,
                     shard_ids, shard_labels, shard_grid=None):
    """New-id, hyperparameter or 2-D axis (dist.py): this rank's part of the
    suggest as columns, then one all-gather of the chosen values."""
    rank, world = next(a for a in (shard_ids, shard_labels, shard_grid) if a is not None)[:2]
    engine = get_engine(device, precision)
    ex = _dist.exchange_for(engine)          # (collective on the first sharded call)
    if ex.world != world or ex.rank != rank:
        raise ValueError('shard (%d, %d) is not this process group (rank %d of %d)'
                         % (rank, world, ex.rank, ex.world))
    n, L = len(new_ids), len(table.rows)
    failed, err = False, None
    if shard_grid is not None:
        gates = set(table.parent_labels)
        if len(shard_grid) > 2:              # (rank, world, G): the label groups given (tests)
            if world % shard_grid[2]:
                raise ValueError('shard_grid: %d label groups do not divide %d ranks' % (shard_grid[2], world))
            shape = (shard_grid[2], world // shard_grid[2])
        else:
            shape = _dist.grid_shape(sum(1 for r in table.rows if r.label not in gates), n, world,
                                     _dist.label_cost(len(hist), n_EI_candidates))
        g, b = _dist.grid_cell(rank, shape)
        owner = _dist.label_owners(table, shape[0])
        remote = tuple(ix for ix, o in enumerate(owner) if o >= 0 and o != g)
        lo, hi = _dist.shard_range(n, b, shape[1])
        vals, act = np.zeros((0, L)), np.zeros((0, L), dtype=bool)
        try:
            if hi > lo:
                cc = _suggest_local(table, hist, new_ids[lo:hi], seed, prior_weight, n_EI_candidates, gamma,
                                    'philox', precision, device, None, True, remote, borrow=True)
                vals, act = cc.values, np.asarray(cc.active, dtype=bool)
        except Exception as e:               # (still takes part in the gather: no rank waits forever)
            failed, err = True, e
        try:
            vals, act = _dist.gather_grid_blocks(ex, shape, vals, act, n, owner, failed)
        except RuntimeError:
            if err is not None:
                raise err
            raise
    elif shard_ids is not None:
        lo, hi = _dist.shard_range(n, rank, world)
        vals, act = np.zeros((0, L)), np.zeros((0, L), dtype=bool)
        try:
            if hi > lo:
                cc = _suggest_local(table, hist, new_ids[lo:hi], seed, prior_weight, n_EI_candidates, gamma,
                                    'philox', precision, device, None, True, borrow=True)
                vals, act = cc.values, cc.active
        except Exception as e:               # (still takes part in the gather: no rank waits forever)
            failed, err = True, e
        try:
            vals, act = _dist.gather_id_blocks(ex, vals, act, n, L, failed)
        except RuntimeError:
            if err is not None:
                raise err
            raise
    else:
        owner = _dist.label_owners(table, world)
        remote = tuple(ix for ix, o in enumerate(owner) if o >= 0 and o != rank)
        vals, act = np.full((n, L), np.nan), np.zeros((n, L), dtype=bool)
        try:
            cc = _suggest_local(table, hist, new_ids, seed, prior_weight, n_EI_candidates, gamma, 'philox',
                                precision, device, None, True, remote, borrow=True)
            vals, act = cc.values, np.array(cc.active, dtype=bool)      # (the gather copies the values)
        except Exception as e:
            failed, err = True, e
        try:
            vals = _dist.gather_label_columns(ex, vals, owner, failed)
        except RuntimeError:
            if err is not None:
                raise err
            raise
    cc = ChoiceColumns(table.labels, vals, act)
    return cc if columns else cc.dicts(table)


# candidates of one engine run of a candidate report: 2^24 x (cand, l, g, coord,
# sort key and value) is about 1 GB of per-candidate buffers — a bound on
# memory, not a tuning knob
REPORT_MAX_RUN_CANDIDATES = 1 << 24

REPORT_TOP_DTYPE = np.dtype([('value', '<f8'), ('l', '<f8'), ('g', '<f8'), ('score', '<f8'), ('index', '<i8')])


class CandidateReport(object):
    """What the device scored for one new id, per hyperparameter label
    (``candidate_report``):

    labels  the reported labels, in table order
    top     REPORT_TOP_DTYPE [n_labels, k]: the k best DISTINCT candidate
            values of each label in np.argmax order of score = l - g (NaN
            first, then descending, ties to the lower index), each with its
            l = log-density under the below mixture, g = under the above
            mixture and global candidate index; row j holds n_top[j] entries
            (fewer than k when the pool has fewer distinct values), the rest
            are value NaN / index -1.  A categorical label's value is its
            category index (``values`` gives reference-typed values)
    n_top   int [n_labels]
    stats   _native.SCORE_STATS_DTYPE [n_labels]: counts of finite, NaN, +inf
            and -inf scores; mean, m2 = sum (s - mean)^2, min and max of the
            finite ones.  ``mean`` is the Monte-Carlo estimate of
            E_l[log l(x) - log g(x)] over the pool (the candidates are draws
            from l): a summary of how far apart the two fitted densities are,
            nothing more — with the handful of observations the below set
            holds it is as large for a label that does not matter as for one
            that does
    """
    __slots__ = ('labels', 'top', 'n_top', 'stats', '_cat')

    def __init__(self, labels, top, n_top, stats, categorical):
        self.labels, self.top, self.n_top, self.stats = list(labels), top, n_top, stats
        self._cat = list(categorical)

    def __len__(self):
        return len(self.labels)

    def values(self, label):
        """The label's ranked distinct values with the reference's value types
        (np.int64 for categorical labels, np.float64 else)."""
        j = self.labels.index(label)
        v = self.top['value'][j, :int(self.n_top[j])]
        return list(v.astype(np.int64)) if self._cat[j] else list(np.asarray(v, dtype=np.float64))

    def dicts(self):
        """{label: dict(top=[dict(value, l, g, score, index), ...], stats=dict(...))}."""
        out = {}
        for j, lab in enumerate(self.labels):
            vals = self.values(lab)
            rows = [dict(value=vals[i], l=float(e['l']), g=float(e['g']), score=float(e['score']),
                         index=int(e['index'])) for i, e in enumerate(self.top[j, :len(vals)])]
            st = self.stats[j]
            out[lab] = dict(top=rows, stats={f: st[f].item() for f in self.stats.dtype.names})
        return out


def _report_check_k(k):
    k = int(k)
    if k < 1 or k > N.REPORT_MAX_K:
        raise ValueError('k must be in [1, %d]: %r' % (N.REPORT_MAX_K, k))
    return k


def candidate_report_columns(table, hist, new_id, seed, k=8, labels=None, prior_weight=_default_prior_weight,
                             n_EI_candidates=_default_n_EI_candidates, gamma=_default_gamma, precision='fp32',
                             device=None):
    """``candidate_report`` on a structure-of-arrays history (as
    ``suggest_choices`` is to ``suggest``)."""
    k = _report_check_k(k)
    if len(hist) == 0:
        raise ValueError('candidate_report needs a history: no completed trial to fit the posteriors from')
    C = int(n_EI_candidates)
    if C < 1 or C >= 2 ** 31:
        raise ValueError('n_EI_candidates out of range: %r' % C)
    if labels is None:
        rows = list(table.rows)
    else:
        want = set(labels)
        unknown = want - set(table.labels)
        if unknown:
            raise ValueError('not labels of the space: %r' % sorted(unknown))
        rows = [r for r in table.rows if r.label in want]
    engine = get_engine(device, precision)
    fits = _Fits(table, hist, _history.split_below(hist, gamma), prior_weight, engine)
    ids = np.array([int(new_id)], dtype=np.int64)
    n = len(rows)
    top = np.zeros((n, k), dtype=REPORT_TOP_DTYPE)
    n_top = np.zeros(n, dtype=np.int64)
    stats = np.zeros(n, dtype=N.SCORE_STATS_DTYPE)
    per_run = max(1, REPORT_MAX_RUN_CANDIDATES // C)
    for lo in range(0, n, per_run):
        group = rows[lo:lo + per_run]
        # one problem per label, scored as if active: its own Philox stream
        # (seed, label, new id, global index) — the pool a suggest of this id
        # with this seed and candidate count scores where the label is active
        problems = [LevelProblem(fits.get(r), r.index, ids) for r in group]
        _, t, nt, st = engine.run(problems, C, seed, report_k=k)
        if (nt < 0).any():
            raise RuntimeError('candidate report: a problem did not fit its chunk slots')
        sl = slice(lo, lo + len(group))
        for f in ('value', 'l', 'g'):
            top[f][sl] = t[f]
        top['index'][sl] = t['global_idx']
        with np.errstate(invalid='ignore'):
            top['score'][sl] = t['l'] - t['g']
        n_top[sl], stats[sl] = nt, st
    empty = np.arange(k)[None, :] >= n_top[:, None]
    for f in ('value', 'l', 'g', 'score'):
        top[f][empty] = np.nan
    return CandidateReport([r.label for r in rows], top, n_top, stats, [r.categorical for r in rows])


def candidate_report(new_id, domain, trials, seed, k=8, labels=None, prior_weight=_default_prior_weight,
                     n_EI_candidates=_default_n_EI_candidates, gamma=_default_gamma, precision='fp32', device=None):
    """The candidate pool behind a ``suggest([new_id], domain, trials, seed,
    n_EI_candidates=...)``: for every label of the space (or the ``labels``
    subset) the ``k`` best distinct candidate values with their l, g and score,
    and statistics of the label's scores — a CandidateReport.

    Every label is scored as if it were active, its posterior fitted from its
    own observations; labels on a conditional branch the suggest does not take
    are reported too.  The per-candidate arrays never leave the device: the
    ranking and the statistics are device stages (tpe_report).  One new id per
    call; ``k`` in [1, 64]."""
    k = _report_check_k(k)
    hist = _history.extract(domain, trials)
    return candidate_report_columns(domain.table, hist, new_id, seed, k=k, labels=labels, prior_weight=prior_weight,
                                    n_EI_candidates=n_EI_candidates, gamma=gamma, precision=precision,
                                    device=device)


JOINT_REPORT_TOP_DTYPE = np.dtype([('l', '<f8'), ('g', '<f8'), ('score', '<f8'), ('index', '<i8')])


class JointGroupReport(object):
    """One joint group of a JointCandidateReport:

    labels     the group's labels in kernel coordinate order (continuous,
               discrete, quantised; each in table order)
    condition  None for the root group, (gate label, option) for a branch group
    vectors    float64 [n_top, D]: the ranked distinct candidate vectors as label
               values (the group model's ``values()``: exp for the log families,
               category indices, multiples of q)
    top        JOINT_REPORT_TOP_DTYPE [n_top]: l, g, score = l - g and the
               candidate index of each vector, in np.argmax order of score
    n_top      min(k, distinct kernel rows of the pool)
    stats      _native.SCORE_STATS_DTYPE record of all the pool's scores (as
               CandidateReport.stats)
    """
    __slots__ = ('labels', 'condition', 'vectors', 'top', 'n_top', 'stats')

    def __init__(self, labels, condition, vectors, top, n_top, stats):
        self.labels, self.condition, self.vectors = list(labels), condition, vectors
        self.top, self.n_top, self.stats = top, int(n_top), stats


class JointCandidateReport(object):
    """What the joint stages scored for one new id (``joint_candidate_report``):
    ``groups``, one JointGroupReport per joint group — the root group first (if
    any), then the branch groups in plan order.  Iterable and indexable."""
    __slots__ = ('groups',)

    def __init__(self, groups):
        self.groups = list(groups)

    def __len__(self):
        return len(self.groups)

    def __iter__(self):
        return iter(self.groups)

    def __getitem__(self, i):
        return self.groups[i]

    def dicts(self):
        """Per group dict(labels, condition, top=[dict(vector={label: value}, l,
        g, score, index), ...], stats=dict(...))."""
        out = []
        for gr in self.groups:
            rows = [dict(vector={lab: float(v) for lab, v in zip(gr.labels, gr.vectors[i])}, l=float(e['l']),
                         g=float(e['g']), score=float(e['score']), index=int(e['index']))
                    for i, e in enumerate(gr.top)]
            out.append(dict(labels=list(gr.labels), condition=gr.condition, top=rows,
                            stats={f: gr.stats[f].item() for f in gr.stats.dtype.names}))
        return out


def _joint_group_report(rows, condition, model, top, z, n_top, stats):
    n = int(n_top)
    t = np.zeros(n, dtype=JOINT_REPORT_TOP_DTYPE)
    t['l'], t['g'], t['index'] = top['l'][:n], top['g'][:n], top['idx'][:n]
    with np.errstate(invalid='ignore'):
        t['score'] = t['l'] - t['g']
    vectors = model.values(np.asarray(z[:n, :len(rows)], dtype=np.float64)).reshape(n, len(rows))
    return JointGroupReport([r.label for r in rows], condition, vectors, t, n, stats.copy())


def joint_candidate_report_columns(table, hist, new_id, seed, k=8, joint=True, joint_discrete=False,
                                   joint_quantized=False, joint_wide=False, joint_branches=False,
                                   prior_weight=_default_prior_weight, n_EI_candidates=_default_n_EI_candidates,
                                   gamma=_default_gamma, device=None, joint_branches_mixed=False,
                                   joint_branches_wide=False, joint_wide_mixed=False, joint_wide_quantized=False):
    """``joint_candidate_report`` on a structure-of-arrays history (as
    ``candidate_report_columns`` is to ``candidate_report``)."""
    k = _report_check_k(k)
    if joint is False or joint is None:
        raise ValueError('joint_candidate_report needs joint=True or joint=[labels]')
    group, branch_groups = _joint_plan(table, joint, 'philox', 'fp32', (None, None, None, None), joint_discrete,
                                       joint_quantized,
                                       _wide_mode(joint_wide, joint_wide_mixed, joint_wide_quantized),
                                       _branch_mode(joint_branches, joint_branches_wide, joint_wide),
                                       joint_branches_mixed)
    if len(hist) == 0:
        raise ValueError('joint_candidate_report needs a history: no completed trial to fit the models from')
    C = int(n_EI_candidates)
    if C < 1 or C >= 2 ** 31:
        raise ValueError('n_EI_candidates out of range: %r' % C)
    engine = get_engine(device, 'fp32')
    ids = np.array([int(new_id)], dtype=np.int64)
    groups = []
    if group is not None:
        group, model, out = _run_root_group(engine, group, hist, ids, seed, prior_weight, C, gamma, report_k=k)
        top, z, nt, st = out[-4:]
        groups.append(_joint_group_report(group, None, model, top[0], z[0], nt[0], st[0]))
    if branch_groups:
        # every branch group as if active: fitted on the trials that took the
        # branch, scored with its own stream word and this id — the pool a
        # suggest that takes the branch scores
        below_tids = _history.split_below(hist, gamma)
        per_run = max(1, REPORT_MAX_RUN_CANDIDATES // C)
        for lo in range(0, len(branch_groups), per_run):
            fits = [_fit_branch_model(rows, hist, below_tids, prior_weight) for rows in branch_groups[lo:lo + per_run]]
            part, models = [f[0] for f in fits], [f[1] for f in fits]
            words = [_joint.branch_stream_word(rows) for rows in part]
            done = {}
            for run, sel in _branch_stages(engine, part):   # the wide groups through their own stage
                out = run([models[i] for i in sel], [words[i] for i in sel], np.arange(len(sel)),
                          np.repeat(ids, len(sel)), C, seed, report_k=k)
                top, z, nt, st = out[-4:]
                for p, i in enumerate(sel):
                    done[i] = _joint_group_report(part[i], _branch_condition(part[i][0]), models[i], top[p], z[p],
                                                  nt[p], st[p])
            groups.extend(done[i] for i in range(len(part)))
    return JointCandidateReport(groups)


def joint_candidate_report(new_id, domain, trials, seed, k=8, joint=True, joint_discrete=False, joint_quantized=False,
                           joint_wide=False, joint_branches=False, prior_weight=_default_prior_weight,
                           n_EI_candidates=_default_n_EI_candidates, gamma=_default_gamma, device=None,
                           joint_branches_mixed=False, joint_branches_wide=False, joint_wide_mixed=False,
                           joint_wide_quantized=False):
    """The candidate pools behind the joint stages of a ``suggest([new_id],
    domain, trials, seed, joint=..., n_EI_candidates=...)`` with the same joint
    keywords: per joint group the ``k`` best distinct candidate vectors with
    their l, g and score, and statistics of the group's scores — a
    JointCandidateReport.  Entry 0 of a group is the vector that suggest joins.

    The groups are the suggest's (the same ValueErrors).  Every branch group is
    reported as if active, whether or not ``new_id`` takes the branch.  The
    per-candidate arrays never leave the device: the ranking and the statistics
    are device stages (tpe_joint_report).  One new id per call; ``k`` in
    [1, 64]."""
    k = _report_check_k(k)
    if joint is not False and joint is not None:
        _joint_plan(domain.table, joint, 'philox', 'fp32', (None, None, None, None), joint_discrete, joint_quantized,
                    _wide_mode(joint_wide, joint_wide_mixed, joint_wide_quantized),
                    _branch_mode(joint_branches, joint_branches_wide, joint_wide),
                    joint_branches_mixed)                    # (argument errors before the history is read)
    hist = _history.extract(domain, trials)
    return joint_candidate_report_columns(domain.table, hist, new_id, seed, k=k, joint=joint,
                                          joint_discrete=joint_discrete, joint_quantized=joint_quantized,
                                          joint_wide=joint_wide, joint_branches=joint_branches,
                                          joint_branches_mixed=joint_branches_mixed,
                                          joint_branches_wide=joint_branches_wide, prior_weight=prior_weight,
                                          n_EI_candidates=n_EI_candidates, gamma=gamma,
                                          device=device, joint_wide_mixed=joint_wide_mixed,
                                          joint_wide_quantized=joint_wide_quantized)


def suggest_replay(new_ids, domain, trials, seed, **kw):
    """``suggest`` in exact-parity mode: the reference's RandomState candidate
    draws and float64 scoring (trajectories identical to the reference)."""
    kw.setdefault('sampler', 'replay')
    kw.setdefault('precision', 'fp64')
    return suggest(new_ids, domain, trials, seed, **kw)
