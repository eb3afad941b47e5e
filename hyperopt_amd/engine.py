"""Device engine: packs fitted posteriors into the C-ABI tables and runs them.

One ``Engine.run`` call = one batched launch sequence (sample -> score ->
select) over every (hyperparameter, new_id) *problem* of one tree level.  All
device memory is owned here through torch tensors (torch is only the
allocator / stream provider); the kernels are libtpe_hip.so.

Device layout (HBM, all caller-owned, grow-only pools):
  problems  tpe_problem[P]            136 B each
  comp32    float4[K_total]           continuous families, f32 precision
  comp64    double4[K_total]          quantized / categorical / f64 precision
  samp      double[8][Kb_total]       below-mixture sampler rows
  cand      double[C_total]           candidate values (returned to the user)
  coord     float[C_total]            kernel coordinate (x or ln x) in f32
  part      double[sum_p splits_p*C_p] above-mixture partial sums
  tile_best tpe_best[T * BEST_PER_TILE], result tpe_result[P]
Mixtures are shared by every problem of the same hyperparameter (the history
is common to all new_ids), so component tables scale with labels, not ids.
"""
import ctypes
import math
import os

import numpy as np

from . import _native as N
from . import joint_pack as JP
from . import parzen

try:
    import torch
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None
# raw current-stream accessor of the torch build (None: go through torch.cuda.current_stream)
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None) if torch is not None else None
try:                                    # (the native trampoline of tpe_suggest_tree; optional until built)
    from ._hostaddr import call_tree as _CALL_TREE
except ImportError:                     # pragma: no cover
    _CALL_TREE = None
# the torch dtype of a row of joint_pack.ROWS
_TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64} if torch is not None else {}

# target number of above-mixture work items per launch (>= 8 per CU on 256 CUs)
TARGET_WORK = 2048
MIN_COMPONENTS_PER_SPLIT = 128
# continuous above mixtures with at least this many observations are fitted on
# the device (tpe_fit_above) in fp32 mode; TPE_DEVICE_FIT_MIN overrides
DEVICE_FIT_MIN = int(os.environ.get('TPE_DEVICE_FIT_MIN', '16384'))
PRUNE_MIN_K = 64
FINE_KEY_MIN_CAND = 65536          # tpe_host.cpp kFineKeyMinCand: 12-bit sort buckets from here
TAIL_MIN_TILES = 32                # tpe_host.cpp kTailMinTiles: per-tile tail splits from here


def _coord_range(post):
    """Value range of the kernel coordinate (x, or ln x for log families) the
    candidates of ``post`` fall in: the bounds, else the below mixture +-8 sigma."""
    if post.family == N.FAM_CATEGORICAL:
        return 0.0, float(max(post.upper, 1))
    if post.low is not None and post.high is not None:
        return float(post.low), float(post.high)
    w, mu, sg = post.below
    return float(np.min(mu - 8 * sg)), float(np.max(mu + 8 * sg))


TAB_ETA = 0.05                     # tpe_host.cpp kTabEta: a_max * h <= eta per cell
TAB_MAX_CELLS = 65536
TAB_MAX_LATTICE = 1 << 18
TAB_MIN_RATIO, TAB_MIN_RATIO_DEVFIT = 8.0, 64.0   # tpe_host.cpp kTabMinRatio*: candidates per cell row
LOGPOLY_MAX_CELLS = 2048           # tpe_host.cpp kLogpolyMaxCells (TPE_F_LOGPOLY: one grid for both sides)
LP_ROW_COST = 1.25                 # tpe_host.cpp kLpRowCost (a LOGPOLY row in cell rows)
LP_DIRECT_ROWS = 64                # tpe_host.cpp kLpDirectRows
MOM_DIRECT_ROWS = 64               # tpe_host.cpp kMomDirectRows
MOM_CELLS_PER_WAVE = 4             # tpe_host.cpp kMomCellsPerWave
LP_ROWS_PER_WAVE = 5               # tpe_host.cpp kLpRowsPerWave
A_SCALE_LIT = 0.84932180028801907  # tpe_host.cpp kAScale (the same double)


def _tab_plan(lp, n_cand, f64):
    """Tabulated scoring of one level label (tpe_host.cpp, "tabulated scoring"):
    dict(mode, n=(cells or lattice values per side), lo, hi, lat_lo)."""
    post = lp.post
    none = dict(mode=N.TAB_NONE, n=(0, 0), lo=0.0, hi=0.0, lat_lo=0)
    if os.environ.get('TPE_TABLES', '1').startswith('0') or n_cand <= 0 or len(lp.ids) == 0:
        return none
    fam = post.family
    if fam == N.FAM_CATEGORICAL or len(post.below[0]) == 0:
        return none
    klo, khi = _coord_range(post)
    if not (math.isfinite(klo) and math.isfinite(khi) and khi > klo):
        return none
    ct = float(len(lp.ids)) * float(n_cand)

    def cells(sig):
        n = math.ceil((khi - klo) * (A_SCALE_LIT / max(sig, parzen.EPS)) / (2.0 * TAB_ETA))
        return int(n) if 1.0 <= n < 1e15 else -1
    if fam in (N.FAM_GAUSS, N.FAM_LOGGAUSS) and not f64:
        s0 = float(np.min(post.below[2]))
        if post.above_dev is not None:
            n_obs, bidx = post.above_dev[1:3]
            s1 = post.prior[1] / min(100.0, 1.0 + float(n_obs - len(bidx) + 1))
        else:
            s1 = float(np.min(post.above[2]))
        n0, n1 = cells(s0), cells(s1)
        ratio = TAB_MIN_RATIO_DEVFIT if post.above_dev is not None else TAB_MIN_RATIO
        nl = max(n0, n1)
        # (a device-fitted label takes box-moment cells when TPE_FGT allows: tpe_host.cpp)
        boxes = post.above_dev is not None and not os.environ.get('TPE_FGT', '1').startswith('0')
        if (not os.environ.get('TPE_LOGPOLY', '1').startswith('0') and not boxes and n0 > 0 and n1 > 0
                and nl <= LOGPOLY_MAX_CELLS and ct >= ratio * LP_ROW_COST * nl):
            return dict(mode=N.TAB_CELLS, n=(nl, nl), lo=klo, hi=khi, lat_lo=0, logpoly=True)
        if 0 < n0 <= TAB_MAX_CELLS and 0 < n1 <= TAB_MAX_CELLS and ct >= ratio * (n0 + n1):
            return dict(mode=N.TAB_CELLS, n=(n0, n1), lo=klo, hi=khi, lat_lo=0)
    elif fam in (N.FAM_QGAUSS, N.FAM_QLOGGAUSS) and post.q and post.q > 0 and lp.inject is None:
        tlo, thi = klo, khi
        if post.low is None or post.high is None:
            w, mu, sg = post.below
            tlo, thi = float(np.min(mu - 9 * sg)), float(np.max(mu + 9 * sg))
        lg = fam == N.FAM_QLOGGAUSS
        xlo, xhi = (math.exp(tlo), math.exp(thi)) if lg else (tlo, thi)
        mlo, mhi = math.floor(xlo / post.q) - 1.0, math.ceil(xhi / post.q) + 1.0
        nl = mhi - mlo + 1.0
        if math.isfinite(nl) and 1.0 <= nl <= TAB_MAX_LATTICE and abs(mlo) < 9e15 and ct >= 2.0 * nl:
            return dict(mode=N.TAB_LATTICE, n=(int(nl), 0), lo=klo, hi=khi, lat_lo=int(mlo))
    return none


def _rows32(mu, a, c):
    """float4 {mu_hi, mu_lo, a, c} rows (mu split so t - mu keeps ~48 bits)."""
    r = np.empty((len(mu), 4), dtype=np.float32)
    hi = np.asarray(mu, dtype=np.float32)
    r[:, 0] = hi
    r[:, 1] = (np.asarray(mu, dtype=np.float64) - hi.astype(np.float64)).astype(np.float32)
    r[:, 2] = a
    r[:, 3] = c
    return r


class LevelProblem(object):
    """One hyperparameter of one tree level, active for ``ids``.

    post     parzen.Posterior
    label_ix stable label index (Philox counter word 2)
    ids      int64 array of new_ids for which this label is active
    inject   optional float64 [len(ids), n_cand] candidates (replay / tests)
    """
    __slots__ = ('post', 'label_ix', 'ids', 'inject')

    def __init__(self, post, label_ix, ids, inject=None):
        self.post, self.label_ix = post, int(label_ix)
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.inject = inject


class _TreeIO(object):
    """Engine.suggest_tree's argument and result arrays (grown, never shrunk)
    with their addresses looked up once."""

    def __init__(self, n, nl, nb, old=None):
        if old is not None:
            n, nl, nb = max(n, old.n_cap), max(nl, old.l_cap), max(nb, old.b_cap)
        self.n_cap, self.l_cap, self.b_cap = n, nl, max(nb, 64)
        self.ids = np.zeros(n, dtype=np.int64)
        self.below = np.zeros(self.b_cap, dtype=np.int64)
        self.values = np.zeros(n * nl)
        self.active = np.ones(n * nl, dtype=np.int8)
        self.need_fit = np.zeros(nl, dtype=np.int8)
        self.ids_ptr, self.below_ptr = self.ids.ctypes.data, self.below.ctypes.data
        self.values_ptr, self.active_ptr = self.values.ctypes.data, self.active.ctypes.data
        self.need_fit_ptr = self.need_fit.ctypes.data


class Engine(object):
    """Per-device engine.  ``precision`` is 'fp32' (default, performance) or
    'fp64' (parity mode: float64 continuous families)."""

    def __init__(self, device=None, precision='fp32'):
        if torch is None:
            raise N.NativeUnavailable('torch is required for device memory')
        self.lib = N.load()
        n = ctypes.c_int(0)
        if self.lib.tpe_device_count(ctypes.byref(n)) != 0 or n.value == 0 or not torch.cuda.is_available():
            raise N.NativeUnavailable('no HIP device visible: the TPE engine has no CPU fallback')
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.tile = self.lib.tpe_tile_size()
        self.device_fit_min = DEVICE_FIT_MIN
        self.tree_calls = 0              # tpe_suggest_tree calls (tests: one per steady-state suggest)
        self.set_precision(precision)
        self._bufs = {}
        self._pinned = None
        self._ws = None                   # cached tpe_level_ws (run_level)
        self._tree_out = ((ctypes.c_int32 * 2)(), N.LevelNeed())   # suggest_tree's path / need records
        # (their addresses and tpe_suggest_tree's, for the native trampoline)
        self._tree_addr = (ctypes.addressof(self._tree_out[0]), ctypes.addressof(self._tree_out[1]),
                           ctypes.cast(self.lib.tpe_suggest_tree, ctypes.c_void_p).value)
        self._tree_io = None              # suggest_tree's argument / result buffers (_TreeIO)
        # when a dict: every run() times each stage with HIP events on the
        # launch stream and appends (ms, CE of the launch) under the kernel name;
        # profile_repeat > 1 re-issues each (idempotent) stage back to back and
        # reports the mean (steady-state stage cost, tools/stage_bench.py)
        self.profile = None
        self.profile_repeat = 1
        # pruned f32 above kernel: local (Taylor) expansion of components whose
        # series converges over a wave's candidate span (False: all exact)
        self.expand = True
        # continuous f32 tiles with one split: score in the above kernel (False:
        # always in the finalize stage)
        self.fuse = True

    def _stream(self):
        """The device's current torch stream as a raw hipStream_t (the same
        handle torch.cuda.current_stream(device).cuda_stream gives, without
        building a Stream object: microseconds per suggest)."""
        raw = _RAW_STREAM
        if raw is not None:
            return raw(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_precision(self, precision):
        if precision not in ('fp32', 'fp64'):
            raise ValueError("precision must be 'fp32' or 'fp64'")
        self.precision = precision

    # ------------------------------------------------------------ buffers
    def _buf(self, name, n, dtype):
        n = max(int(n), 1)
        t = self._bufs.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            cap = max(n, int(1.25 * (t.numel() if t is not None else 0)))
            t = torch.empty(cap, dtype=dtype, device=self.device)
            self._bufs[name] = t
            self._ws = None
            self._drop_resident()
        return t

    def _drop_resident(self):
        """The engine replaced or wrote a pool itself: no level is resident
        there any more (tpe_level_resident, mode 2)."""
        self.lib.tpe_level_resident(2, None)

    # ------------------------------------------------------------- tables
    def _build_numpy(self, problems, n_cand, seed, cand_base, n_cand_global):
        """Host-side packing of one level in numpy — the specification that
        the native packer (tpe_host_pack_level) is tested against."""
        f64 = self.precision == 'fp64'
        T = self.tile
        plans = [_tab_plan(lp, n_cand, f64) for lp in problems]
        # sorted (pruned) problems: continuous f32 above mixtures of > PRUNE_MIN_K
        # components that are not tabulated
        pruned_l = [(not f64) and lp.post.family in (N.FAM_GAUSS, N.FAM_LOGGAUSS)
                    and (lp.post.above_dev is not None or len(lp.post.above[0]) > PRUNE_MIN_K)
                    and pl['mode'] == N.TAB_NONE for lp, pl in zip(problems, plans)]
        # a pruned label active for several ids is pooled: one sort slot for all its problems
        pooled_l = [pr and len(lp.ids) >= 2 for lp, pr in zip(problems, pruned_l)]
        S = sum((1 if po else len(lp.ids)) for lp, pr, po in zip(problems, pruned_l, pooled_l) if pr)
        n_sorted = sum(len(lp.ids) for lp, pr in zip(problems, pruned_l) if pr)
        max_slot = max([n_cand * (len(lp.ids) if po else 1) for lp, pr, po in zip(problems, pruned_l, pooled_l)
                        if pr], default=0)
        pbits = int(math.ceil(math.log2(S))) if S > 1 else 0
        key_bits = max(5, 8 - pbits)
        if max_slot >= FINE_KEY_MIN_CAND:
            key_bits = max(key_bits, min(12, 16 - pbits))
        comp32, comp64, samp, grids = [], [], [], []
        n32 = n64 = ns = ngrid = 0
        rows = []                         # per LevelProblem: (table info)
        for lp, pl in zip(problems, plans):
            post = lp.post
            fam = post.family
            klo, khi = _coord_range(post)
            info = dict(wide_off=0, wide_len=0, grid_off=0, grid_n=0, prior_mu=0.0, prior_a=0.0, prior_c=0.0,
                        narrow_cmax=0.0, narrow_amin=0.0, grid_lo=0.0, grid_inv=0.0, key_lo=klo,
                        key_inv=(1 << key_bits) / (khi - klo) if khi > klo else 0.0,
                        family=fam, flags=(N.F_HAS_LOW if post.low is not None else 0)
                        | (N.F_HAS_HIGH if post.high is not None else 0),
                        low=post.low if post.low is not None else 0.0,
                        high=post.high if post.high is not None else 0.0,
                        q=post.q if post.q is not None else 0.0, n_upper=post.upper)
            st = parzen.sampler_table(post)
            info['samp_off'], info['samp_len'] = ns, st.shape[0]
            if fam == N.FAM_CATEGORICAL and 0 < st.shape[0] <= 64 and len(post.above[0]) == st.shape[0]:
                # TPE_F_CAT_LAZY: best-scoring drawable category selected with p >= 2^-16
                c1, s1, p1 = -1, 0.0, 0.0
                for i in range(st.shape[0]):
                    pi = st[i, 0] - (st[i - 1, 0] if i else 0.0)
                    if not pi > 0:
                        continue
                    pa = float(post.above[0][i])
                    sc = math.log(float(post.below[0][i])) - (math.log(pa) if pa > 0 else -math.inf)
                    if c1 < 0 or ((s1 == s1) if sc != sc else sc > s1):
                        c1, s1, p1 = i, sc, pi
                if c1 >= 0 and p1 >= 1.0 / 65536:
                    info['flags'] |= N.F_CAT_LAZY
            samp.append(st)
            ns += st.shape[0]
            if fam == N.FAM_CATEGORICAL:
                for side in ('below', 'above'):
                    p = np.asarray(getattr(post, side)[0], dtype=float)
                    r = np.zeros((len(p), 4))
                    with np.errstate(divide='ignore'):
                        r[:, 0] = np.log(p)
                    r[:, 1] = p
                    info[side + '_off'], info[side + '_len'] = n64, len(p)
                    info[side + '_base'] = 0.0
                    comp64.append(r)
                    n64 += len(p)
            elif fam in (N.FAM_QGAUSS, N.FAM_QLOGGAUSS):
                for side in ('below', 'above'):
                    w, mu, sg = getattr(post, side)
                    m, b, ww, base = parzen.quant_table(w, mu, sg, post)
                    r = np.zeros((len(w), 4))
                    r[:, 0], r[:, 1], r[:, 2] = m, b, ww
                    info[side + '_off'], info[side + '_len'] = n64, len(w)
                    info[side + '_base'] = base
                    comp64.append(r)
                    n64 += len(w)
            else:
                logf = fam == N.FAM_LOGGAUSS
                for side in ('below', 'above'):
                    w, mu, sg = getattr(post, side)
                    m, a, c, base = parzen.gauss_table(w, mu, sg, post, logf)
                    info[side + '_base'] = base
                    if f64:
                        r = np.zeros((len(w), 4))
                        r[:, 0], r[:, 1], r[:, 2] = m, a, c
                        info[side + '_off'], info[side + '_len'] = n64, len(w)
                        comp64.append(r)
                        n64 += len(w)
                    else:
                        meta, wide, cn = None, None, c
                        if side == 'above' and pl['mode'] == N.TAB_NONE:     # tabulated: no pruning
                            cn, wide, meta = parzen.prune_tables(m, a, c)
                        r = _rows32(m, a, cn)
                        info[side + '_off'], info[side + '_len'] = n32, len(w)
                        comp32.append(r)
                        n32 += len(w)
                        if meta is not None:
                            comp32.append(_rows32(m[wide], a[wide], c[wide]))
                            info['wide_off'], info['wide_len'] = n32, len(wide)
                            n32 += len(wide)
                            g = meta.pop('grid')
                            info['grid_off'], info['grid_n'] = ngrid, len(g) - 1
                            grids.append(g)
                            ngrid += len(g)
                            info.update(meta)
            rows.append(info)

        # score tables: 16-B units, a cell row 3 units, a lattice row 1
        units, jobs, blocks, r0 = 0, [], 0, 0
        for lp, pl, info in zip(problems, plans, rows):
            info['tab_mode'], info['tab_off'], info['tab_n'] = pl['mode'], [0, 0], [0, 0]
            info['tab_lo'], info['tab_inv'], info['lat_lo'] = [0.0, 0.0], [0.0, 0.0], 0
            if pl['mode'] == N.TAB_CELLS and pl.get('logpoly'):
                n = pl['n'][0]                  # one table, both sides' polynomials in each row
                info['flags'] = info['flags'] | N.F_LOGPOLY
                for sd in range(2):
                    info['tab_off'][sd], info['tab_n'][sd] = units, n
                    info['tab_lo'][sd] = float(np.float32(pl['lo']))
                    info['tab_inv'][sd] = float(np.float32(n / (pl['hi'] - pl['lo'])))
                units += N.TAB_ROW_UNITS * n
            elif pl['mode'] == N.TAB_CELLS:
                for sd in range(2):
                    n = pl['n'][sd]
                    info['tab_off'][sd], info['tab_n'][sd] = units, n
                    info['tab_lo'][sd] = float(np.float32(pl['lo']))
                    info['tab_inv'][sd] = float(np.float32(n / (pl['hi'] - pl['lo'])))
                    units += N.TAB_ROW_UNITS * n
            elif pl['mode'] == N.TAB_LATTICE:
                info['tab_off'][0], info['tab_n'][0], info['lat_lo'] = units, pl['n'][0], pl['lat_lo']
                units += pl['n'][0] + (pl['n'][0] + 1 + 3) // 4      # rows, then n + 1 f32 entry thresholds
            if pl['mode'] != N.TAB_NONE and len(lp.ids):
                for sd in range(2 if pl['mode'] == N.TAB_CELLS else 1):
                    geo = (0, 0, 0, 0, 0.0, 0.0)
                    if pl['mode'] == N.TAB_CELLS:     # the side's rows and cell geometry
                        side = 'above' if sd else 'below'
                        geo = (info[side + '_off'], info[side + '_len'], info.get('wide_off', 0) if sd else 0,
                               info.get('wide_len', 0) if sd else 0, info['tab_lo'][sd], info['tab_inv'][sd])
                    kind = N.TAB_LOGPOLY if pl.get('logpoly') else pl['mode']
                    jobs.append((r0, sd, kind, info['tab_n'][sd], info['tab_off'][sd], blocks) + geo)
                    n = info['tab_n'][sd]        # cells: TAB_PER_BLOCK rows a block; lattice: a block a value
                    if kind == N.TAB_LOGPOLY and geo[1] >= 0 and geo[1] + geo[3] <= LP_DIRECT_ROWS:
                        blocks += -(-n // (LP_ROWS_PER_WAVE * N.TAB_PER_BLOCK))    # (a short side: direct sums)
                    elif kind == N.TAB_CELLS and geo[1] >= 0 and geo[1] + geo[3] <= MOM_DIRECT_ROWS:
                        blocks += -(-n // (MOM_CELLS_PER_WAVE * N.TAB_PER_BLOCK))  # (a short moment side)
                    else:
                        blocks += -(-n // N.TAB_PER_BLOCK) if pl['mode'] == N.TAB_CELLS else n
            r0 += len(lp.ids)
        tj = np.zeros(len(jobs), dtype=N.TAB_JOB_DTYPE)
        for c, f in enumerate(N.TAB_JOB_DTYPE.names):
            tj[f] = [jb[c] for jb in jobs]

        # problems: one row per (LevelProblem, id)
        counts = np.array([len(lp.ids) for lp in problems], dtype=np.int64)
        P = int(counts.sum())
        prob = np.zeros(P, dtype=N.PROBLEM_DTYPE)
        owner = np.repeat(np.arange(len(problems)), counts)
        for field in ('family', 'flags', 'n_upper', 'samp_off', 'samp_len', 'below_off', 'below_len',
                      'above_off', 'above_len', 'low', 'high', 'q', 'below_base', 'above_base',
                      'wide_off', 'wide_len', 'grid_off', 'grid_n', 'prior_mu', 'prior_a', 'prior_c',
                      'narrow_cmax', 'narrow_amin', 'grid_lo', 'grid_inv', 'key_lo', 'key_inv',
                      'tab_mode', 'tab_off', 'tab_n', 'tab_lo', 'tab_inv', 'lat_lo'):
            prob[field] = np.array([r[field] for r in rows])[owner] if P else 0
        prob['n_cand'] = n_cand
        ids = np.concatenate([lp.ids for lp in problems]) if P else np.zeros(0, np.int64)
        pr = np.repeat(np.array(pruned_l, dtype=bool), counts) if P else np.zeros(0, bool)
        # sorted problems own the candidate range [0, n_sorted * n_cand)
        srank = np.cumsum(pr) - 1
        unslot = np.cumsum(~pr) - 1
        prob['cand_off'] = np.where(pr, srank * n_cand, (n_sorted + unslot) * n_cand)
        slots, pool_first, nxt, r = [], [], 0, 0
        for lp, p_, po in zip(problems, pruned_l, pooled_l):
            k = len(lp.ids)
            if po:
                slots += [nxt] * k
                nxt += 1
            elif p_:
                slots += list(range(nxt, nxt + k))
                nxt += k
            else:
                slots += [-1] * k
            pool_first += [r if po else -1] * k
            r += k
        prob['sort_slot'] = slots if P else -1
        prob['pool_first'] = pool_first if P else -1
        pooled = np.repeat(np.array(pooled_l, dtype=bool), counts) if P else np.zeros(0, bool)
        prob['flags'] = prob['flags'] | np.where(pooled, N.F_POOLED, 0)
        prob['cand_base'] = cand_base
        prob['n_cand_global'] = n_cand if not n_cand_global else int(n_cand_global)
        s64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        prob['key0'] = s64 & 0xFFFFFFFF
        prob['key1'] = s64 >> 32
        prob['ctr2'] = np.array([lp.label_ix for lp in problems], dtype=np.uint32)[owner] if P else 0
        prob['ctr3'] = (ids & 0xFFFFFFFF).astype(np.uint32)
        n_tiles_p = (n_cand + T - 1) // T if n_cand > 0 else 0
        prob['n_tiles'] = n_tiles_p
        prob['tile_off'] = np.arange(P, dtype=np.int64) * n_tiles_p

        # splits of the above mixture per tile: bulk tiles fill the chip (a
        # function of the GLOBAL candidate count); pruned problems with many
        # tiles use one split and geometrically more on their outermost tiles
        fam = prob['family']
        untab = prob['tab_mode'] == N.TAB_NONE
        cont = ((fam == N.FAM_GAUSS) | (fam == N.FAM_LOGGAUSS)) & untab
        qg, ql = (fam == N.FAM_QGAUSS) & untab, (fam == N.FAM_QLOGGAUSS) & untab
        scored = cont | qg | ql
        C_ref = n_cand if not n_cand_global else int(n_cand_global)
        tiles_ref = (C_ref + T - 1) // T
        n_scored_tiles = int(scored.sum()) * tiles_ref
        target = max(1, math.ceil(TARGET_WORK / max(n_scored_tiles, 1)))
        K = prob['above_len'].astype(np.int64)
        tails = pr & (tiles_ref >= TAIL_MIN_TILES)
        splits = np.where(scored, np.where(tails, 1, np.clip(np.minimum(target, (K + MIN_COMPONENTS_PER_SPLIT - 1)
                                                                      // MIN_COMPONENTS_PER_SPLIT), 1, None)), 0)
        prob['n_splits'] = splits
        j = np.arange(n_tiles_p)
        e = np.minimum(j, n_tiles_p - 1 - j)
        tail_ns = np.select([e < 6, e < 8, e < 10, e < 12], [16, 8, 4, 2], 1)     # tpe_host.cpp tail_splits
        ns_tile = np.zeros((P, n_tiles_p), dtype=np.int64)
        for r in range(P):
            if not scored[r]:
                continue
            if tails[r]:
                ns_tile[r] = np.maximum(1, np.minimum(tail_ns, max(1, (K[r] + 63) // 64)))
            else:
                ns_tile[r] = splits[r]

        # tiles
        tiles = np.zeros(P * n_tiles_p, dtype=N.TILE_DTYPE)
        tiles['problem'] = np.repeat(np.arange(P), n_tiles_p)
        tiles['cand_start'] = np.tile(np.arange(n_tiles_p) * T, P)
        tiles['n_splits'] = ns_tile.reshape(-1)

        # work items, grouped [continuous | qgauss | qlog], a tile's items consecutive
        works = []
        counts_w = []
        nw = 0
        for mask in (cont, qg, ql):
            pidx = np.nonzero(mask)[0]
            rows_w = []
            for r in pidx:
                for t in range(n_tiles_p):
                    ti = r * n_tiles_p + t
                    tiles['work_first'][ti] = nw
                    ns = int(ns_tile[r, t])
                    for sp in range(ns):
                        rows_w.append((r, sp, t * T, (K[r] * sp) // ns, (K[r] * (sp + 1)) // ns, ns))
                        nw += 1
            w = np.array(rows_w, dtype=np.int64).reshape(-1, 6)
            wa = np.zeros(len(w), dtype=N.WORK_DTYPE)
            for c, f in enumerate(N.WORK_DTYPE.names):
                wa[f] = w[:, c]
            works.append(wa)
            counts_w.append(len(wa))
        work = np.concatenate(works) if works else np.zeros(0, dtype=N.WORK_DTYPE)
        part_total = nw * T

        return dict(prob=prob, tiles=tiles, work=work, counts_w=counts_w, part_total=part_total, tab_jobs=tj,
                    tab_units=units, tab_blocks=blocks,
                    comp32=np.concatenate(comp32) if comp32 else np.zeros((0, 4), np.float32),
                    comp64=np.concatenate(comp64) if comp64 else np.zeros((0, 4)),
                    grid=np.concatenate(grids) if grids else np.zeros(1, np.int32),
                    samp=np.concatenate(samp) if samp else np.zeros((0, 8)), P=P)

    # ---------------------------------------------------------------- pack
    @staticmethod
    def _labels(problems):
        """tpe_label_in array of one level (LABEL_DTYPE records; returns its
        address) plus the arrays it points into, which the caller keeps alive
        for the native call.  One tuple assignment per label."""
        n = len(problems)
        recs = np.zeros(max(n, 1), dtype=N.LABEL_DTYPE)
        keep = [recs]
        id_addr = {}                              # the level's problems usually share one ids array
        # room for every device-fitted label's merged order first: making room can
        # re-lay out the History's order buffers, which would move addresses
        # already taken (devhist)
        grow = {}
        for lp in problems:
            ad = lp.post.above_dev
            if ad is not None:
                g = grow.setdefault(id(ad[3].group), (ad[3].group, [], []))
                g[1].append(ad[3].slot)
                g[2].append(ad[1])
        for g, slots, ns in grow.values():
            g.ensure(slots, ns)
        for i, lp in enumerate(problems):
            post = lp.post
            flags = (N.F_HAS_LOW if post.low is not None else 0) | (N.F_HAS_HIGH if post.high is not None else 0)
            if lp.inject is not None:        # caller-drawn candidates need not lie on a quantization lattice
                flags |= N.F_NO_TABLE
            ids = lp.ids                          # int64, contiguous (LevelProblem)
            if post.ptrs is not None and post.above_dev is None:
                # native fits: the addresses are known; the posterior owns the arrays
                keep.append(post)
                pt = post.ptrs
                ia = id_addr.get(id(ids))
                if ia is None:
                    ia = id_addr[id(ids)] = ids.ctypes.data
                recs[i] = (post.family, flags, int(post.upper), lp.label_ix,
                           post.low if post.low is not None else 0.0, post.high if post.high is not None else 0.0,
                           post.q if post.q is not None else 0.0,
                           pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], pt[6], pt[7],
                           ia, len(ids), 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0)
                continue
            bw = [np.ascontiguousarray(a, dtype=np.float64) for a in post.below]
            ids = np.ascontiguousarray(lp.ids, dtype=np.int64)
            keep.append(bw)
            keep.append(ids)
            bptr = [a.ctypes.data for a in bw] + [0] * (3 - len(bw))
            if post.above_dev is not None:
                col, n_obs, bidx, order = post.above_dev
                bidx = np.ascontiguousarray(bidx, dtype=np.int32)
                keep.append(bidx)
                aptr, ak = [0, 0, 0], n_obs - len(bidx) + 1
                dev = (col.data_ptr(), n_obs, bidx.ctypes.data, len(bidx))
                prior = post.prior
                ordp = order.ptrs(n_obs)          # the label's resident value order (ValueOrder)
            else:
                aw = [np.ascontiguousarray(a, dtype=np.float64) for a in post.above]
                keep.append(aw)
                aptr, ak = [a.ctypes.data for a in aw] + [0] * (3 - len(aw)), len(aw[0])
                dev, prior, ordp = (0, 0, 0, 0), (0.0, 0.0, 0.0, 0), (0, 0, 0, 0, 0)
            recs[i] = (post.family, flags, int(post.upper), lp.label_ix,
                       post.low if post.low is not None else 0.0, post.high if post.high is not None else 0.0,
                       post.q if post.q is not None else 0.0,
                       bptr[0], bptr[1], bptr[2], len(bw[0]), aptr[0], aptr[1], aptr[2], ak,
                       ids.ctypes.data, len(ids), dev[0], dev[1], dev[2], dev[3], prior[3],
                       prior[0], prior[1], prior[2]) + ordp
        return recs.ctypes.data, keep

    @staticmethod
    def _commit_orders(problems):
        """A level with these problems was enqueued: the device-fitted labels'
        merged value orders are now their resident orders (stream order makes
        them valid for every later launch on the stream)."""
        for lp in problems:
            ad = lp.post.above_dev
            if ad is not None:
                ad[3].commit(ad[1])

    def _pack(self, problems, n_cand, seed, cand_base, n_cand_global):
        """Pack one level with the native host runtime straight into the pinned
        staging buffer; returns the PackInfo."""
        n = len(problems)
        labels, keep = self._labels(problems)
        info = N.PackInfo()
        prec = N.PREC_F64 if self.precision == 'fp64' else N.PREC_F32
        seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        ncg = int(n_cand_global) if n_cand_global is not None else 0
        for attempt in range(2):
            host = self._pinned
            cap = host.numel() if host is not None else 0
            rc = self.lib.tpe_host_pack_level(labels, n, int(n_cand), seed64, int(cand_base), ncg, prec,
                                              host.data_ptr() if host is not None else None, cap,
                                              ctypes.byref(info))
            if rc == N.E_SPACE:
                self._pinned = torch.empty(max(info.blob_bytes, 2 * cap), dtype=torch.uint8,
                                           pin_memory=torch.cuda.is_available())
                self._ws = None
                self._drop_resident()
                continue
            N.check(rc, self.lib, 'tpe_host_pack_level')
            break
        return info

    def _flags(self):
        # (TPE_DEBUG_FLAGS is read per call: tests switch it on around single runs)
        return (0 if self.expand else N.BATCH_NO_EXPAND) | (0 if self.fuse else N.BATCH_NO_FUSE) | \
            int(os.environ.get('TPE_DEBUG_FLAGS', '0'))

    # ----------------------------------------------------- one-call level
    def _level_ws(self):
        """tpe_level_ws over the engine's pools (rebuilt when a pool grows)."""
        ws = self._ws
        if ws is not None:
            return ws
        B = self._bufs
        ws = N.LevelWS()

        def dev(name, itemsize):
            t = B.get(name)
            return (t.data_ptr(), t.numel() * t.element_size() // itemsize) if t is not None else (None, 0)
        pin = self._pinned
        ws.pinned, ws.pinned_bytes = (pin.data_ptr(), pin.numel()) if pin is not None else (None, 0)
        if pin is not None:            # the staging buffer's device address, once per allocation
            dp = ctypes.c_void_p()
            N.check(self.lib.tpe_pinned_device_address(pin.data_ptr(), ctypes.byref(dp)), self.lib,
                    'tpe_pinned_device_address')
            ws.pinned_dev = dp.value
        ws.blob, ws.blob_bytes = dev('blob', 1)
        ws.cand, n1 = dev('cand', 8)
        ws.coord, n2 = dev('coord', 4)
        ws.keys, n3 = dev('keys', 4)
        ws.vals, n4 = dev('vals', 8)
        ws.keys_sorted, n5 = dev('keys_sorted', 4)
        ws.vals_sorted, n6 = dev('vals_sorted', 8)
        ws.cand_cap = min(n1, n2, n3, n4, n5, n6)
        ws.sort_tmp, ws.sort_tmp_bytes = dev('sort_tmp', 1)
        ws.part, ws.part_cap = dev('part', 8)
        ws.tile_best, ws.best_cap = dev('best', 32)
        ws.result, ws.result_cap = dev('result', 48)
        ws.fit_keys, f1 = dev('fit_keys', 8)
        ws.fit_keys_sorted, f2 = dev('fit_keys_sorted', 8)
        ws.fit_vals, f3 = dev('fit_vals', 4)
        ws.fit_vals_sorted, f4 = dev('fit_vals_sorted', 4)
        ws.fit_cap = min(f1, f2, f3, f4)
        ws.draw_pref, ws.draw_pref_cap = dev('draw_pref', 8)
        ws.pool_best, ws.pool_best_cap = dev('pool_best', 8)
        ws.tab, ws.tab_cap = dev('tab', 16)
        self._ws = ws
        return ws

    def _grow(self, need):
        if need.pinned_bytes > (self._pinned.numel() if self._pinned is not None else 0):
            self._pinned = torch.empty(int(need.pinned_bytes * 1.25) + 4096, dtype=torch.uint8,
                                       pin_memory=torch.cuda.is_available())
            self._drop_resident()
        self._buf('blob', need.blob_bytes, torch.uint8)
        for name, dt in (('cand', torch.float64), ('coord', torch.float32), ('keys', torch.int32),
                         ('vals', torch.int64), ('keys_sorted', torch.int32), ('vals_sorted', torch.int64)):
            self._buf(name, need.cand, dt)
        self._buf('sort_tmp', need.sort_tmp_bytes, torch.uint8)
        self._buf('part', need.part, torch.float64)
        self._buf('best', need.best * 4, torch.float64)
        self._buf('result', need.result * 6, torch.float64)
        for name, dt in (('fit_keys', torch.float64), ('fit_keys_sorted', torch.float64),
                         ('fit_vals', torch.int32), ('fit_vals_sorted', torch.int32)):
            self._buf(name, need.fit, dt)
        self._buf('draw_pref', need.draw_pref, torch.float64)
        self._buf('pool_best', need.pool_best, torch.int64)
        self._buf('tab', 4 * need.tab, torch.float32)
        self._ws = None

    def run_level(self, problems, n_cand, seed, cand_base=0, n_cand_global=None):
        """``run`` for device-drawn candidates without per-candidate outputs:
        one native call (tpe_level_run) packs, uploads, launches every stage
        and reads the per-problem results back.  Returns RESULT_DTYPE [P]."""
        n_cand = int(n_cand)
        if n_cand < 0 or n_cand >= 2 ** 31:
            raise ValueError('n_EI_candidates out of range: %r' % n_cand)
        labels, keep = self._labels(problems)
        P = sum(len(lp.ids) for lp in problems)
        out = np.empty(P, dtype=N.RESULT_DTYPE)
        need = N.LevelNeed()
        prec = N.PREC_F64 if self.precision == 'fp64' else N.PREC_F32
        seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        ncg = int(n_cand_global) if n_cand_global is not None else 0
        stream = self._stream()
        prof = self.profile is not None
        if prof:
            N.check(self.lib.tpe_level_profile(1), self.lib, 'tpe_level_profile')
        for attempt in range(3):
            ws = self._level_ws()
            rc = self.lib.tpe_level_run(labels, len(problems), n_cand, seed64, int(cand_base), ncg, prec,
                                        self._flags(), ctypes.byref(ws),
                                        ctypes.byref(need), stream, out.ctypes.data)
            if rc != N.E_SPACE:
                break
            self._grow(need)
        if prof:
            self.lib.tpe_level_profile(0)
        N.check(rc, self.lib, 'tpe_level_run')
        self._commit_orders(problems)
        del keep
        if prof and P:
            self._record_level_profile()
        return out

    def suggest_tree(self, labels, below_sorted, prior_weight, lf, ids, n_cand, seed, min_draws, flags=0,
                     shard=None, exchange=None, labels_ptr=None):
        """A whole tpe.suggest of a tree space in one native call
        (tpe_suggest_tree): fits, gate prediction and level runs.  ``labels``:
        TREE_LABEL_DTYPE records in label order (``labels_ptr``: their address,
        when the caller keeps it); ``below_sorted``: int64 ascending below
        tids; ``shard`` = (rank, world) with ``exchange`` (a dist._Exchange):
        this rank scores its range of the ``n_cand`` candidates and the native
        call exchanges every level's results.
        Returns (values, active) [n_ids x n_labels] — views of the engine's
        result buffers, valid until its next suggest_tree — or (None,
        need_fit) on TPE_E_FALLBACK: need_fit [n_labels] flags the labels the
        caller must fit and pass back (none: take the general path)."""
        if self.precision != 'fp32':
            return None, np.zeros(len(labels), dtype=np.int8)
        self.tree_calls += 1
        n_cand = int(n_cand)
        if n_cand < 0 or n_cand >= 2 ** 31:
            raise ValueError('n_EI_candidates out of range: %r' % n_cand)
        nl, n, nb = len(labels), len(ids), len(below_sorted)
        io = self._tree_io
        if io is None or io.n_cap < n or io.l_cap < nl or io.b_cap < nb:
            io = self._tree_io = _TreeIO(n, nl, nb, io)
        # arguments into the persistent buffers (their addresses are cached:
        # an ndarray's .ctypes costs microseconds per access)
        io.ids[:n] = ids
        io.below[:nb] = below_sorted
        io.need_fit[:nl] = 0
        if labels_ptr is None:
            labels_ptr = labels.ctypes.data
        path, need = self._tree_out
        seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        stream = self._stream()
        prof = self.profile is not None
        if prof:
            N.check(self.lib.tpe_level_profile(1), self.lib, 'tpe_level_profile')
        c_loc, base, c_glob, ex = n_cand, 0, 0, None
        if shard is not None:
            from .dist import shard_range
            base, hi = shard_range(n_cand, shard[0], shard[1])
            c_loc, c_glob = hi - base, n_cand
            ex = exchange.ptr(nl * n, c_loc)
        # an unsharded call through the trampoline (it ORs in TPE_DEBUG_FLAGS);
        # a sharded one through ctypes (the exchange struct is a ctypes object)
        tramp = _CALL_TREE is not None and ex is None
        fl = ((0 if self.expand else N.BATCH_NO_EXPAND) | (0 if self.fuse else N.BATCH_NO_FUSE) | int(flags)) \
            if tramp else self._flags() | int(flags)
        for attempt in range(8):          # a later tree level may need larger pools than the first
            ws = self._level_ws()
            if tramp:
                a_path, a_need, fn = self._tree_addr
                rc = _CALL_TREE(fn, labels_ptr, nl, io.below_ptr, nb, float(prior_weight), int(lf), io.ids_ptr, n,
                                c_loc, base, c_glob, 0, seed64, float(min_draws), int(self.device_fit_min), fl,
                                ctypes.addressof(ws), a_need, stream or 0, io.values_ptr, io.active_ptr, a_path,
                                io.need_fit_ptr)
            else:
                rc = self.lib.tpe_suggest_tree(labels_ptr, nl, io.below_ptr, nb, float(prior_weight), int(lf),
                                               io.ids_ptr, n, c_loc, base, c_glob, ex, seed64, float(min_draws),
                                               int(self.device_fit_min), fl, ctypes.byref(ws), ctypes.byref(need),
                                               stream, io.values_ptr, io.active_ptr, path, io.need_fit_ptr)
            if rc != N.E_SPACE:
                break
            self._grow(need)
        if prof:
            self.lib.tpe_level_profile(0)
        if rc == N.E_FALLBACK:
            return None, io.need_fit[:nl].copy()
        N.check(rc, self.lib, 'tpe_suggest_tree')
        self.last_tree_path = (int(path[0]), int(path[1]))
        if prof and path[1]:
            self._record_level_profile()
        return io.values[:n * nl].reshape(n, nl), io.active[:n * nl].reshape(n, nl)

    def _record_level_profile(self):
        """profile[stage] gets (ms, units, algorithmic CE) of every stage the
        last tpe_level_run launched, timed by the runner's own HIP events on
        its stream (tpe_level_profile): the production flow, stage by stage."""
        recs = (N.StageProf * len(N.STAGES))()
        N.check(self.lib.tpe_level_profile_read(recs, len(N.STAGES)), self.lib, 'tpe_level_profile_read')
        for name, r in zip(N.STAGES, recs):
            if r.launches:
                self.profile.setdefault(name, []).append((float(r.ms), float(r.units), float(r.ce),
                                                          1e-6 * float(r.kernel_ns)))

    # ---------------------------------------------------------------- run
    def run(self, problems, n_cand, seed, cand_base=0, want_lg=False, return_cand=False, n_cand_global=None,
            report_k=0):
        """Sample, score and select every problem of one level.

        Returns a RESULT_DTYPE array with one row per (LevelProblem, id) in
        order, plus (cand, l, g) float64 [P, n_cand] arrays when requested.

        ``report_k`` > 0 (at most N.REPORT_MAX_K): the candidate report of the
        level (tpe_report, include/tpe_hip.h "Candidate report") runs on the
        same stream after the stages and (top, n_top, stats) is appended to
        the return value, in problem order: top TOP_ENTRY_DTYPE [P, report_k]
        — the report_k best distinct candidate values of each problem with
        their l, g and global index, n_top [P] of them valid — and stats
        SCORE_STATS_DTYPE [P].  The per-candidate arrays stay on the device
        unless want_lg / return_cand ask for them.  A level with a pooled
        label (a pruned label active for several ids) is refused."""
        n_cand = int(n_cand)
        if n_cand < 0 or n_cand >= 2 ** 31:
            raise ValueError('n_EI_candidates out of range: %r' % n_cand)
        report_k = int(report_k)
        if report_k < 0 or report_k > N.REPORT_MAX_K:
            raise ValueError('report_k must be in [0, %d]: %r' % (N.REPORT_MAX_K, report_k))
        info = self._pack(problems, n_cand, seed, cand_base, n_cand_global)
        self._last_info = info
        P = int(info.n_problems)
        if report_k and info.n_pooled:
            # (tpe_report cannot see the problem flags: the check is here)
            raise ValueError('candidate report of a level with a pooled label (one label, several ids, pruned '
                             'above mixture): report its ids one per run')
        if P == 0:
            res = np.zeros(0, dtype=N.RESULT_DTYPE)
            if not report_k:
                return res
            return (res, np.zeros((0, report_k), dtype=N.TOP_ENTRY_DTYPE), np.zeros(0, dtype=np.int32),
                    np.zeros(0, dtype=N.SCORE_STATS_DTYPE))
        C_total = P * n_cand
        if C_total >= 2 ** 32:
            raise ValueError('more than 2^32 candidates in one level: shard the batch')
        nbytes = int(info.blob_bytes)
        dev = self._buf('blob', nbytes, torch.uint8)
        # host-written ranges only: device-fitted rows are produced by tpe_fit_above
        self._drop_resident()             # (the blob is rewritten here, outside a library call)
        for i in range(int(info.n_up)):
            o, n = int(info.up_off[i]), int(info.up_len[i])
            dev[o:o + n].copy_(self._pinned[o:o + n], non_blocking=True)
        base = dev.data_ptr()
        prob = np.frombuffer(self._pinned.numpy(), dtype=N.PROBLEM_DTYPE, count=P, offset=int(info.off_problems))
        d_cand = self._buf('cand', C_total, torch.float64)
        d_coord = self._buf('coord', C_total, torch.float32)
        d_part = self._buf('part', info.part_total, torch.float64)
        n_tiles = int(info.n_tiles)
        d_best = self._buf('best', n_tiles * N.BEST_PER_TILE * 4, torch.float64)
        d_res = self._buf('result', P * 6, torch.float64)
        d_keys = self._buf('keys', C_total, torch.int32)
        d_vals = self._buf('vals', C_total, torch.int64)
        # sort only when some problem of the level prunes its above mixture
        sort = info.sort_end_bit > 0
        if sort:
            d_keys_s = self._buf('keys_sorted', C_total, torch.int32)
            d_vals_s = self._buf('vals_sorted', C_total, torch.int64)
            ws = ctypes.c_uint64(0)
            N.check(self.lib.tpe_sort_workspace_bytes(int(info.sort_count), ctypes.byref(ws)), self.lib,
                    'tpe_sort_workspace_bytes')
            d_sort = self._buf('sort_tmp', ws.value, torch.uint8)
        else:
            d_keys_s, d_vals_s, d_sort = d_keys, d_vals, None
        inject = any(lp.inject is not None for lp in problems)
        if inject:
            if not all(lp.inject is not None for lp in problems):
                raise ValueError('either every problem of a level injects candidates or none does')
            cand = np.concatenate([np.asarray(lp.inject, dtype=np.float64).reshape(len(lp.ids), n_cand)
                                   for lp in problems]).reshape(-1)
            fam = np.repeat(prob['family'], n_cand)
            with np.errstate(divide='ignore', invalid='ignore'):
                coord = np.where((fam == N.FAM_LOGGAUSS) | (fam == N.FAM_QLOGGAUSS), np.log(cand), cand)
            cat = fam == N.FAM_CATEGORICAL
            if cat.any():
                upper = np.repeat(prob['n_upper'], n_cand)[cat]
                cv = cand[cat]
                if np.any((cv < 0) | (cv >= upper) | (cv != np.floor(cv))):
                    raise IndexError('categorical candidate out of range')
            # problem r's candidates live at cand_off[r] (sorted problems first)
            at = (prob['cand_off'][:, None] + np.arange(n_cand)[None, :]).reshape(-1)
            placed, placed_t = np.empty(C_total), np.empty(C_total, dtype=np.float32)
            placed[at] = cand
            placed_t[at] = coord.astype(np.float32)
            d_cand[:C_total].copy_(torch.from_numpy(placed))
            d_coord[:C_total].copy_(torch.from_numpy(placed_t))
        d_l = d_g = None
        if want_lg or report_k:
            d_l = self._buf('l_out', C_total, torch.float64)
            d_g = self._buf('g_out', C_total, torch.float64)
        b = N.Batch()
        b.problems, b.n_problems = base + info.off_problems, P
        b.precision = N.PREC_F64 if self.precision == 'fp64' else N.PREC_F32
        b.flags = self._flags() | (N.BATCH_WRITE_CAND if (return_cand or want_lg or report_k) else 0)
        b.sample = 0 if inject else 1
        b.sort_end_bit, b.key_bits = info.sort_end_bit, info.key_bits
        b.comp32, b.comp64 = base + info.off_comp32, base + info.off_comp64
        b.samp, b.grid = base + info.off_samp, base + info.off_grid
        b.keys, b.vals = d_keys.data_ptr(), d_vals.data_ptr()
        b.keys_sorted, b.vals_sorted = d_keys_s.data_ptr(), d_vals_s.data_ptr()
        if d_sort is not None:
            b.sort_tmp, b.sort_tmp_bytes = d_sort.data_ptr(), d_sort.numel()
        b.total_cand = C_total
        b.sort_count = info.sort_count
        b.cand, b.coord = d_cand.data_ptr(), d_coord.data_ptr()
        b.tiles, b.n_tiles = base + info.off_tiles, n_tiles
        b.fin_tiles, b.n_fin_tiles = base + info.off_fin_tiles, info.n_fin_tiles
        b.work = base + info.off_work
        b.n_work_cont, b.n_work_qgauss, b.n_work_qlog = info.n_work_cont, info.n_work_qgauss, info.n_work_qlog
        b.part = d_part.data_ptr()
        b.l_out = d_l.data_ptr() if d_l is not None else None
        b.g_out = d_g.data_ptr() if d_g is not None else None
        b.tile_best, b.result = d_best.data_ptr(), d_res.data_ptr()
        if info.n_pooled:
            b.pool_best = self._buf('pool_best', P, torch.int64).data_ptr()
        b.samp_tiles, b.n_samp_tiles, b.n_samp_eager = base + info.off_samp_tiles, info.n_samp_tiles, info.n_samp_eager
        b.tab_tiles, b.n_tab_tiles = base + info.off_tab_tiles, info.n_tab_tiles
        if info.n_tab_jobs:
            b.tab_jobs, b.n_tab_jobs, b.tab_blocks = base + info.off_tab_jobs, info.n_tab_jobs, info.tab_blocks
            b.tab = self._buf('tab', 4 * int(info.tab_units), torch.float32).data_ptr()
            b.tab_units = info.tab_units
            b.fgt_max_boxes = info.fgt_max_boxes
            b.fgt_max_cells = info.fgt_max_cells
        if info.n_sorted and not inject and not info.n_pooled:
            b.n_sorted, b.draw_blocks = info.n_sorted, info.draw_blocks
            b.draw_pref = self._buf('draw_pref', int(info.n_sorted) * (int(info.draw_blocks) + 1),
                                    torch.float64).data_ptr()
        if info.n_fit:
            ft = int(info.fit_total)
            d_fk = self._buf('fit_keys', ft, torch.float64)
            d_fks = self._buf('fit_keys_sorted', ft, torch.float64)
            d_fv = self._buf('fit_vals', ft, torch.int32)
            d_fvs = self._buf('fit_vals_sorted', ft, torch.int32)
            b.fit, b.n_fit = base + info.off_fit, info.n_fit
            b.below_idx, b.fit_seg, b.fit_total = base + info.off_below_idx, base + info.off_fit_seg, ft
            b.fit_keys, b.fit_keys_sorted = d_fk.data_ptr(), d_fks.data_ptr()
            b.fit_vals, b.fit_vals_sorted = d_fv.data_ptr(), d_fvs.data_ptr()
            b.fit_max_new, b.fit_max_obs, b.fit_max_merge = info.fit_max_new, info.fit_max_obs, info.fit_max_merge
            b.fit_n_delta = info.fit_n_delta
        stream = self._stream()
        if self.profile is None:
            N.check(self.lib.tpe_run_batch(ctypes.byref(b), ctypes.c_void_p(stream)), self.lib, 'tpe_run_batch')
        else:
            tb = dict(prob=prob.copy(), counts_w=[info.n_work_cont, info.n_work_qgauss, info.n_work_qlog], P=P)
            self._run_profiled(b, stream, tb, n_cand)
        if report_k:
            rep = self._report(b, P, C_total, report_k, stream)
        self._commit_orders(problems)
        res = d_res[:P * 6].cpu().numpy().view(N.RESULT_DTYPE).copy()
        if not (want_lg or return_cand or report_k):
            return res
        out = [res]
        rows = (prob['cand_off'] // max(n_cand, 1)).astype(np.int64)    # sorted problems come first

        def per_problem(d):
            return d[:C_total].cpu().numpy().reshape(P, n_cand)[rows].copy()
        if return_cand:
            out.append(per_problem(d_cand))
        if want_lg:
            out.append(per_problem(d_l))
            out.append(per_problem(d_g))
        if report_k:
            # (the report's records are per problem row: the caller's order already)
            d_top, d_ntop, d_stats = rep
            out.append(d_top[:P * report_k * 4].cpu().numpy().view(N.TOP_ENTRY_DTYPE).reshape(P, report_k).copy())
            out.append(d_ntop[:P].cpu().numpy().copy())
            out.append(d_stats[:P * 8].cpu().numpy().view(N.SCORE_STATS_DTYPE).copy())
        return tuple(out)

    def _report(self, b, P, C_total, k, stream):
        """Enqueue tpe_report for the batch ``b`` just run; returns the device
        tensors (top, n_top, stats)."""
        nb = ctypes.c_uint64(0)
        N.check(self.lib.tpe_report_scratch_bytes(N.report_chunks(P, C_total), k, ctypes.byref(nb)), self.lib,
                'tpe_report_scratch_bytes')
        d_scr = self._buf('report_scratch', (nb.value + 7) // 8, torch.float64)
        d_top = self._buf('report_top', P * k * 4, torch.float64)
        d_ntop = self._buf('report_n_top', P, torch.int32)
        d_stats = self._buf('report_stats', P * 8, torch.float64)
        N.check(self.lib.tpe_report(ctypes.byref(b), k, d_top.data_ptr(), d_ntop.data_ptr(), d_stats.data_ptr(),
                                    d_scr.data_ptr(), d_scr.numel() * 8, ctypes.c_void_p(stream)), self.lib,
                'tpe_report')
        return d_top, d_ntop, d_stats

    def run_joint(self, below, above, low, high, ids, n_cand, seed, inject=None, return_cand=False, want_lg=False,
                  report_k=0, shard=None, stream_word=None, liar=False, given=None, return_sigma=False):
        """One joint TPE stage (tpe_joint_run, include/tpe_hip.h "Joint
        (multivariate) TPE stage"): ``below`` / ``above`` = (w [K], mu [K, D],
        sigma [K, D]) float64 mixtures (joint.side_mixture), ``low`` / ``high``
        [D] the bounds (+-inf: unbounded).  The rows are packed in float64 on
        the host, uploaded and scored; per new id the winner record
        (N.JOINT_RECORD_DTYPE) comes back.  ``inject`` [C, D]: score these
        candidates (every id) instead of sampling.  ``return_cand``: also the
        candidates f32 [n_ids, C, D]; ``want_lg``: also l, g float64 [n_ids, C].
        ``report_k`` > 0 (every run_joint* method): the stage leaves its
        candidates, l and g on the device, tpe_joint_report (include/tpe_hip.h
        "Joint candidate report") runs on the same stream, and the call also
        returns, after everything else, top [P, k] (N.JOINT_TOP_ENTRY_DTYPE),
        top_z f32 [P, k, D] (run_joint_segments: a list of P arrays [k, D_p]),
        n_top int32 [P] and stats [P] (N.SCORE_STATS_DTYPE), P the ids or
        problems; the per-candidate arrays come to the host only with
        ``return_cand`` / ``want_lg``.
        ``shard`` = (cand_base, n_cand_global) (every run_joint* method,
        tpe_joint_run_shard, include/tpe_hip.h "Sharded joint stage"): the call
        scores the ``n_cand`` candidates [cand_base, cand_base + n_cand) of a
        stage of n_cand_global < 2^31 candidates.  The per-candidate arrays are
        the local ones, a record's global_idx is global, and
        joint.combine_records over the parts of a partition gives the unsharded
        records.  ``n_cand`` may then be 0 (a rank whose range is empty): empty
        records (joint.empty_records) and no native call.  ``report_k`` > 0 or
        ``inject`` with a non-zero cand_base raise ValueError.
        ``stream_word`` (every solo run_joint* method): the Philox stream word
        (None: N.JOINT_STREAM; a branch group's joint.branch_stream_word, to
        compare with run_joint_segments).
        ``liar`` (run_joint and run_joint_wide; DESIGN.md "Batch-aware joint
        suggests", the model in joint.py): the ids pick greedily in the order
        given.  The stage keeps its three buffers on the device and
        tpe_joint_liar follows on the same stream; record j then holds pick j's
        index, l, g_j (the above density extended by the ``given`` vectors
        [G, D] and the picks before it, each counted as one more bad trial) and
        z.  ``want_lg`` still returns the base l and g.  True takes the above
        side's un-normalised weight sum W as 1 / w[-1] (the newest trial weighs
        1; a side without trials: 1), a float is W itself
        (joint.side_weight_sum).  ``return_sigma``: also, last, the liars'
        bandwidths float64 [G + n_ids, D].  ``liar`` with ``shard`` or
        ``report_k`` > 0, and ``given`` or ``return_sigma`` without ``liar``,
        raise ValueError."""
        return self._joint_continuous(False, below, above, low, high, ids, n_cand, seed, inject, return_cand, want_lg,
                                      stream_word, report_k, shard, self._liar(liar, given, return_sigma, report_k,
                                                                               shard))

    def run_joint_wide(self, below, above, low, high, ids, n_cand, seed, inject=None, return_cand=False,
                       want_lg=False, report_k=0, shard=None, stream_word=None, liar=False, given=None,
                       return_sigma=False):
        """``run_joint`` for up to N.JOINT_WIDE_MAX_DIMS dimensions
        (tpe_joint_wide_run, include/tpe_hip.h "Wide joint stage"): the same
        arguments, model, Philox streams and return shapes; the records are
        N.JOINT_WIDE_RECORD_DTYPE."""
        return self._joint_continuous(True, below, above, low, high, ids, n_cand, seed, inject, return_cand, want_lg,
                                      stream_word, report_k, shard, self._liar(liar, given, return_sigma, report_k,
                                                                               shard))

    @staticmethod
    def _liar(liar, given, return_sigma, report_k, shard):
        """The ``liar`` / ``given`` / ``return_sigma`` arguments of run_joint as
        one dict (None: no liar stage); their ValueErrors.  Touches no device."""
        if liar is False or liar is None:
            if given is not None or return_sigma:
                raise ValueError('joint stage: given and return_sigma need liar')
            return None
        if shard is not None:
            raise ValueError('joint stage: liar does not combine with shard')
        if int(report_k) > 0:
            raise ValueError('joint stage: liar does not combine with report_k')
        W = None
        if not isinstance(liar, (bool, np.bool_)):
            W = float(liar)
            if not (W > 0 and np.isfinite(W)):
                raise ValueError('joint stage: liar must be True or the positive weight sum W: %r' % (liar,))
        return {'W': W, 'given': given, 'sigma': bool(return_sigma)}

    def _joint_continuous(self, wide, below, above, low, high, ids, n_cand, seed, inject, return_cand, want_lg,
                          stream_word=None, report_k=0, shard=None, liar=None):
        """``run_joint`` (``wide``: ``run_joint_wide``) with the arguments in
        the order this entry has always had; callers that reach past the two
        public methods keep working."""
        return self._joint_solo('wide' if wide else 'run', below, above, low, high, (), (), ids, n_cand, seed, inject,
                                return_cand, want_lg, report_k, stream_word, shard, liar=liar)

    # the solo stages by joint_pack entry: the args struct and the native function
    _JOINT_SOLO = {'run': (N.JointArgs, 'tpe_joint_run'), 'wide': (N.JointWideArgs, 'tpe_joint_wide_run'),
                   'mixed': (N.JointMixedArgs, 'tpe_joint_mixed_run'),
                   'wide_mixed': (N.JointWideMixedArgs, 'tpe_joint_wide_mixed_run'),
                   'quant': (N.JointQuantArgs, 'tpe_joint_quant_run'),
                   'wide_quant': (N.JointWideQuantArgs, 'tpe_joint_wide_quant_run')}

    def _joint_solo(self, entry, below, above, low, high, cats, quants, ids, n_cand, seed, inject, return_cand,
                    want_lg, report_k, stream_word, shard, return_table=False, liar=None):
        """What the six solo stages share: the group's rows (joint_pack.group_rows,
        which also checks the group; an empty part of a sharded stage is checked
        too), one upload per row, the args struct filled from the same rows
        record, the call and its results.  The library derives the f32 bounds
        from the float64 ``low`` / ``high`` in the struct; a quantised label's
        lattice ends follow the continuous bounds there."""
        r = JP.group_rows(below, above, low, high, cats, quants, entry=entry)
        Dc, Dk, Dq = r['Dc'], r['Dk'], r['Dq']
        D, wide = Dc + Dk + Dq, entry in ('wide', 'wide_mixed', 'wide_quant')
        ids, n_ids, C = self._joint_sizes(D, ids, n_cand, shard)
        shard = self._joint_shard(shard, C, report_k, inject)
        if liar is not None:
            liar = (self._liar_mixed_model(liar, above, r, cats, quants) if liar.get('mixed')
                    else self._liar_model(liar, entry, above, r, D))
        if C == 0:
            if return_table:
                raise ValueError('joint stage: return_table needs at least one candidate')
            return self._joint_empty(n_ids, D, return_cand, want_lg, wide)
        up = self._joint_up
        struct, fn = self._JOINT_SOLO[entry]
        a = struct()
        a.n_dims, a.n_cand, a.n_ids, a.flags = Dc, C, n_ids, 0
        a.k_below, a.k_above = r['k_below'], r['k_above']
        a.below_base, a.above_base = r['below_base'], r['above_base']
        a.stream_word = N.JOINT_STREAM if stream_word is None else int(stream_word)
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for key, field, buf, dtype, part in JP.group_rows_present(r):
            # tpe_joint_quant_run takes null pointers for the rows of an absent continuous part
            if not (entry == 'quant' and part == 'cont' and Dc == 0):
                setattr(a, field, up(buf, r[key], _TORCH_OF[dtype]))
        a.ids = up('ids', ids, torch.int64)
        if inject is not None:
            a.flags |= N.JOINT_INJECT
            a.inject = up('inject', JP.inject_rows(inject, C, D), torch.float32)
        for d in range(Dc):
            a.low[d], a.high[d] = r['low'][d], r['high'][d]
        if Dk:
            a.n_cat = Dk
            for d in range(Dk):
                a.cat_upper[d], a.cat_off[d] = r['cat_upper'][d], r['cat_off'][d]
        if Dq:
            a.n_quant, a.n_edges = Dq, len(r['quant_edges'])
            for d in range(Dq):
                a.low[Dc + d], a.high[Dc + d] = r['qlow'][d], r['qhigh'][d]
                a.quant_v[d], a.quant_edge_off[d] = r['quant_v'][d], r['quant_edge_off'][d]
            total = r['n_lattice']
            nb = ctypes.c_uint64(0)
            N.check(self.lib.tpe_joint_quant_table_bytes(a.k_below, a.k_above, total, ctypes.byref(nb)), self.lib,
                    'tpe_joint_quant_table_bytes')
            d_tab = self._buf('joint_qtable', (nb.value + 3) // 4, torch.float32)
            a.quant_table, a.quant_table_bytes = d_tab.data_ptr(), d_tab.numel() * 4
        out = self._joint_call(fn, a, n_ids, C, D, return_cand, want_lg, wide=wide, report_k=report_k, shard=shard,
                               n_cat=Dk if wide else 0, liar=liar, n_quant=Dq if wide else 0)
        if not return_table:
            return out
        tab = d_tab[:(a.k_below + a.k_above) * total].cpu().numpy()
        tb = tab[:total * a.k_below].reshape(total, a.k_below).T.copy()
        ta = tab[total * a.k_below:].reshape(total, a.k_above).T.copy()
        return (out if isinstance(out, tuple) else (out,)) + (tb, ta)

    @staticmethod
    def _liar_model(liar, entry, above, r, D):
        """``liar`` (Engine._liar) completed from the group: W, the prior sigmas,
        the bounds and the given vectors as f32 [G, D]."""
        if entry not in ('run', 'wide'):
            raise ValueError('joint stage: liar needs a group of continuous labels')
        w, sigma = np.asarray(above[0], dtype=np.float64), np.asarray(above[2], dtype=np.float64).reshape(-1, D)
        W = liar['W']
        if W is None:
            W = 1.0 / float(w[-1]) if len(w) > 1 else 1.0
        given = np.zeros((0, D), dtype=np.float32)
        if liar['given'] is not None:
            given = np.ascontiguousarray(liar['given'], dtype=np.float32)
            if given.ndim != 2 or given.shape[1] != D:
                raise ValueError('joint stage: given must be [G, %d]: %r' % (D, given.shape))
        return {'W': W, 'given': given, 'sigma': liar['sigma'], 'psig': sigma[0], 'low': r['low'], 'high': r['high']}

    def run_joint_liar_mixed(self, below, above, low, high, cats, quants, ids, n_cand, seed, liar=True, given=None,
                             return_sigma=False, centres=None, inject=None, return_cand=False, want_lg=False,
                             report_k=0, shard=None, stream_word=None):
        """A batch-aware joint stage over a group with discrete and / or
        quantised labels (DESIGN.md "Batch-aware picks over discrete and
        quantised labels"): the stage ``run_joint_quant`` (``quants`` not
        empty), ``run_joint_wide_mixed`` (more than N.JOINT_MAX_DIMS
        coordinates) or ``run_joint_mixed`` would run over the same group, its
        three buffers kept on the device, then tpe_joint_liar_mixed on the same
        stream.  ``below`` .. ``cats``, ``ids`` .. ``seed``, ``inject``,
        ``return_cand``, ``want_lg`` and ``stream_word`` are those methods';
        ``quants`` as run_joint_quant (() without quantised labels).  ``liar``,
        ``given`` and ``return_sigma`` mean what they mean on ``run_joint``:
        ``given`` is [G, D] in kernel coordinates (continuous, categories,
        lattice indices), the categories and lattice indices integral values in
        range, else ValueError; the bandwidths come back as float64 [G + n_ids,
        Dc + Dq], the continuous dimensions, then the quantised ones.
        ``centres``: per quantised dimension the float64 [V] fit coordinates of
        its lattice values (QuantModel.centres()), required with quantised
        labels.  ``shard`` and ``report_k`` > 0 raise as on ``run_joint``.  The
        three stage methods themselves keep their signatures (tests pin them):
        the liar keywords live here."""
        lm = self._liar(liar, given, return_sigma, report_k, shard)
        if lm is None:
            raise ValueError('joint stage: run_joint_liar_mixed needs liar (True or the weight sum W)')
        lm['mixed'], lm['centres'] = True, centres
        D = len(np.asarray(low).reshape(-1)) + len(cats) + len(quants)
        entry = 'quant' if len(quants) else ('wide_mixed' if D > N.JOINT_MAX_DIMS else 'mixed')
        return self._joint_solo(entry, below, above, low, high, cats, quants, ids, n_cand, seed, inject, return_cand,
                                want_lg, 0, stream_word, None, liar=lm)

    @staticmethod
    def _liar_mixed_model(liar, above, r, cats, quants):
        """``liar`` (run_joint_liar_mixed) completed from a group with discrete or
        quantised labels (joint.py "Batch-aware picks over discrete and quantised
        labels"): W, the prior sigmas of the continuous and the quantised
        dimensions, the bounds, the float64 liar tables of the discrete
        dimensions from the above side's smoothing masses, the centre table, and
        the given rows as f32 [G, D] (categories and lattice indices integral
        and in range, else ValueError)."""
        from . import joint as J
        Dc, Dk, Dq = r['Dc'], r['Dk'], r['Dq']
        D = Dc + Dk + Dq
        w = np.asarray(above[0], dtype=np.float64)
        sigma = np.asarray(above[2], dtype=np.float64).reshape(len(w), Dc)
        W = liar['W']
        if W is None:
            W = 1.0 / float(w[-1]) if len(w) > 1 else 1.0
        ups, vs = list(r.get('cat_upper', ())), list(r.get('quant_v', ()))
        tabs = [J.liar_cat_tables(c[2], c[4]) for c in cats]
        centre = np.zeros(0)
        if Dq:
            cs = liar.get('centres')
            if cs is None or len(cs) != Dq:
                raise ValueError('joint stage: liar with quantised labels needs centres, one array per quantised '
                                 'dimension (joint.quant_centres)')
            cs = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in cs]
            if any(len(c) != V or not np.isfinite(c).all() for c, V in zip(cs, vs)):
                raise ValueError('joint stage: centres must hold one finite value per lattice value')
            centre = np.concatenate(cs)
        elif liar.get('centres'):
            raise ValueError('joint stage: centres without a quantised dimension')
        given = np.zeros((0, D), dtype=np.float32)
        if liar['given'] is not None:
            g64 = np.asarray(liar['given'], dtype=np.float64)
            if g64.ndim != 2 or g64.shape[1] != D:
                raise ValueError('joint stage: given must be [G, %d]: %r' % (D, g64.shape))
            for d, top in enumerate(ups + vs):
                col = g64[:, Dc + d]
                if not ((col == np.rint(col)) & (col >= 0) & (col < top)).all():
                    raise ValueError('joint stage: given holds a %s that is not an integer in [0, %d)'
                                     % ('category' if d < Dk else 'lattice index', top))
            given = np.ascontiguousarray(g64, dtype=np.float32)
        psig = np.concatenate([sigma[0], np.asarray(r['above_qsigma'], dtype=np.float64)[0] if Dq else np.zeros(0)])
        return {'mixed': True, 'W': W, 'given': given, 'sigma': liar['sigma'], 'psig': psig, 'low': r['low'],
                'high': r['high'], 'n_sigma': Dc + Dq,
                'miss': np.concatenate([t[0] for t in tabs]) if tabs else np.zeros(0),
                'bonus': np.concatenate([t[1] for t in tabs]) if tabs else np.zeros(0), 'centre': centre}

    def _joint_sizes(self, D, ids, n_cand, shard=None):
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        n_ids, C = len(ids), int(n_cand)
        if C < (1 if shard is None else 0) or C >= 2 ** 31 or n_ids < 1:   # (an empty part of a sharded stage: C = 0)
            raise ValueError('joint stage: n_cand / ids out of range')
        if n_ids * C * max(D, 2) >= 2 ** 31:
            raise ValueError('joint stage: %d ids x %d candidates do not fit one run' % (n_ids, C))
        return ids, n_ids, C

    @staticmethod
    def _joint_shard(shard, C, report_k=0, inject=None):
        """The N.JointShard of a ``shard`` = (cand_base, n_cand_global) argument
        over ``C`` local candidates (None: no shard); ValueError for a range
        outside [0, n_cand_global), n_cand_global >= 2^31, and a report or
        injected candidates at a non-zero base."""
        if shard is None:
            return None
        try:
            base, total = shard
            base, total = int(base), int(total)
        except (TypeError, ValueError):
            raise ValueError('joint stage: shard must be (cand_base, n_cand_global): %r' % (shard,))
        if base < 0 or total >= 2 ** 31 or base + int(C) > total:
            raise ValueError('joint stage: shard (%d, %d) with %d candidates: need 0 <= cand_base, cand_base + n_cand '
                             '<= n_cand_global < 2^31' % (base, total, int(C)))
        if base != 0 and int(report_k) > 0:
            raise ValueError('joint stage: report_k does not combine with a shard at a non-zero cand_base')
        if base != 0 and inject is not None:
            raise ValueError('joint stage: inject does not combine with a shard at a non-zero cand_base')
        sh = N.JointShard()
        sh.cand_base, sh.n_cand_global = base, total
        return sh

    @staticmethod
    def _joint_empty(P, D, return_cand, want_lg, wide=False, widths=None):
        """What a run_joint* call returns for an empty part of a sharded stage
        (n_cand = 0): joint.empty_records and per-candidate arrays of length 0
        (``widths``: the segmented stages' list of [0, D_p])."""
        from . import joint as J
        rec = J.empty_records(P, N.JOINT_WIDE_RECORD_DTYPE if wide else N.JOINT_RECORD_DTYPE)
        if not (return_cand or want_lg):
            return rec
        out = [rec]
        if return_cand:
            out.append(np.zeros((P, 0, D), dtype=np.float32) if widths is None
                       else [np.zeros((0, int(w)), dtype=np.float32) for w in widths])
        if want_lg:
            out.extend([np.zeros((P, 0)), np.zeros((P, 0))])
        return tuple(out)

    def _joint_native(self, fn, a, shard, *rest):
        """The stage entry point ``fn``, or tpe_joint_run_shard over the same
        arguments where ``shard`` (N.JointShard) is given."""
        if shard is None:
            N.check(getattr(self.lib, fn)(ctypes.byref(a), *rest), self.lib, fn)
        else:
            N.check(self.lib.tpe_joint_run_shard(N.JOINT_STAGES[fn], ctypes.byref(a), ctypes.byref(shard), *rest),
                    self.lib, 'tpe_joint_run_shard')

    def _joint_up(self, name, arr, dtype):
        t = self._buf('joint_' + name, arr.size, dtype)
        t[:arr.size].copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)))
        return t.data_ptr()

    def _joint_call(self, fn, a, n_ids, C, D, return_cand, want_lg, wide=False, report_k=0, shard=None, n_cat=0,
                    liar=None, n_quant=0):
        """Scratch and result buffers, the native call ``fn`` and the records
        (and candidates [n_ids, C, D], l, g [n_ids, C]) on the host.  ``wide``:
        the wide stage's scratch size and record (``n_cat`` > 0: the wide mixed
        stage's, ``n_cat`` of the D coordinates discrete; ``n_quant`` > 0: the
        wide quantised stage's, ``n_quant`` of them quantised).  ``report_k``: the stage
        writes all three device buffers and the joint report follows.
        ``shard`` (N.JointShard): the call goes through tpe_joint_run_shard.
        ``liar`` (Engine._liar_model): the stage writes all three device buffers,
        tpe_joint_liar follows, and the records hold its picks."""
        report_k = self._report_k(report_k)
        keep = report_k > 0 or liar is not None
        dev_cand, dev_lg = return_cand or keep, want_lg or keep
        nb = ctypes.c_uint64(0)
        rec_dtype = N.JOINT_WIDE_RECORD_DTYPE if wide else N.JOINT_RECORD_DTYPE
        if wide and n_quant:
            N.check(self.lib.tpe_joint_wide_quant_scratch_bytes(n_ids, C, D - n_cat - n_quant, n_cat, n_quant,
                                                                ctypes.byref(nb)), self.lib,
                    'tpe_joint_wide_quant_scratch_bytes')
        elif wide and n_cat:
            N.check(self.lib.tpe_joint_wide_mixed_scratch_bytes(n_ids, C, D - n_cat, n_cat, ctypes.byref(nb)), self.lib,
                    'tpe_joint_wide_mixed_scratch_bytes')
        elif wide:
            N.check(self.lib.tpe_joint_wide_scratch_bytes(n_ids, C, D, ctypes.byref(nb)), self.lib,
                    'tpe_joint_wide_scratch_bytes')
        else:
            N.check(self.lib.tpe_joint_scratch_bytes(n_ids, C, ctypes.byref(nb)), self.lib, 'tpe_joint_scratch_bytes')
        d_scr = self._buf('joint_scratch', (nb.value + 7) // 8, torch.float64)
        d_rec = self._buf('joint_records', n_ids * rec_dtype.itemsize // 8, torch.float64)
        d_cand = self._buf('joint_cand', n_ids * C * D, torch.float32) if dev_cand else None
        d_l = self._buf('joint_l', n_ids * C, torch.float64) if dev_lg else None
        d_g = self._buf('joint_g', n_ids * C, torch.float64) if dev_lg else None
        stream = self._stream()
        self._joint_native(fn, a, shard, d_rec.data_ptr(), d_cand.data_ptr() if dev_cand else None,
                           d_l.data_ptr() if dev_lg else None, d_g.data_ptr() if dev_lg else None,
                           d_scr.data_ptr(), d_scr.numel() * 8, ctypes.c_void_p(stream))
        if report_k:
            rep = self._joint_report(d_cand.data_ptr(), d_l.data_ptr(), d_g.data_ptr(), n_ids, C, report_k, stream,
                                     width=D)
        if liar is not None:
            lr = self._joint_liar(a, liar, d_cand.data_ptr(), d_l.data_ptr(), d_g.data_ptr(), n_ids, C, D, stream)
        rec = d_rec[:n_ids * rec_dtype.itemsize // 8].cpu().numpy().view(rec_dtype).copy()
        if liar is not None:
            d_picks, d_z, d_sig, G = lr
            picks = d_picks[:n_ids * 3].cpu().numpy().view(N.JOINT_PICK_DTYPE)
            rec['global_idx'], rec['l'], rec['g'] = picks['idx'], picks['l'], picks['g']
            rec['z'][:, :D] = d_z[:n_ids * D].cpu().numpy().reshape(n_ids, D)
        if not (return_cand or want_lg or report_k or (liar is not None and liar['sigma'])):
            return rec
        out = [rec]
        if return_cand:
            out.append(d_cand[:n_ids * C * D].cpu().numpy().reshape(n_ids, C, D).copy())
        if want_lg:
            out.append(d_l[:n_ids * C].cpu().numpy().reshape(n_ids, C).copy())
            out.append(d_g[:n_ids * C].cpu().numpy().reshape(n_ids, C).copy())
        if report_k:
            out.extend(self._joint_report_host(rep, n_ids, report_k, D))
        if liar is not None and liar['sigma']:
            ns = liar.get('n_sigma', D)
            out.append(d_sig[:(G + n_ids) * ns].cpu().numpy().reshape(G + n_ids, ns).copy())
        return tuple(out)

    def _joint_liar(self, a, liar, cand, l, g, n_ids, C, D, stream):
        """Enqueue tpe_joint_liar_mixed (a continuous group: the library runs
        tpe_joint_liar on the shared prefix) over the device buffers the joint
        stage ``a`` just wrote (the lattice edges and the above side's rows are
        the stage's own uploads); returns the device tensors (picks, pick_z,
        liar_sigma) and the number of given liars."""
        given = liar['given']
        G, Dc, Dk, Dq = len(given), a.n_dims, getattr(a, 'n_cat', 0), getattr(a, 'n_quant', 0)
        la = N.JointLiarMixedArgs()
        la.n_dims, la.n_cand, la.n_ids, la.n_given = Dc, C, n_ids, G
        la.k_above, la.n_trials, la.w_sum = a.k_above, a.k_above - 1, liar['W']
        la.cand, la.l_out, la.g_out = cand, l, g
        if Dc:
            la.above_mu = a.above_mu
        if G:
            la.given = self._joint_up('liar_given', given, torch.float32)
        for d in range(Dc):
            la.psig[d], la.low[d], la.high[d] = liar['psig'][d], liar['low'][d], liar['high'][d]
        la.n_cat, la.n_quant = Dk, Dq
        if Dk:
            for d in range(Dk):
                la.cat_upper[d], la.cat_off[d] = a.cat_upper[d], a.cat_off[d]
            la.cat_miss = self._joint_up('liar_miss', liar['miss'], torch.float64)
            la.cat_bonus = self._joint_up('liar_bonus', liar['bonus'], torch.float64)
        n_lattice = 0
        if Dq:
            for d in range(Dq):
                la.psig[Dc + d], la.low[Dc + d], la.high[Dc + d] = liar['psig'][Dc + d], a.low[Dc + d], a.high[Dc + d]
                la.quant_v[d], la.quant_edge_off[d] = a.quant_v[d], a.quant_edge_off[d]
                n_lattice += a.quant_v[d]
            la.n_edges, la.quant_edges, la.above_qmu = a.n_edges, a.quant_edges, a.above_qmu
            la.quant_centre = self._joint_up('liar_centre', liar['centre'], torch.float64)
        nb = ctypes.c_uint64(0)
        N.check(self.lib.tpe_joint_liar_mixed_scratch_bytes(n_ids, C, Dc, Dk, Dq, n_lattice, G, ctypes.byref(nb)),
                self.lib, 'tpe_joint_liar_mixed_scratch_bytes')
        ns = Dc + Dq
        d_scr = self._buf('joint_liar_scratch', (nb.value + 7) // 8, torch.float64)
        d_picks = self._buf('joint_liar_picks', n_ids * 3, torch.float64)
        d_z = self._buf('joint_liar_z', n_ids * D, torch.float32)
        d_sig = self._buf('joint_liar_sigma', max(1, (G + n_ids) * ns), torch.float64)
        N.check(self.lib.tpe_joint_liar_mixed(ctypes.byref(la), d_picks.data_ptr(), d_z.data_ptr(), d_sig.data_ptr(),
                                              d_scr.data_ptr(), d_scr.numel() * 8, ctypes.c_void_p(stream)), self.lib,
                'tpe_joint_liar_mixed')
        return d_picks, d_z, d_sig, G

    @staticmethod
    def _report_k(report_k):
        report_k = int(report_k)
        if report_k < 0 or report_k > N.REPORT_MAX_K:
            raise ValueError('joint stage: report_k must be in [0, %d]: %r' % (N.REPORT_MAX_K, report_k))
        return report_k

    def _joint_report(self, cand, l, g, P, C, k, stream, width=0, cand_off=None, widths=None):
        """Enqueue tpe_joint_report over the device buffers a joint stage just
        wrote (``widths``: the host int32 [P] row widths of a segmented stage,
        with ``cand_off`` its device offsets); returns the device tensors (top,
        top_z, n_top, stats) and the row stride of top_z."""
        a = N.JointReportArgs()
        zs = int(width if widths is None else widths.max())
        a.n_probs, a.n_cand, a.width, a.z_stride = P, C, int(width), zs
        a.cand, a.l_out, a.g_out = cand, l, g
        if widths is not None:
            widths = np.ascontiguousarray(widths, dtype=np.int32)
            a.cand_off, a.widths, a.host_widths = cand_off, self._joint_up('report_widths', widths, torch.int32), \
                widths.ctypes.data
        nb = ctypes.c_uint64(0)
        N.check(self.lib.tpe_joint_report_scratch_bytes(P, C, k, ctypes.byref(nb)), self.lib,
                'tpe_joint_report_scratch_bytes')
        d_scr = self._buf('joint_report_scratch', (nb.value + 7) // 8, torch.float64)
        d_top = self._buf('joint_report_top', P * k * 4, torch.float64)
        d_z = self._buf('joint_report_z', P * k * zs, torch.float32)
        d_ntop = self._buf('joint_report_n_top', P, torch.int32)
        d_stats = self._buf('joint_report_stats', P * 8, torch.float64)
        N.check(self.lib.tpe_joint_report(ctypes.byref(a), k, d_top.data_ptr(), d_z.data_ptr(), d_ntop.data_ptr(),
                                          d_stats.data_ptr(), d_scr.data_ptr(), d_scr.numel() * 8,
                                          ctypes.c_void_p(stream)), self.lib, 'tpe_joint_report')
        return d_top, d_z, d_ntop, d_stats, zs

    @staticmethod
    def _joint_report_host(rep, P, k, width):
        """(top [P, k], top_z, n_top [P], stats [P]) on the host; ``width`` an
        int (top_z [P, k, width]) or the per-problem widths (a list of [k, w])."""
        d_top, d_z, d_ntop, d_stats, zs = rep
        top = d_top[:P * k * 4].cpu().numpy().view(N.JOINT_TOP_ENTRY_DTYPE).reshape(P, k).copy()
        z = d_z[:P * k * zs].cpu().numpy().reshape(P, k, zs)
        z = z.copy() if np.isscalar(width) else [z[p, :, :int(w)].copy() for p, w in enumerate(width)]
        return (top, z, d_ntop[:P].cpu().numpy().copy(),
                d_stats[:P * 8].cpu().numpy().view(N.SCORE_STATS_DTYPE).copy())

    def run_joint_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, inject=None,
                           return_cand=False, want_lg=False, report_k=0, shard=None):
        """One segmented joint stage (tpe_joint_seg_run, include/tpe_hip.h
        "Segmented joint stage"): problem p scores new id ``prob_id[p]`` under
        group ``prob_seg[p]``.  ``models``: per group a joint.JointModel or a
        (below, above, low, high) tuple as ``run_joint`` takes them (1 to
        N.JOINT_MAX_DIMS continuous dimensions); ``stream_words``: per group its
        Philox stream word.  Every group's rows go into two pools, uploaded with
        the descriptors and the problem list in ONE transfer; one transfer
        brings the results back.  Problem p's results are byte for byte those
        of ``run_joint`` over its group with that stream word and ids =
        [prob_id[p]].  ``inject``: per group an array [C, D_group] (or None for
        a group without a problem): its problems score these candidates.
        Returns the records [P] (N.JOINT_RECORD_DTYPE); with ``return_cand``
        also a list of P arrays f32 [C, D_group]; with ``want_lg`` also l, g
        float64 [P, C].

        A group may also be a joint.MixedModel / joint.QuantModel, or a tuple
        (below, above, low, high, cats) / (below, above, low, high, cats,
        quants) as ``run_joint_mixed`` / ``run_joint_quant`` take them.  With
        such a group among them all groups, continuous ones included, go to
        tpe_joint_mseg_run (include/tpe_hip.h "Mixed segmented joint stage"):
        still one upload, one call and one download, and problem p's results
        are those of the solo run of its group's kind; D_group counts the
        continuous, discrete and quantised coordinates, in that order.  With
        continuous groups only nothing changes: tpe_joint_seg_run, the same blob."""
        # the choice of stage: continuous groups only keep tpe_joint_seg_run and its smaller descriptors
        mixed = any(JP.seg_parts(m)[4] or JP.seg_parts(m)[5] for m in models)
        C = int(n_cand)
        report_k = self._report_k(report_k)
        shard = self._joint_shard(shard, C, report_k, inject)
        b = JP.segment_blob(models, stream_words, prob_seg, prob_id, C, inject,
                            N.JOINT_MSEG_DTYPE if mixed else N.JOINT_SEG_DTYPE, empty_ok=shard is not None)
        P = len(b.prob_seg)
        if C == 0:                                   # an empty part of a sharded stage
            return self._joint_empty(P, 0, return_cand, want_lg, widths=b.widths)
        a = self._joint_seg_args(N.JointMSegArgs if mixed else N.JointSegArgs, b, len(models), C, seed, inject)
        if mixed:
            nb = ctypes.c_uint64(0)
            N.check(self.lib.tpe_joint_mseg_table_bytes(b.segs.ctypes.data, len(models), ctypes.byref(nb)), self.lib,
                    'tpe_joint_mseg_table_bytes')
            assert nb.value == 4 * b.n_table, (nb.value, b.n_table)
            if b.n_table:
                d_tab = self._buf('joint_mseg_table', b.n_table, torch.float32)
                a.quant_table, a.quant_table_bytes = d_tab.data_ptr(), d_tab.numel() * 4
        return self._joint_seg_call('tpe_joint_mseg' if mixed else 'tpe_joint_seg', a, P, C, b.cand_off, b.widths,
                                    return_cand, want_lg, report_k, shard)

    def run_joint_wide_segments(self, models, stream_words, prob_seg, prob_id, n_cand, seed, inject=None,
                                return_cand=False, want_lg=False, report_k=0):
        """``run_joint_segments`` for continuous groups of up to
        N.JOINT_WIDE_MAX_DIMS dimensions (tpe_joint_wide_seg_run,
        include/tpe_hip.h "Wide segmented joint stage"): the same arguments, one
        upload, one call and one download.  Problem p's results are byte for
        byte those of ``run_joint_wide`` over its group with that stream word
        and ids = [prob_id[p]].  Returns the records [P]
        (N.JOINT_WIDE_RECORD_DTYPE); with ``return_cand`` also a list of P
        arrays f32 [C, D_group]; with ``want_lg`` also l, g float64 [P, C]; with
        ``report_k`` also the joint report, as ``run_joint_segments``."""
        C = int(n_cand)
        report_k = self._report_k(report_k)
        b = JP.segment_blob(models, stream_words, prob_seg, prob_id, C, inject, N.JOINT_WIDE_SEG_DTYPE)
        a = self._joint_seg_args(N.JointWideSegArgs, b, len(models), C, seed, inject)
        return self._joint_seg_call('tpe_joint_wide_seg', a, len(b.prob_seg), C, b.cand_off, b.widths, return_cand,
                                    want_lg, report_k, rec_dtype=N.JOINT_WIDE_RECORD_DTYPE)

    def _joint_seg_args(self, struct, b, n_segs, C, seed, inject):
        """Upload the blob ``b`` (joint_pack.segment_blob) and fill the args
        ``struct`` of a segmented stage from it."""
        d_blob = self._buf('joint_seg_blob', len(b.blob), torch.uint8)
        d_blob[:len(b.blob)].copy_(torch.from_numpy(b.blob))
        a = struct()
        a.n_segs, a.n_probs, a.n_cand, a.flags = n_segs, len(b.prob_seg), C, N.JOINT_INJECT if inject is not None else 0
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for name, off in zip(JP.SECTIONS, b.offs):
            setattr(a, name, d_blob.data_ptr() + int(off))
        a.host_segs, a.host_prob_seg = b.segs.ctypes.data, b.prob_seg.ctypes.data
        a.pool_f32_len, a.pool_f64_len = b.n32, b.n64
        return a

    def _joint_seg_call(self, fn, a, P, C, cand_off, pd, return_cand, want_lg, report_k, shard=None,
                        rec_dtype=N.JOINT_RECORD_DTYPE):
        """What the segmented stages share: scratch and the result block, the
        native call ``fn``_run, the report, and one transfer of the results."""
        dev_cand, dev_lg = return_cand or report_k > 0, want_lg or report_k > 0
        nb = ctypes.c_uint64(0)
        N.check(getattr(self.lib, fn + '_scratch_bytes')(P, C, ctypes.byref(nb)), self.lib, fn + '_scratch_bytes')
        d_scr = self._buf('joint_scratch', (nb.value + 7) // 8, torch.float64)
        # one result block of 8-byte words: records, l, g, then the candidates (f32 pairs)
        rec_w = P * rec_dtype.itemsize // 8
        lg_w = P * C if dev_lg else 0
        cand_w = (int(cand_off[-1]) + 1) // 2 if dev_cand else 0
        d_out = self._buf('joint_seg_out', rec_w + 2 * lg_w + cand_w, torch.float64)
        out = d_out.data_ptr()
        stream = self._stream()
        self._joint_native(fn + '_run', a, shard, out, out + 8 * (rec_w + 2 * lg_w) if dev_cand else None,
                           out + 8 * rec_w if dev_lg else None, out + 8 * (rec_w + lg_w) if dev_lg else None,
                           d_scr.data_ptr(), d_scr.numel() * 8, ctypes.c_void_p(stream))
        if report_k:
            rep = self._joint_report(out + 8 * (rec_w + 2 * lg_w), out + 8 * rec_w, out + 8 * (rec_w + lg_w), P, C,
                                     report_k, stream, cand_off=a.cand_off, widths=pd)
        # one transfer of what the caller asked for (the report's buffers stay on the device)
        if not report_k or (want_lg and return_cand):
            host = d_out[:rec_w + 2 * lg_w + cand_w].cpu().numpy()
        else:
            hi = rec_w + (2 * lg_w if want_lg else 0)
            host = np.empty(rec_w + 2 * lg_w + cand_w)
            host[:hi] = d_out[:hi].cpu().numpy()
            if return_cand:
                host[rec_w + 2 * lg_w:] = d_out[rec_w + 2 * lg_w:rec_w + 2 * lg_w + cand_w].cpu().numpy()
        rec = host[:rec_w].view(rec_dtype).copy()
        if not (return_cand or want_lg or report_k):
            return rec
        res = [rec]
        if return_cand:
            flat = host[rec_w + 2 * lg_w:].view(np.float32)
            res.append([flat[cand_off[p]:cand_off[p + 1]].reshape(C, int(pd[p])).copy() for p in range(P)])
        if want_lg:
            res.append(host[rec_w:rec_w + lg_w].reshape(P, C).copy())
            res.append(host[rec_w + lg_w:rec_w + 2 * lg_w].reshape(P, C).copy())
        if report_k:
            res.extend(self._joint_report_host(rep, P, report_k, pd))
        return tuple(res)

    def run_joint_segments_liar(self, models, stream_words, prob_seg, prob_id, n_cand, seed, liar=True, inject=None,
                                return_cand=False, want_lg=False, return_sigma=False):
        """``run_joint_segments`` over continuous groups, batch-aware inside every
        group (tpe_joint_liar_seg, include/tpe_hip.h "Batch-aware picks in
        branch groups"; DESIGN.md of the same name): the problems of group s, in
        the order given, pick greedily as the ids of ``run_joint(..., liar=W_s)``
        do; groups do not see each other.  The segmented stage keeps its three
        buffers on the device, the liar stage follows on the same stream, and
        one transfer brings the results back.  Record p (N.JOINT_RECORD_DTYPE,
        the caller's problem order) holds its pick's index, l, g_j and row.
        The picks, rows and bandwidths of group s are byte for byte those of
        ``run_joint`` over that group with its stream word, ids = its problems'
        ids, ``liar=W_s`` and ``return_sigma=True``.

        ``liar``: True (W_s = 1 / w[-1] of each group's above side, as
        ``run_joint``) or one positive finite W_s per group.  ``return_cand`` /
        ``want_lg``: as ``run_joint_segments``, the base stage's bytes.
        ``return_sigma``: also, last, a list of float64 [L_s, D_s] per group in
        the caller's group order (a group without a problem: [0, D_s]).  A group
        with a discrete or quantised label raises ValueError."""
        for s, m in enumerate(models):
            parts = JP.seg_parts(m)
            if parts[4] or parts[5]:
                raise ValueError('joint stage: the segmented liar stage takes groups of continuous labels only: group '
                                 '%d holds a discrete or quantised label' % s)
        W = JP.liar_weight_sums(liar, models)
        C = int(n_cand)
        b = JP.segment_blob(models, stream_words, prob_seg, prob_id, C, inject, N.JOINT_SEG_DTYPE)
        lb = JP.liar_segment_blob(models, b.segs, W, b.prob_seg)
        P, S = len(b.prob_seg), len(models)
        a = self._joint_seg_args(N.JointSegArgs, b, S, C, seed, inject)
        d_lblob = self._buf('joint_liar_seg_blob', len(lb.blob), torch.uint8)
        d_lblob[:len(lb.blob)].copy_(torch.from_numpy(lb.blob))
        la = N.JointLiarSegArgs()
        la.n_segs, la.n_probs, la.n_cand = S, P, C
        for name, off in zip(JP.LIAR_SECTIONS, lb.offs):
            setattr(la, name, d_lblob.data_ptr() + int(off))
        la.host_segs, la.host_order, la.host_chain = lb.segs.ctypes.data, lb.order.ctypes.data, lb.chain.ctypes.data
        la.host_log_norm, la.host_prob_seg = lb.log_norm.ctypes.data, b.prob_seg.ctypes.data
        la.cand_off, la.pool_f32, la.pool_f32_len = a.cand_off, a.pool_f32, b.n32
        return self._joint_seg_liar_call('seg', a, la, b, lb, C, return_cand, want_lg, return_sigma)

    def _joint_seg_liar_call(self, fn, a, la, b, lb, C, return_cand, want_lg, return_sigma):
        """What the two segmented liar stages share: scratch, the result block,
        the stage ``fn``_run (``a``) with its three buffers kept, the liar
        stage tpe_joint_liar_``fn``'s suffix (``la``) on the same stream, one
        transfer, and the results on the host.  ``b`` / ``lb``: the two blobs."""
        stage, liar = 'tpe_joint_' + fn, 'tpe_joint_liar_' + fn
        P, S = len(b.prob_seg), len(lb.segs)
        nb, lnb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        N.check(getattr(self.lib, stage + '_scratch_bytes')(P, C, ctypes.byref(nb)), self.lib, stage + '_scratch_bytes')
        N.check(getattr(self.lib, liar + '_scratch_bytes')(lb.segs.ctypes.data, S, C, ctypes.byref(lnb)), self.lib,
                liar + '_scratch_bytes')
        d_scr = self._buf('joint_scratch', (nb.value + 7) // 8, torch.float64)
        d_lscr = self._buf('joint_liar_scratch', (lnb.value + 7) // 8, torch.float64)
        # one result block of 8-byte words: picks, pick rows (f32 pairs), bandwidths; then what only the device
        # or a caller of return_cand / want_lg reads: records, l, g, candidates (f32 pairs)
        MD = N.JOINT_MAX_DIMS
        pk_w, z_w, sg_w = 3 * P, P * MD // 2, max(1, lb.n_sigma)
        head = pk_w + z_w + sg_w
        rec_w, lg_w, cand_w = P * N.JOINT_RECORD_DTYPE.itemsize // 8, P * C, (int(b.cand_off[-1]) + 1) // 2
        d_out = self._buf('joint_seg_liar_out', head + rec_w + 2 * lg_w + cand_w, torch.float64)
        out = d_out.data_ptr()
        o_l, o_g, o_cand = out + 8 * (head + rec_w), out + 8 * (head + rec_w + lg_w), out + 8 * (head + rec_w + 2 * lg_w)
        la.cand, la.l_out, la.g_out = o_cand, o_l, o_g
        stream = self._stream()
        N.check(getattr(self.lib, stage + '_run')(ctypes.byref(a), out + 8 * head, o_cand, o_l, o_g, d_scr.data_ptr(),
                                                  d_scr.numel() * 8, ctypes.c_void_p(stream)), self.lib, stage + '_run')
        N.check(getattr(self.lib, liar)(ctypes.byref(la), out, out + 8 * pk_w, out + 8 * (pk_w + z_w),
                                        d_lscr.data_ptr(), d_lscr.numel() * 8, ctypes.c_void_p(stream)), self.lib, liar)
        host = d_out[:head + ((rec_w + 2 * lg_w + cand_w) if (return_cand or want_lg) else 0)].cpu().numpy()
        picks = host[:pk_w].view(N.JOINT_PICK_DTYPE)
        z = host[pk_w:pk_w + z_w].view(np.float32).reshape(P, MD)
        rec = np.zeros(P, dtype=N.JOINT_RECORD_DTYPE)
        rec['global_idx'], rec['l'], rec['g'] = picks['idx'], picks['l'], picks['g']
        for p in range(P):
            rec['z'][p, :int(b.widths[p])] = z[p, :int(b.widths[p])]
        if not (return_cand or want_lg or return_sigma):
            return rec
        res = [rec]
        if return_cand:
            flat = host[head + rec_w + 2 * lg_w:].view(np.float32)
            res.append([flat[b.cand_off[p]:b.cand_off[p + 1]].reshape(C, int(b.widths[p])).copy() for p in range(P)])
        if want_lg:
            res.append(host[head + rec_w:head + rec_w + lg_w].reshape(P, C).copy())
            res.append(host[head + rec_w + lg_w:head + rec_w + 2 * lg_w].reshape(P, C).copy())
        if return_sigma:                                 # a row: the continuous dimensions, then the quantised ones
            sig = host[pk_w + z_w:head]
            quant = 'n_quant' in lb.segs.dtype.names
            rows = []
            for g in lb.segs:
                L, w = int(g['chain_len']), int(g['n_dims']) + (int(g['n_quant']) if quant else 0)
                rows.append(sig[int(g['sigma_off']):int(g['sigma_off']) + L * w].reshape(L, w).copy())
            res.append(rows)
        return tuple(res)

    def run_joint_msegments_liar(self, models, stream_words, prob_seg, prob_id, n_cand, seed, liar=True, centres=None,
                                 inject=None, return_cand=False, want_lg=False, return_sigma=False):
        """``run_joint_segments_liar`` where a group may also hold discrete or
        quantised labels (tpe_joint_mseg_run, then tpe_joint_liar_mseg on the
        same stream, include/tpe_hip.h "Batch-aware picks in mixed branch
        groups"; DESIGN.md of the same name).  ``models`` as
        ``run_joint_segments`` takes them.  The picks, rows and bandwidths of
        group s are byte for byte those of ``run_joint_liar_mixed`` (a
        continuous group: ``run_joint``) over that group with its stream word,
        ids = its problems' ids, ``liar=W_s``, its centres and
        ``return_sigma=True``.

        ``centres``: per group None or one float64 [V_d] array per quantised
        dimension (QuantModel.centres()); a group with a quantised label needs
        them.  ``return_sigma`` rows are [L_s, Dc_s + Dq_s]: the continuous
        dimensions, then the quantised ones.  The other arguments and the
        return shapes are ``run_joint_segments_liar``'s; with no discrete or
        quantised group among ``models`` the call IS that method."""
        if not any(JP.seg_parts(m)[4] or JP.seg_parts(m)[5] for m in models):
            if centres is not None and any(c for c in centres):
                raise ValueError('joint stage: centres without a quantised dimension')
            return self.run_joint_segments_liar(models, stream_words, prob_seg, prob_id, n_cand, seed, liar=liar,
                                                inject=inject, return_cand=return_cand, want_lg=want_lg,
                                                return_sigma=return_sigma)
        W = JP.liar_weight_sums(liar, models)
        C = int(n_cand)
        b = JP.segment_blob(models, stream_words, prob_seg, prob_id, C, inject, N.JOINT_MSEG_DTYPE)
        lb = JP.liar_msegment_blob(models, b.segs, W, b.prob_seg, centres)
        P, S = len(b.prob_seg), len(models)
        a = self._joint_seg_args(N.JointMSegArgs, b, S, C, seed, inject)
        nb = ctypes.c_uint64(0)
        N.check(self.lib.tpe_joint_mseg_table_bytes(b.segs.ctypes.data, S, ctypes.byref(nb)), self.lib,
                'tpe_joint_mseg_table_bytes')
        assert nb.value == 4 * b.n_table, (nb.value, b.n_table)
        if b.n_table:
            d_tab = self._buf('joint_mseg_table', b.n_table, torch.float32)
            a.quant_table, a.quant_table_bytes = d_tab.data_ptr(), d_tab.numel() * 4
        d_lblob = self._buf('joint_liar_seg_blob', len(lb.blob), torch.uint8)
        d_lblob[:len(lb.blob)].copy_(torch.from_numpy(lb.blob))
        la = N.JointLiarMSegArgs()
        la.n_segs, la.n_probs, la.n_cand = S, P, C
        for name, off in zip(JP.LIAR_MSECTIONS, lb.offs):
            setattr(la, name, d_lblob.data_ptr() + int(off))
        la.liar_pool_len = lb.n_pool
        la.host_segs, la.host_order, la.host_chain = lb.segs.ctypes.data, lb.order.ctypes.data, lb.chain.ctypes.data
        la.host_log_norm, la.host_prob_seg = lb.log_norm.ctypes.data, b.prob_seg.ctypes.data
        la.cand_off, la.pool_f32, la.pool_f32_len = a.cand_off, a.pool_f32, b.n32
        la.pool_f64, la.pool_f64_len = a.pool_f64, b.n64
        return self._joint_seg_liar_call('mseg', a, la, b, lb, C, return_cand, want_lg, return_sigma)

    def run_joint_mixed(self, below, above, low, high, cats, ids, n_cand, seed, inject=None, return_cand=False,
                        want_lg=False, report_k=0, stream_word=None, shard=None):
        """One joint stage over a mixed group (tpe_joint_mixed_run,
        include/tpe_hip.h "Mixed joint stage"): ``below`` / ``above`` = (w [K],
        mu [K, Dc], sigma [K, Dc]) the continuous part as in ``run_joint`` (Dc
        may be 0), ``cats`` one (x_below [K_below], x_above [K_above], p [U],
        s_below, s_above) per discrete dimension: the components' categories
        (-1: the prior row), the prior and the two smoothing masses.  Kernel
        coordinates: the Dc continuous ones, then the categories as indices;
        ``inject`` [C, Dc + Dk], candidates f32 [n_ids, C, Dc + Dk].
        ``stream_word``: the Philox stream word (None: N.JOINT_STREAM; a branch
        group's joint.branch_stream_word, to compare with run_joint_segments)."""
        return self._joint_solo('mixed', below, above, low, high, cats, (), ids, n_cand, seed, inject, return_cand,
                                want_lg, report_k, stream_word, shard)

    def run_joint_wide_mixed(self, below, above, low, high, cats, ids, n_cand, seed, inject=None, return_cand=False,
                             want_lg=False, report_k=0, stream_word=None):
        """``run_joint_mixed`` for a group of up to N.JOINT_WIDE_MAX_DIMS
        coordinates of which 1 to N.JOINT_WIDE_MAX_CAT are discrete and at least
        one is continuous (tpe_joint_wide_mixed_run, include/tpe_hip.h "Wide
        mixed joint stage"): the same arguments, model, kernel coordinate order,
        Philox streams and return shapes; the records are
        N.JOINT_WIDE_RECORD_DTYPE.  The continuous coordinates are those of
        ``run_joint_wide`` over the continuous part, and a group of at most
        N.JOINT_MAX_DIMS coordinates draws ``run_joint_mixed``'s candidates.  The
        stage is not sharded: there is no ``shard`` argument."""
        return self._joint_solo('wide_mixed', below, above, low, high, cats, (), ids, n_cand, seed, inject,
                                return_cand, want_lg, report_k, stream_word, None)

    def run_joint_quant(self, below, above, low, high, cats, quants, ids, n_cand, seed, inject=None, return_cand=False,
                        want_lg=False, return_table=False, report_k=0, stream_word=None, shard=None):
        """One joint stage over a group with quantised labels
        (tpe_joint_quant_run, include/tpe_hip.h "Quantised joint stage"):
        ``below`` / ``above``, ``low`` / ``high`` and ``cats`` the continuous and
        discrete parts as in ``run_joint_mixed`` (Dc and Dk may be 0), ``quants``
        one (mu_below [K_below], sigma_below, mu_above [K_above], sigma_above,
        edges [V + 1]) per quantised dimension: its components in the fit
        coordinate and its lattice edges (joint.quant_lattice).  Kernel
        coordinates: the Dc continuous ones, the Dk categories, then the Dq
        lattice indices; ``inject`` [C, Dc + Dk + Dq], candidates f32 [n_ids, C,
        Dc + Dk + Dq].  ``return_table`` (debug): also the two sides' tables
        log2 P as the device built them, f32 [K, sum V] each.  ``stream_word``: as
        in ``run_joint_mixed``."""
        return self._joint_solo('quant', below, above, low, high, cats, quants, ids, n_cand, seed, inject, return_cand,
                                want_lg, report_k, stream_word, shard, return_table)

    def run_joint_wide_quant(self, below, above, low, high, cats, quants, ids, n_cand, seed, inject=None,
                             return_cand=False, want_lg=False, return_table=False, report_k=0, stream_word=None):
        """``run_joint_quant`` for a group of up to N.JOINT_WIDE_MAX_DIMS
        coordinates: at least one continuous label, 0 to N.JOINT_WIDE_MAX_CAT
        discrete ones and 1 to N.JOINT_MAX_QUANT quantised ones
        (tpe_joint_wide_quant_run, include/tpe_hip.h "Wide quantised joint
        stage"): the same arguments, model, tables, kernel coordinate order,
        Philox streams and return shapes; the records are
        N.JOINT_WIDE_RECORD_DTYPE.  The continuous and discrete coordinates are
        those of ``run_joint_wide_mixed`` (``run_joint_wide`` without discrete
        labels) over the group without its quantised labels, and a group that
        ``run_joint_quant`` also takes draws that method's candidates.  The
        stage is neither sharded nor batch-aware: there is no ``shard`` and no
        ``liar`` argument."""
        return self._joint_solo('wide_quant', below, above, low, high, cats, quants, ids, n_cand, seed, inject,
                                return_cand, want_lg, report_k, stream_word, None, return_table)

    def device_tables(self):
        """(problems, comp32) of the last ``run`` as the device holds them after
        its stages ran — device-fitted above rows and the problem fields the fit
        patches included (tests of the device Parzen fit read them back)."""
        info = self._last_info
        nb = int(info.blob_bytes)
        blob = self._bufs['blob'][:nb].cpu().numpy()
        prob = np.frombuffer(blob, dtype=N.PROBLEM_DTYPE, count=int(info.n_problems),
                             offset=int(info.off_problems)).copy()
        o = int(info.off_comp32)
        comp32 = np.frombuffer(blob[o:o + (nb - o) // 16 * 16], dtype=np.float32).reshape(-1, 4).copy()
        return prob, comp32

    def _run_profiled(self, b, stream, tb, n_cand):
        """The same launches as tpe_run_batch, one stage at a time, bracketed
        by events on the launch stream (bench.py's roofline measurement).
        profile[name] gets (ms, units) per launch: units = algorithmic CE for
        the above kernels (+ exact CE, expanded components and candidates for
        k_above_f32), algorithmic bytes for the sort, candidates otherwise."""
        prob = tb['prob']
        fam = prob['family']
        ce = (prob['above_len'].astype(np.float64) * n_cand)
        groups = [((fam == N.FAM_GAUSS) | (fam == N.FAM_LOGGAUSS),
                   'k_above_f32' if self.precision == 'fp32' else 'k_above_f64'),
                  (fam == N.FAM_QGAUSS, 'k_above_qgauss'), (fam == N.FAM_QLOGGAUSS, 'k_above_qlog')]
        counts = list(tb['counts_w'])
        stages = []
        if b.n_fit:
            stages.append(('fit', self.lib.tpe_fit_above, None, float(b.fit_total)))
        if b.n_tab_jobs:
            stages.append(('k_tables', self.lib.tpe_tables, None, float(b.tab_units)))
        stages.append(('k_sample', self.lib.tpe_sample, None, float(tb['P'] * n_cand)))
        ordered = (bool(b.draw_pref) and b.sample and b.precision == N.PREC_F32 and b.n_sorted > 0
                   and (b.flags & N.BATCH_ORDERED_DRAWS))
        if b.sort_end_bit and b.sort_count and not ordered:     # ordered draws need no sort
            # units: bytes of an LSD radix sort of (u32 key, u64 value) pairs —
            # every 8-bit pass reads and writes both arrays
            passes = (int(b.sort_end_bit) + 7) // 8
            stages.append(('sort', self.lib.tpe_sort, None, float(passes * 2 * 12 * int(b.sort_count))))
        for gi, (mask, name) in enumerate(groups):
            if counts[gi]:
                stages.append((name, self.lib.tpe_score_above, gi, float(ce[mask].sum())))
        stages.append(('k_finalize', self.lib.tpe_finalize, None, float(tb['P'] * n_cand)))
        stages.append(('k_select', self.lib.tpe_select, None, float(tb['P'])))
        cnt = self._buf('ce_count', 2 * max(counts[0], 1), torch.int64)
        cnt.zero_()
        b.ce_count = cnt.data_ptr()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        cur = torch.cuda.current_stream(self.device)
        evs[0].record(cur)
        work0 = b.work
        rep = max(1, int(self.profile_repeat))
        for i, (name, fn, gi, units) in enumerate(stages):
            arg = b
            if gi is not None:
                arg = N.Batch.from_buffer_copy(b)
                arg.n_work_cont, arg.n_work_qgauss, arg.n_work_qlog = [c if j == gi else 0 for j, c in
                                                                       enumerate(counts)]
                arg.work = work0 + N.WORK_DTYPE.itemsize * sum(counts[:gi])   # this group's first item
            for _ in range(rep):
                N.check(fn(ctypes.byref(arg), ctypes.c_void_p(stream)), self.lib, name)
            evs[i + 1].record(cur)
        evs[-1].synchronize()
        self.last_ce = cnt[:2 * counts[0]].view(-1, 2).cpu().numpy() if counts[0] else None   # per work item
        cc = cnt[:2 * counts[0]].view(-1, 2).sum(0).tolist() if counts[0] else [0, 0]
        executed, expanded = int(cc[0]), int(cc[1])
        b.ce_count = None
        for i, (name, fn, gi, units) in enumerate(stages):
            rec = (evs[i].elapsed_time(evs[i + 1]) / rep, units)
            if name == 'k_sample':
                # algorithmic component evaluations of the tabulated problems (C x K
                # per problem: what the reference evaluates; the tables do not)
                tabp = prob['tab_mode'] != N.TAB_NONE
                rec = rec + (float(((prob['below_len'] + prob['above_len'])[tabp]).astype(np.float64).sum()
                                   * n_cand),)
            if name == 'k_above_f32':
                n_c = float(((fam == N.FAM_GAUSS) | (fam == N.FAM_LOGGAUSS)).sum() * n_cand)
                rec = rec + (float(executed), float(expanded), n_c)
            self.profile.setdefault(name, []).append(rec)


_ENGINES = {}
_CURRENT = {}      # device index -> its engine key (get_engine without a device)


def get_engine(device=None, precision='fp32'):
    """Process-wide engine per device (buffers are reused across suggests)."""
    if torch is None:
        raise N.NativeUnavailable('torch is required for device memory')
    if device is None:
        # (an engine already made for the current device: no availability query per suggest)
        eng = _ENGINES.get(_CURRENT.get(torch.cuda.current_device()) if _CURRENT else None)
        if eng is not None:
            eng.set_precision(precision)
            return eng
        if not torch.cuda.is_available():
            raise N.NativeUnavailable('no HIP device visible: the TPE engine has no CPU fallback')
        device = torch.device('cuda', torch.cuda.current_device())
        _CURRENT[device.index] = str(device)
    key = str(device)
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = Engine(device, precision)
    eng.set_precision(precision)
    return eng
