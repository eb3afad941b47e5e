"""The lazy categorical selection's cases and its model in numpy, shared by
tests/test_lazy_host.py (CPU) and tests/test_gpu_lazy_fused.py.

A spec is (name, below p, above p, n_cand, cand_base): the category weights of
a categorical label as a parzen.Posterior takes them.  A case adds the per-call
words and the three columns the selection reads — cum (the sampler rows'
first), l and g (ln p: the comp64 rows' first) — either made here (the packer's
arithmetic: tests/draw_ref.sampler_rows, np.log) or read from a packed level.

The model draws every candidate with draw_ref's Philox and component search,
takes each category's first index, and gives the winner in np.argmax order (NaN
first, then the score, then the smaller index) together with `need`: the draws
after which no undrawn drawable category could beat the best (n_cand if that
never holds) — the fewest a draw budget must allow.  The host selection
(hyperopt_amd/csrc/tpe_lazy_host.h) is run through the stand-alone program
tools/ubench/lazy_scan_ubench.cpp, built here with the C++ compiler.
"""
import os
import shutil
import subprocess

import numpy as np

from tests import draw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNLIMITED = 1 << 62
BASES = (0, 12345677, (1 << 32) + 5)           # 0, odd, the counter's high word set
SEED = 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF
LABEL, NEW_ID = 11, 2000


def _weights(K, s):
    rs = np.random.RandomState(300 + 7 * K + s)
    pb, pa = rs.uniform(0.2, 1.0, K), rs.uniform(0.2, 1.0, K)
    return pb / pb.sum(), pa / pa.sum()


def specs():
    out = []
    for K in (2, 3, 64):
        for s, base in enumerate(BASES):
            pb, pa = _weights(K, s)
            out.append(('K%d base%d' % (K, s), pb, pa, 5000, base))
    eq = np.array([0.3, 0.3, 0.4])
    out.append(('equal scores', eq, eq.copy(), 4096, 7))
    # a category no draw can reach (its weight vanishes in the running sum) with the best score
    out.append(('zero mass best', np.array([0.5, 1e-20, 0.5]), np.array([0.5, 1e-30, 0.5]), 4096, 1))
    for n in (40, 5000):                       # the best category rare: n_cand below and above its first draw
        out.append(('rare best n%d' % n, np.array([1 - 1 / 300., 1 / 300.]), np.array([1 - 1e-6, 1e-6]), n, 9))
    pb, pa = _weights(3, 9)
    out.append(('one candidate', pb, pa, 1, 11))
    return out


def made_case(spec, nan_at=None):
    """The case of a spec with the columns made here; nan_at: that category's l
    (and so its score) a NaN."""
    name, pb, pa, n_cand, base = spec
    with np.errstate(divide='ignore'):
        l, g = np.log(pb), np.log(pa)
    if nan_at is not None:
        l = l.copy()
        l[nan_at] = np.nan
    return dict(name=name, key0=SEED & 0xFFFFFFFF, key1=SEED >> 32, ctr2=LABEL, ctr3=NEW_ID, cand_base=base,
                n_cand=n_cand, cum=R.sampler_rows(R.CATEGORICAL, p=pb)[:, 0].copy(), l=l, g=g)


def cpu_cases():
    out = [made_case(s) for s in specs()]
    nan = made_case(('nan score', *_weights(3, 5), 4096, 3), nan_at=1)
    return out + [nan]


def _better(s, i, bs, bi):
    if bi < 0:
        return i >= 0
    if i < 0:
        return False
    n, bn = s != s, bs != bs
    if n or bn:
        return n and (not bn or i < bi)
    return s > bs or (s == bs and i < bi)


def model(c):
    """(need, (score, l, g, value, idx, global_idx)) of a case."""
    n, K = int(c['n_cand']), len(c['cum'])
    if n == 0:
        return 0, (0.0, 0.0, 0.0, 0.0, -1, -1)
    gidx = np.uint64(c['cand_base']) + np.arange(n, dtype=np.uint64)
    x, y, _, _ = R.philox4x32_10(gidx & np.uint64(0xFFFFFFFF), gidx >> np.uint64(32), c['ctr2'], c['ctr3'],
                                 c['key0'], c['key1'])
    cat = R.component(c['cum'], R.u01d(x, y))
    cats, first = np.unique(cat, return_index=True)
    with np.errstate(invalid='ignore'):
        score = np.asarray(c['l'], dtype=np.float64) - np.asarray(c['g'], dtype=np.float64)
    drawable = np.diff(np.concatenate([[0.0], c['cum']])) > 0
    bs, bi, bc = 0.0, -1, -1
    drawn = np.zeros(K, dtype=bool)
    need = n
    for i, k in sorted(zip(first.tolist(), cats.tolist())):
        drawn[k] = True
        if _better(float(score[k]), i, bs, bi):
            bs, bi, bc = float(score[k]), i, k
        more = any((not drawn[j]) and drawable[j] and _better(float(score[j]), 1 << 62, bs, bi) for j in range(K))
        if not more and need == n:
            need = i + 1
    return need, (bs, float(c['l'][bc]), float(c['g'][bc]), float(bc), bi, int(c['cand_base']) + bi)


def build_program(out_dir):
    gxx = shutil.which(os.environ.get('CXX', 'g++'))
    assert gxx is not None, 'no C++ compiler'
    exe = os.path.join(str(out_dir), 'lazy_scan_ubench')
    subprocess.check_call([gxx, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'hyperopt_amd', 'csrc'),
                           os.path.join(ROOT, 'tools', 'ubench', 'lazy_scan_ubench.cpp'), '-o', exe])
    return exe


def _hex(v):
    v = float(v)
    return 'nan' if v != v else v.hex()


def host_select(exe, cases, budgets, tmp_dir):
    """The program's result of each (case, budget): (draws, (score, l, g, value,
    idx, global_idx)), draws = -1 when the selection did not settle."""
    path = os.path.join(str(tmp_dir), 'lazy_cases.txt')
    with open(path, 'w') as f:
        for c, b in zip(cases, budgets):
            K = len(c['cum'])
            head = [c['key0'], c['key1'], c['ctr2'], c['ctr3'], c['cand_base'], c['n_cand'], K, int(b)]
            cols = [_hex(v) for col in (c['cum'], c['l'], c['g']) for v in col]
            f.write(' '.join(str(int(v)) for v in head) + ' ' + ' '.join(cols) + '\n')
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    res = []
    for line in out.stdout.splitlines():
        t = line.split()
        res.append((int(t[0]), tuple(float.fromhex(v) for v in t[1:5]) + (int(t[5]), int(t[6]))))
    assert len(res) == len(cases), out.stdout
    return res


def same(a, b):
    """Two results equal bit for bit; a NaN equals a NaN (the program's text
    output carries no payload)."""
    fa, fb = np.array(a[:4], dtype=np.float64), np.array(b[:4], dtype=np.float64)
    nan = np.isnan(fa)
    return bool(np.array_equal(nan, np.isnan(fb)) and fa[~nan].tobytes() == fb[~nan].tobytes() and
                tuple(int(v) for v in a[4:]) == tuple(int(v) for v in b[4:]))


# ------------------------------------------------------------ the fused hit
def fused_level(domain, trials, n_cand):
    """The problem rows (numpy, _native.PROBLEM_DTYPE) of the one level a
    single-id tpe.suggest runs on this history at n_cand candidates — the
    predicted branch's labels, packed by tpe_host_pack_level on the host (no
    GPU) — or None when the gates' prediction does not hold at this count."""
    import ctypes
    from hyperopt_amd import _native as N, history as H, tpe
    from hyperopt_amd.engine import Engine, LevelProblem
    hist = H.extract(domain, trials)
    fits = tpe._Fits(domain.table, hist, H.split_below(hist, 0.25), 1.0, None)
    pred = tpe._predict_activity(domain.table, fits, n_cand)
    if pred is None:
        return None
    ids = np.array([len(hist)], dtype=np.int64)
    problems = [LevelProblem(fits.get(r), r.index, ids) for r in domain.table.rows if pred[r.label] is not None]
    recs, keep = Engine._labels(problems)
    lib = N.load()
    blob = np.zeros(64 << 20, dtype=np.uint8)
    info = N.PackInfo()
    rc = lib.tpe_host_pack_level(recs, len(problems), int(n_cand), 7, 0, 0, N.PREC_F32, blob.ctypes.data, blob.size,
                                 ctypes.byref(info))
    assert rc == 0, rc
    del keep
    return np.frombuffer(blob, dtype=N.PROBLEM_DTYPE, count=int(info.n_problems), offset=int(info.off_problems)).copy()


def fused_eligible(rows):
    """Whether the level's rows allow the fused hit (level_run_impl): every
    problem a lazy categorical or tabulated within k_sample_fast's reach
    (tab_fast >= 2: log-polynomial cells of at most 896 rows or a lattice of at
    most 1024 values, at most 64 sampler rows)."""
    from hyperopt_amd import _native as N
    if rows is None:
        return False
    for p in rows:
        if p['tab_mode'] == N.TAB_NONE:
            if not (p['family'] == N.FAM_CATEGORICAL and (p['flags'] & N.F_CAT_LAZY) and p['samp_len'] <= 64):
                return False
        elif p['tab_mode'] == N.TAB_CELLS:
            if not ((p['flags'] & N.F_LOGPOLY) and p['tab_n'][0] <= 896 and 0 < p['samp_len'] <= 64):
                return False
        elif not (p['tab_mode'] == N.TAB_LATTICE and p['tab_n'][0] <= 1024 and 0 < p['samp_len'] <= 64):
            return False
    return bool((rows['tab_mode'] != N.TAB_NONE).any())


def min_fused_count(domain, trials, hi=1 << 20):
    """The smallest candidate count whose level is fused-eligible, by bisection
    (eligibility is monotone in the count: the packer tabulates a label from a
    count on, and the gates' prediction holds from a count on)."""
    assert fused_eligible(fused_level(domain, trials, hi))
    lo = 1                                     # (not eligible: no label is tabulated for one candidate)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fused_eligible(fused_level(domain, trials, mid)):
            hi = mid
        else:
            lo = mid
    return hi
