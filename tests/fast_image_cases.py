"""Small histories for the fused hit's prepared image (tests/test_gpu_fast_image.py,
tests/test_fast_image_host.py) and the host's view of the level a single-id
tpe.suggest runs on them: the packed rows and the pack info (tpe_host_pack_level,
no GPU), which give the offsets of the staging buffer's sections.

What the packer can make decides the edges: a label's sampler rows are its
below observations and the prior, 1 to 26 (history.split_below caps the below
set at 25), and a bounded label's log-polynomial table has 9 cells on an empty
history and 850 from 99 observations on (tab_cells: the range over the
smallest bandwidth, which the fit clips at a hundredth of the range); an
unbounded label's grows with its observations' spread, up to the fused kernel's
896 rows."""
import ctypes

import numpy as np


def make(space, n, seed=0, loss=None, fix=None):
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(seed)
    for tid in range(n):
        d = rand.suggest([tid], domain, trials, rs.randint(2 ** 31 - 1))[0]
        if fix:
            fix(tid, d)
        d['state'] = base.JOB_STATE_DONE
        d['result'] = {'status': 'ok', 'loss': float(loss(tid) if loss else rs.uniform())}
        trials.insert_trial_docs([d])
    trials.refresh()
    return domain, trials


def _outlier(tid, doc):
    if tid == 2:
        doc['misc']['vals']['z'] = [5.5]


def cases():
    """name -> (domain, trials, gamma, {label: (sampler rows, cells or None)})"""
    from hyperopt_amd import hp
    x = lambda: {'x': hp.uniform('x', -1, 1)}
    xz = lambda: {'x': hp.uniform('x', -1, 1), 'z': hp.normal('z', 0, 1)}
    return {
        'one row, nine cells': make(x(), 0) + (0.25, {'x': (1, 9)}),
        'two rows': make(xz(), 5) + (0.25, {'x': (2, None), 'z': (2, None)}),
        '26 rows': make(x(), 120) + (3.0, {'x': (26, None)}),
        '850 cells': make(x(), 200) + (0.25, {'x': (None, 850)}),
        # an unbounded label whose best trial lies 5.5 prior sigmas out: cells over [-8, 9.5], 892 of
        # the fused kernel's 896 (5.7 makes 902 and an unfused level), and draws beyond them
        'outlier': make({'z': hp.normal('z', 0, 1)}, 5, loss=lambda tid: -1.0 if tid == 2 else 1.0 + tid,
                        fix=_outlier) + (0.25, {'z': (2, 892)}),
    }


def level(domain, trials, n_cand, gamma=0.25):
    """(rows, info) of the level, or (None, None) when the gates' prediction does not hold"""
    from hyperopt_amd import _native as N, history as H, tpe
    from hyperopt_amd.engine import Engine, LevelProblem
    hist = H.extract(domain, trials)
    fits = tpe._Fits(domain.table, hist, H.split_below(hist, gamma), 1.0, None)
    pred = tpe._predict_activity(domain.table, fits, n_cand)
    if pred is None:
        return None, None
    ids = np.array([len(hist)], dtype=np.int64)
    problems = [LevelProblem(fits.get(r), r.index, ids) for r in domain.table.rows if pred[r.label] is not None]
    recs, keep = Engine._labels(problems)
    blob = np.zeros(64 << 20, dtype=np.uint8)
    info = N.PackInfo()
    rc = N.load().tpe_host_pack_level(recs, len(problems), int(n_cand), 7, 0, 0, N.PREC_F32, blob.ctypes.data, blob.size,
                                      ctypes.byref(info))
    assert rc == 0, rc
    del keep
    rows = np.frombuffer(blob, dtype=N.PROBLEM_DTYPE, count=int(info.n_problems), offset=int(info.off_problems)).copy()
    return rows, info


def staged(engine, info):
    """the engine's staging buffer after a suggest: (problem rows, f64 sampler
    rows [n, 8], result rows) at the offsets of `info`"""
    from hyperopt_amd import _native as N
    host = engine._pinned.numpy()
    P = int(info.n_problems)
    rows = np.frombuffer(host, dtype=N.PROBLEM_DTYPE, count=P, offset=int(info.off_problems)).copy()
    n_samp = int(max(int(p['samp_off']) + int(p['samp_len']) for p in rows))
    samp = np.frombuffer(host, dtype=np.float64, count=8 * n_samp, offset=int(info.off_samp)).reshape(-1, 8).copy()
    res_off = (int(info.blob_bytes) + 255) & ~255          # (level_need: the results follow the blob)
    res = np.frombuffer(host, dtype=N.RESULT_DTYPE, count=P, offset=res_off).copy()
    return rows, samp, res
