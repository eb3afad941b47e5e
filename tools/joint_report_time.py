"""Time the joint candidate report against the only route there was before it.
Usage: python tools/joint_report_time.py [--pairs 10] [--warmup 2] [--k 8] [--cand 1048576]
                                         [--history 10000] [--out FILE]

Workload: tools/joint_time.py's case — 4 continuous labels, a 10,000-trial
history, one new id, C = 2^20 candidate vectors, k = 8.  Two routes to the k
best distinct vectors and the score statistics, in alternating pairs, each
timed from a synchronised device to its results on the host (wall clock):

  (a) host    Engine.run_joint(return_cand=True, want_lg=True) — the f32
              [C, 4] rows and two float64 [C] arrays copied to the host — then
              the numpy ranking of rows and the statistics
  (b) device  Engine.run_joint(report_k=k) — tpe_joint_report on the device,
              k * (32 + 4 D) + 68 bytes copied

Both routes run the same joint scoring stage first; its own time (a call
without either) is reported beside them.  Also: the two report kernels' device
times (tpe_joint_report_profile) and the pass-1 read rate at (4 D + 16) B per
candidate (re-reads of rows whose hash matches a round winner's not counted)
against the 8 TB/s HBM peak.  One JSON line goes to stdout and is appended to
--out (default profiles/joint_report_time.jsonl)."""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def top_distinct_rows(cand, l, g, k):
    with np.errstate(invalid='ignore'):
        s = l - g
    i = np.arange(len(s))
    nan = np.isnan(s)
    order = np.lexsort((i, np.where(nan, 0.0, -s), ~nan))
    out, seen = [], set()
    for j in order:
        row = cand[j] + np.float32(0.0)
        key = tuple(row.tolist())
        if np.isnan(row).any() or key not in seen:
            seen.add(key)
            out.append(j)
            if len(out) == k:
                break
    return np.asarray(out, dtype=np.int64)


def host_stats(s):
    fin = s[np.isfinite(s)]
    mean = fin.mean() if len(fin) else np.nan
    return (len(fin), int(np.isnan(s).sum()), int((s == np.inf).sum()), int((s == -np.inf).sum()), mean,
            float(np.sum((fin - mean) ** 2)) if len(fin) else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--cand', type=int, default=1 << 20)
    ap.add_argument('--history', type=int, default=10000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_report_time.jsonl'))
    args = ap.parse_args()

    import torch
    import joint_time
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    domain, hist = joint_time.make_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    model = J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0)
    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C, D, k = args.cand, len(rows), args.k
    ids = np.array([args.history], dtype=np.int64)
    m = (model.below, model.above, model.low, model.high, ids, C, joint_time.SEED)

    def route_stage():
        return eng.run_joint(*m)

    def route_host():
        rec, cand, l, g = eng.run_joint(*m, return_cand=True, want_lg=True)
        with np.errstate(invalid='ignore'):
            return top_distinct_rows(cand[0], l[0], g[0], k), host_stats(l[0] - g[0])

    def route_device():
        return eng.run_joint(*m, report_k=k)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        route_stage()
        a = route_host()
        b = route_device()
    # the two routes agree (ranking and counts) before anything is timed
    assert list(b[1]['idx'][0, :b[3][0]]) == list(a[0]), (b[1], a[0])
    st = b[4][0]
    assert (st['n_finite'], st['n_nan'], st['n_posinf'], st['n_neginf']) == a[1][:4]

    wall = {'stage': [], 'host': [], 'device': []}
    kern = []
    ms2 = (ctypes.c_double * 2)()
    for _ in range(args.pairs):
        wall['stage'].append(timed(route_stage)[0])
        wall['host'].append(timed(route_host)[0])
        N.check(lib.tpe_joint_report_profile(1, None), lib, 'tpe_joint_report_profile')
        wall['device'].append(timed(route_device)[0])
        N.check(lib.tpe_joint_report_profile(0, ms2), lib, 'tpe_joint_report_profile')
        kern.append((ms2[0], ms2[1]))
    med = lambda x: float(np.median(x))   # noqa: E731
    k1, k2 = med([x for x, _ in kern]), med([y for _, y in kern])
    per_cand = 4 * D + 16
    line = dict(tool='joint_report_time', labels=[r.label for r in rows], history=args.history, n_cand=C, k=k,
                pairs=args.pairs, k_below=len(model.below[0]), k_above=len(model.above[0]),
                stage_only_ms=dict(wall_median=med(wall['stage']), wall_min=min(wall['stage']),
                                   wall_max=max(wall['stage'])),
                host_route_ms=dict(wall_median=med(wall['host']), wall_min=min(wall['host']),
                                   wall_max=max(wall['host'])),
                device_route_ms=dict(wall_median=med(wall['device']), wall_min=min(wall['device']),
                                     wall_max=max(wall['device'])),
                host_route_bytes=C * (4 * D + 16), device_route_bytes=k * (32 + 4 * D) + 68,
                k_joint_report_chunk_ms=dict(median=k1, min=min(x for x, _ in kern), max=max(x for x, _ in kern)),
                k_joint_report_merge_ms=dict(median=k2, min=min(y for _, y in kern), max=max(y for _, y in kern)),
                pass1_bytes=per_cand * C, pass1_read_rate_tbs=per_cand * C / (k1 * 1e-3) / 1e12 if k1 > 0 else None,
                pass1_fraction_of_hbm_peak=per_cand * C / (k1 * 1e-3) / HBM_PEAK if k1 > 0 else None,
                device_route_faster=med(wall['device']) < med(wall['host']),
                gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
