"""Time the candidate report against the only route there was before it.
Usage: python tools/report_time.py [--pairs 50] [--warmup 3] [--k 8] [--cand 1048576] [--out FILE]

Workload: config 3's four headline labels (model, svm_kernel, svm_C,
svm_rbf_gamma fitted from bench.py's 10k-trial history), one new id,
C = 2^20 candidates each, k = 8.  Two routes to the k best distinct values and
the score statistics of every label, alternating, each timed from a
synchronised device to its results on the host (wall clock) and by device
events around the same work:

  (a) host    Engine.run(want_lg=True, return_cand=True) — three float64
              [P, C] arrays copied to the host — then the numpy ranking and
              statistics
  (b) device  Engine.run(report_k=k) — tpe_report on the device, P * (k * 32 +
              68) bytes copied

plus the two report kernels' own device times (tpe_report_profile) and the
pass-1 read rate at 24 B per candidate against the 8 TB/s HBM peak.  One JSON
line goes to stdout and is appended to --out (default
profiles/report_time.jsonl)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def top_distinct(cand, l, g, k):
    s = l - g
    i = np.arange(len(s))
    nan = np.isnan(s)
    order = np.lexsort((i, np.where(nan, 0.0, -s), ~nan))
    out, seen = [], set()
    for j in order:
        if cand[j] not in seen:
            seen.add(cand[j])
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
    ap.add_argument('--pairs', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--cand', type=int, default=1 << 20)
    ap.add_argument('--history', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'report_time.jsonl'))
    args = ap.parse_args()

    import torch
    import bench
    from hyperopt_amd import _native as N, history as H, tpe
    from hyperopt_amd.engine import LevelProblem, get_engine

    n_hist = bench.N_HISTORY if args.history is None else args.history
    domain, trials = bench.make_history(n_hist, bench.SEED)
    T = domain.table
    hist = H.extract(domain, trials)
    eng = get_engine(None, 'fp32')
    fits = tpe._Fits(T, hist, H.split_below(hist, 0.25), 1.0, eng)
    rows = [T.by_label[lab] for lab in ('model', 'svm_kernel', 'svm_C', 'svm_rbf_gamma')]
    ids = np.array([len(hist)], dtype=np.int64)
    problems = [LevelProblem(fits.get(r), r.index, ids) for r in rows]
    C, k, P = args.cand, args.k, len(rows)
    lib = eng.lib

    def route_host():
        res, cand, l, g = eng.run(problems, C, bench.SEED, want_lg=True, return_cand=True)
        out = []
        with np.errstate(invalid='ignore'):
            for p in range(P):
                out.append((top_distinct(cand[p], l[p], g[p], k), host_stats(l[p] - g[p])))
        return out

    def route_device():
        return eng.run(problems, C, bench.SEED, report_k=k)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), out

    for _ in range(args.warmup):
        a = route_host()
        b = route_device()
    # the two routes agree (ranking and counts) before anything is timed
    for p in range(P):
        assert list(b[1][p]['global_idx'][:b[2][p]]) == list(a[p][0]), (p, b[1][p], a[p][0])
        st = b[3][p]
        assert (st['n_finite'], st['n_nan'], st['n_posinf'], st['n_neginf']) == a[p][1][:4], p

    wall = {'host': [], 'device': []}
    dev = {'host': [], 'device': []}
    kern = []
    ms2 = (ctypes.c_double * 2)()
    for _ in range(args.pairs):
        w, d, _ = timed(route_host)
        wall['host'].append(w)
        dev['host'].append(d)
        N.check(lib.tpe_report_profile(1, None), lib, 'tpe_report_profile')
        w, d, _ = timed(route_device)
        N.check(lib.tpe_report_profile(0, ms2), lib, 'tpe_report_profile')
        wall['device'].append(w)
        dev['device'].append(d)
        kern.append((ms2[0], ms2[1]))
    med = lambda x: float(np.median(x))   # noqa: E731
    k1, k2 = med([a for a, _ in kern]), med([b for _, b in kern])
    line = dict(tool='report_time', labels=[r.label for r in rows], history=n_hist, n_cand=C, k=k, pairs=args.pairs,
                host_route_ms=dict(wall_median=med(wall['host']), wall_min=min(wall['host']),
                                   wall_max=max(wall['host']), device_events_median=med(dev['host'])),
                device_route_ms=dict(wall_median=med(wall['device']), wall_min=min(wall['device']),
                                     wall_max=max(wall['device']), device_events_median=med(dev['device'])),
                k_report_chunk_ms=k1, k_report_merge_ms=k2,
                pass1_bytes=24 * P * C, pass1_read_rate_tbs=24.0 * P * C / (k1 * 1e-3) / 1e12 if k1 > 0 else None,
                pass1_fraction_of_hbm_peak=24.0 * P * C / (k1 * 1e-3) / HBM_PEAK if k1 > 0 else None,
                device_route_faster=med(wall['device']) < med(wall['host']),
                gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')
    return 0 if line['device_route_faster'] else 1


if __name__ == '__main__':
    sys.exit(main())
