"""Time the segmented joint stage against one tpe_joint_run per branch group.
Usage: python tools/joint_branch_time.py [--pairs 7] [--warmup 2] [--out FILE] [--small] [--wide]

Two workloads (DESIGN.md "Branch groups"), each with two routes to the same
winners, alternating in one process, each timed from a synchronised device to
the records on the host (wall clock):

  (a) 64 new ids over 8 branch groups of D = 4 (8 ids a group), 2,000 seeded
      trials a group (K_below = 13, K_above = 1989), C = 4096 candidates:
        segmented  one Engine.run_joint_segments call: one upload, the order
                   kernel, one k_joint_seg_chunk<4> launch of 256 workgroups,
                   one merge, one download
        per group  eight Engine.run_joint calls, each with its group's 8 ids:
                   an upload, a k_joint_chunk<4> launch of 32 workgroups, a
                   merge and a download per group (the code before the
                   segmented stage: the baseline)
  (b) one id, one group of D = 4, 10,000 trials, C = 2^20: what the descriptor
      indirection costs k_joint_seg_chunk<4> against k_joint_chunk<4>.

The routes' records must be equal where they can be: the segmented call runs
with each group's own stream word, the per-group route with the root word, so
the tool checks the bytes against per-group runs at the group's word (untimed).
After the wall-clock rounds the kernels are timed by their own events
(tpe_joint_profile), alternating again: the chunk launches summed (with the
order kernel for the segmented route) and the merge.  One JSON line per
workload goes to stdout and is appended to --out (default
profiles/joint_branch_time.jsonl).  --small: tiny sizes, to rehearse the tool.

--wide: the same two comparisons for the wide segmented stage (DESIGN.md "Wide
branch groups"), appended to profiles/joint_branch_wide_time.jsonl:
  (a) 64 new ids over 4 branch groups of D = 20, 24, 33 and 64 (16 ids a
      group), 2,000 trials a group, C = 4096: one
      Engine.run_joint_wide_segments call against four Engine.run_joint_wide
      calls, each with its group's ids
  (b) one id, one group of D = 32, 10,000 trials, C = 2^20:
      k_joint_wide_seg_chunk<32, 2> against k_joint_wide_chunk<32, 2>.
Here the chunk figure holds the scoring launches (with the order kernel for the
segmented route) and the sampling kernels are reported beside it
(tpe_joint_wide_profile)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SEED = 20240607


def make_group(n, seed):
    """A seeded D = 4 group (uniform, log-uniform, normal, uniform coordinates)
    of n trials whose loss couples x0 with x1: (below, above, low, high)."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-5, 5, n), rs.uniform(-3, 2, n), rs.normal(0, 2, n), rs.uniform(0, 1, n)], axis=1)
    loss = (X[:, 0] * np.exp(X[:, 1]) - 2.0) ** 2 + 0.1 * X[:, 2] ** 2 + (X[:, 3] - 0.3) ** 2 \
        + 0.01 * rs.standard_normal(n)
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    priors = [(0.0, 10.0), (-0.5, 5.0), (0.0, 2.0), (0.5, 1.0)]
    low, high = np.array([-5.0, -3.0, -np.inf, 0.0]), np.array([5.0, 2.0, np.inf, 1.0])
    return J.side_mixture(X[m], priors), J.side_mixture(X[~m], priors), low, high


def make_wide_group(D, n, seed):
    """A seeded group of D coordinates (even ones uniform on [-5, 5), odd ones
    normal) of n trials whose loss couples neighbouring coordinates."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(seed)
    even = np.arange(D) % 2 == 0
    X = np.where(even[None, :], rs.uniform(-5, 5, (n, D)), rs.normal(0, 2, (n, D)))
    loss = np.mean((X[:, :-1] + X[:, 1:] - 1.0) ** 2, axis=1) + 0.01 * rs.standard_normal(n)
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    priors = [(0.0, 10.0) if e else (0.0, 2.0) for e in even]
    low, high = np.where(even, -5.0, -np.inf), np.where(even, 5.0, np.inf)
    return J.side_mixture(X[m], priors), J.side_mixture(X[~m], priors), low, high


def stats(x):
    return dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)), all=[float(v) for v in x])


def measure(name, eng, models, words, prob_seg, prob_id, C, args):
    import torch
    from hyperopt_amd import _native as N
    lib = eng.lib
    wide = args.wide
    run_segments = eng.run_joint_wide_segments if wide else eng.run_joint_segments
    run_group = eng.run_joint_wide if wide else eng.run_joint
    prob_seg, prob_id = np.asarray(prob_seg), np.asarray(prob_id, dtype=np.int64)
    groups = [(s, prob_id[prob_seg == s]) for s in range(len(models))]

    def segmented():
        return run_segments(models, words, prob_seg, prob_id, C, SEED)

    def per_group(word=False):
        out = []
        for s, ids in groups:
            b, a, lo, hi = models[s]
            if word:
                out.append(run_group(b, a, lo, hi, ids, C, SEED, None, False, False, stream_word=words[s]))
            else:
                out.append(run_group(b, a, lo, hi, ids, C, SEED))
        return out

    def sample_ms():
        """The sampling kernel of the last profiled wide call."""
        ms = ctypes.c_double(0.0)
        N.check(lib.tpe_joint_wide_profile(ctypes.byref(ms)), lib, 'tpe_joint_wide_profile')
        return ms.value

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                     # (returns with the records on the host)
        return (time.perf_counter() - t0) * 1e3

    def kernel_ms(fn, n_calls):
        """Device times {chunk launches, merge, wide: sampling kernels} summed over the route's calls."""
        ms2 = (ctypes.c_double * 2)()
        tot = [0.0, 0.0, 0.0]
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        if n_calls == 1:
            fn()
            samp = sample_ms() if wide else 0.0  # (before tpe_joint_profile starts the next round)
            N.check(lib.tpe_joint_profile(1, ms2), lib, 'tpe_joint_profile')
            tot = [ms2[0], ms2[1], samp]
        else:                                    # the per-group route: read after every call
            for s, ids in groups:
                b, a, lo, hi = models[s]
                run_group(b, a, lo, hi, ids, C, SEED)
                tot[2] += sample_ms() if wide else 0.0
                N.check(lib.tpe_joint_profile(1, ms2), lib, 'tpe_joint_profile')
                tot[0] += ms2[0]
                tot[1] += ms2[1]
        N.check(lib.tpe_joint_profile(0, None), lib, 'tpe_joint_profile')
        return tot

    for _ in range(args.warmup):
        segmented()
        per_group()
    # the same winners: the segmented records against per-group runs at each group's stream word
    rec = segmented()
    ref = per_group(word=True)
    for s, ids in groups:
        assert rec[prob_seg == s].tobytes() == ref[s].tobytes(), 'group %d: records differ' % s
    ws, wg = [], []
    for i in range(args.pairs):
        ws.append(wall(segmented))
        wg.append(wall(per_group))
        print('%s round %d: segmented %.3f ms, per group %.3f ms' % (name, i, ws[-1], wg[-1]), file=sys.stderr,
              flush=True)
    ks, kg = [], []
    for i in range(args.pairs):
        ks.append(kernel_ms(segmented, 1))
        kg.append(kernel_ms(per_group, len(groups)))
    D = len(models[0][2])
    evals = float(sum(len(ids) * C * (len(models[s][0][0]) + len(models[s][1][0])) * len(models[s][2])
                      for s, ids in groups))
    ks_chunk, kg_chunk = np.median([k[0] for k in ks]), np.median([k[0] for k in kg])
    if wide:                                     # chunks of 256 R candidates, R by the group's padded width
        def chunks(s):
            return -(-C // (512 if len(models[s][2]) <= 32 else 256))
        wgs = dict(segmented_launches=[int(len(ids) * chunks(s)) for s, ids in groups],
                   per_group_launch=[int(len(ids) * chunks(s)) for s, ids in groups])
    else:
        wgs = dict(segmented_launch=int(len(prob_seg) * -(-C // N.JOINT_CHUNK)),
                   per_group_launch=[int(len(ids) * -(-C // N.JOINT_CHUNK)) for _, ids in groups])
    line = dict(tool='joint_branch_time', workload=name, n_groups=len(models), n_problems=int(len(prob_seg)),
                n_dims=[len(m[2]) for m in models] if wide else D, n_cand=C,
                k_below=[len(m[0][0]) for m in models], k_above=[len(m[1][0]) for m in models],
                pairs=args.pairs, warmup=args.warmup,
                workgroups=wgs,
                wall_ms=dict(segmented=stats(ws), per_group=stats(wg),
                             ratio_of_medians=float(np.median(wg) / np.median(ws))),
                kernel_ms=dict(segmented_chunk=stats([k[0] for k in ks]), segmented_merge=stats([k[1] for k in ks]),
                               per_group_chunk=stats([k[0] for k in kg]), per_group_merge=stats([k[1] for k in kg]),
                               chunk_ratio_of_medians=float(kg_chunk / ks_chunk) if ks_chunk > 0 else None),
                evals_per_s=dict(segmented=evals / (ks_chunk * 1e-3) if ks_chunk > 0 else None,
                                 per_group=evals / (kg_chunk * 1e-3) if kg_chunk > 0 else None),
                records_equal=True, gpu=torch.cuda.get_device_name(0))
    if wide:
        line['kernel_ms'].update(segmented_sample=stats([k[2] for k in ks]), per_group_sample=stats([k[2] for k in kg]))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_branch_wide_time.jsonl' if wide
                                   else 'joint_branch_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--small', action='store_true')
    ap.add_argument('--wide', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print('joint_branch_time needs a GPU: nothing is measured without one', file=sys.stderr)
        return 2
    from hyperopt_amd.engine import get_engine
    eng = get_engine(None, 'fp32')
    n_a, n_b, c_b = (200, 500, 8192) if args.small else (2000, 10000, 1 << 20)
    if args.wide:
        dims = (20, 24, 33, 64)
        models = [make_wide_group(D, n_a, SEED + s) for s, D in enumerate(dims)]
        words = [0xFFFFFFFE - 70 * s for s in range(4)]
        prob_id = np.arange(n_a, n_a + 64, dtype=np.int64)
        measure('wide a: 64 ids over 4 groups', eng, models, words, np.arange(64) % 4, prob_id, 4096, args)
        measure('wide b: 1 id, 1 group', eng, [make_wide_group(32, n_b, SEED)], [0xFFFFFFFE], [0], [n_b], c_b, args)
        return 0
    models = [make_group(n_a, SEED + s) for s in range(8)]
    words = [0xFFFFFFFE - 5 * s for s in range(8)]
    prob_id = np.arange(n_a, n_a + 64, dtype=np.int64)
    prob_seg = np.arange(64) % 8                 # (every id its own branch: the groups interleave)
    measure('a: 64 ids over 8 groups', eng, models, words, prob_seg, prob_id, 4096, args)
    measure('b: 1 id, 1 group', eng, [make_group(n_b, SEED)], [0xFFFFFFFE], [0], [n_b], c_b, args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
