"""Time the segmented joint stage against one tpe_joint_run per branch group.
Usage: python tools/joint_branch_time.py [--pairs 7] [--warmup 2] [--out FILE] [--small] [--wide | --fp64 [--mixed]]

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
(tpe_joint_wide_profile).

--fp64: the float64 segmented stage (DESIGN.md "Float64 branch groups"),
appended to profiles/joint_branch_fp64_time.jsonl.  Workloads (a) and (b) above
and (c), as (b) at D = 16; three routes alternating in one process:
  seg64      one Engine.run_joint_segments(precision='fp64') call
  group64    one Engine.run_joint(precision='fp64', stream_word=...) per group
  seg32      one Engine.run_joint_segments call
Wall clock from a synchronised device, then the kernels by their own events
(tpe_joint_profile; the psi kernel: tpe_joint_seg_f64_profile).  seg64's records
must be group64's bytes.  A difference of two medians is `shown` only if it
exceeds three times the larger of the two ranges.  Each
line also holds the worst distance of seg32's l and g from seg64's over the
shared pool, as a fraction of 1e-5 max(1, |ref|); a last line does that for a
clustered branch (every bandwidth psig / 100).

--fp64 --mixed: the float64 mixed segmented stage (DESIGN.md "Float64 mixed
branch groups"), appended to profiles/joint_branch_mq_fp64_time.jsonl, the same
three routes over groups with discrete and quantised labels:
  seg64      one Engine.run_joint_msegments_f64 call
  group64    one Engine.run_joint_quant / run_joint_mixed(precision='fp64',
             stream_word=...) per group
  seg32      one Engine.run_joint_segments call (tpe_joint_mseg_run)
Workloads: (a) 64 ids over 8 groups of 3 continuous labels + a choice of 4 + a
quniform of 32, 2,000 trials a group, C = 4096; (b) 1 id, one group of a
quniform of 50 x a choice of 2 (no continuous label), 10,000 trials, C = 2^20;
(c) 1 id, one group of 3 continuous labels + a quniform of 256, 10,000 trials,
C = 2^20.  The psi and the table kernel: tpe_joint_mseg_f64_profile."""
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


def make_clustered_group(n, seed):
    """make_group's space with every trial within 1e-3 prior sigmas of one point."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(seed)
    priors = [(0.0, 10.0), (-0.5, 5.0), (0.0, 2.0), (0.5, 1.0)]
    X = np.array([m + 0.03 * sg for m, sg in priors])[None, :] + 1e-3 * np.array([sg for _, sg in priors])[None, :] \
        * rs.uniform(0, 1, (n, 4))
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    low, high = np.array([-5.0, -3.0, -np.inf, 0.0]), np.array([5.0, 2.0, np.inf, 1.0])
    return J.side_mixture(X[:nb], priors), J.side_mixture(X[nb:], priors), low, high


def make_mixed_group(n, seed, Dc, us, Vs):
    """make_group's first Dc coordinates, then a category of u values for every
    u in us and a lattice of V values for every V in Vs, each trial's drawn at
    random; a component's lattice bandwidth is V / 8 (the prior row: V):
    (below, above, low, high, cats, quants) as Engine.run_joint_quant takes them."""
    below, above, low, high = make_group(n, seed)
    rs = np.random.RandomState(seed + 1)
    sides = [(w, np.asarray(mu)[:, :Dc], np.asarray(sg)[:, :Dc]) for w, mu, sg in (below[:3], above[:3])]
    kb, ka = len(below[0]), len(above[0])
    cats = [(np.concatenate([[-1], rs.randint(0, u, kb - 1)]), np.concatenate([[-1], rs.randint(0, u, ka - 1)]),
             np.full(u, 1.0 / u), 1.0, 1.0) for u in us]
    quants = []
    for V in Vs:
        side = [x for K in (kb, ka) for x in (np.concatenate([[0.5 * (V - 1)], np.rint(rs.uniform(0, V - 1, K - 1))]),
                                              np.concatenate([[float(V)], np.full(K - 1, V / 8.0)]))]
        quants.append(tuple(side) + (np.arange(V + 1) - 0.5,))
    return sides[0], sides[1], low[:Dc], high[:Dc], cats, quants


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


def shown(x, y):
    """Whether the medians of x and y differ by more than three times the larger range."""
    return bool(abs(np.median(x) - np.median(y)) > 3 * max(np.ptp(x), np.ptp(y)))


def measure_fp64(name, eng, models, words, prob_seg, prob_id, C, args, time_it=True, mixed=False):
    import torch
    from hyperopt_amd import _native as N
    lib = eng.lib
    prob_seg, prob_id = np.asarray(prob_seg), np.asarray(prob_id, dtype=np.int64)
    groups = [(s, prob_id[prob_seg == s]) for s in range(len(models))]

    def seg(precision, **kw):
        if mixed and precision == 'fp64':
            return eng.run_joint_msegments_f64(models, words, prob_seg, prob_id, C, SEED, **kw)
        return eng.run_joint_segments(models, words, prob_seg, prob_id, C, SEED, precision=precision, **kw)

    def solo64(s, ids):
        if not mixed:
            return eng.run_joint(*models[s], ids, C, SEED, stream_word=words[s], precision='fp64')
        b, a, lo, hi, cats, quants = models[s]
        if quants:
            return eng.run_joint_quant(b, a, lo, hi, cats, quants, ids, C, SEED, stream_word=words[s], precision='fp64')
        return eng.run_joint_mixed(b, a, lo, hi, cats, ids, C, SEED, stream_word=words[s], precision='fp64')

    def group64():
        return [solo64(s, ids) for s, ids in groups]
    routes = dict(seg64=lambda: seg('fp64'), group64=group64, seg32=lambda: seg('fp32'))

    def events(route):
        """{launches before the merge, merge, psi kernel, mixed: table kernel} of one profiled run of the route, in ms."""
        ms2, psi, tab, tot = (ctypes.c_double * 2)(), ctypes.c_double(0.0), ctypes.c_double(0.0), [0.0, 0.0, 0.0, 0.0]
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        for s, ids in (groups if route == 'group64' else [(None, None)]):   # (the per-group route: read after every call)
            if route == 'group64':
                solo64(s, ids)
            else:
                routes[route]()
            if route == 'seg64' and mixed:
                N.check(lib.tpe_joint_mseg_f64_profile(ctypes.byref(psi), ctypes.byref(tab)), lib,
                        'tpe_joint_mseg_f64_profile')
            elif route == 'seg64':
                N.check(lib.tpe_joint_seg_f64_profile(ctypes.byref(psi)), lib, 'tpe_joint_seg_f64_profile')
            N.check(lib.tpe_joint_profile(1, ms2), lib, 'tpe_joint_profile')
            tot = [tot[0] + ms2[0], tot[1] + ms2[1], psi.value, tab.value]
        N.check(lib.tpe_joint_profile(0, None), lib, 'tpe_joint_profile')
        return tot

    line = dict(tool='joint_branch_time --fp64' + (' --mixed' if mixed else ''), workload=name, n_groups=len(models),
                n_problems=int(len(prob_seg)), n_dims=len(models[0][2]), n_cand=C, k_below=[len(m[0][0]) for m in models],
                k_above=[len(m[1][0]) for m in models], pairs=args.pairs, warmup=args.warmup)
    # the fp32 stage's distance from the float64 stage over the shared pool, in units of the fp32 tolerance
    r64, r32 = seg('fp64', return_cand=True, want_lg=True), seg('fp32', return_cand=True, want_lg=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r64[1], r32[1])), 'the pools differ'
    line['fp32_distance'] = dict((k, float(np.max(np.abs(r32[i] - r64[i]) / (1e-5 * np.maximum(1.0, np.abs(r64[i]))))))
                                 for k, i in (('l', 2), ('g', 3)))
    line['same_winners'] = bool((r64[0]['global_idx'] == r32[0]['global_idx']).all())
    if time_it:
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        rec, ref = routes['seg64'](), routes['group64']()
        for s, ids in groups:
            assert rec[prob_seg == s].tobytes() == ref[s].tobytes(), 'group %d: records differ' % s
        wall, kern = dict((k, []) for k in routes), dict((k, []) for k in routes)
        for i in range(args.pairs):
            for k, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                                 # (returns with the records on the host)
                wall[k].append((time.perf_counter() - t0) * 1e3)
        for i in range(args.pairs):
            for k in routes:
                kern[k].append(events(k))
        # (mixed: a category or lattice slot counts as a dimension)
        evals = float(sum(len(ids) * C * (len(models[s][0][0]) + len(models[s][1][0]))
                          * (len(models[s][2]) + sum(len(x) for x in models[s][4:])) for s, ids in groups))
        pre = dict((k, [e[0] for e in kern[k]]) for k in routes)
        # seg64's launches before the merge without the psi kernel: what compares with k_joint_f64_chunk
        chunk64 = [e[0] - e[2] for e in kern['seg64']]
        line.update(records_equal=True,
                    wall_ms=dict((k, stats(v)) for k, v in wall.items()),
                    kernel_ms=dict([(k + '_before_merge', stats(v)) for k, v in pre.items()] +
                                   [('seg64_psi', stats([e[2] for e in kern['seg64']])),
                                    ('seg64_without_psi', stats(chunk64))] +
                                   ([('seg64_table', stats([e[3] for e in kern['seg64']]))] if mixed else [])),
                    evals_per_s=dict(seg64=evals / (np.median(pre['seg64']) * 1e-3),
                                     group64=evals / (np.median(pre['group64']) * 1e-3),
                                     seg32=evals / (np.median(pre['seg32']) * 1e-3)),
                    shown=dict(wall_seg64_vs_group64=shown(wall['seg64'], wall['group64']),
                               kernels_seg64_vs_group64=shown(pre['seg64'], pre['group64']),
                               wall_seg64_vs_seg32=shown(wall['seg64'], wall['seg32']),
                               kernels_seg64_vs_seg32=shown(pre['seg64'], pre['seg32'])))
    line['gpu'] = torch.cuda.get_device_name(0)
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_branch_mq_fp64_time.jsonl' if mixed
                                   else 'joint_branch_fp64_time.jsonl')
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
    ap.add_argument('--fp64', action='store_true')
    ap.add_argument('--mixed', action='store_true')
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
    if args.mixed and not args.fp64:
        print('--mixed goes with --fp64', file=sys.stderr)
        return 2
    if args.mixed:
        words = [0xFFFFFFFE - 5 * s for s in range(8)]
        measure_fp64('mixed a: 64 ids over 8 groups of 3 + choice 4 + quniform 32', eng,
                     [make_mixed_group(n_a, SEED + s, 3, (4,), (32,)) for s in range(8)], words, np.arange(64) % 8,
                     np.arange(n_a, n_a + 64, dtype=np.int64), 4096, args, mixed=True)
        measure_fp64('mixed b: 1 id, quniform 50 x choice 2', eng, [make_mixed_group(n_b, SEED, 0, (2,), (50,))],
                     [0xFFFFFFFE], [0], [n_b], c_b, args, mixed=True)
        measure_fp64('mixed c: 1 id, 3 + quniform 256', eng, [make_mixed_group(n_b, SEED, 3, (), (256,))], [0xFFFFFFFE],
                     [0], [n_b], c_b, args, mixed=True)
        return 0
    models = [make_group(n_a, SEED + s) for s in range(8)]
    words = [0xFFFFFFFE - 5 * s for s in range(8)]
    prob_id = np.arange(n_a, n_a + 64, dtype=np.int64)
    prob_seg = np.arange(64) % 8                 # (every id its own branch: the groups interleave)
    if args.fp64:
        measure_fp64('a: 64 ids over 8 groups', eng, models, words, prob_seg, prob_id, 4096, args)
        measure_fp64('b: 1 id, 1 group', eng, [make_group(n_b, SEED)], [0xFFFFFFFE], [0], [n_b], c_b, args)
        measure_fp64('c: 1 id, 1 group, D = 16', eng, [make_wide_group(16, n_b, SEED)], [0xFFFFFFFE], [0], [n_b], c_b,
                     args)
        measure_fp64('clustered branch: 1 id, 1 group', eng, [make_clustered_group(n_a, SEED)], [0xFFFFFFFE], [0], [n_a],
                     c_b, args, time_it=False)
        return 0
    measure('a: 64 ids over 8 groups', eng, models, words, prob_seg, prob_id, 4096, args)
    measure('b: 1 id, 1 group', eng, [make_group(n_b, SEED)], [0xFFFFFFFE], [0], [n_b], c_b, args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
