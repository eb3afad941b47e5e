"""Time the mixed segmented joint stage against one tpe_joint_quant_run per
branch group.
Usage: python tools/joint_branch_mixed_time.py [--pairs 7] [--warmup 2] [--out FILE] [--small]

Workload (c) of DESIGN.md "Discrete and quantised labels in branch groups",
beside (a) and (b) of tools/joint_branch_time.py, with the same protocol: two
routes to the same winners, alternating in one process, each timed from a
synchronised device to the records on the host (wall clock), then the kernels
by their own events (tpe_joint_profile, tpe_joint_quant_profile).

  (c) 64 new ids over 8 branch groups of 2 continuous + 1 discrete (U = 3) + 1
      quantised (V = 50) labels (8 ids a group), 2,000 seeded trials a group,
      C = 4096 candidates:
        segmented  one Engine.run_joint_segments call: one upload, the order
                   kernel, one table launch for all groups and sides, one
                   k_joint_mseg_quant_chunk<2, 1, 1> launch of 256 workgroups,
                   one merge, one download
        per group  eight Engine.run_joint_quant calls, each with its group's 8
                   ids: an upload, two table launches, a chunk launch of 32
                   workgroups, a merge and a download per group (what the code
                   offers without the mixed segmented stage: the baseline)

The segmented call runs with each group's own stream word, the per-group route
with the root word, so the tool checks the bytes against per-group runs at the
group's word (untimed).  One JSON line goes to stdout and is appended to --out
(default profiles/joint_branch_mixed_time.jsonl).  --small: tiny sizes, to
rehearse the tool."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.joint_branch_time import SEED, stats  # noqa: E402

U, V = 3, 50


def make_group(n, seed):
    """A seeded group of n trials: x0 uniform, x1 normal, a category of U and a
    quniform(0, V - 1, 1) value, with a loss that couples them: the model tuple
    Engine.run_joint_segments and Engine.run_joint_quant take."""
    from hyperopt_amd import joint as J
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-5, 5, n), rs.normal(0, 2, n), np.rint(rs.uniform(0, V - 1.0, n))], axis=1)
    XC = rs.randint(U, size=n)
    loss = (X[:, 0] - 0.1 * X[:, 2]) ** 2 + 0.1 * X[:, 1] ** 2 + 0.5 * (XC != 1) + 0.01 * rs.standard_normal(n)
    nb = min(int(np.ceil(0.25 * np.sqrt(n))), 25)
    m = np.zeros(n, dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    priors = [(0.0, 10.0), (0.0, 2.0), (0.5 * (V - 1.0), V - 1.0)]
    sides = []
    for sel in (m, ~m):
        w, mu, sigma, xc = J.mixed_side_mixture(X[sel], priors, XC[sel])
        sides.append((w, mu[:, :2], sigma[:, :2], xc, mu[:, 2:], sigma[:, 2:]))
    b, a = sides
    p = np.full(U, 1.0 / U)
    cats = [(b[3][:, 0], a[3][:, 0], p, J.smoothing(1.0, U, int(m.sum())), J.smoothing(1.0, U, int((~m).sum())))]
    edges = J.quant_lattice('quniform', dict(low=0.0, high=V - 1.0, q=1.0))[3]
    quants = [(b[4][:, 0], b[5][:, 0], a[4][:, 0], a[5][:, 0], edges)]
    return b[:3], a[:3], np.array([-5.0, -np.inf]), np.array([5.0, np.inf]), cats, quants


def measure(name, eng, models, words, prob_seg, prob_id, C, args):
    import torch
    from hyperopt_amd import _native as N
    lib = eng.lib
    prob_seg, prob_id = np.asarray(prob_seg), np.asarray(prob_id, dtype=np.int64)
    groups = [(s, prob_id[prob_seg == s]) for s in range(len(models))]

    def segmented():
        return eng.run_joint_segments(models, words, prob_seg, prob_id, C, SEED)

    def per_group(word=False):
        return [eng.run_joint_quant(*models[s], ids, C, SEED, stream_word=words[s] if word else None)
                for s, ids in groups]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                     # (returns with the records on the host)
        return (time.perf_counter() - t0) * 1e3

    def kernel_ms(route):
        """Device times {the launches before the merge, the merge} summed over the route's calls."""
        ms2, tab = (ctypes.c_double * 2)(), ctypes.c_double(0)
        tot = [0.0, 0.0]
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        if route == 'segmented':
            segmented()
            N.check(lib.tpe_joint_profile(1, ms2), lib, 'tpe_joint_profile')
            tot = [ms2[0], ms2[1]]
        else:                                    # the per-group route: read after every call
            for s, ids in groups:
                eng.run_joint_quant(*models[s], ids, C, SEED)
                N.check(lib.tpe_joint_quant_profile(ctypes.byref(tab)), lib, 'tpe_joint_quant_profile')
                N.check(lib.tpe_joint_profile(1, ms2), lib, 'tpe_joint_profile')
                tot[0] += ms2[0] + tab.value
                tot[1] += ms2[1]
        N.check(lib.tpe_joint_profile(0, None), lib, 'tpe_joint_profile')
        return tot

    for _ in range(args.warmup):
        segmented()
        per_group()
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
        ks.append(kernel_ms('segmented'))
        kg.append(kernel_ms('per_group'))
    ks_dev, kg_dev = np.median([k[0] for k in ks]), np.median([k[0] for k in kg])
    line = dict(tool='joint_branch_mixed_time', workload=name, n_groups=len(models), n_problems=int(len(prob_seg)),
                n_dims=2, n_cat=1, n_quant=1, categories=U, lattice=V, n_cand=C,
                k_below=[len(m[0][0]) for m in models], k_above=[len(m[1][0]) for m in models],
                pairs=args.pairs, warmup=args.warmup,
                workgroups=dict(segmented_launch=int(len(prob_seg) * -(-C // N.JOINT_CHUNK)),
                                per_group_launch=[int(len(ids) * -(-C // N.JOINT_CHUNK)) for _, ids in groups]),
                wall_ms=dict(segmented=stats(ws), per_group=stats(wg),
                             ratio_of_medians=float(np.median(wg) / np.median(ws))),
                kernel_ms=dict(segmented_before_merge=stats([k[0] for k in ks]),
                               segmented_merge=stats([k[1] for k in ks]),
                               per_group_tables_and_chunk=stats([k[0] for k in kg]),
                               per_group_merge=stats([k[1] for k in kg]),
                               ratio_of_medians=float(kg_dev / ks_dev) if ks_dev > 0 else None),
                records_equal=True, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_branch_mixed_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--small', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print('joint_branch_mixed_time needs a GPU: nothing is measured without one', file=sys.stderr)
        return 2
    from hyperopt_amd.engine import get_engine
    eng = get_engine(None, 'fp32')
    n = 200 if args.small else 2000
    models = [make_group(n, SEED + s) for s in range(8)]
    words = [0xFFFFFFFE - 5 * s for s in range(8)]
    prob_id = np.arange(n, n + 64, dtype=np.int64)
    prob_seg = np.arange(64) % 8                 # (every id its own branch: the groups interleave)
    measure('c: 64 ids over 8 mixed groups', eng, models, words, prob_seg, prob_id, 4096, args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
