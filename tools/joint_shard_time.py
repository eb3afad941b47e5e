"""Time the per-rank slices of a candidate-sharded joint stage on ONE device.
Usage: python tools/joint_shard_time.py [--reps 5] [--warmup 1] [--cand 1048576] [--history 10000]
                                        [--ids 1,8] [--worlds 1,2,4,8] [--out FILE] [--exchange]

Nothing here is a multi-GPU measurement: one device runs, one after the other,
the slice that rank 0 and the slice that the last rank of a world of W ranks
would run (DESIGN.md "Sharded joint stage").  Workload: tools/joint_time.py's
(4 continuous labels, a seeded 10,000-trial history, C = 2^20 candidates), for
one new id and for 8.  Per (ids, world, rank) the slice
dist.shard_range(C, rank, world) goes through Engine.run_joint(shard=...):

  kernel_ms  k_joint_chunk's own event time (tpe_joint_profile)
  wall_ms    the whole engine call from a synchronised device to the records on
             the host (row packing, upload, launch, download), wall clock

each the median of --reps runs.  projected_speedup = T(world 1) / T(slice) is
what a rank of W would gain if the other ranks ran beside it at the same speed;
the exchange and everything replicated per rank are outside it.  replicated_ms
reports that replicated host part once: the model fit (joint.fit_model), the
numpy row packing (joint.density_rows twice, joint.sampler_rows) and the upload
of the packed rows.  One JSON line goes to stdout and is appended to --out
(default profiles/joint_shard_time.jsonl).

--exchange: the cost of the record exchange on one rank.  A one-rank nccl
process group on the device; tpe.suggest_choices(joint=True) on the same
workload, plain against joint_shard=(0, 1) with dist.EXCHANGE_ALWAYS (the
records go through the RCCL all-gather), alternating for --reps pairs, wall
clock; the line carries both medians, their spans and the difference."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from joint_time import SEED, make_history  # noqa: E402


def med(x):
    return float(np.median(x))


def write(line, out):
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')


def main_exchange(args):
    import socket
    import torch
    import torch.distributed as td
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(s.getsockname()[1])
    s.close()
    torch.cuda.set_device(0)
    td.init_process_group('nccl', rank=0, world_size=1)
    try:
        from hyperopt_amd import _native as N, dist as D, tpe
        from hyperopt_amd.engine import get_engine
        domain, hist = make_history(args.history)
        eng = get_engine(None, 'fp32')
        ids = [args.history]
        D.EXCHANGE_ALWAYS = True

        def run(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cc = tpe.suggest_choices(domain.table, hist, ids, SEED, n_EI_candidates=args.cand, joint=True,
                                     columns=True, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, cc
        for _ in range(max(args.warmup, 1)):
            run()
            run(joint_shard=(0, 1))
        n0 = N.collectives_issued(eng.lib)
        plain, sharded, same = [], [], True
        for _ in range(args.reps):
            a, ca = run()
            b, cb = run(joint_shard=(0, 1))
            plain.append(a)
            sharded.append(b)
            same = same and ca.values.tobytes() == cb.values.tobytes()
        issued = N.collectives_issued(eng.lib) - n0
        ex = D.exchange_for(eng)
        write(dict(tool='joint_shard_time --exchange', what='one nccl rank, dist.EXCHANGE_ALWAYS: not a multi-GPU figure',
                   history=args.history, n_cand=args.cand, pairs=args.reps, rccl=ex.comm is not None,
                   collectives_issued=issued, same_bytes=same,
                   plain_ms=dict(median=med(plain), min=min(plain), max=max(plain)),
                   joint_shard_0_1_ms=dict(median=med(sharded), min=min(sharded), max=max(sharded)),
                   exchange_ms=med(sharded) - med(plain), gpu=torch.cuda.get_device_name(0)), args.out)
        ex.close()
    finally:
        td.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cand', type=int, default=1 << 20)
    ap.add_argument('--history', type=int, default=10000)
    ap.add_argument('--ids', default='1,8')
    ap.add_argument('--worlds', default='1,2,4,8')
    ap.add_argument('--exchange', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_shard_time.jsonl'))
    args = ap.parse_args()
    if args.exchange:
        return main_exchange(args)

    import torch
    from hyperopt_amd import _native as N, dist as D, history as H, joint as J, joint_pack as JP
    from hyperopt_amd.engine import get_engine

    domain, hist = make_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # the part every rank repeats: fit, pack, upload
    fit_ms, pack_ms, up_ms = [], [], []
    for _ in range(max(args.reps, 1)):
        t, model = wall(lambda: J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0))
        fit_ms.append(t)

        def pack():                                  # what run_joint does before its uploads
            r = JP.group_rows(model.below, model.above, model.low, model.high, entry='run')
            return [r[row[0]] for row in JP.group_rows_present(r)]
        t, packed = wall(pack)
        pack_ms.append(t)
        t, _ = wall(lambda: [eng._joint_up('time_%d' % i, a, torch.float64 if a.dtype == np.float64 else torch.float32)
                             for i, a in enumerate(packed)])
        up_ms.append(t)

    ms2 = (ctypes.c_double * 2)()
    runs = []
    for n_ids in [int(x) for x in args.ids.split(',')]:
        ids = np.arange(args.history, args.history + n_ids, dtype=np.int64)
        base = {}
        for world in [int(x) for x in args.worlds.split(',')]:
            for rank in sorted(set([0, world - 1])):
                lo, hi = D.shard_range(C, rank, world)

                def call():
                    return eng.run_joint(model.below, model.above, model.low, model.high, ids, hi - lo, SEED,
                                         shard=(lo, C))
                for _ in range(args.warmup):
                    call()
                kern, walls = [], []
                for _ in range(args.reps):
                    N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
                    w, _ = wall(call)
                    N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
                    kern.append(ms2[0])
                    walls.append(w)
                r = dict(n_ids=n_ids, world=world, rank=rank, cand_base=lo, n_cand=hi - lo,
                         workgroups=n_ids * (-(-(hi - lo) // N.JOINT_CHUNK)),
                         kernel_ms=med(kern), kernel_ms_min=min(kern), kernel_ms_max=max(kern),
                         wall_ms=med(walls), wall_ms_min=min(walls), wall_ms_max=max(walls))
                if world == 1:
                    base = r
                r['projected_speedup_kernel'] = base['kernel_ms'] / r['kernel_ms'] if base and r['kernel_ms'] > 0 else None
                r['projected_speedup_wall'] = base['wall_ms'] / r['wall_ms'] if base and r['wall_ms'] > 0 else None
                print('ids %d world %d rank %d: kernel %.3f ms, call %.3f ms' % (n_ids, world, rank, r['kernel_ms'],
                                                                                 r['wall_ms']),
                      file=sys.stderr, flush=True)
                runs.append(r)
    write(dict(tool='joint_shard_time', what='slices of one device, one after the other: projections, not multi-GPU runs',
               labels=[r.label for r in rows], history=args.history, n_cand=C, n_dims=len(rows),
               k_below=len(model.below[0]), k_above=len(model.above[0]), reps=args.reps, runs=runs,
               replicated_ms=dict(fit=med(fit_ms), pack=med(pack_ms), upload=med(up_ms)),
               gpu=torch.cuda.get_device_name(0)), args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
