"""Time the joint TPE stage against the host route.
Usage: python tools/joint_time.py [--pairs 3] [--warmup 1] [--cand 1048576] [--history 10000]
                                  [--host-cand N] [--out FILE] [--mixed | --quant | --wide | --wide-mixed | --wide-quant | --liar |
                                   --liar-mixed | --liar-branches | --liar-branches-mixed]

Workload: a flat space of 4 continuous labels (uniform, loguniform, normal,
uniform), a seeded 10,000-trial history whose loss has an x0 * x1 term, one
new id, C = 2^20 candidate vectors: K_below = 26 and K_above = 9976 components
of 4 dimensions.  Two routes to the winner, alternating, each timed from a
synchronised device to its result on the host (wall clock):

  (a) host    Engine.run_joint(return_cand=True) — the candidates copied to the
              host — then the float64 numpy model (joint.lpdf_numpy) on both
              sides and np.argmax.  --host-cand N scores only the first N
              candidates on the host (the numpy model takes minutes for 2^20 x
              10^4 x 4); the line then carries the measured time for N and its
              linear extrapolation to C, labelled as such
  (b) device  Engine.run_joint() — tpe_joint_run, one 152-byte record copied

then (untimed) the device's l and g of the host-scored candidates against the
host's, plus the two joint kernels' own device times (tpe_joint_profile), the achieved
(candidate x component x dimension) evaluations per second and the fraction of
the VALU issue peak (256 CU x 4 SIMD x 2.4 GHz / 2 = 1228.8 G
wave-instructions/s) at the kernel's instruction count per
(candidate, component): 3 D + 7 lane-operations, D = 4.  One JSON line goes to
stdout and is appended to --out (default profiles/joint_time.jsonl).

--mixed: the mixed stage instead of the host route.  A second flat space of 3
continuous labels and one hp.choice of 4 (the same history size, the loss
couples x0 with the choice) runs through Engine.run_joint_mixed; each round is
one 4-continuous-label run, one 3 + 1 mixed run and one run over the mixed
space's 3 continuous labels alone (k_joint_chunk<3>: what the mixed kernel's
padded fourth continuous slot costs is read off against it), alternating in
one process, each timed by the chunk kernel's own events (tpe_joint_profile).
The line carries the three medians and the ratios mixed / continuous; --out defaults to
profiles/joint_mixed_time.jsonl.

--quant: the quantised stage (DESIGN.md "Quantised labels in the joint stage").
Three continuous labels with, per round, (a) one hp.quniform of 32 values
through Engine.run_joint_quant, (a256) the same with 256 values, (b) one
hp.choice of 32 through Engine.run_joint_mixed (k_joint_mixed_chunk<4, 1>: the
yardstick) and (c) the three continuous labels alone (k_joint_chunk<3>),
alternating in one process, each chunk kernel by its own events; the two table
launches of (a) and (a256) by theirs (tpe_joint_quant_profile).  The line
carries the medians and ranges, (a) / (b), (a) - (c), and the worst l / g error
of the first --host-cand (default 4096) sampled vectors of (a) as a fraction of
the lpdf tolerance; --out defaults to profiles/joint_quant_time.jsonl.

--wide: the wide stage (DESIGN.md "Wide groups").  Flat spaces of D labels of
hp.uniform(-5, 5) with the same history size; per round one run of
Engine.run_joint at D = 16 (k_joint_chunk<16>: the yardstick) and one of
Engine.run_joint_wide at each of D = 20, 32 and 64, alternating in one
process, the chunk kernels by their own events (tpe_joint_profile) and the
sampling kernel by its own (tpe_joint_wide_profile).  The line carries per run
the medians and ranges, the (candidate x component x dimension) evaluations per
second of the chunk kernel and their ratio to the yardstick's; the worst l / g
error of the first --host-cand (default 1024) sampled vectors at D = 64 as a
fraction of the lpdf tolerance; and the host route at D = 20: joint.lpdf_numpy on
both sides of those --host-cand vectors, measured and scaled linearly to C.
--out defaults to profiles/joint_wide_time.jsonl.

--wide-mixed: the wide mixed stage (DESIGN.md "Discrete labels in wide groups").
Flat spaces of Dc labels of hp.uniform(-5, 5) and Dk labels of hp.choice of 4,
the same history size.  Per round, alternating in one process: Engine.run_joint_wide
at D = 20 and Engine.run_joint_wide_mixed at 18 + 2; run_joint_wide at D = 32 and
run_joint_wide_mixed at 28 + 4 (the yardsticks: k_joint_wide_chunk at the same
number of coordinates); Engine.run_joint_mixed and run_joint_wide_mixed on one
8 + 4 group (the yardstick: k_joint_mixed_chunk<8, 4>).  Each chunk kernel by its
own events, the sampling kernels by theirs.  The line carries per run the
medians and ranges, the chunk kernel's time per (candidate x component x
coordinate) evaluation and its ratio to the yardstick's, and for the new stage
the worst l / g error of the first --host-cand (default 1024) sampled vectors as
a fraction of the lpdf tolerance.  --out defaults to
profiles/joint_wide_mixed_time.jsonl.

--wide-quant: the wide quantised stage (DESIGN.md "Quantised labels in wide
groups").  Flat spaces of Dc labels of hp.uniform(-5, 5), Dk labels of hp.choice
of 4 and Dq labels of hp.quniform (32 values the first, 8 the second), the same
history size.  Per round, alternating in one process: Engine.run_joint_wide_mixed
at 18 + 2 and Engine.run_joint_wide_quant at 17 + 2 + 1; run_joint_wide_mixed at
28 + 4 and run_joint_wide_quant at 26 + 4 + 2 (the yardsticks:
k_joint_wide_mixed_chunk at the same number of coordinates);
Engine.run_joint_quant and run_joint_wide_quant on one 8 + 4 + 2 group (the
yardstick: k_joint_quant_chunk<8, 4, 2>); and run_joint_wide_quant at 17 + 2 + 2
with two lattices of 256 values (512 in all: the shortest tile).  Each chunk
kernel by its own events, the sampling and table kernels by theirs.  The line
carries per run the medians and ranges, the chunk kernel's time per (candidate x
component x coordinate) evaluation and its ratio to the yardstick's, and for the
new stage the worst l / g error of the first --host-cand (default 1024) sampled
vectors as a fraction of the lpdf tolerance.  --out defaults to
profiles/joint_wide_quant_time.jsonl.

--liar: batch-aware joint suggests (DESIGN.md "Batch-aware joint suggests").  The
4-label workload above with --batch (default 64) new ids in one call; per round,
alternating in one process, Engine.run_joint without the keyword (the stage as
it was) and with liar=W, each timed from a synchronised device to its records
on the host (wall clock).  The line carries both medians and ranges, their
difference (what the keyword costs: the three per-candidate buffers the stage
now writes, and the 2 B + 1 launches of tpe_joint_liar), that difference per
step, and how far apart the B picks of either call lie: the median distance of a
pick to its nearest other pick, each coordinate in units of its prior sigma (every id
draws its own candidates, so the picks of the plain call differ in their bytes but sit
on one mode).  --out defaults to profiles/joint_liar_time.jsonl.

--liar-mixed: batch-aware picks over discrete and quantised labels.
The shape of --liar on a group of the 4 continuous labels, one hp.choice of 3 and
one hp.quniform of 32 values: Engine.run_joint_quant (the stage as it was) and
Engine.run_joint_liar_mixed with liar=W, alternating, wall clock from a synchronised
device to the records on the host.  The nearest-pick distance counts a
continuous or quantised coordinate in units of its prior sigma and a differing
category as 1.  --out defaults to profiles/joint_liar_mixed_time.jsonl.

--liar-branches: batch-aware picks in branch groups.  4 groups of the
4 continuous labels above, each fitted on its own quarter of --history trials,
--batch (default 64) new ids dealt round-robin over the groups, every group with
its own stream word.  Per round, alternating in one process, wall clock from a
synchronised device to the records on the host: (a) Engine.run_joint_segments
(no liar stage), (b) Engine.run_joint_segments_liar (one segmented liar stage:
2 launches a round of ALL chains), (c) one Engine.run_joint(liar=W_s) per group
(the only way without the segmented stage: 2 launches a step of EVERY chain, one
group after another).  (b) and (c) must agree byte for byte.  The line carries
the three medians and ranges, (b) - (a) per step of the longest chain, and the
median nearest-pick distance inside a branch (prior sigmas) with and without the
stage.  --out defaults to profiles/joint_liar_seg_time.jsonl.

--liar-branches-mixed: batch-aware picks in mixed branch groups.  The
shape of --liar-branches on 4 groups of 2 continuous labels, one hp.choice of 3 and
one hp.quniform of 32 values: (a) Engine.run_joint_segments, (b)
Engine.run_joint_msegments_liar, (c) one Engine.run_joint_liar_mixed(liar=W_s) per
group; (b) and (c) must agree byte for byte.  The nearest-pick distance is
--liar-mixed's, inside a branch.  --out defaults to
profiles/joint_liar_mseg_time.jsonl."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

VALU_PEAK = 1228.8e9          # wave-instructions per second
SEED = 20240607


def make_history(n, seed=SEED):
    from hyperopt_amd import base, history as H, hp
    space = {'x0': hp.uniform('x0', -5, 5), 'x1': hp.loguniform('x1', -3, 2), 'x2': hp.normal('x2', 0, 2),
             'x3': hp.uniform('x3', 0, 1)}
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(seed)
    cols = {'x0': rs.uniform(-5, 5, n), 'x1': np.exp(rs.uniform(-3, 2, n)), 'x2': rs.normal(0, 2, n),
            'x3': rs.uniform(0, 1, n)}
    loss = (cols['x0'] * cols['x1'] - 2.0) ** 2 + 0.1 * cols['x2'] ** 2 + (cols['x3'] - 0.3) ** 2 \
        + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    return domain, H.History(tids, loss, {k: (tids, v) for k, v in cols.items()})


def make_mixed_history(n):
    from hyperopt_amd import base, history as H, hp
    space = {'x0': hp.uniform('x0', -5, 5), 'x1': hp.loguniform('x1', -3, 2), 'x2': hp.normal('x2', 0, 2),
             'c3': hp.choice('c3', [0, 1, 2, 3])}
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(SEED)
    cols = {'x0': rs.uniform(-5, 5, n), 'x1': np.exp(rs.uniform(-3, 2, n)), 'x2': rs.normal(0, 2, n)}
    c3 = rs.randint(4, size=n).astype(np.int64)
    loss = (cols['x0'] - (2.0 * c3 - 3.0)) ** 2 + 0.1 * (np.log(cols['x1']) - 1.0) ** 2 + 0.1 * cols['x2'] ** 2 \
        + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    obs = {k: (tids, v) for k, v in cols.items()}
    obs['c3'] = (tids, c3)
    return domain, H.History(tids, loss, obs)


def main_mixed(args):
    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    domain, hist = make_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    cont = J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0)
    mdomain, mhist = make_mixed_history(args.history)
    mrows = [r for r in mdomain.table.rows if J.eligible(r)]
    drows = [r for r in mdomain.table.rows if J.eligible_discrete(r, mdomain.table)]
    mixed = J.fit_mixed_model(mrows, drows, mhist, H.split_below(mhist, 0.25), 1.0)
    cont3 = J.fit_model(mrows, mhist, H.split_below(mhist, 0.25), 1.0)
    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand
    ids = np.array([args.history], dtype=np.int64)

    def run_cont(**kw):
        return eng.run_joint(cont.below, cont.above, cont.low, cont.high, ids, C, SEED, **kw)

    def run_cont3(**kw):
        return eng.run_joint(cont3.below, cont3.above, cont3.low, cont3.high, ids, C, SEED, **kw)

    def run_mixed(**kw):
        return eng.run_joint_mixed(mixed.below[:3], mixed.above[:3], mixed.low, mixed.high, mixed.cats(), ids, C,
                                   SEED, **kw)

    def kernel_ms(fn):
        ms2 = (ctypes.c_double * 2)()
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        fn()
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        return ms2[0], ms2[1]

    for _ in range(args.warmup):
        run_cont()
        run_mixed()
        run_cont3()
    kc, km, k3 = [], [], []
    for i in range(args.pairs):
        kc.append(kernel_ms(run_cont))
        km.append(kernel_ms(run_mixed))
        k3.append(kernel_ms(run_cont3))
        print('round %d: continuous %.3f ms, mixed %.3f ms, 3 continuous %.3f ms' % (i, kc[-1][0], km[-1][0],
                                                                                   k3[-1][0]),
              file=sys.stderr, flush=True)
    # (untimed) the mixed stage's l and g of the first --host-cand candidates against the float64 model
    n_host = min(C, args.host_cand or 4096)
    _, cand, dl, dg = run_mixed(return_cand=True, want_lg=True)
    z, v = cand[0, :n_host, :len(mrows)].astype(np.float64), cand[0, :n_host, len(mrows):].astype(np.int64)
    err = 0.0
    for side, s, dev in ((mixed.below, mixed.s_below, dl), (mixed.above, mixed.s_above, dg)):
        ref = J.mixed_lpdf_numpy(z, v, side[0], side[1], side[2], mixed.low, mixed.high, side[3], mixed.ps, s)
        err = max(err, float(np.max(np.abs(dev[0, :n_host] - ref) / np.maximum(1.0, np.abs(ref)))) / 1e-5)
    med = lambda x: float(np.median(x))   # noqa: E731
    c1, m1, t1 = med([a for a, _ in kc]), med([a for a, _ in km]), med([a for a, _ in k3])
    line = dict(tool='joint_time --mixed', history=args.history, n_cand=C, pairs=args.pairs,
                continuous=dict(labels=[r.label for r in rows], n_dims=len(rows), k_below=len(cont.below[0]),
                                k_above=len(cont.above[0]), k_joint_chunk_ms=c1,
                                k_joint_chunk_ms_all=[a for a, _ in kc], k_joint_merge_ms=med([b for _, b in kc])),
                mixed=dict(labels=[r.label for r in mrows] + [r.label for r in drows], n_dims=len(mrows),
                           n_cat=len(drows), categories=[len(p) for p in mixed.ps], k_below=len(mixed.below[0]),
                           k_above=len(mixed.above[0]), k_joint_mixed_chunk_ms=m1,
                           k_joint_mixed_chunk_ms_all=[a for a, _ in km], k_joint_merge_ms=med([b for _, b in km]),
                           lpdf_err_over_tol=err, host_cand=n_host),
                continuous3=dict(labels=[r.label for r in mrows], n_dims=len(mrows), k_joint_chunk_ms=t1,
                                 k_joint_chunk_ms_all=[a for a, _ in k3]),
                ratio_mixed_over_continuous=m1 / c1 if c1 > 0 else None,
                ratio_mixed_over_continuous3=m1 / t1 if t1 > 0 else None, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_mixed_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def make_quant_history(n, V):
    """make_mixed_history's continuous columns with a quniform(0, V - 1, 1) label
    'q3' and a choice 'c3' of V options; the loss couples x0 with both."""
    from hyperopt_amd import base, history as H, hp
    space = {'x0': hp.uniform('x0', -5, 5), 'x1': hp.loguniform('x1', -3, 2), 'x2': hp.normal('x2', 0, 2),
             'q3': hp.quniform('q3', 0, V - 1, 1), 'c3': hp.choice('c3', list(range(V)))}
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(SEED)
    cols = {'x0': rs.uniform(-5, 5, n), 'x1': np.exp(rs.uniform(-3, 2, n)), 'x2': rs.normal(0, 2, n)}
    q3 = np.rint(rs.uniform(0, V - 1, n))
    c3 = rs.randint(V, size=n).astype(np.int64)
    loss = (cols['x0'] - (10.0 * q3 / (V - 1) - 5.0)) ** 2 + (cols['x0'] - (10.0 * c3 / (V - 1) - 5.0)) ** 2 \
        + 0.1 * (np.log(cols['x1']) - 1.0) ** 2 + 0.1 * cols['x2'] ** 2 + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    obs = {k: (tids, v) for k, v in cols.items()}
    obs['q3'] = (tids, q3)
    obs['c3'] = (tids, c3)
    return domain, H.History(tids, loss, obs)


def main_quant(args):
    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand
    ids = np.array([args.history], dtype=np.int64)
    models = {}
    for V in (32, 256):
        domain, hist = make_quant_history(args.history, V)
        t = domain.table
        crows = [r for r in t.rows if J.eligible(r)]
        below = H.split_below(hist, 0.25)
        models[V] = J.fit_quant_model(crows, [], [t.by_label['q3']], hist, below, 1.0)
        if V == 32:
            mixed = J.fit_mixed_model(crows, [t.by_label['c3']], hist, below, 1.0)
            cont3 = J.fit_model(crows, hist, below, 1.0)

    def run_quant(V, **kw):
        m = models[V]
        return eng.run_joint_quant(m.below[:3], m.above[:3], m.low, m.high, [], m.quants(), ids, C, SEED, **kw)

    def run_mixed(**kw):
        return eng.run_joint_mixed(mixed.below[:3], mixed.above[:3], mixed.low, mixed.high, mixed.cats(), ids, C,
                                   SEED, **kw)

    def run_cont3(**kw):
        return eng.run_joint(cont3.below, cont3.above, cont3.low, cont3.high, ids, C, SEED, **kw)

    def kernel_ms(fn, table=False):
        ms2, tms = (ctypes.c_double * 2)(), ctypes.c_double(0.0)
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        fn()
        if table:
            N.check(lib.tpe_joint_quant_profile(ctypes.byref(tms)), lib, 'tpe_joint_quant_profile')
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        return ms2[0], ms2[1], tms.value

    routes = [('quant32', lambda: run_quant(32), True), ('quant256', lambda: run_quant(256), True),
              ('mixed32', run_mixed, False), ('continuous3', run_cont3, False)]
    for _ in range(args.warmup):
        for _, fn, _ in routes:
            fn()
    ms = dict((name, []) for name, _, _ in routes)
    for i in range(args.pairs):
        for name, fn, table in routes:
            ms[name].append(kernel_ms(fn, table))
        print('round %d: %s' % (i, ', '.join('%s %.3f ms' % (name, ms[name][-1][0]) for name, _, _ in routes)),
              file=sys.stderr, flush=True)
    # (untimed) the stage's l and g of the first --host-cand sampled vectors against the float64 model
    n_host = min(C, args.host_cand or 4096)
    m = models[32]
    _, cand, dl, dg = run_quant(32, return_cand=True, want_lg=True)
    z, qi = cand[0, :n_host, :3].astype(np.float64), cand[0, :n_host, 3:].astype(np.int64)
    err = 0.0
    for side, dev in ((m.below, dl), (m.above, dg)):
        ref = J.quant_lpdf_numpy(z, np.zeros((n_host, 0)), qi, side[0], side[1], side[2], m.low, m.high, side[3], [], [],
                                 [(side[4][:, 0], side[5][:, 0], m.lattices[0][3])])
        err = max(err, float(np.max(np.abs(dev[0, :n_host] - ref) / np.maximum(1.0, np.abs(ref)))) / 1e-5)

    def stat(name, j=0):
        x = [r[j] for r in ms[name]]
        return dict(median=float(np.median(x)), min=min(x), max=max(x), all=x)
    a, b, c = stat('quant32')['median'], stat('mixed32')['median'], stat('continuous3')['median']
    line = dict(tool='joint_time --quant', history=args.history, n_cand=C, rounds=args.pairs,
                k_below=len(m.below[0]), k_above=len(m.above[0]),
                a_quant32=dict(kernel='k_joint_quant_chunk<4, 0, 1>', chunk_ms=stat('quant32'),
                               table_ms=stat('quant32', 2), merge_ms=stat('quant32', 1)['median']),
                a_quant256=dict(kernel='k_joint_quant_chunk<4, 0, 1>', chunk_ms=stat('quant256'),
                                table_ms=stat('quant256', 2)),
                b_mixed32=dict(kernel='k_joint_mixed_chunk<4, 1>', chunk_ms=stat('mixed32')),
                c_continuous3=dict(kernel='k_joint_chunk<3>', chunk_ms=stat('continuous3')),
                ratio_a_over_b=a / b if b > 0 else None, a_minus_c_ms=a - c,
                ratio_a256_over_b=stat('quant256')['median'] / b if b > 0 else None,
                lpdf_err_over_tol=err, host_cand=n_host, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_quant_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def make_flat_history(n, D):
    """D labels of hp.uniform(-5, 5) (bench.py config 4's space at D = 20), a
    seeded history whose loss is a shifted bowl with one product term."""
    from hyperopt_amd import base, history as H, hp
    labels = ['x%02d' % i for i in range(D)]
    domain = base.Domain(lambda d: 0.0, {k: hp.uniform(k, -5, 5) for k in labels})
    rs = np.random.RandomState(SEED + D)
    X = rs.uniform(-5, 5, (n, D))
    loss = ((X - np.linspace(-2, 2, D)[None, :]) ** 2).sum(axis=1) + X[:, 0] * X[:, 1] + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    return domain, H.History(tids, loss, {k: (tids, X[:, i]) for i, k in enumerate(labels)})


def main_wide(args):
    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand
    ids = np.array([args.history], dtype=np.int64)
    dims = (16, 20, 32, 64)
    models = {}
    for D in dims:
        domain, hist = make_flat_history(args.history, D)
        models[D] = J.fit_model(list(domain.table.rows), hist, H.split_below(hist, 0.25), 1.0)

    def run(D, **kw):
        m = models[D]
        fn = eng.run_joint if D <= N.JOINT_MAX_DIMS else eng.run_joint_wide
        return fn(m.below, m.above, m.low, m.high, ids, C, SEED, **kw)

    def kernel_ms(D):
        ms2, sms = (ctypes.c_double * 2)(), ctypes.c_double(0.0)
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        run(D)
        if D > N.JOINT_MAX_DIMS:
            N.check(lib.tpe_joint_wide_profile(ctypes.byref(sms)), lib, 'tpe_joint_wide_profile')
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        return ms2[0], ms2[1], sms.value

    for _ in range(args.warmup):
        for D in dims:
            run(D)
    ms = dict((D, []) for D in dims)
    for i in range(args.pairs):
        for D in dims:
            ms[D].append(kernel_ms(D))
        print('round %d: %s' % (i, ', '.join('D=%d %.3f ms' % (D, ms[D][-1][0]) for D in dims)), file=sys.stderr,
              flush=True)

    # (untimed) l and g of the first --host-cand sampled vectors against the float64 model, at D = 64
    # and D = 20; the D = 20 evaluation is also the host route's measured time
    n_host = min(C, args.host_cand or 1024)
    err, host_ms = {}, None
    for D in (64, 20):
        m = models[D]
        _, cand, dl, dg = run(D, return_cand=True, want_lg=True)
        z = cand[0, :n_host].astype(np.float64)
        t0 = time.perf_counter()
        refs = [J.lpdf_numpy(z, side[0], side[1], side[2], m.low, m.high) for side in (m.below, m.above)]
        if D == 20:
            host_ms = (time.perf_counter() - t0) * 1e3
        err[D] = max(float(np.max(np.abs(dev[0, :n_host] - ref) / np.maximum(1.0, np.abs(ref))))
                     for dev, ref in zip((dl, dg), refs)) / 1e-5

    def stat(D, j=0):
        x = [r[j] for r in ms[D]]
        return dict(median=float(np.median(x)), min=min(x), max=max(x), all=x)

    def rate(D):
        m = models[D]
        k = stat(D)['median']
        return float(C) * (len(m.below[0]) + len(m.above[0])) * D / (k * 1e-3) if k > 0 else None
    yard = rate(16)
    runs = {}
    for D in dims:
        m = models[D]
        wide = D > N.JOINT_MAX_DIMS
        dp = D if not wide else (20 if D <= 20 else 24 if D <= 24 else 32 if D <= 32 else 48 if D <= 48 else 64)
        runs['D%d' % D] = dict(
            kernel='k_joint_wide_chunk<%d, %d>' % (dp, 2 if dp <= 32 else 1) if wide else 'k_joint_chunk<16>',
            n_dims=D, k_below=len(m.below[0]), k_above=len(m.above[0]), chunk_ms=stat(D),
            merge_ms=stat(D, 1)['median'], sample_ms=stat(D, 2) if wide else None,
            evals_per_s=rate(D), ratio_to_yardstick=rate(D) / yard if yard else None)
    line = dict(tool='joint_time --wide', history=args.history, n_cand=C, rounds=args.pairs, runs=runs,
                lpdf_err_over_tol_D64=err[64], lpdf_err_over_tol_D20=err[20], host_cand=n_host,
                host_route_D20_ms=dict(measured_for_host_cand=host_ms, scaled_to_all_candidates=host_ms * C / n_host),
                gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_wide_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def make_flat_mixed_history(n, Dc, Dk):
    """make_flat_history's Dc continuous labels with Dk labels of hp.choice of 4;
    the loss also couples x00 with the first choice."""
    from hyperopt_amd import base, history as H, hp
    labels = ['x%02d' % i for i in range(Dc)]
    clabels = ['c%02d' % i for i in range(Dk)]
    space = {k: hp.uniform(k, -5, 5) for k in labels}
    space.update({k: hp.choice(k, [0, 1, 2, 3]) for k in clabels})
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(SEED + 100 * Dc + Dk)
    X = rs.uniform(-5, 5, (n, Dc))
    XC = rs.randint(4, size=(n, Dk)).astype(np.int64)
    loss = ((X - np.linspace(-2, 2, Dc)[None, :]) ** 2).sum(axis=1) + X[:, 0] * X[:, 1] \
        + (X[:, 0] - (2.0 * XC[:, 0] - 3.0)) ** 2 + 0.1 * XC[:, 1:].sum(axis=1) + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    obs = {k: (tids, X[:, i]) for i, k in enumerate(labels)}
    obs.update({k: (tids, XC[:, i]) for i, k in enumerate(clabels)})
    return domain, H.History(tids, loss, obs)


def main_wide_mixed(args):
    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand
    ids = np.array([args.history], dtype=np.int64)
    wide, mixed = {}, {}
    for D in (20, 32):
        domain, hist = make_flat_history(args.history, D)
        wide[D] = J.fit_model(list(domain.table.rows), hist, H.split_below(hist, 0.25), 1.0)
    for Dc, Dk in ((18, 2), (28, 4), (8, 4)):
        domain, hist = make_flat_mixed_history(args.history, Dc, Dk)
        t = domain.table
        crows = [r for r in t.rows if J.eligible(r)]
        drows = [r for r in t.rows if J.eligible_discrete(r, t)]
        assert (len(crows), len(drows)) == (Dc, Dk)
        mixed[Dc, Dk] = J.fit_mixed_model(crows, drows, hist, H.split_below(hist, 0.25), 1.0)

    def run_wide(D, **kw):
        m = wide[D]
        return eng.run_joint_wide(m.below, m.above, m.low, m.high, ids, C, SEED, **kw)

    def run_mixed(key, narrow=False, **kw):
        m = mixed[key]
        fn = eng.run_joint_mixed if narrow else eng.run_joint_wide_mixed
        return fn(m.below[:3], m.above[:3], m.low, m.high, m.cats(), ids, C, SEED, **kw)

    # (name, the call, whether a sampling kernel of its own runs, coordinates, the model, the kernel, its yardstick)
    routes = [
        ('wide20', lambda **kw: run_wide(20, **kw), True, 20, wide[20], 'k_joint_wide_chunk<20, 2>', None),
        ('wide_mixed_18_2', lambda **kw: run_mixed((18, 2), **kw), True, 20, mixed[18, 2],
         'k_joint_wide_mixed_chunk<20, 2, 2>', 'wide20'),
        ('wide32', lambda **kw: run_wide(32, **kw), True, 32, wide[32], 'k_joint_wide_chunk<32, 2>', None),
        ('wide_mixed_28_4', lambda **kw: run_mixed((28, 4), **kw), True, 32, mixed[28, 4],
         'k_joint_wide_mixed_chunk<32, 4, 2>', 'wide32'),
        ('mixed_8_4', lambda **kw: run_mixed((8, 4), narrow=True, **kw), False, 12, mixed[8, 4],
         'k_joint_mixed_chunk<8, 4>', None),
        ('wide_mixed_8_4', lambda **kw: run_mixed((8, 4), **kw), True, 12, mixed[8, 4],
         'k_joint_wide_mixed_chunk<12, 4, 2>', 'mixed_8_4'),
    ]

    def kernel_ms(fn, sampled):
        ms2, sms = (ctypes.c_double * 2)(), ctypes.c_double(0.0)
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        fn()
        if sampled:
            N.check(lib.tpe_joint_wide_profile(ctypes.byref(sms)), lib, 'tpe_joint_wide_profile')
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        return ms2[0], ms2[1], sms.value

    for _ in range(args.warmup):
        for r in routes:
            r[1]()
    ms = dict((r[0], []) for r in routes)
    for i in range(args.pairs):
        for r in routes:
            ms[r[0]].append(kernel_ms(r[1], r[2]))
        print('round %d: %s' % (i, ', '.join('%s %.3f ms' % (r[0], ms[r[0]][-1][0]) for r in routes)), file=sys.stderr,
              flush=True)

    # (untimed) l and g of the first --host-cand sampled vectors of the new stage against the float64 model
    n_host = min(C, args.host_cand or 1024)
    err = {}
    for r in routes:
        if not r[0].startswith('wide_mixed'):
            continue
        m = r[4]
        Dc = len(m.rows)
        _, cand, dl, dg = r[1](return_cand=True, want_lg=True)
        z, v = cand[0, :n_host, :Dc].astype(np.float64), cand[0, :n_host, Dc:].astype(np.int64)
        e = 0.0
        for side, s, dev in ((m.below, m.s_below, dl), (m.above, m.s_above, dg)):
            ref = J.mixed_lpdf_numpy(z, v, side[0], side[1], side[2], m.low, m.high, side[3], m.ps, s)
            e = max(e, float(np.max(np.abs(dev[0, :n_host] - ref) / np.maximum(1.0, np.abs(ref)))) / 1e-5)
        err[r[0]] = e

    def stat(name, j=0):
        x = [q[j] for q in ms[name]]
        return dict(median=float(np.median(x)), min=min(x), max=max(x), all=x)

    def per_eval_ps(r):
        """picoseconds of chunk-kernel time per (candidate x component x coordinate) evaluation"""
        m = r[4]
        return stat(r[0])['median'] * 1e9 / (float(C) * (len(m.below[0]) + len(m.above[0])) * r[3])
    by_name = dict((r[0], r) for r in routes)
    runs = {}
    for r in routes:
        m = r[4]
        yard = by_name.get(r[6])
        runs[r[0]] = dict(kernel=r[5], coordinates=r[3], n_cat=len(getattr(m, 'drows', ())),
                          k_below=len(m.below[0]), k_above=len(m.above[0]), chunk_ms=stat(r[0]),
                          merge_ms=stat(r[0], 1)['median'], sample_ms=stat(r[0], 2) if r[2] else None,
                          ps_per_eval=per_eval_ps(r), yardstick=r[6],
                          ratio_to_yardstick=per_eval_ps(r) / per_eval_ps(yard) if yard else None,
                          lpdf_err_over_tol=err.get(r[0]))
    line = dict(tool='joint_time --wide-mixed', history=args.history, n_cand=C, rounds=args.pairs, runs=runs,
                host_cand=n_host, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_wide_mixed_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def make_flat_quant_history(n, Dc, Dk, Vs):
    """make_flat_mixed_history's labels with one hp.quniform(0, V - 1, 1) per entry
    of ``Vs``; the loss also couples x00 with the first quantised label."""
    from hyperopt_amd import base, history as H, hp
    labels = ['x%02d' % i for i in range(Dc)]
    clabels = ['c%02d' % i for i in range(Dk)]
    qlabels = ['q%02d' % i for i in range(len(Vs))]
    space = {k: hp.uniform(k, -5, 5) for k in labels}
    space.update({k: hp.choice(k, [0, 1, 2, 3]) for k in clabels})
    space.update({k: hp.quniform(k, 0, V - 1, 1) for k, V in zip(qlabels, Vs)})
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(SEED + 10000 * len(Vs) + 100 * Dc + Dk)
    X = rs.uniform(-5, 5, (n, Dc))
    XC = rs.randint(4, size=(n, Dk)).astype(np.int64)
    XQ = np.stack([np.rint(rs.uniform(0, V - 1, n)) for V in Vs], axis=1)
    loss = ((X - np.linspace(-2, 2, Dc)[None, :]) ** 2).sum(axis=1) + X[:, 0] * X[:, 1] \
        + (X[:, 0] - (10.0 * XQ[:, 0] / (Vs[0] - 1) - 5.0)) ** 2 + 0.1 * XC.sum(axis=1) \
        + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    obs = {k: (tids, X[:, i]) for i, k in enumerate(labels)}
    obs.update({k: (tids, XC[:, i]) for i, k in enumerate(clabels)})
    obs.update({k: (tids, XQ[:, i]) for i, k in enumerate(qlabels)})
    return domain, H.History(tids, loss, obs)


def main_wide_quant(args):
    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C = args.cand
    ids = np.array([args.history], dtype=np.int64)
    mixed, quant = {}, {}
    for Dc, Dk in ((18, 2), (28, 4)):
        domain, hist = make_flat_mixed_history(args.history, Dc, Dk)
        t = domain.table
        crows = [r for r in t.rows if J.eligible(r)]
        drows = [r for r in t.rows if J.eligible_discrete(r, t)]
        mixed[Dc, Dk] = J.fit_mixed_model(crows, drows, hist, H.split_below(hist, 0.25), 1.0)
    for Dc, Dk, Vs in ((17, 2, (32,)), (26, 4, (32, 8)), (8, 4, (32, 8)), (17, 2, (256, 256))):
        domain, hist = make_flat_quant_history(args.history, Dc, Dk, Vs)
        t = domain.table
        crows = [r for r in t.rows if J.eligible(r)]
        drows = [r for r in t.rows if J.eligible_discrete(r, t)]
        qrows = [r for r in t.rows if J.eligible_quant(r, t)]
        assert (len(crows), len(drows), len(qrows)) == (Dc, Dk, len(Vs))
        quant[Dc, Dk, Vs] = J.fit_quant_model(crows, drows, qrows, hist, H.split_below(hist, 0.25), 1.0)

    def run_mixed(key, **kw):
        m = mixed[key]
        return eng.run_joint_wide_mixed(m.below[:3], m.above[:3], m.low, m.high, m.cats(), ids, C, SEED, **kw)

    def run_quant(key, narrow=False, **kw):
        m = quant[key]
        fn = eng.run_joint_quant if narrow else eng.run_joint_wide_quant
        return fn(m.below[:3], m.above[:3], m.low, m.high, m.cats(), m.quants(), ids, C, SEED, **kw)

    # (name, the call, sampling kernel of its own, table kernels, coordinates, the model, the kernel, its yardstick)
    routes = [
        ('wide_mixed_18_2', lambda **kw: run_mixed((18, 2), **kw), True, False, 20, mixed[18, 2],
         'k_joint_wide_mixed_chunk<20, 2, 2>', None),
        ('wide_quant_17_2_1', lambda **kw: run_quant((17, 2, (32,)), **kw), True, True, 20, quant[17, 2, (32,)],
         'k_joint_wide_quant_chunk<24, 2, 1, 2>', 'wide_mixed_18_2'),
        ('wide_mixed_28_4', lambda **kw: run_mixed((28, 4), **kw), True, False, 32, mixed[28, 4],
         'k_joint_wide_mixed_chunk<32, 4, 2>', None),
        ('wide_quant_26_4_2', lambda **kw: run_quant((26, 4, (32, 8)), **kw), True, True, 32, quant[26, 4, (32, 8)],
         'k_joint_wide_quant_chunk<32, 8, 2, 2>', 'wide_mixed_28_4'),
        ('quant_8_4_2', lambda **kw: run_quant((8, 4, (32, 8)), narrow=True, **kw), False, True, 14,
         quant[8, 4, (32, 8)], 'k_joint_quant_chunk<8, 4, 2>', None),
        ('wide_quant_8_4_2', lambda **kw: run_quant((8, 4, (32, 8)), **kw), True, True, 14, quant[8, 4, (32, 8)],
         'k_joint_wide_quant_chunk<16, 8, 2, 2>', 'quant_8_4_2'),
        ('wide_quant_17_2_2_v512', lambda **kw: run_quant((17, 2, (256, 256)), **kw), True, True, 21,
         quant[17, 2, (256, 256)], 'k_joint_wide_quant_chunk<24, 2, 2, 2>', 'wide_mixed_18_2'),
    ]

    def kernel_ms(r):
        ms2, sms, tms = (ctypes.c_double * 2)(), ctypes.c_double(0.0), ctypes.c_double(0.0)
        torch.cuda.synchronize()
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        r[1]()
        if r[2]:
            prof = 'tpe_joint_wide_quant_profile' if r[0].startswith('wide_quant') else 'tpe_joint_wide_profile'
            N.check(getattr(lib, prof)(ctypes.byref(sms)), lib, prof)
        if r[3]:
            N.check(lib.tpe_joint_quant_profile(ctypes.byref(tms)), lib, 'tpe_joint_quant_profile')
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        return ms2[0], ms2[1], sms.value, tms.value

    for _ in range(args.warmup):
        for r in routes:
            r[1]()
    ms = dict((r[0], []) for r in routes)
    for i in range(args.pairs):
        for r in routes:
            ms[r[0]].append(kernel_ms(r))
        print('round %d: %s' % (i, ', '.join('%s %.3f ms' % (r[0], ms[r[0]][-1][0]) for r in routes)), file=sys.stderr,
              flush=True)

    # (untimed) l and g of the first --host-cand sampled vectors of the new stage against the float64 model
    n_host = min(C, args.host_cand or 1024)
    err = {}
    for r in routes:
        if not r[0].startswith('wide_quant'):
            continue
        m = r[5]
        Dc, Dk = len(m.rows), len(m.drows)
        _, cand, dl, dg = r[1](return_cand=True, want_lg=True)
        z, v = cand[0, :n_host, :Dc].astype(np.float64), cand[0, :n_host, Dc:Dc + Dk].astype(np.int64)
        qi = cand[0, :n_host, Dc + Dk:].astype(np.int64)
        e = 0.0
        for side, s, dev in ((m.below, m.s_below, dl), (m.above, m.s_above, dg)):
            qs = [(side[4][:, d], side[5][:, d], lat[3]) for d, lat in enumerate(m.lattices)]
            ref = J.quant_lpdf_numpy(z, v, qi, side[0], side[1], side[2], m.low, m.high, side[3], m.ps, s, qs)
            e = max(e, float(np.max(np.abs(dev[0, :n_host] - ref) / np.maximum(1.0, np.abs(ref)))) / 1e-5)
        err[r[0]] = e

    def stat(name, j=0):
        x = [q[j] for q in ms[name]]
        return dict(median=float(np.median(x)), min=min(x), max=max(x), all=x)

    def per_eval_ps(r):
        """picoseconds of chunk-kernel time per (candidate x component x coordinate) evaluation"""
        m = r[5]
        return stat(r[0])['median'] * 1e9 / (float(C) * (len(m.below[0]) + len(m.above[0])) * r[4])
    by_name = dict((r[0], r) for r in routes)
    runs = {}
    for r in routes:
        m = r[5]
        yard = by_name.get(r[7])
        runs[r[0]] = dict(kernel=r[6], coordinates=r[4], n_cat=len(m.drows), n_quant=len(getattr(m, 'qrows', ())),
                          lattice_values=[lat[1] for lat in getattr(m, 'lattices', ())],
                          k_below=len(m.below[0]), k_above=len(m.above[0]), chunk_ms=stat(r[0]),
                          merge_ms=stat(r[0], 1)['median'], sample_ms=stat(r[0], 2) if r[2] else None,
                          table_ms=stat(r[0], 3) if r[3] else None, ps_per_eval=per_eval_ps(r), yardstick=r[7],
                          ratio_to_yardstick=per_eval_ps(r) / per_eval_ps(yard) if yard else None,
                          lpdf_err_over_tol=err.get(r[0]))
    line = dict(tool='joint_time --wide-quant', history=args.history, n_cand=C, rounds=args.pairs, runs=runs,
                host_cand=n_host, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_wide_quant_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def main_liar(args):
    import torch
    from hyperopt_amd import history as H, joint as J
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF

    domain, hist = make_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    model = J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0)
    eng = get_engine(None, 'fp32')
    C, D, B = args.cand, len(rows), args.batch
    Kb, Ka = len(model.below[0]), len(model.above[0])
    W = J.side_weight_sum(Ka - 1, 1.0, DEFAULT_LF)
    ids = np.arange(args.history, args.history + B, dtype=np.int64)

    def run(liar):
        return eng.run_joint(model.below, model.above, model.low, model.high, ids, C, SEED, liar=liar)

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        run(False)
        run(W)
    wall = {'plain': [], 'liar': []}
    for i in range(args.pairs):
        w, plain = timed(run, False)
        wall['plain'].append(w)
        w, liar = timed(run, W)
        wall['liar'].append(w)
        print('pair %d: plain %.2f ms, liar %.2f ms' % (i, wall['plain'][-1], w), file=sys.stderr, flush=True)
    assert liar[:1].tobytes() == plain[:1].tobytes()
    med = lambda x: float(np.median(x))   # noqa: E731

    def spread(rec):
        z = rec['z'][:, :D] / np.asarray(model.above[2])[0][None, :]
        d = np.sqrt(((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2))
        np.fill_diagonal(d, np.inf)
        return float(np.median(d.min(axis=1)))
    extra = med(wall['liar']) - med(wall['plain'])
    line = dict(tool='joint_time --liar', labels=[r.label for r in rows], history=args.history, n_cand=C, n_dims=D,
                k_below=Kb, k_above=Ka, batch=B, pairs=args.pairs, w_sum=W,
                plain_ms=dict(wall_median=med(wall['plain']), wall_min=min(wall['plain']), wall_max=max(wall['plain'])),
                liar_ms=dict(wall_median=med(wall['liar']), wall_min=min(wall['liar']), wall_max=max(wall['liar'])),
                liar_minus_plain_ms=extra, per_step_ms=extra / B, ratio=med(wall['liar']) / med(wall['plain']),
                nearest_pick_median=dict(plain=spread(plain), liar=spread(liar)), gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_liar_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def make_liar_mixed_history(n):
    from hyperopt_amd import base, history as H, hp
    space = {'x0': hp.uniform('x0', -5, 5), 'x1': hp.loguniform('x1', -3, 2), 'x2': hp.normal('x2', 0, 2),
             'x3': hp.uniform('x3', 0, 1), 'c4': hp.choice('c4', [0, 1, 2]), 'q5': hp.quniform('q5', 1, 32, 1)}
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(SEED)
    cols = {'x0': rs.uniform(-5, 5, n), 'x1': np.exp(rs.uniform(-3, 2, n)), 'x2': rs.normal(0, 2, n),
            'x3': rs.uniform(0, 1, n), 'c4': rs.randint(3, size=n), 'q5': np.rint(rs.uniform(1, 32, n))}
    loss = (cols['x0'] * cols['x1'] - 2.0) ** 2 + 0.1 * cols['x2'] ** 2 + (cols['x3'] - 0.3) ** 2 \
        + 0.2 * (cols['c4'] != 1) + 1e-3 * (cols['q5'] - 12.0) ** 2 + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    return domain, H.History(tids, loss, {k: (tids, v) for k, v in cols.items()})


def main_liar_mixed(args):
    import torch
    from hyperopt_amd import history as H, joint as J
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF

    domain, hist = make_liar_mixed_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    drows = [r for r in domain.table.rows if J.eligible_discrete(r, domain.table)]
    qrows = [r for r in domain.table.rows if J.eligible_quant(r, domain.table)]
    model = J.fit_quant_model(rows, drows, qrows, hist, H.split_below(hist, 0.25), 1.0)
    eng = get_engine(None, 'fp32')
    C, B = args.cand, args.batch
    Dc, Dk, Dq = len(rows), len(drows), len(qrows)
    Kb, Ka = len(model.below[0]), len(model.above[0])
    W = J.side_weight_sum(Ka - 1, 1.0, DEFAULT_LF)
    ids = np.arange(args.history, args.history + B, dtype=np.int64)
    cats, quants, centres = model.cats(), model.quants(), model.centres()

    def run(liar):
        head = (model.below[:3], model.above[:3], model.low, model.high, cats, quants, ids, C, SEED)
        return eng.run_joint_liar_mixed(*head, liar=W, centres=centres) if liar else eng.run_joint_quant(*head)

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        run(False)
        run(True)
    wall = {'plain': [], 'liar': []}
    for i in range(args.pairs):
        w, plain = timed(run, False)
        wall['plain'].append(w)
        w, liar = timed(run, True)
        wall['liar'].append(w)
        print('pair %d: plain %.2f ms, liar %.2f ms' % (i, wall['plain'][-1], w), file=sys.stderr, flush=True)
    assert liar[:1].tobytes() == plain[:1].tobytes()
    med = lambda x: float(np.median(x))   # noqa: E731

    def spread(rec):
        z = rec['z'][:, :Dc] / np.asarray(model.above[2])[0][None, :]
        q = np.stack([centres[d][rec['z'][:, Dc + Dk + d].astype(np.int64)] / model.above[5][0, d] for d in range(Dq)],
                     axis=1)
        z = np.hstack([z, q])
        d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2)
        v = rec['z'][:, Dc:Dc + Dk]
        d2 = d2 + (v[:, None, :] != v[None, :, :]).sum(axis=2)
        d = np.sqrt(d2)
        np.fill_diagonal(d, np.inf)
        return float(np.median(d.min(axis=1)))
    extra = med(wall['liar']) - med(wall['plain'])
    line = dict(tool='joint_time --liar-mixed', labels=[r.label for r in rows + drows + qrows], history=args.history,
                n_cand=C, n_dims=Dc, n_cat=Dk, n_quant=Dq, lattice=[lat[1] for lat in model.lattices],
                k_below=Kb, k_above=Ka, batch=B, pairs=args.pairs, w_sum=W,
                plain_ms=dict(wall_median=med(wall['plain']), wall_min=min(wall['plain']), wall_max=max(wall['plain'])),
                liar_ms=dict(wall_median=med(wall['liar']), wall_min=min(wall['liar']), wall_max=max(wall['liar'])),
                liar_minus_plain_ms=extra, per_step_ms=extra / B, ratio=med(wall['liar']) / med(wall['plain']),
                nearest_pick_median=dict(plain=spread(plain), liar=spread(liar)), gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    out = args.out or os.path.join(ROOT, 'profiles', 'joint_liar_mixed_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'a') as f:
        f.write(text + '\n')
    return 0


def main_liar_branches(args):
    import torch
    from hyperopt_amd import history as H, joint as J
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF

    S = 4
    models = []
    for s in range(S):
        domain, hist = make_history(args.history // S, SEED + s)
        rows = [r for r in domain.table.rows if J.eligible(r)]
        models.append(J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0))
    eng = get_engine(None, 'fp32')
    C, D, B = args.cand, len(rows), args.batch
    W = [J.side_weight_sum(len(m.above[0]) - 1, 1.0, DEFAULT_LF) for m in models]
    words = [0x51000 + s for s in range(S)]
    prob_seg = (np.arange(B) % S).astype(np.int32)
    prob_id = np.arange(args.history, args.history + B, dtype=np.int64)
    chains = [np.flatnonzero(prob_seg == s) for s in range(S)]

    def seg():
        return eng.run_joint_segments(models, words, prob_seg, prob_id, C, SEED)

    def seg_liar():
        return eng.run_joint_segments_liar(models, words, prob_seg, prob_id, C, SEED, liar=W)

    def solo_liars():
        return [eng.run_joint(m.below, m.above, m.low, m.high, prob_id[ps], C, SEED, liar=w, stream_word=word)
                for m, w, word, ps in zip(models, W, words, chains)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    runs = (('seg', seg), ('seg_liar', seg_liar), ('solo_liars', solo_liars))
    for _ in range(args.warmup):
        for _, fn in runs:
            fn()
    wall, out = dict((k, []) for k, _ in runs), {}
    for i in range(args.pairs):
        for k, fn in runs:
            w, out[k] = timed(fn)
            wall[k].append(w)
        print('round %d: %s' % (i, ', '.join('%s %.2f ms' % (k, wall[k][-1]) for k, _ in runs)), file=sys.stderr,
              flush=True)
    for ps, solo in zip(chains, out['solo_liars']):        # the defining property, on the timed runs
        for f in ('global_idx', 'l', 'g', 'z'):
            assert out['seg_liar'][f][ps].tobytes() == solo[f].tobytes(), f
    med = lambda x: float(np.median(x))   # noqa: E731

    def spread(rec):
        per = []
        for m, ps in zip(models, chains):
            z = rec['z'][ps][:, :D] / np.asarray(m.above[2])[0][None, :]
            d = np.sqrt(((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2))
            np.fill_diagonal(d, np.inf)
            per.append(float(np.median(d.min(axis=1))))
        return float(np.median(per))
    stat = lambda k: dict(wall_median=med(wall[k]), wall_min=min(wall[k]), wall_max=max(wall[k]))   # noqa: E731
    longest = max(len(ps) for ps in chains)
    extra = med(wall['seg_liar']) - med(wall['seg'])
    line = dict(tool='joint_time --liar-branches', groups=S, n_dims=D, history=args.history, n_cand=C, batch=B,
                chain=longest, pairs=args.pairs, k_above=[len(m.above[0]) for m in models], w_sum=W,
                launches=dict(seg_liar=2 * longest, solo_liars=2 * B),
                seg_ms=stat('seg'), seg_liar_ms=stat('seg_liar'), solo_liars_ms=stat('solo_liars'),
                seg_liar_minus_seg_ms=extra, per_round_ms=extra / longest, per_pick_ms=extra / B,
                seg_liar_over_solo_liars=med(wall['seg_liar']) / med(wall['solo_liars']),
                nearest_pick_median=dict(seg=spread(out['seg']), seg_liar=spread(out['seg_liar'])),
                gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    path = args.out or os.path.join(ROOT, 'profiles', 'joint_liar_seg_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'a') as f:
        f.write(text + '\n')
    return 0


def make_branch_mixed_history(n, seed):
    from hyperopt_amd import base, history as H, hp
    space = {'x0': hp.uniform('x0', -5, 5), 'x1': hp.loguniform('x1', -3, 2), 'c2': hp.choice('c2', [0, 1, 2]),
             'q3': hp.quniform('q3', 1, 32, 1)}
    domain = base.Domain(lambda d: 0.0, space)
    rs = np.random.RandomState(seed)
    cols = {'x0': rs.uniform(-5, 5, n), 'x1': np.exp(rs.uniform(-3, 2, n)), 'c2': rs.randint(3, size=n),
            'q3': np.rint(rs.uniform(1, 32, n))}
    loss = (cols['x0'] * cols['x1'] - 2.0) ** 2 + 0.2 * (cols['c2'] != 1) + 1e-3 * (cols['q3'] - 12.0) ** 2 \
        + 0.01 * rs.standard_normal(n)
    tids = np.arange(n, dtype=np.int64)
    return domain, H.History(tids, loss, {k: (tids, v) for k, v in cols.items()})


def main_liar_branches_mixed(args):
    import torch
    from hyperopt_amd import history as H, joint as J
    from hyperopt_amd.engine import get_engine
    from hyperopt_amd.parzen import DEFAULT_LF

    S = 4
    models = []
    for s in range(S):
        domain, hist = make_branch_mixed_history(args.history // S, SEED + s)
        rows = [r for r in domain.table.rows if J.eligible(r)]
        drows = [r for r in domain.table.rows if J.eligible_discrete(r, domain.table)]
        qrows = [r for r in domain.table.rows if J.eligible_quant(r, domain.table)]
        models.append(J.fit_quant_model(rows, drows, qrows, hist, H.split_below(hist, 0.25), 1.0))
    eng = get_engine(None, 'fp32')
    C, B = args.cand, args.batch
    Dc, Dk, Dq = len(rows), len(drows), len(qrows)
    W = [J.side_weight_sum(len(m.above[0]) - 1, 1.0, DEFAULT_LF) for m in models]
    words = [0x52000 + s for s in range(S)]
    centres = [m.centres() for m in models]
    prob_seg = (np.arange(B) % S).astype(np.int32)
    prob_id = np.arange(args.history, args.history + B, dtype=np.int64)
    chains = [np.flatnonzero(prob_seg == s) for s in range(S)]

    def seg():
        return eng.run_joint_segments(models, words, prob_seg, prob_id, C, SEED)

    def seg_liar():
        return eng.run_joint_msegments_liar(models, words, prob_seg, prob_id, C, SEED, liar=W, centres=centres)

    def solo_liars():
        return [eng.run_joint_liar_mixed(m.below[:3], m.above[:3], m.low, m.high, m.cats(), m.quants(), prob_id[ps], C,
                                         SEED, liar=w, stream_word=word, centres=cs)
                for m, w, word, cs, ps in zip(models, W, words, centres, chains)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    runs = (('seg', seg), ('seg_liar', seg_liar), ('solo_liars', solo_liars))
    for _ in range(args.warmup):
        for _, fn in runs:
            fn()
    wall, out = dict((k, []) for k, _ in runs), {}
    for i in range(args.pairs):
        for k, fn in runs:
            w, out[k] = timed(fn)
            wall[k].append(w)
        print('round %d: %s' % (i, ', '.join('%s %.2f ms' % (k, wall[k][-1]) for k, _ in runs)), file=sys.stderr,
              flush=True)
    for ps, solo in zip(chains, out['solo_liars']):        # the defining property, on the timed runs
        for f in ('global_idx', 'l', 'g', 'z'):
            assert out['seg_liar'][f][ps].tobytes() == solo[f].tobytes(), f
    med = lambda x: float(np.median(x))   # noqa: E731

    def spread(rec):                                       # main_liar_mixed's distance, inside every branch
        per = []
        for m, cs, ps in zip(models, centres, chains):
            r = rec['z'][ps]
            z = r[:, :Dc] / np.asarray(m.above[2])[0][None, :]
            q = np.stack([cs[d][r[:, Dc + Dk + d].astype(np.int64)] / m.above[5][0, d] for d in range(Dq)], axis=1)
            z = np.hstack([z, q])
            v = r[:, Dc:Dc + Dk]
            d = np.sqrt(((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2) + (v[:, None, :] != v[None, :, :]).sum(axis=2))
            np.fill_diagonal(d, np.inf)
            per.append(float(np.median(d.min(axis=1))))
        return float(np.median(per))
    stat = lambda k: dict(wall_median=med(wall[k]), wall_min=min(wall[k]), wall_max=max(wall[k]))   # noqa: E731
    longest = max(len(ps) for ps in chains)
    extra = med(wall['seg_liar']) - med(wall['seg'])
    line = dict(tool='joint_time --liar-branches-mixed', groups=S, n_dims=Dc, n_cat=Dk, n_quant=Dq,
                lattice=[lat[1] for lat in models[0].lattices], history=args.history, n_cand=C, batch=B,
                chain=longest, pairs=args.pairs, k_above=[len(m.above[0]) for m in models], w_sum=W,
                launches=dict(seg_liar=2 * longest, solo_liars=2 * B),
                seg_ms=stat('seg'), seg_liar_ms=stat('seg_liar'), solo_liars_ms=stat('solo_liars'),
                seg_liar_minus_seg_ms=extra, per_round_ms=extra / longest, per_pick_ms=extra / B,
                seg_liar_over_solo_liars=med(wall['seg_liar']) / med(wall['solo_liars']),
                nearest_pick_median=dict(seg=spread(out['seg']), seg_liar=spread(out['seg_liar'])),
                gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    path = args.out or os.path.join(ROOT, 'profiles', 'joint_liar_mseg_time.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'a') as f:
        f.write(text + '\n')
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cand', type=int, default=1 << 20)
    ap.add_argument('--history', type=int, default=10000)
    ap.add_argument('--host-cand', type=int, default=None)
    ap.add_argument('--mixed', action='store_true')
    ap.add_argument('--quant', action='store_true')
    ap.add_argument('--wide', action='store_true')
    ap.add_argument('--wide-mixed', action='store_true')
    ap.add_argument('--wide-quant', action='store_true')
    ap.add_argument('--liar', action='store_true')
    ap.add_argument('--liar-mixed', action='store_true')
    ap.add_argument('--liar-branches', action='store_true')
    ap.add_argument('--liar-branches-mixed', action='store_true')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.mixed:
        return main_mixed(args)
    if args.quant:
        return main_quant(args)
    if args.wide:
        return main_wide(args)
    if args.wide_mixed:
        return main_wide_mixed(args)
    if args.wide_quant:
        return main_wide_quant(args)
    if args.liar:
        return main_liar(args)
    if args.liar_mixed:
        return main_liar_mixed(args)
    if args.liar_branches:
        return main_liar_branches(args)
    if args.liar_branches_mixed:
        return main_liar_branches_mixed(args)
    args.out =args.out or os.path.join(ROOT, 'profiles', 'joint_time.jsonl')

    import torch
    from hyperopt_amd import _native as N, history as H, joint as J
    from hyperopt_amd.engine import get_engine

    domain, hist = make_history(args.history)
    rows = [r for r in domain.table.rows if J.eligible(r)]
    model = J.fit_model(rows, hist, H.split_below(hist, 0.25), 1.0)
    eng = get_engine(None, 'fp32')
    lib = eng.lib
    C, D = args.cand, len(rows)
    Kb, Ka = len(model.below[0]), len(model.above[0])
    n_host = C if args.host_cand is None else min(C, args.host_cand)
    ids = np.array([args.history], dtype=np.int64)

    def route_device():
        return eng.run_joint(model.below, model.above, model.low, model.high, ids, C, SEED)

    def route_host():
        rec, cand = eng.run_joint(model.below, model.above, model.low, model.high, ids, C, SEED, return_cand=True)
        z = cand[0, :n_host].astype(np.float64)
        l = J.lpdf_numpy(z, model.below[0], model.below[1], model.below[2], model.low, model.high)
        g = J.lpdf_numpy(z, model.above[0], model.above[1], model.above[2], model.low, model.high)
        return rec, l, g

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        rec = route_device()
    wall = {'host': [], 'device': []}
    kern = []
    ms2 = (ctypes.c_double * 2)()
    for i in range(args.pairs):
        w, (rec_h, l, g) = timed(route_host)
        wall['host'].append(w)
        print('pair %d: host route %.0f ms' % (i, w), file=sys.stderr, flush=True)
        N.check(lib.tpe_joint_profile(1, None), lib, 'tpe_joint_profile')
        w, rec = timed(route_device)
        N.check(lib.tpe_joint_profile(0, ms2), lib, 'tpe_joint_profile')
        wall['device'].append(w)
        kern.append((ms2[0], ms2[1]))
    # (untimed) the device's l and g of the host-scored candidates against the float64 model, in
    # units of the project's lpdf tolerance 1e-5 * max(1, |ref|)
    _, dl, dg = eng.run_joint(model.below, model.above, model.low, model.high, ids, C, SEED, want_lg=True)
    err = max(float(np.max(np.abs(dl[0, :n_host] - l) / np.maximum(1.0, np.abs(l)))),
              float(np.max(np.abs(dg[0, :n_host] - g) / np.maximum(1.0, np.abs(g))))) / 1e-5
    med = lambda x: float(np.median(x))   # noqa: E731
    k1, k2 = med([a for a, _ in kern]), med([b for _, b in kern])
    evals = float(C) * (Kb + Ka) * D
    ops = 3 * D + 7                        # lane-operations per (candidate, component)
    wave_instr = float(C) * (Kb + Ka) * ops / 64.0
    line = dict(tool='joint_time', labels=[r.label for r in rows], history=args.history, n_cand=C, n_dims=D,
                k_below=Kb, k_above=Ka, pairs=args.pairs, host_cand=n_host,
                host_route_ms=dict(wall_median=med(wall['host']), wall_min=min(wall['host']),
                                   wall_max=max(wall['host']),
                                   extrapolated_to_all_candidates_median=med(wall['host']) * C / n_host),
                device_route_ms=dict(wall_median=med(wall['device']), wall_min=min(wall['device']),
                                     wall_max=max(wall['device'])),
                k_joint_chunk_ms=k1, k_joint_merge_ms=k2,
                evals_per_s=evals / (k1 * 1e-3) if k1 > 0 else None,
                ops_per_cand_comp=ops,
                valu_wave_instr_per_s=wave_instr / (k1 * 1e-3) if k1 > 0 else None,
                fraction_of_valu_peak=wave_instr / (k1 * 1e-3) / VALU_PEAK if k1 > 0 else None,
                lpdf_err_over_tol=err, gpu=torch.cuda.get_device_name(0))
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
