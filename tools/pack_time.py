"""CPU timing and digests of tpe_host_pack_level on fixed levels (no GPU).
Usage: python tools/pack_time.py SHAPE [args] [--digest] [--cap BYTES]

  headline [REPS]         config 3's svm/rbf branch (model, svm_kernel, svm_C,
                          svm_rbf_gamma fitted on the host from the 10k-trial
                          history), one new id, 2^20 candidates
  config4 [D] [N_IDS] [REPS]   D uniform(-5, 5) labels fitted on the host (25
                          below, 9975 above), each active for N_IDS new ids,
                          C = 4096: an expanded level (include/tpe_hip.h)
  config5 [D] [N] [REPS]  D device-fitted uniform labels (the above side a
                          device fit of N observations — fake device addresses:
                          the packer only records them), C = 4096
  mixed [REPS]            seven families in one level at C = 24, 5000 and 2^17,
                          f32 (with a device-fitted label of three ids) and f64

Prints microseconds per call (median of REPS).  --digest: one call per level
into a zero-filled blob, then a sha256 over the tpe_pack_info bytes and the
host-written ranges (up_off / up_len) — section padding and device-only regions
are never written.  --cap 0 is the sizing call (TPE_E_SPACE): the info alone.
TPE_PACK_LIB selects a host-only build (tools/build_pack_trace.sh: the packer's
sections timed on stderr, tools/pack_sections.py), TPE_HIP_LIB another full one."""
import ctypes
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np  # noqa: E402

from hyperopt_amd import _native as N, parzen  # noqa: E402
from hyperopt_amd.engine import Engine, LevelProblem  # noqa: E402


def load():
    if not os.environ.get('TPE_PACK_LIB'):
        return N.load()
    lib = ctypes.CDLL(os.environ['TPE_PACK_LIB'])
    lib.tpe_host_pack_level.restype = ctypes.c_int
    lib.tpe_host_pack_level.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.c_void_p]
    return lib


def headline(args):
    import bench
    from hyperopt_amd import history as H, tpe
    domain, trials = bench.make_history(10000, bench.SEED)
    hist = H.extract(domain, trials)
    fits = tpe._Fits(domain.table, hist, H.split_below(hist, 0.25), 1.0, None)
    rows = [domain.table.by_label[k] for k in ('model', 'svm_kernel', 'svm_C', 'svm_rbf_gamma')]
    ids = np.array([len(hist)], dtype=np.int64)
    problems = [LevelProblem(fits.get(r), r.index, ids) for r in rows]
    recs, keep = Engine._labels(problems)
    return [('svm/rbf C %d' % (1 << 20), recs, len(problems), 1 << 20, N.PREC_F32, keep)], 64 << 20, \
        int(args[0]) if args else 200


def _uniform_label(r, i, below, ids):
    w, mu, sg = below
    r['family'], r['flags'], r['label_ix'] = N.FAM_GAUSS, N.F_HAS_LOW | N.F_HAS_HIGH, i
    r['low'], r['high'] = -5.0, 5.0
    r['below_w'], r['below_mu'], r['below_sigma'], r['below_k'] = w.ctypes.data, mu.ctypes.data, sg.ctypes.data, len(w)
    r['ids'], r['n_ids'] = ids.ctypes.data, len(ids)
    r['lf'] = 25
    r['prior_mu'], r['prior_sigma'], r['prior_weight'] = 0.0, 10.0, 1.0


def _fit(rs, n):
    return tuple(np.ascontiguousarray(a) for a in parzen.fit_parzen(rs.uniform(-5, 5, n), 1.0, 0.0, 10.0))


def config4(args):
    D, n_ids, reps = [int(a) for a in args] + [20, 4096, 30][len(args):]
    rs = np.random.RandomState(0)
    recs = np.zeros(D, dtype=N.LABEL_DTYPE)
    ids = np.arange(10000, 10000 + n_ids, dtype=np.int64)
    keep = [recs, ids]
    for i in range(D):
        below, (aw, am, as_) = _fit(rs, 25), _fit(rs, 9975)
        keep += [below, aw, am, as_]
        _uniform_label(recs[i], i, below, ids)
        r = recs[i]
        r['above_w'], r['above_mu'], r['above_sigma'], r['above_k'] = aw.ctypes.data, am.ctypes.data, as_.ctypes.data, len(aw)
    return [('D %d ids %d' % (D, n_ids), recs.ctypes.data, D, 4096, N.PREC_F32, keep)], 256 << 20, reps


def config5(args):
    D, n_obs, reps = [int(a) for a in args] + [1000, 100000, 50][len(args):]
    rs = np.random.RandomState(0)
    recs = np.zeros(D, dtype=N.LABEL_DTYPE)
    ids = np.array([n_obs], dtype=np.int64)
    bidx = np.sort(rs.choice(n_obs, 25, replace=False)).astype(np.int32)
    keep = [recs, ids, bidx]
    for i in range(D):
        below = _fit(rs, 25)
        keep.append(below)
        _uniform_label(recs[i], i, below, ids)
        r = recs[i]
        r['above_k'] = n_obs - 25 + 1
        r['dev_obs'], r['n_obs'] = 0x1000, n_obs            # (a device address the packer only copies)
        r['below_idx'], r['n_below'] = bidx.ctypes.data, 25
        r['ord_key_in'], r['ord_idx_in'], r['n_ord_in'] = 0x2000, 0x3000, n_obs
    # (the device-fit reserve counts: untouched pages)
    return [('D %d n_obs %d' % (D, n_obs), recs.ctypes.data, D, 4096, N.PREC_F32, keep)], 4 << 30, reps


class _FakeColumn(object):
    """Stand-in for a device column: the packer only records its address."""

    def data_ptr(self):
        return 0xD0000000


class _FakeOrder(object):
    """Stand-in for a devhist.ValueOrder with nothing sorted yet."""

    class _Group(object):
        def ensure(self, slots, n_obs):
            pass

    group, slot = _Group(), 0

    def ptrs(self, n_obs):
        return (0, 0, 0, 0xE2000000, 0xE3000000)


def mixed(args):
    rs = np.random.RandomState(2)
    fp = parzen.fit_posterior
    posts = [fp('loguniform', dict(low=-5.0, high=5.0), np.exp(rs.uniform(-5, 5, 20)), np.exp(rs.uniform(-5, 5, 3000)), 1.0),
             fp('uniform', dict(low=-1.0, high=2.0), rs.uniform(-1, 2, 5), rs.uniform(-1, 2, 40), 1.0),
             fp('normal', dict(mu=0.0, sigma=2.0), rs.normal(0, 2, 9), rs.normal(0, 2, 500), 1.0),
             fp('quniform', dict(low=0.0, high=10.0, q=1.0), np.round(rs.uniform(0, 10, 9)),
                np.round(rs.uniform(0, 10, 300)), 1.0),
             fp('qlognormal', dict(mu=1.0, sigma=0.5, q=0.25), np.round(np.exp(rs.normal(1, .5, 9)) / .25) * .25,
                np.round(np.exp(rs.normal(1, .5, 90)) / .25) * .25, 1.0),
             fp('categorical', dict(p=[.2, .3, .5], upper=3), rs.randint(0, 3, 9), rs.randint(0, 3, 90), 1.0),
             fp('quniform', dict(low=-3.0, high=3.0, q=0.01), np.round(rs.uniform(-3, 3, 9), 2),
                np.round(np.clip(rs.normal(2.5, 0.4, 3000), -3, 3), 2), 1.0)]
    dev = fp('uniform', dict(low=-1.0, high=2.0), rs.uniform(-1, 2, 3), None, 1.0,
             above_dev=(_FakeColumn(), 500, np.array([3, 10, 77], dtype=np.int32), _FakeOrder()))
    lps = [LevelProblem(p, i + 3, np.arange(i + 1) + 100) for i, p in enumerate(posts)]
    levels = []
    for prec, name in ((N.PREC_F32, 'f32'), (N.PREC_F64, 'f64')):
        # (the device fit is f32 only)
        level = lps + [LevelProblem(dev, 2, [5, 6, 7])] if prec == N.PREC_F32 else lps
        recs, keep = Engine._labels(level)
        for C in (24, 5000, 1 << 17):
            levels.append(('%s C %d' % (name, C), recs, len(level), C, prec, keep))
    return levels, 64 << 20, int(args[0]) if args else 200


def main():
    argv = sys.argv[1:]
    digest = '--digest' in argv
    cap = None
    if '--cap' in argv:
        cap = int(argv[argv.index('--cap') + 1])
        del argv[argv.index('--cap'):argv.index('--cap') + 2]
    argv = [a for a in argv if a != '--digest']
    shapes = dict(headline=headline, config4=config4, config5=config5, mixed=mixed)
    if not argv or argv[0] not in shapes:
        sys.exit(__doc__)
    lib = load()
    levels, cap_default, reps = shapes[argv[0]](argv[1:])
    cap = cap_default if cap is None else cap
    blob = np.zeros(max(cap, 1), dtype=np.uint8)
    info = N.PackInfo()
    for name, recs, n, C, prec, _keep in levels:
        def pack():
            return lib.tpe_host_pack_level(recs, n, C, 7, 0, 0, prec, blob.ctypes.data if cap else None, cap,
                                           ctypes.byref(info))
        if digest:
            if name != levels[0][0]:
                blob[:] = 0                  # (the first level's is still zero: config 5's reserve stays untouched)
            ctypes.memset(ctypes.byref(info), 0, ctypes.sizeof(info))
            rc = pack()
            assert rc == (0 if cap else N.E_SPACE), rc
            h = hashlib.sha256(bytes(info))
            for i in range(info.n_up if cap else 0):
                h.update(blob[int(info.up_off[i]):int(info.up_off[i] + info.up_len[i])].tobytes())
            print('%s %s: rc %d blob %d B sha256 %s' % (argv[0], name, rc, info.blob_bytes, h.hexdigest()))
            continue
        ts = []
        for _ in range(reps):
            s = time.perf_counter()
            rc = pack()
            ts.append(time.perf_counter() - s)
            assert rc == 0, rc
        print('%s %s: tpe_host_pack_level p50 %.1f us, p10 %.1f, min %.1f (blob %d B, expanded %d, %d tab jobs, '
              '%d tab units, fgt boxes %d, upload %s)'
              % (argv[0], name, 1e6 * np.median(ts), 1e6 * np.percentile(ts, 10), 1e6 * min(ts), info.blob_bytes,
                 info.n_expand, info.n_tab_jobs, info.tab_units, info.fgt_max_boxes,
                 [(int(info.up_off[i]), int(info.up_len[i])) for i in range(info.n_up)]))


if __name__ == '__main__':
    main()
