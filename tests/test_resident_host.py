"""Resident levels, the parts that need no GPU (include/tpe_hip.h "Resident
levels"): the invariant the hit path rests on — two packs of one level with
different seeds and new ids differ only in key0 / key1 / ctr3 of the problem
rows — the new export, and the fit keys' copy / compare / cap logic, run as a
stand-alone sanitized program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CALL_FIELDS = ('key0', 'key1', 'ctr3')


def _pack(problems, n_cand, seed):
    """(blob bytes, PackInfo) of one level packed by tpe_host_pack_level into a
    zeroed buffer."""
    from hyperopt_amd.engine import Engine
    lib = N.load()
    labels, keep = Engine._labels(problems)
    info = N.PackInfo()
    rc = lib.tpe_host_pack_level(labels, len(problems), n_cand, seed, 0, 0, N.PREC_F32, None, 0, ctypes.byref(info))
    assert rc == N.E_SPACE and info.blob_bytes > 0, rc
    buf = np.zeros(int(info.blob_bytes) + 256, dtype=np.uint8)
    rc = lib.tpe_host_pack_level(labels, len(problems), n_cand, seed, 0, 0, N.PREC_F32, buf.ctypes.data, buf.size,
                                 ctypes.byref(info))
    assert rc == 0, (rc, lib.tpe_last_error())
    del keep
    return buf, info


def _per_call_bytes(info):
    """Blob offsets of key0 / key1 / ctr3 of every host-written problem row."""
    P, size = int(info.n_problems), N.PROBLEM_DTYPE.itemsize
    out = set()
    for r in range(P):
        for f in PER_CALL_FIELDS:
            dt, off = N.PROBLEM_DTYPE.fields[f][:2]
            out.update(range(int(info.off_problems) + r * size + off,
                             int(info.off_problems) + r * size + off + dt.itemsize))
    return out


def _check_invariant(make_problems, n_cand):
    p1, p2 = make_problems(0), make_problems(1)
    b1, i1 = _pack(p1, n_cand, 0x1234567855AA33CC)
    b2, i2 = _pack(p2, n_cand, 0xFEDCBA9800112277)
    # the same plan: every PackInfo field, the upload ranges included
    assert bytes(i1) == bytes(i2)
    assert int(i1.n_expand) == 0 and int(i1.n_fit) == 0
    diff = set(np.flatnonzero(b1 != b2).tolist())
    assert diff, 'the seed and the ids left no trace in the blob'
    assert diff <= _per_call_bytes(i1), sorted(diff - _per_call_bytes(i1))[:16]
    # every difference lies in a host-written range: the hit path's patch of the
    # device rows is the whole upload it owes (both layouts of up_*: one range
    # or several)
    ranges = [(int(i1.up_off[k]), int(i1.up_off[k]) + int(i1.up_len[k])) for k in range(int(i1.n_up))]
    assert ranges and all(any(lo <= d < hi for lo, hi in ranges) for d in diff)
    return int(i1.n_up)


def _tree_problems(loss_name, n_cand):
    import bench
    from hyperopt_amd import history as H, tpe
    from hyperopt_amd.engine import LevelProblem
    domain, trials = bench.make_history(2000, 0, loss=getattr(bench, loss_name) if loss_name else None)
    hist = H.extract(domain, trials)
    table = domain.table
    fits = tpe._Fits(table, hist, H.split_below(hist, 0.25), 1.0, None)
    pred = tpe._predict_activity(table, fits, n_cand)
    if pred is None:                     # (too few candidates for a prediction: the first level)
        rows = list(table.levels())[0]
    else:
        rows = [r for r in table.rows if pred[r.label] is not None]
    posts = [(fits.get(r), r.index) for r in rows]

    def make(which):
        ids = np.array([2000 + 13 * which], dtype=np.int64)
        return [LevelProblem(post, ix, ids) for post, ix in posts]
    return make


@pytest.fixture(scope='module')
def tree_levels():
    cache = {}

    def get(loss_name, n_cand):
        key = (loss_name, n_cand)
        if key not in cache:
            cache[key] = _tree_problems(loss_name, n_cand)
        return cache[key]
    return get


@pytest.mark.parametrize('n_cand', [24, 4096, 1 << 20])
@pytest.mark.parametrize('loss_name', [None, 'rf_loss'])
def test_packs_differ_only_in_per_call_fields(tree_levels, loss_name, n_cand):
    """svm-steered (default loss) and rf-steered config-3 trees on 2000
    trials: per-candidate scoring (24), lattice and cell tables (4096, 2^20)."""
    _check_invariant(tree_levels(loss_name, n_cand), n_cand)


def test_flat_level_three_ids_differs_only_in_per_call_fields():
    import bench
    from hyperopt_amd import history as H, tpe
    from hyperopt_amd.engine import LevelProblem
    labels = ['x%d' % i for i in range(5)]
    hist = bench.soa_history(labels, 400, 1, lambda v: sum((x - 0.3) ** 2 for x in v.values()))
    table = bench.flat_uniform_table(labels)
    fits = tpe._Fits(table, hist, H.split_below(hist, 0.25), 1.0, None)
    posts = [(fits.get(r), r.index) for r in table.rows]

    def make(which):
        ids = np.array([400, 401, 402], dtype=np.int64) + 7 * which
        return [LevelProblem(post, ix, ids) for post, ix in posts]
    for n_cand in (24, 4096, 1 << 16):
        _check_invariant(make, n_cand)


def test_level_resident_export():
    """Declared in the header, bound, and callable without a device: the mode
    switch, the query and the counters."""
    src = open(os.path.join(ROOT, 'include', 'tpe_hip.h')).read()
    assert 'int tpe_level_resident(int32_t mode, int64_t* stats);' in src
    assert 'tpe_level_resident' in N.EXPORTS
    assert '#define TPE_ABI_VERSION 24' in src.replace('  ', ' ') or N.load().tpe_abi_version() == 24
    lib = N.load()
    assert lib.tpe_abi_version() == 24
    env_on = os.environ.get('TPE_RESIDENT_LEVEL', '1')[:1] != '0'
    on, st0 = N.level_resident(-1)
    assert on == env_on and set(st0) == {'hits', 'misses', 'fit_reuses', 'drops'}
    try:
        on, st1 = N.level_resident(0)
        assert not on and st1['drops'] == st0['drops'] + 1
        assert not N.level_resident(-1)[0]
        on, st2 = N.level_resident(2)                # drop only: the mode stays
        assert not on and st2['drops'] == st1['drops'] + 1
    finally:
        on, st3 = N.level_resident(1)
    assert on == env_on and st3['hits'] == st0['hits']
    assert lib.tpe_level_resident(-1, None) == int(env_on)     # (a NULL stats pointer)


def test_fit_reuse_counts_without_gpu():
    """tpe_suggest_tree twice on one history with empty workspaces (it stops at
    TPE_E_SPACE, after the fits): the second call's labels match their keys —
    rebuilt arrays at other addresses included — and a changed value does not."""
    import bench
    from hyperopt_amd import history as H, tpe
    if not N.level_resident(-1)[0]:
        pytest.skip('TPE_RESIDENT_LEVEL=0')
    domain, trials = bench.make_history(600, 0)
    hist = H.extract(domain, trials)
    arr, keep = tpe._tree_labels(domain.table, hist)[:2]
    below = np.sort(H.split_below(hist, 0.25)).astype(np.int64)
    lib = N.load()

    def call(a, b):
        ws, need = N.LevelWS(), N.LevelNeed()
        vals = np.empty((1, len(a)))
        act = np.empty((1, len(a)), dtype=np.int8)
        path = (ctypes.c_int32 * 2)()
        nf = np.zeros(len(a), dtype=np.int8)
        ids = np.array([600], dtype=np.int64)
        rc = lib.tpe_suggest_tree(a.ctypes.data, len(a), b.ctypes.data, len(b), 1.0, 25, ids.ctypes.data, 1, 1 << 16,
                                  0, 0, None, 5, 64.0, 16384, 0, ctypes.byref(ws), ctypes.byref(need), None,
                                  vals.ctypes.data, act.ctypes.data, path, nf.ctypes.data)
        assert rc == N.E_SPACE, rc
        return N.level_resident(-1)[1]
    s0 = call(arr, below)
    s1 = call(arr, below)
    n_fit = s1['fit_reuses'] - s0['fit_reuses']
    assert n_fit >= 4 and s1['hits'] == s0['hits']           # (every fitted label of the predicted branch)
    # the same content in rebuilt arrays: still the same keys
    arr2 = arr.copy()
    copies = {}
    for i in range(len(arr2)):
        n = int(arr2[i]['n_obs'])
        if n > 0 and arr2[i]['tids'] and arr2[i]['values']:
            t = np.ctypeslib.as_array(ctypes.cast(int(arr2[i]['tids']), ctypes.POINTER(ctypes.c_int64)), (n,)).copy()
            v = np.ctypeslib.as_array(ctypes.cast(int(arr2[i]['values']), ctypes.POINTER(ctypes.c_int64)), (n,)).copy()
            copies[i] = (t, v)
            arr2[i]['tids'], arr2[i]['values'] = t.ctypes.data, v.ctypes.data
    s2 = call(arr2, below.copy())
    assert s2['fit_reuses'] - s1['fit_reuses'] == n_fit
    # one below tid replaced: every label is fitted anew
    b2 = below.copy()
    b2[-1] = [t for t in range(600) if t not in set(below.tolist())][-1]
    b2.sort()
    s3 = call(arr2, b2)
    assert s3['fit_reuses'] == s2['fit_reuses']
    s4 = call(arr2, b2)
    assert s4['fit_reuses'] - s3['fit_reuses'] == n_fit
    # one value of one fitted label overwritten in place (same address): that label alone misses
    root = copies[domain.table.by_label['model'].index][1]      # (the root gate: a category 0 <-> 1)
    root[0] ^= 1
    s5 = call(arr2, b2)
    assert 0 < s5['fit_reuses'] - s4['fit_reuses'] < n_fit or n_fit == 1
    del keep, copies


def test_keystore_sanitized_program(tmp_path):
    """tools/ubench/keystore_test.cpp (growth, shrink, equal and unequal sizes,
    a one-element change at the first and the last position, the cap) built
    with AddressSanitizer and UBSan and run as a plain executable."""
    gxx = shutil.which(os.environ.get('CXX', 'g++'))
    if gxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path / 'keystore_test')
    # (the sanitizer runtimes linked into the executable itself: nothing to load beside it)
    subprocess.check_call([gxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-static-libasan',
                           '-static-libubsan', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'hyperopt_amd', 'csrc'),
                           os.path.join(ROOT, 'tools', 'ubench', 'keystore_test.cpp'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and 'keystore_test: ok' in out.stdout, out.stdout + out.stderr
