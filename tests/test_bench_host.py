"""bench.py's host-side records (no GPU): the tail record's cgroup counters and
the contention counters it carries beside them, and the
arrays --dump-outputs writes."""
import time

import numpy as np

import bench


def test_cgroup_cpu_stat_is_a_dict_of_counters():
    st = bench.cgroup_cpu_stat()
    assert isinstance(st, dict)
    assert all(isinstance(v, int) for v in st.values())


def test_host_contention_counts_grow_and_are_non_negative():
    a = bench.host_contention()
    time.sleep(0.01)                               # (a voluntary switch at least)
    b = bench.host_contention()
    assert {'nivcsw', 'nvcsw'} <= set(a)
    for k in ('nivcsw', 'nvcsw') + tuple(k for k in a if k.startswith('psi_') and k != 'psi_source'):
        assert b[k] >= a[k] >= 0, k
    assert b['nvcsw'] > a['nvcsw']
    if 'psi_source' in a:
        assert a['psi_source'] in ('/sys/fs/cgroup/cpu.pressure', '/proc/pressure/cpu')


def _doc(tid, vals):
    return {'tid': tid, 'misc': {'vals': vals}}


def test_doc_arrays_follow_the_table_order_and_mark_inactive_labels():
    from hyperopt_amd import hp
    from hyperopt_amd.space import ParamTable
    table = ParamTable(bench.tree_space(hp))
    labels = list(table.labels)
    docs = [_doc(7, {k: [] for k in labels}), _doc(8, {k: [float(i) + 0.5] for i, k in enumerate(labels)})]
    docs[0]['misc']['vals']['model'] = [2]
    a = bench.doc_arrays(table, docs)
    assert a['values'].dtype == np.float64 and a['active'].dtype == np.float32
    assert a['values'].shape == a['active'].shape == (2, len(labels))
    m = labels.index('model')
    assert a['values'][0, m] == 2.0 and a['active'][0].sum() == 1 and a['active'][0, m] == 1
    assert np.all(a['values'][0, np.arange(len(labels)) != m] == 0)
    assert np.array_equal(a['values'][1], np.arange(len(labels)) + 0.5) and np.all(a['active'][1] == 1)
    assert np.array_equal(a['tids'], [7.0, 8.0])


def test_choice_arrays_same_for_columns_and_dicts():
    from hyperopt_amd import tpe
    table = bench.flat_uniform_table(['b', 'a', 'c'])
    dicts = [{'a': 1.5, 'b': None, 'c': -2.0}, {'a': 0.25, 'b': 3.0, 'c': None}]
    cc = tpe.ChoiceColumns.from_dicts(table, dicts)
    a, b = bench.choice_arrays(table, cc), bench.choice_arrays(table, dicts)
    for k in ('values', 'active'):
        assert np.array_equal(a[k], b[k]), k
    assert not np.isnan(a['values']).any()
    for j, d in enumerate(dicts):
        for i, k in enumerate(table.labels):
            assert a['active'][j, i] == (d[k] is not None)
            assert a['values'][j, i] == (0.0 if d[k] is None else d[k])


def test_dump_outputs_writes_float_arrays_and_samples_above_the_limit(tmp_path, monkeypatch):
    arrays = dict(values=np.arange(12.0).reshape(4, 3), active=np.ones((4, 3), dtype=np.float32),
                  tids=np.arange(4, dtype=np.int64))
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    got = {f.name[:-4]: np.load(str(f)) for f in (tmp_path / 'a').iterdir()}
    assert sorted(got) == ['active', 'tids', 'values']
    assert got['values'].dtype == np.float64 and got['active'].dtype == np.float32 and got['tids'].dtype == np.float64
    for k in arrays:
        assert np.array_equal(got[k], arrays[k]), k
    # above the limit: the same seeded rows of every array, within the limit in all, the same from run to run
    big = dict(values=np.arange(3000.0).reshape(1000, 3), active=np.ones((1000, 3), dtype=np.float32))
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 6000)
    bench.dump_outputs(str(tmp_path / 'b'), big)
    bench.dump_outputs(str(tmp_path / 'c'), big)
    vb, ab = np.load(str(tmp_path / 'b' / 'values.npy')), np.load(str(tmp_path / 'b' / 'active.npy'))
    assert 0 < len(vb) == len(ab) < 1000 and vb.nbytes + ab.nbytes <= 6000
    assert np.array_equal(vb, big['values'][(vb[:, 0] / 3).astype(int)]) and np.all(np.diff(vb[:, 0]) > 0)
    assert np.array_equal(vb, np.load(str(tmp_path / 'c' / 'values.npy')))
