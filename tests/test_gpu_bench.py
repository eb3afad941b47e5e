"""bench.py's command line on the device, at a small size: a plain run prints
the timed steps' line alone and --dump-outputs writes what the last timed step
returned; --full adds the other measurements to the same line."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_HIST, CANDS, STEPS = 600, 4096, 3
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup')
FULL_ONLY = ('tail', 'stage_ms', 'roofline', 'kernels', 'cpu_baseline', 'quantized_branch', 'appending',
             'config4_strong', 'strong_scaling')


def run_bench(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', str(STEPS), '--warmup', '1',
                                      '--history', str(N_HIST), '--cands', str(CANDS)] + list(argv))
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith('{')]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def check_headline(line):
    assert all(k in line for k in HEADLINE), sorted(line)
    assert line['steps'] == STEPS and line['warmup'] == 1
    assert line['unit'] == 'candidate-scores/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] > 0 and line['value'] > 0
    # value = active hyperparameters x candidates per step / the step's time
    per_step = line['active_hyperparameters_per_suggest'] * CANDS
    assert line['value'] == pytest.approx(per_step / (1e-3 * line['ms_per_step']), rel=1e-9)


def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(monkeypatch, capsys, tmp_path):
    import bench
    from hyperopt_amd import tpe
    out = tmp_path / 'dump'
    line = run_bench(monkeypatch, capsys, '--dump-outputs', str(out))
    check_headline(line)
    assert line['full'] is False
    assert not [k for k in FULL_ONLY if k in line]
    # the dumped arrays: the document a caller of the last timed step receives
    domain, trials = bench.make_history(N_HIST, bench.SEED)
    docs = tpe.suggest([N_HIST], domain, trials, bench.SEED + 1000 + STEPS - 1, n_EI_candidates=CANDS)
    want = bench.doc_arrays(domain.table, docs)
    assert sorted(f.name for f in out.iterdir()) == ['active.npy', 'tids.npy', 'values.npy']
    for k, w in want.items():
        got = np.load(str(out / (k + '.npy')))
        assert got.dtype == w.dtype and got.dtype in (np.float32, np.float64)
        assert np.array_equal(got, w), (k, got, w)
    assert want['active'].sum() >= 1 and want['tids'][0] == N_HIST


@pytest.mark.parametrize('appending', [False, True], ids=['dicts', 'appending-columns'])
def test_other_config_plain_run_and_dump(monkeypatch, capsys, tmp_path, appending):
    """Config 5 at 8 dimensions: per-id dicts (plain) and ChoiceColumns
    (--appending) results dump as the same [n_ids x n_labels] arrays."""
    out = tmp_path / 'dump'
    line = run_bench(monkeypatch, capsys, '--config', '5', '--dims', '8', '--history5', '500',
                     '--dump-outputs', str(out), *(['--appending'] if appending else []))
    assert all(k in line for k in HEADLINE), sorted(line)
    assert line['steps'] == STEPS and line['ms_per_step'] > 0 and line['full'] is False
    assert line['value'] == pytest.approx(8 * 4096 / (1e-3 * line['ms_per_step']), rel=1e-9)
    assert 'stage_ms_per_step' not in line and 'host_phases_us' not in line
    assert sorted(f.name for f in out.iterdir()) == ['active.npy', 'values.npy']
    values, active = np.load(str(out / 'values.npy')), np.load(str(out / 'active.npy'))
    assert values.dtype == np.float64 and active.dtype == np.float32
    assert values.shape == active.shape == (1, 8)
    assert np.all(active == 1) and np.all((values >= -5) & (values <= 5)) and len(np.unique(values)) == 8


def test_full_run_carries_the_other_measurements(monkeypatch, capsys):
    line = run_bench(monkeypatch, capsys, '--full', '--no-cpu-baseline', '--no-config4')
    check_headline(line)
    assert line['full'] is True
    assert all(k in line for k in FULL_ONLY), sorted(line)
    assert len(line['tail']['steps_ms']) == STEPS
    assert line['stage_ms'] and line['appending']['suggests'] >= 10
    assert line['quantized_branch']['p50_suggest_ms'] > 0
    assert line['cpu_baseline'] is None and line['config4_strong'] is None
