"""A resident level's fused hit (include/tpe_hip.h "Resident levels"): one id
across the labels and nothing to launch but k_sample_fast — the seed and the id
are that launch's arguments, the lazy categoricals are selected on the host
(hyperopt_amd/csrc/tpe_lazy_host.h), and k_resident_patch is not launched.
Every comparison is exact.

Scan against scan: the cases of tests/lazy_cases.py as one-label categorical
levels through Engine.run_level (the device's select_cat_lazy) and, from the
very rows that level packed, through the host selection: the six result fields
bit for bit.

End to end: single-id suggests on the svm- and rf-steered histories against the
feature switched off, with the counters of tpe_level_resident_fused.  Candidate
counts: 2^20 and the smallest count whose level is fused (MIN_C: 8500 on the svm
histories, ten candidates per cell row of svm_C's 850-row table, the packer's
bar for tabulating it; 104 on the rf history, two per value of rf_depth_n's
52-value lattice) — found from tpe_pack_info's rows by lazy_cases.min_fused_count
and checked here, with one candidate fewer giving no fused hit."""
import numpy as np
import pytest

from tests import draw_cases as DC
from tests import lazy_cases as LC
from tests.helpers import doc_values

from hyperopt_amd import _native as N

pytestmark = pytest.mark.gpu

MIN_C = {'svm': 8500, 'rf': 104}
WHICH = [('svm', 600), ('svm', 2000), ('rf', 2000)]
SEEDS = (3, 4, 5, 6, 7)


@pytest.fixture(scope='module')
def hists():
    import bench
    return {('svm', 600): bench.make_history(600, 0), ('svm', 2000): bench.make_history(2000, 0),
            ('rf', 2000): bench.make_history(2000, 0, loss=bench.rf_loss)}


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return LC.build_program(tmp_path_factory.mktemp('lazy_scan'))


@pytest.fixture(autouse=True)
def _resident_on(monkeypatch):
    monkeypatch.delenv('TPE_LAZY_HOST_BUDGET', raising=False)
    if not N.level_resident(1)[0]:
        pytest.skip('TPE_RESIDENT_LEVEL=0')
    yield
    N.level_resident(1)


def _stats():
    s = dict(N.level_resident(-1)[1])
    s.update(N.level_resident_fused())
    return s


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _off(fn):
    N.level_resident(0)
    try:
        return fn()
    finally:
        N.level_resident(1)


def _suggest(domain, trials, ids, seed, C):
    from hyperopt_amd import tpe
    return [doc_values([d]) for d in tpe.suggest(list(ids), domain, trials, seed, n_EI_candidates=C)]


# ------------------------------------------------------------ scan against scan
def _gpu_specs():
    """lazy_cases.specs() and the NaN score: a drawable category whose above
    weight is a NaN (g = ln NaN)."""
    pb, pa = LC._weights(3, 5)
    pa = pa.copy()
    pa[1] = np.nan
    return LC.specs() + [('nan score', pb, pa, 4096, 3)]


def test_device_scan_equals_host_scan(exe, tmp_path):
    from hyperopt_amd.engine import Engine, LevelProblem
    engine = Engine(precision='fp32')
    cases, dev = [], []
    for name, pb, pa, n_cand, base in _gpu_specs():
        c = DC.case('categorical', (pb,), (pa,), upper=len(pb))
        lps = [LevelProblem(DC.posterior(c), LC.LABEL, [LC.NEW_ID])]
        info = engine._pack(lps, n_cand, LC.SEED, base, base + n_cand)
        host = engine._pinned.numpy()
        p = np.frombuffer(host, dtype=N.PROBLEM_DTYPE, count=1, offset=int(info.off_problems))[0]
        assert p['flags'] & N.F_CAT_LAZY and p['samp_len'] == len(pb), name
        samp = np.frombuffer(host, dtype=np.float64, count=8 * (int(p['samp_off']) + len(pb)),
                             offset=int(info.off_samp)).reshape(-1, 8)[int(p['samp_off']):]
        c64 = np.frombuffer(host, dtype=np.float64,
                            count=4 * (max(int(p['below_off']), int(p['above_off'])) + len(pb)),
                            offset=int(info.off_comp64)).reshape(-1, 4)
        cases.append(dict(name=name, key0=int(p['key0']), key1=int(p['key1']), ctr2=int(p['ctr2']), ctr3=int(p['ctr3']),
                          cand_base=int(p['cand_base']), n_cand=int(p['n_cand']), cum=samp[:, 0].copy(),
                          l=c64[int(p['below_off']):int(p['below_off']) + len(pb), 0].copy(),
                          g=c64[int(p['above_off']):int(p['above_off']) + len(pb), 0].copy()))
        assert cases[-1]['cand_base'] == base and cases[-1]['n_cand'] == n_cand, name
        engine._drop_resident()
        r = engine.run_level(lps, n_cand, LC.SEED, cand_base=base, n_cand_global=base + n_cand)[0]
        dev.append((float(r['score']), float(r['l']), float(r['g']), float(r['value']), int(r['idx']),
                    int(r['global_idx'])))
    by = {c['name']: c for c in cases}
    assert np.isnan(by['nan score']['g'][1])
    assert by['zero mass best']['cum'][1] == by['zero mass best']['cum'][0]
    got = LC.host_select(exe, cases, [LC.UNLIMITED] * len(cases), tmp_path)
    for c, d, (draws, h) in zip(cases, dev, got):
        assert draws >= 0 and LC.same(h, d), (c['name'], draws, h, d)
        assert LC.same(h, LC.model(c)[1]), c['name']


# ------------------------------------------------------------------ end to end
def _count(which, C):
    return C if C else MIN_C[which[0]]


def test_min_counts_are_the_packers(hists):
    for which in WHICH:
        assert LC.min_fused_count(*hists[which]) == MIN_C[which[0]], which


@pytest.mark.parametrize('which', WHICH)
@pytest.mark.parametrize('C', [1 << 20, 0])
def test_fused_hits_equal_off(hists, which, C, monkeypatch):
    domain, trials = hists[which]
    n, C = which[1], _count(which, C)
    ref = _off(lambda: [_suggest(domain, trials, [n], s, C) for s in SEEDS])
    s0 = _stats()
    got = [_suggest(domain, trials, [n], s, C) for s in SEEDS]
    d = _delta(s0, _stats())
    assert got == ref
    assert d['misses'] == 1 and d['hits'] >= 4 and d['fused'] == d['hits'] and d['fallbacks'] == 0, d
    # no budget: the same results, every fused hit by the patch kernel behind the sample kernel
    monkeypatch.setenv('TPE_LAZY_HOST_BUDGET', '0')
    s1 = _stats()
    got = [_suggest(domain, trials, [n], s, C) for s in SEEDS]
    d = _delta(s1, _stats())
    assert got == ref
    assert d['misses'] == 1 and d['hits'] >= 4 and d['fused'] == d['hits'] and d['fallbacks'] == d['fused'], d


@pytest.mark.parametrize('which', WHICH)
def test_one_candidate_fewer_is_not_fused(hists, which):
    domain, trials = hists[which]
    n, C = which[1], MIN_C[which[0]] - 1
    ref = _off(lambda: [_suggest(domain, trials, [n], s, C) for s in SEEDS[:3]])
    s0 = _stats()
    got = [_suggest(domain, trials, [n], s, C) for s in SEEDS[:3]]
    d = _delta(s0, _stats())
    assert got == ref and d['fused'] == 0, d


@pytest.mark.parametrize('which', WHICH)
def test_three_ids_take_the_patch_path(hists, which):
    domain, trials = hists[which]
    n, C = which[1], 1 << 20
    ids = [n, n + 1, n + 2]
    ref = _off(lambda: [_suggest(domain, trials, ids, s, C) for s in SEEDS])
    s0 = _stats()
    got = [_suggest(domain, trials, ids, s, C) for s in SEEDS]
    d = _delta(s0, _stats())
    assert got == ref
    assert d['hits'] >= 4 and d['fused'] == 0 and d['fallbacks'] == 0, d


@pytest.mark.parametrize('which', WHICH)
def test_stale_rows_are_never_consumed(hists, which, monkeypatch):
    """Fused hits leave an older call's words in the device rows.  The budget
    switch is part of the record's key: flipping it is a miss (the rows are
    uploaded afresh), the hit after it falls back to the patch kernel (which
    rewrites every row), and flipping it back is a miss again."""
    domain, trials = hists[which]
    n, C = which[1], 1 << 20
    seeds = list(range(20, 29))
    ref = _off(lambda: [_suggest(domain, trials, [n], s, C) for s in seeds])
    got = []
    s0 = _stats()
    got += [_suggest(domain, trials, [n], s, C) for s in seeds[:3]]          # a miss, two fused hits
    d0 = _delta(s0, _stats())
    monkeypatch.setenv('TPE_LAZY_HOST_BUDGET', '0')
    s1 = _stats()
    got += [_suggest(domain, trials, [n], s, C) for s in seeds[3:6]]         # a miss, two fallbacks
    d1 = _delta(s1, _stats())
    monkeypatch.delenv('TPE_LAZY_HOST_BUDGET')
    s2 = _stats()
    got += [_suggest(domain, trials, [n], s, C) for s in seeds[6:]]          # a miss, two fused hits
    d2 = _delta(s2, _stats())
    assert got == ref
    assert d0['misses'] == 1 and d0['fused'] >= 2 and d0['fallbacks'] == 0, d0
    assert d1['misses'] == 1 and d1['fused'] >= 2 and d1['fallbacks'] == d1['fused'], d1
    assert d2['misses'] == 1 and d2['fused'] >= 2 and d2['fallbacks'] == 0, d2
