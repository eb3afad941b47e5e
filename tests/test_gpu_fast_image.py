"""The fused hit from the prepared image (DESIGN.md section 3 "Two hit paths")
against the same calls with TPE_FAST_IMAGE=0 (no image: the patch path and the
row-keyed kernel): the suggested values, exactly.  Candidate counts at the
kernel's edges: the smallest fused count, one tile + 1 and two tiles + 1 (the
last unit and the i < n_cand edge), on the cells labels of the svm-steered
history and the lattices of the rf-steered one (their levels hold lazy
categoricals besides the tabulated labels), then without a host budget (the
patch kernel behind the image kernel), across an epoch bump and across a
changed history."""
import pytest

from tests import lazy_cases as LC
from tests.helpers import doc_values

from hyperopt_amd import _native as N

pytestmark = pytest.mark.gpu

SEEDS = (3, 4, 5, 6)


@pytest.fixture(scope='module')
def hists():
    import bench
    return {'svm': bench.make_history(600, 0), 'rf': bench.make_history(600, 0, loss=bench.rf_loss)}


@pytest.fixture(autouse=True)
def _resident_on(monkeypatch):
    monkeypatch.delenv('TPE_LAZY_HOST_BUDGET', raising=False)
    monkeypatch.delenv('TPE_FAST_IMAGE', raising=False)
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


def _suggest(domain, trials, seed, C, n=600):
    from hyperopt_amd import tpe
    return doc_values(tpe.suggest([n], domain, trials, seed, n_EI_candidates=C))


def _counts(domain, trials):
    tile = N.load().tpe_tile_size()
    m = LC.min_fused_count(domain, trials)
    return sorted({m, max(m, tile + 1), max(m, 2 * tile + 1)})


@pytest.mark.parametrize('which', ['svm', 'rf'])
def test_image_hits_equal_image_off(hists, which, monkeypatch):
    domain, trials = hists[which]
    for C in _counts(domain, trials):
        _suggest(domain, trials, 1, C)                       # (the pools grow to this count: growth is a miss)
        monkeypatch.setenv('TPE_FAST_IMAGE', '0')
        s0 = _stats()
        ref = [_suggest(domain, trials, s, C) for s in SEEDS]
        d = _delta(s0, _stats())
        assert d['misses'] == 1 and d['hits'] == len(SEEDS) - 1 and d['fused'] == 0, (C, d)
        monkeypatch.delenv('TPE_FAST_IMAGE')
        s1 = _stats()
        got = [_suggest(domain, trials, s, C) for s in SEEDS]
        d = _delta(s1, _stats())
        assert got == ref, C
        assert d['misses'] == 1 and d['fused'] == d['hits'] == len(SEEDS) - 1 and d['fallbacks'] == 0, (C, d)
        # no host budget: the patch kernel behind the image kernel
        monkeypatch.setenv('TPE_LAZY_HOST_BUDGET', '0')
        s2 = _stats()
        got = [_suggest(domain, trials, s, C) for s in SEEDS]
        d = _delta(s2, _stats())
        monkeypatch.delenv('TPE_LAZY_HOST_BUDGET')
        assert got == ref, C
        assert d['misses'] == 1 and d['fused'] == d['hits'] and d['fallbacks'] == d['fused'], (C, d)


@pytest.mark.parametrize('which', ['svm', 'rf'])
def test_an_epoch_bump_makes_new_images(hists, which):
    """Hit, the record dropped (tpe_level_resident(2)), then a miss whose images
    serve the next hits: every call equals the resident-off one."""
    domain, trials = hists[which]
    C = _counts(domain, trials)[-1]
    N.level_resident(0)
    try:
        ref = [_suggest(domain, trials, s, C) for s in SEEDS]
    finally:
        N.level_resident(1)
    s0 = _stats()
    got = [_suggest(domain, trials, s, C) for s in SEEDS[:2]]
    N.level_resident(2)
    got += [_suggest(domain, trials, s, C) for s in SEEDS[2:]]
    d = _delta(s0, _stats())
    assert got == ref
    assert d['misses'] == 2 and d['fused'] == d['hits'] == len(SEEDS) - 2, d


def test_a_changed_history_gets_its_own_images(hists):
    """Hit on one history, miss and hit on a longer one: the second level's
    hits equal its own image-off calls."""
    import bench
    domain, trials = hists['svm']
    domain2, trials2 = bench.make_history(601, 0)
    C = _counts(domain, trials)[-1]
    N.level_resident(0)
    try:
        ref = [_suggest(domain2, trials2, s, C, n=601) for s in SEEDS]
    finally:
        N.level_resident(1)
    s0 = _stats()
    [_suggest(domain, trials, s, C) for s in SEEDS[:2]]
    got = [_suggest(domain2, trials2, s, C, n=601) for s in SEEDS]
    d = _delta(s0, _stats())
    assert got == ref
    assert d['misses'] == 2 and d['fused'] == d['hits'] == len(SEEDS), d


# ------------------------------------------------------- the packer's edges
EDGE_C = {'outlier': 1 << 20}               # (else 2^16; the outlier's tail draws want many candidates)
EDGES = ('one row, nine cells', 'two rows', '26 rows', '850 cells', 'outlier')


@pytest.fixture(scope='module')
def edge_cases():
    from tests import fast_image_cases as FC
    return FC.cases()


def _full(domain, trials, seed, C, gamma, info):
    """One single-id suggest: the document's values, the native call's value
    and active rows, and the level's winning tpe_result rows (staging buffer)."""
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    from tests import fast_image_cases as FC
    n = len(trials.trials)
    docs = tpe.suggest([n], domain, trials, seed, n_EI_candidates=C, gamma=gamma, n_startup_jobs=0)
    eng = get_engine()
    nl = len(domain.table.rows)
    io = eng._tree_io
    res = FC.staged(eng, info)[2]
    return doc_values(docs), io.values[:nl].tobytes(), io.active[:nl].tobytes(), res.tobytes()


@pytest.mark.parametrize('name', EDGES)
def test_edge_levels_equal_image_off(edge_cases, name, monkeypatch):
    """Sampler rows 1, 2 and 26 (the guide's a == len - 1 and `never` cases),
    the smallest log-polynomial table the packer makes (9 cells), a bounded
    label's largest (850) and an unbounded label's at 892 of the kernel's 896
    rows, whose draws beyond the cells take the exact fallback from the
    header's offsets: values, active flags and every field of the winning
    results, bit for bit, against TPE_FAST_IMAGE=0."""
    from tests import fast_image_cases as FC
    domain, trials, gamma, want = edge_cases[name]
    C = EDGE_C.get(name, 1 << 16)
    rows, info = FC.level(domain, trials, C, gamma)
    assert LC.fused_eligible(rows), name
    by_ix = {r.index: r.label for r in domain.table.rows}
    for p in rows:
        n_samp, n_cells = want[by_ix[int(p['ctr2'])]]
        assert n_samp is None or p['samp_len'] == n_samp, (name, p['samp_len'])
        assert n_cells is None or p['tab_n'][0] == n_cells, (name, p['tab_n'])
    _full(domain, trials, 1, C, gamma, info)               # (the pools grow to this level: growth is a miss)
    monkeypatch.setenv('TPE_FAST_IMAGE', '0')
    s0 = _stats()
    ref = [_full(domain, trials, s, C, gamma, info) for s in SEEDS]
    d = _delta(s0, _stats())
    assert d['misses'] == 1 and d['hits'] == len(SEEDS) - 1 and d['fused'] == 0, d
    monkeypatch.delenv('TPE_FAST_IMAGE')
    s1 = _stats()
    got = [_full(domain, trials, s, C, gamma, info) for s in SEEDS]
    d = _delta(s1, _stats())
    assert got == ref
    assert d['misses'] == 1 and d['fused'] == d['hits'] == len(SEEDS) - 1 and d['fallbacks'] == 0, d
