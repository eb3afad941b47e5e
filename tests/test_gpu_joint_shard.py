"""GPU tests of the sharded joint stage (tpe_joint_run_shard through the
``shard=`` keyword of Engine.run_joint*; DESIGN.md "Sharded joint stage"), one
process, one device.

Everything here is byte equality, no tolerance: a candidate is a function of
(seed, stream word, new id, global index) alone, so a part's candidates, l and
g are the unsharded arrays' slices, and joint.combine_records over the parts'
winner records is the unsharded record.  What the unsharded stages compute is
checked against the float64 models elsewhere (tests/test_gpu_joint*.py)."""
import functools

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

C = 2 * 1024 + 37     # three chunks, the last ragged
W = 3                 # parts at 0, 695, 1390: no base a multiple of 2, a chunk straddles every cut
IDS = [7, 1000003]
SEED = 17
# (new id, segment) of the segmented stages
SEG_PROBLEMS = [(7, 0), (9, 1), (7, 2), (12, 1), (3, 0)]
MSEG_PROBLEMS = [(9, 2), (5, 0), (9, 1), (40, 2)]


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def _ranges(n, world):
    from hyperopt_amd import dist
    return [dist.shard_range(n, r, world) for r in range(world)]


# ------------------------------------------------------------------ the stages
# A stage is run(engine, n_cand, seed, shard) -> (records [P], cand, l [P, n], g
# [P, n]); cand is f32 [P, n, D], or a list of P arrays [n, D_p] (segmented).
@functools.lru_cache(maxsize=None)
def _quant_model(Dc, us, Vs, n):
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, list(us), list(Vs), n)
    cats = M.cats_of(below, above, ps, sb, sa) if us else []
    return below[:3], above[:3], low, high, cats, Q.quants_of(below, above, edges)


@functools.lru_cache(maxsize=None)
def _mixed_model(Dc, us, n):
    below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, list(us), n)
    return below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa)


@functools.lru_cache(maxsize=None)
def _cont_model(D, n, seed):
    return R.seeded_case(D, n, seed)[:4]


def _continuous(engine, n, seed, shard, **kw):
    return engine.run_joint(*_cont_model(4, 40, 404), IDS, n, seed, return_cand=True, want_lg=True, shard=shard, **kw)


def _wide(engine, n, seed, shard, **kw):
    return engine.run_joint_wide(*_cont_model(20, 40, 420), IDS, n, seed, return_cand=True, want_lg=True, shard=shard,
                                 **kw)


def _mixed(engine, n, seed, shard, **kw):
    return engine.run_joint_mixed(*_mixed_model(2, (3,), 40), IDS, n, seed, return_cand=True, want_lg=True,
                                  shard=shard, **kw)


def _quant(engine, n, seed, shard, **kw):
    """1 + 1 + 1 coordinates, 300 trials: the above side's table (296
    components) streams through several LDS tiles."""
    model = _quant_model(1, (3,), (50,), 300)
    assert len(model[1][0]) > 2 * 128
    return engine.run_joint_quant(*model, IDS, n, seed, return_cand=True, want_lg=True, shard=shard, **kw)


def _segments(engine, n, seed, shard, **kw):
    """Three continuous segments of three kernel classes (2, 5 and 9
    dimensions: DP 2, 6 and 12) over five problems."""
    models = [_cont_model(2, 40, 502), _cont_model(5, 40, 505), _cont_model(9, 40, 509)]
    words = [0xFFFFFFFE - 3 * s for s in range(3)]
    return engine.run_joint_segments(models, words, [p[1] for p in SEG_PROBLEMS], [p[0] for p in SEG_PROBLEMS], n, seed,
                                     return_cand=True, want_lg=True, shard=shard, **kw)


def _msegments(engine, n, seed, shard, **kw):
    """The mixed segmented stage, one segment of each kind: 3 continuous; 2
    continuous + 1 discrete; 1 continuous + 1 discrete + 1 quantised."""
    models = [_cont_model(3, 40, 603), _mixed_model(2, (3,), 40), _quant_model(1, (3,), (50,), 40)]
    words = [0xFFFFFFFE - 5 * s for s in range(3)]
    return engine.run_joint_segments(models, words, [p[1] for p in MSEG_PROBLEMS], [p[0] for p in MSEG_PROBLEMS], n,
                                     seed, return_cand=True, want_lg=True, shard=shard, **kw)


STAGES = dict(continuous=_continuous, wide=_wide, mixed=_mixed, quant=_quant, segments=_segments,
              msegments=_msegments)


@pytest.fixture(scope='module')
def whole(engine):
    """The unsharded run of every stage over C candidates (computed once, shared, not modified)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = STAGES[name](engine, C, SEED, None)
        return cache[name]
    return get


def _cand_slice(cand, lo, hi):
    return [c[lo:hi] for c in cand] if isinstance(cand, list) else cand[:, lo:hi]


def _same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_parts(run, engine, full, n, world, seed=SEED):
    """Every part of the partition of n over ``world``: its arrays are the
    unsharded slices, and the combined records the unsharded records."""
    from hyperopt_amd import joint as J
    rec, cand, l, g = full
    recs = []
    for lo, hi in _ranges(n, world):
        prec, pcand, pl, pg = run(engine, hi - lo, seed, (lo, n))
        assert _same(pcand, _cand_slice(cand, lo, hi)), (lo, hi)
        assert _same(pl, l[:, lo:hi]) and _same(pg, g[:, lo:hi]), (lo, hi)
        inside = prec['global_idx'] >= 0
        assert inside.all() == (hi > lo) and not (inside.any() and hi == lo)
        assert ((prec['global_idx'][inside] >= lo) & (prec['global_idx'][inside] < hi)).all()
        recs.append(prec)
    got = J.combine_records(np.stack(recs))
    assert got.dtype == rec.dtype and got.tobytes() == rec.tobytes()
    return recs


# ------------------------------------------------------- partition invariance
@pytest.mark.parametrize('name', sorted(STAGES))
def test_parts_are_the_unsharded_slices_and_combine_to_the_unsharded_records(name, engine, whole):
    assert [lo for lo, hi in _ranges(C, W)] == [0, 695, 1390]
    full = whole(name)
    assert (full[0]['global_idx'] >= 0).all()
    _check_parts(STAGES[name], engine, full, C, W)


def test_winners_of_eight_seeds_fall_in_several_parts(engine):
    """The continuous stage's records over 8 seeds: combined = unsharded, and the
    winners do not all sit in one part (or the combine would prove nothing)."""
    from hyperopt_amd import joint as J
    homes = set()
    for seed in range(100, 108):
        rec = engine.run_joint(*_cont_model(4, 40, 404), IDS, C, seed)
        parts = [engine.run_joint(*_cont_model(4, 40, 404), IDS, hi - lo, seed, shard=(lo, C))
                 for lo, hi in _ranges(C, W)]
        assert J.combine_records(np.stack(parts)).tobytes() == rec.tobytes(), seed
        homes.update(int(np.searchsorted([695, 1390], i, side='right')) for i in rec['global_idx'])
    assert len(homes) >= 2, homes


@pytest.mark.parametrize('name', sorted(STAGES))
def test_empty_parts(name, engine):
    """3 candidates over 5 ranks: two ranges are empty, the engine returns empty
    records for them without a native call, and the combine still gives the
    unsharded records."""
    ranges = _ranges(3, 5)
    assert sum(lo == hi for lo, hi in ranges) == 2
    run = STAGES[name]
    full = run(engine, 3, SEED, None)
    recs = _check_parts(run, engine, full, 3, 5)
    for (lo, hi), prec in zip(ranges, recs):
        if lo == hi:
            assert (prec['global_idx'] == -1).all() and not prec['l'].any() and not prec['g'].any() \
                and not prec['z'].any()


def test_cross_shard_ties_go_to_the_first_occurrence(engine):
    """No continuous label and two discrete ones (U = 2 and 3): six distinct
    vectors among 2085 candidates, so the best score occurs in every part; the
    combined winner is the unsharded one, its first occurrence."""
    from hyperopt_amd import joint as J
    model = _mixed_model(0, (2, 3), 40)

    def run(engine, n, seed, shard):
        return engine.run_joint_mixed(*model, IDS, n, seed, return_cand=True, want_lg=True, shard=shard)
    full = run(engine, C, SEED, None)
    rec, cand, l, g = full
    score = l - g
    for j in range(len(IDS)):
        assert len(set(map(tuple, cand[j].tolist()))) <= 6
        best = score[j] == score[j].max()
        assert rec['global_idx'][j] == np.flatnonzero(best)[0]
        for lo, hi in _ranges(C, W):
            assert best[lo:hi].any(), (j, lo, hi)      # a tie across every cut
    recs = _check_parts(run, engine, full, C, W)
    got = J.combine_records(np.stack(recs[::-1]))      # (whatever the order of the parts)
    assert got.tobytes() == rec.tobytes()


# -------------------------------------------------------------------- high base
@pytest.mark.parametrize('name', ['continuous', 'wide'])
def test_the_last_300_candidates_below_2_to_the_31(name, engine):
    """n_cand_global = 2^31 - 1, base 2^31 - 301: the ragged chunk's lanes past
    the part's end form indices beyond 2^31.  One part of 300 and two of 150
    give the same candidates, l and g and the same winner; every value is
    finite and inside the bounds."""
    from hyperopt_amd import joint as J
    G = 2 ** 31 - 1
    base = G - 300
    run = STAGES[name]
    rec, cand, l, g = run(engine, 300, SEED, (base, G))
    a = run(engine, 150, SEED, (base, G))
    b = run(engine, 150, SEED, (base + 150, G))
    assert _same(np.concatenate([a[1], b[1]], axis=1), cand)
    assert _same(np.concatenate([a[2], b[2]], axis=1), l) and _same(np.concatenate([a[3], b[3]], axis=1), g)
    assert J.combine_records(np.stack([a[0], b[0]])).tobytes() == rec.tobytes()
    assert ((rec['global_idx'] >= base) & (rec['global_idx'] < G)).all()
    assert ((a[0]['global_idx'] < base + 150) & (b[0]['global_idx'] >= base + 150)).all()
    low, high = _cont_model(4, 40, 404)[2:] if name == 'continuous' else _cont_model(20, 40, 420)[2:]
    assert np.isfinite(cand).all() and np.isfinite(l).all() and np.isfinite(g).all()
    assert (cand >= low[None, None, :]).all() and (cand < high[None, None, :]).all()
    # the winner is the argmax of the part's own scores
    for j in range(len(IDS)):
        i = int(np.argmax(l[j] - g[j]))
        assert rec['global_idx'][j] == base + i
        np.testing.assert_array_equal(rec['z'][j, :cand.shape[2]], cand[j, i].astype(np.float64))
    # and these are other candidates than those at the low end of the range
    low_end = run(engine, 300, SEED, (0, G))
    assert low_end[1].tobytes() != cand.tobytes()


# ------------------------------------------------- the existing entry points
@pytest.mark.parametrize('name', sorted(STAGES))
def test_shard_0_C_is_the_call_without_shard(name, engine, whole):
    full = whole(name)
    again = STAGES[name](engine, C, SEED, (0, C))
    for x, y in zip(full, again):
        assert _same(x, y)


def test_report_and_inject_need_base_zero(engine):
    model = _cont_model(4, 40, 404)
    inj = np.zeros((8, 4), dtype=np.float32)
    with pytest.raises(ValueError, match='report_k'):
        engine.run_joint(*model, IDS, 8, SEED, report_k=2, shard=(1, 9))
    with pytest.raises(ValueError, match='inject'):
        engine.run_joint(*model, IDS, 8, SEED, inject=inj, shard=(1, 9))
    a = engine.run_joint(*model, IDS, 8, SEED, inject=inj, shard=(0, 9), want_lg=True)
    b = engine.run_joint(*model, IDS, 8, SEED, inject=inj, want_lg=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
