"""GPU tests of the wide mixed joint stage (tpe_joint_wide_mixed_run through
Engine.run_joint_wide_mixed) and of tpe.suggest(..., joint=True, joint_wide=True,
joint_discrete=True, joint_wide_mixed=True), against the float64 model restated
in numpy (tests/joint_mixed_ref.py).

Tolerances are the project's (tests/joint_ref.py, tests/test_gpu_joint_mixed.py):
l and g within 1e-5 * max(1, |ref|) (check_lpdf); the winner inside
joint_ref.tie_set, which may hold at most 8 distinct vectors, at the lowest index
holding its vector; sampled frequencies within 5 binomial standard deviations.
"""
import functools

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_ref as R
from tests import joint_report_ref as RR

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # distinct vectors: a plateau of near-equal scores must not hide a wrong winner
WIDE = 64             # TPE_JOINT_WIDE_MAX_DIMS: the record's z


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def mixed_candidates(below, low, high, psig, ps, C, seed, n_far=32):
    """tests/test_gpu_joint_mixed.py's recipe: the continuous coordinates as
    test_gpu_joint._candidates draws them, categories appended — the eighth
    drawn around below components carries its component's categories (random
    ones for the prior row), the rest uniform random categories.  Returns f32
    [C, Dc + Dk]."""
    rs = np.random.RandomState(seed)
    w, mu, sigma, xc = below
    Dc = mu.shape[1]
    n_near = C // 8
    k = rs.choice(len(w), size=n_near, p=w)
    near = mu[k] + sigma[k] * rs.standard_normal((n_near, Dc))
    bounded = np.isfinite(low)
    wide = np.where(bounded[None, :], rs.uniform(-10, 10, (C - n_near, Dc)), rs.normal(1.0, 4.0, (C - n_near, Dc)))
    z = np.vstack([near, wide])
    free = np.flatnonzero(~bounded)
    if len(free) and n_far:
        d = free[0]
        z[-n_far:, d] = mu[:, d].max() + 40.0 * psig[d] + rs.uniform(0, 1, n_far)
    z = z.astype(np.float32)
    lo32 = np.where(bounded, low, -np.inf).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, high, np.inf).astype(np.float32), np.float32(-np.inf))
    z = np.clip(z, lo32[None, :], hi32[None, :])
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1)
    vk = xc[k]
    v[:n_near] = np.where(vk >= 0, vk, v[:n_near])
    return np.hstack([z, v.astype(np.float32)])


def ref_lg(cand, Dc, below, above, low, high, ps, sb, sa):
    """The float64 l and g of f32 candidates [C, Dc + Dk] (blocks sized so that
    the reference's [block, K, Dc] temporary stays near 100 MB)."""
    z64, v = cand[:, :Dc].astype(np.float64), cand[:, Dc:].astype(np.int64)
    block = max(64, min(2048, (1 << 24) // (max(len(below[0]), len(above[0])) * max(Dc, 1))))
    return (M.ref_mixed_lpdf(z64, v, below, low, high, ps, sb, block=block),
            M.ref_mixed_lpdf(z64, v, above, low, high, ps, sa, block=block))


def check_winner(rec, cand, l_ref, g_ref, D, what):
    """The winner's vector is in the tie set (at most MAX_TIES distinct vectors)
    and its index the lowest one holding that vector; the record carries the
    vector in its first D entries and zeros after."""
    ties, score = R.tie_set(l_ref, g_ref)
    idx = int(rec['global_idx'])
    distinct = np.unique(cand[ties], axis=0)
    print('%s: winner %d, argmax %d, %d ties, %d distinct' % (what, idx, int(np.argmax(score)), len(ties),
                                                             len(distinct)))
    assert len(distinct) <= MAX_TIES, (what, len(distinct))
    same = np.flatnonzero((cand == cand[idx][None, :]).all(axis=1))
    assert np.isin(same, ties).any(), (what, idx, int(np.argmax(score)), ties[:10])
    assert idx == int(same[0]), (what, idx, same[:10])
    if len(distinct) == 1:
        assert idx == int(np.argmax(score))
    assert rec['z'].shape == (WIDE,)
    np.testing.assert_array_equal(rec['z'][:D], cand[idx].astype(np.float64))
    assert (rec['z'][D:] == 0).all()


@functools.lru_cache(maxsize=None)
def _case(Dc, us, n, seed=None):
    below, above, low, high, pmu, psig, ps, sb, sa, _ = M.seeded_mixed_case(Dc, list(us), n, seed)
    return below, above, low, high, psig, ps, sb, sa


@functools.lru_cache(maxsize=None)
def _injected(Dc, us, n, C=4096):
    """(cand, l_ref, g_ref) of an injected-scoring case: computed once, read only."""
    below, above, low, high, psig, ps, sb, sa = _case(Dc, us, n)
    cand = mixed_candidates(below, low, high, psig, ps, C, Dc + len(us))
    l_ref, g_ref = ref_lg(cand, Dc, below, above, low, high, ps, sb, sa)
    for a in (cand, l_ref, g_ref):
        a.setflags(write=False)
    return cand, l_ref, g_ref


def _run(engine, case, ids, C, seed, **kw):
    below, above, low, high, psig, ps, sb, sa = case
    return engine.run_joint_wide_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), ids, C,
                                       seed, **kw)


# ------------------------------------------------------- 1. injected scoring
CASES = [
    (16, (3,), 60),                              # 17: the smallest wide mixed group; DP 16, KP 1
    (9, (2, 3, '5p', 17, 2, 3, 4, 7), 120),      # 17: DP 12, KP 8
    (17, (2, '5p', 4), 300),                     # 20: DP 20, KP 4 with a padded slot; 296 above components
    (21, (2, 3, '5p', 17, 2, 3, 4, 7), 120),     # 29: DP 24, KP 8
    (30, (4, '5p'), 60),                         # 32: DP 32, KP 2
    (44, (3, 2, 2, 4), 200),                     # 48: DP 48, R = 1; 197 above components wrap the 80-tile
    (56, (2, 3, '5p', 17, 2, 3, 4, 7), 90),      # 64: DP 64, KP 8
    (63, (5,), 300),                             # 64: DP 64 with a padded continuous slot
    (13, (3, 4), 4000),                          # 15: many tiles
]


@pytest.mark.parametrize('Dc,us,n', CASES)
def test_scoring_of_injected_wide_mixed_candidates(engine, Dc, us, n):
    """l, g and the winner of 4096 given candidates at every padded continuous
    width, every padded discrete width, both tile sizes wrapping, a padded slot
    of either kind, and a narrow group of many tiles."""
    case = _case(Dc, us, n)
    below, above = case[0], case[1]
    cand, l_ref, g_ref = _injected(Dc, us, n)
    D, C = Dc + len(us), len(cand)
    if (Dc, n) == (17, 300):
        assert len(above[0]) == 296
    if (Dc, n) == (44, 200):
        assert len(above[0]) == 197
    rec, l, g = _run(engine, case, [7], C, 3, inject=cand.copy(), want_lg=True)   # (the shared array stays read-only)
    what = 'Dc=%d us=%s n=%d' % (Dc, list(us), n)
    assert rec.dtype.itemsize == 24 + 8 * WIDE
    assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(g[0]))          # the far candidates too: no -inf
    assert np.all(np.isfinite(l_ref)) and np.all(np.isfinite(g_ref))
    R.check_lpdf(l[0], l_ref, 'l ' + what)
    R.check_lpdf(g[0], g_ref, 'g ' + what)
    far = slice(C - 32, C)
    assert np.all(g_ref[far] < -700) or np.all(l_ref[far] < -700)          # they are beyond a fixed shift's reach
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_winner(rec[0], cand, l_ref, g_ref, D, what)


# ------------------------------------------------ 2. against the narrow stage
def test_narrow_group_draws_the_mixed_stage_candidates(engine):
    """At Dc + Dk <= 16 the stage draws tpe_joint_mixed_run's candidates byte for
    byte (same seed and id); l and g are the densities of those vectors and the
    winner np.argmax of the stage's own scores."""
    Dc, us, C = 9, (2, '5p', 4), 4096
    case = _case(Dc, us, 60)
    below, above, low, high, psig, ps, sb, sa = case
    rec, cand, l, g = _run(engine, case, [11], C, 42, return_cand=True, want_lg=True)
    _, narrow = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [11], C,
                                       seed=42, return_cand=True)
    assert cand.shape == narrow.shape == (1, C, 12) and cand.tobytes() == narrow.tobytes()
    l_ref, g_ref = ref_lg(cand[0], Dc, below, above, low, high, ps, sb, sa)
    R.check_lpdf(l[0], l_ref, 'l narrow')
    R.check_lpdf(g[0], g_ref, 'g narrow')
    i = int(rec['global_idx'][0])
    assert i == int(np.argmax(l[0] - g[0]))
    np.testing.assert_array_equal(rec['z'][0, :12], cand[0][i].astype(np.float64))
    assert (rec['z'][0, 12:] == 0).all()


# -------------------------------------------------- 3. against the wide stage
@pytest.mark.parametrize('Dc,us', [(17, (3, '5p')), (49, (2, 4))])
def test_continuous_coordinates_are_the_wide_stage_draws(engine, Dc, us):
    """The continuous columns equal run_joint_wide's over the continuous part
    byte for byte; the categories (words 1 + Dc ...: at Dc = 49 from Philox
    block 12) are integral, in range and all turn up; l, g are the densities of
    the returned vectors."""
    C = 4096
    case = _case(Dc, us, 60)
    below, above, low, high, psig, ps, sb, sa = case
    rec, cand, l, g = _run(engine, case, [11], C, 42, return_cand=True, want_lg=True)
    _, cont = engine.run_joint_wide(below[:3], above[:3], low, high, [11], C, seed=42, return_cand=True)
    assert cand.shape == (1, C, Dc + len(us))
    z, vf = cand[0][:, :Dc], cand[0][:, Dc:]
    assert np.ascontiguousarray(z).tobytes() == cont[0].tobytes()
    v = vf.astype(np.int64)
    assert (v == vf).all()
    for d, p in enumerate(ps):
        assert v[:, d].min() >= 0 and v[:, d].max() < len(p)
        assert len(np.unique(v[:, d])) == len(p)             # 4096 draws: every category (p >= 0.05) turns up
    l_ref, g_ref = ref_lg(cand[0], Dc, below, above, low, high, ps, sb, sa)
    R.check_lpdf(l[0], l_ref, 'l Dc=%d' % Dc)
    R.check_lpdf(g[0], g_ref, 'g Dc=%d' % Dc)
    i = int(rec['global_idx'][0])
    assert i == int(np.argmax(l[0] - g[0]))
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    np.testing.assert_array_equal(rec['z'][0, :Dc + len(us)], cand[0][i].astype(np.float64))
    assert (rec['z'][0, Dc + len(us):] == 0).all()


# ------------------------------------- 4. sampling follows the below mixture
def test_wide_mixed_sampling_follows_the_below_mixture(engine):
    Dc, us, C = 17, (3, '5p'), 1 << 16
    case = _case(Dc, us, 60)
    below, ps, sb = case[0], case[5], case[6]
    _, cand = _run(engine, case, [0], C, 99, return_cand=True)
    vf = cand[0][:, Dc:]
    v = vf.astype(np.int64)
    assert (v == vf).all()
    for d, p in enumerate(ps):
        assert v[:, d].min() >= 0 and v[:, d].max() < len(p)
        want = M.marginal(below, d, p, sb[d])
        assert abs(want.sum() - 1.0) < 1e-12
        freq = np.bincount(v[:, d], minlength=len(p)) / C
        sd = np.sqrt(want * (1 - want) / C)
        print('dimension %d: (freq - p) / sd = %s' % (d, np.round((freq - want) / sd, 2)))
        assert (np.abs(freq - want) <= 5 * sd).all(), (d, freq, want)


def test_one_component_per_wide_mixed_vector(engine):
    """test_one_component_per_mixed_vector's construction with 16 more continuous
    dimensions copied from the first: two components of weight 1/2, (-3 ...,
    category 0) and (+3 ..., category 1), sigma 0.25, s = 1e-3.  The category
    comes from the vector's OWN component, so it disagrees with the sign of z
    only when the smoothing mass draws the other category: s / (1 + s) / 2 of the
    vectors; and all 17 coordinates of a vector have one sign."""
    C, s, Dc = 1 << 16, 1e-3, 17
    w = np.array([0.5, 0.5])
    mu = np.repeat(np.array([[-3.0], [3.0]]), Dc, axis=1)
    sigma = np.full((2, Dc), 0.25)
    above = (np.array([1.0]), np.zeros((1, Dc)), np.full((1, Dc), 5.0))
    cats = [(np.array([0, 1]), np.array([-1]), np.array([0.5, 0.5]), s, s)]
    inf = np.full(Dc, np.inf)
    rec, cand = engine.run_joint_wide_mixed((w, mu, sigma), above, -inf, inf, cats, [3], C, seed=5, return_cand=True)
    z, v = cand[0][:, :Dc], cand[0][:, Dc]
    assert np.isin(v, [0.0, 1.0]).all() and np.all(np.abs(np.abs(z) - 3.0) < 3.0)
    assert ((z > 0) == (z[:, :1] > 0)).all()
    p = 0.5 * s / (1 + s)
    frac = float(np.mean((z[:, 0] > 0) != (v == 1)))
    print('off-component categories: %.3e of the vectors, expected %.3e' % (frac, p))
    assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / C)
    assert abs(float(np.mean(z[:, 0] > 0)) - 0.5) <= 5 * np.sqrt(0.25 / C)


# ------------------------------------------------ 5. determinism and batching
def test_wide_mixed_determinism_and_batching(engine):
    """The same call twice gives the same bytes; ids [5, 9, 12] in one call are
    three single calls; 4097 candidates leave a ragged last chunk at R = 2."""
    C, Dc, us = 4096 + 1, 17, (3, '5p')
    case = _case(Dc, us, 60)
    ids = [5, 9, 12]
    a = _run(engine, case, ids, C, 17, return_cand=True, want_lg=True)
    b = _run(engine, case, ids, C, 17, return_cand=True, want_lg=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, Dc + 2) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    for j, new_id in enumerate(ids):
        s = _run(engine, case, [new_id], C, 17, return_cand=True, want_lg=True)
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    other = _run(engine, case, ids, C, 18, return_cand=True)
    assert other[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------------ 6. report
def test_wide_mixed_report(engine):
    """report_k = 4: entry 0 is the record's vector, the vectors are distinct and
    ranked, and they are the numpy ranking of the returned cand, l, g."""
    Dc, us, C, K = 17, (2, '5p', 4), 4096, 4
    D = Dc + len(us)
    rec, cand, l, g, top, z, n_top, stats = _run(engine, _case(Dc, us, 300), [7], C, 17, return_cand=True,
                                                 want_lg=True, report_k=K)
    assert top.shape == (1, K) and z.shape == (1, K, D) and n_top.tolist() == [K]
    RR.check_report(cand[0], l[0], g[0], K, top[0], z[0], n_top[0], stats[0], 'wide mixed report')
    assert rec['global_idx'][0] == top['idx'][0, 0]
    assert rec['l'][0] == top['l'][0, 0] and rec['g'][0] == top['g'][0, 0]
    assert rec['z'][0, :D].tobytes() == z[0][0].astype(np.float64).tobytes()
    assert len(np.unique(z[0], axis=0)) == K
    score = top['l'][0] - top['g'][0]
    assert (np.diff(score) <= 0).all()
    for j in range(K):
        assert z[0][j].tobytes() == cand[0][int(top['idx'][0, j])].tobytes()
    only = _run(engine, _case(Dc, us, 300), [7], C, 17, report_k=K)
    assert len(only) == 5 and only[1].tobytes() == top.tobytes() and only[2].tobytes() == z.tobytes()


# ------------------------------------------------------------ 7. public path
KW = dict(joint=True, joint_wide=True, joint_discrete=True, joint_wide_mixed=True)


@functools.lru_cache(maxsize=None)
def _public_case():
    """A network space: 18 continuous knobs, an optimizer choice and an
    activation pchoice (joined), a quantised label and a gate with a conditional
    child (univariate).  60 trials; the loss couples the optimizer with lr."""
    from hyperopt_amd import base, hp, rand
    space = {'w%02d' % i: (hp.loguniform('w%02d' % i, -6, 0) if i % 3 == 0 else hp.uniform('w%02d' % i, -5, 5))
             for i in range(18)}
    space.update({'opt': hp.choice('opt', ['adam', 'sgd', 'rmsprop']),
                  'act': hp.pchoice('act', [(0.7, 'relu'), (0.3, 'gelu')]),
                  'q': hp.quniform('q', 0, 10, 1),
                  'gate': hp.choice('gate', [0, {'k': hp.uniform('inner', 0, 1)}])})
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        target = [-4.0, -1.0, -2.5][int(v['opt'])]
        loss = (np.log(float(v['w00'])) - target) ** 2 + 0.1 * sum(float(v['w%02d' % i]) ** 2 for i in (1, 2, 4)) \
            + 0.2 * int(v['act']) + 0.05 * float(v['q']) + 0.3 * float(v.get('inner', 0.5)) + 1e-3 * tid
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_joint_wide_mixed_suggest():
    from hyperopt_amd import history, joint as J, tpe
    from hyperopt_amd.engine import get_engine
    domain, trials = _public_case()
    table = domain.table
    C, seed, ids = 4096, 321, [60, 61]
    crows = [r for r in table.rows if r.label.startswith('w')]
    drows = [table.by_label['act'], table.by_label['opt']]
    drows.sort(key=lambda r: r.index)
    group = crows + drows                                    # kernel coordinates: continuous, then discrete
    assert len(crows) == 18 and [r.index for r in crows] == sorted(r.index for r in crows)
    joined = [r.label for r in group]

    plain = [_vals(d) for d in tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C)]
    docs = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, **KW)
    hist = history.extract(domain, trials)
    model = J.fit_mixed_model(crows, drows, hist, history.split_below(hist, tpe._default_gamma),
                              tpe._default_prior_weight, tpe.DEFAULT_LF)
    rec = get_engine().run_joint_wide_mixed(model.below[:3], model.above[:3], model.low, model.high, model.cats(),
                                            ids, C, seed)
    assert (rec['global_idx'] >= 0).all()
    want = model.values(rec['z'][:, :len(group)])
    choices = tpe.suggest_choices(table, hist, ids, seed, n_EI_candidates=C, **KW)
    for j, doc in enumerate(docs):
        trials.assert_valid_trial(doc)
        got = _vals(doc)
        assert set(got) == set(plain[j])
        for d, r in enumerate(group):                       # the joined labels: the stage's winner through the model
            typed = np.int64(int(want[j, d])) if r.categorical else np.float64(want[j, d])
            assert type(got[r.label]) is type(typed) and got[r.label].tobytes() == typed.tobytes(), r.label
        for r in crows:
            assert type(got[r.label]) is np.float64
        for r in drows:
            assert type(got[r.label]) is np.int64 and 0 <= got[r.label] < int(r.args['upper'])
        for k in got:                                       # not joined: the bytes of the call without joint
            if k not in joined:
                assert type(got[k]) is type(plain[j][k]) and np.asarray(got[k]).tobytes() == \
                    np.asarray(plain[j][k]).tobytes(), k
        assert {'q', 'gate'} <= set(got) - set(joined)
        assert set(k for k, v in choices[j].items() if v is not None) == set(got)
        for k, v in got.items():
            assert type(choices[j][k]) is type(v) and choices[j][k] == v, k

    rep = tpe.joint_candidate_report(ids[0], domain, trials, seed, k=4, n_EI_candidates=C, **KW)
    assert len(rep) == 1
    gr = rep[0]
    assert gr.condition is None and list(gr.labels) == joined and gr.n_top == 4
    first = _vals(docs[0])
    for d, lab in enumerate(joined):
        assert float(gr.vectors[0][d]) == float(first[lab]), lab
    assert int(gr.top['index'][0]) == int(rec['global_idx'][0])
