"""GPU tests of the mixed joint stage (tpe_joint_mixed_run through
Engine.run_joint_mixed) and of tpe.suggest(..., joint=..., joint_discrete=True),
against the float64 model restated in numpy (tests/joint_mixed_ref.py).

Tolerances are the project's (tests/test_gpu_kernels.py, tests/test_gpu_joint.py):
l and g within 1e-5 * max(1, |ref|); the winner inside joint_ref.tie_set, which
may hold at most 8 distinct vectors; sampled frequencies within 5 binomial
standard deviations.
"""
import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # distinct vectors: a plateau of near-equal scores must not hide a wrong winner


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


def mixed_candidates(below, low, high, psig, ps, C, seed, n_far=32):
    """test_gpu_joint._candidates' recipe for the continuous coordinates (the
    same draws in the same order) with categories appended: the eighth drawn
    around below components carries its component's categories (random ones for
    the prior row), the rest uniform random categories.  Returns f32 [C, Dc + Dk]."""
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


def check_mixed_winner(rec, cand, l_ref, g_ref, D, what):
    """The winner's vector is in the tie set (at most MAX_TIES distinct vectors)
    and its index the lowest one holding that vector: identical candidates
    score identically."""
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
    np.testing.assert_array_equal(rec['z'][:D], cand[idx].astype(np.float64))
    assert (rec['z'][D:] == 0).all()


CASES = [(2, [3], 60), (0, [3, '5p'], 40), (3, [2, '5p', 17], 300), (8, [2, 3, '5p', 17, 2, 3, 4, 7], 120),
         (1, [4], 3013)]


def injected_case(Dc, us, n, C=4096):
    """(below, above, low, high, ps, s_below, s_above, cand, l_ref, g_ref) of an injected-scoring case."""
    below, above, low, high, pmu, psig, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, n)
    cand = mixed_candidates(below, low, high, psig, ps, C, Dc + len(us))
    z64, v = cand[:, :Dc].astype(np.float64), cand[:, Dc:].astype(np.int64)
    l_ref = M.ref_mixed_lpdf(z64, v, below, low, high, ps, sb)
    g_ref = M.ref_mixed_lpdf(z64, v, above, low, high, ps, sa)
    return below, above, low, high, ps, sb, sa, cand, l_ref, g_ref


@pytest.mark.parametrize('Dc,us,n', CASES)
def test_scoring_of_injected_mixed_candidates(engine, Dc, us, n):
    """l, g and the winner of 4096 given candidates: an all-discrete group, a
    pchoice prior, 16 coordinates, and above sides of 296 and 3000 components
    (the LDS tile loop wraps)."""
    below, above, low, high, ps, sb, sa, cand, l_ref, g_ref = injected_case(Dc, us, n)
    D, C = Dc + len(us), len(cand)
    if n == 300:
        assert len(above[0]) == 296
    if n == 3013:
        assert len(above[0]) == 3000
    rec, l, g = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [7], C,
                                       seed=3, inject=cand, want_lg=True)
    what = 'Dc=%d us=%s n=%d' % (Dc, us, n)
    assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(g[0]))          # the far candidates too: no -inf
    R.check_lpdf(l[0], l_ref, 'l ' + what)
    R.check_lpdf(g[0], g_ref, 'g ' + what)
    if Dc >= 2:
        far = slice(C - 32, C)
        assert np.all(g_ref[far] < -700) or np.all(l_ref[far] < -700)      # they are beyond a fixed shift's reach
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_mixed_winner(rec[0], cand, l_ref, g_ref, D, what)


def test_scoring_with_more_than_eight_discrete_labels(engine):
    """Nine discrete labels take the 16-slot discrete instantiation (seven of
    its slots padded: bonus 0, category -1)."""
    Dc, us, n = 2, [2, 3, 2, '5p', 2, 3, 4, 3, 2], 60
    below, above, low, high, ps, sb, sa, cand, l_ref, g_ref = injected_case(Dc, us, n)
    D, C = Dc + len(us), len(cand)
    rec, l, g = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa), [7], C,
                                       seed=3, inject=cand, want_lg=True)
    R.check_lpdf(l[0], l_ref, 'l 2 + 9')
    R.check_lpdf(g[0], g_ref, 'g 2 + 9')
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_mixed_winner(rec[0], cand, l_ref, g_ref, D, '2 + 9')


@pytest.mark.parametrize('Dc,us', [(5, [3]), (9, [2, '5p', 4])])
def test_continuous_coordinates_past_the_first_philox_block(engine, Dc, us):
    """From the fourth coordinate on the words come from Philox blocks 1, 2, ...:
    the continuous coordinates still equal the continuous stage's byte for
    byte, the categories (words 1 + Dc ...) are in range, and l, g are the
    densities of the returned vectors.  (9, ...) is a 16-slot continuous
    instantiation."""
    C = 4096
    below, above, low, high, pmu, psig, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, 60)
    rec, cand, l, g = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                             [11], C, seed=42, return_cand=True, want_lg=True)
    _, cont = engine.run_joint(below[:3], above[:3], low, high, [11], C, seed=42, return_cand=True)
    z, vf = cand[0][:, :Dc], cand[0][:, Dc:]
    assert np.ascontiguousarray(z).tobytes() == cont[0].tobytes()
    v = vf.astype(np.int64)
    assert (v == vf).all()
    for d, p in enumerate(ps):
        assert v[:, d].min() >= 0 and v[:, d].max() < len(p)
        assert len(np.unique(v[:, d])) == len(p)             # 4096 draws: every category (p >= 0.05) turns up
    z64 = z.astype(np.float64)
    R.check_lpdf(l[0], M.ref_mixed_lpdf(z64, v, below, low, high, ps, sb), 'l Dc=%d' % Dc)
    R.check_lpdf(g[0], M.ref_mixed_lpdf(z64, v, above, low, high, ps, sa), 'g Dc=%d' % Dc)
    i = int(rec['global_idx'][0])
    assert i == int(np.argmax(l[0] - g[0]))
    np.testing.assert_array_equal(rec['z'][0, :Dc + len(us)], cand[0][i].astype(np.float64))


def test_mixed_sampling_follows_the_below_mixture(engine):
    """2^18 sampled vectors: categories in range with the mixture's marginals,
    the continuous coordinates those of the continuous stage (same seed and id)
    byte for byte, l and g the densities of the returned vectors."""
    Dc, us, C = 2, [3, '5p'], 1 << 18
    below, above, low, high, pmu, psig, ps, sb, sa, _ = M.seeded_mixed_case(Dc, us, 60)
    rec, cand, l, g = engine.run_joint_mixed(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                             [0], C, seed=99, return_cand=True, want_lg=True)
    assert cand.shape == (1, C, 4)
    z, vf = cand[0][:, :Dc], cand[0][:, Dc:]
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
    _, cont = engine.run_joint(below[:3], above[:3], low, high, [0], C, seed=99, return_cand=True)
    assert np.ascontiguousarray(z).tobytes() == cont[0].tobytes()
    sub = slice(0, C, 16)                      # (the density check on every 16th vector: 2^14 of them)
    z64 = z[sub].astype(np.float64)
    R.check_lpdf(l[0][sub], M.ref_mixed_lpdf(z64, v[sub], below, low, high, ps, sb), 'sampled l')
    R.check_lpdf(g[0][sub], M.ref_mixed_lpdf(z64, v[sub], above, low, high, ps, sa), 'sampled g')
    i = int(rec['global_idx'][0])
    np.testing.assert_array_equal(rec['z'][0, :4], cand[0][i].astype(np.float64))
    assert (rec['z'][0, 4:] == 0).all()
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    assert i == int(np.argmax(l[0] - g[0]))    # the device's own scores: np.argmax order exactly


def test_one_component_per_mixed_vector(engine):
    """Two components of weight 1/2, (-3, category 0) and (+3, category 1),
    sigma 0.25, s = 1e-3: the category comes from the vector's OWN component,
    so it disagrees with the sign of z only when the smoothing mass draws the
    other category: s / (1 + s) / 2 of the vectors.  A component pick per
    dimension would give 1/2."""
    C, s = 1 << 18, 1e-3
    w = np.array([0.5, 0.5])
    mu = np.array([[-3.0], [3.0]])
    sigma = np.full((2, 1), 0.25)
    above = (np.array([1.0]), np.zeros((1, 1)), np.full((1, 1), 5.0))
    cats = [(np.array([0, 1]), np.array([-1]), np.array([0.5, 0.5]), s, s)]
    inf = np.full(1, np.inf)
    rec, cand = engine.run_joint_mixed((w, mu, sigma), above, -inf, inf, cats, [3], C, seed=5, return_cand=True)
    z, v = cand[0][:, 0], cand[0][:, 1]
    assert np.isin(v, [0.0, 1.0]).all() and np.all(np.abs(np.abs(z) - 3.0) < 3.0)
    p = 0.5 * s / (1 + s)
    frac = float(np.mean((z > 0) != (v == 1)))
    print('off-component categories: %.3e of the vectors, expected %.3e' % (frac, p))
    assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / C)
    assert abs(float(np.mean(z > 0)) - 0.5) <= 5e-3      # 5 binomial standard deviations at 2^18


def test_mixed_determinism_and_batching(engine):
    """The same call twice gives the same bytes; ids [5, 9, 12] in one call are
    three single calls; 4097 candidates leave a ragged last chunk."""
    C = 4096 + 1
    below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(3, [4, '5p'], 90, seed=21)
    cats = M.cats_of(below, above, ps, sb, sa)
    ids = [5, 9, 12]
    a = engine.run_joint_mixed(below[:3], above[:3], low, high, cats, ids, C, seed=17, return_cand=True, want_lg=True)
    b = engine.run_joint_mixed(below[:3], above[:3], low, high, cats, ids, C, seed=17, return_cand=True, want_lg=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, 5) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    for j, new_id in enumerate(ids):
        s = engine.run_joint_mixed(below[:3], above[:3], low, high, cats, [new_id], C, seed=17, return_cand=True,
                                   want_lg=True)
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    other = engine.run_joint_mixed(below[:3], above[:3], low, high, cats, ids, C, seed=18, return_cand=True)
    assert other[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------ the public path
PC = [0.5, 0.3, 0.2]


def _public_case():
    """test_gpu_joint._public_case's space plus a leaf hp.pchoice and a gate
    hp.choice with an inner label; the loss couples x with the leaf choice."""
    from hyperopt_amd import base, hp, rand
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.loguniform('y', -3, 2), 'z': hp.normal('z', 0, 2),
             'q': hp.quniform('q', 0, 10, 1), 'c': hp.choice('c', [0, 1, 2]),
             'pc': hp.pchoice('pc', list(zip(PC, [-2.0, 0.0, 2.0]))),
             'gate': hp.choice('gate', [0, {'k': hp.uniform('inner', 0, 1)}])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(80):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        target = [-2.0, 0.0, 2.0][int(v['pc'])]
        loss = (float(v['x']) - target) ** 2 + 0.2 * (float(v['y']) - 1.0) ** 2 + 0.1 * float(v['z']) ** 2 \
            + 0.05 * float(v['q']) + 0.1 * int(v['c']) + 0.3 * float(v.get('inner', 0.5))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _model_from_trials(trials):
    """The float64 mixed model of (x, y, z | c, pc) from the Trials alone: the
    gamma = 0.25 split, then per side the restated mixture in tid order."""
    spec = {'x': (lambda v: v, 0.0, 10.0, -5.0, 5.0), 'y': (np.log, -0.5, 5.0, -3.0, 2.0),
            'z': (lambda v: v, 0.0, 2.0, -np.inf, np.inf)}
    cont, disc = ['x', 'y', 'z'], ['c', 'pc']
    ps = [np.full(3, 1.0 / 3), np.array(PC)]
    docs = sorted(trials.trials, key=lambda d: d['tid'])
    loss = np.array([d['result']['loss'] for d in docs])
    assert len(np.unique(loss)) == len(loss)
    nb = min(int(np.ceil(0.25 * np.sqrt(len(loss)))), 25)
    m = np.zeros(len(loss), dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    X = np.stack([spec[k][0](np.array([float(d['misc']['vals'][k][0]) for d in docs])) for k in cont], axis=1)
    XC = np.stack([np.array([int(d['misc']['vals'][k][0]) for d in docs]) for k in disc], axis=1)
    pmu, psig = np.array([spec[k][1] for k in cont]), np.array([spec[k][2] for k in cont])
    low, high = np.array([spec[k][3] for k in cont]), np.array([spec[k][4] for k in cont])
    sb = np.array([M.smoothing(len(p), int(m.sum())) for p in ps])
    sa = np.array([M.smoothing(len(p), int((~m).sum())) for p in ps])
    return (M.ref_mixed_side(X[m], pmu, psig, XC[m]), M.ref_mixed_side(X[~m], pmu, psig, XC[~m]), low, high, ps,
            sb, sa)


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_joint_discrete_suggest():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    domain, trials = _public_case()
    C, seed = 4096, 321
    plain = _vals(tpe.suggest([80], domain, trials, seed, n_EI_candidates=C)[0])
    doc = tpe.suggest([80], domain, trials, seed, n_EI_candidates=C, joint=True, joint_discrete=True)[0]
    trials.assert_valid_trial(doc)
    got = _vals(doc)
    assert set(got) == set(plain)
    for k in ('q', 'gate', 'inner'):           # not joined: the same bytes and types as without joint
        if k in plain:
            assert type(got[k]) is type(plain[k]) and got[k] == plain[k], k
    for k in ('x', 'y', 'z'):
        assert type(got[k]) is np.float64
    for k in ('c', 'pc'):                      # joined discrete values: the univariate path's type
        assert type(got[k]) is type(plain[k]) and 0 <= got[k] < 3, k
    assert -5 <= got['x'] < 5 and np.exp(-3) <= got['y'] <= np.exp(2)

    below, above, low, high, ps, sb, sa = _model_from_trials(trials)
    rec, cand, l, g = get_engine().run_joint_mixed(below[:3], above[:3], low, high,
                                                   M.cats_of(below, above, ps, sb, sa), [80], C, seed,
                                                   return_cand=True, want_lg=True)
    zc = np.array([got['x'], np.log(got['y']), got['z'], got['c'], got['pc']]).astype(np.float32)
    hit = np.flatnonzero((cand[0] == zc[None, :]).all(axis=1))
    assert len(hit) >= 1, zc
    z64, v = cand[0][:, :3].astype(np.float64), cand[0][:, 3:].astype(np.int64)
    l_ref = M.ref_mixed_lpdf(z64, v, below, low, high, ps, sb)
    g_ref = M.ref_mixed_lpdf(z64, v, above, low, high, ps, sa)
    R.check_lpdf(l[0], l_ref, 'public l')
    R.check_lpdf(g[0], g_ref, 'public g')
    ties, score = R.tie_set(l_ref, g_ref)
    print('row %s, argmax %d, %d ties' % (hit, int(np.argmax(score)), len(ties)))
    assert len(np.unique(cand[0][ties], axis=0)) <= MAX_TIES
    assert int(hit[0]) in ties and int(rec['global_idx'][0]) == int(hit[0])
    if len(ties) == 1:
        assert int(hit[0]) == int(np.argmax(score))

    # a list may name discrete labels; the others stay univariate
    two = _vals(tpe.suggest([80], domain, trials, seed, n_EI_candidates=C, joint=['x', 'pc'], joint_discrete=True)[0])
    for k in ('y', 'z', 'q', 'c', 'gate', 'inner'):
        if k in plain:
            assert type(two[k]) is type(plain[k]) and two[k] == plain[k], k
    assert type(two['pc']) is type(plain['pc']) and type(two['x']) is np.float64

    # batched ids equal single calls; the columns carry the joined labels
    ids = [80, 81, 82]
    batch = tpe.suggest(ids, domain, trials, seed, n_EI_candidates=C, joint=True, joint_discrete=True)
    assert _vals(batch[0]) == got
    for j, new_id in enumerate(ids[1:], 1):
        one = tpe.suggest([new_id], domain, trials, seed, n_EI_candidates=C, joint=True, joint_discrete=True)[0]
        assert _vals(one) == _vals(batch[j])
    from hyperopt_amd import history
    hist = history.extract(domain, trials)
    cc = tpe.suggest_choices(domain.table, hist, ids, seed, n_EI_candidates=C, joint=True, joint_discrete=True,
                             columns=True)
    for j in range(3):
        for lab, val in _vals(batch[j]).items():
            assert cc.values[j, cc.labels.index(lab)] == float(val), (j, lab)


def test_no_discrete_label_in_the_group_is_the_continuous_stage():
    """joint_discrete=True on a space without an eligible discrete label (its
    only choice is a gate) gives the documents of joint=True."""
    from hyperopt_amd import base, hp, rand, tpe
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.loguniform('y', -3, 2), 'q': hp.quniform('q', 0, 10, 1),
             'gate': hp.choice('gate', [0, {'k': hp.normal('inner', 0, 1)}])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(4)
    for tid in range(40):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': (float(v['x']) * float(v['y']) - 1.0) ** 2 + 0.01 * tid}
        trials.insert_trial_docs(docs)
    trials.refresh()
    ids = [40, 41]
    a = tpe.suggest(ids, domain, trials, 77, n_EI_candidates=2048, joint=True)
    b = tpe.suggest(ids, domain, trials, 77, n_EI_candidates=2048, joint=True, joint_discrete=True)
    c = tpe.suggest(ids, domain, trials, 77, n_EI_candidates=2048, joint=['x', 'y'], joint_discrete=True)
    for da, db, dc in zip(a, b, c):
        va, vb, vc = _vals(da), _vals(db), _vals(dc)
        assert set(va) == set(vb) == set(vc)
        for k in va:
            assert type(va[k]) is type(vb[k]) is type(vc[k])
            assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes() == np.asarray(vc[k]).tobytes(), k
