"""GPU tests of the quantised joint stage (tpe_joint_quant_run through
Engine.run_joint_quant) and of tpe.suggest(..., joint=..., joint_quantized=True),
against the float64 model restated in numpy (tests/joint_quant_ref.py).

Tolerances are the project's (tests/test_gpu_kernels.py, tests/test_gpu_joint.py):
l and g within 1e-5 * max(1, |ref|); the winner inside joint_ref.tie_set, which
may hold at most 8 distinct vectors; sampled frequencies within 5 binomial
standard deviations.  The table kernel is read back through the debug return
``return_table`` of Engine.run_joint_quant: every entry within 1e-6 * max(1,
|T_ref|) of the float64 reference (f32 storage is 6e-8 relative), entries whose
reference is below the floor exactly at the floor.
"""
import functools
import math

import numpy as np
import pytest

from tests import joint_mixed_ref as M
from tests import joint_quant_ref as Q
from tests import joint_ref as R

pytestmark = pytest.mark.gpu

MAX_TIES = 8          # distinct vectors: a plateau of near-equal scores must not hide a wrong winner


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


# ------------------------------------------------------------- table kernel
QLOG0 = ('qloguniform', math.log(1e-3), math.log(10.0), 1.0)        # the value 0 is in the lattice
QLOG16 = ('qloguniform', math.log(16.0), math.log(512.0), 16.0)     # the value 512 sits at `high`
TABLE_RUNS = {
    # V = 2, 11, 32, 256
    'sizes': [('quniform', 0.0, 1.0, 1.0), ('quniform', 0.0, 10.0, 1.0), ('quniform', 16.0, 512.0, 16.0),
              ('quniform', 0.0, 255.0, 1.0)],
    # a lattice with the value 0; components outside the bounds (4 > 3.5; log 512 = high; a far one on each side)
    'edges': [QLOG0, ('quniform', 0.0, 3.5, 1.0), QLOG16],
}
EXTRA = {('quniform', 0.0, 3.5, 1.0): (4.0, 4.0), QLOG16: (512.0,), QLOG0: (0.0,)}


@pytest.mark.parametrize('name', sorted(TABLE_RUNS))
def test_table_kernel(engine, name):
    cases = TABLE_RUNS[name]
    lat = [Q.ref_lattice(*c) for c in cases]
    sides = []
    for n in (4, 50):                                    # below: 5 components (+ extras), above: 51
        cols = [Q.lattice_components(c, n, seed=n + d, extra=EXTRA.get(c, ())[:1] if n == 4 else EXTRA.get(c, ()))
                for d, c in enumerate(cases)]
        K = max(len(mu) for mu, _ in cols)
        # one row count per side: shorter columns repeat their last component
        mu = np.stack([np.concatenate([m_, np.full(K - len(m_), m_[-1])]) for m_, _ in cols], axis=1)
        sg = np.stack([np.concatenate([s_, np.full(K - len(s_), s_[-1])]) for _, s_ in cols], axis=1)
        w = np.full(K, 1.0 / K)
        sides.append((w, np.zeros((K, 0)), np.zeros((K, 0)), np.zeros((K, 0), dtype=np.int64), mu, sg))
    below, above = sides
    if name == 'edges':
        assert above[4][:, 1].max() == 4.0 > 3.5 and above[4][:, 2].max() >= cases[2][2] - 1e-12
        assert abs(above[4][:, 0].min() - cases[0][1]) < 1e-12     # the value 0 is fitted at `low`
    edges = [la[2] for la in lat]
    out = engine.run_joint_quant(below[:3], above[:3], [], [], [], Q.quants_of(below, above, edges), [3], 1024,
                                 seed=1, return_table=True)
    rec, tb, ta = out
    total = sum(len(e) - 1 for e in edges)
    n_floor = 0
    for side, got, what in ((below, tb, 'below'), (above, ta, 'above')):
        assert got.shape == (len(side[0]), total) and got.dtype == np.float32
        off = 0
        for d, e in enumerate(edges):
            V = len(e) - 1
            ref, raw = Q.ref_table(side[4][:, d], side[5][:, d], e)
            g = got[:, off:off + V].astype(np.float64)
            low = raw < Q.QFLOOR
            n_floor += int(low.sum())
            err = np.abs(g - ref) / np.maximum(1.0, np.abs(ref))
            print('%s %s V=%d: max err / tol = %.3f, %d at the floor, min ref above it %.1f'
                  % (name, what, V, err.max() / 1e-6, int(low.sum()), ref[~low].min()))
            assert (g[low] == Q.QFLOOR).all(), (what, d)
            assert err.max() <= 1e-6, (what, d, float(err.max()), np.unravel_index(np.argmax(err), err.shape))
            off += V
    if name == 'sizes':
        assert n_floor > 0                                   # the 256-value lattice: far bins of mass exactly 0


# --------------------------------------------------------------- candidates
def quant_candidates(below, low, high, ps, edges, C, seed, n_far=32):
    """test_gpu_joint_mixed.mixed_candidates' recipe with lattice indices
    appended: the eighth drawn around below components carries its component's
    categories and the lattice values next to its component's centre, the rest
    uniform random ones.  Returns f32 [C, Dc + Dk + Dq]."""
    rs = np.random.RandomState(seed)
    w, mu, sigma, xc, qmu, qsig = below
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
        z[-n_far:, d] = mu[:, d].max() + 40.0 * 4.0 + rs.uniform(0, 1, n_far)
    z = z.astype(np.float32)
    lo32 = np.where(bounded, low, -np.inf).astype(np.float32)
    hi32 = np.nextafter(np.where(bounded, high, np.inf).astype(np.float32), np.float32(-np.inf))
    z = np.clip(z, lo32[None, :], hi32[None, :])
    v = np.stack([rs.randint(len(p), size=C) for p in ps], axis=1) if ps else np.zeros((C, 0), dtype=np.int64)
    if ps:
        vk = xc[k]
        v[:n_near] = np.where(vk >= 0, vk, v[:n_near])
    qi = np.stack([rs.randint(len(e) - 1, size=C) for e in edges], axis=1)
    for d, e in enumerate(edges):
        zq = qmu[k, d] + qsig[k, d] * rs.standard_normal(n_near)
        qi[:n_near, d] = np.searchsorted(e[1:-1], np.clip(zq, e[0], np.nextafter(e[-1], -np.inf)), 'right')
    return np.hstack([z, v.astype(np.float32), qi.astype(np.float32)])


def check_quant_winner(rec, cand, l_ref, g_ref, D, what):
    """test_gpu_joint_mixed.check_mixed_winner: the winner's vector is in the
    tie set (at most MAX_TIES distinct vectors) and its index the lowest one
    holding that vector."""
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


# (Dc, us, Vs, n, C): an all-quantised group with the largest lattice; an above side of 296 components
# (the tile loop wraps); 16 coordinates at every count limit; 512 lattice values; 3000 above components; a
# partial last chunk
CASES = [(2, (), (5,), 60, 4096), (0, (), (2, 256), 40, 4096), (3, (3,), (17,), 300, 4096),
         (8, (2, 3, '5p', 4), (3, 64, 256, 10), 120, 4096), (2, (3,), (256, 250, 4, 2), 90, 4096),
         (1, (), (32,), 3013, 4096), (2, (), (5,), 60, 1500)]


@functools.lru_cache(maxsize=None)
def injected_case(Dc, us, Vs, n, C):
    """(below, above, low, high, ps, s_below, s_above, edges, cand, l_ref, g_ref), computed once."""
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, list(us), list(Vs), n)
    cand = quant_candidates(below, low, high, ps, edges, C, Dc + len(us) + len(Vs))
    Dk = len(us)
    z64, v, qi = cand[:, :Dc].astype(np.float64), cand[:, Dc:Dc + Dk].astype(np.int64), \
        cand[:, Dc + Dk:].astype(np.int64)
    l_ref = Q.ref_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges)
    g_ref = Q.ref_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges)
    return below, above, low, high, ps, sb, sa, edges, cand, l_ref, g_ref


def test_a_case_has_table_entries_at_the_floor():
    """(asserted on the reference) the 256-value lattices' above tables hold bins of mass 0"""
    for case in (CASES[1], CASES[3]):
        _, above, _, _, _, _, _, edges, _, _, _ = injected_case(*case)
        d = list(case[2]).index(256)
        _, raw = Q.ref_table(above[4][:, d], above[5][:, d], edges[d])
        assert (raw < Q.QFLOOR).sum() > 0 and np.isneginf(raw).any()


@pytest.mark.parametrize('Dc,us,Vs,n,C', CASES)
def test_scoring_of_injected_quant_candidates(engine, Dc, us, Vs, n, C):
    below, above, low, high, ps, sb, sa, edges, cand, l_ref, g_ref = injected_case(Dc, us, Vs, n, C)
    D = Dc + len(us) + len(Vs)
    if n == 300:
        assert len(above[0]) == 296
    if n == 3013:
        assert len(above[0]) == 3000
    if len(Vs) == 4 and Dc == 2:
        assert sum(Vs) == 512
    if Dc == 8:
        assert D == 16
    assert len(cand) == C
    rec, l, g = engine.run_joint_quant(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                       Q.quants_of(below, above, edges), [7], C, seed=3, inject=cand, want_lg=True)
    what = 'Dc=%d us=%s Vs=%s n=%d C=%d' % (Dc, us, Vs, n, C)
    assert l.shape == g.shape == (1, C)
    assert np.all(np.isfinite(l[0])) and np.all(np.isfinite(g[0]))
    R.check_lpdf(l[0], l_ref, 'l ' + what)
    R.check_lpdf(g[0], g_ref, 'g ' + what)
    i = int(rec['global_idx'][0])
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    check_quant_winner(rec[0], cand, l_ref, g_ref, D, what)


# ------------------------------------------------------------------ sampling
def test_quant_sampling_follows_the_below_mixture(engine):
    """2^16 sampled vectors: per quantised dimension the lattice-index
    frequencies follow sum_k w_k P_kd(i); l and g are the densities of the
    returned vectors."""
    Dc, us, Vs, C = 1, [3], [5, 32], 1 << 16
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, us, Vs, 60)
    rec, cand, l, g = engine.run_joint_quant(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                             Q.quants_of(below, above, edges), [0], C, seed=99, return_cand=True,
                                             want_lg=True)
    assert cand.shape == (1, C, 4)
    qf = cand[0][:, 2:]
    qi = qf.astype(np.int64)
    assert (qi == qf).all()
    for d, e in enumerate(edges):
        V = len(e) - 1
        assert qi[:, d].min() >= 0 and qi[:, d].max() < V
        want = Q.marginal(below, d, e)
        assert abs(want.sum() - 1.0) < 1e-12
        freq = np.bincount(qi[:, d], minlength=V) / C
        sd = np.sqrt(want * (1 - want) / C)
        print('dimension %d: (freq - p) / sd = %s' % (d, np.round((freq - want) / sd, 2)))
        assert (np.abs(freq - want) <= 5 * sd).all(), (d, freq, want)
    sub = slice(0, C, 8)
    z64, v = cand[0][sub, :1].astype(np.float64), cand[0][sub, 1:2].astype(np.int64)
    R.check_lpdf(l[0][sub], Q.ref_quant_lpdf(z64, v, qi[sub], below, low, high, ps, sb, edges), 'sampled l')
    R.check_lpdf(g[0][sub], Q.ref_quant_lpdf(z64, v, qi[sub], above, low, high, ps, sa, edges), 'sampled g')
    i = int(rec['global_idx'][0])
    np.testing.assert_array_equal(rec['z'][0, :4], cand[0][i].astype(np.float64))
    assert (rec['z'][0, 4:] == 0).all()
    assert rec['l'][0] == l[0][i] and rec['g'][0] == g[0][i]
    assert i == int(np.argmax(l[0] - g[0]))


def test_one_component_per_quant_vector(engine):
    """test_one_component_per_mixed_vector's construction: two components of
    weight 1/2, (-3, lattice value 1) and (+3, lattice value 6) of 8, sigma
    0.25.  The lattice index comes from the vector's OWN component, so it falls
    on the other half of the lattice than the sign of z says only when a normal
    draw strays 10 sigma: never.  A component pick per dimension would give 1/2."""
    C = 1 << 16
    w = np.array([0.5, 0.5])
    mu = np.array([[-3.0], [3.0]])
    sigma = np.full((2, 1), 0.25)
    above = (np.array([1.0]), np.zeros((1, 1)), np.full((1, 1), 5.0))
    e = Q.lattice_of(8)
    quants = [(np.array([1.0, 6.0]), np.array([0.25, 0.25]), np.array([3.5]), np.array([7.0]), e)]
    inf = np.full(1, np.inf)
    rec, cand = engine.run_joint_quant((w, mu, sigma), above, -inf, inf, [], quants, [3], C, seed=5, return_cand=True)
    z, i = cand[0][:, 0], cand[0][:, 1]
    assert np.isin(i, np.arange(8.0)).all() and np.all(np.abs(np.abs(z) - 3.0) < 3.0)
    frac = float(np.mean((z > 0) != (i >= 4)))
    print('off-component lattice values: %.3e of the vectors' % frac)
    p = 1e-20                                            # (above Phi(-10))
    assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / C)
    assert abs(float(np.mean(z > 0)) - 0.5) <= 5 * np.sqrt(0.25 / C)
    assert set(np.unique(i)) <= {0.0, 1.0, 2.0, 5.0, 6.0, 7.0}


# --------------------------------------------------- bit-for-bit coordinates
def test_continuous_and_discrete_coordinates_are_the_mixed_stage_s(engine):
    """The same seed and id: the continuous and discrete coordinates of a quant
    run are those of run_joint_mixed over the group without its quantised
    labels, byte for byte."""
    C = 4096
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(2, [3, '5p'], [5, 11], 60)
    cats = M.cats_of(below, above, ps, sb, sa)
    _, cand = engine.run_joint_quant(below[:3], above[:3], low, high, cats, Q.quants_of(below, above, edges), [11], C,
                                     seed=42, return_cand=True)
    _, mixed = engine.run_joint_mixed(below[:3], above[:3], low, high, cats, [11], C, seed=42, return_cand=True)
    assert cand.shape == (1, C, 6) and mixed.shape == (1, C, 4)
    assert np.ascontiguousarray(cand[0][:, :4]).tobytes() == mixed[0].tobytes()
    for d, e in enumerate(edges):
        assert len(np.unique(cand[0][:, 4 + d])) == len(e) - 1       # every lattice value turns up


@pytest.mark.parametrize('Dc,Vs', [(2, [5]), (5, [17, 4])])
def test_quantised_indices_are_the_binned_continuous_draws(engine, Dc, Vs):
    """No discrete label: the continuous coordinates equal run_joint's, and the
    lattice indices equal searchsorted over the coordinates run_joint draws
    when the quantised dimensions' sampler rows stand in those word positions
    as continuous ones.  (5, [17, 4]): words 6 and 7, the second Philox block."""
    C = 4096
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(Dc, [], Vs, 60)
    rec, cand, l, g = engine.run_joint_quant(below[:3], above[:3], low, high, [], Q.quants_of(below, above, edges),
                                             [11], C, seed=42, return_cand=True, want_lg=True)
    _, cont = engine.run_joint(below[:3], above[:3], low, high, [11], C, seed=42, return_cand=True)
    assert np.ascontiguousarray(cand[0][:, :Dc]).tobytes() == cont[0].tobytes()
    wide = [(s[0], np.hstack([s[1], s[4]]), np.hstack([s[2], s[5]])) for s in (below, above)]
    lo = np.concatenate([low, [e[0] for e in edges]])
    hi = np.concatenate([high, [e[-1] for e in edges]])
    _, full = engine.run_joint(wide[0], wide[1], lo, hi, [11], C, seed=42, return_cand=True)
    assert np.ascontiguousarray(full[0][:, :Dc]).tobytes() == cont[0].tobytes()
    for d, e in enumerate(edges):
        zq = full[0][:, Dc + d].astype(np.float64)
        assert zq.min() >= e[0] and zq.max() < e[-1]
        want = np.searchsorted(e[1:-1], zq, 'right')
        np.testing.assert_array_equal(cand[0][:, Dc + d], want.astype(np.float32))
    qi = cand[0][:, Dc:].astype(np.int64)
    z64 = cand[0][:, :Dc].astype(np.float64)
    none = np.zeros((C, 0), dtype=np.int64)
    R.check_lpdf(l[0], Q.ref_quant_lpdf(z64, none, qi, below, low, high, [], sb, edges), 'l Dc=%d' % Dc)
    R.check_lpdf(g[0], Q.ref_quant_lpdf(z64, none, qi, above, low, high, [], sa, edges), 'g Dc=%d' % Dc)
    i = int(rec['global_idx'][0])
    assert i == int(np.argmax(l[0] - g[0]))
    np.testing.assert_array_equal(rec['z'][0, :Dc + len(Vs)], cand[0][i].astype(np.float64))


def test_quant_determinism_and_batching(engine):
    """The same call twice gives the same bytes; ids [5, 9, 12] in one call are
    three single calls; 4097 candidates leave a ragged last chunk."""
    C = 4096 + 1
    below, above, low, high, ps, sb, sa, edges, _ = Q.seeded_quant_case(3, [4], [7, 12], 90, seed=21)
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    ids = [5, 9, 12]

    def run(ids, seed=17):
        return engine.run_joint_quant(below[:3], above[:3], low, high, cats, quants, ids, C, seed=seed,
                                      return_cand=True, want_lg=True)
    a, b = run(ids), run(ids)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].shape == (3, C, 6) and a[2].shape == (3, C)
    assert len({a[1][j].tobytes() for j in range(3)}) == 3                 # every id its own stream
    for j, new_id in enumerate(ids):
        s = run([new_id])
        assert s[0].tobytes() == a[0][j:j + 1].tobytes()
        for k in (1, 2, 3):
            assert s[k][0].tobytes() == a[k][j].tobytes()
        assert int(s[0]['global_idx'][0]) == int(np.argmax(s[2][0] - s[3][0]))
    assert run(ids, seed=18)[1].tobytes() != a[1].tobytes()


# ------------------------------------------------------------ the public path
LOW_B, HIGH_B = math.log(16.0), math.log(512.0)
OPTS = ['sgd', 'adam', 'rmsprop']


def _public_case():
    """lr x batch x layers with a leaf choice and one conditional branch; the
    loss couples lr with batch and layers."""
    from hyperopt_amd import base, hp, rand
    space = {'lr': hp.loguniform('lr', math.log(1e-4), math.log(1.0)),
             'batch': hp.qloguniform('batch', LOW_B, HIGH_B, 16),
             'layers': hp.quniform('layers', 1, 8, 1),
             'opt': hp.choice('opt', OPTS),
             'reg': hp.choice('reg', [0, {'k': hp.uniform('l2', 0, 1)}])}
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(8)
    for tid in range(60):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        v = {k: x[0] for k, x in docs[0]['misc']['vals'].items() if len(x)}
        loss = (math.log(float(v['lr'])) - math.log(float(v['batch']) / 256.0) + 4.0) ** 2 \
            + 0.3 * (float(v['layers']) - 5.0) ** 2 + 0.2 * int(v['opt']) + 0.3 * float(v.get('l2', 0.5))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': loss}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _model_from_trials(trials, qlabels):
    """The float64 model of (lr | opt | qlabels) from the Trials alone: the gamma
    = 0.25 split, then per side the restated mixtures in tid order."""
    lat = {'batch': Q.ref_lattice('qloguniform', LOW_B, HIGH_B, 16.0), 'layers': Q.ref_lattice('quniform', 1.0, 8.0, 1.0)}
    coord = {'batch': lambda x: np.log(np.maximum(x, max(1e-12, math.exp(LOW_B)))), 'layers': lambda x: x}
    docs = sorted(trials.trials, key=lambda d: d['tid'])
    loss = np.array([d['result']['loss'] for d in docs])
    assert len(np.unique(loss)) == len(loss)
    nb = min(int(np.ceil(0.25 * np.sqrt(len(loss)))), 25)
    m = np.zeros(len(loss), dtype=bool)
    m[np.argsort(loss)[:nb]] = True
    col = lambda k: np.array([float(d['misc']['vals'][k][0]) for d in docs])
    X = np.log(col('lr'))[:, None]
    XC = col('opt').astype(np.int64)[:, None]
    XQ = np.stack([coord[k](col(k)) for k in qlabels], axis=1)
    pmu, psig = np.array([0.5 * (math.log(1e-4) + 0.0)]), np.array([0.0 - math.log(1e-4)])
    low, high = np.array([math.log(1e-4)]), np.array([math.log(1.0)])
    edges = [lat[k][2] for k in qlabels]
    qpmu = np.array([0.5 * (e[0] + e[-1]) for e in edges])
    qpsig = np.array([e[-1] - e[0] for e in edges])
    ps = [np.full(3, 1.0 / 3)]
    sides = []
    for sel in (m, ~m):
        w, mu, sigma, xc = M.ref_mixed_side(X[sel], pmu, psig, XC[sel])
        _, qmu, qsig = R.ref_side(XQ[sel], qpmu, qpsig)
        sides.append((w, mu, sigma, xc, qmu, qsig))
    sb = np.array([M.smoothing(3, int(m.sum()))])
    sa = np.array([M.smoothing(3, int((~m).sum()))])
    return sides[0], sides[1], low, high, ps, sb, sa, edges, [lat[k] for k in qlabels]


def _vals(doc):
    return {k: v[0] for k, v in doc['misc']['vals'].items() if len(v)}


def test_public_joint_quantized_suggest():
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    domain, trials = _public_case()
    C, seed = 4096, 321
    kw = dict(n_EI_candidates=C, joint=True, joint_discrete=True, joint_quantized=True)
    plain = _vals(tpe.suggest([60], domain, trials, seed, n_EI_candidates=C)[0])
    doc = tpe.suggest([60], domain, trials, seed, **kw)[0]
    trials.assert_valid_trial(doc)
    got = _vals(doc)
    assert set(got) == set(plain)
    for k in ('reg', 'l2'):                    # not joined: the same bytes and types as without joint
        if k in plain:
            assert type(got[k]) is type(plain[k]) and got[k] == plain[k], k
    assert type(got['lr']) is np.float64 and 1e-4 <= got['lr'] <= 1.0
    assert type(got['opt']) is type(plain['opt']) and 0 <= got['opt'] < 3
    for k, q, lo, hi in (('batch', 16.0, 16.0, 512.0), ('layers', 1.0, 1.0, 8.0)):
        assert type(got[k]) is np.float64 and type(plain[k]) is np.float64
        assert got[k] == np.rint(got[k] / q) * q and lo <= got[k] <= hi, (k, got[k])

    qlabels = [r.label for r in domain.table.rows if r.label in ('batch', 'layers')]      # table order
    below, above, low, high, ps, sb, sa, edges, lat = _model_from_trials(trials, qlabels)
    rec, cand, l, g = get_engine().run_joint_quant(below[:3], above[:3], low, high, M.cats_of(below, above, ps, sb, sa),
                                                   Q.quants_of(below, above, edges), [60], C, seed, return_cand=True,
                                                   want_lg=True)
    qs = {'batch': 16.0, 'layers': 1.0}
    idx = [got[k] / qs[k] - la[0] for k, la in zip(qlabels, lat)]
    zc = np.array([np.log(got['lr']), got['opt']] + idx).astype(np.float32)
    hit = np.flatnonzero((cand[0] == zc[None, :]).all(axis=1))
    assert len(hit) >= 1, zc
    z64, v, qi = cand[0][:, :1].astype(np.float64), cand[0][:, 1:2].astype(np.int64), cand[0][:, 2:].astype(np.int64)
    l_ref = Q.ref_quant_lpdf(z64, v, qi, below, low, high, ps, sb, edges)
    g_ref = Q.ref_quant_lpdf(z64, v, qi, above, low, high, ps, sa, edges)
    R.check_lpdf(l[0], l_ref, 'public l')
    R.check_lpdf(g[0], g_ref, 'public g')
    ties, score = R.tie_set(l_ref, g_ref)
    print('row %s, argmax %d, %d ties' % (hit, int(np.argmax(score)), len(ties)))
    assert len(np.unique(cand[0][ties], axis=0)) <= MAX_TIES
    assert int(hit[0]) in ties and int(rec['global_idx'][0]) == int(hit[0])
    if len(ties) == 1:
        assert int(hit[0]) == int(np.argmax(score))

    # a list may name quantised labels; the others stay univariate
    two = _vals(tpe.suggest([60], domain, trials, seed, n_EI_candidates=C, joint=['lr', 'batch'],
                            joint_quantized=True)[0])
    for k in ('layers', 'opt', 'reg', 'l2'):
        if k in plain:
            assert type(two[k]) is type(plain[k]) and two[k] == plain[k], k
    assert type(two['batch']) is np.float64 and two['batch'] == np.rint(two['batch'] / 16.0) * 16.0

    # batched ids equal single calls; the columns carry the joined labels
    ids = [60, 61, 62]
    batch = tpe.suggest(ids, domain, trials, seed, **kw)
    assert _vals(batch[0]) == got
    for j, new_id in enumerate(ids[1:], 1):
        assert _vals(tpe.suggest([new_id], domain, trials, seed, **kw)[0]) == _vals(batch[j])
    from hyperopt_amd import history
    hist = history.extract(domain, trials)
    cc = tpe.suggest_choices(domain.table, hist, ids, seed, columns=True, **kw)
    for j in range(3):
        for lab, val in _vals(batch[j]).items():
            assert cc.values[j, cc.labels.index(lab)] == float(val), (j, lab)


def test_no_quantised_label_in_the_group_is_the_stage_without_the_keyword():
    """joint_quantized=True on a space whose only quantised labels are not
    eligible (a qnormal, a conditional quniform) gives the documents of the
    same call without the keyword."""
    from hyperopt_amd import base, hp, rand, tpe
    space = {'x': hp.uniform('x', -5, 5), 'y': hp.loguniform('y', -3, 2), 'qn': hp.qnormal('qn', 0, 3, 1),
             'leaf': hp.choice('leaf', [0, 1, 2]),
             'gate': hp.choice('gate', [0, {'k': hp.quniform('inner', 0, 5, 1)}])}
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
    for kw in (dict(joint=True), dict(joint=True, joint_discrete=True), dict(joint=['x', 'y'])):
        a = tpe.suggest(ids, domain, trials, 77, n_EI_candidates=2048, **kw)
        b = tpe.suggest(ids, domain, trials, 77, n_EI_candidates=2048, joint_quantized=True, **kw)
        for da, db in zip(a, b):
            va, vb = _vals(da), _vals(db)
            assert set(va) == set(vb)
            for k in va:
                assert type(va[k]) is type(vb[k])
                assert np.asarray(va[k]).tobytes() == np.asarray(vb[k]).tobytes(), k
