"""Every univariate device draw against the numpy model of tests/draw_ref.py,
draw for draw: candidate i of (seed, label, id) has one value, whichever kernel
draws it and whichever search finds its component.

The sampler rows the device holds are read back after each Engine.run and must
be draw_ref.sampler_rows' bytes (as the packers' are on the CPU,
tests/test_draw_ref_host.py); the model is drawn from them.

A  every candidate of every family, both precisions, through Engine.run
B  component edges placed on a candidate's own 32-bit selection word
C  the same index gives the same value at every draw site (eight paths; the
   three A/B switches that are read once per process run in child processes)
D  counter words past 32 bits and odd candidate bases

Measured on an MI355X over section A's own draws (printed by
test_every_candidate; the figures are the widening beyond the bracket's
arithmetic terms that the worst draw needs, relative to |z|):
  f32, ndtri_f32:   1.05e-7 |z|, within the header's 3e-7: no re-measured bound
  f64, erfcinv:     5.67e-16 |z|; draw_ref.ERFCINV_REL = 4 x that = 2.3e-15 (<= 1e-12)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import draw_cases as DC
from tests import draw_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


# ------------------------------------------------------------------ helpers
def _lps(cases, ids, labels=None):
    from hyperopt_amd.engine import LevelProblem
    return [LevelProblem(DC.posterior(c), labels[i] if labels is not None else i, list(ids))
            for i, c in enumerate(cases)]


def _host_prob(engine, info=None):
    """The problem rows of the last pack, from the staging buffer."""
    from hyperopt_amd import _native as N
    info = info if info is not None else engine._last_info
    return np.frombuffer(engine._pinned.numpy(), dtype=N.PROBLEM_DTYPE, count=int(info.n_problems),
                         offset=int(info.off_problems)).copy()


def _device_rows(engine):
    """(problems, [sampler rows of each problem]) as the device holds them
    after the last Engine.run."""
    from hyperopt_amd import _native as N
    info = engine._last_info
    blob = engine._bufs['blob'][:int(info.blob_bytes)].cpu().numpy()
    prob = np.frombuffer(blob, dtype=N.PROBLEM_DTYPE, count=int(info.n_problems), offset=int(info.off_problems)).copy()
    n = max(int(p['samp_off']) + int(p['samp_len']) for p in prob)
    samp = np.frombuffer(blob, dtype=np.float64, count=8 * n, offset=int(info.off_samp)).reshape(n, 8).copy()
    return prob, [samp[int(p['samp_off']):int(p['samp_off']) + int(p['samp_len'])] for p in prob]


def _check_rows(dev, c, what):
    ref = DC.rows_of(c)
    assert dev.shape == ref.shape, what
    assert dev.tobytes() == ref.tobytes(), what


def _model(c, rows, label_ix, new_id, g, precision, **kw):
    return R.draw(c['family'], rows, c['low'], c['high'], c['q'], DC.SEED, label_ix, new_id, g, precision, **kw)


def _assert_inside(d, x, c, what, at=None):
    """x (all candidates, or those at indices `at` of d) lies in the model's
    bracket; categories exactly; a quantised value is one of the bracket's two
    lattice points (equal for all but the either-point candidates)."""
    lo, hi = (d.x_lo, d.x_hi) if at is None else (d.x_lo[at], d.x_hi[at])
    x = np.asarray(x, dtype=np.float64)
    if c['family'] == R.CATEGORICAL or c['q'] is not None:
        ok = (x == lo) | (x == hi)
    else:
        ok = (x >= lo) & (x <= hi)
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), x[bad[:5]].tolist(), lo[bad[:5]].tolist(),
                           hi[bad[:5]].tolist())


def _excess(c, rows, label_ix, new_id, g, precision, x):
    """The relative widening of z the worst unclipped draw needs beyond the
    bracket's arithmetic terms (pr +- 1 ulp, 2 ulps of the multiply-add): the
    device inverse's error against scipy's, as far as the values show it."""
    d0 = _model(c, rows, label_ix, new_id, g, precision, ndtri_rel=0.0, erfcinv_rel=0.0)
    out = np.maximum(np.maximum(d0.t_lo - x, x - d0.t_hi), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(d0.clipped | (d0.z == 0), 0.0, out / (d0.sigma * np.abs(d0.z)))
    return float(np.max(rel)) if len(rel) else 0.0


# ------------------------------------------------------------------------ A
@pytest.mark.parametrize('precision', ['fp32', 'fp64'])
@pytest.mark.parametrize('dist', DC.DISTS)
def test_every_candidate(engine, dist, precision, monkeypatch):
    """Section A: C = 2 * 2048 + 37 candidates of every mixture of the family
    (K = 1, 26, 64, 65, TPE_SAMPLE_LDS_ROWS and + 1; components wholly outside
    the bounds, mirrored, nearly all outside on either side, sigma = psig / 100),
    two ids (one with its high bit set), label index 0 and large ones, a seed
    with both words set: every value inside the model's bracket, categories and
    lattice points exact, and the winner's re-drawn value equal to its candidate.
    f32 runs through the tabulated sample kernel and, with TPE_TABLES=0, the
    general one.

    Measured (MI355X, these draws, uniform and normal): the widening of z beyond
    the arithmetic terms that the worst draw needs is 0 for f32 at the header's
    3e-7 (rel = 0 would need 1.05e-7 |z|) and 5.67e-16 |z| for the f64 erfcinv;
    draw_ref.ERFCINV_REL is 4 x that (2.3e-15, under the 1e-12 cap)."""
    named = DC.cases_a(dist)
    cases = [c for _, c in named]
    labels = [(k // 2) if k % 2 == 0 else DC.LABEL_BIG - k for k in range(len(cases))]
    lps = _lps(cases, DC.IDS, labels)
    engine.set_precision(precision)
    try:
        for tables in (('1', '0') if precision == 'fp32' and cases[0]['family'] != R.CATEGORICAL else ('1',)):
            monkeypatch.setenv('TPE_TABLES', tables)
            res, cand = engine.run(lps, DC.C_A, DC.SEED, return_cand=True)
            prob, rows = _device_rows(engine)
            assert len(prob) == 2 * len(cases)
            if tables == '0':
                assert np.all(prob['tab_mode'] == 0)
            g = np.arange(DC.C_A)
            worst = 0.0
            for r in range(len(prob)):
                k, nid = r // 2, DC.IDS[r % 2]
                what = (named[k][0], precision, tables, r % 2)
                assert int(prob[r]['ctr2']) == labels[k] and int(prob[r]['ctr3']) == nid & 0xFFFFFFFF, what
                _check_rows(rows[r], cases[k], what)
                d = _model(cases[k], rows[r], labels[k], nid, g, precision)
                if dist in ('uniform', 'normal'):
                    worst = max(worst, _excess(cases[k], rows[r], labels[k], nid, g, precision, cand[r]))
                _assert_inside(d, cand[r], cases[k], what)
                i = int(res[r]['idx'])
                assert res[r]['value'] == cand[r][i] and int(res[r]['global_idx']) == i, what
            if dist in ('uniform', 'normal'):
                print('draw excess beyond the arithmetic terms, relative to |z|: %s %s tables=%s %.3g'
                      % (dist, precision, tables, worst))
    finally:
        engine.set_precision('fp32')


# ------------------------------------------------------------------------ B
def test_component_edges_on_the_word(engine):
    """Section B: a component edge c placed on the selection word w* of
    candidates 0, 1, 2047, 2048 and C - 1 — c = (w* + 0.5) 2^-32 (u = c: not
    below the edge), the next double above (below it) and c - 2^-33 — sends
    that candidate to component 1, 0, 1 (by its value: the components are 16
    sigma apart) and moves no other; likewise on each of the five edges of a
    six-component mixture whose edges share one 1/256 slice of the CDF."""
    cb = DC.cases_b()
    cases = [c for _, _, c, _, _ in cb]
    labels = [ix for _, ix, _, _, _ in cb]
    res, cand = engine.run(_lps(cases, [DC.IDS[0]], labels), DC.C_A, DC.SEED, return_cand=True)
    prob, rows = _device_rows(engine)
    g = np.arange(DC.C_A)
    for r, (name, ix, c, i, want) in enumerate(cb):
        _check_rows(rows[r], c, name)
        d = _model(c, rows[r], ix, DC.IDS[0], g, 'fp32')
        assert d.comp[i] == want, name
        _assert_inside(d, cand[r], c, name)
        mu = c['below'][1]
        by_value = np.argmin(np.abs(cand[r][:, None] - mu[None, :]), axis=1)
        # (six components: 6 sigma apart, a draw past 3 sigma is nearer its neighbour)
        sure = np.abs(d.z) < 2.9
        assert sure[i] or len(mu) == 2, name
        if len(mu) == 2:
            np.testing.assert_array_equal(by_value, d.comp, err_msg=name)
        else:
            np.testing.assert_array_equal(by_value[sure], d.comp[sure], err_msg=name)
        if sure[i] or len(mu) == 2:
            assert by_value[i] == want, (name, float(cand[r][i]))


# ------------------------------------------------------------------------ C
def _c_cases():
    cb = DC.cases_b()
    extra = DC.cases_c_extra()
    names = [n for n, _, _, _, _ in cb] + [n for n, _, _ in extra]
    labels = [ix for _, ix, _, _, _ in cb] + [ix for _, ix, _ in extra]
    cases = [c for _, _, c, _, _ in cb] + [c for _, _, c in extra]
    return names, labels, cases


def _fast_report(engine, lps, n_cand, cand_base=0, n_cand_global=None):
    """One run_level with the stage profile on and tpe_debug_fast_lg armed:
    (results, records [P * n_cand, 4] (NaN where no fast kernel wrote), whether
    the sample stage launched, its specialised pass's kernel time)."""
    import torch
    from hyperopt_amd import _native as N
    P = sum(len(lp.ids) for lp in lps)
    buf = torch.full((4 * P * n_cand,), float('nan'), dtype=torch.float64, device=engine.device)
    N.check(engine.lib.tpe_debug_fast_lg(buf.data_ptr(), P * n_cand), engine.lib, 'tpe_debug_fast_lg')
    engine.profile = {}
    try:
        res = engine.run_level(lps, n_cand, DC.SEED, cand_base=cand_base, n_cand_global=n_cand_global)
        torch.cuda.synchronize()
    finally:
        N.check(engine.lib.tpe_debug_fast_lg(None, 0), engine.lib, 'tpe_debug_fast_lg')
        prof, engine.profile = engine.profile, None
    stage = prof.get('k_sample')
    return res, buf.cpu().numpy().reshape(-1, 4), stage is not None, (stage[-1][3] if stage else 0.0)


def _level_summary(engine, cases, labels, ids, n_cand, cand_base=0, n_cand_global=None):
    """A level through run_level, as a JSON-able record: which sample kernel
    ran (by the profile and the debug records), how many candidates a fast
    kernel wrote and how many of those left the model's bracket, and every
    problem's winner [idx, value, global_idx]."""
    import torch
    lps = _lps(cases, ids, labels)
    info = engine._pack(lps, n_cand, DC.SEED, cand_base, n_cand_global)
    prob = _host_prob(engine, info)
    engine._drop_resident()
    res, rec, launched, kernel_ms = _fast_report(engine, lps, n_cand, cand_base, n_cand_global)
    written = np.isfinite(rec[:, 3])
    outside = 0
    g = cand_base + np.arange(n_cand, dtype=np.uint64)
    rows_of = [DC.rows_of(c) for c in cases]
    for r in range(len(prob)):
        k = r // len(ids)
        o = int(prob[r]['cand_off'])
        mine = rec[o:o + n_cand]
        w = written[o:o + n_cand]
        if not w.any():
            continue
        d = _model(cases[k], rows_of[k], labels[k], ids[r % len(ids)], g, 'fp32')
        x = mine[:, 0]
        if cases[k]['q'] is not None:
            ok = (x == d.x_lo) | (x == d.x_hi)
        else:
            ok = (x >= d.x_lo) & (x <= d.x_hi)
        outside += int(np.count_nonzero(w & ~ok)) + int(np.count_nonzero(w & (mine[:, 3] != labels[k])))
    return dict(tab_modes=sorted(set(int(m) for m in prob['tab_mode'])), launched=bool(launched),
                kernel_ns_positive=bool(kernel_ms > 0), written=int(written.sum()), total=int(len(rec)),
                outside=outside, n_tiles=int(info.n_tiles),
                cu_count=int(torch.cuda.get_device_properties(engine.device).multi_processor_count),
                np2_forced=os.environ.get('TPE_FAST_NP2', '') == '1',
                winners=[[int(x['idx']), float(x['value']), int(x['global_idx'])] for x in res])


D_BASE_FAST = 1
D_C_FAST = 2048 + 1


def _child_report():
    """What a child process (one A/B switch set in its environment) prints:
    section C's level and section D's odd-base level through run_level."""
    from hyperopt_amd.engine import Engine
    engine = Engine(precision='fp32')
    names, labels, cases = _c_cases()
    # (the quniform apart: k_sample_tab's FAST pass takes cells only, so a level
    # with a lattice in it would fall back to the general kernel as a whole)
    out = dict(c=_level_summary(engine, cases[:-1], labels[:-1], [DC.IDS[0]], DC.C_A),
               q=_level_summary(engine, cases[-1:], labels[-1:], [DC.IDS[0]], DC.C_A),
               d=_level_summary(engine, [DC.case_d_fast()], [7], [DC.IDS[1]], D_C_FAST, D_BASE_FAST,
                                D_BASE_FAST + D_C_FAST))
    print('DRAWS_JSON ' + json.dumps(out))


_GPU_STOPPED = []          # why, once a child faulted or hung: nothing of this file touches the GPU after it


def _stop_gpu_work(why):
    """A child process faulted, aborted or hung: no later child and no later
    test may start work on that card.  Ends the whole pytest session (a flag
    besides, for a runner that survives the exit: see _no_gpu_after_a_fault)."""
    _GPU_STOPPED.append(why)
    pytest.exit('GPU child process faulted or hung, stopping: ' + why, returncode=1)


@pytest.fixture(autouse=True)
def _no_gpu_after_a_fault():
    if _GPU_STOPPED:
        pytest.fail('not run: ' + _GPU_STOPPED[0], pytrace=False)


def _run_child(switch):
    env = dict(os.environ)
    for k in ('TPE_TAB_FAST', 'TPE_SAMPLE_FAST2', 'TPE_FAST_NP2', 'TPE_TABLES', 'TPE_DEBUG_FLAGS'):
        env.pop(k, None)
    env.update(switch)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    try:
        r = subprocess.run([sys.executable, '-c', 'from tests.test_gpu_draws import _child_report; _child_report()'],
                           cwd=ROOT, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True)
    except subprocess.TimeoutExpired:
        _stop_gpu_work('child %r ran past its %d s limit' % (switch, CHILD_TIMEOUT))
    # a signal (negative status), an abort or a kill: the card may be faulted or hung
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or 'illegal memory access' in r.stderr:
        _stop_gpu_work('child %r ended with status %d: %s' % (switch, r.returncode, r.stderr[-800:]))
    assert r.returncode == 0, (switch, r.returncode, r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('DRAWS_JSON ')]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len('DRAWS_JSON '):])


@pytest.fixture(scope='module')
def c_reference(engine):
    """Section C's level through path 1 (Engine.run, candidates written: the
    tabulated sample kernel without its FAST pass): the candidates, the model's
    draws and the oracle's scores of those candidates, shared by every path."""
    from hyperopt_amd import _native as N
    names, labels, cases = _c_cases()
    lps = _lps(cases, [DC.IDS[0]], labels)
    # C_A candidates: section B's edge indices (2047, 2048, C_A - 1) need them; the
    # six-component mixtures (391 cells) are tabulated from 3910 candidates on, so
    # C_A is within 6 % of the smallest count at which every mixture is
    res, cand = engine.run(lps, DC.C_A, DC.SEED, return_cand=True)
    prob, rows = _device_rows(engine)
    g = np.arange(DC.C_A)
    model, l_ref, g_ref = [], [], []
    for r, c in enumerate(cases):
        assert prob[r]['tab_mode'] == (N.TAB_LATTICE if c['q'] else N.TAB_CELLS), names[r]
        _check_rows(rows[r], c, names[r])
        d = _model(c, rows[r], labels[r], DC.IDS[0], g, 'fp32')
        model.append(d)
        lb, la = _oracle_scores(c, cand[r])
        l_ref.append(lb)
        g_ref.append(la)
    return dict(names=names, labels=labels, cases=cases, lps=lps, res=res, cand=cand, model=model, l=l_ref,
                g=g_ref)


def _oracle_scores(c, x):
    """The oracle's (l, g) of the candidates x of case c."""
    from oracle import tpe_oracle as O
    lpdf = O.lgmm1_lpdf if c['family'] in (R.LOGGAUSS, R.QLOGGAUSS) else O.gmm1_lpdf
    kw = dict(low=c['low'], high=c['high'], q=c['q'])
    return lpdf(x, *c['below'], **kw), lpdf(x, *c['above'], **kw)


def _check_winners(ref, winners, what, stride=1, ids=None):
    """Every problem's winner [idx, value, ..]: inside the eps-tie set of the
    oracle's scores of path 1's candidates (the first id's rows), and its value
    the model's draw at that index — whichever index won."""
    from tests.test_gpu_kernels import _check_argmax
    for r, w in enumerate(winners):
        k, j = r // stride, r % stride
        c = ref['cases'][k]
        idx, value = int(w[0]), float(w[1])
        assert 0 <= idx < DC.C_A, (what, ref['names'][k])
        if j == 0:
            d = ref['model'][k]
            _check_argmax(idx, ref['l'][k], ref['g'][k], 1e-9 if c['q'] else 1e-5, (what, ref['names'][k]))
            _assert_inside(d, [value], c, (what, ref['names'][k]), at=np.array([idx]))
        else:
            d = _model(c, DC.rows_of(c), ref['labels'][k], ids[j], np.array([idx]), 'fp32')
            _assert_inside(d, [value], c, (what, ref['names'][k], j))


def test_path1_candidates_written(engine, c_reference):
    """Path 1 (k_sample_tab without the FAST pass, every mixture tabulated —
    asserted in the fixture): the winner's re-draw equals its candidate."""
    ref = c_reference
    for r, x in enumerate(ref['res']):
        _assert_inside(ref['model'][r], ref['cand'][r], ref['cases'][r], ref['names'][r])
        assert x['value'] == ref['cand'][r][int(x['idx'])], ref['names'][r]
    _check_winners(ref, [[x['idx'], x['value']] for x in ref['res']], 'path1')


def test_path2_per_candidate_select(engine, c_reference, monkeypatch):
    """Path 2 (TPE_TABLES=0, nothing written): sort, k_above_*, k_finalize and
    select_generic's re-draw of the winner."""
    from hyperopt_amd import _native as N
    ref = c_reference
    monkeypatch.setenv('TPE_TABLES', '0')
    res = engine.run(ref['lps'], DC.C_A, DC.SEED)
    prob, info = _host_prob(engine), engine._last_info
    assert np.all(prob['tab_mode'] == N.TAB_NONE) and info.n_tab_jobs == 0
    assert info.sort_end_bit > 0 and info.n_sorted > 0 and info.n_pooled == 0
    _check_winners(ref, [[x['idx'], x['value']] for x in res], 'path2')


def test_path3_pooled_select(engine, c_reference, monkeypatch):
    """Path 3: three ids on each pruned label (pooled: one sort slot, winners by
    select_pooled).  Every id's winner lies in the eps-tie set of the oracle's
    scores of that id's own candidates (written by a run of the same level with
    tables, each inside the model's bracket) and has the model's value."""
    from hyperopt_amd import _native as N
    from tests.test_gpu_kernels import _check_argmax
    ref = c_reference
    ids = [DC.IDS[0], DC.IDS[1], 77]
    lps = _lps(ref['cases'], ids, ref['labels'])
    _, cand = engine.run(lps, DC.C_A, DC.SEED, return_cand=True)
    monkeypatch.setenv('TPE_TABLES', '0')
    res = engine.run(lps, DC.C_A, DC.SEED)
    prob, info = _host_prob(engine), engine._last_info
    cont = np.repeat([c['q'] is None for c in ref['cases']], 3)
    assert info.n_pooled > 0 and np.all((prob['flags'][cont] & N.F_POOLED) != 0)
    assert np.all(prob['tab_mode'] == N.TAB_NONE)
    _check_winners(ref, [[x['idx'], x['value']] for x in res], 'path3', stride=3, ids=ids)
    g = np.arange(DC.C_A)
    for r, x in enumerate(res):
        k, j = r // 3, r % 3
        c, what = ref['cases'][k], ('path3', ref['names'][k], j)
        d = _model(c, DC.rows_of(c), ref['labels'][k], ids[j], g, 'fp32')
        _assert_inside(d, cand[r], c, what)
        lb, la = _oracle_scores(c, cand[r])
        _check_argmax(int(x['idx']), lb, la, 1e-9 if c['q'] else 1e-5, what)


def test_path4_fast_kernel_every_candidate(engine, c_reference):
    """Path 4, the tabulated default (k_sample_fast<4>): the kernel itself
    writes every candidate's value (tpe_debug_fast_lg) and every one is the
    model's draw of its index; the winners as on every path."""
    ref = c_reference
    s = _level_summary(engine, ref['cases'], ref['labels'], [DC.IDS[0]], DC.C_A)
    assert s['launched'] and s['kernel_ns_positive'] and s['written'] == s['total'], s
    _assert_np4(s)
    assert s['outside'] == 0, s
    _check_winners(ref, s['winners'], 'path4')


def _assert_np4(s):
    """k_sample_fast<4>, not <2>: tpe_sample takes NP = 4 when the stage's
    workgroups number at most two a CU and TPE_FAST_NP2 is not set; there are
    never more workgroups than tiles."""
    assert not s['np2_forced'] and s['n_tiles'] <= 2 * s['cu_count'], s


@pytest.mark.parametrize('switch,fast_writes,timed,timed_lattice', [
    ({'TPE_FAST_NP2': '1'}, True, True, True),          # path 5: k_sample_fast<2>
    ({'TPE_SAMPLE_FAST2': '0'}, False, True, False),    # path 6: k_sample_tab<F32, true> (cells only)
    ({'TPE_TAB_FAST': '0'}, False, False, False)])      # path 7: k_sample_tab<F32> on the early-selection flow
def test_paths_5_to_7_switches(c_reference, switch, fast_writes, timed, timed_lattice):
    """Paths 5 to 7: the A/B switches are read once per process, so each runs in
    one fresh child (one alive at a time, under its own time limit).  Which
    kernel ran: k_sample_fast writes the debug records (all of them, every one
    the model's draw) and the other two none; the profiler times the
    specialised pass (tab_fast) and not the general kernel.  The quniform
    runs as a level of its own: k_sample_tab's FAST pass has no lattice path, so
    under TPE_SAMPLE_FAST2=0 a lattice takes the general kernel (and a level
    with one in it would, as a whole).  Section D's level (cand_base = 1,
    C = 2049: every Philox pair straddles two blocks) runs in the same child."""
    ref = c_reference
    rep = _run_child(switch)
    for key in ('c', 'q', 'd'):
        s = rep[key]
        assert s['launched'] and s['kernel_ns_positive'] == (timed_lattice if key == 'q' else timed), (switch, key, s)
        assert s['written'] == (s['total'] if fast_writes else 0) and s['outside'] == 0, (switch, key, s)
        assert 0 not in s['tab_modes'], (switch, key, s)
        assert s['np2_forced'] == ('TPE_FAST_NP2' in switch), (switch, key, s)    # (path 5: <2> by the switch)
    _check_winners(ref, rep['c']['winners'] + rep['q']['winners'], str(switch))
    _check_d_fast(rep['d'], str(switch))


def test_path8_lazy_categorical(engine):
    """Path 8: select_cat_lazy (run_level, TPE_F_CAT_LAZY set by the packer)
    returns the model's category at the index it reports, the same winner as
    the full scan with candidates written."""
    from hyperopt_amd import _native as N
    c = DC.categorical_case('categorical', 26)
    rows = DC.rows_of(c)
    lps = _lps([c], DC.IDS, [9])
    info = engine._pack(lps, DC.C_A, DC.SEED, 0, None)
    prob = _host_prob(engine, info)
    assert np.all((prob['flags'] & N.F_CAT_LAZY) != 0)
    engine._drop_resident()
    lazy = engine.run_level(lps, DC.C_A, DC.SEED)
    full, cand = engine.run(lps, DC.C_A, DC.SEED, return_cand=True)
    np.testing.assert_array_equal(lazy, full)
    for r, nid in enumerate(DC.IDS):
        d = _model(c, rows, 9, nid, np.arange(DC.C_A), 'fp32')
        np.testing.assert_array_equal(cand[r], d.x)
        assert lazy[r]['value'] == d.x[int(lazy[r]['idx'])]


# ------------------------------------------------------------------------ D
def _check_d_fast(s, what):
    c = DC.case_d_fast()
    idx, value, gidx = s['winners'][0]
    assert gidx == D_BASE_FAST + idx, what
    d = _model(c, DC.rows_of(c), 7, DC.IDS[1], np.array([D_BASE_FAST + idx], dtype=np.uint64), 'fp32')
    _assert_inside(d, [value], c, what)


def test_odd_base_fast_kernel(engine):
    """cand_base = 1, C = 2049 through k_sample_fast<4>: no candidate pair
    shares a Philox block with its neighbour the way an even base's does."""
    s = _level_summary(engine, [DC.case_d_fast()], [7], [DC.IDS[1]], D_C_FAST, D_BASE_FAST, D_BASE_FAST + D_C_FAST)
    assert s['launched'] and s['kernel_ns_positive'] and s['written'] == s['total'] and s['outside'] == 0, s
    _assert_np4(s)
    _check_d_fast(s, 'fast<4>')


@pytest.mark.parametrize('precision,base', [('fp32', 2 ** 33 - 3), ('fp64', 2 ** 32 - 3)])
def test_counter_words_past_32_bits(engine, precision, base):
    """f32: cand_base = 2^33 - 3, C = 8 — the block index g >> 1 carries into
    counter word 1 mid-run and the base is odd; f64 and categorical:
    cand_base = 2^32 - 3 — g itself carries.  Candidates written, and the
    winner's re-draw without them (Engine.run and run_level)."""
    C = 8
    cases = [DC.continuous_case('normal', 26), DC.continuous_case('quniform', 26), DC.case_d_fast(),
             DC.categorical_case('randint', 65)]
    labels = [3, 4, 5, 6]
    lps = _lps(cases, DC.IDS, labels)
    engine.set_precision(precision)
    try:
        res, cand = engine.run(lps, C, DC.SEED, cand_base=base, n_cand_global=base + C, return_cand=True)
        prob, rows = _device_rows(engine)
        assert np.all(prob['cand_base'] == base)
        g = base + np.arange(C, dtype=np.uint64)
        plain = engine.run(lps, C, DC.SEED, cand_base=base, n_cand_global=base + C)
        level = engine.run_level(lps, C, DC.SEED, cand_base=base, n_cand_global=base + C)
        for r in range(len(prob)):
            k, nid = r // 2, DC.IDS[r % 2]
            d = _model(cases[k], rows[r], labels[k], nid, g, precision)
            _assert_inside(d, cand[r], cases[k], (k, precision))
            for out in (res, plain, level):
                i = int(out[r]['idx'])
                assert int(out[r]['global_idx']) == base + i
                assert out[r]['value'] == cand[r][i], (k, precision)
    finally:
        engine.set_precision('fp32')
