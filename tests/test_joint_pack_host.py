"""The host-side packer of the joint stages (hyperopt_amd/joint_pack.py), on the
CPU: what every Engine.run_joint* entry hands to the native library equals what
the commit before the packer moved handed to it (tests/joint_pack_capture.py,
tests/golden/joint_pack_parent.json); a group's rows in a segmented blob are
the bytes of its solo rows; every fault of a group raises one text whichever
entry it comes through."""
import json

import numpy as np
import pytest

from hyperopt_amd import _native as N
from hyperopt_amd import joint as J
from hyperopt_amd import joint_pack as JP
from tests import joint_pack_capture as K

C, SEED, IDS = K.C, K.SEED, K.IDS


# ------------------------------------------------------- the parent's bytes
@pytest.fixture(scope='module')
def parent(golden):
    data = golden('joint_pack_parent.json')
    assert len(data['commit']) == 40
    return data['cases']


def test_golden_holds_the_cases_of_today(parent):
    assert sorted(parent) == sorted(K.cases())


@pytest.mark.parametrize('name', sorted(K.cases()))
def test_native_call_equals_parent(parent, name):
    got = json.loads(json.dumps(K.capture(K.cases()[name])))
    want = parent[name]
    assert got['returns'] == want['returns']
    assert len(got['calls']) == len(want['calls']) == (0 if name.startswith('shard_empty') else 1)
    for g, w in zip(got['calls'], want['calls']):
        for key in sorted(w):
            assert g[key] == w[key], (name, key)
        assert g == w


# ------------------------------------------------ solo rows = segment rows
KINDS = {'continuous': ('run', K.cont_group(5)), 'mixed': ('mixed', K.mixed_group(2, [4])),
         'quant': ('quant', K.quant_group(2, [3], [50, 7])), 'quant_alone': ('quant', K.quant_group(0, [], [5]))}
SOLO = {'run': 'run_joint', 'wide': 'run_joint_wide', 'mixed': 'run_joint_mixed', 'quant': 'run_joint_quant'}


def _solo_fields(entry, group):
    """The plain fields of the args struct of the group's solo run."""
    eng, lib = K.stub_engine()
    getattr(eng, SOLO[entry])(*group, IDS, C, SEED)
    return lib.calls[0]['fields']


# (tpe_joint_seg descriptors hold continuous groups only)
@pytest.mark.parametrize('kind,dtype', [('continuous', 'seg')] + [(k, 'mseg') for k in sorted(KINDS)])
def test_segment_rows_are_the_solo_rows(kind, dtype):
    entry, group = KINDS[kind]
    if dtype == 'seg':
        models, seg_dtype = [K.cont_group(2), group, K.cont_group(3)], N.JOINT_SEG_DTYPE
    else:
        models, seg_dtype = [K.mixed_group(0, [3, '5p']), group, K.cont_group(3)], N.JOINT_MSEG_DTYPE
    inject = [K.inject_of(m, 3 + i) for i, m in enumerate(models)]
    r = JP.group_rows(*group, entry=entry)
    b = JP.segment_blob(models, [7, 8, 9], [2, 1, 0, 1], [4, 5, 6, 7], C, inject, seg_dtype)
    sec = dict(zip(JP.SECTIONS, zip(b.offs[:-1], b.offs[1:])))
    pool = {np.float32: b.blob[slice(*sec['pool_f32'])].view(np.float32),
            np.float64: b.blob[slice(*sec['pool_f64'])].view(np.float64)}
    assert len(pool[np.float32]) == b.n32 and len(pool[np.float64]) == b.n64
    assert b.blob[slice(*sec['segs'])].tobytes() == b.segs.tobytes()
    g = b.segs[1]
    rows = JP.group_rows_present(r)
    want_keys = {'continuous': 8, 'mixed': 16, 'quant': 22, 'quant_alone': 14}[kind]
    assert len(rows) == want_keys
    for key, field, _, dt, _ in rows:
        arr = np.ascontiguousarray(r[key], dtype=dt).reshape(-1)
        lo = int(g[field])
        assert pool[dt][lo:lo + arr.size].tobytes() == arr.tobytes(), (key, lo)
    inj = inject[1].reshape(-1)
    assert pool[np.float32][int(g['inject']):int(g['inject']) + inj.size].tobytes() == inj.tobytes()
    Dc, Dk, Dq = r['Dc'], r['Dk'], r['Dq']
    assert (g['n_dims'], g['k_below'], g['k_above'], g['stream_word']) == (Dc, r['k_below'], r['k_above'], 8)
    assert g['below_base'] == r['below_base'] and g['above_base'] == r['above_base']
    # the bounds: joint.f32_bounds of what the solo args carry, padded with -+inf
    f = _solo_fields(entry, group)
    low, high = [np.array([float.fromhex(x) for x in f[k]]) for k in ('low', 'high')]
    assert f['n_dims'] == Dc and (f['k_below'], f['k_above']) == (r['k_below'], r['k_above'])
    lo, hi = J.f32_bounds(low[:Dc], high[:Dc])
    assert g['lo'][:Dc].tobytes() == lo.tobytes() and g['hi'][:Dc].tobytes() == hi.tobytes()
    assert (g['lo'][Dc:] == -np.inf).all() and (g['hi'][Dc:] == np.inf).all()
    if dtype == 'mseg':
        assert (g['n_cat'], g['n_quant']) == (Dk, Dq)
        qlo, qhi = J.f32_bounds(low[Dc:Dc + Dq], high[Dc:Dc + Dq])
        assert g['qlo'][:Dq].tobytes() == qlo.tobytes() and g['qhi'][:Dq].tobytes() == qhi.tobytes()
        assert (g['qlo'][Dq:] == -np.inf).all() and (g['qhi'][Dq:] == np.inf).all()
        assert list(g['cat_upper'][:Dk]) == f.get('cat_upper', [])[:Dk]
        assert list(g['cat_off'][:Dk]) == f.get('cat_off', [])[:Dk]
        assert list(g['quant_v'][:Dq]) == f.get('quant_v', [])[:Dq]
        assert list(g['quant_edge_off'][:Dq]) == f.get('quant_edge_off', [])[:Dq]
        assert g['n_edges'] == f.get('n_edges', 0)


# ------------------------------------------------- one message per fault
CONT, MIXED, QUANT = K.cont_group(3), K.mixed_group(2, [4]), K.quant_group(2, [3], [50, 7])
ENTRIES = {'cont': ('run', 'wide', 'seg', 'mseg'), 'mixed': ('mixed', 'mseg'), 'quant': ('quant', 'mseg')}


def _wider(group):
    """The group with one column too many in the below side's mu and sigma."""
    w, mu, sigma = group[0]
    pad = np.ones((len(w), 1))
    return ((w, np.hstack([mu, pad]), np.hstack([sigma, pad])),) + tuple(group[1:])


def _cat(group, **kw):
    """The group with fields of its first discrete dimension replaced."""
    c = dict(zip(('xb', 'xa', 'p', 'sb', 'sa'), group[4][0]), **kw)
    return tuple(group[:4]) + ([(c['xb'], c['xa'], c['p'], c['sb'], c['sa'])] + list(group[4][1:]),) + tuple(group[5:])


def _quant(group, **kw):
    """The group with fields of its first quantised dimension replaced."""
    q = dict(zip(('mb', 'sb', 'ma', 'sa', 'edges'), group[5][0]), **kw)
    return tuple(group[:5]) + ([(q['mb'], q['sb'], q['ma'], q['sa'], q['edges'])] + list(group[5][1:]),)


def _set(arr, i, v):
    arr = np.array(arr)
    arr[i] = v
    return arr


SEGMENT_LIMIT = 'a segment with discrete or quantised dimensions holds at most 8 continuous and 4 discrete ones, not '
# (fault, kind, faulty group, the text: one for every entry, or per entry where the limits differ)
FAULTS = [
    ('shape', 'cont', _wider(CONT), 'joint stage: mixture shapes do not match 3 dimensions'),
    ('shape', 'mixed', _wider(MIXED), 'joint stage: mixture shapes do not match 2 dimensions'),
    ('shape', 'quant', _wider(QUANT), 'joint stage: mixture shapes do not match 2 dimensions'),
    ('dims', 'cont', K.cont_group(17), {'run': 'joint stage: 17 dimensions, at most 16',
                                        'seg': 'joint stage: 17 dimensions, at most 16',
                                        'mseg': 'joint stage: 17 dimensions, at most 16'}),
    ('dims_wide', 'cont', K.cont_group(65), {'wide': 'joint stage: 65 dimensions, at most 64'}),
    ('dims', 'mixed', K.mixed_group(15, [2, 2]), {'mixed': 'joint stage: 17 dimensions, at most 16',
                                                  'mseg': SEGMENT_LIMIT + '15 and 2'}),
    ('dims', 'quant', K.quant_group(9, [3], [5]), {
        'quant': 'joint stage: beside a quantised dimension at most 8 continuous and 4 discrete ones, not 9 and 1',
        'mseg': SEGMENT_LIMIT + '9 and 1'}),
    ('n_quant', 'quant', K.quant_group(0, [], [3] * 5), 'joint stage: 5 quantised dimensions, at most 4'),
    ('cats', 'mixed', _cat(MIXED, p=np.ones(1)), 'joint stage: 1 categories, outside [2, 256]'),
    ('cats', 'quant', _cat(QUANT, p=np.ones(1)), 'joint stage: 1 categories, outside [2, 256]'),
    ('cat_total', 'mixed', K.mixed_group(0, [256] * 5), {
        'mixed': 'joint stage: 1280 categories in the group, at most 1024'}),
    ('prior_0', 'mixed', _cat(MIXED, p=np.array([0.5, 0.25, 0.25, 0.0])), 'joint stage: a prior probability of 0'),
    ('prior_0', 'quant', _cat(QUANT, p=np.array([0.5, 0.5, 0.0])), 'joint stage: a prior probability of 0'),
    ('category', 'mixed', _cat(MIXED, xb=_set(MIXED[4][0][0], 1, 4)),
     'joint stage: a component category outside [-1, 4)'),
    ('category', 'quant', _cat(QUANT, xa=_set(QUANT[4][0][1], 2, -2)),
     'joint stage: a component category outside [-1, 3)'),
    ('per_component', 'mixed', _cat(MIXED, xb=MIXED[4][0][0][:-1]),
     'joint stage: one category / (mu, sigma) per component and dimension'),
    ('per_component', 'quant', _quant(QUANT, ma=QUANT[5][0][2][:-1]),
     'joint stage: one category / (mu, sigma) per component and dimension'),
    ('smoothing', 'mixed', _cat(MIXED, sb=0.0), 'joint stage: the smoothing masses must be positive'),
    ('smoothing', 'quant', _cat(QUANT, sa=-1.0), 'joint stage: the smoothing masses must be positive'),
    ('lattice', 'quant', _quant(QUANT, edges=np.array([0.0, 1.0])), 'joint stage: 1 lattice values, outside [2, 256]'),
    ('lattice_total', 'quant', K.quant_group(0, [], [200] * 3),
     'joint stage: 600 lattice values in the group, at most 512'),
    ('edges', 'quant', _quant(QUANT, edges=_set(QUANT[5][0][4], 2, QUANT[5][0][4][1])),
     'joint stage: the lattice edges must be finite and strictly increasing'),
    ('bandwidth', 'quant', _quant(QUANT, sb=_set(QUANT[5][0][1], 1, 0.0)),
     'joint stage: the quantised bandwidths must be positive'),
]
OTHER, OTHER_MIXED = K.cont_group(2), K.mixed_group(0, [3, '5p'])


def _run(entry, group, inject=None, probs=None):
    """The group through one entry point of a device-less engine; in a
    segmented call it is group 1, beside a continuous group (and, 'mseg', a
    mixed one that sends the call to the mixed segmented stage)."""
    eng, lib = K.stub_engine()
    if entry in SOLO:
        return getattr(eng, SOLO[entry])(*group, IDS, C, SEED, inject=inject)
    models = [OTHER, group] + ([OTHER_MIXED] if entry == 'mseg' else [])
    if inject is not None and not isinstance(inject, list):
        inject = [K.inject_of(OTHER), inject] + ([K.inject_of(OTHER_MIXED)] if entry == 'mseg' else [])
    probs = [1, 0, 1] if probs is None else probs
    return eng.run_joint_segments(models, list(range(len(models))), probs, list(range(len(probs))), C, SEED,
                                  inject=inject)


def _raises(text, *args, **kw):
    with pytest.raises(ValueError) as e:
        _run(*args, **kw)
    assert text in str(e.value)


@pytest.mark.parametrize('fault,kind,group,text', FAULTS, ids=['%s-%s' % f[:2] for f in FAULTS])
def test_one_message_per_fault(fault, kind, group, text):
    texts = text if isinstance(text, dict) else dict.fromkeys(ENTRIES[kind], text)
    for entry, t in texts.items():
        _raises(t, entry, group)


@pytest.mark.parametrize('kind,group', [('cont', CONT), ('mixed', MIXED), ('quant', QUANT)])
def test_inject_messages(kind, group):
    D = sum(len(x) for x in group[3:])
    good = K.inject_of(group)
    for entry in ENTRIES[kind]:
        _run(entry, group, inject=good)                               # (the group itself is sound)
        _raises('joint stage: inject must be [n_cand, %d]' % D, entry, group, inject=np.zeros((C, D + 1), np.float32))
        _raises('joint stage: inject must be [n_cand, %d]' % D, entry, group, inject=good[:-1])
        if entry in SOLO:
            continue
        full = [K.inject_of(OTHER), good, K.inject_of(OTHER_MIXED)][:3 if entry == 'mseg' else 2]
        S = len(full)
        _run(entry, group, inject=[None] + full[1:], probs=[1, 1] + [2] * (S - 2))   # group 0 has no problem
        _raises('joint stage: inject lacks the candidates of a group that has a problem', entry, group,
                inject=[None] + full[1:])
        _raises('joint stage: inject must hold one entry per group', entry, group, inject=full[:-1])
        _raises('joint stage: a problem names a group outside [0, %d)' % S, entry, group, probs=[1, S])
        _raises('joint stage: a problem names a group outside [0, %d)' % S, entry, group, probs=[-1, 1])
