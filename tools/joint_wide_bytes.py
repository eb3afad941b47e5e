"""The bytes of the three wide joint stages over a fixed list of small cases:

    python tools/joint_wide_bytes.py OUT.json [COMMIT]

Each case runs once sampled and once per id with `inject` set to the sampled
run's own candidates (Engine.run_joint_wide, run_joint_wide_mixed and
run_joint_wide_quant with return_cand=True, want_lg=True).  Per case OUT.json
gets the SHA-256 of records / cand / l / g and the winner records in full (l and
g as hex floats).  tests/golden/joint_wide_parent.json is this file made on the
commit it names; tests/test_gpu_joint_wide_bytes.py recomputes it.

The cases are the shapes of the three stages' GPU tests with C cut to two
chunks and a ragged third; `check_coverage` restates the kernels' dispatch
rules and fails on the CPU if a padded width, R, tile or edge is not reached."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import joint_mixed_ref as M          # noqa: E402
from tests import joint_quant_ref as Q          # noqa: E402
from tests import joint_ref as R                # noqa: E402
from tests import joint_wide_quant_ref as W     # noqa: E402

SEED = 23


def chunk_of(dp):
    """Candidates per scoring workgroup: 256 R, R = 2 up to 32 padded continuous slots."""
    return 256 * (2 if dp <= 32 else 1)


def ragged(dp):
    """Two whole chunks and 37 candidates: a ragged last chunk and sample block."""
    return 2 * chunk_of(dp) + 37


def pad_to(n, widths):
    for p in widths:
        if n <= p:
            return p
    return widths[-1]


WIDE_DP, MIXED_DP, QUANT_DP = (20, 24, 32, 48, 64), (12, 16, 20, 24, 32, 48, 64), (16, 24, 32, 48, 64)
MIXED_KP, QUANT_KP, QP = (1, 2, 4, 8), (0, 2, 8), (1, 2, 4)

# tests/test_gpu_joint_wide.py's (D, n) list, and (30, 60) for the padded width 32
WIDE = [(17, 40), (17, 120), (20, 3013), (24, 300), (30, 60), (33, 60), (48, 120), (64, 26), (64, 300)]
WIDE_IDS = {(17, 120): (7, 11)}
# tests/test_gpu_joint_wide_mixed.py's CASES
MIXED = [
    (16, (3,), 60),
    (9, (2, 3, '5p', 17, 2, 3, 4, 7), 120),
    (17, (2, '5p', 4), 300),
    (21, (2, 3, '5p', 17, 2, 3, 4, 7), 120),
    (30, (4, '5p'), 60),
    (44, (3, 2, 2, 4), 200),
    (56, (2, 3, '5p', 17, 2, 3, 4, 7), 90),
    (63, (5,), 300),
    (13, (3, 4), 4000),
]
MIXED_IDS = {(17, 300): (7, 8, 9)}
# tests/test_gpu_joint_wide_quant.py's SHAPES (its own ids and C)
QUANT = [
    (17, (), (2,), 301, (3,), 700, False),
    (9, (3,), (11,), 60, (5, 9), 2 * 512 + 37, False),
    (20, (3, '5p'), (256, 256), 70, (7,), 2 * 512 + 37, False),
    (28, (2, 3, '5p', 4, 2, 3, 2, 6), (2, 3, 5, 7), 301, (1, 2, 4), 2 * 512 + 37, False),
    (44, (3, 2, 4), (37,), 200, (11, 12), 2 * 256 + 37, True),
    (59, (3,), (4, 4, 4, 4), 150, (8,), 2 * 256 + 37, False),
]


def n_above(n):
    """Components of the above side of a seeded case of n trials (the prior row included)."""
    return n - int(np.ceil(np.sqrt(n) / 4.0)) + 1


def cases():
    """[(name, stage, kernel instantiation, C, ids, above components, tile, builder)]"""
    out = []
    for D, n in WIDE:
        dp = pad_to(D, WIDE_DP)
        out.append(('wide_%d_%d' % (D, n), 'wide', (dp,), ragged(dp), WIDE_IDS.get((D, n), (7,)), n_above(n),
                    128 if dp <= 32 else (4096 // dp) & ~7, (D, n)))
    for Dc, us, n in MIXED:
        dp = pad_to(Dc, MIXED_DP)
        out.append(('mixed_%d_%d_%d' % (Dc, len(us), n), 'mixed', (dp, pad_to(len(us), MIXED_KP)), ragged(dp),
                    MIXED_IDS.get((Dc, n), (7,)), n_above(n), 128 if dp <= 32 else (4096 // dp) & ~7, (Dc, us, n)))
    for Dc, us, Vs, n, ids, C, qlog in QUANT:
        dp = W.dp_of(Dc)
        assert dp == pad_to(Dc, QUANT_DP)
        out.append(('quant_%d_%d_%d_%d' % (Dc, len(us), len(Vs), n), 'quant',
                    (dp, pad_to(len(us), QUANT_KP), pad_to(len(Vs), QP)), C, ids, n_above(n), W.tile_of(Dc, sum(Vs)),
                    (Dc, us, Vs, n, qlog)))
    return out


def check_coverage(cs=None):
    """Every padded width of the three dispatchers, both R, the ragged edges,
    several ids, a ragged component tile and the tile of 8 are reached."""
    cs = cases() if cs is None else cs
    seen = {s: set() for s in ('wide', 'mixed', 'quant')}
    for name, stage, inst, C, ids, ka, tile, _ in cs:
        seen[stage].add(inst)
        per = chunk_of(inst[0])
        assert C % per != 0 and C % 256 != 0 and C <= 1061, (name, C)      # ragged chunk, ragged sample block
    assert {i[0] for i in seen['wide']} == set(WIDE_DP)
    assert {i[0] for i in seen['mixed']} == set(MIXED_DP) and {i[1] for i in seen['mixed']} == set(MIXED_KP)
    assert {i[0] for i in seen['quant']} == set(QUANT_DP) and {i[1] for i in seen['quant']} == set(QUANT_KP)
    assert {i[2] for i in seen['quant']} == set(QP)
    for stage in seen:
        assert {chunk_of(i[0]) for i in seen[stage]} == {256, 512}, stage     # both R
        mine = [c for c in cs if c[1] == stage]
        assert any(len(c[4]) > 1 for c in mine), stage                        # more than one id
        assert any(c[3] > chunk_of(c[2][0]) and c[3] % chunk_of(c[2][0]) == 37 for c in mine), stage
        # an above side of several component tiles whose last one is ragged and no multiple of 4
        assert any(c[5] > c[6] and (c[5] % c[6]) % 4 != 0 for c in mine), stage
    assert any(c[6] == 8 for c in cs if c[1] == 'quant')                      # V = [256, 256]
    return True


def build(stage, spec):
    """(run(ids, C, inject), D): the stage's call on the seeded model of one case."""
    if stage == 'wide':
        D, n = spec
        below, above, low, high, _, _ = R.seeded_case(D, n, 1000 * D + n)
        return (lambda engine, ids, C, inject: engine.run_joint_wide(
            below, above, low, high, list(ids), C, SEED, inject=inject, return_cand=True, want_lg=True)), D
    if stage == 'mixed':
        Dc, us, n = spec
        below, above, low, high, _, _, ps, sb, sa, _ = M.seeded_mixed_case(Dc, list(us), n, None)
        cats = M.cats_of(below, above, ps, sb, sa)
        return (lambda engine, ids, C, inject: engine.run_joint_wide_mixed(
            below[:3], above[:3], low, high, cats, list(ids), C, SEED, inject=inject, return_cand=True,
            want_lg=True)), Dc + len(us)
    Dc, us, Vs, n, qlog = spec
    below, above, low, high, ps, sb, sa, edges, _ = W.wide_quant_case(Dc, list(us), list(Vs), n, qlog=qlog)
    cats, quants = M.cats_of(below, above, ps, sb, sa), Q.quants_of(below, above, edges)
    return (lambda engine, ids, C, inject: engine.run_joint_wide_quant(
        below[:3], above[:3], low, high, cats, quants, list(ids), C, SEED, inject=inject, return_cand=True,
        want_lg=True)), Dc + len(us) + len(Vs)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(engine, c):
    """The digests of one case; asserts that each id's injected run repeats the
    sampled run's l, g and record."""
    name, stage, _, C, ids, _, _, spec = c
    run, D = build(stage, spec)
    rec, cand, l, g = run(engine, ids, C, None)
    assert cand.shape == (len(ids), C, D) and l.shape == g.shape == (len(ids), C), name
    for j, new_id in enumerate(ids):
        rj, cj, lj, gj = run(engine, [new_id], C, cand[j].copy())
        assert rj.tobytes() == rec[j:j + 1].tobytes(), (name, 'record of the injected run', j)
        assert lj[0].tobytes() == l[j].tobytes() and gj[0].tobytes() == g[j].tobytes(), (name, 'l / g injected', j)
        assert cj[0].tobytes() == cand[j].tobytes(), (name, 'cand of the injected run', j)
    return {
        'records': sha(rec), 'cand': sha(cand), 'l': sha(l), 'g': sha(g),
        'winners': [{'id': int(i), 'global_idx': int(r['global_idx']), 'l': float(r['l']).hex(),
                     'g': float(r['g']).hex()} for i, r in zip(ids, rec)],
    }


def run_all(engine):
    cs = cases()
    check_coverage(cs)
    return {c[0]: run_case(engine, c) for c in cs}


def main(argv):
    out, commit = argv[1], (argv[2] if len(argv) > 2 else None)
    check_coverage()
    from hyperopt_amd.engine import Engine
    data = run_all(Engine(precision='fp32'))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump({'commit': commit, 'data': data}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%d cases -> %s' % (len(data), out))


if __name__ == '__main__':
    main(sys.argv)
