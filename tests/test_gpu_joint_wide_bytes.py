"""The three wide joint stages give the bytes they gave at the commit recorded
in tests/golden/joint_wide_parent.json (made by tools/joint_wide_bytes.py): the
SHA-256 of records, cand, l and g of every case, sampled; and each id's run on
its own injected candidates repeats the sampled l, g and record
(joint_wide_bytes.run_case asserts that).  The cases reach every padded width
of the three scoring kernels, both R, ragged chunks and component tiles
(joint_wide_bytes.check_coverage, also run without a GPU)."""
import json
import os

import pytest

from tools import joint_wide_bytes as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'joint_wide_parent.json')
CASES = B.cases()


@pytest.fixture(scope='module')
def engine():
    from hyperopt_amd.engine import Engine
    return Engine(precision='fp32')


@pytest.fixture(scope='module')
def parent():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert len(doc['commit']) == 40
    return doc['data']


def test_the_cases_reach_every_instantiation(parent):
    assert B.check_coverage(CASES)
    assert sorted(parent) == sorted(c[0] for c in CASES)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_bytes_of_the_parent(engine, parent, case):
    got, want = B.run_case(engine, case), parent[case[0]]
    print(case[0], got['winners'])
    assert got['winners'] == want['winners']
    for what in ('records', 'cand', 'l', 'g'):
        assert got[what] == want[what], (case[0], what)
