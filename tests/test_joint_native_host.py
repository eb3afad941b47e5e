"""The native driver of the six joint stages, the parts that need no GPU,
against the commit before its rewrite (tests/golden/joint_native_parent.json,
section ``host``, written by tests/joint_native_capture.py): the return code
and the whole message of every faulty call of the table (doubly faulty ones
pin the order of the checks), and every size function's value."""
import json
import os

import pytest

from hyperopt_amd import _native as N
from tests import joint_native_capture as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'joint_native_parent.json')
with open(GOLDEN) as fh:
    WANT = json.load(fh)['host']['data']
FAULTS, SIZES = dict(C.host_table()), dict(C.size_table())


def test_the_tables_are_the_captured_ones():
    assert sorted(FAULTS) == sorted(WANT['faults']) and sorted(SIZES) == sorted(WANT['sizes'])
    # every message the driver can give without a device is in the table
    assert len(set(m for _, m in WANT['faults'].values() if m)) == 115


@pytest.mark.parametrize('name', sorted(FAULTS))
def test_fault_code_and_message(name):
    lib, keep = N.load(), []
    rc = FAULTS[name](lib, keep)
    assert [rc, lib.tpe_last_error().decode() if rc != 0 else None] == WANT['faults'][name]


@pytest.mark.parametrize('name', sorted(SIZES))
def test_size(name):
    lib, keep = N.load(), []
    rc, nb = SIZES[name](lib, keep)
    assert [rc, nb, lib.tpe_last_error().decode() if rc != 0 else None] == WANT['sizes'][name]
