"""The native driver of the six joint stages against the commit before its
rewrite (tests/golden/joint_native_parent.json, section ``gpu``, written by
tests/joint_native_capture.py on an MI355X): every chunk-kernel class of every
stage, an inject case and an off-chunk shard per stage, byte for byte (the
device code is the same and the stages have no atomics), and the profiled
launches (tpe_joint_profile and its two companions), which return the same
bytes and a time."""
import ctypes
import json
import math
import os

import pytest

from tests import joint_native_capture as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'joint_native_parent.json')
with open(GOLDEN) as fh:
    WANT = json.load(fh)['gpu']['data']
CASES = C.gpu_cases()


@pytest.fixture(scope='module')
def eng():
    return C.gpu_engine()


def test_the_cases_are_the_captured_ones():
    assert sorted(CASES) == sorted(WANT)
    assert len(CASES) == 8 + 5 + 24 + 48 + 2 + 12


@pytest.mark.parametrize('name', sorted(CASES))
def test_bytes_are_the_parents(eng, name):
    assert C.digest(CASES[name](eng)) == WANT[name]


def _time(x):
    return math.isfinite(x) and x > 0


@pytest.mark.parametrize('stage', sorted(C.STAGE_CASES))
def test_profiled_launches_give_the_same_bytes_and_a_time(eng, stage):
    lib, name = eng.lib, C.STAGE_CASES[stage]
    plain = C.digest(CASES[name](eng))
    ms2, ms = (ctypes.c_double * 2)(), ctypes.c_double(0.0)
    assert lib.tpe_joint_profile(1, None) == 0
    try:
        timed = C.digest(CASES[name](eng))
        # (for a segmented stage ms2[0] sums the order, table and class launches)
        assert lib.tpe_joint_profile(0, ms2) == 0
        assert _time(ms2[0]) and _time(ms2[1]), list(ms2)
        if stage == 'quant':
            assert lib.tpe_joint_quant_profile(ctypes.byref(ms)) == 0 and _time(ms.value), ms.value
        if stage == 'wide':
            assert lib.tpe_joint_wide_profile(ctypes.byref(ms)) == 0 and _time(ms.value), ms.value
            assert lib.tpe_joint_profile(1, None) == 0
            inj = C.digest(CASES['wide_inject'](eng))
            assert lib.tpe_joint_wide_profile(ctypes.byref(ms)) == -1      # no sampling launch to read
            assert b'no profiled sampling tpe_joint_wide_run' in lib.tpe_last_error()
            assert lib.tpe_joint_profile(0, ms2) == 0 and _time(ms2[0]) and _time(ms2[1]), list(ms2)
            assert inj == WANT['wide_inject']
    finally:
        lib.tpe_joint_profile(0, None)
    assert timed == plain == WANT[name]
    # turned off: nothing to read
    assert lib.tpe_joint_profile(0, ms2) == -1
