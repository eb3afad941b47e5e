"""The host selection of a lazy categorical (hyperopt_amd/csrc/tpe_lazy_host.h,
what a resident level's fused hit runs instead of the device scan) against the
numpy model of tests/lazy_cases.py, exactly: K = 2, 3 and 64; equal scores; a
NaN score; a zero-mass category with the best score; the best category rare
with n_cand below and above its first draw; one candidate; cand_base 0, odd and
past 2^32.  Unlimited budget: the model's winner after the model's number of
draws.  A small budget: "not settled" exactly when the model needs more."""
import shutil
import subprocess

import pytest

from tests import lazy_cases as LC


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return LC.build_program(tmp_path_factory.mktemp('lazy_scan'))


@pytest.fixture(scope='module')
def cases():
    return [(c, LC.model(c)) for c in LC.cpu_cases()]


def test_cases_are_what_they_say(cases):
    by = {c['name']: (c, m) for c, m in cases}
    c, (need, res) = by['zero mass best']
    assert c['cum'][1] == c['cum'][0] and (c['l'] - c['g']).argmax() == 1 and res[3] != 1.0 and need < 64
    c, (need, res) = by['equal scores']
    assert res[4] == 0                                   # the first draw wins whatever its category
    c, (need, res) = by['nan score']
    assert res[0] != res[0] and res[3] == 1.0
    assert by['rare best n40'][1][1][3] == 0.0 and by['rare best n40'][1][0] == 40       # never drawn: all 40 scanned
    assert by['rare best n5000'][1][1][3] == 1.0 and 40 < by['rare best n5000'][1][0] < 5000
    assert by['one candidate'][1][0] == 1


def test_unlimited_budget_equals_model(exe, cases, tmp_path):
    got = LC.host_select(exe, [c for c, _ in cases], [LC.UNLIMITED] * len(cases), tmp_path)
    for (c, (need, res)), (draws, r) in zip(cases, got):
        assert draws == need and LC.same(r, res), (c['name'], draws, need, r, res)


def test_small_budget_settles_exactly_when_the_model_does(exe, cases, tmp_path):
    runs = [(c, m, b) for c, m in cases for b in sorted({0, 1, 2, 4, 8, 64, max(m[0] - 1, 0), m[0], m[0] + 1})]
    got = LC.host_select(exe, [c for c, _, _ in runs], [b for _, _, b in runs], tmp_path)
    for (c, (need, res), b), (draws, r) in zip(runs, got):
        if b >= need:
            assert draws == need and LC.same(r, res), (c['name'], b, draws, need, r, res)
        else:
            assert draws == -1, (c['name'], b, draws, need)


def test_program_self_check_sanitized(tmp_path):
    """The program's own cases (against a scan of every candidate) built with
    AddressSanitizer and UBSan and run as a plain executable."""
    gxx = shutil.which('g++')
    assert gxx is not None
    exe = str(tmp_path / 'lazy_scan_asan')
    subprocess.check_call([gxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-static-libasan',
                           '-static-libubsan', '-fno-sanitize-recover=all', '-I', LC.ROOT + '/hyperopt_amd/csrc',
                           LC.ROOT + '/tools/ubench/lazy_scan_ubench.cpp', '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and 'lazy_scan_ubench: ok' in out.stdout, out.stdout + out.stderr
