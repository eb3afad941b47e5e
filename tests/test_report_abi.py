"""Candidate report (include/tpe_hip.h "Candidate report"), the parts that need
no GPU: record layouts against the C compiler, the argument checks tpe_report
makes before any launch, the scratch formula, and the public interface's own
argument checks."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hyperopt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tpe_hip.h')

MIRRORS = (('tpe_top_entry', 'TOP_ENTRY_DTYPE'), ('tpe_score_stats', 'SCORE_STATS_DTYPE'))


def _c_layout():
    lines = ['printf("TPE_REPORT_CHUNK %d\\nTPE_REPORT_MAX_K %d\\n", TPE_REPORT_CHUNK, TPE_REPORT_MAX_K);']
    for cname, dname in MIRRORS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in getattr(N, dname).names:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tpe_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % (
        '\n'.join(lines))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'r.c')
        open(c, 'w').write(prog)
        exe = os.path.join(d, 'r')
        subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), c, '-o', exe])
        out = subprocess.check_output([exe]).decode()
    return dict((line.split()[0], int(line.split()[1])) for line in out.strip().splitlines())


def test_report_records_match_c():
    lay = _c_layout()
    assert lay['TPE_REPORT_CHUNK'] == N.REPORT_CHUNK == 4096
    assert lay['TPE_REPORT_MAX_K'] == N.REPORT_MAX_K == 64
    assert lay['tpe_top_entry'] == 32 and lay['tpe_score_stats'] == 64
    for cname, dname in MIRRORS:
        dt = getattr(N, dname)
        assert lay[cname] == dt.itemsize, cname
        for f in dt.names:
            assert dt.fields[f][1] == lay[cname + '.' + f], (cname, f)


def _report(lib, batch, k, top=None, n_top=None, stats=None, scratch=None, scratch_bytes=0):
    return lib.tpe_report(batch, k, top, n_top, stats, scratch, scratch_bytes, None)


def test_null_batch_is_rejected():
    lib = N.load()
    assert _report(lib, None, 8) == -1
    assert b'null batch' in lib.tpe_last_error()


def _host_batch(keep):
    """A batch whose pointers are host arrays: only good for calls that return
    before any launch."""
    b = N.Batch()
    arr = np.zeros(64)
    keep.append(arr)
    b.problems = b.cand = b.l_out = b.g_out = arr.ctypes.data
    b.n_problems, b.total_cand, b.flags = 1, 4096, N.BATCH_WRITE_CAND
    return b


@pytest.mark.parametrize('k', [0, 65, -1])
def test_k_out_of_range_is_rejected(k):
    lib, keep = N.load(), []
    b = _host_batch(keep)
    out = np.zeros(1 << 16, dtype=np.uint8)
    p = out.ctypes.data
    assert _report(lib, ctypes.byref(b), k, p, p, p, p, out.nbytes) == -1
    assert b'k outside' in lib.tpe_last_error()


def test_missing_buffers_flag_and_scratch_are_rejected():
    lib, keep = N.load(), []
    out = np.zeros(1 << 16, dtype=np.uint8)
    p = out.ctypes.data
    for field in ('cand', 'l_out', 'g_out'):
        b = _host_batch(keep)
        setattr(b, field, None)
        assert _report(lib, ctypes.byref(b), 8, p, p, p, p, out.nbytes) == -1, field
        assert b'null cand' in lib.tpe_last_error()
    b = _host_batch(keep)
    b.flags = 0
    assert _report(lib, ctypes.byref(b), 8, p, p, p, p, out.nbytes) == -1
    assert b'TPE_BATCH_WRITE_CAND' in lib.tpe_last_error()
    b = _host_batch(keep)
    need = ctypes.c_uint64(0)
    assert lib.tpe_report_scratch_bytes(N.report_chunks(1, 4096), 8, ctypes.byref(need)) == 0
    assert _report(lib, ctypes.byref(b), 8, p, p, p, p, need.value - 1) == -1
    assert b'scratch too small' in lib.tpe_last_error()
    assert _report(lib, ctypes.byref(b), 8, p, p, p, None, need.value) == -1
    assert _report(lib, ctypes.byref(b), 8, None, p, p, p, need.value) == -1


@pytest.mark.parametrize('chunks,k', [(1, 1), (3, 8), (4096, 64)])
def test_scratch_bytes_formula(chunks, k):
    """n_chunks_total * (80-B chunk record + k 32-B entries)."""
    lib = N.load()
    nb = ctypes.c_uint64(0)
    assert lib.tpe_report_scratch_bytes(chunks, k, ctypes.byref(nb)) == 0
    assert nb.value == chunks * (80 + 32 * k)


def test_scratch_bytes_rejects_bad_arguments():
    lib = N.load()
    nb = ctypes.c_uint64(0)
    assert lib.tpe_report_scratch_bytes(1, 0, ctypes.byref(nb)) == -1
    assert lib.tpe_report_scratch_bytes(1, 65, ctypes.byref(nb)) == -1
    assert lib.tpe_report_scratch_bytes(-1, 8, ctypes.byref(nb)) == -1
    assert lib.tpe_report_scratch_bytes(1, 8, None) == -1


def test_report_profile_has_nothing_to_read_before_a_profiled_call():
    lib = N.load()
    ms = (ctypes.c_double * 2)()
    assert lib.tpe_report_profile(0, ms) == -1
    assert b'tpe_report_profile' in lib.tpe_last_error()
    assert lib.tpe_report_profile(0, None) == 0


def test_report_chunks():
    assert N.report_chunks(0, 0) == 0 and N.report_chunks(3, 0) == 0
    assert N.report_chunks(1, 1) == 1 and N.report_chunks(1, 4096) == 1 and N.report_chunks(1, 4097) == 2
    assert N.report_chunks(3, 3 * 12305) == 3 * 4
    assert N.report_chunks(4, 4 << 20) == 4 * 256


def _space():
    from hyperopt_amd import base, hp
    return base.Domain(lambda d: 0.0, {'x': hp.uniform('x', -10, 10), 'c': hp.choice('c', [0, 1, 2])})


@pytest.mark.parametrize('k', [0, 65])
def test_candidate_report_rejects_k_before_any_device_use(k, monkeypatch):
    from hyperopt_amd import base, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **kw: pytest.fail('the engine was touched'))
    with pytest.raises(ValueError, match='k must be'):
        tpe.candidate_report(0, _space(), base.Trials(), 1234, k=k)


def test_candidate_report_rejects_an_empty_history_before_any_device_use(monkeypatch):
    from hyperopt_amd import base, tpe
    monkeypatch.setattr(tpe, 'get_engine', lambda *a, **kw: pytest.fail('the engine was touched'))
    with pytest.raises(ValueError, match='history'):
        tpe.candidate_report(0, _space(), base.Trials(), 1234, k=8)
