"""The fused hit's prepared image (DESIGN.md section 3 "Two hit paths").

Host: the run descriptors (tpe_debug_fast_runs) against a restatement of the
sample stage's partition — workgroup w takes list entries [w per, (w + 1) per),
consecutive tiles of one problem are a run.

GPU: a live level's images (tpe_debug_fast_image) against numpy on the staging
buffer's f64 sampler rows: the cumulative masses, the f32 rows and the guide
entries {t0, t1, k0, never}, bit for bit."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _native as N

K_GUIDE, K_SAMP, HDR_UNITS, IMG_UNITS = 256, 64, 8, 616
MAX_PER = 16                                  # kTabMaxTilesPerWg


def _runs(n_problems, tpp, per):
    lib = N.load()
    cap = n_problems * tpp * 2 + 64
    out = np.zeros((cap, 8), np.int32)
    runs = ctypes.c_int32(0)
    n = lib.tpe_debug_fast_runs(n_problems, tpp, per, out.ctypes.data, cap, ctypes.byref(runs))
    assert n >= 0, n
    return out[:n], runs.value


def _restated(n_problems, tpp, per, tile):
    n_tab = n_problems * tpp
    wgs = []
    for w in range((n_tab + per - 1) // per):
        runs = []
        for i in range(w * per, min(n_tab, (w + 1) * per)):
            pid, k = divmod(i, tpp)
            if runs and runs[-1][0] == pid:
                runs[-1][2] += 1
            else:
                runs.append([pid, k * tile, 1])
        wgs.append(runs)
    return wgs


@pytest.mark.parametrize('n_problems', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('tpp', [1, 2, 3, MAX_PER + 1])
@pytest.mark.parametrize('per', [1, 2, 3, MAX_PER])
def test_run_descriptors_follow_the_partition(n_problems, tpp, per):
    tile = N.load().tpe_tile_size()
    got, runs = _runs(n_problems, tpp, per)
    want = _restated(n_problems, tpp, per, tile)
    assert runs == max(len(r) for r in want) and len(got) == runs * len(want)
    covered = np.zeros((n_problems, tpp), int)
    for w, rs in enumerate(want):
        slots = got[w * runs:(w + 1) * runs]
        for j, (pid, start, n) in enumerate(rs):
            assert tuple(slots[j, :3]) == (pid, start, n), (w, j)
            assert slots[j, 3] == pid * IMG_UNITS
            covered[pid, start // tile:start // tile + n] += 1
        assert not slots[len(rs):, 2].any()              # the unused slots say "no run"
    assert (covered == 1).all()


def _guide(cum):
    """GuideEnt {t0, t1, k0, never} of every b: k0 the first k with cum_k >
    b / 256 (clipped to the last row); t0, t1 the thresholds ceil(c 2^32 - 0.5)
    of cum[k0] and cum[k0 + 1] on the draw's 32-bit word — a step at or past
    the last row, or a threshold of 2^32, is never passed (all ones, its
    `never` bit set)."""
    n = len(cum)
    k0 = np.minimum(np.searchsorted(cum, np.arange(K_GUIDE) / K_GUIDE, side='right'), n - 1)
    out = np.zeros((K_GUIDE, 4), np.uint32)
    out[:, 2] = k0
    for step in (0, 1):
        k = k0 + step
        c = np.where(k < n - 1, cum[np.minimum(k, n - 1)], np.inf)
        t = np.ceil(c * 4294967296.0 - 0.5)
        never = ~(t < 4294967296.0)
        out[:, step] = np.where(never, 0xffffffff, np.maximum(np.where(never, 0.0, t), 0.0)).astype(np.uint32)
        out[:, 3] |= never.astype(np.uint32) << step
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['one row, nine cells', 'two rows', '26 rows', 'svm', 'rf'])
def test_image_equals_the_staged_sampler_rows(name):
    """Every tabulated row of a live level: the image's cumulative masses, f32
    sampler rows and guide, bit for bit, against numpy on the f64 sampler rows
    the staging buffer holds; an untabulated row has no image."""
    import bench
    from hyperopt_amd import tpe
    from hyperopt_amd.engine import get_engine
    from tests import fast_image_cases as FC
    if not N.level_resident(1)[0]:
        pytest.skip('TPE_RESIDENT_LEVEL=0')
    if name in ('svm', 'rf'):
        domain, trials = bench.make_history(600, 0, loss=None if name == 'svm' else bench.rf_loss)
        gamma = 0.25
    else:
        domain, trials, gamma, _ = FC.cases()[name]
    C, n = 1 << 16, len(trials.trials)
    info = FC.level(domain, trials, C, gamma)[1]
    eng = get_engine()
    seen = 0
    for r in range(int(info.n_problems)):
        # a miss (the debug entry ends the record): the record, its images, the staged level
        tpe.suggest([n], domain, trials, 11, n_EI_candidates=C, gamma=gamma, n_startup_jobs=0)
        rows, samp, _ = FC.staged(eng, info)
        buf = np.zeros(IMG_UNITS * 16, np.uint8)
        rc = eng.lib.tpe_debug_fast_image(r, buf.ctypes.data, buf.nbytes)
        if rows[r]['tab_mode'] == N.TAB_NONE:
            assert rc != 0, r
            continue
        assert rc == 0, (r, rc)
        ln, off = int(rows[r]['samp_len']), int(rows[r]['samp_off'])
        assert int(buf[48:64].view(np.int32)[2]) == ln and 1 <= ln <= K_SAMP
        cum = buf[HDR_UNITS * 16:][:K_SAMP * 8].view(np.float64)
        f32 = buf[HDR_UNITS * 16 + K_SAMP * 8:][:K_SAMP * 16].view(np.uint32).reshape(K_SAMP, 4)
        guide = buf[HDR_UNITS * 16 + K_SAMP * 24:][:K_GUIDE * 16].view(np.uint32).reshape(K_GUIDE, 4)
        s = samp[off:off + ln]
        sg = s[:, 2].astype(np.float32)
        want = np.stack([s[:, 1].astype(np.float32), np.where(s[:, 5] != 0.0, -sg, sg), s[:, 3].astype(np.float32),
                         s[:, 4].astype(np.float32)], axis=1)
        assert cum[:ln].tobytes() == s[:, 0].tobytes() and not cum[ln:].any()
        assert np.array_equal(f32[:ln], want.view(np.uint32)) and not f32[ln:].any()
        assert np.array_equal(guide, _guide(s[:, 0])), r
        seen += 1
    assert seen >= 1
