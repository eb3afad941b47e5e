"""The numpy statement of the joint candidate report (include/tpe_hip.h "Joint
candidate report"): the k best distinct candidate rows of one problem and the
statistics of its scores."""
import math

import numpy as np


def rank_order(l, g):
    """np.argmax order of s = l - g: NaN first (equal to each other), then
    descending (+-inf ordinary values), ties to the lower index."""
    with np.errstate(invalid='ignore'):
        s = np.asarray(l, dtype=np.float64) - np.asarray(g, dtype=np.float64)
    i = np.arange(len(s))
    nan = np.isnan(s)
    return np.lexsort((i, np.where(nan, 0.0, -s), ~nan))


def top_distinct_rows(cand, l, g, k):
    """Indices of the first k candidates, in rank order, whose row [W] equals
    no kept candidate's row: all coordinates ==, so -0 equals +0 and a row with
    a NaN coordinate equals nothing (it is always kept)."""
    cand = np.asarray(cand, dtype=np.float32)
    out, seen = [], set()
    for j in rank_order(l, g):
        row = cand[j] + np.float32(0.0)                 # -0 -> +0
        if np.isnan(row).any():
            out.append(j)
        else:
            key = tuple(row.tolist())
            if key in seen:
                continue
            seen.add(key)
            out.append(j)
        if len(out) == k:
            break
    return np.asarray(out, dtype=np.int64)


def n_distinct_rows(cand):
    cand = np.asarray(cand, dtype=np.float32) + np.float32(0.0)
    nan = np.isnan(cand).any(axis=1)
    return int(nan.sum()) + len(set(tuple(r.tolist()) for r in cand[~nan]))


def score_stats(l, g):
    """dict(n_finite, n_nan, n_posinf, n_neginf, mean, m2, min, max, mean_abs):
    tpe_score_stats in float64 numpy (none finite: mean, min, max NaN, m2 0)."""
    with np.errstate(invalid='ignore'):
        s = np.asarray(l, dtype=np.float64) - np.asarray(g, dtype=np.float64)
    fin = s[np.isfinite(s)]
    out = dict(n_finite=len(fin), n_nan=int(np.isnan(s).sum()), n_posinf=int((s == np.inf).sum()),
               n_neginf=int((s == -np.inf).sum()), mean=math.nan, m2=0.0, min=math.nan, max=math.nan, mean_abs=0.0)
    if len(fin):
        mean = fin.mean()
        out.update(mean=mean, m2=float(np.sum((fin - mean) ** 2)), min=fin.min(), max=fin.max(),
                   mean_abs=float(np.mean(np.abs(fin))))
    return out


def check_report(cand, l, g, k, top, z, n_top, stats, what):
    """One problem's device report (top [k] of N.JOINT_TOP_ENTRY_DTYPE, z [k,
    >= W] f32, n_top, stats) against this file.  Indices, l, g, rows, n_top,
    counts, min and max exactly; mean within 1e-10 mean|s| and m2 within 1e-9
    relative (the bounds of tests/test_gpu_report.py: two float64 summations
    of n <= 2^16 terms).  Returns the reference indices."""
    cand = np.asarray(cand, dtype=np.float32)
    W = cand.shape[1]
    ref = top_distinct_rows(cand, l, g, k)
    assert int(n_top) == len(ref) == min(k, n_distinct_rows(cand)), (what, int(n_top), len(ref))
    n = len(ref)
    np.testing.assert_array_equal(top['idx'][:n], ref, err_msg=str(what))
    assert top['l'][:n].tobytes() == np.asarray(l, dtype=np.float64)[ref].tobytes(), what
    assert top['g'][:n].tobytes() == np.asarray(g, dtype=np.float64)[ref].tobytes(), what
    assert np.ascontiguousarray(z[:n, :W]).tobytes() == cand[ref].tobytes(), what      # bit for bit (-0 stays -0)
    assert not z[:n, W:].any() and not z[n:].any(), what
    rest = top[n:]
    assert (rest['idx'] == -1).all() and not rest['l'].any() and not rest['g'].any(), what
    assert not top['reserved'].any(), what
    want = score_stats(l, g)
    for f in ('n_finite', 'n_nan', 'n_posinf', 'n_neginf'):
        assert int(stats[f]) == want[f], (what, f)
    if want['n_finite'] == 0:
        assert math.isnan(stats['mean']) and math.isnan(stats['min']) and math.isnan(stats['max']), what
        assert stats['m2'] == 0.0, what
        return ref
    assert stats['min'] == want['min'] and stats['max'] == want['max'], what
    print(what, 'mean err', abs(stats['mean'] - want['mean']), 'bound', 1e-10 * want['mean_abs'],
          'm2 rel err', abs(stats['m2'] - want['m2']) / want['m2'] if want['m2'] else 0.0)
    assert abs(stats['mean'] - want['mean']) <= 1e-10 * want['mean_abs'], what
    assert abs(stats['m2'] - want['m2']) <= 1e-9 * want['m2'], what
    return ref
