"""The joint TPE model with quantised labels at the widths of the wide quantised
stage (DESIGN.md "Quantised labels in wide groups"), in plain numpy on top of
tests/joint_quant_ref.py: nothing here calls hyperopt_amd.joint or the native
library.  The model is the quantised stage's, so the density is
joint_quant_ref.ref_quant_lpdf evaluated in blocks small enough for 64
coordinates; what is new here are the seeded cases at those widths, one of
them with a qloguniform lattice."""
import math

import numpy as np

from tests import joint_quant_ref as Q

WIDE_MAX_DIMS, WIDE_MAX_CAT, MAX_QUANT = 64, 8, 4
NARROW_MAX_DIMS, NARROW_MAX_CONT, NARROW_MAX_DISC = 16, 8, 4
WQ_TILE_BYTES = 26 * 1024                 # the table tile's share of a workgroup's LDS


def ref_wide_quant_lpdf(z, v, qi, side, low, high, ps, s, edges):
    """float64 log p(z, v, i) of joint_quant_ref.ref_quant_lpdf at up to 64
    coordinates: the [candidates, components, dimensions] temporary is kept
    below 2^24 elements."""
    w, mu = side[0], side[1]
    block = max(1, min(2048, (1 << 24) // max(1, len(w) * max(1, mu.shape[1]))))
    return Q.ref_quant_lpdf(z, v, qi, side, low, high, ps, s, edges, block=block)


def takes_wide_stage(Dc, Dk, Dq):
    """Whether a root group of Dc continuous, Dk discrete and Dq >= 1 quantised
    labels is past the quantised stage's limits."""
    return Dq > 0 and (Dc + Dk + Dq > NARROW_MAX_DIMS or Dc > NARROW_MAX_CONT or Dk > NARROW_MAX_DISC)


def dp_of(Dc):
    """The padded continuous width of the scoring kernel."""
    for dp in (16, 24, 32, 48, 64):
        if Dc <= dp:
            return dp
    raise ValueError(Dc)


def tile_of(Dc, total):
    """Components per LDS tile of the scoring kernel for Dc continuous
    coordinates and ``total`` lattice values: the longest multiple of 8, at
    most the wide stage's tile, whose table tile [total + 1][tile + 4] f32
    fits WQ_TILE_BYTES (8 at the least)."""
    dp = dp_of(Dc)
    tk = 128 if dp <= 32 else (4096 // dp) & ~7
    for t in range(tk, 7, -8):
        if (total + 1) * (t + 4) * 4 <= WQ_TILE_BYTES:
            return t
    return 8


def scratch_bytes(n_ids, n_cand, Dc, Dk, Dq):
    """tpe_joint_wide_quant_scratch_bytes: one 536-byte record per chunk of
    256 R candidates (R = 2 up to 32 continuous coordinates, else 1), then the
    f32 candidate blocks of 256 over all coordinates."""
    per = 256 * (2 if Dc <= 32 else 1)
    chunks = (n_cand + per - 1) // per
    blocks = (n_cand + 255) // 256
    return n_ids * chunks * 536 + n_ids * blocks * 256 * (Dc + Dk + Dq) * 4


QLOG37 = ('qloguniform', math.log(16.0), math.log(592.0), 16.0)       # the 37 values 16, 32, .., 592


def wide_quant_case(Dc, us, Vs, n, qlog=False):
    """joint_quant_ref.seeded_quant_case at any width (its own seed).  ``qlog``
    (with Vs == [37]): the quantised dimension is QLOG37, its edges those of
    the qloguniform lattice in the log coordinate and its components the
    case's, carried affinely from [0, V - 1] onto [low, high]."""
    seed = 7000000 + 100000 * len(Vs) + 1000 * Dc + 10 * len(us) + n
    below, above, low, high, ps, sb, sa, edges, rs = Q.seeded_quant_case(Dc, list(us), list(Vs), n, seed=seed)
    if qlog:
        assert list(Vs) == [37]
        m_lo, V, e = Q.ref_lattice(*QLOG37)
        assert (m_lo, V) == (1, 37)
        lo, hi = QLOG37[1], QLOG37[2]
        scale = (hi - lo) / (V - 1.0)
        below = below[:4] + (lo + below[4] * scale, below[5] * scale)
        above = above[:4] + (lo + above[4] * scale, above[5] * scale)
        edges = [e]
    return below, above, low, high, ps, sb, sa, edges, rs
