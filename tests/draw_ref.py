"""The univariate device draw, restated in numpy: what candidate g of a
(seed, label, id) must be, independent of the package and of anything native.

Sources restated here (text, not code that is imported):
  csrc/tpe_device_rng.h     philox4x32_10, u01f, u01d, u01w, ndtri_f32's bound
  csrc/tpe_kernels.hip      draw_uniforms (counter layout), find_comp,
                            f32_bounds, comp_coord_f32, draw_comp
  parzen.sampler_table      its docstring: rows {cum, mu, sigma, fa, fb, flip}

An f32 draw is returned as a bracket [t_lo, t_hi] of its kernel coordinate
(and [x_lo, x_hi] of its value): the device evaluates Phi^-1 with ndtri_f32,
whose header states a relative error bound, and forms pr and mu + sigma z in
f32, where the compiler may or may not contract to an fma.  Every term of the
bracket is one of those statements; none is tuned:

  pr       np.float32 fa + uf (fb - fa), inverted at pr - 1 ulp and pr + 1 ulp
  z        scipy.special.ndtri in float64, each end widened by NDTRI_F32_REL |z|
  t        f32(mu) + f32(sigma) z in float64, each end widened by 2 f32 ulps of
           max(|mu|, |sigma z|)

An f64 draw has the same bracket with f64 ulps, scipy.special.erfcinv, and the
relative widening ERFCINV_REL on z for the device's erfcinv (measured on the
device over tests/test_gpu_draws.py's own draws, times 4; see there).

Ordered draws (TPE_BATCH_ORDERED_DRAWS, a debug flag) are outside this model.
"""
import math

import numpy as np
from scipy.special import erfcinv, ndtri

# the sampler rows take erfc from the C library (math.erfc), as parzen.sampler_table's
# docstring says: scipy.special.erfc differs from it in the last bits (up to 371 ulps
# of fa in the far tail), and the rows are compared bit for bit with both packers
_erfc_each = np.frompyfunc(math.erfc, 1, 1)


def erfc(x):
    return _erfc_each(np.asarray(x, dtype=np.float64)).astype(np.float64)

GAUSS, LOGGAUSS, QGAUSS, QLOGGAUSS, CATEGORICAL = 0, 1, 2, 3, 4
FAMILY = {'uniform': GAUSS, 'normal': GAUSS, 'quniform': QGAUSS, 'qnormal': QGAUSS,
          'loguniform': LOGGAUSS, 'lognormal': LOGGAUSS, 'qloguniform': QLOGGAUSS, 'qlognormal': QLOGGAUSS,
          'randint': CATEGORICAL, 'categorical': CATEGORICAL}

# tpe_device_rng.h: "Relative error <= 3e-7 over the f32 uniforms"
NDTRI_F32_REL = 3e-7
# device erfcinv against scipy's: 4 x the worst excess measured on an MI355X over
# test_gpu_draws.py's f64 draws, 5.67e-16 |z| (test_every_candidate's docstring);
# must stay <= 1e-12
ERFCINV_REL = 4 * 5.67e-16
# exp of the log families: the device's and numpy's f64 exp are each within an ulp
EXP_ULPS = 2

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _family(family):
    return FAMILY[family] if isinstance(family, str) else int(family)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32 with 10 rounds (Salmon et al., Random123): four uint32
    arrays from the counter words c0..c3 and the key (k0, k1); uint64
    arithmetic, broadcasting."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                  # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO32, p1 >> _S32, p1 & _LO32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def u01f(r):
    """23-bit f32 uniform in [2^-24, 1 - 2^-24]: ((r >> 9) + 0.5) 2^-23, exact."""
    r = np.asarray(r, dtype=np.uint32)
    return ((r >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def u01d(a, b):
    """53-bit f64 uniform: m = (a << 21) ^ (b >> 11), (m + 0.5) 2^-53."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    m = (a << np.uint64(21)) ^ (b >> np.uint64(11))
    return (m.astype(np.float64) + 0.5) * 2.0 ** -53


def u01w(a):
    """32-bit uniform as an f64 in (0, 1): (a + 0.5) 2^-32, exact."""
    return (np.asarray(a, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def sampler_rows(family, w=None, mu=None, sigma=None, low=None, high=None, p=None):
    """Sampler rows [K, 8] = {cum, mu, sigma, fa, fb, flip, 0, 0} of a below
    mixture, from parzen.sampler_table's docstring: rejection sampling of a
    bounded mixture accepts component k with probability proportional to
    w_k mass_k and then draws a normal truncated to [low, high), inverted at
    fa + u (fb - fa); the standardised interval is mirrored (flip) when its low
    end is > 0, so fa and fb are small numbers, not numbers near 1.  cum is the
    normalised running sum with its last entry 1; a categorical has cum of p."""
    if _family(family) == CATEGORICAL:
        p = np.asarray(p, dtype=np.float64)
        rows = np.zeros((len(p), 8))
        cum = np.cumsum(p) / np.sum(p)
        cum[-1] = 1.0
        rows[:, 0] = cum
        return rows
    w, mu, sigma = (np.asarray(v, dtype=np.float64) for v in (w, mu, sigma))
    K = len(w)
    rows = np.zeros((K, 8))
    bounded = low is not None or high is not None
    if bounded:
        za, zb = (low - mu) / sigma, (high - mu) / sigma
    else:
        za, zb = np.full(K, -np.inf), np.full(K, np.inf)
    flip = za > 0
    a, b = np.where(flip, -zb, za), np.where(flip, -za, zb)
    fa, fb = 0.5 * erfc(-a / np.sqrt(2)), 0.5 * erfc(-b / np.sqrt(2))
    sel = w * np.maximum(fb - fa, 0.0) if bounded else w * 1.0
    if not np.any(sel > 0):
        sel = w * 1.0
    cum = np.cumsum(sel) / np.sum(sel)
    cum[-1] = 1.0
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = cum, mu, sigma, fa, fb, flip
    return rows


def f32_bounds(low, high):
    """(smallest float >= low, largest float < high); +-inf where unbounded."""
    lo_f, hi_f = np.float32(-np.inf), np.float32(np.inf)
    if low is not None:
        lo_f = np.float32(low)
        if float(lo_f) < low:
            lo_f = np.nextafter(lo_f, np.float32(np.inf))
    if high is not None:
        hi_f = np.float32(high)
        while float(hi_f) >= high:
            hi_f = np.nextafter(hi_f, np.float32(-np.inf))
    return lo_f, hi_f


def uniforms(family, seed, label_ix, new_id, g, precision):
    """draw_uniforms: (us, uf, ud, ws) of the global candidate indices g.  Key =
    the seed's low and high words; counter words 2, 3 = the label index and the
    id's low word.  f32 non-categorical: block g >> 1, words (x, y) for even g,
    (z, w) for odd g (32-bit selection, 23-bit inversion); f64 and categorical:
    block g, u01d(x, y) selects, u01d(z, w) inverts."""
    g = np.asarray(g, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c2, c3 = int(label_ix) & 0xFFFFFFFF, int(new_id) & 0xFFFFFFFF
    if precision == 'fp32' and _family(family) != CATEGORICAL:
        blk = g >> np.uint64(1)
        x, y, z, w = philox4x32_10(blk & _LO32, blk >> _S32, c2, c3, k0, k1)
        odd = (g & np.uint64(1)).astype(bool)
        ws = np.where(odd, z, x)
        return u01w(ws), u01f(np.where(odd, w, y)), None, ws
    x, y, z, w = philox4x32_10(g & _LO32, g >> _S32, c2, c3, k0, k1)
    return u01d(x, y), None, u01d(z, w), None


def component(cum, us):
    """The first k with u < cum_k, capped at K - 1."""
    return np.minimum(np.searchsorted(cum, us, side='right'), len(cum) - 1).astype(np.int64)


class Draws(object):
    """comp [n]; t_lo, t_hi: the kernel coordinate's bracket (x, or ln x for the
    log families, before quantisation); x_lo, x_hi: the value's bracket (for a
    quantised label both ends are lattice points: equal unless the coordinate
    bracket straddles a rounding edge); t, x: the model's point draw; z, scale:
    the point's standard normal and max(|mu|, |sigma z|) (for error measurements)."""
    __slots__ = ('comp', 't_lo', 't_hi', 'x_lo', 'x_hi', 't', 'x', 'z', 'scale', 'sigma', 'clipped')

    def inside(self, x):
        return (x >= self.x_lo) & (x <= self.x_hi)

    def either(self):
        """Candidates whose bracket ends quantise to different lattice points."""
        return self.x_lo != self.x_hi


def _ulp(v, dtype):
    return np.spacing(np.abs(v).astype(dtype)).astype(np.float64)


def _step(pr, direction, dtype):
    return np.nextafter(pr, dtype(direction))


def draw(family, rows, low, high, q, seed, label_ix, new_id, g, precision, ndtri_rel=NDTRI_F32_REL,
         erfcinv_rel=ERFCINV_REL):
    """Candidates g (global indices) of one problem: a Draws."""
    fam = _family(family)
    us, uf, ud, _ = uniforms(fam, seed, label_ix, new_id, g, precision)
    rows = np.asarray(rows, dtype=np.float64)
    comp = component(rows[:, 0], us)
    d = Draws()
    d.comp = comp
    if fam == CATEGORICAL:
        v = comp.astype(np.float64)
        d.t_lo = d.t_hi = d.x_lo = d.x_hi = d.t = d.x = v
        d.z = d.scale = d.sigma = np.zeros(len(v))
        d.clipped = np.zeros(len(v), dtype=bool)
        return d
    mu, sg, fa, fb = rows[comp, 1], rows[comp, 2], rows[comp, 3], rows[comp, 4]
    flip = rows[comp, 5] != 0
    with np.errstate(all='ignore'):
        if precision == 'fp32':
            fa32, fb32 = fa.astype(np.float32), fb.astype(np.float32)
            pr = fa32 + uf * (fb32 - fa32)                              # np.float32, two roundings
            tiny, top = np.float32(1e-45), np.float32(1.0 - 2.0 ** -24)
            p_lo = np.clip(_step(pr, -1, np.float32), tiny, top).astype(np.float64)
            p_hi = np.clip(_step(pr, 2, np.float32), tiny, top).astype(np.float64)
            z_lo, z_hi, z = ndtri(p_lo), ndtri(p_hi), ndtri(np.clip(pr, tiny, top).astype(np.float64))
            rel, ft = ndtri_rel, np.float32
            mu_d, sg_d = mu.astype(np.float32).astype(np.float64), sg.astype(np.float32).astype(np.float64)
        else:
            pr = fa + ud * (fb - fa)
            tiny, top = 5e-324, 1.0 - 2.0 ** -53
            p_lo = np.clip(_step(pr, -1, np.float64), tiny, top)
            p_hi = np.clip(_step(pr, 2, np.float64), tiny, top)
            inv = lambda v: -np.sqrt(2.0) * erfcinv(2.0 * v)
            z_lo, z_hi, z = inv(p_lo), inv(p_hi), inv(np.clip(pr, tiny, top))
            rel, ft = erfcinv_rel, np.float64
            mu_d, sg_d = mu, sg
        z_lo, z_hi = z_lo - rel * np.abs(z_lo), z_hi + rel * np.abs(z_hi)
        z_lo, z_hi = np.where(flip, -z_hi, z_lo), np.where(flip, -z_lo, z_hi)
        z = np.where(flip, -z, z)
        scale = np.maximum(np.abs(mu_d), np.abs(sg_d * z))
        slack = 2 * _ulp(scale, ft)
        t_lo, t_hi, t = mu_d + sg_d * z_lo - slack, mu_d + sg_d * z_hi + slack, mu_d + sg_d * z
        nan = ~((t_lo == t_lo) & (t_hi == t_hi) & (t == t))
        t_lo, t_hi, t = (np.where(nan, mu_d, v) for v in (t_lo, t_hi, t))
        # low <= draw < high
        if precision == 'fp32':
            lo_c, hi_c = (float(v) for v in f32_bounds(low, high))
        else:
            lo_c = -np.inf if low is None else float(low)
            hi_c = np.inf if high is None else float(np.nextafter(high, -np.inf))
        d.clipped = (t_lo < lo_c) | (t_hi > hi_c)
        t_lo, t_hi, t = (np.minimum(np.maximum(v, lo_c), hi_c) for v in (t_lo, t_hi, t))
        x_lo, x_hi, x = t_lo, t_hi, t
        if fam in (LOGGAUSS, QLOGGAUSS):
            x_lo, x_hi, x = np.exp(t_lo), np.exp(t_hi), np.exp(t)
            x_lo, x_hi = x_lo - EXP_ULPS * _ulp(x_lo, np.float64), x_hi + EXP_ULPS * _ulp(x_hi, np.float64)
        if fam in (QGAUSS, QLOGGAUSS):
            x_lo, x_hi, x = (np.round(v / q) * q for v in (x_lo, x_hi, x))
    d.t_lo, d.t_hi, d.t, d.x_lo, d.x_hi, d.x = t_lo, t_hi, t, x_lo, x_hi, x
    d.z, d.scale, d.sigma = z, scale, sg_d
    return d
