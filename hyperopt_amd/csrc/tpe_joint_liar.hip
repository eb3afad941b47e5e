// MI355X (gfx950) batch-aware joint suggests: the greedy "liar" stage that runs
// after a joint stage (include/tpe_hip.h, "Batch-aware joint suggests" and
// "Batch-aware picks over discrete and quantised labels").  Id j picks under the
// above mixture extended by the vectors the ids before it picked (and the given
// ones), each a component of un-normalised weight 1.  Nothing on the default
// suggest path runs through this file.
//
// Every kernel exists in two instantiations of one template.  <false> serves a
// group of continuous labels (tpe_joint_liar); <true> a group that also holds
// discrete and / or quantised labels (tpe_joint_liar_mixed): a candidate row is
// then [z (f32) | category index | lattice index], a liar's discrete factor is
// that of a trial component of the above side and its quantised factor the
// binned normal at the picked lattice value's fit coordinate.  What only <true>
// needs sits under `if constexpr (kMixed)` and in LiarMK / PickLds<true>: the
// continuous instantiation holds none of it, in registers, LDS or arguments.
//
// k_liar_pick   one 256-thread workgroup per step: merges the previous step's
//               chunk records in index order, copies the winner's row, then
//               fits the new liar's bandwidths (the adaptive-Parzen neighbour
//               rule over the K_above f32 mu values and the earlier liars of
//               each dimension, float64 on f32 values: exact) and writes its
//               float64 row {mu[Dc], sqrt(1/2) / sigma[Dc], c}.  <true>: the
//               row goes on with {cat[Dk], centre[Dq]}: the category copy, a
//               float64 sweep over above_qmu and the earlier centres, then the
//               liar's bin tables T_i[d][v] = log Q_i(v), one thread per lattice
//               value, the V_d + 1 tails once through LDS.  Step 0 adds the
//               given liars one after the other.
// k_liar_chunk  one 256-thread workgroup per chunk of TPE_JOINT_CHUNK
//               consecutive candidates of ONE id: the liar rows stream through
//               LDS in tiles of TPE_JOINT_LIAR_TILE, a lane accumulates
//               sum_d ((z_d - mu_d) / (sigma_d sqrt 2))^2 of four liars at a
//               time in float64 (subtract, then scale), keeps a running
//               maximum, finishes against the stored g and writes the chunk
//               winner through the butterfly on (score key, index).  <true>:
//               per (candidate, liar) also one compare-select-add per discrete
//               dimension and one table read (through L1 / L2, at the
//               candidate's own lattice index) per quantised one; sum_d
//               miss_d(v_d) depends on the candidate alone and is added after
//               the sum over the liars.
// The bodies of the two kernels are device functions (pick_step, chunk_step,
// add_liar) over a view of ONE group, so that the segmented stage
// (tpe_joint_liar_seg, "Batch-aware picks in branch groups": one greedy chain per
// group of a tpe_joint_seg_run) runs the same code:
// k_liar_seg_chunk  round r, grid (chunks) x (groups with more than r problems):
//               the workgroup reads its group's descriptor from device memory
//               and runs chunk_step<false> over problem chain[first + r].
// k_liar_seg_pick   round r, one workgroup per such group: pick_step<false>.
// k_liar_mseg_chunk / k_liar_mseg_pick   the same rounds after a tpe_joint_mseg_run
//               (tpe_joint_liar_mseg, "Batch-aware picks in mixed branch
//               groups"): the <true> bodies over SegMView, whose per-dimension
//               arrays point into the group's descriptor; a continuous group
//               is their case Dk = Dq = 0.
// The steps are ordered by the stream alone: no workgroup waits on another, no
// atomics, every reduction has a fixed shape, so the output bytes are a
// function of the input bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "../../include/tpe_hip.h"

extern "C" int tpe_internal_fail(int code, const char* what);   // tpe_kernels.hip (hidden)
extern "C" void tpe_internal_epoch_bump(void);                    // tpe_kernels.hip (hidden): the device epoch

namespace {

constexpr int kThreads = 256;                       // 4 waves of 64
constexpr int kR = TPE_JOINT_CHUNK / kThreads;      // candidates per lane
constexpr int kTile = TPE_JOINT_LIAR_TILE;          // liars per LDS tile
constexpr int kQ = 4;                               // liars a lane accumulates at once
constexpr int kMaxD = TPE_JOINT_WIDE_MAX_DIMS;
constexpr int kMaxK = TPE_JOINT_MAX_DIMS;           // discrete dimensions
constexpr int kMaxQ = TPE_JOINT_MAX_QUANT;
constexpr int kMaxV = TPE_JOINT_MAX_LATTICE;
constexpr int kMaxRow = 2 * kMaxD + 1;              // doubles of a liar row: 2 Dc + 1 + Dk + Dq, with Dc + Dk + Dq <= 64
constexpr double kSqrtHalf = 0.70710678118654752440;
constexpr double kTailMax = 26.5;                   // joint.QUANT_TAIL_MAX
static_assert(kR * kThreads == TPE_JOINT_CHUNK && kTile % kQ == 0, "chunk and tile shapes");
static_assert(sizeof(tpe_joint_pick) == 24, "layout");
static_assert(offsetof(tpe_joint_liar_mixed_args, n_cat) == sizeof(tpe_joint_liar_args), "the shared prefix");
static_assert(kMaxV <= kThreads, "one thread per lattice value");

struct LiarK {                  // what both instantiations take
  int D, C, n_chunks, K, G, n;  // D: the width of a candidate row
  const float* cand;
  const double *l_out, *g_out;
  const float* amu;
  const float* given;
  double* rows;                 // scratch [(G + n_ids) * LS]
  tpe_joint_pick* chunk_rec;    // scratch [n_chunks]: the records of the step that ran last
  tpe_joint_pick* picks;
  float* pick_z;
  double* liar_sigma;
  double psig[kMaxD], low[kMaxD], high[kMaxD];   // [Dc + d]: quantised dimension d (psig only)
};
struct LiarMK : LiarK {         // <true> alone
  int Dc, Dk, Dq, LS, totV;
  const double* aqmu;
  const double *miss, *bonus;   // [sum U_d], natural log
  const double *edges, *centre; // [n_edges], [sum V_d]
  double* tabs;                 // scratch [(G + n_ids) * totV]: log Q_i(v)
  int cat_upper[kMaxK], cat_off[kMaxK];
  int qv[kMaxQ], qeoff[kMaxQ], qtoff[kMaxQ];
};
template <bool kMixed>
using Params = std::conditional_t<kMixed, LiarMK, LiarK>;

// What the two bodies below (pick_step, chunk_step) read of ONE group, for the
// segmented kernels: LiarK's fields of the same names, built in registers from
// the group's device descriptor (psig / low / high point into it).  The solo
// kernels hand the bodies their kernel argument itself; View is either.
struct SegView {
  int D, C, K, n;
  const float* amu;
  const double *l_out, *g_out;
  double* rows;                 // the group's rows in scratch [chain_len * (2 D + 1)]
  double* liar_sigma;           // the group's rows of liar_sigma [chain_len * D]
  const double *psig, *low, *high;
};
// The same for a group of a tpe_joint_mseg_run: LiarMK's fields too.  The
// per-dimension arrays are pointers into the device descriptor, so a lane may
// index them (through a pointer that costs no private copy).
struct SegMView {
  int D, C, K, n;
  int Dc, Dk, Dq, LS, totV;
  const float* amu;
  const double *l_out, *g_out;
  double* rows;                 // [chain_len * LS]
  double* liar_sigma;           // [chain_len * (Dc + Dq)]
  double* tabs;                 // [chain_len * totV]
  const double *psig, *low, *high;
  const double* aqmu;
  const double *miss, *bonus, *edges, *centre;
  const int32_t *cat_upper, *cat_off, *qv, *qeoff, *qtoff;
};
// whether View's per-dimension arrays are pointers (SegMView) or kernel arguments (LiarMK)
template <class View>
constexpr bool kDimsByPointer = std::is_pointer_v<decltype(View::cat_upper)>;

// the continuous dimensions and the doubles of a liar row
template <bool kMixed, class View>
__device__ __forceinline__ int cont_dims(const View& p) {
  if constexpr (kMixed) return p.Dc;
  else return p.D;
}
template <bool kMixed, class View>
__device__ __forceinline__ int row_len(const View& p) {
  if constexpr (kMixed) return p.LS;
  else return 2 * p.D + 1;
}

// np.argmax order of a score as one unsigned key (as tpe_joint.hip)
__device__ __forceinline__ uint64_t score_key(double s) {
  if (s != s) return ~0ull;
  const uint64_t b = (uint64_t)__double_as_longlong(s + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
struct Pick {
  uint64_t key;
  int64_t idx;
};
__device__ __forceinline__ bool beats(const Pick& a, const Pick& b) {
  return a.key > b.key || (a.key == b.key && a.key != 0 && a.idx < b.idx);
}
// the block's best competitor, the same in every thread
__device__ __forceinline__ Pick block_best(Pick p, Pick* slot) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    Pick o;
    o.key = (uint64_t)__shfl_xor((unsigned long long)p.key, m, 64);
    o.idx = (int64_t)__shfl_xor((long long)p.idx, m, 64);
    if (beats(o, p)) p = o;
  }
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = p;
  __syncthreads();
  Pick w = slot[0];
#pragma unroll
  for (int i = 1; i < kThreads / 64; ++i)
    if (beats(slot[i], w)) w = slot[i];
  __syncthreads();
  return w;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the neighbour rule's end: the larger gap (a missing side dropped, none: 0), clipped
__device__ __forceinline__ double neighbour_sigma(double z, double L, double U, bool hasL, bool hasU, double ps, int n,
                                                  int i) {
  double s = 0.0;
  if (hasL) s = z - L;
  if (hasU) s = hasL ? fmax(s, U - z) : U - z;
  const double m = (double)n + (double)i + 1.0;
  return fmin(fmax(s, ps / fmin(100.0, m + 2.0)), ps);
}

// joint.quant_bin_masses' three-way rule on the two smaller tails
__device__ __forceinline__ double bin_mass(double ta, double sa, double tb, double sb) {
  return tb <= 0.0 ? sb - sa : (ta >= 0.0 ? sa - sb : 1.0 - sa - sb);
}

struct PickLdsCont {
  float sL[kThreads], sU[kThreads];
  double sterm[kMaxD];
  Pick slot[kThreads / 64];
};
struct PickLdsMixed : PickLdsCont {
  double dL[kThreads], dU[kThreads];
  double qc[kMaxQ], qs[kMaxQ];
  double st[kMaxV + 1], ss[kMaxV + 1];
};
template <bool kMixed>
using PickLds = std::conditional_t<kMixed, PickLdsMixed, PickLdsCont>;

// Liar `i` (ordinal among all liars) at the f32 row src[D] (nullptr: a row of
// zeros): bandwidths, liar_sigma, the row and (<true>) the bin tables.  S = the
// largest multiple of Dc up to 256 threads scan: thread t serves dimension
// t % Dc and the points t / Dc, t / Dc + S / Dc, ..., so a sweep reads S
// consecutive floats.  zcopy: where the row is also copied to, bit for bit.
template <bool kMixed, class View>
__device__ __forceinline__ void add_liar(const View& p, int i, const float* __restrict__ src,
                                         float* __restrict__ zcopy, PickLds<kMixed>& s) {
  const int t = threadIdx.x, Dc = cont_dims<kMixed>(p), LS = row_len<kMixed>(p);
  int DS = Dc;                                  // the width of a liar_sigma row
  if constexpr (kMixed) DS += p.Dq;
  if (zcopy && t < p.D) zcopy[t] = src ? src[t] : 0.f;
  if (!kMixed || Dc > 0) {
    const int S = (kThreads / Dc) * Dc, d = t % Dc;
    const float zd = src ? src[d] : 0.f;
    float L = -INFINITY, U = INFINITY;          // -inf / +inf: no neighbour on that side
    if (t < S) {
      const int64_t total = (int64_t)p.K * Dc;
      for (int64_t e = t; e < total; e += S) {
        const float x = p.amu[e];
        if (x <= zd) L = fmaxf(L, x);
        else if (x > zd) U = fminf(U, x);
      }
      for (int q = t / Dc; q < i; q += S / Dc) {
        const float x = (float)p.rows[(int64_t)q * LS + d];   // an earlier liar's f32 coordinate
        if (x <= zd) L = fmaxf(L, x);
        else if (x > zd) U = fminf(U, x);
      }
    }
    s.sL[t] = L;
    s.sU[t] = U;
    __syncthreads();
    if (t < Dc) {
      for (int u = t + Dc; u < S; u += Dc) { L = fmaxf(L, s.sL[u]); U = fminf(U, s.sU[u]); }
      const double z = (double)zd;
      const double sg = neighbour_sigma(z, (double)L, (double)U, L != -INFINITY, U != INFINITY, p.psig[d], p.n, i);
      p.liar_sigma[(int64_t)i * DS + d] = sg;
      double* row = p.rows + (int64_t)i * LS;   // (formed here: held across the sweep it costs <false> 12 VGPRs)
      row[d] = z;
      row[Dc + d] = kSqrtHalf / sg;
      // the mass of the normal truncated to the label's bounds (joint._std_bounds)
      const double za = (p.low[d] - z) / sg, zb = (p.high[d] - z) / sg;
      const bool flip = za > 0.0;
      const double a = flip ? -zb : za, b = flip ? -za : zb;
      const double fa = 0.5 * erfc(-a * kSqrtHalf), fb = 0.5 * erfc(-b * kSqrtHalf);
      s.sterm[d] = log(sg * 2.50662827463100050242 * (fb - fa));
    }
  }
  if constexpr (kMixed) {
    const int Dk = p.Dk, Dq = p.Dq;
    double* row = p.rows + (int64_t)i * LS;
    if (t < Dk) {                               // a discrete dimension: the category, no bandwidth
      const int v = src ? (int)src[Dc + t] : 0;
      int U = 2;
      if constexpr (kDimsByPointer<View>) {
        U = p.cat_upper[t];
      } else {
#pragma unroll
        for (int dd = 0; dd < kMaxK; ++dd)      // (static indices into the kernel arguments: no private copy)
          if (dd == t) U = p.cat_upper[dd];
      }
      row[2 * Dc + 1 + t] = (double)clampi(v, U - 1);
    }
    if (Dq > 0) {                               // thread t serves quantised dimension t % Dq, in float64
      const int S = (kThreads / Dq) * Dq, d = t % Dq;
      int V = 2, toff = 0;
      if constexpr (kDimsByPointer<View>) {
        V = p.qv[d];
        toff = p.qtoff[d];
      } else {
#pragma unroll
        for (int dd = 0; dd < kMaxQ; ++dd)
          if (dd == d) { V = p.qv[dd]; toff = p.qtoff[dd]; }
      }
      const int v = clampi(src ? (int)src[Dc + Dk + d] : 0, V - 1);
      const double c = p.centre[toff + v];
      double L = -INFINITY, U = INFINITY;
      if (t < S) {
        const int64_t total = (int64_t)p.K * Dq;
        for (int64_t e = t; e < total; e += S) {
          const double x = p.aqmu[e];
          if (x <= c) L = fmax(L, x);
          else if (x > c) U = fmin(U, x);
        }
        for (int q = t / Dq; q < i; q += S / Dq) {
          const double x = p.rows[(int64_t)q * LS + 2 * Dc + 1 + Dk + d];   // an earlier liar's centre
          if (x <= c) L = fmax(L, x);
          else if (x > c) U = fmin(U, x);
        }
      }
      s.dL[t] = L;
      s.dU[t] = U;
      __syncthreads();
      if (t < Dq) {
        for (int u = t + Dq; u < S; u += Dq) { L = fmax(L, s.dL[u]); U = fmin(U, s.dU[u]); }
        const double sg = neighbour_sigma(c, L, U, L != -INFINITY, U != INFINITY, p.psig[Dc + d], p.n, i);
        p.liar_sigma[(int64_t)i * DS + Dc + d] = sg;
        row[2 * Dc + 1 + Dk + d] = c;
        s.qc[d] = c;
        s.qs[d] = sg;
      }
      __syncthreads();
      for (int dd = 0; dd < Dq; ++dd) {         // T_i[dd][v] = log Q_i(v): the V + 1 tails once, then the differences
        const int V = p.qv[dd];
        const double* __restrict__ e = p.edges + p.qeoff[dd];
        const double cc = s.qc[dd], sc = kSqrtHalf / s.qs[dd];
        for (int u = t; u <= V; u += kThreads) {
          const double tt = (e[u] - cc) * sc;
          s.st[u] = tt;
          s.ss[u] = fabs(tt) > kTailMax ? 0.0 : 0.5 * erfc(fabs(tt));
        }
        __syncthreads();
        if (t < V) {
          const double diff = bin_mass(s.st[t], s.ss[t], s.st[t + 1], s.ss[t + 1]);
          const double mass = bin_mass(s.st[0], s.ss[0], s.st[V], s.ss[V]);
          p.tabs[(int64_t)i * p.totV + p.qtoff[dd] + t] = diff > 0.0 ? log(diff / mass) : -INFINITY;
        }
        __syncthreads();                        // st / ss are read: the next dimension may overwrite them
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    double c = 0.0;
    for (int u = 0; u < Dc; ++u) c += s.sterm[u];
    p.rows[(int64_t)i * LS + 2 * Dc] = -c;
  }
  __syncthreads();                              // the row is written: the next liar of this launch may scan it
}

// One pick: merges the n_chunks records at `chunk_rec` (one problem's, in chunk
// order) into *pick, copies the winner's row (row zo + idx of `cand`) to zcopy
// and adds it as liar i of the group `p`.
template <bool kMixed, class View>
__device__ __forceinline__ void pick_step(const View& p, const tpe_joint_pick* chunk_rec, int n_chunks,
                                          tpe_joint_pick* pick, const float* cand, int64_t zo, int i, float* zcopy,
                                          PickLds<kMixed>& s) {
  const int t = threadIdx.x;
  Pick best{0, 0};
  for (int c = t; c < n_chunks; c += kThreads) {
    const tpe_joint_pick r = chunk_rec[c];
    if (r.idx < 0) continue;
    const Pick x{score_key(r.l - r.g), r.idx};
    if (beats(x, best)) best = x;            // (chunk order = candidate index order)
  }
  const Pick w = block_best(best, s.slot);
  const bool none = w.key == 0;
  if (t == 0) *pick = none ? tpe_joint_pick{-1, 0.0, 0.0} : chunk_rec[w.idx / TPE_JOINT_CHUNK];
  add_liar<kMixed>(p, i, none ? nullptr : cand + (zo + w.idx) * p.D, zcopy, s);
}

// step: 0 adds the given liars; j >= 1 merges step j - 1's chunk records into
// picks[j - 1], copies its row and adds it as liar G + j - 1
template <bool kMixed>
__global__ __launch_bounds__(kThreads) void k_liar_pick(const Params<kMixed> p, int step) {
  __shared__ PickLds<kMixed> s;
  if (step == 0) {
    for (int i = 0; i < p.G; ++i) add_liar<kMixed>(p, i, p.given + (int64_t)i * p.D, nullptr, s);
    return;
  }
  const int j = step - 1;
  pick_step<kMixed>(p, p.chunk_rec, p.n_chunks, p.picks + j, p.cand, (int64_t)j * p.C, p.G + j,
                    p.pick_z + (int64_t)j * p.D, s);
}

// One chunk of one problem under the above mixture of the group `p` extended by
// its first J liars: candidate i is row zo + i of `cand`, its l and g are at
// o + i; the chunk's winner goes to *rec.  tile: LDS [kTile * row length].
template <bool kMixed, class View>
__device__ __forceinline__ void chunk_step(const View& p, int J, const float* cand, int64_t zo, int64_t o,
                                           tpe_joint_pick* rec, double log_w, double log_norm, double* tile,
                                           Pick* slot) {
  const int t = threadIdx.x, D = p.D, Dc = cont_dims<kMixed>(p), LS = row_len<kMixed>(p);
  const int first = blockIdx.x * TPE_JOINT_CHUNK;

  double m[kR], s[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) { m[r] = -1.0e300; s[r] = 0.0; }   // a finite floor: all terms -inf leave s = 0, no NaN
  for (int q0 = 0; q0 < J; q0 += kTile) {
    const int nq = min(kTile, J - q0), nq4 = (nq + kQ - 1) / kQ * kQ;
    __syncthreads();                         // the previous tile is read
    for (int e = t; e < nq4 * LS; e += kThreads) {
      const int q = e / LS, f = e % LS;      // a padded liar: h = 0, c = -inf, category -1 adds nothing
      double pad = f == 2 * Dc ? -INFINITY : 0.0;
      if constexpr (kMixed)
        if (f > 2 * Dc) pad = -1.0;
      tile[e] = q < nq ? p.rows[(int64_t)(q0 + q) * LS + f] : pad;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int i = first + r * kThreads + t;
      if (i >= p.C) continue;
      const float* __restrict__ zr = cand + (zo + i) * D;
      for (int qq = 0; qq < nq4; qq += kQ) {
        const double* __restrict__ row = tile + qq * LS;
        double acc[kQ], tt[kQ];
#pragma unroll
        for (int u = 0; u < kQ; ++u) acc[u] = 0.0;
        for (int d = 0; d < Dc; ++d) {
          const double zd = (double)zr[d];
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            const double x = (zd - row[u * LS + d]) * row[u * LS + Dc + d];
            acc[u] = fma(x, x, acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < kQ; ++u) tt[u] = row[u * LS + 2 * Dc] - acc[u];
        if constexpr (kMixed) {
          for (int d = 0; d < p.Dk; ++d) {   // one compare, one select, one add per (candidate, liar)
            const double vc = (double)zr[Dc + d];
            const double b = p.bonus[p.cat_off[d] + clampi((int)vc, p.cat_upper[d] - 1)];
#pragma unroll
            for (int u = 0; u < kQ; ++u) tt[u] += row[u * LS + 2 * Dc + 1 + d] == vc ? b : 0.0;
          }
          for (int d = 0; d < p.Dq; ++d) {   // one table read at the candidate's own lattice index
            const int v = p.qtoff[d] + clampi((int)zr[Dc + p.Dk + d], p.qv[d] - 1);
#pragma unroll
            for (int u = 0; u < kQ; ++u)     // (a padded liar reads the last real one's table: its c is -inf)
              tt[u] += p.tabs[(int64_t)min(q0 + qq + u, J - 1) * p.totV + v];
          }
        }
#pragma unroll
        for (int u = 0; u < kQ; ++u) {
          const double dl = tt[u] - m[r];
          const double e2 = exp(-fabs(dl));
          s[r] = dl > 0.0 ? fma(s[r], e2, 1.0) : s[r] + e2;
          m[r] = fmax(m[r], tt[u]);
        }
      }
    }
  }

  Pick best{0, 0};
  double lv[kR], gv[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = gv[r] = 0.0;
    if (i >= p.C) continue;
    lv[r] = p.l_out[o + i];
    double g = p.g_out[o + i];
    if (J > 0 && g == g) {                   // logaddexp(g, lse - log W) - log1p(J / W)
      double x;
      if constexpr (kMixed) {
        const float* __restrict__ zr = cand + (zo + i) * D;
        double miss = 0.0;                   // sum_d miss_d(v_d): the candidate's alone
        for (int d = 0; d < p.Dk; ++d)
          miss += p.miss[p.cat_off[d] + clampi((int)zr[Dc + d], p.cat_upper[d] - 1)];
        x = m[r] + log(s[r]) + miss - log_w;
      } else {
        x = m[r] + log(s[r]) - log_w;
      }
      const double hi = fmax(g, x), lo = fmin(g, x);
      g = (hi == -INFINITY ? hi : hi + log1p(exp(lo - hi))) - log_norm;
    }
    gv[r] = g;
    const uint64_t key = score_key(lv[r] - g);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  const Pick w = block_best(best, slot);
  if (w.key == 0) {
    if (t == 0) *rec = tpe_joint_pick{-1, 0.0, 0.0};
    return;
  }
  const int off = (int)(w.idx - first);
  if (t != off % kThreads) return;
#pragma unroll
  for (int r = 0; r < kR; ++r)
    if (r == off / kThreads) *rec = tpe_joint_pick{w.idx, lv[r], gv[r]};
}

// id j's candidates under the above mixture extended by J = G + j liars
template <bool kMixed>
__global__ __launch_bounds__(kThreads) void k_liar_chunk(const Params<kMixed> p, int j, double log_w,
                                                         double log_norm) {
  __shared__ double tile[kTile * kMaxRow];
  __shared__ Pick slot[kThreads / 64];
  const int64_t o = (int64_t)j * p.C;
  chunk_step<kMixed>(p, p.G + j, p.cand, o, o, p.chunk_rec + blockIdx.x, log_w, log_norm, tile, slot);
}

// ---- the segmented stage (tpe_joint_liar_seg): one greedy chain per group ----
constexpr int kSegRow = 2 * TPE_JOINT_MAX_DIMS + 1;   // doubles of a liar row of a segment

struct SegK {                   // the kernel argument of both segmented kernels
  int C, n_chunks;
  const tpe_joint_liar_seg_desc* segs;   // [n_segs], read on the device: not a kernel argument of n_segs descriptors
  const int32_t* order;             // rank -> group, chain length descending
  const int32_t* chain;             // slot -> problem
  const double* log_norm;           // [slot]
  const float* cand;
  const int64_t* cand_off;
  const double *l_out, *g_out;
  const float* pool;
  double* rows;                     // scratch
  tpe_joint_pick* chunk_rec;        // scratch [n_active * n_chunks], by rank
  tpe_joint_pick* picks;
  float* pick_z;
  double* liar_sigma;
};

__device__ __forceinline__ SegView seg_view(const SegK& k, const tpe_joint_liar_seg_desc& g) {
  SegView v;
  v.D = g.n_dims; v.C = k.C; v.K = g.k_above; v.n = g.n_trials;
  v.amu = k.pool + g.above_mu;
  v.l_out = k.l_out; v.g_out = k.g_out;
  v.rows = k.rows + g.row_off;
  v.liar_sigma = k.liar_sigma + g.sigma_off;
  v.psig = g.psig; v.low = g.low; v.high = g.high;
  return v;
}

// round r, group of rank blockIdx.y (chain length > r): one chunk of problem
// chain[first + r] under its group's r liars
__global__ __launch_bounds__(kThreads) void k_liar_seg_chunk(const SegK k, int r) {
  __shared__ double tile[kTile * kSegRow];
  __shared__ Pick slot[kThreads / 64];
  const int rank = blockIdx.y;
  const tpe_joint_liar_seg_desc& g = k.segs[k.order[rank]];
  const int sl = g.chain_first + r, prob = k.chain[sl];
  const SegView v = seg_view(k, g);
  chunk_step<false>(v, r, k.cand + k.cand_off[prob], 0, (int64_t)prob * k.C,
                    k.chunk_rec + (int64_t)rank * k.n_chunks + blockIdx.x, g.log_w, k.log_norm[sl], tile, slot);
}

// round r, group of rank blockIdx.x: the merge of that problem's records, the
// row copy, and the pick as liar r of its group
__global__ __launch_bounds__(kThreads) void k_liar_seg_pick(const SegK k, int r) {
  __shared__ PickLds<false> s;
  const int rank = blockIdx.x;
  const tpe_joint_liar_seg_desc& g = k.segs[k.order[rank]];
  const int prob = k.chain[g.chain_first + r];
  const SegView v = seg_view(k, g);
  pick_step<false>(v, k.chunk_rec + (int64_t)rank * k.n_chunks, k.n_chunks, k.picks + prob,
                   k.cand + k.cand_off[prob], 0, r, k.pick_z + (int64_t)prob * TPE_JOINT_MAX_DIMS, s);
}

// ---- the mixed segmented stage (tpe_joint_liar_mseg): groups of a tpe_joint_mseg_run ----
static_assert(2 * TPE_JOINT_MSEG_MAX_CONT + 1 + TPE_JOINT_MSEG_MAX_CAT + TPE_JOINT_MAX_QUANT <= kSegRow,
              "a mixed segment's liar row fits the continuous segments' tile");
static_assert(offsetof(tpe_joint_liar_mseg_desc, n_cat) == sizeof(tpe_joint_liar_seg_desc), "the shared prefix");
static_assert(offsetof(tpe_joint_liar_mseg_args, pool_f64) == sizeof(tpe_joint_liar_seg_args), "the shared prefix");

struct SegMK {                  // the kernel argument of both mixed segmented kernels: SegK's fields, then the f64 pools
  int C, n_chunks;
  const tpe_joint_liar_mseg_desc* segs;
  const int32_t* order;
  const int32_t* chain;
  const double* log_norm;
  const float* cand;
  const int64_t* cand_off;
  const double *l_out, *g_out;
  const float* pool;
  const double* pool64;             // the mseg stage's pool_f64: above_qmu, quant_edges
  const double* lpool;              // the liar pool: category tables, centres
  double* rows;                     // scratch
  double* tabs;                     // scratch, behind the rows
  tpe_joint_pick* chunk_rec;        // scratch [n_active * n_chunks], by rank
  tpe_joint_pick* picks;
  float* pick_z;
  double* liar_sigma;
};

__device__ __forceinline__ SegMView seg_mview(const SegMK& k, const tpe_joint_liar_mseg_desc& g) {
  SegMView v;
  v.Dc = g.n_dims; v.Dk = g.n_cat; v.Dq = g.n_quant;
  v.D = v.Dc + v.Dk + v.Dq; v.LS = 2 * v.Dc + 1 + v.Dk + v.Dq; v.totV = g.n_lattice;
  v.C = k.C; v.K = g.k_above; v.n = g.n_trials;
  v.amu = k.pool + g.above_mu;
  v.l_out = k.l_out; v.g_out = k.g_out;
  v.rows = k.rows + g.row_off;
  v.liar_sigma = k.liar_sigma + g.sigma_off;
  v.tabs = k.tabs + g.tab_off;
  v.psig = g.psig; v.low = g.low; v.high = g.high;
  v.aqmu = k.pool64 + g.above_qmu; v.edges = k.pool64 + g.quant_edges;
  v.miss = k.lpool + g.cat_miss; v.bonus = k.lpool + g.cat_bonus; v.centre = k.lpool + g.quant_centre;
  v.cat_upper = g.cat_upper; v.cat_off = g.cat_off;
  v.qv = g.quant_v; v.qeoff = g.quant_edge_off; v.qtoff = g.quant_tab_off;
  return v;
}

// k_liar_seg_chunk's round over the groups of a tpe_joint_mseg_run
__global__ __launch_bounds__(kThreads) void k_liar_mseg_chunk(const SegMK k, int r) {
  __shared__ double tile[kTile * kSegRow];
  __shared__ Pick slot[kThreads / 64];
  const int rank = blockIdx.y;
  const tpe_joint_liar_mseg_desc& g = k.segs[k.order[rank]];
  const int sl = g.chain_first + r, prob = k.chain[sl];
  const SegMView v = seg_mview(k, g);
  chunk_step<true>(v, r, k.cand + k.cand_off[prob], 0, (int64_t)prob * k.C,
                   k.chunk_rec + (int64_t)rank * k.n_chunks + blockIdx.x, g.log_w, k.log_norm[sl], tile, slot);
}

// k_liar_seg_pick's round over the groups of a tpe_joint_mseg_run
__global__ __launch_bounds__(kThreads) void k_liar_mseg_pick(const SegMK k, int r) {
  __shared__ PickLds<true> s;
  const int rank = blockIdx.x;
  const tpe_joint_liar_mseg_desc& g = k.segs[k.order[rank]];
  const int prob = k.chain[g.chain_first + r];
  const SegMView v = seg_mview(k, g);
  pick_step<true>(v, k.chunk_rec + (int64_t)rank * k.n_chunks, k.n_chunks, k.picks + prob,
                  k.cand + k.cand_off[prob], 0, r, k.pick_z + (int64_t)prob * TPE_JOINT_MAX_DIMS, s);
}

struct Sizes {
  uint64_t rows_bytes, tabs_bytes, bytes;
};

// whether the counts of one group of a tpe_joint_liar_mseg are inside the limits
bool mseg_counts_ok(const tpe_joint_liar_mseg_desc& g) {
  if (g.n_dims < 0 || g.n_cat < 0 || g.n_quant < 0 || g.n_lattice < 0 || g.chain_len < 0) return false;
  if (g.n_cat == 0 && g.n_quant == 0) return g.n_dims >= 1 && g.n_dims <= TPE_JOINT_MAX_DIMS && g.n_lattice == 0;
  return g.n_dims <= TPE_JOINT_MSEG_MAX_CONT && g.n_cat <= TPE_JOINT_MSEG_MAX_CAT && g.n_quant <= kMaxQ &&
         g.n_lattice <= TPE_JOINT_MAX_LATTICE_TOTAL && (g.n_quant == 0) == (g.n_lattice == 0);
}

// the scratch of one tpe_joint_liar_mseg from the host descriptors, or false
// where a count is out of range; n_active: the groups with a problem
bool liar_mseg_scratch(const tpe_joint_liar_mseg_desc* segs, int32_t n_segs, int32_t n_cand, Sizes* z, int* n_active) {
  if (!segs || n_segs < 1 || n_cand < 1) return false;
  uint64_t row_doubles = 0, tab_doubles = 0;
  int active = 0;
  for (int s = 0; s < n_segs; ++s) {
    const tpe_joint_liar_mseg_desc& g = segs[s];
    if (!mseg_counts_ok(g)) return false;
    row_doubles += (uint64_t)g.chain_len * (2 * (uint64_t)g.n_dims + 1 + (uint64_t)g.n_cat + (uint64_t)g.n_quant);
    tab_doubles += (uint64_t)g.chain_len * (uint64_t)g.n_lattice;
    active += g.chain_len > 0;
  }
  const uint64_t chunks = ((uint64_t)n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK;
  z->rows_bytes = row_doubles * sizeof(double);
  z->tabs_bytes = tab_doubles * sizeof(double);
  z->bytes = z->rows_bytes + z->tabs_bytes + (uint64_t)active * chunks * sizeof(tpe_joint_pick);
  if (n_active) *n_active = active;
  return true;
}

// the scratch of one tpe_joint_liar_seg from the host descriptors, or false
// where a count is out of range; n_active: the groups with a problem
bool liar_seg_scratch(const tpe_joint_liar_seg_desc* segs, int32_t n_segs, int32_t n_cand, Sizes* z, int* n_active) {
  if (!segs || n_segs < 1 || n_cand < 1) return false;
  uint64_t row_doubles = 0;
  int active = 0;
  for (int s = 0; s < n_segs; ++s) {
    if (segs[s].n_dims < 1 || segs[s].n_dims > TPE_JOINT_MAX_DIMS || segs[s].chain_len < 0) return false;
    row_doubles += (uint64_t)segs[s].chain_len * (2 * (uint64_t)segs[s].n_dims + 1);
    active += segs[s].chain_len > 0;
  }
  const uint64_t chunks = ((uint64_t)n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK;
  z->rows_bytes = row_doubles * sizeof(double);
  z->tabs_bytes = 0;
  z->bytes = z->rows_bytes + (uint64_t)active * chunks * sizeof(tpe_joint_pick);
  if (n_active) *n_active = active;
  return true;
}

// the scratch of one call, or false where the sizes are out of range
bool liar_scratch(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, int32_t n_quant, int32_t n_lattice,
                  int32_t n_given, Sizes* z) {
  if (n_ids < 1 || n_cand < 1 || n_dims < 0 || n_cat < 0 || n_quant < 0 || n_given < 0 || n_lattice < 0) return false;
  if (n_cat > kMaxK || n_quant > kMaxQ || n_lattice > TPE_JOINT_MAX_LATTICE_TOTAL) return false;
  const int D = n_dims + n_cat + n_quant;
  if (D < 1 || D > kMaxD || (n_quant == 0) != (n_lattice == 0)) return false;
  const uint64_t chunks = ((uint64_t)n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK;
  const uint64_t liars = (uint64_t)n_ids + (uint64_t)n_given;
  z->rows_bytes = liars * (2 * (uint64_t)n_dims + 1 + (uint64_t)n_cat + (uint64_t)n_quant) * sizeof(double);
  z->tabs_bytes = liars * (uint64_t)n_lattice * sizeof(double);
  z->bytes = z->rows_bytes + z->tabs_bytes + chunks * sizeof(tpe_joint_pick);
  return true;
}

// TPE_E_ARG with the message "<who>: <what>"
int bad(const char* who, const char* what) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return tpe_internal_fail(TPE_E_ARG, msg);
}

// The checks of the prefix both args structs share, in the entry `who`'s words;
// x: the whole struct of tpe_joint_liar_mixed (nullptr: tpe_joint_liar, n_dims
// alone is the row).
int check_args(const char* who, const tpe_joint_liar_args* a, const tpe_joint_liar_mixed_args* x,
               const tpe_joint_pick* picks, const float* pick_z, const double* liar_sigma) {
  const int Dc = a->n_dims, Dk = x ? x->n_cat : 0, Dq = x ? x->n_quant : 0;
  if (!x) {
    if (Dc < 1 || Dc > kMaxD) return bad(who, "n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
  } else {
    if (Dc < 0 || Dk < 0 || Dq < 0) return bad(who, "n_dims / n_cat / n_quant < 0");
    if (Dk > kMaxK || Dq > kMaxQ)
      return bad(who, "n_cat above TPE_JOINT_MAX_DIMS or n_quant above TPE_JOINT_MAX_QUANT");
    if (Dc + Dk + Dq < 1 || Dc + Dk + Dq > kMaxD) return bad(who, "row width outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
    if (Dq > 0 && (Dc > 8 || Dk > 4)) return bad(who, "beside a quantised label n_dims <= 8 and n_cat <= 4");
  }
  if (a->n_ids < 1 || a->n_cand < 1 || a->k_above < 1) return bad(who, "n_ids / n_cand / k_above < 1");
  if (a->n_given < 0 || a->n_trials < 0) return bad(who, "n_given / n_trials < 0");
  if (!(a->w_sum > 0.0) || !(a->w_sum < INFINITY)) return bad(who, "w_sum must be positive and finite");
  if (!a->cand || !a->l_out || !a->g_out || (Dc > 0 && !a->above_mu))
    return bad(who, "null cand / l_out / g_out / above_mu");
  if (a->n_given > 0 && !a->given) return bad(who, "n_given > 0 without given");
  if (!picks || !pick_z || !liar_sigma) return bad(who, "null outputs");
  for (int d = 0; d < Dc + Dq; ++d)             // the continuous dimensions, then the quantised ones
    if (!(a->psig[d] > 0.0)) return bad(who, "a prior sigma that is not positive");
  return TPE_OK;
}

// The shared fields of `k` from the checked prefix (the instantiation's own are
// the caller's), then the launches: the given liars, then a chunk and a pick
// launch per id.  D: the row width; Dq: the quantised dimensions.
template <bool kMixed>
int run(Params<kMixed>& k, const tpe_joint_liar_args* a, int D, int Dq, tpe_joint_pick* picks, float* pick_z,
        double* liar_sigma, void* scratch, const Sizes& z, void* stream) {
  k.D = D; k.C = a->n_cand; k.K = a->k_above; k.G = a->n_given; k.n = a->n_trials;
  k.n_chunks = (int)(((int64_t)a->n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK);
  k.cand = a->cand; k.l_out = a->l_out; k.g_out = a->g_out; k.amu = a->above_mu; k.given = a->given;
  k.rows = (double*)scratch;
  k.chunk_rec = (tpe_joint_pick*)((char*)scratch + z.rows_bytes + z.tabs_bytes);
  k.picks = picks; k.pick_z = pick_z; k.liar_sigma = liar_sigma;
  for (int d = 0; d < kMaxD; ++d) {
    const bool cont = d < a->n_dims, in = cont || d < a->n_dims + Dq;
    k.psig[d] = in ? a->psig[d] : 1.0;
    k.low[d] = cont ? a->low[d] : -INFINITY;
    k.high[d] = cont ? a->high[d] : INFINITY;
  }
  const hipStream_t s = (hipStream_t)stream;
  const double log_w = log(a->w_sum);
  if (k.G > 0) hipLaunchKernelGGL(k_liar_pick<kMixed>, dim3(1), dim3(kThreads), 0, s, k, 0);
  for (int j = 0; j < a->n_ids; ++j) {
    hipLaunchKernelGGL(k_liar_chunk<kMixed>, dim3((unsigned)k.n_chunks), dim3(kThreads), 0, s, k, j, log_w,
                       log1p((double)(k.G + j) / a->w_sum));
    hipLaunchKernelGGL(k_liar_pick<kMixed>, dim3(1), dim3(kThreads), 0, s, k, j + 1);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

}  // namespace

extern "C" {

int tpe_joint_liar_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_given, uint64_t* bytes) {
  Sizes z;
  if (!bytes || n_dims < 1 || !liar_scratch(n_ids, n_cand, n_dims, 0, 0, 0, n_given, &z))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar_scratch_bytes: bad arguments");
  *bytes = z.bytes;
  return TPE_OK;
}

int tpe_joint_liar_mixed_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, int32_t n_quant,
                                       int32_t n_lattice, int32_t n_given, uint64_t* bytes) {
  Sizes z;
  if (!bytes || !liar_scratch(n_ids, n_cand, n_dims, n_cat, n_quant, n_lattice, n_given, &z))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar_mixed_scratch_bytes: bad arguments");
  *bytes = z.bytes;
  return TPE_OK;
}

int tpe_joint_liar(const tpe_joint_liar_args* a, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                   void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* who = "tpe_joint_liar";
  tpe_internal_epoch_bump();
  if (!a) return bad(who, "null args");
  if (const int rc = check_args(who, a, nullptr, picks, pick_z, liar_sigma)) return rc;
  Sizes z;
  liar_scratch(a->n_ids, a->n_cand, a->n_dims, 0, 0, 0, a->n_given, &z);
  if (!scratch || scratch_bytes < z.bytes) return bad(who, "scratch too small");
  LiarK k;
  return run<false>(k, a, a->n_dims, 0, picks, pick_z, liar_sigma, scratch, z, stream);
}

int tpe_joint_liar_mixed(const tpe_joint_liar_mixed_args* a, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                         void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* who = "tpe_joint_liar_mixed";
  const tpe_joint_liar_args* pre = (const tpe_joint_liar_args*)a;   // (the shared prefix)
  if (!a) {
    tpe_internal_epoch_bump();
    return bad(who, "null args");
  }
  // a continuous group: tpe_joint_liar over the shared prefix, its checks and its bytes
  if (a->n_cat == 0 && a->n_quant == 0)
    return tpe_joint_liar(pre, picks, pick_z, liar_sigma, scratch, scratch_bytes, stream);
  tpe_internal_epoch_bump();
  if (const int rc = check_args(who, pre, a, picks, pick_z, liar_sigma)) return rc;
  const int Dc = a->n_dims, Dk = a->n_cat, Dq = a->n_quant;
  int64_t cat_total = 0, lat_total = 0;
  if (Dk > 0) {
    if (!a->cat_miss || !a->cat_bonus) return bad(who, "null category table");
    for (int d = 0; d < Dk; ++d) {
      if (a->cat_upper[d] < 2 || a->cat_upper[d] > TPE_JOINT_MAX_CATS)
        return bad(who, "a U_d outside [2, TPE_JOINT_MAX_CATS]");
      cat_total += a->cat_upper[d];
    }
    if (cat_total > TPE_JOINT_MAX_CAT_TOTAL) return bad(who, "more than TPE_JOINT_MAX_CAT_TOTAL categories");
    for (int d = 0; d < Dk; ++d)
      if (a->cat_off[d] < 0 || a->cat_off[d] > cat_total - a->cat_upper[d])
        return bad(who, "a cat_off that leaves the table");
  }
  if (Dq > 0) {
    if (!a->quant_edges || !a->quant_centre || !a->above_qmu)
      return bad(who, "null quant_edges / quant_centre / above_qmu");
    for (int d = 0; d < Dq; ++d) {
      if (a->quant_v[d] < 2 || a->quant_v[d] > kMaxV) return bad(who, "a V_d outside [2, TPE_JOINT_MAX_LATTICE]");
      lat_total += a->quant_v[d];
    }
    if (lat_total > TPE_JOINT_MAX_LATTICE_TOTAL)
      return bad(who, "more than TPE_JOINT_MAX_LATTICE_TOTAL lattice values");
    for (int d = 0; d < Dq; ++d)
      if (a->quant_edge_off[d] < 0 || a->quant_edge_off[d] > a->n_edges - a->quant_v[d] - 1)
        return bad(who, "a quant_edge_off that leaves quant_edges");
  }
  Sizes z;
  if (!liar_scratch(a->n_ids, a->n_cand, Dc, Dk, Dq, (int32_t)lat_total, a->n_given, &z))
    return bad(who, "sizes out of range");
  if (!scratch || scratch_bytes < z.bytes) return bad(who, "scratch too small");

  LiarMK k;
  k.Dc = Dc; k.Dk = Dk; k.Dq = Dq; k.LS = 2 * Dc + 1 + Dk + Dq; k.totV = (int)lat_total;
  k.aqmu = a->above_qmu; k.miss = a->cat_miss; k.bonus = a->cat_bonus; k.edges = a->quant_edges;
  k.centre = a->quant_centre;
  k.tabs = (double*)((char*)scratch + z.rows_bytes);
  for (int d = 0; d < kMaxK; ++d) {
    k.cat_upper[d] = d < Dk ? a->cat_upper[d] : 2;
    k.cat_off[d] = d < Dk ? a->cat_off[d] : 0;
  }
  int toff = 0;
  for (int d = 0; d < kMaxQ; ++d) {
    k.qv[d] = d < Dq ? a->quant_v[d] : 2;
    k.qeoff[d] = d < Dq ? a->quant_edge_off[d] : 0;
    k.qtoff[d] = d < Dq ? toff : 0;
    if (d < Dq) toff += a->quant_v[d];
  }
  return run<true>(k, pre, Dc + Dk + Dq, Dq, picks, pick_z, liar_sigma, scratch, z, stream);
}

int tpe_joint_liar_seg_scratch_bytes(const tpe_joint_liar_seg_desc* host_segs, int32_t n_segs, int32_t n_cand,
                                     uint64_t* bytes) {
  Sizes z;
  if (!bytes || !liar_seg_scratch(host_segs, n_segs, n_cand, &z, nullptr))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar_seg_scratch_bytes: bad arguments");
  *bytes = z.bytes;
  return TPE_OK;
}

int tpe_joint_liar_seg(const tpe_joint_liar_seg_args* a, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                       void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* who = "tpe_joint_liar_seg";
  tpe_internal_epoch_bump();
  if (!a) return bad(who, "null args");
  if (a->n_segs < 1 || a->n_probs < 1 || a->n_cand < 1) return bad(who, "n_segs / n_probs / n_cand < 1");
  if (!a->segs || !a->host_segs || !a->order || !a->host_order || !a->chain || !a->host_chain || !a->log_norm ||
      !a->host_log_norm || !a->host_prob_seg)
    return bad(who, "null segs / order / chain / log_norm / host_prob_seg");
  if (!a->cand || !a->cand_off || !a->l_out || !a->g_out || !a->pool_f32)
    return bad(who, "null cand / cand_off / l_out / g_out / pool_f32");
  if (!picks || !pick_z || !liar_sigma) return bad(who, "null outputs");
  const int S = a->n_segs, P = a->n_probs;
  const tpe_joint_liar_seg_desc* hs = a->host_segs;
  for (int s = 0; s < S; ++s) {
    const tpe_joint_liar_seg_desc& g = hs[s];
    if (g.n_dims < 1 || g.n_dims > TPE_JOINT_MAX_DIMS) return bad(who, "n_dims outside [1, TPE_JOINT_MAX_DIMS]");
    if (g.k_above < 1) return bad(who, "k_above < 1");
    if (g.n_trials < 0) return bad(who, "n_trials < 0");
    if (!(g.w_sum > 0.0) || !(g.w_sum < INFINITY)) return bad(who, "w_sum must be positive and finite");
    for (int d = 0; d < g.n_dims; ++d)
      if (!(g.psig[d] > 0.0)) return bad(who, "a prior sigma that is not positive");
    if (g.above_mu < 0 || g.above_mu > a->pool_f32_len - (int64_t)g.k_above * g.n_dims)
      return bad(who, "an above_mu range that leaves pool_f32");
    // tpe_joint_liar takes log W from the host's log: the device's differs in the last bits
    if (g.log_w != log(g.w_sum)) return bad(who, "a log_w that is not the host's log(w_sum)");
  }
  // the chains: host_prob_seg alone fixes every count, the order, the slots and the offsets
  const char* part = "a chain table that is not the partition of the problems host_prob_seg gives";
  for (int p = 0; p < P; ++p)
    if (a->host_prob_seg[p] < 0 || a->host_prob_seg[p] >= S) return bad(who, "a host_prob_seg entry outside [0, n_segs)");
  int64_t slot = 0, row = 0, sig = 0;
  int n_active = 0, longest = 0;
  for (int rank = 0; rank < S; ++rank) {
    const int s = a->host_order[rank];
    if (s < 0 || s >= S) return bad(who, part);
    const tpe_joint_liar_seg_desc& g = hs[s];
    if (g.chain_len < 0 || g.chain_len > P - slot || g.chain_first != slot) return bad(who, part);
    if (rank > 0) {                               // chain length descending, ties by group index: a permutation
      const int q = a->host_order[rank - 1];
      if (hs[q].chain_len < g.chain_len || (hs[q].chain_len == g.chain_len && q >= s)) return bad(who, part);
    }
    if (g.row_off != row || g.sigma_off != sig) return bad(who, "a row_off / sigma_off that is not the running sum");
    slot += g.chain_len;
    row += (int64_t)g.chain_len * (2 * g.n_dims + 1);
    sig += (int64_t)g.chain_len * g.n_dims;
    n_active += g.chain_len > 0;
    if (g.chain_len > longest) longest = g.chain_len;
  }
  if (slot != P) return bad(who, part);
  {                                               // slot first_s + j holds the (j + 1)-th problem of group s
    std::vector<int> next((size_t)S, 0);          // (the lengths sum to P, so full chains hit every slot once)
    for (int p = 0; p < P; ++p) {
      const tpe_joint_liar_seg_desc& g = hs[a->host_prob_seg[p]];
      const int j = next[(size_t)a->host_prob_seg[p]]++;
      if (j >= g.chain_len || a->host_chain[g.chain_first + j] != p) return bad(who, part);
      if (a->host_log_norm[g.chain_first + j] != log1p((double)j / g.w_sum))
        return bad(who, "a log_norm that is not the host's log1p(j / w_sum)");
    }
    for (int s = 0; s < S; ++s)
      if (next[(size_t)s] != hs[s].chain_len) return bad(who, part);
  }
  Sizes z;
  if (n_active > 65535 || !liar_seg_scratch(hs, S, a->n_cand, &z, nullptr)) return bad(who, "sizes out of range");
  if (!scratch || scratch_bytes < z.bytes) return bad(who, "scratch too small");

  SegK k;
  k.C = a->n_cand;
  k.n_chunks = (int)(((int64_t)a->n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK);
  k.segs = a->segs; k.order = a->order; k.chain = a->chain; k.log_norm = a->log_norm;
  k.cand = a->cand; k.cand_off = a->cand_off; k.l_out = a->l_out; k.g_out = a->g_out; k.pool = a->pool_f32;
  k.rows = (double*)scratch;
  k.chunk_rec = (tpe_joint_pick*)((char*)scratch + z.rows_bytes);
  k.picks = picks; k.pick_z = pick_z; k.liar_sigma = liar_sigma;
  const hipStream_t st = (hipStream_t)stream;
  int active = n_active;                          // the groups of chain length > r: a prefix of the order
  for (int r = 0; r < longest; ++r) {
    while (hs[a->host_order[active - 1]].chain_len <= r) --active;
    hipLaunchKernelGGL(k_liar_seg_chunk, dim3((unsigned)k.n_chunks, (unsigned)active), dim3(kThreads), 0, st, k, r);
    hipLaunchKernelGGL(k_liar_seg_pick, dim3((unsigned)active), dim3(kThreads), 0, st, k, r);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

int tpe_joint_liar_mseg_scratch_bytes(const tpe_joint_liar_mseg_desc* host_segs, int32_t n_segs, int32_t n_cand,
                                      uint64_t* bytes) {
  Sizes z;
  if (!bytes || !liar_mseg_scratch(host_segs, n_segs, n_cand, &z, nullptr))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar_mseg_scratch_bytes: bad arguments");
  *bytes = z.bytes;
  return TPE_OK;
}

int tpe_joint_liar_mseg(const tpe_joint_liar_mseg_args* a, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                        void* scratch, uint64_t scratch_bytes, void* stream) {
  const char* who = "tpe_joint_liar_mseg";
  tpe_internal_epoch_bump();
  if (!a) return bad(who, "null args");
  if (a->n_segs < 1 || a->n_probs < 1 || a->n_cand < 1) return bad(who, "n_segs / n_probs / n_cand < 1");
  if (!a->segs || !a->host_segs || !a->order || !a->host_order || !a->chain || !a->host_chain || !a->log_norm ||
      !a->host_log_norm || !a->host_prob_seg)
    return bad(who, "null segs / order / chain / log_norm / host_prob_seg");
  if (!a->cand || !a->cand_off || !a->l_out || !a->g_out || !a->pool_f32)
    return bad(who, "null cand / cand_off / l_out / g_out / pool_f32");
  if (!picks || !pick_z || !liar_sigma) return bad(who, "null outputs");
  const int S = a->n_segs, P = a->n_probs;
  const tpe_joint_liar_mseg_desc* hs = a->host_segs;
  const int64_t n64 = a->pool_f64 ? a->pool_f64_len : 0, nl = a->liar_pool ? a->liar_pool_len : 0;
  for (int s = 0; s < S; ++s) {
    const tpe_joint_liar_mseg_desc& g = hs[s];
    const int Dc = g.n_dims, Dk = g.n_cat, Dq = g.n_quant;
    if (Dc < 0 || Dk < 0 || Dq < 0) return bad(who, "n_dims / n_cat / n_quant < 0");
    if (Dk == 0 && Dq == 0) {
      if (Dc < 1 || Dc > TPE_JOINT_MAX_DIMS) return bad(who, "n_dims outside [1, TPE_JOINT_MAX_DIMS]");
    } else if (Dc > TPE_JOINT_MSEG_MAX_CONT || Dk > TPE_JOINT_MSEG_MAX_CAT || Dq > kMaxQ) {
      return bad(who, "n_dims above TPE_JOINT_MSEG_MAX_CONT, n_cat above TPE_JOINT_MSEG_MAX_CAT or n_quant above "
                      "TPE_JOINT_MAX_QUANT");
    }
    if (g.k_above < 1) return bad(who, "k_above < 1");
    if (g.n_trials < 0) return bad(who, "n_trials < 0");
    if (!(g.w_sum > 0.0) || !(g.w_sum < INFINITY)) return bad(who, "w_sum must be positive and finite");
    for (int d = 0; d < Dc + Dq; ++d)             // the continuous dimensions, then the quantised ones
      if (!(g.psig[d] > 0.0)) return bad(who, "a prior sigma that is not positive");
    if (g.above_mu < 0 || g.above_mu > a->pool_f32_len - (int64_t)g.k_above * Dc)
      return bad(who, "an above_mu range that leaves pool_f32");
    if (g.log_w != log(g.w_sum)) return bad(who, "a log_w that is not the host's log(w_sum)");
    int64_t cat_total = 0, lat_total = 0;
    for (int d = 0; d < Dk; ++d) {
      if (g.cat_upper[d] < 2 || g.cat_upper[d] > TPE_JOINT_MAX_CATS)
        return bad(who, "a U_d outside [2, TPE_JOINT_MAX_CATS]");
      cat_total += g.cat_upper[d];
    }
    static_assert(TPE_JOINT_MSEG_MAX_CAT * TPE_JOINT_MAX_CATS <= TPE_JOINT_MAX_CAT_TOTAL, "no total to check");
    for (int d = 0; d < Dk; ++d)
      if (g.cat_off[d] < 0 || g.cat_off[d] > cat_total - g.cat_upper[d])
        return bad(who, "a cat_off that leaves the table");
    if (Dk > 0 && (g.cat_miss < 0 || g.cat_miss > nl - cat_total || g.cat_bonus < 0 || g.cat_bonus > nl - cat_total))
      return bad(who, "a cat_miss / cat_bonus range that leaves liar_pool");
    for (int d = 0; d < Dq; ++d) {
      if (g.quant_v[d] < 2 || g.quant_v[d] > kMaxV) return bad(who, "a V_d outside [2, TPE_JOINT_MAX_LATTICE]");
      if (g.quant_tab_off[d] != lat_total) return bad(who, "a quant_tab_off that is not the running sum of V_d");
      lat_total += g.quant_v[d];
    }
    if (lat_total > TPE_JOINT_MAX_LATTICE_TOTAL)
      return bad(who, "more than TPE_JOINT_MAX_LATTICE_TOTAL lattice values");
    if (g.n_lattice != lat_total) return bad(who, "an n_lattice that is not the sum of V_d");
    if (Dq > 0) {
      for (int d = 0; d < Dq; ++d)
        if (g.quant_edge_off[d] < 0 || g.quant_edge_off[d] > g.n_edges - g.quant_v[d] - 1)
          return bad(who, "a quant_edge_off that leaves quant_edges");
      if (g.quant_edges < 0 || g.quant_edges > n64 - g.n_edges || g.above_qmu < 0 ||
          g.above_qmu > n64 - (int64_t)g.k_above * Dq)
        return bad(who, "a quant_edges / above_qmu range that leaves pool_f64");
      if (g.quant_centre < 0 || g.quant_centre > nl - lat_total)
        return bad(who, "a quant_centre range that leaves liar_pool");
    }
  }
  // the chains: host_prob_seg alone fixes every count, the order, the slots and the offsets
  const char* part = "a chain table that is not the partition of the problems host_prob_seg gives";
  for (int p = 0; p < P; ++p)
    if (a->host_prob_seg[p] < 0 || a->host_prob_seg[p] >= S) return bad(who, "a host_prob_seg entry outside [0, n_segs)");
  int64_t slot = 0, row = 0, tab = 0, sig = 0;
  int n_active = 0, longest = 0;
  for (int rank = 0; rank < S; ++rank) {
    const int s = a->host_order[rank];
    if (s < 0 || s >= S) return bad(who, part);
    const tpe_joint_liar_mseg_desc& g = hs[s];
    if (g.chain_len < 0 || g.chain_len > P - slot || g.chain_first != slot) return bad(who, part);
    if (rank > 0) {                               // chain length descending, ties by group index: a permutation
      const int q = a->host_order[rank - 1];
      if (hs[q].chain_len < g.chain_len || (hs[q].chain_len == g.chain_len && q >= s)) return bad(who, part);
    }
    if (g.row_off != row || g.tab_off != tab || g.sigma_off != sig)
      return bad(who, "a row_off / tab_off / sigma_off that is not the running sum");
    slot += g.chain_len;
    row += (int64_t)g.chain_len * (2 * g.n_dims + 1 + g.n_cat + g.n_quant);
    tab += (int64_t)g.chain_len * g.n_lattice;
    sig += (int64_t)g.chain_len * (g.n_dims + g.n_quant);
    n_active += g.chain_len > 0;
    if (g.chain_len > longest) longest = g.chain_len;
  }
  if (slot != P) return bad(who, part);
  {                                               // slot first_s + j holds the (j + 1)-th problem of group s
    std::vector<int> next((size_t)S, 0);
    for (int p = 0; p < P; ++p) {
      const tpe_joint_liar_mseg_desc& g = hs[a->host_prob_seg[p]];
      const int j = next[(size_t)a->host_prob_seg[p]]++;
      if (j >= g.chain_len || a->host_chain[g.chain_first + j] != p) return bad(who, part);
      if (a->host_log_norm[g.chain_first + j] != log1p((double)j / g.w_sum))
        return bad(who, "a log_norm that is not the host's log1p(j / w_sum)");
    }
    for (int s = 0; s < S; ++s)
      if (next[(size_t)s] != hs[s].chain_len) return bad(who, part);
  }
  Sizes z;
  if (n_active > 65535 || !liar_mseg_scratch(hs, S, a->n_cand, &z, nullptr)) return bad(who, "sizes out of range");
  if (!scratch || scratch_bytes < z.bytes) return bad(who, "scratch too small");

  SegMK k;
  k.C = a->n_cand;
  k.n_chunks = (int)(((int64_t)a->n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK);
  k.segs = a->segs; k.order = a->order; k.chain = a->chain; k.log_norm = a->log_norm;
  k.cand = a->cand; k.cand_off = a->cand_off; k.l_out = a->l_out; k.g_out = a->g_out; k.pool = a->pool_f32;
  k.pool64 = a->pool_f64; k.lpool = a->liar_pool;
  k.rows = (double*)scratch;
  k.tabs = (double*)((char*)scratch + z.rows_bytes);
  k.chunk_rec = (tpe_joint_pick*)((char*)scratch + z.rows_bytes + z.tabs_bytes);
  k.picks = picks; k.pick_z = pick_z; k.liar_sigma = liar_sigma;
  const hipStream_t st = (hipStream_t)stream;
  int active = n_active;                          // the groups of chain length > r: a prefix of the order
  for (int r = 0; r < longest; ++r) {
    while (hs[a->host_order[active - 1]].chain_len <= r) --active;
    hipLaunchKernelGGL(k_liar_mseg_chunk, dim3((unsigned)k.n_chunks, (unsigned)active), dim3(kThreads), 0, st, k, r);
    hipLaunchKernelGGL(k_liar_mseg_pick, dim3((unsigned)active), dim3(kThreads), 0, st, k, r);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

}  // extern "C"
