// MI355X (gfx950) batch-aware joint suggests: the greedy "liar" stage that runs
// after a continuous joint stage (include/tpe_hip.h, "Batch-aware joint
// suggests").  Id j picks under the above mixture extended by the vectors the
// ids before it picked (and the given ones), each a component of un-normalised
// weight 1.  Nothing on the default suggest path runs through this file.
//
// k_liar_pick   one 256-thread workgroup per step: merges the previous step's
//               chunk records in index order, copies the winner's row, then
//               fits the new liar's bandwidths (the adaptive-Parzen neighbour
//               rule over the K_above f32 mu values and the earlier liars of
//               each dimension, float64 on f32 values: exact) and writes its
//               float64 row {mu[D], sqrt(1/2) / sigma[D], c}.  Step 0 adds the
//               given liars one after the other.
// k_liar_chunk  one 256-thread workgroup per chunk of TPE_JOINT_CHUNK
//               consecutive candidates of ONE id: the liar rows stream through
//               LDS in tiles of TPE_JOINT_LIAR_TILE, a lane accumulates
//               sum_d ((z_d - mu_d) / (sigma_d sqrt 2))^2 of four liars at a
//               time in float64 (subtract, then scale), keeps a running
//               maximum, finishes against the stored g and writes the chunk
//               winner through the butterfly on (score key, index).
// The steps are ordered by the stream alone: no workgroup waits on another, no
// atomics, every reduction has a fixed shape, so the output bytes are a
// function of the input bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tpe_hip.h"

extern "C" int tpe_internal_fail(int code, const char* what);   // tpe_kernels.hip (hidden)
extern "C" void tpe_internal_epoch_bump(void);                    // tpe_kernels.hip (hidden): the device epoch

namespace {

constexpr int kThreads = 256;                       // 4 waves of 64
constexpr int kR = TPE_JOINT_CHUNK / kThreads;      // candidates per lane
constexpr int kTile = TPE_JOINT_LIAR_TILE;          // liars per LDS tile
constexpr int kQ = 4;                               // liars a lane accumulates at once
constexpr int kMaxD = TPE_JOINT_WIDE_MAX_DIMS;
constexpr int kMaxRow = 2 * kMaxD + 1;              // doubles of a liar row: mu[D], h[D], c
static_assert(kR * kThreads == TPE_JOINT_CHUNK && kTile % kQ == 0, "chunk and tile shapes");
static_assert(sizeof(tpe_joint_pick) == 24, "layout");

struct LiarK {
  int D, C, n_chunks, K, G, n;
  const float* cand;
  const double *l_out, *g_out;
  const float* amu;
  const float* given;
  double* rows;                 // scratch [(G + n_ids) * (2 D + 1)]
  tpe_joint_pick* chunk_rec;    // scratch [n_chunks]: the records of the step that ran last
  tpe_joint_pick* picks;
  float* pick_z;
  double* liar_sigma;
  double psig[kMaxD], low[kMaxD], high[kMaxD];
};

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

// Liar `i` (ordinal among all liars) at the f32 vector zsrc[D]: bandwidths,
// liar_sigma and the row.  S = the largest multiple of D up to 256 threads scan:
// thread t serves dimension t % D and the points t / D, t / D + S / D, ..., so a
// sweep reads S consecutive floats.  zcopy: where the vector is also copied to.
__device__ __forceinline__ void add_liar(const LiarK& p, int i, const float* __restrict__ zsrc,
                                         float* __restrict__ zcopy, float* sL, float* sU, double* sterm) {
  const int t = threadIdx.x, D = p.D, S = (kThreads / D) * D, LS = 2 * D + 1;
  const int d = t % D;
  const float zd = zsrc ? zsrc[d] : 0.f;
  float L = -INFINITY, U = INFINITY;          // -inf / +inf: no neighbour on that side
  if (t < S) {
    const int64_t total = (int64_t)p.K * D;
    for (int64_t e = t; e < total; e += S) {
      const float x = p.amu[e];
      if (x <= zd) L = fmaxf(L, x);
      else if (x > zd) U = fminf(U, x);
    }
    for (int q = t / D; q < i; q += S / D) {
      const float x = (float)p.rows[(int64_t)q * LS + d];   // an earlier liar's f32 coordinate
      if (x <= zd) L = fmaxf(L, x);
      else if (x > zd) U = fminf(U, x);
    }
  }
  sL[t] = L;
  sU[t] = U;
  __syncthreads();
  if (t < D) {
    for (int u = t + D; u < S; u += D) { L = fmaxf(L, sL[u]); U = fminf(U, sU[u]); }
    const double z = (double)zd;
    const bool hasL = L != -INFINITY, hasU = U != INFINITY;
    double s = 0.0;
    if (hasL) s = z - (double)L;
    if (hasU) s = hasL ? fmax(s, (double)U - z) : (double)U - z;
    const double ps = p.psig[d];
    const double m = (double)p.n + (double)i + 1.0;
    s = fmin(fmax(s, ps / fmin(100.0, m + 2.0)), ps);
    p.liar_sigma[(int64_t)i * D + d] = s;
    double* row = p.rows + (int64_t)i * LS;
    row[d] = z;
    row[D + d] = 0.70710678118654752440 / s;
    // the mass of the normal truncated to the label's bounds (joint._std_bounds)
    const double za = (p.low[d] - z) / s, zb = (p.high[d] - z) / s;
    const bool flip = za > 0.0;
    const double a = flip ? -zb : za, b = flip ? -za : zb;
    const double fa = 0.5 * erfc(-a * 0.70710678118654752440), fb = 0.5 * erfc(-b * 0.70710678118654752440);
    sterm[d] = log(s * 2.50662827463100050242 * (fb - fa));
    if (zcopy) zcopy[d] = zd;
  }
  __syncthreads();
  if (t == 0) {
    double c = 0.0;
    for (int u = 0; u < D; ++u) c += sterm[u];
    p.rows[(int64_t)i * LS + 2 * D] = -c;
  }
  __syncthreads();                            // the row is written: the next liar of this launch may scan it
}

// step: 0 adds the given liars; j >= 1 merges step j - 1's chunk records into
// picks[j - 1], copies its row and adds it as liar G + j - 1
__global__ __launch_bounds__(kThreads) void k_liar_pick(const LiarK p, int step) {
  __shared__ float sL[kThreads], sU[kThreads];
  __shared__ double sterm[kMaxD];
  __shared__ Pick slot[kThreads / 64];
  const int t = threadIdx.x, D = p.D;
  if (step == 0) {
    for (int i = 0; i < p.G; ++i) add_liar(p, i, p.given + (int64_t)i * D, nullptr, sL, sU, sterm);
    return;
  }
  const int j = step - 1;
  Pick best{0, 0};
  for (int c = t; c < p.n_chunks; c += kThreads) {
    const tpe_joint_pick r = p.chunk_rec[c];
    if (r.idx < 0) continue;
    const Pick x{score_key(r.l - r.g), r.idx};
    if (beats(x, best)) best = x;            // (chunk order = candidate index order)
  }
  const Pick w = block_best(best, slot);
  const bool none = w.key == 0;
  if (t == 0) p.picks[j] = none ? tpe_joint_pick{-1, 0.0, 0.0} : p.chunk_rec[w.idx / TPE_JOINT_CHUNK];
  add_liar(p, p.G + j, none ? nullptr : p.cand + ((int64_t)j * p.C + w.idx) * D, p.pick_z + (int64_t)j * D, sL, sU,
           sterm);
}

// id j's candidates under the above mixture extended by J = G + j liars
__global__ __launch_bounds__(kThreads) void k_liar_chunk(const LiarK p, int j, double log_w, double log_norm) {
  __shared__ double tile[kTile * kMaxRow];
  __shared__ Pick slot[kThreads / 64];
  const int t = threadIdx.x, D = p.D, LS = 2 * D + 1, J = p.G + j;
  const int first = blockIdx.x * TPE_JOINT_CHUNK;
  const int64_t o = (int64_t)j * p.C;

  double m[kR], s[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) { m[r] = -1.0e300; s[r] = 0.0; }
  for (int q0 = 0; q0 < J; q0 += kTile) {
    const int nq = min(kTile, J - q0), nq4 = (nq + kQ - 1) / kQ * kQ;
    __syncthreads();                         // the previous tile is read
    for (int e = t; e < nq4 * LS; e += kThreads) {
      const int q = e / LS, f = e % LS;      // a padded liar: h = 0, c = -inf adds nothing
      tile[e] = q < nq ? p.rows[(int64_t)(q0 + q) * LS + f] : (f == 2 * D ? -INFINITY : 0.0);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int i = first + r * kThreads + t;
      if (i >= p.C) continue;
      const float* __restrict__ zr = p.cand + (o + i) * D;
      for (int qq = 0; qq < nq4; qq += kQ) {
        const double* __restrict__ row = tile + qq * LS;
        double acc[kQ];
#pragma unroll
        for (int u = 0; u < kQ; ++u) acc[u] = 0.0;
        for (int d = 0; d < D; ++d) {
          const double zd = (double)zr[d];
#pragma unroll
          for (int u = 0; u < kQ; ++u) {
            const double x = (zd - row[u * LS + d]) * row[u * LS + D + d];
            acc[u] = fma(x, x, acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < kQ; ++u) {
          const double tt = row[u * LS + 2 * D] - acc[u];
          const double dl = tt - m[r];
          const double e2 = exp(-fabs(dl));
          s[r] = dl > 0.0 ? fma(s[r], e2, 1.0) : s[r] + e2;
          m[r] = fmax(m[r], tt);
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
      const double x = m[r] + log(s[r]) - log_w;
      const double hi = fmax(g, x), lo = fmin(g, x);
      g = (hi == -INFINITY ? hi : hi + log1p(exp(lo - hi))) - log_norm;
    }
    gv[r] = g;
    const uint64_t key = score_key(lv[r] - g);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  const Pick w = block_best(best, slot);
  tpe_joint_pick* rec = p.chunk_rec + blockIdx.x;
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

// the scratch of one call in bytes, or false where the sizes are out of range
bool liar_scratch(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_given, uint64_t* rows_bytes, uint64_t* bytes) {
  if (n_ids < 1 || n_cand < 1 || n_dims < 1 || n_dims > kMaxD || n_given < 0) return false;
  const uint64_t chunks = ((uint64_t)n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK;
  *rows_bytes = ((uint64_t)n_ids + (uint64_t)n_given) * (2 * (uint64_t)n_dims + 1) * sizeof(double);
  *bytes = *rows_bytes + chunks * sizeof(tpe_joint_pick);
  return true;
}

}  // namespace

extern "C" {

int tpe_joint_liar_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_given, uint64_t* bytes) {
  uint64_t rows_bytes = 0;
  if (!bytes || !liar_scratch(n_ids, n_cand, n_dims, n_given, &rows_bytes, bytes))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar_scratch_bytes: bad arguments");
  return TPE_OK;
}

int tpe_joint_liar(const tpe_joint_liar_args* a, tpe_joint_pick* picks, float* pick_z, double* liar_sigma,
                   void* scratch, uint64_t scratch_bytes, void* stream) {
  tpe_internal_epoch_bump();
  if (!a) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: null args");
  if (a->n_dims < 1 || a->n_dims > kMaxD)
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
  if (a->n_ids < 1 || a->n_cand < 1 || a->k_above < 1)
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: n_ids / n_cand / k_above < 1");
  if (a->n_given < 0 || a->n_trials < 0) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: n_given / n_trials < 0");
  if (!(a->w_sum > 0.0) || !(a->w_sum < INFINITY))
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: w_sum must be positive and finite");
  if (!a->cand || !a->l_out || !a->g_out || !a->above_mu)
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: null cand / l_out / g_out / above_mu");
  if (a->n_given > 0 && !a->given) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: n_given > 0 without given");
  if (!picks || !pick_z || !liar_sigma) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: null outputs");
  for (int d = 0; d < a->n_dims; ++d)
    if (!(a->psig[d] > 0.0)) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: a prior sigma that is not positive");
  uint64_t rows_bytes = 0, need = 0;
  liar_scratch(a->n_ids, a->n_cand, a->n_dims, a->n_given, &rows_bytes, &need);
  if (!scratch || scratch_bytes < need) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_liar: scratch too small");

  LiarK k;
  k.D = a->n_dims; k.C = a->n_cand; k.K = a->k_above; k.G = a->n_given; k.n = a->n_trials;
  k.n_chunks = (int)(((int64_t)a->n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK);
  k.cand = a->cand; k.l_out = a->l_out; k.g_out = a->g_out; k.amu = a->above_mu; k.given = a->given;
  k.rows = (double*)scratch;
  k.chunk_rec = (tpe_joint_pick*)((char*)scratch + rows_bytes);
  k.picks = picks; k.pick_z = pick_z; k.liar_sigma = liar_sigma;
  for (int d = 0; d < kMaxD; ++d) {
    const bool in = d < a->n_dims;
    k.psig[d] = in ? a->psig[d] : 1.0;
    k.low[d] = in ? a->low[d] : -INFINITY;
    k.high[d] = in ? a->high[d] : INFINITY;
  }
  const hipStream_t s = (hipStream_t)stream;
  const double log_w = log(a->w_sum);
  if (k.G > 0) hipLaunchKernelGGL(k_liar_pick, dim3(1), dim3(kThreads), 0, s, k, 0);
  for (int j = 0; j < a->n_ids; ++j) {
    hipLaunchKernelGGL(k_liar_chunk, dim3((unsigned)k.n_chunks), dim3(kThreads), 0, s, k, j, log_w,
                       log1p((double)(k.G + j) / a->w_sum));
    hipLaunchKernelGGL(k_liar_pick, dim3(1), dim3(kThreads), 0, s, k, j + 1);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

}  // extern "C"
