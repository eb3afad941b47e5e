// MI355X (gfx950) joint TPE stage: whole-vector candidates scored under two
// product-kernel mixtures (include/tpe_hip.h, "Joint (multivariate) TPE
// stage").  Nothing on the univariate suggest path runs through this file.
//
// k_joint_chunk  one 256-thread workgroup per (new id, chunk of 1024
//                candidates).  A lane holds kR = 4 candidates' z[D] in
//                registers (candidate first + r * 256 + t: coalesced stores),
//                drawn from the below mixture (one component per candidate,
//                then D truncated-normal inversions) or loaded (inject).  Both
//                sides' rows stream through LDS in tiles of kTileK components;
//                every lane reads the same row, so an LDS read is a broadcast
//                that serves 64 * kR evaluations.  Per (candidate, component):
//                3 D VALU operations (subtract, scale, fma) and 7 for the
//                running-maximum sum of 2^term (one v_exp_f32).
// k_joint_mixed_chunk  the same for a group that also holds discrete labels: a
//                category costs one compare, one select and one add per
//                (candidate, component).
// k_joint_qtable  per side of a group with quantised labels: log2 of every
//                (component, lattice value) bin mass in f64, stored as f32.
// k_joint_quant_chunk  k_joint_mixed_chunk for such a group: the table streams
//                through LDS as [lattice value][component], and a quantised
//                dimension costs one read at the candidate's own lattice index
//                (four components a 16-byte read) and one add.
// k_joint_merge  one wave per new id: the chunk winners in index order.
// k_joint_seg_order / k_joint_seg_chunk  k_joint_chunk over the (id, group)
//                problems of many groups at once ("segmented stage" below): a
//                workgroup reads its problem's group descriptor, then runs the
//                same device code; k_joint_merge serves it unchanged.
// k_joint_mseg_qtable / k_joint_mseg_mixed_chunk / k_joint_mseg_quant_chunk  the
//                segmented stage for groups that also hold discrete and
//                quantised labels ("Mixed segmented joint stage"): one table
//                launch for all segments, then the mixed / quantised chunk
//                bodies (mixed_chunk_body, quant_chunk_body, shared with the
//                solo kernels) behind a descriptor read.
// k_joint_wide_sample / k_joint_wide_chunk / k_joint_wide_merge  the continuous
//                stage for 17 to 64 coordinates ("wide groups" below): the
//                candidates are drawn by a kernel of their own into scratch.
// k_joint_wide_mixed_sample / k_joint_wide_mixed_chunk  the wide stage for a
//                group that also holds up to 8 discrete labels.
// k_joint_wide_quant_sample / k_joint_wide_quant_chunk  the wide stage for a
//                group that also holds up to 4 quantised labels: k_joint_qtable's
//                tables stream through LDS beside the rows, in one common tile.
// k_joint_wide_seg_sample / k_joint_wide_seg_chunk  the wide continuous stage
//                over the (id, group) problems of many groups at once ("wide
//                segmented stage" below): a workgroup builds the solo kernels'
//                argument view of its problem from the group's descriptor and
//                runs their parts; k_joint_seg_order (over the wide classes)
//                and k_joint_wide_merge serve it.
// tpe_joint_run_shard  any of the six stages over the candidates [cand_base,
//                cand_base + n_cand) of a larger run: the views carry cand_base (a
//                kernel argument: scalar registers), added to the local index
//                where it becomes a Philox word or a record's global_idx, and
//                nowhere else (bounds tests and addressing stay local).
// Every reduction has a fixed shape and there are no atomics: the output bytes
// are a function of the input bytes.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/tpe_hip.h"
#include "tpe_device_rng.h"

extern "C" void tpe_internal_epoch_bump(void);                    // tpe_kernels.hip (hidden): the device epoch

extern "C" int tpe_internal_fail(int code, const char* what);   // tpe_kernels.hip (hidden)

namespace {

constexpr int kThreads = 256;                       // 4 waves of 64
constexpr int kR = TPE_JOINT_CHUNK / kThreads;      // candidates per lane
constexpr int kTileK = 128;                         // components per LDS tile
constexpr double kLn2 = 0.69314718055994530942;
static_assert(kR * kThreads == TPE_JOINT_CHUNK, "chunk = threads x candidates per lane");
static_assert(sizeof(tpe_joint_record) == 24 + 8 * TPE_JOINT_MAX_DIMS, "layout");

// the kernels' view of tpe_joint_args (f32 bounds made on the host)
struct JointK {
  int D, C, n_chunks, inject;
  int kb, ka;
  uint32_t key0, key1, stream_word;
  uint32_t cand_base;               // the global index of local candidate 0 (tpe_joint_run_shard)
  const float *bmu, *ba, *bc, *amu, *aa, *ac;
  double bbase, abase;
  const double* cum;
  const float* samp;
  const int64_t* ids;
  const float* inj;
  float lo[TPE_JOINT_MAX_DIMS], hi[TPE_JOINT_MAX_DIMS];
  float* cand;
  double *l_out, *g_out;
  tpe_joint_record* chunk_rec;      // scratch [n_ids * n_chunks]
};

// np.argmax order of a score as one unsigned key, larger = better, 0 = no
// candidate: every NaN the largest key, then the f64 bits made monotone (-0 as
// +0); -inf maps above 0  (as tpe_report.hip)
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
__device__ __forceinline__ Pick wave_best(Pick p) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    Pick o;
    o.key = (uint64_t)__shfl_xor((unsigned long long)p.key, m, 64);
    o.idx = (int64_t)__shfl_xor((long long)p.idx, m, 64);
    if (beats(o, p)) p = o;
  }
  return p;
}

// log2 of one side's mixture at the lane's kR candidates, rows through LDS.
// s accumulates 2^(term - m) with m the running maximum of the terms.
template <int DP>
__device__ __forceinline__ void score_side(const float* __restrict__ mu, const float* __restrict__ a,
                                           const float* __restrict__ c, int K, int D, const float (&z)[kR][DP],
                                           float* __restrict__ rows, float* __restrict__ cl, double (&out)[kR]) {
  float m[kR], s[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) { m[r] = -3.0e38f; s[r] = 0.f; }
  for (int k0 = 0; k0 < K; k0 += kTileK) {
    const int nk = min(kTileK, K - k0);
    __syncthreads();                       // the previous tile (or side) is read
    for (int e = threadIdx.x; e < nk * DP; e += kThreads) {
      const int kk = e / DP, d = e % DP;
      const bool in = d < D;               // padded dimensions: a = 0 adds nothing
      const int64_t src = (int64_t)(k0 + kk) * D + d;
      rows[kk * 2 * DP + d] = in ? mu[src] : 0.f;
      rows[kk * 2 * DP + DP + d] = in ? a[src] : 0.f;
    }
    for (int e = threadIdx.x; e < nk; e += kThreads) cl[e] = c[k0 + e];
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      const float* row = rows + kk * 2 * DP;
      float rm[DP], ra[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) { rm[d] = row[d]; ra[d] = row[DP + d]; }
      const float ck = cl[kk];
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const float u = (z[r][d] - rm[d]) * ra[d];
          acc = __builtin_fmaf(u, u, acc);
        }
        const float t = ck - acc;
        const float dl = t - m[r];
        const float e2 = __builtin_amdgcn_exp2f(-__builtin_fabsf(dl));
        s[r] = dl > 0.f ? __builtin_fmaf(s[r], e2, 1.f) : s[r] + e2;
        m[r] = fmaxf(m[r], t);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) out[r] = (double)m[r] + log2((double)s[r]);
}

// What one workgroup of k_joint_chunk / k_joint_seg_chunk works on: the model
// rows, the Philox words and the outputs of ONE (id, group) problem.  Every
// field is wave-uniform.
struct ChunkIO {
  int D, C, inject;
  int kb, ka;
  uint32_t key0, key1, stream_word, c3;   // c3: the new id's low word
  uint32_t base;                    // global index of local candidate 0: Philox word and record index only
  const float *bmu, *ba, *bc, *amu, *aa, *ac;
  double bbase, abase;
  const double* cum;
  const float* samp;
  const float* inj;
  float* cand;                      // the problem's [C][D] rows, or null
  double *l_out, *g_out;            // the problem's [C], or null
  tpe_joint_record* rec;            // this workgroup's chunk record
};

// The chunk of candidates [first, first + TPE_JOINT_CHUNK) of one problem: draw
// (or load) kR candidates a lane, score both sides, write the optional outputs
// and the chunk winner.  blo / bhi: the f32 bounds of the DP padded dimensions.
template <int DP>
__device__ __forceinline__ void joint_chunk_body(const ChunkIO& p, const float (&blo)[DP], const float (&bhi)[DP],
                                                 int first, float* __restrict__ rows, float* __restrict__ cl,
                                                 Pick* __restrict__ slot) {
  const int t = threadIdx.x, D = p.D;

  float z[kR][DP];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
#pragma unroll
    for (int d = 0; d < DP; ++d) z[r][d] = 0.f;
    const int i = first + r * kThreads + t;
    if (i >= p.C) continue;
    if (p.inject) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) z[r][d] = p.inj[(int64_t)i * D + d];
      continue;
    }
    const uint32_t c3 = p.c3, gi = p.base + (uint32_t)i;   // gi < 2^31: i < C and base + C <= n_cand_global
    U4 w = philox4x32_10(gi, 0u, p.stream_word, c3, p.key0, p.key1);
    const double us = u01w(w.x);
    int lo = 0, hi = p.kb - 1;             // first k with us < cum[k]
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (us < p.cum[mid]) hi = mid; else lo = mid + 1; }
    const float* srow = p.samp + (int64_t)lo * D * 5;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      if (d >= D) continue;
      const int wi = d + 1;
      if ((wi & 3) == 0) w = philox4x32_10(gi, (uint32_t)(wi >> 2), p.stream_word, c3, p.key0, p.key1);
      const uint32_t word = (wi & 3) == 0 ? w.x : (wi & 3) == 1 ? w.y : (wi & 3) == 2 ? w.z : w.w;
      const float* sr = srow + d * 5;
      const float pr = sr[2] + u01f(word) * (sr[3] - sr[2]);
      float zz = ndtri_f32(pr);
      if (sr[4] != 0.f) zz = -zz;
      float x = sr[0] + sr[1] * zz;
      if (!(x == x)) x = sr[0];
      z[r][d] = fminf(fmaxf(x, blo[d]), bhi[d]);        // low <= z < high
    }
  }

  double l2[kR], g2[kR];
  score_side<DP>(p.bmu, p.ba, p.bc, p.kb, D, z, rows, cl, l2);
  score_side<DP>(p.amu, p.aa, p.ac, p.ka, D, z, rows, cl, g2);

  Pick best{0, 0};
  double lv[kR], gv[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = l2[r] * kLn2 + p.bbase;
    gv[r] = g2[r] * kLn2 + p.abase;
    if (i >= p.C) continue;
    if (p.l_out) p.l_out[i] = lv[r];
    if (p.g_out) p.g_out[i] = gv[r];
    if (p.cand)
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) p.cand[(int64_t)i * D + d] = z[r][d];
    const uint64_t key = score_key(lv[r] - gv[r]);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  Pick w = wave_best(best);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  w = slot[0];
#pragma unroll
  for (int q = 1; q < kThreads / 64; ++q)
    if (beats(slot[q], w)) w = slot[q];

  tpe_joint_record* rec = p.rec;
  if (w.key == 0) {
    if (t == 0) rec->global_idx = -1;
    return;
  }
  const int off = (int)(w.idx - first);
  if (t != off % kThreads) return;
  const int wr = off / kThreads;
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    if (r != wr) continue;
    rec->global_idx = w.idx + (int64_t)p.base;
    rec->l = lv[r];
    rec->g = gv[r];
#pragma unroll
    for (int d = 0; d < TPE_JOINT_MAX_DIMS; ++d) rec->z[d] = d < DP ? (double)z[r][d < DP ? d : 0] : 0.0;
  }
}

template <int DP>
__global__ __launch_bounds__(kThreads) void k_joint_chunk(const JointK p) {
  __shared__ __attribute__((aligned(16))) float rows[kTileK * 2 * DP];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  const int id = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;

  ChunkIO q;
  q.D = p.D; q.C = p.C; q.inject = p.inject;
  q.kb = p.kb; q.ka = p.ka;
  q.key0 = p.key0; q.key1 = p.key1; q.stream_word = p.stream_word;
  q.c3 = p.inject ? 0u : (uint32_t)p.ids[id];
  q.base = p.cand_base;
  q.bmu = p.bmu; q.ba = p.ba; q.bc = p.bc; q.amu = p.amu; q.aa = p.aa; q.ac = p.ac;
  q.bbase = p.bbase; q.abase = p.abase;
  q.cum = p.cum; q.samp = p.samp; q.inj = p.inj;
  const int64_t o = (int64_t)id * p.C;
  q.cand = p.cand ? p.cand + o * p.D : nullptr;
  q.l_out = p.l_out ? p.l_out + o : nullptr;
  q.g_out = p.g_out ? p.g_out + o : nullptr;
  q.rec = p.chunk_rec + blockIdx.x;
  float blo[DP], bhi[DP];                  // (kernel-argument arrays: constant indices only)
#pragma unroll
  for (int d = 0; d < DP; ++d) { blo[d] = p.lo[d]; bhi[d] = p.hi[d]; }
  joint_chunk_body<DP>(q, blo, bhi, chunk * TPE_JOINT_CHUNK, rows, cl, slot);
}

// --------------------------------------------------------- segmented stage
// One launch scores problems of MANY groups (include/tpe_hip.h "Segmented joint
// stage"): a workgroup reads its problem's group descriptor and then runs
// joint_chunk_body, so a problem's bytes are those of a k_joint_chunk launch
// over that group alone.
struct SegK {
  int C, n_chunks, inject, first;   // first: this launch's first entry of `order`
  int n_probs, n_segs;
  uint32_t key0, key1;
  uint32_t cand_base;               // as JointK
  const tpe_joint_seg* segs;        // (MIXED kernels: the tpe_joint_mseg array behind this pointer)
  const float* pool;
  const double* pool64;
  const int32_t* prob_seg;
  const int64_t* prob_id;
  const int64_t* cand_off;
  int32_t* order;                   // scratch [n_probs]: the problems by (DP class, group, index)
  float* cand;
  double *l_out, *g_out;
  tpe_joint_record* chunk_rec;      // scratch [n_probs * n_chunks], problem-major
};

// the kernel instantiation of a group of D dimensions, as an index 0 .. 7
__host__ __device__ __forceinline__ int dp_class(int D) {
  return D <= 4 ? D - 1 : D <= 6 ? 4 : D <= 8 ? 5 : D <= 12 ? 6 : 7;
}

// The kernel instantiation of a segment with Dc continuous, Dk discrete and Dq
// quantised coordinates as an index 0 .. kMClasses - 1: the continuous DP
// classes first (dp_class), then the 12 (CP, KP) shapes of the mixed kernel,
// then the 48 (CP, KP, QP) shapes of the quantised one.
constexpr int kMClasses = 8 + 12 + 48;
__host__ __device__ __forceinline__ int cp_index(int Dc) { return Dc == 0 ? 0 : Dc <= 2 ? 1 : Dc <= 4 ? 2 : 3; }
__host__ __device__ __forceinline__ int mseg_class(int Dc, int Dk, int Dq) {
  if (Dq > 0) return 20 + (cp_index(Dc) * 4 + (Dk <= 2 ? Dk : 3)) * 3 + (Dq <= 2 ? Dq - 1 : 2);
  if (Dk > 0) return 8 + cp_index(Dc) * 3 + (Dk <= 2 ? Dk - 1 : 2);
  return dp_class(Dc);
}

// Segment s of a launch.  MIXED: the descriptors are tpe_joint_mseg (the launches
// of tpe_joint_mseg_run), and this is the tpe_joint_seg at the head of one.
__device__ __forceinline__ const tpe_joint_mseg* mseg_at(const SegK& p, int s) {
  return reinterpret_cast<const tpe_joint_mseg*>(p.segs) + s;
}
template <bool MIXED>
__device__ __forceinline__ const tpe_joint_seg* seg_at(const SegK& p, int s) {
  if constexpr (MIXED) return reinterpret_cast<const tpe_joint_seg*>(mseg_at(p, s));
  else return p.segs + s;
}
template <bool MIXED>
__device__ __forceinline__ int seg_class(const SegK& p, int s) {
  if constexpr (MIXED) {
    const tpe_joint_mseg* m = mseg_at(p, s);
    return mseg_class(m->n_dims, m->n_cat, m->n_quant);
  } else {
    return dp_class(p.segs[s].n_dims);
  }
}

// order[rank of p] = p, the rank by (kernel class, group, problem index): one
// thread a problem counts the problems before it.  No atomics; P^2 / 256 reads a
// workgroup from arrays that sit in L2.
// (K: SegK, or the wide segmented stage's WideSegK with its own seg_class)
template <bool MIXED, typename K>
__global__ __launch_bounds__(kThreads) void k_joint_seg_order(const K p) {
  const int me = blockIdx.x * kThreads + threadIdx.x;
  if (me >= p.n_probs) return;
  const int sme = p.prob_seg[me];
  const int kme = seg_class<MIXED>(p, sme) * p.n_segs + sme;
  int rank = 0;
  for (int q = 0; q < p.n_probs; ++q) {
    const int sq = p.prob_seg[q];
    const int kq = seg_class<MIXED>(p, sq) * p.n_segs + sq;
    rank += (kq < kme || (kq == kme && q < me)) ? 1 : 0;
  }
  p.order[rank] = me;
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni(int64_t v) {
  return (int64_t)(((uint64_t)(uint32_t)uni((int)((uint64_t)v >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)v));
}
__device__ __forceinline__ float unif(float v) { return __int_as_float(uni(__float_as_int(v))); }
__device__ __forceinline__ double unid(double v) { return __longlong_as_double(uni((int64_t)__double_as_longlong(v))); }

template <int DP, bool MIXED>
__global__ __launch_bounds__(kThreads) void k_joint_seg_chunk(const SegK p) {
  __shared__ __attribute__((aligned(16))) float rows[kTileK * 2 * DP];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  const int chunk = blockIdx.x % p.n_chunks;
  // the problem and its group: the same for every lane, kept in scalar registers
  const int prob = uni(p.order[p.first + blockIdx.x / p.n_chunks]);
  const tpe_joint_seg* __restrict__ sg = seg_at<MIXED>(p, uni(p.prob_seg[prob]));

  ChunkIO q;
  q.D = uni(sg->n_dims); q.C = p.C; q.inject = p.inject;
  q.kb = uni(sg->k_below); q.ka = uni(sg->k_above);
  q.key0 = p.key0; q.key1 = p.key1; q.stream_word = (uint32_t)uni((int)sg->stream_word);
  q.c3 = (uint32_t)uni((int)(uint32_t)p.prob_id[prob]);
  q.base = p.cand_base;
  q.bmu = p.pool + uni(sg->below_mu); q.ba = p.pool + uni(sg->below_a); q.bc = p.pool + uni(sg->below_c);
  q.amu = p.pool + uni(sg->above_mu); q.aa = p.pool + uni(sg->above_a); q.ac = p.pool + uni(sg->above_c);
  q.bbase = unid(sg->below_base); q.abase = unid(sg->above_base);
  q.cum = p.inject ? nullptr : p.pool64 + uni(sg->samp_cum);
  q.samp = p.inject ? nullptr : p.pool + uni(sg->samp);
  q.inj = p.inject ? p.pool + uni(sg->inject) : nullptr;
  q.cand = p.cand ? p.cand + uni(p.cand_off[prob]) : nullptr;
  q.l_out = p.l_out ? p.l_out + (int64_t)prob * p.C : nullptr;
  q.g_out = p.g_out ? p.g_out + (int64_t)prob * p.C : nullptr;
  q.rec = p.chunk_rec + (int64_t)prob * p.n_chunks + chunk;
  float blo[DP], bhi[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) { blo[d] = unif(sg->lo[d]); bhi[d] = unif(sg->hi[d]); }
  joint_chunk_body<DP>(q, blo, bhi, chunk * TPE_JOINT_CHUNK, rows, cl, slot);
}

__global__ __launch_bounds__(64) void k_joint_merge(const tpe_joint_record* __restrict__ chunk_rec, int n_chunks,
                                                    tpe_joint_record* __restrict__ records) {
  const tpe_joint_record* rec = chunk_rec + (int64_t)blockIdx.x * n_chunks;
  Pick best{0, 0};
  for (int c = threadIdx.x; c < n_chunks; c += 64) {
    if (rec[c].global_idx < 0) continue;
    const Pick x{score_key(rec[c].l - rec[c].g), (int64_t)c};
    if (beats(x, best)) best = x;            // (chunk order = candidate index order)
  }
  const Pick w = wave_best(best);
  if (threadIdx.x != 0) return;
  tpe_joint_record* out = records + blockIdx.x;
  if (w.key == 0) {
    out->global_idx = -1;
    out->l = out->g = 0.0;
    for (int d = 0; d < TPE_JOINT_MAX_DIMS; ++d) out->z[d] = 0.0;
  } else {
    *out = rec[w.idx];
  }
}

// ------------------------------------------------------------ mixed groups
// Dc continuous coordinates (as above) followed by Dk discrete ones; a category
// is its index as an f32 (include/tpe_hip.h "Mixed joint stage").
struct MixedK {
  JointK j;                         // j.D = Dc; cand / inject rows are [Dc + Dk]
  int Dk;
  int U[TPE_JOINT_MAX_DIMS], off[TPE_JOINT_MAX_DIMS];
  const float *bcat, *acat;
  const float *bmiss, *bbonus, *amiss, *abonus;
  const double* bh;
  const double* ccum;
};

// the candidate's category of dimension d as a table index (a category outside
// [0, U) is the caller's error: the index is kept inside the table, no more)
__device__ __forceinline__ int cat_index(float v, int U) { return min(max((int)v, 0), U - 1); }

// score_side with KP discrete dimensions: a component's term gains the
// candidate's bonus where the categories are equal.  nb = -bonus_d(v_d) is read
// once per candidate here; per (candidate, component) and dimension then one
// compare, one select and one add.  out gets + sum_d miss_d(v_d) in f64.
template <int CP, int KP>
__device__ __forceinline__ void score_side_mixed(const float* __restrict__ mu, const float* __restrict__ a,
                                                 const float* __restrict__ c, const float* __restrict__ cat,
                                                 const float* __restrict__ miss, const float* __restrict__ bonus,
                                                 int K, int Dc, int Dk, const int (&U)[KP], const int (&off)[KP],
                                                 const float (&z)[kR][CP + KP], float* __restrict__ rows,
                                                 float* __restrict__ cl, double (&out)[kR]) {
  constexpr int S = 2 * CP + KP;
  float m[kR], s[kR], nb[kR][KP];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    m[r] = -3.0e38f;
    s[r] = 0.f;
#pragma unroll
    for (int d = 0; d < KP; ++d) nb[r][d] = d < Dk ? -bonus[off[d] + cat_index(z[r][CP + d], U[d])] : 0.f;
  }
  for (int k0 = 0; k0 < K; k0 += kTileK) {
    const int nk = min(kTileK, K - k0);
    __syncthreads();                       // the previous tile (or side) is read
    if constexpr (CP > 0)
      for (int e = threadIdx.x; e < nk * CP; e += kThreads) {
        const int kk = e / CP, d = e % CP;
        const bool in = d < Dc;              // padded dimensions: a = 0 adds nothing
        const int64_t src = (int64_t)(k0 + kk) * Dc + d;
        rows[kk * S + d] = in ? mu[src] : 0.f;
        rows[kk * S + CP + d] = in ? a[src] : 0.f;
      }
    for (int e = threadIdx.x; e < nk * KP; e += kThreads) {
      const int kk = e / KP, d = e % KP;     // padded dimensions: category -1 never matches
      rows[kk * S + 2 * CP + d] = d < Dk ? cat[(int64_t)(k0 + kk) * Dk + d] : -1.f;
    }
    for (int e = threadIdx.x; e < nk; e += kThreads) cl[e] = c[k0 + e];
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      const float* row = rows + kk * S;
      float rm[CP + 1], ra[CP + 1], rc[KP];
#pragma unroll
      for (int d = 0; d < CP; ++d) { rm[d] = row[d]; ra[d] = row[CP + d]; }
#pragma unroll
      for (int d = 0; d < KP; ++d) rc[d] = row[2 * CP + d];
      const float ck = cl[kk];
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < CP; ++d) {
          const float u = (z[r][d] - rm[d]) * ra[d];
          acc = __builtin_fmaf(u, u, acc);
        }
#pragma unroll
        for (int d = 0; d < KP; ++d) acc += z[r][CP + d] == rc[d] ? nb[r][d] : 0.f;
        const float t = ck - acc;
        const float dl = t - m[r];
        const float e2 = __builtin_amdgcn_exp2f(-__builtin_fabsf(dl));
        s[r] = dl > 0.f ? __builtin_fmaf(s[r], e2, 1.f) : s[r] + e2;
        m[r] = fmaxf(m[r], t);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    double M = 0.0;
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) M += (double)miss[off[d] + cat_index(z[r][CP + d], U[d])];
    out[r] = (double)m[r] + log2((double)s[r]) + M;
  }
}

// What one workgroup of k_joint_mixed_chunk / k_joint_mseg_mixed_chunk works on:
// ChunkIO (q.D = Dc; cand / inject rows are [Dc + Dk]) and the discrete part of
// ONE (id, group) problem.  Every field is wave-uniform; the arrays are only
// ever indexed by constants (they stay in scalar registers).
template <int CP, int KP>
struct MixedIO {
  ChunkIO q;
  int Dk;
  float lo[CP > 0 ? CP : 1], hi[CP > 0 ? CP : 1];
  int U[KP], off[KP];
  const float *bcat, *acat;
  const float *bmiss, *bbonus, *amiss, *abonus;
  const double* bh;
  const double* ccum;
};

// joint_chunk_body for a mixed group: CP / KP the padded continuous / discrete
// counts (CP = 0: an all-discrete group).  z[r] holds the continuous
// coordinates at [0, CP) and the categories at [CP, CP + KP).
template <int CP, int KP>
__device__ __forceinline__ void mixed_chunk_body(const MixedIO<CP, KP>& p, int first, float* __restrict__ rows,
                                                 float* __restrict__ cl, Pick* __restrict__ slot) {
  constexpr int ZP = CP + KP;
  const ChunkIO& q = p.q;
  const int t = threadIdx.x, Dc = q.D, Dk = p.Dk, D = Dc + Dk;

  float z[kR][ZP];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
#pragma unroll
    for (int d = 0; d < ZP; ++d) z[r][d] = 0.f;
    const int i = first + r * kThreads + t;
    if (i >= q.C) continue;
    if (q.inject) {
#pragma unroll
      for (int d = 0; d < CP; ++d)
        if (d < Dc) z[r][d] = q.inj[(int64_t)i * D + d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) z[r][CP + d] = q.inj[(int64_t)i * D + Dc + d];
      continue;
    }
    const uint32_t c3 = q.c3, gi = q.base + (uint32_t)i;   // gi < 2^31: i < C and base + C <= n_cand_global
    U4 w = philox4x32_10(gi, 0u, q.stream_word, c3, q.key0, q.key1);
    const double us = u01w(w.x);
    int lo = 0, hi = q.kb - 1;             // first k with us < cum[k]
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (us < q.cum[mid]) hi = mid; else lo = mid + 1; }
    const int comp = lo;
    const float* srow = q.samp + (int64_t)comp * Dc * 5;
    // One loop over the kernel coordinates, not unrolled (4 (CP + KP) copies of
    // the samplers would keep z out of registers); word 1 + j serves coordinate
    // j, and a continuous one is k_joint_chunk's draw, operation for operation.
    for (int j = 0; j < D; ++j) {
      const int wi = j + 1;
      if ((wi & 3) == 0) w = philox4x32_10(gi, (uint32_t)(wi >> 2), q.stream_word, c3, q.key0, q.key1);
      const uint32_t word = (wi & 3) == 0 ? w.x : (wi & 3) == 1 ? w.y : (wi & 3) == 2 ? w.z : w.w;
      float x;
      if (j < Dc) {
        const float* sr = srow + j * 5;
        const float pr = sr[2] + u01f(word) * (sr[3] - sr[2]);
        float zz = ndtri_f32(pr);
        if (sr[4] != 0.f) zz = -zz;
        x = sr[0] + sr[1] * zz;
        if (!(x == x)) x = sr[0];
        float blo = 0.f, bhi = 0.f;                       // (the bound arrays: constant indices only)
#pragma unroll
        for (int f = 0; f < CP; ++f)
          if (f == j) { blo = p.lo[f]; bhi = p.hi[f]; }
        x = fminf(fmaxf(x, blo), bhi);                    // low <= z < high
      } else {
        const int d = j - Dc;
        const double u = u01w(word);
        x = p.bcat[(int64_t)comp * Dk + d];               // the component's category, -1: the prior row
        const double h = x >= 0.f ? p.bh[d] : 0.0;
        if (!(u < h)) {
          const double u2 = (u - h) / (1.0 - h);
          int off = 0, U = 1;
#pragma unroll
          for (int f = 0; f < KP; ++f)
            if (f == d) { off = p.off[f]; U = p.U[f]; }
          const double* cum = p.ccum + off;
          int a = 0, b = U - 1;                           // first category with u2 < cum[v]
          while (a < b) { const int mid = (a + b) >> 1; if (u2 < cum[mid]) b = mid; else a = mid + 1; }
          x = (float)a;
        }
      }
      const int e = j < Dc ? j : CP + (j - Dc);
#pragma unroll
      for (int f = 0; f < ZP; ++f)
        if (f == e) z[r][f] = x;
    }
  }

  double l2[kR], g2[kR];
  score_side_mixed<CP, KP>(q.bmu, q.ba, q.bc, p.bcat, p.bmiss, p.bbonus, q.kb, Dc, Dk, p.U, p.off, z, rows, cl, l2);
  score_side_mixed<CP, KP>(q.amu, q.aa, q.ac, p.acat, p.amiss, p.abonus, q.ka, Dc, Dk, p.U, p.off, z, rows, cl, g2);

  Pick best{0, 0};
  double lv[kR], gv[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = l2[r] * kLn2 + q.bbase;
    gv[r] = g2[r] * kLn2 + q.abase;
    if (i >= q.C) continue;
    if (q.l_out) q.l_out[i] = lv[r];
    if (q.g_out) q.g_out[i] = gv[r];
    if (q.cand) {
#pragma unroll
      for (int d = 0; d < CP; ++d)
        if (d < Dc) q.cand[(int64_t)i * D + d] = z[r][d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) q.cand[(int64_t)i * D + Dc + d] = z[r][CP + d];
    }
    const uint64_t key = score_key(lv[r] - gv[r]);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  Pick w = wave_best(best);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  w = slot[0];
#pragma unroll
  for (int s = 1; s < kThreads / 64; ++s)
    if (beats(slot[s], w)) w = slot[s];

  tpe_joint_record* rec = q.rec;
  if (w.key == 0) {
    if (t == 0) rec->global_idx = -1;
    return;
  }
  const int off = (int)(w.idx - first);
  if (t != off % kThreads) return;
  const int wr = off / kThreads;
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    if (r != wr) continue;
    rec->global_idx = w.idx + (int64_t)q.base;
    rec->l = lv[r];
    rec->g = gv[r];
    // kernel coordinate order: the Dc continuous entries, the categories, then zeros
#pragma unroll
    for (int d = 0; d < TPE_JOINT_MAX_DIMS; ++d)
      if (d >= D) rec->z[d] = 0.0;
#pragma unroll
    for (int d = 0; d < CP; ++d)
      if (d < Dc) rec->z[d] = (double)z[r][d];
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) rec->z[Dc + d] = (double)z[r][CP + d];
  }
}

// ChunkIO of workgroup blockIdx.x of a solo launch (JointK: k_joint_chunk's
// arguments) over a group of D coordinates in all
__device__ __forceinline__ void solo_chunk_io(ChunkIO& q, const JointK& p, int D) {
  const int id = blockIdx.x / p.n_chunks;
  q.D = p.D; q.C = p.C; q.inject = p.inject;
  q.kb = p.kb; q.ka = p.ka;
  q.key0 = p.key0; q.key1 = p.key1; q.stream_word = p.stream_word;
  q.c3 = p.inject ? 0u : (uint32_t)p.ids[id];
  q.base = p.cand_base;
  q.bmu = p.bmu; q.ba = p.ba; q.bc = p.bc; q.amu = p.amu; q.aa = p.aa; q.ac = p.ac;
  q.bbase = p.bbase; q.abase = p.abase;
  q.cum = p.cum; q.samp = p.samp; q.inj = p.inj;
  const int64_t o = (int64_t)id * p.C;
  q.cand = p.cand ? p.cand + o * D : nullptr;
  q.l_out = p.l_out ? p.l_out + o : nullptr;
  q.g_out = p.g_out ? p.g_out + o : nullptr;
  q.rec = p.chunk_rec + blockIdx.x;
}

// (From 12 padded coordinates on the register allocator is told not to aim above
// 2 waves a SIMD: left alone it spills a few dwords to hold 3.)
template <int CP, int KP>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, (CP + KP >= 12 ? 2 : 8))))
void k_joint_mixed_chunk(const MixedK p) {
  __shared__ __attribute__((aligned(16))) float rows[kTileK * (2 * CP + KP)];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  MixedIO<CP, KP> io;
  solo_chunk_io(io.q, p.j, p.j.D + p.Dk);
  io.Dk = p.Dk;
#pragma unroll
  for (int d = 0; d < CP; ++d) { io.lo[d] = p.j.lo[d]; io.hi[d] = p.j.hi[d]; }   // (kernel-argument arrays: constant indices only)
#pragma unroll
  for (int d = 0; d < KP; ++d) { io.U[d] = p.U[d]; io.off[d] = p.off[d]; }
  io.bcat = p.bcat; io.acat = p.acat;
  io.bmiss = p.bmiss; io.bbonus = p.bbonus; io.amiss = p.amiss; io.abonus = p.abonus;
  io.bh = p.bh; io.ccum = p.ccum;
  mixed_chunk_body<CP, KP>(io, (int)(blockIdx.x % p.j.n_chunks) * TPE_JOINT_CHUNK, rows, cl, slot);
}

// The segmented launch of the same body: the problem's descriptor (a
// tpe_joint_mseg) read into scalar registers, as k_joint_seg_chunk does.
struct MSegK {
  SegK s;                           // s.segs: the tpe_joint_mseg array
  float* table;                     // the table workspace
};

__device__ __forceinline__ void mseg_chunk_io(ChunkIO& q, const SegK& p, const tpe_joint_mseg* __restrict__ sg, int prob,
                                              int chunk) {
  q.D = uni(sg->n_dims); q.C = p.C; q.inject = p.inject;
  q.kb = uni(sg->k_below); q.ka = uni(sg->k_above);
  q.key0 = p.key0; q.key1 = p.key1; q.stream_word = (uint32_t)uni((int)sg->stream_word);
  q.c3 = (uint32_t)uni((int)(uint32_t)p.prob_id[prob]);
  q.base = p.cand_base;
  q.bmu = p.pool + uni(sg->below_mu); q.ba = p.pool + uni(sg->below_a); q.bc = p.pool + uni(sg->below_c);
  q.amu = p.pool + uni(sg->above_mu); q.aa = p.pool + uni(sg->above_a); q.ac = p.pool + uni(sg->above_c);
  q.bbase = unid(sg->below_base); q.abase = unid(sg->above_base);
  q.cum = p.inject ? nullptr : p.pool64 + uni(sg->samp_cum);
  q.samp = p.inject ? nullptr : p.pool + uni(sg->samp);
  q.inj = p.inject ? p.pool + uni(sg->inject) : nullptr;
  q.cand = p.cand ? p.cand + uni(p.cand_off[prob]) : nullptr;
  q.l_out = p.l_out ? p.l_out + (int64_t)prob * p.C : nullptr;
  q.g_out = p.g_out ? p.g_out + (int64_t)prob * p.C : nullptr;
  q.rec = p.chunk_rec + (int64_t)prob * p.n_chunks + chunk;
}

template <int CP, int KP>
__device__ __forceinline__ void mseg_mixed_io(MixedIO<CP, KP>& io, const SegK& p, const tpe_joint_mseg* __restrict__ sg) {
  io.Dk = uni(sg->n_cat);
#pragma unroll
  for (int d = 0; d < CP; ++d) { io.lo[d] = unif(sg->lo[d]); io.hi[d] = unif(sg->hi[d]); }
#pragma unroll
  for (int d = 0; d < KP; ++d) { io.U[d] = uni(sg->cat_upper[d]); io.off[d] = uni(sg->cat_off[d]); }
  io.bcat = p.pool + uni(sg->below_cat); io.acat = p.pool + uni(sg->above_cat);
  io.bmiss = p.pool + uni(sg->below_miss); io.bbonus = p.pool + uni(sg->below_bonus);
  io.amiss = p.pool + uni(sg->above_miss); io.abonus = p.pool + uni(sg->above_bonus);
  io.bh = p.inject ? nullptr : p.pool64 + uni(sg->below_h);
  io.ccum = p.inject ? nullptr : p.pool64 + uni(sg->cat_cum);
}

template <int CP, int KP>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, (CP + KP >= 12 ? 2 : 8))))
void k_joint_mseg_mixed_chunk(const MSegK p) {
  static_assert(KP <= TPE_JOINT_MSEG_MAX_CAT && CP <= TPE_JOINT_MSEG_MAX_CONT, "the descriptor's arrays");
  __shared__ __attribute__((aligned(16))) float rows[kTileK * (2 * CP + KP)];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  const int chunk = blockIdx.x % p.s.n_chunks;
  const int prob = uni(p.s.order[p.s.first + blockIdx.x / p.s.n_chunks]);
  const tpe_joint_mseg* __restrict__ sg = mseg_at(p.s, uni(p.s.prob_seg[prob]));
  MixedIO<CP, KP> io;
  mseg_chunk_io(io.q, p.s, sg, prob, chunk);
  mseg_mixed_io<CP, KP>(io, p.s, sg);
  mixed_chunk_body<CP, KP>(io, chunk * TPE_JOINT_CHUNK, rows, cl, slot);
}


// -------------------------------------------------------- quantised groups
// Dc continuous and Dk discrete coordinates (as above) followed by Dq
// quantised ones; a quantised coordinate is its lattice index as an f32
// (include/tpe_hip.h "Quantised joint stage").
constexpr int kQTileBytes = 41 * 1024;      // the table tile's share of the LDS (dynamic)
constexpr double kQFloor = (double)TPE_JOINT_QFLOOR;

struct QuantK {
  MixedK m;                         // m.j.D = Dc, m.Dk = Dk; cand / inject rows are [Dc + Dk + Dq]
  int Dq, tile, stride, total;      // components per tile, floats per lattice value in the tile, sum V_d
  int V[TPE_JOINT_MAX_QUANT], voff[TPE_JOINT_MAX_QUANT], eoff[TPE_JOINT_MAX_QUANT];
  float qlo[TPE_JOINT_MAX_QUANT], qhi[TPE_JOINT_MAX_QUANT];
  const double* edges;
  const float* qsamp;
  const float *bT, *aT;             // [total][K] of a side
};

// One side's table: thread k of block row d walks the V_d + 1 edges of its
// (component, dimension) once, one erfc per edge (the smaller tail), shared by
// the two bins that meet there.
struct QTabK {
  int K, Dq;
  int V[TPE_JOINT_MAX_QUANT], voff[TPE_JOINT_MAX_QUANT], eoff[TPE_JOINT_MAX_QUANT];
  const double *mu, *sigma, *edges;
  float* T;
};

// The smaller tail of a standardised edge, u = |e - mu| / (sigma sqrt 2).  Beyond
// kQTailMax the tail (below 2^-1018) counts as exactly 0: float64 would go
// subnormal there, and the result must not depend on how a libm rounds them.
constexpr double kQTailMax = 26.5;
__device__ __forceinline__ double small_tail(double u) { return u > kQTailMax ? 0.0 : 0.5 * erfc(u); }

// Phi(tb) - Phi(ta) of ta < tb from the smaller tails sa, sb
__device__ __forceinline__ double bin_mass(double ta, double sa, double tb, double sb) {
  return tb <= 0.0 ? sb - sa : ta >= 0.0 ? sa - sb : 1.0 - sa - sb;
}

// One (component, dimension) column of a side's table: walk the V + 1 edges e of
// the dimension once, one erfc per edge (the smaller tail), shared by the two
// bins that meet there; out[i * K] = log2 P(i), floored at TPE_JOINT_QFLOOR.
__device__ __forceinline__ void qtable_column(double m, double s, const double* __restrict__ e, int V,
                                              float* __restrict__ out, int K) {
  const double r = 0.70710678118654752440 / s;
  const double t0 = (e[0] - m) * r, tv = (e[V] - m) * r;
  const double s0 = small_tail(fabs(t0)), sv = small_tail(fabs(tv));
  const double lmass = log2(bin_mass(t0, s0, tv, sv));
  double ta = t0, sa = s0;
  for (int i = 0; i < V; ++i) {
    const double tb = i + 1 < V ? (e[i + 1] - m) * r : tv;
    const double sb = i + 1 < V ? small_tail(fabs(tb)) : sv;
    double v = log2(bin_mass(ta, sa, tb, sb)) - lmass;
    if (!(v >= kQFloor)) v = kQFloor;       // -inf (a far bin's mass is 0) and NaN included
    out[(int64_t)i * K] = (float)v;
    ta = tb; sa = sb;
  }
}


__global__ __launch_bounds__(kThreads) void k_joint_qtable(const QTabK p) {
  const int k = blockIdx.x * kThreads + threadIdx.x, d = blockIdx.y;
  if (k >= p.K) return;
  int V = 2, voff = 0, eoff = 0;            // (kernel-argument arrays: constant indices only)
#pragma unroll
  for (int f = 0; f < TPE_JOINT_MAX_QUANT; ++f)
    if (f == d) { V = p.V[f]; voff = p.voff[f]; eoff = p.eoff[f]; }
  qtable_column(p.mu[(int64_t)k * p.Dq + d], p.sigma[(int64_t)k * p.Dq + d], p.edges + eoff, V,
                p.T + (int64_t)voff * p.K + k, p.K);
}

// k_joint_qtable for every quantised segment and side of a tpe_joint_mseg_run in
// one launch: blockIdx.z = 2 * segment + side, blockIdx.y the quantised
// dimension, thread k of blockIdx.x the component.  A segment's table holds the
// bytes its solo run builds (qtable_column).
__global__ __launch_bounds__(kThreads) void k_joint_mseg_qtable(const MSegK p) {
  const tpe_joint_mseg* __restrict__ sg = mseg_at(p.s, (int)(blockIdx.z >> 1));
  const int side = blockIdx.z & 1, d = blockIdx.y, Dq = sg->n_quant;
  const int kb = sg->k_below, K = side ? sg->k_above : kb;
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (d >= Dq || k >= K) return;
  int voff = 0, total = 0;
  for (int f = 0; f < Dq; ++f) {
    if (f < d) voff += sg->quant_v[f];
    total += sg->quant_v[f];
  }
  const double* mu = p.s.pool64 + (side ? sg->above_qmu : sg->below_qmu);
  const double* sigma = p.s.pool64 + (side ? sg->above_qsigma : sg->below_qsigma);
  float* T = p.table + sg->table + (side ? (int64_t)total * kb : 0);
  qtable_column(mu[(int64_t)k * Dq + d], sigma[(int64_t)k * Dq + d],
                p.s.pool64 + sg->quant_edges + sg->quant_edge_off[d], sg->quant_v[d], T + (int64_t)voff * K + k, K);
}

// What one workgroup of k_joint_quant_chunk / k_joint_mseg_quant_chunk works on:
// MixedIO (cand / inject rows are [Dc + Dk + Dq]) and the quantised part of ONE
// (id, group) problem.  Wave-uniform; arrays indexed by constants only.
template <int CP, int KP, int QP>
struct QuantIO {
  MixedIO<CP, (KP > 0 ? KP : 1)> m;
  int Dq, tile, stride, total;      // components per tile, floats per lattice value in the tile, sum V_d
  int V[QP], voff[QP], eoff[QP];
  float qlo[QP], qhi[QP];
  const double* edges;
  const float* qsamp;
  const float *bT, *aT;             // [total][K] of a side
};

// the longest tile (a multiple of 8 components, at most kTileK) whose table of
// `total` lattice values (and the zero row) fits kQTileBytes
__host__ __device__ __forceinline__ int quant_tile(int total) {
  int tile = 8;
  for (int tk = kTileK; tk >= 8; tk -= 8)
    if ((int64_t)(total + 1) * (tk + 4) * (int64_t)sizeof(float) <= kQTileBytes) { tile = tk; break; }
  return tile;
}

// score_side_mixed with QP quantised dimensions.  The side's table streams
// through the dynamic LDS tile qt, laid out [lattice value][component] with
// p.stride floats a value (p.tile + 4: consecutive values start 4 banks apart,
// and stride / 4 is odd, so 16 lanes with 16 consecutive values hit 16 different
// bank quads); row p.total is all zeros (padded slots).  A lane fetches four
// consecutive components of its own lattice value with one 16-byte read; qo is
// that value's row offset in floats.  Components are taken four at a time: the
// tile's tail is padded with c = -3e38 (such a term adds 2^-inf = 0).
template <int CP, int KP, int QP>
__device__ __forceinline__ void score_side_quant(const float* __restrict__ mu, const float* __restrict__ a,
                                                 const float* __restrict__ c, const float* __restrict__ cat,
                                                 const float* __restrict__ miss, const float* __restrict__ bonus,
                                                 const float* __restrict__ T, int K, const QuantIO<CP, KP, QP>& p,
                                                 const float (&z)[kR][CP + KP + QP], const int (&qo)[kR][QP],
                                                 float* __restrict__ rows, float* __restrict__ cl,
                                                 float* __restrict__ qt, double (&out)[kR]) {
  constexpr int S = 2 * CP + KP, KPa = KP > 0 ? KP : 1;
  const int Dc = p.m.q.D, Dk = p.m.Dk, tile = p.tile, stride = p.stride;
  float m[kR], s[kR], nb[kR][KPa];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    m[r] = -3.0e38f;
    s[r] = 0.f;
#pragma unroll
    for (int d = 0; d < KP; ++d)
      nb[r][d] = d < Dk ? -bonus[p.m.off[d] + cat_index(z[r][CP + d], p.m.U[d])] : 0.f;
  }
  for (int k0 = 0; k0 < K; k0 += tile) {
    const int nk = min(tile, K - k0), nk4 = (nk + 3) & ~3;
    __syncthreads();                       // the previous tile (or side) is read
    if constexpr (CP > 0)
      for (int e = threadIdx.x; e < nk4 * CP; e += kThreads) {
        const int kk = e / CP, d = e % CP;
        const bool in = d < Dc && kk < nk;   // padded dimensions and components: a = 0 adds nothing
        const int64_t src = (int64_t)(k0 + kk) * Dc + d;
        rows[kk * S + d] = in ? mu[src] : 0.f;
        rows[kk * S + CP + d] = in ? a[src] : 0.f;
      }
    if constexpr (KP > 0)
      for (int e = threadIdx.x; e < nk4 * KP; e += kThreads) {
        const int kk = e / KP, d = e % KP;   // padded: category -1 never matches
        rows[kk * S + 2 * CP + d] = (d < Dk && kk < nk) ? cat[(int64_t)(k0 + kk) * Dk + d] : -1.f;
      }
    for (int e = threadIdx.x; e < nk4; e += kThreads) cl[e] = e < nk ? c[k0 + e] : -3.0e38f;
    for (int e = threadIdx.x; e < p.total * tile; e += kThreads) {
      const int b = e / tile, kk = e - b * tile;         // a run over k of one lattice value: coalesced
      if (kk < nk4) qt[b * stride + kk] = kk < nk ? T[(int64_t)b * K + k0 + kk] : 0.f;
    }
    __syncthreads();
    for (int k4 = 0; k4 < nk4; k4 += 4) {
      float tq[kR][QP][4];
#pragma unroll
      for (int r = 0; r < kR; ++r)
#pragma unroll
        for (int d = 0; d < QP; ++d) {
          const float4 v = *reinterpret_cast<const float4*>(qt + qo[r][d] + k4);
          tq[r][d][0] = v.x; tq[r][d][1] = v.y; tq[r][d][2] = v.z; tq[r][d][3] = v.w;
        }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k4 + j;
        float rm[CP + 1], ra[CP + 1], rc[KPa];
        if constexpr (S > 0) {
          const float* row = rows + kk * S;
#pragma unroll
          for (int d = 0; d < CP; ++d) { rm[d] = row[d]; ra[d] = row[CP + d]; }
#pragma unroll
          for (int d = 0; d < KP; ++d) rc[d] = row[2 * CP + d];
        }
        const float ck = cl[kk];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
          float acc = 0.f;
#pragma unroll
          for (int d = 0; d < CP; ++d) {
            const float u = (z[r][d] - rm[d]) * ra[d];
            acc = __builtin_fmaf(u, u, acc);
          }
#pragma unroll
          for (int d = 0; d < KP; ++d) acc += z[r][CP + d] == rc[d] ? nb[r][d] : 0.f;
#pragma unroll
          for (int d = 0; d < QP; ++d) acc -= tq[r][d][j];
          const float t = ck - acc;
          const float dl = t - m[r];
          const float e2 = __builtin_amdgcn_exp2f(-__builtin_fabsf(dl));
          s[r] = dl > 0.f ? __builtin_fmaf(s[r], e2, 1.f) : s[r] + e2;
          m[r] = fmaxf(m[r], t);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    double M = 0.0;
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) M += (double)miss[p.m.off[d] + cat_index(z[r][CP + d], p.m.U[d])];
    out[r] = (double)m[r] + log2((double)s[r]) + M;
  }
}

// mixed_chunk_body for a group with quantised labels: CP / KP / QP the padded
// continuous / discrete / quantised counts (CP = 0, KP = 0 allowed).  z[r] holds
// the continuous coordinates at [0, CP), the categories at [CP, CP + KP) and the
// lattice indices at [CP + KP, CP + KP + QP).  qt: the dynamic LDS tile,
// [(total + 1) * stride].
template <int CP, int KP, int QP>
__device__ __forceinline__ void quant_chunk_body(const QuantIO<CP, KP, QP>& p, int first, float* __restrict__ rows,
                                                 float* __restrict__ cl, float* __restrict__ qt,
                                                 Pick* __restrict__ slot) {
  constexpr int ZP = CP + KP + QP;
  const ChunkIO& q = p.m.q;
  const int t = threadIdx.x, Dc = q.D, Dk = p.m.Dk, Dq = p.Dq, D = Dc + Dk + Dq;

  for (int e = t; e < p.stride; e += kThreads) qt[p.total * p.stride + e] = 0.f;   // the padded slots' row

  float z[kR][ZP];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
#pragma unroll
    for (int d = 0; d < ZP; ++d) z[r][d] = 0.f;
    const int i = first + r * kThreads + t;
    if (i >= q.C) continue;
    if (q.inject) {
#pragma unroll
      for (int d = 0; d < CP; ++d)
        if (d < Dc) z[r][d] = q.inj[(int64_t)i * D + d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) z[r][CP + d] = q.inj[(int64_t)i * D + Dc + d];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) z[r][CP + KP + d] = q.inj[(int64_t)i * D + Dc + Dk + d];
      continue;
    }
    const uint32_t c3 = q.c3, gi = q.base + (uint32_t)i;   // gi < 2^31: i < C and base + C <= n_cand_global
    U4 w = philox4x32_10(gi, 0u, q.stream_word, c3, q.key0, q.key1);
    const double us = u01w(w.x);
    int lo = 0, hi = q.kb - 1;             // first k with us < cum[k]
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (us < q.cum[mid]) hi = mid; else lo = mid + 1; }
    const int comp = lo;
    // One loop over the kernel coordinates, not unrolled, word 1 + j for
    // coordinate j; a continuous or discrete one is k_joint_mixed_chunk's draw,
    // operation for operation, and a quantised one the continuous draw binned.
    for (int j = 0; j < D; ++j) {
      const int wi = j + 1;
      if ((wi & 3) == 0) w = philox4x32_10(gi, (uint32_t)(wi >> 2), q.stream_word, c3, q.key0, q.key1);
      const uint32_t word = (wi & 3) == 0 ? w.x : (wi & 3) == 1 ? w.y : (wi & 3) == 2 ? w.z : w.w;
      float x;
      if (j < Dc || j >= Dc + Dk) {
        const bool quant = j >= Dc;
        const int d = quant ? j - Dc - Dk : j;
        const float* sr = quant ? p.qsamp + ((int64_t)comp * Dq + d) * 5 : q.samp + ((int64_t)comp * Dc + d) * 5;
        const float pr = sr[2] + u01f(word) * (sr[3] - sr[2]);
        float zz = ndtri_f32(pr);
        if (sr[4] != 0.f) zz = -zz;
        x = sr[0] + sr[1] * zz;
        if (!(x == x)) x = sr[0];
        float blo = 0.f, bhi = 0.f;                       // (the bound arrays: constant indices only)
        if (!quant) {
#pragma unroll
          for (int f = 0; f < CP; ++f)
            if (f == d) { blo = p.m.lo[f]; bhi = p.m.hi[f]; }
        } else {
#pragma unroll
          for (int f = 0; f < QP; ++f)
            if (f == d) { blo = p.qlo[f]; bhi = p.qhi[f]; }
        }
        x = fminf(fmaxf(x, blo), bhi);                    // low <= z < high
        if (quant) {
          int V = 2, eoff = 0;
#pragma unroll
          for (int f = 0; f < QP; ++f)
            if (f == d) { V = p.V[f]; eoff = p.eoff[f]; }
          const double* e = p.edges + eoff + 1;           // the interior edges e_1 .. e_{V-1}
          const double zd = (double)x;
          int a = 0, b = V - 1;                           // how many of them are <= z
          while (a < b) { const int mid = (a + b) >> 1; if (e[mid] <= zd) a = mid + 1; else b = mid; }
          x = (float)a;
        }
      } else {
        if constexpr (KP > 0) {
          const int d = j - Dc;
          const double u = u01w(word);
          x = p.m.bcat[(int64_t)comp * Dk + d];             // the component's category, -1: the prior row
          const double h = x >= 0.f ? p.m.bh[d] : 0.0;
          if (!(u < h)) {
            const double u2 = (u - h) / (1.0 - h);
            int off = 0, U = 1;
#pragma unroll
            for (int f = 0; f < KP; ++f)
              if (f == d) { off = p.m.off[f]; U = p.m.U[f]; }
            const double* cum = p.m.ccum + off;
            int a = 0, b = U - 1;                           // first category with u2 < cum[v]
            while (a < b) { const int mid = (a + b) >> 1; if (u2 < cum[mid]) b = mid; else a = mid + 1; }
            x = (float)a;
          }
        } else {
          x = 0.f;
        }
      }
      const int e = j < Dc ? j : j < Dc + Dk ? CP + (j - Dc) : CP + KP + (j - Dc - Dk);
#pragma unroll
      for (int f = 0; f < ZP; ++f)
        if (f == e) z[r][f] = x;
    }
  }

  // the lattice value's row in the tile (kept inside the table); a padded slot reads the zero row
  int qo[kR][QP];
#pragma unroll
  for (int r = 0; r < kR; ++r)
#pragma unroll
    for (int d = 0; d < QP; ++d)
      qo[r][d] = (d < Dq ? p.voff[d] + cat_index(z[r][CP + KP + d], p.V[d]) : p.total) * p.stride;

  double l2[kR], g2[kR];
  score_side_quant<CP, KP, QP>(q.bmu, q.ba, q.bc, p.m.bcat, p.m.bmiss, p.m.bbonus, p.bT, q.kb, p, z, qo, rows, cl, qt,
                               l2);
  score_side_quant<CP, KP, QP>(q.amu, q.aa, q.ac, p.m.acat, p.m.amiss, p.m.abonus, p.aT, q.ka, p, z, qo, rows, cl, qt,
                               g2);

  Pick best{0, 0};
  double lv[kR], gv[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = l2[r] * kLn2 + q.bbase;
    gv[r] = g2[r] * kLn2 + q.abase;
    if (i >= q.C) continue;
    if (q.l_out) q.l_out[i] = lv[r];
    if (q.g_out) q.g_out[i] = gv[r];
    if (q.cand) {
      float* row = q.cand + (int64_t)i * D;
#pragma unroll
      for (int d = 0; d < CP; ++d)
        if (d < Dc) row[d] = z[r][d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) row[Dc + d] = z[r][CP + d];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) row[Dc + Dk + d] = z[r][CP + KP + d];
    }
    const uint64_t key = score_key(lv[r] - gv[r]);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  Pick w = wave_best(best);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  w = slot[0];
#pragma unroll
  for (int s = 1; s < kThreads / 64; ++s)
    if (beats(slot[s], w)) w = slot[s];

  tpe_joint_record* rec = q.rec;
  if (w.key == 0) {
    if (t == 0) rec->global_idx = -1;
    return;
  }
  const int off = (int)(w.idx - first);
  if (t != off % kThreads) return;
  const int wr = off / kThreads;
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    if (r != wr) continue;
    rec->global_idx = w.idx + (int64_t)q.base;
    rec->l = lv[r];
    rec->g = gv[r];
    // kernel coordinate order: continuous, categories, lattice indices, then zeros
#pragma unroll
    for (int d = 0; d < TPE_JOINT_MAX_DIMS; ++d)
      if (d >= D) rec->z[d] = 0.0;
#pragma unroll
    for (int d = 0; d < CP; ++d)
      if (d < Dc) rec->z[d] = (double)z[r][d];
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) rec->z[Dc + d] = (double)z[r][CP + d];
#pragma unroll
    for (int d = 0; d < QP; ++d)
      if (d < Dq) rec->z[Dc + Dk + d] = (double)z[r][CP + KP + d];
  }
}

template <int CP, int KP, int QP>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, (CP + KP + QP >= 12 ? 2 : 8))))
void k_joint_quant_chunk(const QuantK p) {
  constexpr int S = 2 * CP + KP;
  __shared__ __attribute__((aligned(16))) float rows[kTileK * (S > 0 ? S : 1)];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  extern __shared__ __attribute__((aligned(16))) float qt[];     // [(total + 1) * stride]
  const JointK& j = p.m.j;
  QuantIO<CP, KP, QP> io;
  solo_chunk_io(io.m.q, j, j.D + p.m.Dk + p.Dq);
  io.m.Dk = p.m.Dk;
#pragma unroll
  for (int d = 0; d < CP; ++d) { io.m.lo[d] = j.lo[d]; io.m.hi[d] = j.hi[d]; }   // (kernel-argument arrays: constant indices only)
#pragma unroll
  for (int d = 0; d < KP; ++d) { io.m.U[d] = p.m.U[d]; io.m.off[d] = p.m.off[d]; }
  io.m.bcat = p.m.bcat; io.m.acat = p.m.acat;
  io.m.bmiss = p.m.bmiss; io.m.bbonus = p.m.bbonus; io.m.amiss = p.m.amiss; io.m.abonus = p.m.abonus;
  io.m.bh = p.m.bh; io.m.ccum = p.m.ccum;
  io.Dq = p.Dq; io.tile = p.tile; io.stride = p.stride; io.total = p.total;
#pragma unroll
  for (int d = 0; d < QP; ++d) {
    io.V[d] = p.V[d]; io.voff[d] = p.voff[d]; io.eoff[d] = p.eoff[d];
    io.qlo[d] = p.qlo[d]; io.qhi[d] = p.qhi[d];
  }
  io.edges = p.edges; io.qsamp = p.qsamp; io.bT = p.bT; io.aT = p.aT;
  quant_chunk_body<CP, KP, QP>(io, (int)(blockIdx.x % j.n_chunks) * TPE_JOINT_CHUNK, rows, cl, qt, slot);
}

template <int CP, int KP, int QP>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, (CP + KP + QP >= 12 ? 2 : 8))))
void k_joint_mseg_quant_chunk(const MSegK p) {
  static_assert(KP <= TPE_JOINT_MSEG_MAX_CAT && CP <= TPE_JOINT_MSEG_MAX_CONT && QP <= TPE_JOINT_MAX_QUANT,
                "the descriptor's arrays");
  constexpr int S = 2 * CP + KP;
  __shared__ __attribute__((aligned(16))) float rows[kTileK * (S > 0 ? S : 1)];
  __shared__ float cl[kTileK];
  __shared__ Pick slot[kThreads / 64];
  extern __shared__ __attribute__((aligned(16))) float qt[];     // at least [(total + 1) * stride] of this segment
  const int chunk = blockIdx.x % p.s.n_chunks;
  const int prob = uni(p.s.order[p.s.first + blockIdx.x / p.s.n_chunks]);
  const tpe_joint_mseg* __restrict__ sg = mseg_at(p.s, uni(p.s.prob_seg[prob]));
  QuantIO<CP, KP, QP> io;
  mseg_chunk_io(io.m.q, p.s, sg, prob, chunk);
  if constexpr (KP > 0) {
    mseg_mixed_io<CP, KP>(io.m, p.s, sg);
  } else {
    io.m.Dk = 0;
#pragma unroll
    for (int d = 0; d < CP; ++d) { io.m.lo[d] = unif(sg->lo[d]); io.m.hi[d] = unif(sg->hi[d]); }
    io.m.U[0] = 1; io.m.off[0] = 0;
    io.m.bcat = io.m.acat = io.m.bmiss = io.m.bbonus = io.m.amiss = io.m.abonus = nullptr;
    io.m.bh = io.m.ccum = nullptr;
  }
  io.Dq = uni(sg->n_quant);
  int total = 0;
#pragma unroll
  for (int d = 0; d < QP; ++d) {
    const bool in = d < io.Dq;                // padded slots: as tpe_joint_quant_run fills them
    io.V[d] = in ? uni(sg->quant_v[d]) : 2;
    io.voff[d] = in ? total : 0;
    io.eoff[d] = in ? uni(sg->quant_edge_off[d]) : 0;
    io.qlo[d] = in ? unif(sg->qlo[d]) : -INFINITY;
    io.qhi[d] = in ? unif(sg->qhi[d]) : INFINITY;
    total += in ? io.V[d] : 0;
  }
  io.total = total;
  io.tile = quant_tile(total); io.stride = io.tile + 4;     // the solo run's tiling of this segment
  io.edges = p.s.pool64 + uni(sg->quant_edges);
  io.qsamp = p.s.inject ? nullptr : p.s.pool + uni(sg->quant_samp);
  io.bT = p.table + uni(sg->table);
  io.aT = io.bT + (int64_t)total * io.m.q.kb;
  quant_chunk_body<CP, KP, QP>(io, chunk * TPE_JOINT_CHUNK, rows, cl, qt, slot);
}


// -------------------------------------------------------------- wide groups
// 17 to TPE_JOINT_WIDE_MAX_DIMS coordinates (include/tpe_hip.h "Wide joint
// stage", "Wide mixed joint stage", "Wide quantised joint stage"): Dc continuous
// ones, then Dk <= TPE_JOINT_WIDE_MAX_CAT discrete and Dq <= TPE_JOINT_MAX_QUANT
// quantised ones -- the models, tables (k_joint_qtable) and draws of the narrow
// stages.  A lane cannot hold 4 x 64 coordinates, and 64 inlined copies of the
// sampler cannot be unrolled, so the work is split:
// k_joint_wide_sample / _mixed_sample / _quant_sample  one thread per (id,
//                candidate): k_joint_chunk's / k_joint_mixed_chunk's /
//                k_joint_quant_chunk's draw, word for word (word 1 + j serves
//                kernel coordinate j), in loops that are not unrolled.  Block b
//                of an id (256 consecutive candidates) writes zbuf[(id * nblk +
//                b)][D][256], D = Dc + Dk + Dq: thread t stores at d * 256 + t, a
//                coalesced store.  A category and a lattice index are f32.
// k_joint_wide_chunk<DP, R>  one workgroup per (id, chunk of 256 R candidates):
//                loads R candidates' z[DP] per lane from zbuf (coalesced) or
//                from `inject`, every index a compile-time constant, and scores
//                them as k_joint_chunk does.  A tile row is read four dimensions
//                at a time (16-byte broadcast reads of mu and a).
// k_joint_wide_mixed_chunk<DP, KP, R>  the same with KP category slots a
//                candidate: the component tile also holds cat[KP], a discrete
//                slot costs one compare, one select and one add per (candidate,
//                component), and sum_d miss_d(v_d) is added in f64 at the end.
// k_joint_wide_quant_chunk<DP, KP, QP, R>  the same with QP lattice slots a
//                candidate (KP = 0: no discrete slot).  The side's table streams
//                through a dynamic LDS tile beside the rows, laid out [lattice
//                value][component] as in k_joint_quant_chunk (stride tile + 4: 16
//                lanes with 16 consecutive values read 16 different bank quads);
//                rows and table share ONE tile length, the longest that keeps the
//                table tile inside kWQTileBytes (and at most wide_tile(DP)).
//                Components are taken four at a time (one 16-byte table read per
//                candidate and quantised slot); the tile's tail is padded with
//                c = -3e38.
// k_joint_wide_merge  k_joint_merge on the wide record; it serves all three.
// The kernels are their arguments, their LDS and calls into the parts below;
// each part exists once.  A count of 0 slots (KP, QP) means "none": arrays of a
// slot kind then have one unused entry (slots()).
constexpr int kWD = TPE_JOINT_WIDE_MAX_DIMS;
constexpr int kWK = TPE_JOINT_WIDE_MAX_CAT;
constexpr int kWQ = TPE_JOINT_MAX_QUANT;
static_assert(sizeof(tpe_joint_wide_record) == 24 + 8 * kWD, "layout");

// components per LDS tile: at most 32 KiB of rows, so four workgroups fit a CU's 160 KiB
constexpr int wide_tile(int DP) { return DP <= 32 ? 128 : ((4096 / DP) & ~7); }
constexpr int wide_r(int DP) { return DP <= 32 ? 2 : 1; }
constexpr int slots(int P) { return P > 0 ? P : 1; }

// rows (<= 32 KiB) + cats (<= 4 KiB) + c + the quantised stage's table tile stay
// under 64 KiB: no launch attribute is needed, and two workgroups fit a CU's 160 KiB.
constexpr int kWQTileBytes = 26 * 1024;

// the common tile length of a group with `total` lattice values: a multiple of 8
// components, at most tk; 8 at the least ((512 + 1) * 12 * 4 B = 24 KiB fits)
__host__ __device__ __forceinline__ int wide_quant_tile(int total, int tk) {
  int tile = 8;
  for (int t = tk; t >= 8; t -= 8)
    if ((int64_t)(total + 1) * (t + 4) * (int64_t)sizeof(float) <= kWQTileBytes) { tile = t; break; }
  return tile;
}
static_assert((int64_t)(TPE_JOINT_MAX_LATTICE_TOTAL + 1) * 12 * sizeof(float) <= kWQTileBytes, "the shortest tile fits");

// the workgroup's best of every lane's pick: the waves' winners meet in slot[4]
__device__ __forceinline__ Pick block_best(Pick best, Pick* __restrict__ slot) {
  const int t = threadIdx.x;
  Pick w = wave_best(best);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  w = slot[0];
#pragma unroll
  for (int q = 1; q < kThreads / 64; ++q)
    if (beats(slot[q], w)) w = slot[q];
  return w;
}

// ---- the steps the wide samplers and scoring loops are made of (the narrow
// stages above carry the same steps written out: their code generation is pinned)
// One candidate's Philox stream: block b of it holds the words 4 b .. 4 b + 3.
struct Stream {
  uint32_t gi, stream_word, c3, key0, key1;   // gi: the candidate's global index; c3: the new id's low word
};
__device__ __forceinline__ U4 stream_block(const Stream& q, uint32_t b) {
  return philox4x32_10(q.gi, b, q.stream_word, q.c3, q.key0, q.key1);
}
// Word 0 picks the candidate's component of the below mixture: w becomes block
// 0 of the stream, the result is the first k with us < cum[k].
__device__ __forceinline__ int draw_component(const Stream& q, U4& w, const double* cum, int kb) {
  w = stream_block(q, 0u);
  const double us = u01w(w.x);
  int lo = 0, hi = kb - 1;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (us < cum[mid]) hi = mid; else lo = mid + 1; }
  return lo;
}
// Word 1 + j serves kernel coordinate j (w: the block drawn last; the
// coordinates are visited in ascending order).
__device__ __forceinline__ uint32_t coord_word(const Stream& q, U4& w, int j) {
  const int wi = j + 1;
  if ((wi & 3) == 0) w = stream_block(q, (uint32_t)(wi >> 2));
  return (wi & 3) == 0 ? w.x : (wi & 3) == 1 ? w.y : (wi & 3) == 2 ? w.z : w.w;
}
// One continuous coordinate from its 5-float sampler row (mu, sigma, the two
// ends of the truncated uniform, the tail's sign), kept in [lo, hi]: low <= z < high.
__device__ __forceinline__ float draw_continuous(const float* sr, uint32_t word, float lo, float hi) {
  const float pr = sr[2] + u01f(word) * (sr[3] - sr[2]);
  float zz = ndtri_f32(pr);
  if (sr[4] != 0.f) zz = -zz;
  float x = sr[0] + sr[1] * zz;
  if (!(x == x)) x = sr[0];
  return fminf(fmaxf(x, lo), hi);
}
// The lattice index of a drawn quantised coordinate: how many of the interior
// edges e_1 .. e_{V-1} (e points at e_1) are <= z.
__device__ __forceinline__ int lattice_index(const double* e, int V, float z) {
  const double zd = (double)z;
  int a = 0, b = V - 1;
  while (a < b) { const int mid = (a + b) >> 1; if (e[mid] <= zd) a = mid + 1; else b = mid; }
  return a;
}
// One component's term t joins the running sum: s accumulates 2^(term - m) with
// m the running maximum of the terms (one v_exp_f32).
__device__ __forceinline__ void lse_step(float t, float& m, float& s) {
  const float dl = t - m;
  const float e2 = __builtin_amdgcn_exp2f(-__builtin_fabsf(dl));
  s = dl > 0.f ? __builtin_fmaf(s, e2, 1.f) : s + e2;
  m = fmaxf(m, t);
}
// ... and log2 of the sum when the side is through
__device__ __forceinline__ double lse_log2(float m, float s) { return (double)m + log2((double)s); }

// The kernels' arguments: a stage's struct begins with the one of the stage it extends.
struct WideSampK {
  int D, C, nblk, kb;               // D = Dc; a block of zbuf is [Dc + Dk + Dq][256]
  uint32_t key0, key1, stream_word;
  uint32_t cand_base;               // as JointK: the Philox word
  const double* cum;
  const float* samp;
  const int64_t* ids;
  float* zbuf;
  float lo[kWD], hi[kWD];
};
struct WideMixedSampK : WideSampK {
  int Dk;
  int U[kWK], off[kWK];
  const float* bcat;
  const double* bh;
  const double* ccum;
};
struct WideQuantSampK : WideMixedSampK {
  int Dq;
  int V[kWQ], eoff[kWQ];
  float qlo[kWQ], qhi[kWQ];
  const double* edges;
  const float* qsamp;
};

struct WideK {
  int D, C, n_chunks, nblk, inject; // D = Dc; zsrc / cand rows are [Dc + Dk + Dq]
  int kb, ka;
  uint32_t cand_base;               // as JointK: the record index only (the draws are the sampling kernel's)
  const float *bmu, *ba, *bc, *amu, *aa, *ac;
  double bbase, abase;
  const float* zsrc;                // inject: [C][D]; else zbuf [n_ids * nblk][D][256]
  float* cand;
  double *l_out, *g_out;
  tpe_joint_wide_record* chunk_rec; // scratch [n_ids * n_chunks]
};
struct WideMixedK : WideK {
  int Dk;
  int U[kWK], off[kWK];
  const float *bcat, *acat;
  const float *bmiss, *bbonus, *amiss, *abonus;
};
struct WideQuantK : WideMixedK {
  int Dq, tile, stride, total;      // components per tile, floats per lattice value in the tile, sum V_d
  int V[kWQ], voff[kWQ];
  const float *bT, *aT;             // [total][K] of a side
};

// ---- the samplers' parts.  Arguments that a loop indexes at run time are
// staged in LDS by thread 0 (kernel-argument arrays: constant indices only).
template <typename T, int N>
__device__ __forceinline__ void stage(T (&lds)[N], const T (&arg)[N]) {
#pragma unroll
  for (int f = 0; f < N; ++f) lds[f] = arg[f];
}

// a sampler thread's candidate: its stream, its component, its column of zbuf
struct WideDraw {
  Stream st;
  U4 w;
  int comp;
  float* out;                       // coordinate j goes to out[j * 256]
};
// Which of a scoring launch's problems a workgroup serves.  id indexes the
// view's zsrc blocks, cand and l_out / g_out; chunk is the chunk of that id; slot
// is the workgroup's place in chunk_rec.  The solo kernels: id * n_chunks + chunk
// = slot = blockIdx.x.
struct WideAt {
  int id, chunk;
  int64_t slot;
};
__device__ __forceinline__ WideAt wide_at(int per_id) {
  return WideAt{(int)(blockIdx.x / per_id), (int)(blockIdx.x % per_id), (int64_t)blockIdx.x};
}

// candidate i of the view's id `id`: its stream and its component
__device__ __forceinline__ void wide_sample_stream(const WideSampK& p, int i, int id, WideDraw& c) {
  c.st = Stream{p.cand_base + (uint32_t)i, p.stream_word, (uint32_t)p.ids[id], p.key0, p.key1};   // gi < 2^31 (i < C)
  c.comp = draw_component(c.st, c.w, p.cum, p.kb);
}
// false: the thread is past the last candidate.  D: all the group's coordinates.
__device__ __forceinline__ bool wide_sample_head(const WideSampK& p, int D, WideDraw& c) {
  const int t = threadIdx.x;
  const int id = blockIdx.x / p.nblk, blk = blockIdx.x % p.nblk;
  const int i = blk * kThreads + t;
  if (i >= p.C) return false;
  c.out = p.zbuf + (int64_t)blockIdx.x * kThreads * D + t;
  wide_sample_stream(p, i, id, c);
  return true;
}
// the Dc continuous coordinates: k_joint_chunk's draw, operation for operation
__device__ __forceinline__ void wide_sample_continuous(const WideSampK& p, WideDraw& c, const float* blo,
                                                       const float* bhi) {
  const int Dc = p.D;
  const float* srow = p.samp + (int64_t)c.comp * Dc * 5;
#pragma unroll 1
  for (int d = 0; d < Dc; ++d) {
    const uint32_t word = coord_word(c.st, c.w, d);
    c.out[(int64_t)d * kThreads] = draw_continuous(srow + d * 5, word, blo[d], bhi[d]);
  }
}
// the Dk categories as k_joint_mixed_chunk's sampler draws them: the category index as an f32
__device__ __forceinline__ void wide_sample_categories(const WideMixedSampK& p, WideDraw& c, const int* cU,
                                                       const int* coff) {
  const int Dc = p.D, Dk = p.Dk;
#pragma unroll 1
  for (int d = 0; d < Dk; ++d) {
    const double u = u01w(coord_word(c.st, c.w, Dc + d));
    float x = p.bcat[(int64_t)c.comp * Dk + d];           // the component's category, -1: the prior row
    const double h = x >= 0.f ? p.bh[d] : 0.0;
    if (!(u < h)) {
      const double u2 = (u - h) / (1.0 - h);
      const double* cum = p.ccum + coff[d];
      int a = 0, b = cU[d] - 1;                           // first category with u2 < cum[v]
      while (a < b) { const int mid = (a + b) >> 1; if (u2 < cum[mid]) b = mid; else a = mid + 1; }
      x = (float)a;
    }
    c.out[(int64_t)(Dc + d) * kThreads] = x;
  }
}
// the Dq lattice indices as k_joint_quant_chunk's sampler draws them: the continuous
// draw through the dimension's sampler row, binned; the lattice index as an f32
__device__ __forceinline__ void wide_sample_lattice(const WideQuantSampK& p, WideDraw& c, const int* qV,
                                                    const int* qeoff, const float* qlo, const float* qhi) {
  const int Dq = p.Dq, first = p.D + p.Dk;
#pragma unroll 1
  for (int d = 0; d < Dq; ++d) {
    const uint32_t word = coord_word(c.st, c.w, first + d);
    const float x = draw_continuous(p.qsamp + ((int64_t)c.comp * Dq + d) * 5, word, qlo[d], qhi[d]);
    c.out[(int64_t)(first + d) * kThreads] = (float)lattice_index(p.edges + qeoff[d] + 1, qV[d], x);
  }
}

__global__ __launch_bounds__(kThreads) void k_joint_wide_sample(const WideSampK p) {
  __shared__ float blo[kWD], bhi[kWD];
  if (threadIdx.x == 0) { stage(blo, p.lo); stage(bhi, p.hi); }
  __syncthreads();
  WideDraw c;
  if (!wide_sample_head(p, p.D, c)) return;
  wide_sample_continuous(p, c, blo, bhi);
}

__global__ __launch_bounds__(kThreads) void k_joint_wide_mixed_sample(const WideMixedSampK p) {
  __shared__ float blo[kWD], bhi[kWD];
  __shared__ int cU[kWK], coff[kWK];
  if (threadIdx.x == 0) {
    stage(blo, p.lo); stage(bhi, p.hi);
    stage(cU, p.U); stage(coff, p.off);
  }
  __syncthreads();
  WideDraw c;
  if (!wide_sample_head(p, p.D + p.Dk, c)) return;
  wide_sample_continuous(p, c, blo, bhi);
  wide_sample_categories(p, c, cU, coff);
}

__global__ __launch_bounds__(kThreads) void k_joint_wide_quant_sample(const WideQuantSampK p) {
  __shared__ float blo[kWD], bhi[kWD];
  __shared__ int cU[kWK], coff[kWK];
  __shared__ int qV[kWQ], qeoff[kWQ];
  __shared__ float qlo[kWQ], qhi[kWQ];
  if (threadIdx.x == 0) {
    stage(blo, p.lo); stage(bhi, p.hi);
    stage(cU, p.U); stage(coff, p.off);
    stage(qV, p.V); stage(qeoff, p.eoff); stage(qlo, p.qlo); stage(qhi, p.qhi);
  }
  __syncthreads();
  WideDraw c;
  if (!wide_sample_head(p, p.D + p.Dk + p.Dq, c)) return;
  wide_sample_continuous(p, c, blo, bhi);
  wide_sample_categories(p, c, cU, coff);
  wide_sample_lattice(p, c, qV, qeoff, qlo, qhi);
}

// ---- the scoring kernels' parts
// A lane's R candidates: continuous coordinates, categories, lattice indices.
template <int DP, int KP, int QP, int R>
struct WideCand {
  float z[R][DP], v[R][slots(KP)], x[R][slots(QP)];
};

// Zero, then the candidates first + r * 256 + t of this workgroup's id from
// `inject` rows or from zbuf; every register index is a compile-time constant.
template <int DP, int KP, int QP, int R>
__device__ __forceinline__ void wide_load(const WideK& p, const WideAt& at, int Dk, int Dq,
                                          WideCand<DP, KP, QP, R>& c) {
  const int t = threadIdx.x, Dc = p.D, D = Dc + Dk + Dq;
  const int id = at.id, chunk = at.chunk;
  const int first = chunk * (R * kThreads);
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int d = 0; d < DP; ++d) c.z[r][d] = 0.f;
#pragma unroll
    for (int d = 0; d < slots(KP); ++d) c.v[r][d] = 0.f;
#pragma unroll
    for (int d = 0; d < slots(QP); ++d) c.x[r][d] = 0.f;
    const int i = first + r * kThreads + t;
    if (i >= p.C) continue;
    if (p.inject) {
      const float* src = p.zsrc + (int64_t)i * D;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) c.z[r][d] = src[d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) c.v[r][d] = src[Dc + d];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) c.x[r][d] = src[Dc + Dk + d];
    } else {
      // block chunk * R + r of this id (i < C: the block exists)
      const float* src = p.zsrc + ((int64_t)id * p.nblk + chunk * R + r) * kThreads * D + t;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) c.z[r][d] = src[(int64_t)d * kThreads];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) c.v[r][d] = src[(int64_t)(Dc + d) * kThreads];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) c.x[r][d] = src[(int64_t)(Dc + Dk + d) * kThreads];
    }
  }
}

// The components [k0, k0 + nk) of a side into the tile: rows, cats (KP > 0) and
// cl.  PAD4 (the quantised stage, which takes components four at a time): the
// tile is filled up to a multiple of 4 with components that add nothing.
template <int DP, int KP, bool PAD4>
__device__ __forceinline__ void wide_fill_tile(const float* __restrict__ mu, const float* __restrict__ a,
                                               const float* __restrict__ c, const float* __restrict__ cat, int k0,
                                               int nk, int Dc, int Dk, float* __restrict__ rows,
                                               float* __restrict__ cats, float* __restrict__ cl) {
  const int nkp = PAD4 ? (nk + 3) & ~3 : nk;
  for (int e = threadIdx.x; e < nkp * DP; e += kThreads) {
    const int kk = e / DP, d = e % DP;
    const bool in = d < Dc && (!PAD4 || kk < nk);   // padded dimensions (and components): a = 0 adds nothing
    const int64_t src = (int64_t)(k0 + kk) * Dc + d;
    rows[kk * 2 * DP + d] = in ? mu[src] : 0.f;
    rows[kk * 2 * DP + DP + d] = in ? a[src] : 0.f;
  }
  if constexpr (KP > 0)
    for (int e = threadIdx.x; e < nkp * KP; e += kThreads) {
      const int kk = e / KP, d = e % KP;     // padded slots: category -1 never matches
      cats[e] = (d < Dk && (!PAD4 || kk < nk)) ? cat[(int64_t)(k0 + kk) * Dk + d] : -1.f;
    }
  for (int e = threadIdx.x; e < nkp; e += kThreads) cl[e] = (!PAD4 || e < nk) ? c[k0 + e] : -3.0e38f;
}

// acc[r] = sum_d ((z_d - mu_d) a_d)^2 of tile row kk, read four dimensions at a
// time: every lane reads the same 16 bytes, a broadcast
template <int DP, int R>
__device__ __forceinline__ void wide_row_product(const float* __restrict__ rows, int kk, const float (&z)[R][DP],
                                                 float (&acc)[R]) {
  const float4* row = reinterpret_cast<const float4*>(rows + kk * 2 * DP);
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    const float4 rm = row[q], ra = row[DP / 4 + q];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float u = (z[r][4 * q] - rm.x) * ra.x;
      acc[r] = __builtin_fmaf(u, u, acc[r]);
      u = (z[r][4 * q + 1] - rm.y) * ra.y;
      acc[r] = __builtin_fmaf(u, u, acc[r]);
      u = (z[r][4 * q + 2] - rm.z) * ra.z;
      acc[r] = __builtin_fmaf(u, u, acc[r]);
      u = (z[r][4 * q + 3] - rm.w) * ra.w;
      acc[r] = __builtin_fmaf(u, u, acc[r]);
    }
  }
}

// The category terms (score_side_mixed's discrete part): component kk's categories,
// as 16-byte broadcasts where KP allows.
template <int KP>
__device__ __forceinline__ void wide_cat_row(const float* __restrict__ cats, int kk, float (&rc)[slots(KP)]) {
  if constexpr (KP > 0 && KP % 4 == 0) {
    const float4* cr = reinterpret_cast<const float4*>(cats + kk * KP);
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) {
      const float4 x = cr[q];
      rc[4 * q] = x.x; rc[4 * q + 1] = x.y; rc[4 * q + 2] = x.z; rc[4 * q + 3] = x.w;
    }
  } else if constexpr (KP == 2) {
    const float2 x = *reinterpret_cast<const float2*>(cats + kk * 2);
    rc[0] = x.x; rc[1] = x.y;
  } else if constexpr (KP == 1) {
    rc[0] = cats[kk];
  }
}
// (nb = -bonus_d(v_d), read once per candidate, the compare-add and the f64 sum of
// miss_d(v_d) are a short loop each in the two score sides: as functions they
// cost four quantised instantiations a wave of occupancy.)

// score_side for R candidates a lane and KP category slots (0: none; cat, miss,
// bonus and cats are not read): log2 of one side's mixture, + sum_d miss_d(v_d).
template <int DP, int KP, int R>
__device__ __forceinline__ void score_side_wide(const float* __restrict__ mu, const float* __restrict__ a,
                                                const float* __restrict__ c, const float* __restrict__ cat,
                                                const float* __restrict__ miss, const float* __restrict__ bonus,
                                                int K, int Dc, int Dk, const int (&U)[slots(KP)],
                                                const int (&off)[slots(KP)], const float (&z)[R][DP],
                                                const float (&v)[R][slots(KP)], float* __restrict__ rows,
                                                float* __restrict__ cats, float* __restrict__ cl, double (&out)[R]) {
  constexpr int TK = wide_tile(DP);
  float m[R], s[R], nb[R][slots(KP)];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -3.0e38f;
    s[r] = 0.f;
#pragma unroll
    for (int d = 0; d < KP; ++d) nb[r][d] = d < Dk ? -bonus[off[d] + cat_index(v[r][d], U[d])] : 0.f;
  }
  for (int k0 = 0; k0 < K; k0 += TK) {
    const int nk = min(TK, K - k0);
    __syncthreads();                       // the previous tile (or side) is read
    wide_fill_tile<DP, KP, false>(mu, a, c, cat, k0, nk, Dc, Dk, rows, cats, cl);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      float acc[R], rc[slots(KP)];
      wide_row_product<DP, R>(rows, kk, z, acc);
      wide_cat_row<KP>(cats, kk, rc);
      const float ck = cl[kk];
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int d = 0; d < KP; ++d) acc[r] += v[r][d] == rc[d] ? nb[r][d] : 0.f;   // one compare, one select, one add
        lse_step(ck - acc[r], m[r], s[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    out[r] = lse_log2(m[r], s[r]);
    if constexpr (KP > 0) {
      double M = 0.0;
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) M += (double)miss[off[d] + cat_index(v[r][d], U[d])];
      out[r] += M;
    }
  }
}

// score_side_wide with QP quantised slots (score_side_quant's table part).  qo: a
// candidate's table row offsets in floats.  Its own component loop: four at a
// time, the table tile in dynamic LDS.
template <int DP, int KP, int QP, int R>
__device__ __forceinline__ void score_side_wide_quant(const float* __restrict__ mu, const float* __restrict__ a,
                                                      const float* __restrict__ c, const float* __restrict__ cat,
                                                      const float* __restrict__ miss, const float* __restrict__ bonus,
                                                      const float* __restrict__ T, int K, int Dc, int Dk, int tile,
                                                      int stride, int total, const int (&U)[slots(KP)],
                                                      const int (&off)[slots(KP)], const float (&z)[R][DP],
                                                      const float (&v)[R][slots(KP)], const int (&qo)[R][QP],
                                                      float* __restrict__ rows, float* __restrict__ cats,
                                                      float* __restrict__ cl, float* __restrict__ qt,
                                                      double (&out)[R]) {
  float m[R], s[R], nb[R][slots(KP)];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -3.0e38f;
    s[r] = 0.f;
#pragma unroll
    for (int d = 0; d < KP; ++d) nb[r][d] = d < Dk ? -bonus[off[d] + cat_index(v[r][d], U[d])] : 0.f;
  }
  for (int k0 = 0; k0 < K; k0 += tile) {
    const int nk = min(tile, K - k0), nk4 = (nk + 3) & ~3;
    __syncthreads();                       // the previous tile (or side) is read
    wide_fill_tile<DP, KP, true>(mu, a, c, cat, k0, nk, Dc, Dk, rows, cats, cl);
    for (int e = threadIdx.x; e < total * tile; e += kThreads) {
      const int b = e / tile, kk = e - b * tile;           // a run over k of one lattice value: coalesced
      if (kk < nk4) qt[b * stride + kk] = kk < nk ? T[(int64_t)b * K + k0 + kk] : 0.f;
    }
    __syncthreads();
    for (int k4 = 0; k4 < nk4; k4 += 4) {
      float tq[R][QP][4];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int d = 0; d < QP; ++d) {
          const float4 x = *reinterpret_cast<const float4*>(qt + qo[r][d] + k4);
          tq[r][d][0] = x.x; tq[r][d][1] = x.y; tq[r][d][2] = x.z; tq[r][d][3] = x.w;
        }
      // (R = 1, the widths above 32: the four components are a loop, not four copies,
      // which would hold their 4 x 2 DP row values at once and leave one wave a SIMD)
#pragma unroll(R == 1 ? 1 : 4)
      for (int j = 0; j < 4; ++j) {
        const int kk = k4 + j;
        float acc[R], rc[slots(KP)];
        wide_row_product<DP, R>(rows, kk, z, acc);
        wide_cat_row<KP>(cats, kk, rc);
        const float ck = cl[kk];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int d = 0; d < KP; ++d) acc[r] += v[r][d] == rc[d] ? nb[r][d] : 0.f;
#pragma unroll
          for (int d = 0; d < QP; ++d)   // (selects, not an indexed read: tq stays in registers in the looped form)
            acc[r] -= j == 0 ? tq[r][d][0] : j == 1 ? tq[r][d][1] : j == 2 ? tq[r][d][2] : tq[r][d][3];
          lse_step(ck - acc[r], m[r], s[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    double M = 0.0;
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) M += (double)miss[off[d] + cat_index(v[r][d], U[d])];
    out[r] = lse_log2(m[r], s[r]) + M;
  }
}

// What every scoring kernel ends with: l and g of the lane's candidates, the
// optional outputs, the chunk's winner (the first of a tie) and its record.  The
// coordinate order in cand and in the record's z: continuous, categories,
// lattice indices, then zeros.
template <int DP, int KP, int QP, int R>
__device__ __forceinline__ void wide_finish(const WideK& p, const WideAt& at, int Dk, int Dq,
                                            const WideCand<DP, KP, QP, R>& c, const double (&l2)[R],
                                            const double (&g2)[R], Pick* __restrict__ slot) {
  const int t = threadIdx.x, Dc = p.D, D = Dc + Dk + Dq;
  const int id = at.id, chunk = at.chunk;
  const int first = chunk * (R * kThreads);

  Pick best{0, 0};
  double lv[R], gv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = l2[r] * kLn2 + p.bbase;
    gv[r] = g2[r] * kLn2 + p.abase;
    if (i >= p.C) continue;
    const int64_t o = (int64_t)id * p.C + i;
    if (p.l_out) p.l_out[o] = lv[r];
    if (p.g_out) p.g_out[o] = gv[r];
    if (p.cand) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) p.cand[o * D + d] = c.z[r][d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) p.cand[o * D + Dc + d] = c.v[r][d];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) p.cand[o * D + Dc + Dk + d] = c.x[r][d];
    }
    const uint64_t key = score_key(lv[r] - gv[r]);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  const Pick w = block_best(best, slot);

  tpe_joint_wide_record* rec = p.chunk_rec + at.slot;
  if (w.key == 0) {
    if (t == 0) rec->global_idx = -1;
    return;
  }
  const int woff = (int)(w.idx - first);
  if (t != woff % kThreads) return;
  const int wr = woff / kThreads;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r != wr) continue;
    rec->global_idx = w.idx + (int64_t)p.cand_base;
    rec->l = lv[r];
    rec->g = gv[r];
    if constexpr (KP == 0 && QP == 0) {     // continuous alone: the padded slots hold zeros, no compare against D
#pragma unroll
      for (int d = 0; d < kWD; ++d) rec->z[d] = d < DP ? (double)c.z[r][d < DP ? d : 0] : 0.0;
    } else {
#pragma unroll
      for (int d = 0; d < kWD; ++d)
        if (d >= D) rec->z[d] = 0.0;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) rec->z[d] = (double)c.z[r][d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) rec->z[Dc + d] = (double)c.v[r][d];
#pragma unroll
      for (int d = 0; d < QP; ++d)
        if (d < Dq) rec->z[Dc + Dk + d] = (double)c.x[r][d];
    }
  }
}

template <int DP, int R>
__global__ __launch_bounds__(kThreads) void k_joint_wide_chunk(const WideK p) {
  static_assert(DP % 4 == 0 && DP <= kWD, "rows are read as float4");
  constexpr int TK = wide_tile(DP);
  __shared__ __attribute__((aligned(16))) float rows[TK * 2 * DP];
  __shared__ float cl[TK];
  __shared__ Pick slot[kThreads / 64];
  const int none[1] = {0};

  WideCand<DP, 0, 0, R> c;
  wide_load(p, wide_at(p.n_chunks), 0, 0, c);
  double l2[R], g2[R];
  score_side_wide<DP, 0, R>(p.bmu, p.ba, p.bc, nullptr, nullptr, nullptr, p.kb, p.D, 0, none, none, c.z, c.v, rows,
                            nullptr, cl, l2);
  score_side_wide<DP, 0, R>(p.amu, p.aa, p.ac, nullptr, nullptr, nullptr, p.ka, p.D, 0, none, none, c.z, c.v, rows,
                            nullptr, cl, g2);
  wide_finish(p, wide_at(p.n_chunks), 0, 0, c, l2, g2, slot);
}

// (This kernel carries wide_load and wide_finish written out, KP slots and no
// lattice slot: through the shared functions <20, 2, 2> needs 130 VGPRs for 124
// and drops from 4 waves a SIMD to 3.  A change to either part is made here too.)
template <int DP, int KP, int R>
__global__ __launch_bounds__(kThreads) void k_joint_wide_mixed_chunk(const WideMixedK p) {
  static_assert(DP % 4 == 0 && DP <= kWD && KP <= kWK, "rows are read as float4; the argument arrays");
  constexpr int TK = wide_tile(DP);
  // at most 128 * (64 + 8) * 4 B = 36 KiB of tile: four workgroups fit a CU's 160 KiB
  __shared__ __attribute__((aligned(16))) float rows[TK * 2 * DP];
  __shared__ __attribute__((aligned(16))) float cats[TK * KP];
  __shared__ float cl[TK];
  __shared__ Pick slot[kThreads / 64];
  const int t = threadIdx.x, Dc = p.D, Dk = p.Dk, D = Dc + Dk;
  const int id = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;
  const int first = chunk * (R * kThreads);
  int U[KP], off[KP];                      // (kernel-argument arrays: constant indices only)
#pragma unroll
  for (int d = 0; d < KP; ++d) { U[d] = p.U[d]; off[d] = p.off[d]; }

  float z[R][DP], v[R][KP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int d = 0; d < DP; ++d) z[r][d] = 0.f;
#pragma unroll
    for (int d = 0; d < KP; ++d) v[r][d] = 0.f;
    const int i = first + r * kThreads + t;
    if (i >= p.C) continue;
    if (p.inject) {
      const float* src = p.zsrc + (int64_t)i * D;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) z[r][d] = src[d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) v[r][d] = src[Dc + d];
    } else {
      // block chunk * R + r of this id (i < C: the block exists)
      const float* src = p.zsrc + ((int64_t)id * p.nblk + chunk * R + r) * kThreads * D + t;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) z[r][d] = src[(int64_t)d * kThreads];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) v[r][d] = src[(int64_t)(Dc + d) * kThreads];
    }
  }

  double l2[R], g2[R];
  score_side_wide<DP, KP, R>(p.bmu, p.ba, p.bc, p.bcat, p.bmiss, p.bbonus, p.kb, Dc, Dk, U, off, z, v, rows, cats, cl,
                             l2);
  score_side_wide<DP, KP, R>(p.amu, p.aa, p.ac, p.acat, p.amiss, p.abonus, p.ka, Dc, Dk, U, off, z, v, rows, cats, cl,
                             g2);

  Pick best{0, 0};
  double lv[R], gv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = first + r * kThreads + t;
    lv[r] = l2[r] * kLn2 + p.bbase;
    gv[r] = g2[r] * kLn2 + p.abase;
    if (i >= p.C) continue;
    const int64_t o = (int64_t)id * p.C + i;
    if (p.l_out) p.l_out[o] = lv[r];
    if (p.g_out) p.g_out[o] = gv[r];
    if (p.cand) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < Dc) p.cand[o * D + d] = z[r][d];
#pragma unroll
      for (int d = 0; d < KP; ++d)
        if (d < Dk) p.cand[o * D + Dc + d] = v[r][d];
    }
    const uint64_t key = score_key(lv[r] - gv[r]);
    if (key > best.key) best = Pick{key, (int64_t)i};   // ascending index: strict > keeps the first of a tie
  }
  Pick w = wave_best(best);
  if ((t & 63) == 0) slot[t >> 6] = w;
  __syncthreads();
  w = slot[0];
#pragma unroll
  for (int q = 1; q < kThreads / 64; ++q)
    if (beats(slot[q], w)) w = slot[q];

  tpe_joint_wide_record* rec = p.chunk_rec + blockIdx.x;
  if (w.key == 0) {
    if (t == 0) rec->global_idx = -1;
    return;
  }
  const int woff = (int)(w.idx - first);
  if (t != woff % kThreads) return;
  const int wr = woff / kThreads;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r != wr) continue;
    rec->global_idx = w.idx + (int64_t)p.cand_base;
    rec->l = lv[r];
    rec->g = gv[r];
    // kernel coordinate order: the Dc continuous entries, the categories, then zeros
#pragma unroll
    for (int d = 0; d < kWD; ++d)
      if (d >= D) rec->z[d] = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d)
      if (d < Dc) rec->z[d] = (double)z[r][d];
#pragma unroll
    for (int d = 0; d < KP; ++d)
      if (d < Dk) rec->z[Dc + d] = (double)v[r][d];
  }
}

template <int DP, int KP, int QP, int R>
__global__ __launch_bounds__(kThreads) void k_joint_wide_quant_chunk(const WideQuantK p) {
  static_assert(DP % 4 == 0 && DP <= kWD && KP <= kWK && QP >= 1 && QP <= kWQ,
                "rows are read as float4; the argument arrays");
  constexpr int TK = wide_tile(DP);
  __shared__ __attribute__((aligned(16))) float rows[TK * 2 * DP];
  __shared__ __attribute__((aligned(16))) float cats[TK * slots(KP)];
  __shared__ float cl[TK];
  __shared__ Pick slot[kThreads / 64];
  extern __shared__ __attribute__((aligned(16))) float qt[];     // [(total + 1) * stride]
  static_assert(sizeof(float) * (TK * 2 * DP + TK * slots(KP) + TK) + sizeof(Pick) * (kThreads / 64) + kWQTileBytes <=
                    64 * 1024, "static and dynamic LDS of a workgroup stay under 64 KiB");
  int U[slots(KP)], off[slots(KP)];        // (kernel-argument arrays: constant indices only)
  U[0] = 1; off[0] = 0;
#pragma unroll
  for (int d = 0; d < KP; ++d) { U[d] = p.U[d]; off[d] = p.off[d]; }

  for (int e = threadIdx.x; e < p.stride; e += kThreads) qt[p.total * p.stride + e] = 0.f;   // the padded slots' row

  WideCand<DP, KP, QP, R> c;
  wide_load(p, wide_at(p.n_chunks), p.Dk, p.Dq, c);
  // the lattice value's row in the tile (kept inside the table); a padded slot reads the zero row
  int qo[R][QP];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int d = 0; d < QP; ++d)
      qo[r][d] = (d < p.Dq ? p.voff[d] + cat_index(c.x[r][d], p.V[d]) : p.total) * p.stride;

  double l2[R], g2[R];
  score_side_wide_quant<DP, KP, QP, R>(p.bmu, p.ba, p.bc, p.bcat, p.bmiss, p.bbonus, p.bT, p.kb, p.D, p.Dk, p.tile,
                                       p.stride, p.total, U, off, c.z, c.v, qo, rows, cats, cl, qt, l2);
  score_side_wide_quant<DP, KP, QP, R>(p.amu, p.aa, p.ac, p.acat, p.amiss, p.abonus, p.aT, p.ka, p.D, p.Dk, p.tile,
                                       p.stride, p.total, U, off, c.z, c.v, qo, rows, cats, cl, qt, g2);
  wide_finish(p, wide_at(p.n_chunks), p.Dk, p.Dq, c, l2, g2, slot);
}

__global__ __launch_bounds__(64) void k_joint_wide_merge(const tpe_joint_wide_record* __restrict__ chunk_rec,
                                                         int n_chunks, tpe_joint_wide_record* __restrict__ records) {
  const tpe_joint_wide_record* rec = chunk_rec + (int64_t)blockIdx.x * n_chunks;
  Pick best{0, 0};
  for (int c = threadIdx.x; c < n_chunks; c += 64) {
    if (rec[c].global_idx < 0) continue;
    const Pick x{score_key(rec[c].l - rec[c].g), (int64_t)c};
    if (beats(x, best)) best = x;            // (chunk order = candidate index order)
  }
  const Pick w = wave_best(best);
  if (threadIdx.x != 0) return;
  tpe_joint_wide_record* out = records + blockIdx.x;
  if (w.key == 0) {
    out->global_idx = -1;
    out->l = out->g = 0.0;
    for (int d = 0; d < kWD; ++d) out->z[d] = 0.0;
  } else {
    *out = rec[w.idx];
  }
}

// ---------------------------------------------------- wide segmented stage
// The wide stage over the (id, group) problems of MANY groups at once
// (include/tpe_hip.h "Wide segmented joint stage"): a workgroup reads its
// problem's descriptor, builds the solo kernels' argument view of that problem
// alone (one id, its pointers set to the problem's rows and outputs) and runs
// the solo kernels' parts, so a problem's bytes are those of a solo launch over
// its group.
struct WideSegK {
  int C, n_chunks, inject, first;   // n_chunks, first: this launch's class (as SegK::first)
  int n_probs, n_segs, nblk;        // nblk: 256-candidate blocks a problem = chunk_rec's stride
  uint32_t key0, key1;
  uint32_t cand_base;
  const tpe_joint_wide_seg* segs;
  const float* pool;
  const double* pool64;
  const int32_t* prob_seg;
  const int64_t* prob_id;
  const int64_t* cand_off;
  int32_t* order;                   // scratch [n_probs]: the problems by (DP class, group, index)
  float* cand;
  double *l_out, *g_out;
  tpe_joint_wide_record* chunk_rec; // scratch [n_probs * nblk], problem-major
  float* zbuf;                      // scratch [n_probs] slabs of nblk * 256 * kWD floats; a slab is [nblk][D][256]
};
__host__ __device__ __forceinline__ int wide_class(int D) { return D <= 20 ? 0 : D <= 24 ? 1 : D <= 32 ? 2 : D <= 48 ? 3 : 4; }
template <bool MIXED>
__device__ __forceinline__ int seg_class(const WideSegK& p, int s) { return wide_class(p.segs[s].n_dims); }
__device__ __forceinline__ float* wide_seg_slab(const WideSegK& p, int prob) {
  return p.zbuf + (int64_t)prob * p.nblk * (kThreads * kWD);
}

// one workgroup per (problem, 256-candidate block), in the caller's problem order
__global__ __launch_bounds__(kThreads) void k_joint_wide_seg_sample(const WideSegK p) {
  __shared__ float blo[kWD], bhi[kWD];
  const int prob = blockIdx.x / p.nblk, blk = blockIdx.x % p.nblk;
  const tpe_joint_wide_seg* __restrict__ sg = p.segs + uni(p.prob_seg[prob]);
  if (threadIdx.x < kWD) { blo[threadIdx.x] = sg->lo[threadIdx.x]; bhi[threadIdx.x] = sg->hi[threadIdx.x]; }
  __syncthreads();

  WideSampK q;                      // (q.lo / q.hi: the parts read the LDS copies)
  q.D = uni(sg->n_dims); q.C = p.C; q.nblk = p.nblk; q.kb = uni(sg->k_below);
  q.key0 = p.key0; q.key1 = p.key1; q.stream_word = (uint32_t)uni((int)sg->stream_word);
  q.cand_base = p.cand_base;
  q.cum = p.pool64 + uni(sg->samp_cum); q.samp = p.pool + uni(sg->samp);
  q.ids = p.prob_id; q.zbuf = wide_seg_slab(p, prob);
  const int i = blk * kThreads + threadIdx.x;
  if (i >= p.C) return;
  WideDraw c;                       // wide_sample_head over this problem: block blk of its slab, its id
  c.out = q.zbuf + (int64_t)blk * kThreads * q.D + threadIdx.x;
  wide_sample_stream(q, i, prob, c);
  wide_sample_continuous(q, c, blo, bhi);
}

// one workgroup per (problem of the launch's DP class, chunk of 256 R candidates)
template <int DP, int R>
__global__ __launch_bounds__(kThreads) void k_joint_wide_seg_chunk(const WideSegK p) {
  static_assert(DP % 4 == 0 && DP <= kWD, "rows are read as float4");
  constexpr int TK = wide_tile(DP);
  __shared__ __attribute__((aligned(16))) float rows[TK * 2 * DP];
  __shared__ float cl[TK];
  __shared__ Pick slot[kThreads / 64];
  const int none[1] = {0};
  const int chunk = blockIdx.x % p.n_chunks;
  // the problem and its group: the same for every lane, kept in scalar registers
  const int prob = uni(p.order[p.first + blockIdx.x / p.n_chunks]);
  const tpe_joint_wide_seg* __restrict__ sg = p.segs + uni(p.prob_seg[prob]);

  WideK k;
  k.D = uni(sg->n_dims); k.C = p.C; k.n_chunks = p.n_chunks; k.nblk = p.nblk; k.inject = p.inject;
  k.kb = uni(sg->k_below); k.ka = uni(sg->k_above); k.cand_base = p.cand_base;
  k.bmu = p.pool + uni(sg->below_mu); k.ba = p.pool + uni(sg->below_a); k.bc = p.pool + uni(sg->below_c);
  k.amu = p.pool + uni(sg->above_mu); k.aa = p.pool + uni(sg->above_a); k.ac = p.pool + uni(sg->above_c);
  k.bbase = unid(sg->below_base); k.abase = unid(sg->above_base);
  k.zsrc = p.inject ? p.pool + uni(sg->inject) : wide_seg_slab(p, prob);
  k.cand = p.cand ? p.cand + uni(p.cand_off[prob]) : nullptr;
  k.l_out = p.l_out ? p.l_out + (int64_t)prob * p.C : nullptr;
  k.g_out = p.g_out ? p.g_out + (int64_t)prob * p.C : nullptr;
  k.chunk_rec = p.chunk_rec + (int64_t)prob * p.nblk;
  const WideAt at{0, chunk, (int64_t)chunk};
  // R = 2: the class has n_chunks <= nblk <= 2 n_chunks records a problem; the merge reads nblk
  if (R > 1 && threadIdx.x == 0 && p.n_chunks + chunk < p.nblk) k.chunk_rec[p.n_chunks + chunk].global_idx = -1;

  WideCand<DP, 0, 0, R> c;
  wide_load(k, at, 0, 0, c);
  double l2[R], g2[R];
  score_side_wide<DP, 0, R>(k.bmu, k.ba, k.bc, nullptr, nullptr, nullptr, k.kb, k.D, 0, none, none, c.z, c.v, rows,
                            nullptr, cl, l2);
  score_side_wide<DP, 0, R>(k.amu, k.aa, k.ac, nullptr, nullptr, nullptr, k.ka, k.D, 0, none, none, c.z, c.v, rows,
                            nullptr, cl, g2);
  wide_finish(k, at, 0, 0, c, l2, g2, slot);
}

// ------------------------------------------------------------- host driver
// Everything from here on runs on the host: the stages' argument checks,
// the kernel-argument fills and the launches.  What the stages share exists
// once (the launch and its profiling events, the padded-width dispatchers, the
// solo stages' head checks and JointK fill, the category and lattice checks,
// the segmented stages' skeleton, every scratch size); a joint_*_run_at below
// checks what is particular to its stage, fills what is particular and picks
// the kernel.

// "<entry>: <pre><what><post>" as the call's error; pre / post carry the
// segmented stages' "a segment's " / " in a segment"
constexpr const char* kSegs = "a segment's ";
constexpr const char* kInSeg = " in a segment";
int fail(const char* entry, const char* what, const char* pre = "", const char* post = "") {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s%s%s", entry, pre, what, post);
  return tpe_internal_fail(TPE_E_ARG, msg);
}
int hip_fail(hipError_t e) { return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e)); }

// ---- profiling (tpe_joint_profile and its companions; off: no events at all)
struct Ev {
  hipEvent_t start = nullptr, stop = nullptr;
};
// tpe_joint_profile: start / stop events of the chunk launch and the merge
struct {
  int on, valid;
  hipEvent_t ev[4];
} g_prof = {0, 0, {}};
// tpe_joint_seg_run's / tpe_joint_mseg_run's launches before the merge: the order
// kernel, the table kernel and one chunk launch per kernel class present
// (g_prof.valid == 2: sum these for last_ms[0])
constexpr int kSegLaunches = 2 + kMClasses;
struct {
  int n;
  hipEvent_t ev[2 * kSegLaunches];
} g_sprof = {0, {}};
// start / stop events around the two table launches of tpe_joint_quant_run
struct {
  int valid;
  hipEvent_t ev[2];
} g_qprof = {0, {}};
// start / stop events of the wide stage's sampling kernel
struct {
  int valid;
  hipEvent_t ev[2];
} g_wprof = {0, {}};

// the events of ev[0 .. n) that do not exist yet
int ensure_events(hipEvent_t* ev, int n) {
  for (int i = 0; i < n; ++i) {
    if (ev[i]) continue;
    const hipError_t e = hipEventCreate(&ev[i]);
    if (e != hipSuccess) return hip_fail(e);
  }
  return TPE_OK;
}

// the device time between two recorded events (it WAITS for the second)
int elapsed_ms(hipEvent_t start, hipEvent_t stop, double* out) {
  float ms = 0.f;
  hipError_t e = hipEventSynchronize(stop);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, start, stop);
  if (e != hipSuccess) return hip_fail(e);
  *out = (double)ms;
  return TPE_OK;
}

// One launch of 256-thread (merge: 64-thread) workgroups: the event launch when a
// start or a stop event is given (profiling), else the plain one.
template <typename K, typename... Args>
void launch(K kernel, dim3 grid, unsigned block, unsigned lds, hipStream_t s, hipEvent_t start, hipEvent_t stop,
            const Args&... args) {
  if (start || stop) hipExtLaunchKernelGGL(kernel, grid, dim3(block), lds, s, start, stop, 0u, args...);
  else hipLaunchKernelGGL(kernel, grid, dim3(block), lds, s, args...);
}

// a solo stage's chunk launch under profiling
Ev chunk_marks(bool timed) { return timed ? Ev{g_prof.ev[0], g_prof.ev[1]} : Ev{}; }
// the next launch of a segmented stage under profiling: n counts them
Ev seg_marks(bool timed, int& n) {
  if (!timed) return Ev{};
  const Ev e{g_sprof.ev[2 * n], g_sprof.ev[2 * n + 1]};
  ++n;
  return e;
}

// What every run ends with: the merge over n_probs problems (k_joint_merge, or
// k_joint_wide_merge on the wide record), under profiling what
// tpe_joint_profile reads (valid: 1 a solo stage, 2 a segmented one with
// n_timed launches before the merge), and the launches' error.
template <typename Rec>
int finish(void (*merge)(const Rec*, int, Rec*), const Rec* chunk_rec, int n_chunks, Rec* records, int n_probs,
           hipStream_t s, bool timed, int valid, int n_timed = 0) {
  launch(merge, dim3((unsigned)n_probs), 64u, 0u, s, timed ? g_prof.ev[2] : nullptr, timed ? g_prof.ev[3] : nullptr,
         chunk_rec, n_chunks, records);
  if (timed) {
    g_sprof.n = n_timed;
    g_prof.valid = valid;
  }
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(e) : TPE_OK;
}

// ---- the padded widths: one dispatcher per axis, f(std::integral_constant<int, P>)
template <int N>
using Int = std::integral_constant<int, N>;
// the first P of the list that n fits (the last one if none does)
template <int P, int... Rest, typename F>
void pad_to(int n, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(Int<P>());
  else if (n <= P) f(Int<P>());
  else pad_to<Rest...>(n, f);
}
// the continuous width of class c (dp_class, which the order kernel sorts by)
template <typename F>
void for_dp(int c, F&& f) {
  switch (c) {
    case 0: f(Int<1>()); break;
    case 1: f(Int<2>()); break;
    case 2: f(Int<3>()); break;
    case 3: f(Int<4>()); break;
    case 4: f(Int<6>()); break;
    case 5: f(Int<8>()); break;
    case 6: f(Int<12>()); break;
    default: f(Int<16>()); break;
  }
}
// padded counts of a group with discrete labels: CP in {0, 2, 4, 8, 16}, KP in
// {1, 2, 4, 8, 16}; 16 continuous slots mean at least 9 continuous labels, so at
// most 7 discrete ones: 24 instantiations in all.  Beside a quantised label and
// in a segment (TOP 8 / 4): CP in {0, 2, 4, 8}, KP in {0, 1, 2, 4} (without a
// quantised label from 1), QP in {1, 2, 4}: 48 instantiations
template <int TOP, typename F>
void for_cp(int Dc, F&& f) {
  if constexpr (TOP == 16) pad_to<0, 2, 4, 8, 16>(Dc, f);
  else pad_to<0, 2, 4, 8>(Dc, f);
}
template <int LOW, int TOP, typename F>
void for_kp(int Dk, F&& f) {
  if constexpr (LOW == 0) pad_to<0, 1, 2, 4>(Dk, f);
  else if constexpr (TOP == 4) pad_to<1, 2, 4>(Dk, f);
  else if constexpr (TOP == 8) pad_to<1, 2, 4, 8>(Dk, f);
  else pad_to<1, 2, 4, 8, 16>(Dk, f);
}
template <typename F>
void for_qp(int Dq, F&& f) { pad_to<1, 2, 4>(Dq, f); }
// the counts that cp_index and mseg_class's discrete and quantised indices stand for
constexpr int kCpOf[4] = {0, 2, 4, 8}, kKpOf[4] = {0, 1, 2, 4}, kQpOf[3] = {1, 2, 4};

// ---- sizes: each once, for the *_bytes exports and the runs' checks
int64_t n_chunks_of(int32_t n_cand) { return ((int64_t)n_cand + TPE_JOINT_CHUNK - 1) / TPE_JOINT_CHUNK; }
uint64_t joint_scratch_need(int32_t n_ids, int32_t n_cand) {
  return (uint64_t)n_ids * (uint64_t)n_chunks_of(n_cand) * sizeof(tpe_joint_record);
}
uint64_t seg_order_bytes(int32_t n_probs) { return ((uint64_t)n_probs * sizeof(int32_t) + 7) & ~(uint64_t)7; }
uint64_t seg_scratch_need(int32_t n_probs, int32_t n_cand) {
  return seg_order_bytes(n_probs) + joint_scratch_need(n_probs, n_cand);
}
uint64_t quant_table_floats(int64_t k_below, int64_t k_above, int64_t total) {
  return ((uint64_t)k_below + (uint64_t)k_above) * (uint64_t)total;
}
// padded width of a wide group: DP in {20, 24, 32, 48, 64}
template <typename F>
void for_wide_dp(int D, F&& f) { pad_to<20, 24, 32, 48, 64>(D, f); }
int wide_dp(int D) {
  int dp = 0;
  for_wide_dp(D, [&](auto p) { dp = decltype(p)::value; });
  return dp;
}
int64_t wide_blocks_of(int32_t n_cand) { return ((int64_t)n_cand + kThreads - 1) / kThreads; }
int64_t wide_chunks_of(int32_t n_cand, int D) {
  const int64_t per = (int64_t)kThreads * wide_r(wide_dp(D));
  return ((int64_t)n_cand + per - 1) / per;
}
uint64_t wide_record_bytes(int32_t n_ids, int32_t n_cand, int D) {
  return (uint64_t)n_ids * (uint64_t)wide_chunks_of(n_cand, D) * sizeof(tpe_joint_wide_record);
}
// (Dk: the discrete coordinates of a wide mixed run beside its D continuous ones;
// the chunk size follows the continuous width, and R is 2 below 20 coordinates too)
uint64_t wide_scratch_need(int32_t n_ids, int32_t n_cand, int D, int Dk = 0) {
  return wide_record_bytes(n_ids, n_cand, D) +
         (uint64_t)n_ids * (uint64_t)wide_blocks_of(n_cand) * kThreads * (uint64_t)(D + Dk) * sizeof(float);
}
// the wide segmented stage: the order, nblk chunk records a problem (the count at
// R = 1), then a slab of nblk blocks of kWD coordinates a problem
uint64_t wide_seg_record_bytes(int32_t n_probs, int32_t n_cand) {
  return (uint64_t)n_probs * (uint64_t)wide_blocks_of(n_cand) * sizeof(tpe_joint_wide_record);
}
uint64_t wide_seg_scratch_need(int32_t n_probs, int32_t n_cand) {
  return seg_order_bytes(n_probs) + wide_seg_record_bytes(n_probs, n_cand) +
         (uint64_t)n_probs * (uint64_t)wide_blocks_of(n_cand) * kThreads * kWD * sizeof(float);
}
// padded continuous width of a wide group with discrete labels: narrow groups too
template <typename F>
void for_wide_mixed_dp(int Dc, F&& f) { pad_to<12, 16, 20, 24, 32, 48, 64>(Dc, f); }
static_assert(wide_r(12) == wide_r(20) && wide_r(16) == wide_r(20), "wide_chunks_of serves the narrow widths");
int size_out(const char* entry, bool ok, uint64_t value, uint64_t* bytes) {
  if (!bytes || !ok) return fail(entry, "bad arguments");
  *bytes = value;
  return TPE_OK;
}

// ---- what the solo stages share
// tpe_joint_args, tpe_joint_wide_args (with it tpe_joint_wide_mixed_args, which
// begins with it) and tpe_joint_mixed_args (with it tpe_joint_quant_args, which
// begins with it) have the same fields at the same offsets up to `low`: the
// head checks and the JointK fill are templates over them
static_assert(offsetof(tpe_joint_wide_args, low) == offsetof(tpe_joint_args, low) &&
                  offsetof(tpe_joint_mixed_args, low) == offsetof(tpe_joint_args, low) &&
                  offsetof(tpe_joint_mixed_args, n_cat) == offsetof(tpe_joint_args, reserved),
              "the solo stages' shared head");
// a mixed group without a discrete label IS a tpe_joint_args (n_cat = 0 reads as reserved)
static_assert(sizeof(tpe_joint_args) == offsetof(tpe_joint_mixed_args, cat_upper) &&
                  offsetof(tpe_joint_mixed_args, high) == offsetof(tpe_joint_args, high),
              "tpe_joint_mixed_args starts with tpe_joint_args");
// ... and a quantised group without a quantised label a tpe_joint_mixed_args
static_assert(offsetof(tpe_joint_quant_args, n_quant) == sizeof(tpe_joint_mixed_args) &&
                  offsetof(tpe_joint_quant_args, cat_cum) == offsetof(tpe_joint_mixed_args, cat_cum),
              "tpe_joint_quant_args starts with tpe_joint_mixed_args");

// ... and a wide group without a discrete label a tpe_joint_wide_args
static_assert(offsetof(tpe_joint_wide_mixed_args, n_cat) == sizeof(tpe_joint_wide_args) &&
                  offsetof(tpe_joint_wide_mixed_args, low) == offsetof(tpe_joint_wide_args, low) &&
                  offsetof(tpe_joint_wide_mixed_args, high) == offsetof(tpe_joint_wide_args, high),
              "tpe_joint_wide_mixed_args starts with tpe_joint_wide_args");

// The checks after the stage's own ones on its dimensions; Dc: the continuous
// coordinates (0: the group has none, and their rows may be null).
template <typename A, typename Rec>
int check_solo_head(const char* entry, const A* a, const Rec* records, int Dc) {
  if (a->n_cand < 1) return fail(entry, "n_cand < 1");
  if (a->n_ids < 1) return fail(entry, "n_ids < 1");
  if (a->k_below < 1 || a->k_above < 1) return fail(entry, "k_below < 1 or k_above < 1");
  if (!a->below_c || !a->above_c || (Dc > 0 && (!a->below_mu || !a->below_a || !a->above_mu || !a->above_a)))
    return fail(entry, "null density rows");
  const bool inject = (a->flags & TPE_JOINT_INJECT) != 0;
  if (inject && !a->inject) return fail(entry, "TPE_JOINT_INJECT without candidates");
  if (!inject && (!a->samp_cum || (Dc > 0 && !a->samp))) return fail(entry, "null sampler rows");
  if (!a->ids || !records) return fail(entry, "null ids / records");
  return TPE_OK;
}
// every stage's last checks: the launch grid, then the scratch
int check_scratch(const char* entry, int64_t blocks, uint64_t need, const void* scratch, uint64_t scratch_bytes) {
  if (blocks > INT32_MAX) return fail(entry, "too many candidates");
  if (!scratch || scratch_bytes < need) return fail(entry, "scratch too small");
  return TPE_OK;
}

// f32 bounds: smallest float >= low, largest float < high
void f32_bounds(double L, double H, float& lo, float& hi) {
  lo = -INFINITY; hi = INFINITY;
  if (L > -INFINITY) { lo = (float)L; if ((double)lo < L) lo = nextafterf(lo, INFINITY); }
  if (H < INFINITY) { hi = (float)H; while ((double)hi >= H) hi = nextafterf(hi, -INFINITY); }
}

// the kernels' view of a solo stage's head, Dc continuous coordinates
template <typename A>
void fill_joint(JointK& k, const A* a, int Dc, uint32_t cand_base, float* cand, double* l_out, double* g_out,
                void* scratch) {
  k.D = Dc; k.C = a->n_cand; k.n_chunks = (int)n_chunks_of(a->n_cand);
  k.inject = (a->flags & TPE_JOINT_INJECT) ? 1 : 0;
  k.kb = a->k_below; k.ka = a->k_above;
  k.key0 = (uint32_t)a->seed; k.key1 = (uint32_t)(a->seed >> 32); k.stream_word = a->stream_word;
  k.cand_base = cand_base;
  k.bmu = a->below_mu; k.ba = a->below_a; k.bc = a->below_c;
  k.amu = a->above_mu; k.aa = a->above_a; k.ac = a->above_c;
  k.bbase = a->below_base; k.abase = a->above_base;
  k.cum = a->samp_cum; k.samp = a->samp; k.ids = a->ids; k.inj = a->inject;
  for (int d = 0; d < TPE_JOINT_MAX_DIMS; ++d) {
    k.lo[d] = -INFINITY; k.hi[d] = INFINITY;
    if (d < Dc) f32_bounds(a->low[d], a->high[d], k.lo[d], k.hi[d]);
  }
  k.cand = cand; k.l_out = l_out; k.g_out = g_out;
  k.chunk_rec = (tpe_joint_record*)scratch;
}
// ... and of its discrete labels, for every stage that has them.  K: MixedK, a
// wide sampling kernel's or a wide scoring kernel's arguments; the padded slots
// hold one category at offset 0.
template <typename K, typename A>
void fill_cat_slots(K& k, const A* a) {
  constexpr int N = (int)(sizeof k.U / sizeof k.U[0]);
  k.Dk = a->n_cat;
  for (int d = 0; d < N; ++d) {
    k.U[d] = d < k.Dk ? a->cat_upper[d] : 1;
    k.off[d] = d < k.Dk ? a->cat_off[d] : 0;
  }
  k.bcat = a->below_cat;
}
// what the sampler reads of them ...
template <typename K, typename A>
void fill_cat_draw(K& k, const A* a) {
  k.bh = a->below_h; k.ccum = a->cat_cum;
}
// ... and what the scoring loop reads
template <typename K, typename A>
void fill_cat_score(K& k, const A* a) {
  k.acat = a->above_cat;
  k.bmiss = a->below_miss; k.bbonus = a->below_bonus; k.amiss = a->above_miss; k.abonus = a->above_bonus;
}
template <typename A>
bool cat_tables_null(const A* a) {
  return !a->below_cat || !a->above_cat || !a->below_miss || !a->below_bonus || !a->above_miss || !a->above_bonus ||
         !a->below_h || !a->cat_cum;
}

// ---- category and lattice checks: the total, or -1 with the call's error set
// n discrete labels' category counts and their offsets in the flat tables
int64_t check_cats(const char* entry, const char* where, const int32_t* upper, const int32_t* off, int n) {
  int64_t total = 0;
  for (int d = 0; d < n; ++d) {
    if (upper[d] < 2 || upper[d] > TPE_JOINT_MAX_CATS)
      return fail(entry, "categories of a label outside [2, TPE_JOINT_MAX_CATS]"), -1;
    total += upper[d];
  }
  if (total > TPE_JOINT_MAX_CAT_TOTAL) return fail(entry, "more than TPE_JOINT_MAX_CAT_TOTAL categories", "", where), -1;
  for (int d = 0; d < n; ++d)
    if (off[d] < 0 || off[d] > total - upper[d]) return fail(entry, "cat_off outside the tables"), -1;
  return total;
}
// n quantised labels' lattice sizes and, with edge_off (null: the sizes alone, as
// the table size needs them), their edges' places in an edge array of n_edges
int64_t check_lattice(const char* entry, const char* where, const int32_t* v, const int32_t* edge_off, int n,
                      int64_t n_edges) {
  int64_t total = 0;
  for (int d = 0; d < n; ++d) {
    if (v[d] < 2 || v[d] > TPE_JOINT_MAX_LATTICE)
      return fail(entry, "lattice values of a label outside [2, TPE_JOINT_MAX_LATTICE]"), -1;
    total += v[d];
  }
  if (!edge_off) return total;
  if (total > TPE_JOINT_MAX_LATTICE_TOTAL)
    return fail(entry, "more than TPE_JOINT_MAX_LATTICE_TOTAL lattice values", "", where), -1;
  for (int d = 0; d < n; ++d)
    if (edge_off[d] < 0 || (int64_t)edge_off[d] + v[d] + 1 > n_edges)
      return fail(entry, "quant_edge_off outside the edge array"), -1;
  return total;
}
// the dynamic LDS of a quantised chunk launch: the table tile of `total` lattice values
unsigned quant_lds(int total) { return (unsigned)((total + 1) * (quant_tile(total) + 4) * sizeof(float)); }

// ---- what the two stages with quantised labels share (tpe_joint_quant_args,
// tpe_joint_wide_quant_args): the checks on the labels, their rows and the table
// workspace (the lattice total, or -1 with the call's error set) ...
template <typename A>
int64_t check_quant(const char* entry, const A* a) {
  const int64_t total = check_lattice(entry, "", a->quant_v, a->quant_edge_off, a->n_quant, a->n_edges);
  if (total < 0) return -1;
  if (!a->quant_edges || !a->below_qmu || !a->below_qsigma || !a->above_qmu || !a->above_qsigma || !a->quant_samp ||
      !a->quant_table)
    return fail(entry, "null quantised rows or table"), -1;
  if (a->quant_table_bytes < quant_table_floats(a->k_below, a->k_above, total) * sizeof(float))
    return fail(entry, "table workspace too small"), -1;
  return total;
}
// ... the labels' padded slots: sizes, table and edge offsets (in tb) and f32
// bounds (a quantised dimension's outer edges: low / high [Dc + d]) ...
template <typename A>
void fill_quant_slots(QTabK& tb, float (&qlo)[TPE_JOINT_MAX_QUANT], float (&qhi)[TPE_JOINT_MAX_QUANT], const A* a) {
  const int Dc = a->n_dims, Dq = a->n_quant;
  int voff = 0;
  for (int d = 0; d < TPE_JOINT_MAX_QUANT; ++d) {
    const bool in = d < Dq;
    tb.V[d] = in ? a->quant_v[d] : 2;
    tb.voff[d] = in ? voff : 0;
    tb.eoff[d] = in ? a->quant_edge_off[d] : 0;
    qlo[d] = -INFINITY; qhi[d] = INFINITY;
    if (in) {
      f32_bounds(a->low[Dc + d], a->high[Dc + d], qlo[d], qhi[d]);
      voff += a->quant_v[d];
    }
  }
}
// ... and the two sides' table launches (tb: fill_quant_slots'), under profiling
// between the events that tpe_joint_quant_profile reads
template <typename A>
int launch_qtables(QTabK& tb, const A* a, int64_t total, hipStream_t s, bool timed) {
  if (timed)
    if (int rc = ensure_events(g_qprof.ev, 2)) return rc;
  const int Dq = a->n_quant;
  tb.K = a->k_below; tb.Dq = Dq; tb.mu = a->below_qmu; tb.sigma = a->below_qsigma; tb.edges = a->quant_edges;
  tb.T = a->quant_table;
  QTabK ta = tb;
  ta.K = a->k_above; ta.mu = a->above_qmu; ta.sigma = a->above_qsigma; ta.T = a->quant_table + total * a->k_below;
  const dim3 gb((unsigned)((a->k_below + kThreads - 1) / kThreads), (unsigned)Dq);
  const dim3 ga((unsigned)((a->k_above + kThreads - 1) / kThreads), (unsigned)Dq);
  launch(k_joint_qtable, gb, kThreads, 0u, s, timed ? g_qprof.ev[0] : nullptr, nullptr, tb);
  launch(k_joint_qtable, ga, kThreads, 0u, s, nullptr, timed ? g_qprof.ev[1] : nullptr, ta);
  if (timed) g_qprof.valid = 1;
  return TPE_OK;
}

// ---- the solo stages; local candidate i is global candidate cand_base + i (tpe_joint_run_shard)
int joint_run_at(const tpe_joint_args* a, tpe_joint_record* records, float* cand, double* l_out, double* g_out,
                 void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_dims < 1 || a->n_dims > TPE_JOINT_MAX_DIMS) return fail(E, "n_dims outside [1, TPE_JOINT_MAX_DIMS]");
  if (int rc = check_solo_head(E, a, records, a->n_dims)) return rc;
  const int64_t blocks = n_chunks_of(a->n_cand) * a->n_ids;
  if (int rc = check_scratch(E, blocks, joint_scratch_need(a->n_ids, a->n_cand), scratch, scratch_bytes)) return rc;

  JointK k;
  fill_joint(k, a, a->n_dims, cand_base, cand, l_out, g_out, scratch);
  const bool timed = g_prof.on != 0;
  hipStream_t s = (hipStream_t)stream;
  const Ev ev = chunk_marks(timed);
  for_dp(dp_class(a->n_dims), [&](auto dp) {
    launch(k_joint_chunk<decltype(dp)::value>, dim3((unsigned)blocks), kThreads, 0u, s, ev.start, ev.stop, k);
  });
  return finish(k_joint_merge, (const tpe_joint_record*)scratch, k.n_chunks, records, a->n_ids, s, timed, 1);
}

// ---- the wide stages: one skeleton (joint_wide_stage); a stage supplies its
// checks, the extra fields of its sampling and scoring arguments and its kernels.
// The sampling kernel's arguments of a group of D continuous coordinates (the
// bounds staged as f32), its launch under profiling, the scoring kernel's arguments.
template <typename A>
void fill_wide_samp(WideSampK& sk, const A* a, int D, int64_t nblk, uint32_t cand_base, float* zbuf) {
  sk.D = D; sk.C = a->n_cand; sk.nblk = (int)nblk; sk.kb = a->k_below;
  sk.key0 = (uint32_t)a->seed; sk.key1 = (uint32_t)(a->seed >> 32); sk.stream_word = a->stream_word;
  sk.cand_base = cand_base;
  sk.cum = a->samp_cum; sk.samp = a->samp; sk.ids = a->ids; sk.zbuf = zbuf;
  for (int d = 0; d < TPE_JOINT_WIDE_MAX_DIMS; ++d) {
    sk.lo[d] = -INFINITY; sk.hi[d] = INFINITY;
    if (d < D) f32_bounds(a->low[d], a->high[d], sk.lo[d], sk.hi[d]);
  }
}
template <typename K, typename SK>
int launch_wide_samp(K kernel, int64_t sblocks, hipStream_t s, bool timed, const SK& sk) {
  if (timed)
    if (int rc = ensure_events(g_wprof.ev, 2)) return rc;
  launch(kernel, dim3((unsigned)sblocks), kThreads, 0u, s, timed ? g_wprof.ev[0] : nullptr,
         timed ? g_wprof.ev[1] : nullptr, sk);
  g_wprof.valid = timed ? 1 : 0;
  return TPE_OK;
}
template <typename A>
void fill_wide(WideK& k, const A* a, int D, int64_t n_chunks, int64_t nblk, uint32_t cand_base, const float* zbuf,
               float* cand, double* l_out, double* g_out, void* scratch) {
  const bool inject = (a->flags & TPE_JOINT_INJECT) != 0;
  k.D = D; k.C = a->n_cand; k.n_chunks = (int)n_chunks; k.nblk = (int)nblk; k.inject = inject ? 1 : 0;
  k.kb = a->k_below; k.ka = a->k_above; k.cand_base = cand_base;
  k.bmu = a->below_mu; k.ba = a->below_a; k.bc = a->below_c;
  k.amu = a->above_mu; k.aa = a->above_a; k.ac = a->above_c;
  k.bbase = a->below_base; k.abase = a->above_base;
  k.zsrc = inject ? a->inject : zbuf;
  k.cand = cand; k.l_out = l_out; k.g_out = g_out;
  k.chunk_rec = (tpe_joint_wide_record*)scratch;
}

// What follows a wide stage's own checks.  Dx: the group's discrete and
// quantised coordinates beside its a->n_dims continuous ones.  sk / k: the
// stage's sampling / scoring arguments with its own fields filled; the shared
// ones are filled here.  tables(s, timed): the stage's launches before the
// sampling kernel (the quantised stage's tables); chunk(blocks, s, ev): its
// scoring launch at its padded widths.
template <typename A, typename SK, typename K, typename SampKernel, typename Tables, typename Chunk>
int joint_wide_stage(const char* E, const A* a, int Dx, SK& sk, K& k, SampKernel samp_kernel, Tables tables,
                     Chunk chunk, tpe_joint_wide_record* records, float* cand, double* l_out, double* g_out,
                     void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  const int D = a->n_dims;
  const bool inject = (a->flags & TPE_JOINT_INJECT) != 0;
  const int64_t n_chunks = wide_chunks_of(a->n_cand, D), blocks = n_chunks * a->n_ids;
  const int64_t nblk = wide_blocks_of(a->n_cand), sblocks = nblk * a->n_ids;
  if (int rc = check_scratch(E, sblocks, wide_scratch_need(a->n_ids, a->n_cand, D, Dx), scratch, scratch_bytes)) return rc;

  const bool timed = g_prof.on != 0;
  hipStream_t s = (hipStream_t)stream;
  float* zbuf = (float*)((char*)scratch + wide_record_bytes(a->n_ids, a->n_cand, D));
  if (int rc = tables(s, timed)) return rc;
  g_wprof.valid = 0;
  if (!inject) {
    fill_wide_samp(sk, a, D, nblk, cand_base, zbuf);
    if (int rc = launch_wide_samp(samp_kernel, sblocks, s, timed, sk)) return rc;
  }
  fill_wide(k, a, D, n_chunks, nblk, cand_base, zbuf, cand, l_out, g_out, scratch);
  chunk((unsigned)blocks, s, chunk_marks(timed));
  return finish(k_joint_wide_merge, (const tpe_joint_wide_record*)scratch, (int)n_chunks, records, a->n_ids, s, timed, 1);
}
constexpr auto kNoTables = [](hipStream_t, bool) { return (int)TPE_OK; };

int joint_wide_run_at(const tpe_joint_wide_args* a, tpe_joint_wide_record* records, float* cand, double* l_out,
                      double* g_out, void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_wide_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_dims < 1 || a->n_dims > TPE_JOINT_WIDE_MAX_DIMS)
    return fail(E, "n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
  if (int rc = check_solo_head(E, a, records, a->n_dims)) return rc;

  WideSampK sk;
  WideK k;
  auto chunk = [&](unsigned blocks, hipStream_t s, Ev ev) {
    for_wide_dp(a->n_dims, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      launch(k_joint_wide_chunk<DP, wide_r(DP)>, dim3(blocks), kThreads, 0u, s, ev.start, ev.stop, k);
    });
  };
  return joint_wide_stage(E, a, 0, sk, k, k_joint_wide_sample, kNoTables, chunk, records, cand, l_out, g_out, scratch,
                          scratch_bytes, stream, cand_base);
}

// (cand_base: the kernels carry it as the wide stage's do; tpe_joint_run_shard does not take this stage yet)
int joint_wide_mixed_run_at(const tpe_joint_wide_mixed_args* a, tpe_joint_wide_record* records, float* cand,
                            double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream,
                            uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_wide_mixed_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_cat < 0 || a->n_cat > TPE_JOINT_WIDE_MAX_CAT) return fail(E, "n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]");
  if (a->n_cat == 0) {                      // no discrete label: the wide stage, the same bytes
    tpe_joint_wide_args c;
    memcpy(&c, a, sizeof c);
    return joint_wide_run_at(&c, records, cand, l_out, g_out, scratch, scratch_bytes, stream, cand_base);
  }
  if (a->n_dims < 1 || a->n_dims + a->n_cat > TPE_JOINT_WIDE_MAX_DIMS)
    return fail(E, "n_dims < 1 or n_dims + n_cat outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
  const int Dc = a->n_dims, Dk = a->n_cat;
  if (int rc = check_solo_head(E, a, records, Dc)) return rc;
  if (cat_tables_null(a)) return fail(E, "null category tables");
  if (check_cats(E, "", a->cat_upper, a->cat_off, Dk) < 0) return TPE_E_ARG;

  WideMixedSampK sk;
  WideMixedK k;
  fill_cat_slots(sk, a); fill_cat_draw(sk, a);
  fill_cat_slots(k, a); fill_cat_score(k, a);
  auto chunk = [&](unsigned blocks, hipStream_t s, Ev ev) {
    for_wide_mixed_dp(Dc, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      for_kp<1, 8>(Dk, [&](auto kp) {
        launch(k_joint_wide_mixed_chunk<DP, decltype(kp)::value, wide_r(DP)>, dim3(blocks), kThreads, 0u, s, ev.start,
               ev.stop, k);
      });
    });
  };
  return joint_wide_stage(E, a, Dk, sk, k, k_joint_wide_mixed_sample, kNoTables, chunk, records, cand, l_out, g_out,
                          scratch, scratch_bytes, stream, cand_base);
}

// ... and a wide quantised group without a quantised label a tpe_joint_wide_mixed_args
static_assert(offsetof(tpe_joint_wide_quant_args, n_quant) == sizeof(tpe_joint_wide_mixed_args) &&
                  offsetof(tpe_joint_wide_quant_args, n_cat) == offsetof(tpe_joint_wide_mixed_args, n_cat) &&
                  offsetof(tpe_joint_wide_quant_args, cat_cum) == offsetof(tpe_joint_wide_mixed_args, cat_cum),
              "tpe_joint_wide_quant_args starts with tpe_joint_wide_mixed_args");

// padded widths of a wide group with quantised labels: DP in {16, 24, 32, 48, 64}
// (of for_wide_mixed_dp's set), KP in {0, 2, 8}, QP in {1, 2, 4}: 45 instantiations
template <typename F>
void for_wide_quant_dp(int Dc, F&& f) { pad_to<16, 24, 32, 48, 64>(Dc, f); }
template <typename F>
void for_wide_quant_kp(int Dk, F&& f) { pad_to<0, 2, 8>(Dk, f); }
int wide_quant_dp(int Dc) {
  int dp = 0;
  for_wide_quant_dp(Dc, [&](auto p) { dp = decltype(p)::value; });
  return dp;
}
static_assert(wide_r(16) == wide_r(20) && wide_r(24) == wide_r(20), "wide_chunks_of serves these widths");
// the scratch of a wide quantised run: the chunk records (their count follows the
// continuous width), then the candidate block over all Dc + Dk + Dq coordinates
uint64_t wide_quant_scratch_need(int32_t n_ids, int32_t n_cand, int Dc, int Dk, int Dq) {
  return wide_scratch_need(n_ids, n_cand, Dc, Dk + Dq);
}
// ... and its limits on the counts alone (tpe_joint_wide_quant_scratch_bytes, the run)
bool wide_quant_counts_ok(int Dc, int Dk, int Dq) {
  return Dc >= 1 && Dk >= 0 && Dk <= TPE_JOINT_WIDE_MAX_CAT && Dq >= 1 && Dq <= TPE_JOINT_MAX_QUANT &&
         Dc <= TPE_JOINT_WIDE_MAX_DIMS && Dc + Dk + Dq <= TPE_JOINT_WIDE_MAX_DIMS;
}

// (cand_base: as the wide mixed stage; tpe_joint_run_shard does not take this stage)
int joint_wide_quant_run_at(const tpe_joint_wide_quant_args* a, tpe_joint_wide_record* records, float* cand,
                            double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream,
                            uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_wide_quant_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_quant < 1 || a->n_quant > TPE_JOINT_MAX_QUANT) return fail(E, "n_quant outside [1, TPE_JOINT_MAX_QUANT]");
  if (a->n_cat < 0 || a->n_cat > TPE_JOINT_WIDE_MAX_CAT) return fail(E, "n_cat outside [0, TPE_JOINT_WIDE_MAX_CAT]");
  if (!wide_quant_counts_ok(a->n_dims, a->n_cat, a->n_quant))
    return fail(E, "n_dims < 1 or n_dims + n_cat + n_quant outside [2, TPE_JOINT_WIDE_MAX_DIMS]");
  const int Dc = a->n_dims, Dk = a->n_cat, Dq = a->n_quant;
  if (int rc = check_solo_head(E, a, records, Dc)) return rc;
  if (Dk > 0) {
    if (cat_tables_null(a)) return fail(E, "null category tables");
    if (check_cats(E, "", a->cat_upper, a->cat_off, Dk) < 0) return TPE_E_ARG;
  }
  const int64_t total = check_quant(E, a);
  if (total < 0) return TPE_E_ARG;

  WideQuantSampK sk;
  WideQuantK k;
  QTabK tb;
  fill_cat_slots(sk, a); fill_cat_draw(sk, a);
  fill_cat_slots(k, a); fill_cat_score(k, a);
  fill_quant_slots(tb, sk.qlo, sk.qhi, a);
  memcpy(sk.V, tb.V, sizeof tb.V); memcpy(sk.eoff, tb.eoff, sizeof tb.eoff);
  memcpy(k.V, tb.V, sizeof tb.V); memcpy(k.voff, tb.voff, sizeof tb.voff);
  sk.Dq = Dq; sk.edges = a->quant_edges; sk.qsamp = a->quant_samp;
  k.Dq = Dq; k.total = (int)total;
  k.tile = wide_quant_tile((int)total, wide_tile(wide_quant_dp(Dc))); k.stride = k.tile + 4;
  k.bT = a->quant_table; k.aT = a->quant_table + total * a->k_below;
  const unsigned lds = (unsigned)((total + 1) * k.stride * sizeof(float));
  auto tables = [&](hipStream_t s, bool timed) { return launch_qtables(tb, a, total, s, timed); };
  auto chunk = [&](unsigned blocks, hipStream_t s, Ev ev) {
    for_wide_quant_dp(Dc, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      for_wide_quant_kp(Dk, [&](auto kp) {
        for_qp(Dq, [&](auto qp) {
          launch(k_joint_wide_quant_chunk<DP, decltype(kp)::value, decltype(qp)::value, wide_r(DP)>, dim3(blocks),
                 kThreads, lds, s, ev.start, ev.stop, k);
        });
      });
    });
  };
  return joint_wide_stage(E, a, Dk + Dq, sk, k, k_joint_wide_quant_sample, tables, chunk, records, cand, l_out, g_out,
                          scratch, scratch_bytes, stream, cand_base);
}

int joint_mixed_run_at(const tpe_joint_mixed_args* a, tpe_joint_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_mixed_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_cat < 0) return fail(E, "n_cat < 0");
  if (a->n_dims < 0 || a->n_dims > TPE_JOINT_MAX_DIMS || a->n_dims + a->n_cat < 1 ||
      a->n_dims + a->n_cat > TPE_JOINT_MAX_DIMS)
    return fail(E, "n_dims + n_cat outside [1, TPE_JOINT_MAX_DIMS]");
  if (a->n_cat == 0) {                      // no discrete label: the continuous stage, the same bytes
    tpe_joint_args c;
    memcpy(&c, a, sizeof c);
    return joint_run_at(&c, records, cand, l_out, g_out, scratch, scratch_bytes, stream, cand_base);
  }
  const int Dc = a->n_dims, Dk = a->n_cat;
  if (int rc = check_solo_head(E, a, records, Dc)) return rc;
  if (cat_tables_null(a)) return fail(E, "null category tables");
  if (check_cats(E, "", a->cat_upper, a->cat_off, Dk) < 0) return TPE_E_ARG;
  const int64_t blocks = n_chunks_of(a->n_cand) * a->n_ids;
  if (int rc = check_scratch(E, blocks, joint_scratch_need(a->n_ids, a->n_cand), scratch, scratch_bytes)) return rc;

  MixedK m;
  fill_joint(m.j, a, Dc, cand_base, cand, l_out, g_out, scratch);
  fill_cat_slots(m, a); fill_cat_draw(m, a); fill_cat_score(m, a);
  const bool timed = g_prof.on != 0;
  hipStream_t s = (hipStream_t)stream;
  const Ev ev = chunk_marks(timed);
  for_cp<16>(Dc, [&](auto cp) {
    constexpr int CP = decltype(cp)::value;
    for_kp<1, (CP < 16 ? 16 : 8)>(Dk, [&](auto kp) {       // (no <16, 16>: see for_cp)
      launch(k_joint_mixed_chunk<CP, decltype(kp)::value>, dim3((unsigned)blocks), kThreads, 0u, s, ev.start, ev.stop, m);
    });
  });
  return finish(k_joint_merge, (const tpe_joint_record*)scratch, m.j.n_chunks, records, a->n_ids, s, timed, 1);
}

int joint_quant_run_at(const tpe_joint_quant_args* a, tpe_joint_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  constexpr const char* E = "tpe_joint_quant_run";
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_quant < 0 || a->n_quant > TPE_JOINT_MAX_QUANT) return fail(E, "n_quant outside [0, TPE_JOINT_MAX_QUANT]");
  if (a->n_quant == 0) {                    // no quantised label: the mixed stage, the same bytes
    tpe_joint_mixed_args m;
    memcpy(&m, a, sizeof m);
    return joint_mixed_run_at(&m, records, cand, l_out, g_out, scratch, scratch_bytes, stream, cand_base);
  }
  const int Dc = a->n_dims, Dk = a->n_cat, Dq = a->n_quant;
  if (Dk < 0) return fail(E, "n_cat < 0");
  if (Dc < 0 || Dc > TPE_JOINT_MAX_DIMS || Dk > TPE_JOINT_MAX_DIMS || Dc + Dk + Dq > TPE_JOINT_MAX_DIMS)
    return fail(E, "n_dims + n_cat + n_quant outside [1, TPE_JOINT_MAX_DIMS]");
  if (Dc > 8 || Dk > 4) return fail(E, "n_dims > 8 or n_cat > 4 beside a quantised label");
  if (int rc = check_solo_head(E, a, records, Dc)) return rc;
  if (Dk > 0) {
    if (cat_tables_null(a)) return fail(E, "null category tables");
    if (check_cats(E, "", a->cat_upper, a->cat_off, Dk) < 0) return TPE_E_ARG;
  }
  const int64_t total = check_quant(E, a);
  if (total < 0) return TPE_E_ARG;
  const int64_t blocks = n_chunks_of(a->n_cand) * a->n_ids;
  if (int rc = check_scratch(E, blocks, joint_scratch_need(a->n_ids, a->n_cand), scratch, scratch_bytes)) return rc;

  QuantK qk;
  fill_joint(qk.m.j, a, Dc, cand_base, cand, l_out, g_out, scratch);
  fill_cat_slots(qk.m, a); fill_cat_draw(qk.m, a); fill_cat_score(qk.m, a);
  qk.Dq = Dq; qk.total = (int)total;
  qk.edges = a->quant_edges; qk.qsamp = a->quant_samp;
  qk.bT = a->quant_table; qk.aT = a->quant_table + total * a->k_below;
  QTabK tb;
  fill_quant_slots(tb, qk.qlo, qk.qhi, a);
  memcpy(qk.V, tb.V, sizeof tb.V); memcpy(qk.voff, tb.voff, sizeof tb.voff); memcpy(qk.eoff, tb.eoff, sizeof tb.eoff);
  qk.tile = quant_tile((int)total); qk.stride = qk.tile + 4;

  const bool timed = g_prof.on != 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_qtables(tb, a, total, s, timed)) return rc;

  const Ev ev = chunk_marks(timed);
  for_cp<8>(Dc, [&](auto cp) {
    for_kp<0, 4>(Dk, [&](auto kp) {
      for_qp(Dq, [&](auto qp) {
        launch(k_joint_quant_chunk<decltype(cp)::value, decltype(kp)::value, decltype(qp)::value>,
               dim3((unsigned)blocks), kThreads, quant_lds((int)total), s, ev.start, ev.stop, qk);
      });
    });
  });
  return finish(k_joint_merge, (const tpe_joint_record*)scratch, qk.m.j.n_chunks, records, a->n_ids, s, timed, 1);
}

// ---- the segmented stages: one skeleton (joint_seg_run_at); a stage supplies its
// per-segment check, its class function and its class launcher as overloads on
// its descriptor, tpe_joint_seg or tpe_joint_mseg
static_assert(offsetof(tpe_joint_mseg, hi) == offsetof(tpe_joint_seg, hi) &&
                  offsetof(tpe_joint_mseg, n_cat) == sizeof(tpe_joint_seg),
              "tpe_joint_mseg starts with tpe_joint_seg");
static_assert(offsetof(tpe_joint_mseg_args, cand_off) == offsetof(tpe_joint_seg_args, cand_off), "the shared fields");

// rows [off, off + n) inside a pool of len elements
bool inside(int64_t off, int64_t n, int64_t len) { return off >= 0 && n <= len && off <= len - n; }

// what the checks leave for the launches: the problems per kernel class and, for
// the mixed stage, the table launch's grid and the classes' dynamic LDS
struct SegPlan {
  int64_t per_class[kMClasses] = {};
  unsigned lds[kMClasses] = {};
  int max_kblocks = 0;
  bool any_quant = false;
};
constexpr int n_classes_of(const tpe_joint_seg*) { return 8; }
constexpr int n_classes_of(const tpe_joint_mseg*) { return kMClasses; }
constexpr int n_classes_of(const tpe_joint_wide_seg*) { return 5; }

// a continuous segment, narrow or wide: its counts and its rows' places
template <typename A, typename Seg>
int check_cont_segment(const char* entry, const A* a, const Seg& g, bool inject, int max_dims, const char* range) {
  if (g.n_dims < 1 || g.n_dims > max_dims) return fail(entry, range, kSegs);
  if (g.k_below < 1 || g.k_above < 1) return fail(entry, "k_below < 1 or k_above < 1", kSegs);
  const int64_t D = g.n_dims, kb = g.k_below, ka = g.k_above, L = a->pool_f32_len;
  bool ok = inside(g.below_mu, kb * D, L) && inside(g.below_a, kb * D, L) && inside(g.below_c, kb, L) &&
            inside(g.above_mu, ka * D, L) && inside(g.above_a, ka * D, L) && inside(g.above_c, ka, L);
  if (!inject) ok = ok && inside(g.samp, kb * D * 5, L) && inside(g.samp_cum, kb, a->pool_f64_len);
  if (inject && g.inject >= 0) ok = ok && inside(g.inject, (int64_t)a->n_cand * D, L);
  if (!ok) return fail(entry, "rows leave its pool", kSegs);
  return TPE_OK;
}
int check_segment(const char* entry, const tpe_joint_seg_args* a, const tpe_joint_seg& g, bool inject, SegPlan&) {
  return check_cont_segment(entry, a, g, inject, TPE_JOINT_MAX_DIMS, "n_dims outside [1, TPE_JOINT_MAX_DIMS]");
}
int check_segment(const char* entry, const tpe_joint_wide_seg_args* a, const tpe_joint_wide_seg& g, bool inject,
                  SegPlan&) {
  return check_cont_segment(entry, a, g, inject, TPE_JOINT_WIDE_MAX_DIMS, "n_dims outside [1, TPE_JOINT_WIDE_MAX_DIMS]");
}

int check_segment(const char* entry, const tpe_joint_mseg_args* a, const tpe_joint_mseg& g, bool inject, SegPlan& plan) {
  const int64_t L = a->pool_f32_len, L64 = a->pool_f64_len, LT = (int64_t)(a->quant_table_bytes / sizeof(float));
  if (g.n_cat < 0 || g.n_cat > TPE_JOINT_MAX_DIMS) return fail(entry, "n_cat outside [0, TPE_JOINT_MAX_DIMS]", kSegs);
  if (g.n_quant < 0 || g.n_quant > TPE_JOINT_MAX_QUANT)
    return fail(entry, "n_quant outside [0, TPE_JOINT_MAX_QUANT]", kSegs);
  const int64_t Dc = g.n_dims, Dk = g.n_cat, Dq = g.n_quant, D = Dc + Dk + Dq, kb = g.k_below, ka = g.k_above;
  if (Dk + Dq == 0) {
    if (Dc < 1 || Dc > TPE_JOINT_MAX_DIMS) return fail(entry, "n_dims outside [1, TPE_JOINT_MAX_DIMS]", kSegs);
  } else {
    if (Dc < 0) return fail(entry, "n_dims < 0", kSegs);
    if (Dc > TPE_JOINT_MSEG_MAX_CONT || Dk > TPE_JOINT_MSEG_MAX_CAT)
      return fail(entry, "n_dims > 8 or n_cat > 4 in a segment with a discrete or quantised label");
  }
  if (kb < 1 || ka < 1) return fail(entry, "k_below < 1 or k_above < 1", kSegs);
  const int64_t cat_total = check_cats(entry, kInSeg, g.cat_upper, g.cat_off, (int)Dk);
  if (cat_total < 0) return TPE_E_ARG;
  const int64_t total = check_lattice(entry, kInSeg, g.quant_v, g.quant_edge_off, (int)Dq, g.n_edges);
  if (total < 0) return TPE_E_ARG;
  if (Dq > 0 && !a->pool_f64) return fail(entry, "null pool_f64 with a quantised segment");
  if (Dq > 0 && !a->quant_table) return fail(entry, "null table workspace with a quantised segment");
  bool ok = inside(g.below_c, kb, L) && inside(g.above_c, ka, L);
  if (Dc > 0)
    ok = ok && inside(g.below_mu, kb * Dc, L) && inside(g.below_a, kb * Dc, L) && inside(g.above_mu, ka * Dc, L) &&
         inside(g.above_a, ka * Dc, L);
  if (!inject) ok = ok && inside(g.samp_cum, kb, L64) && (Dc == 0 || inside(g.samp, kb * Dc * 5, L));
  if (inject && g.inject >= 0) ok = ok && inside(g.inject, (int64_t)a->n_cand * D, L);
  if (Dk > 0) {
    ok = ok && inside(g.below_cat, kb * Dk, L) && inside(g.above_cat, ka * Dk, L) &&
         inside(g.below_miss, cat_total, L) && inside(g.below_bonus, cat_total, L) &&
         inside(g.above_miss, cat_total, L) && inside(g.above_bonus, cat_total, L);
    if (!inject) ok = ok && inside(g.below_h, Dk, L64) && inside(g.cat_cum, cat_total, L64);
  }
  if (Dq > 0) {
    ok = ok && inside(g.quant_edges, g.n_edges, L64) && inside(g.below_qmu, kb * Dq, L64) &&
         inside(g.below_qsigma, kb * Dq, L64) && inside(g.above_qmu, ka * Dq, L64) &&
         inside(g.above_qsigma, ka * Dq, L64);
    if (!inject) ok = ok && inside(g.quant_samp, kb * Dq * 5, L);
  }
  if (!ok) return fail(entry, "rows leave its pool", kSegs);
  if (Dq > 0) {
    if (!inside(g.table, (int64_t)quant_table_floats(kb, ka, total), LT))
      return fail(entry, "table leaves the table workspace", kSegs);
    plan.any_quant = true;
    const int kblocks = (int)(((kb > ka ? kb : ka) + kThreads - 1) / kThreads);
    if (kblocks > plan.max_kblocks) plan.max_kblocks = kblocks;
  }
  return TPE_OK;
}

// the kernel class of a segment that has a problem
int segment_class(const tpe_joint_seg& g, SegPlan&) { return dp_class(g.n_dims); }
int segment_class(const tpe_joint_wide_seg& g, SegPlan&) { return wide_class(g.n_dims); }
int segment_class(const tpe_joint_mseg& g, SegPlan& plan) {
  const int c = mseg_class(g.n_dims, g.n_cat, g.n_quant);
  if (g.n_quant > 0) {                     // the segment's own tile (the solo run's rule); the launch takes the largest
    int total = 0;
    for (int d = 0; d < g.n_quant; ++d) total += g.quant_v[d];
    if (quant_lds(total) > plan.lds[c]) plan.lds[c] = quant_lds(total);
  }
  return c;
}

// one chunk launch of kernel class c over `blocks` workgroups
void launch_class(const tpe_joint_seg*, int c, const MSegK& k, unsigned blocks, unsigned, hipStream_t s, Ev ev) {
  for_dp(c, [&](auto dp) {
    launch(k_joint_seg_chunk<decltype(dp)::value, false>, dim3(blocks), kThreads, 0u, s, ev.start, ev.stop, k.s);
  });
}
void launch_class(const tpe_joint_mseg*, int c, const MSegK& k, unsigned blocks, unsigned lds, hipStream_t s, Ev ev) {
  if (c < 8) {
    for_dp(c, [&](auto dp) {
      launch(k_joint_seg_chunk<decltype(dp)::value, true>, dim3(blocks), kThreads, 0u, s, ev.start, ev.stop, k.s);
    });
  } else if (c < 20) {                      // (mseg_class's numbering)
    for_cp<8>(kCpOf[(c - 8) / 3], [&](auto cp) {
      for_kp<1, 4>(kKpOf[(c - 8) % 3 + 1], [&](auto kp) {
        launch(k_joint_mseg_mixed_chunk<decltype(cp)::value, decltype(kp)::value>, dim3(blocks), kThreads, 0u, s,
               ev.start, ev.stop, k);
      });
    });
  } else {
    for_cp<8>(kCpOf[(c - 20) / 12], [&](auto cp) {
      for_kp<0, 4>(kKpOf[(c - 20) / 3 % 4], [&](auto kp) {
        for_qp(kQpOf[(c - 20) % 3], [&](auto qp) {
          launch(k_joint_mseg_quant_chunk<decltype(cp)::value, decltype(kp)::value, decltype(qp)::value>, dim3(blocks),
                 kThreads, lds, s, ev.start, ev.stop, k);
        });
      });
    });
  }
}

constexpr int kWideDpOf[5] = {20, 24, 32, 48, 64};   // (wide_class's numbering)
void launch_class(const tpe_joint_wide_seg*, int c, const WideSegK& k, unsigned blocks, unsigned, hipStream_t s, Ev ev) {
  for_wide_dp(kWideDpOf[c], [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    launch(k_joint_wide_seg_chunk<DP, wide_r(DP)>, dim3(blocks), kThreads, 0u, s, ev.start, ev.stop, k);
  });
}

// the merge kernel of a stage's record
auto merge_of(const tpe_joint_record*) { return &k_joint_merge; }
auto merge_of(const tpe_joint_wide_record*) { return &k_joint_wide_merge; }

// the stages' kernel arguments: SegK (inside MSegK, whose table the mixed stage
// adds) or WideSegK, which names the shared fields alike
SegK& seg_view(MSegK& mk) { return mk.s; }
WideSegK& seg_view(WideSegK& k) { return k; }

template <typename A, typename Rec>
int joint_seg_run_at(const char* E, const A* a, Rec* records, float* cand, double* l_out, double* g_out,
                     void* scratch, uint64_t scratch_bytes, void* stream, uint32_t cand_base) {
  using Seg = std::remove_cv_t<std::remove_pointer_t<decltype(A::host_segs)>>;
  constexpr bool MIXED = std::is_same<Seg, tpe_joint_mseg>::value;
  constexpr bool WIDE = std::is_same<Seg, tpe_joint_wide_seg>::value;
  static_assert(std::is_same<Rec, std::conditional_t<WIDE, tpe_joint_wide_record, tpe_joint_record>>::value,
                "the stage's record");
  constexpr int n_classes = n_classes_of((const Seg*)nullptr);
  tpe_internal_epoch_bump();
  if (!a) return fail(E, "null args");
  if (a->n_segs < 1) return fail(E, "n_segs < 1");
  if (MIXED && a->n_segs > 32767) return fail(E, "more than 32767 segments");
  if (a->n_probs < 1) return fail(E, "n_probs < 1");
  if (a->n_cand < 1) return fail(E, "n_cand < 1");
  if (!a->segs || !a->host_segs) return fail(E, "null segs / host_segs");
  const bool inject = (a->flags & TPE_JOINT_INJECT) != 0;
  if (!a->pool_f32 || (!inject && !a->pool_f64)) return fail(E, "null pool");
  if (!a->prob_seg || !a->host_prob_seg || !a->prob_id) return fail(E, "null prob_seg / host_prob_seg / prob_id");
  if (!records) return fail(E, "null records");
  if (cand && !a->cand_off) return fail(E, "cand without cand_off");
  SegPlan plan;
  for (int s = 0; s < a->n_segs; ++s)
    if (int rc = check_segment(E, a, a->host_segs[s], inject, plan)) return rc;
  for (int p = 0; p < a->n_probs; ++p) {
    const int s = a->host_prob_seg[p];
    if (s < 0 || s >= a->n_segs) return fail(E, "prob_seg outside [0, n_segs)");
    if (inject && a->host_segs[s].inject < 0) return fail(E, "TPE_JOINT_INJECT without candidates");
    ++plan.per_class[segment_class(a->host_segs[s], plan)];
  }
  // the chunk records a problem: the wide stage's count at R = 1, its sampler's grid a problem too
  const int64_t n_chunks = WIDE ? wide_blocks_of(a->n_cand) : n_chunks_of(a->n_cand);
  if ((int64_t)a->n_segs * n_classes > INT32_MAX) return fail(E, "too many candidates");
  const uint64_t need = WIDE ? wide_seg_scratch_need(a->n_probs, a->n_cand) : seg_scratch_need(a->n_probs, a->n_cand);
  if (int rc = check_scratch(E, n_chunks * a->n_probs, need, scratch, scratch_bytes)) return rc;

  std::conditional_t<WIDE, WideSegK, MSegK> mk;   // (the continuous stage's kernels take mk.s alone)
  auto& k = seg_view(mk);
  k.C = a->n_cand; k.n_chunks = (int)n_chunks; k.inject = inject ? 1 : 0; k.first = 0;
  k.n_probs = a->n_probs; k.n_segs = a->n_segs;
  k.key0 = (uint32_t)a->seed; k.key1 = (uint32_t)(a->seed >> 32); k.cand_base = cand_base;
  k.segs = reinterpret_cast<decltype(k.segs)>(a->segs); k.pool = a->pool_f32; k.pool64 = a->pool_f64;
  k.prob_seg = a->prob_seg; k.prob_id = a->prob_id; k.cand_off = a->cand_off;
  k.order = (int32_t*)scratch;
  k.cand = cand; k.l_out = l_out; k.g_out = g_out;
  k.chunk_rec = (Rec*)((char*)scratch + seg_order_bytes(a->n_probs));
  if constexpr (WIDE) {
    k.nblk = (int)n_chunks;
    k.zbuf = (float*)((char*)k.chunk_rec + wide_seg_record_bytes(a->n_probs, a->n_cand));
  } else {
    mk.table = nullptr;
  }

  const bool timed = g_prof.on != 0;
  hipStream_t s = (hipStream_t)stream;
  if (timed)
    if (int rc = ensure_events(g_sprof.ev, 2 * kSegLaunches)) return rc;
  int n_timed = 0;
  Ev ev = seg_marks(timed, n_timed);
  launch(k_joint_seg_order<MIXED, std::remove_reference_t<decltype(k)>>,
         dim3((unsigned)((a->n_probs + kThreads - 1) / kThreads)), kThreads, 0u, s, ev.start, ev.stop, k);
  if constexpr (MIXED) {
    mk.table = a->quant_table;
    if (plan.any_quant) {
      ev = seg_marks(timed, n_timed);
      launch(k_joint_mseg_qtable, dim3((unsigned)plan.max_kblocks, (unsigned)TPE_JOINT_MAX_QUANT, (unsigned)(2 * a->n_segs)),
             kThreads, 0u, s, ev.start, ev.stop, mk);
    }
  }
  if constexpr (WIDE) {                     // the sampler's time is tpe_joint_wide_profile's, as in the solo wide stage
    g_wprof.valid = 0;
    if (!inject)
      if (int rc = launch_wide_samp(k_joint_wide_seg_sample, n_chunks * a->n_probs, s, timed, k)) return rc;
  }
  int64_t first = 0;
  for (int c = 0; c < n_classes; ++c) {
    if (!plan.per_class[c]) continue;
    k.first = (int)first;
    int64_t class_chunks = n_chunks;
    if constexpr (WIDE) k.n_chunks = (int)(class_chunks = wide_chunks_of(a->n_cand, kWideDpOf[c]));
    launch_class((const Seg*)nullptr, c, mk, (unsigned)(plan.per_class[c] * class_chunks), plan.lds[c], s,
                 seg_marks(timed, n_timed));
    first += plan.per_class[c];
  }
  return finish(merge_of(records), (const Rec*)k.chunk_rec, (int)n_chunks, records, a->n_probs, s, timed, 2, n_timed);
}

}  // namespace

extern "C" {

int tpe_joint_profile(int32_t enable, double* last_ms) {
  if (last_ms) {
    if (!g_prof.valid) return fail("tpe_joint_profile", "no profiled tpe_joint_run to read");
    for (int i = g_prof.valid == 2 ? 1 : 0; i < 2; ++i)
      if (int rc = elapsed_ms(g_prof.ev[2 * i], g_prof.ev[2 * i + 1], &last_ms[i])) return rc;
    if (g_prof.valid == 2) {               // a segmented run: its launches before the merge, summed
      last_ms[0] = 0.0;
      for (int i = 0; i < g_sprof.n; ++i) {
        double ms = 0.0;
        if (int rc = elapsed_ms(g_sprof.ev[2 * i], g_sprof.ev[2 * i + 1], &ms)) return rc;
        last_ms[0] += ms;
      }
    }
  }
  if (enable)
    if (int rc = ensure_events(g_prof.ev, 4)) return rc;
  g_prof.on = enable ? 1 : 0;
  g_prof.valid = 0;
  return TPE_OK;
}

int tpe_joint_quant_profile(double* table_ms) {
  if (!table_ms || !g_qprof.valid) return fail("tpe_joint_quant_profile", "no profiled tpe_joint_quant_run to read");
  return elapsed_ms(g_qprof.ev[0], g_qprof.ev[1], table_ms);
}

int tpe_joint_wide_profile(double* sample_ms) {
  if (!sample_ms || !g_wprof.valid)
    return fail("tpe_joint_wide_profile", "no profiled sampling tpe_joint_wide_run to read");
  return elapsed_ms(g_wprof.ev[0], g_wprof.ev[1], sample_ms);
}

int tpe_joint_scratch_bytes(int32_t n_ids, int32_t n_cand, uint64_t* bytes) {
  const bool ok = n_ids >= 1 && n_cand >= 1;
  return size_out("tpe_joint_scratch_bytes", ok, ok ? joint_scratch_need(n_ids, n_cand) : 0, bytes);
}

int tpe_joint_seg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes) {
  const bool ok = n_probs >= 1 && n_cand >= 1;
  return size_out("tpe_joint_seg_scratch_bytes", ok, ok ? seg_scratch_need(n_probs, n_cand) : 0, bytes);
}

int tpe_joint_mseg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes) {
  const bool ok = n_probs >= 1 && n_cand >= 1;
  return size_out("tpe_joint_mseg_scratch_bytes", ok, ok ? seg_scratch_need(n_probs, n_cand) : 0, bytes);
}

int tpe_joint_wide_seg_scratch_bytes(int32_t n_probs, int32_t n_cand, uint64_t* bytes) {
  const bool ok = n_probs >= 1 && n_cand >= 1;
  return size_out("tpe_joint_wide_seg_scratch_bytes", ok, ok ? wide_seg_scratch_need(n_probs, n_cand) : 0, bytes);
}

int tpe_joint_wide_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, uint64_t* bytes) {
  const bool ok = n_ids >= 1 && n_cand >= 1 && n_dims >= 1 && n_dims <= TPE_JOINT_WIDE_MAX_DIMS;
  return size_out("tpe_joint_wide_scratch_bytes", ok, ok ? wide_scratch_need(n_ids, n_cand, n_dims) : 0, bytes);
}

int tpe_joint_wide_mixed_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, uint64_t* bytes) {
  const bool ok = n_ids >= 1 && n_cand >= 1 && n_dims >= 1 && n_cat >= 0 && n_cat <= TPE_JOINT_WIDE_MAX_CAT &&
                  n_dims + n_cat <= TPE_JOINT_WIDE_MAX_DIMS;
  return size_out("tpe_joint_wide_mixed_scratch_bytes", ok, ok ? wide_scratch_need(n_ids, n_cand, n_dims, n_cat) : 0,
                  bytes);
}

int tpe_joint_wide_quant_scratch_bytes(int32_t n_ids, int32_t n_cand, int32_t n_dims, int32_t n_cat, int32_t n_quant,
                                       uint64_t* bytes) {
  const bool ok = n_ids >= 1 && n_cand >= 1 && wide_quant_counts_ok(n_dims, n_cat, n_quant);
  return size_out("tpe_joint_wide_quant_scratch_bytes", ok,
                  ok ? wide_quant_scratch_need(n_ids, n_cand, n_dims, n_cat, n_quant) : 0, bytes);
}

int tpe_joint_quant_table_bytes(int32_t k_below, int32_t k_above, int32_t total_bins, uint64_t* bytes) {
  const bool ok = k_below >= 1 && k_above >= 1 && total_bins >= 1;
  return size_out("tpe_joint_quant_table_bytes", ok, quant_table_floats(k_below, k_above, total_bins) * sizeof(float),
                  bytes);
}

int tpe_joint_mseg_table_bytes(const tpe_joint_mseg* host_segs, int32_t n_segs, uint64_t* bytes) {
  constexpr const char* E = "tpe_joint_mseg_table_bytes";
  if (!bytes || !host_segs || n_segs < 1) return fail(E, "bad arguments");
  uint64_t n = 0;
  for (int s = 0; s < n_segs; ++s) {
    const tpe_joint_mseg& g = host_segs[s];
    if (g.n_quant < 0 || g.n_quant > TPE_JOINT_MAX_QUANT || g.k_below < 1 || g.k_above < 1)
      return fail(E, "n_quant, k_below or k_above out of range", kSegs);
    const int64_t total = check_lattice(E, "", g.quant_v, nullptr, g.n_quant, 0);
    if (total < 0) return TPE_E_ARG;
    n += quant_table_floats(g.k_below, g.k_above, total);
  }
  *bytes = n * sizeof(float);
  return TPE_OK;
}

int tpe_joint_run(const tpe_joint_args* a, tpe_joint_record* records, float* cand, double* l_out,
                  double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_seg_run(const tpe_joint_seg_args* a, tpe_joint_record* records, float* cand, double* l_out,
                      double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_seg_run_at("tpe_joint_seg_run", a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_mseg_run(const tpe_joint_mseg_args* a, tpe_joint_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_seg_run_at("tpe_joint_mseg_run", a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_wide_seg_run(const tpe_joint_wide_seg_args* a, tpe_joint_wide_record* records, float* cand,
                           double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_seg_run_at("tpe_joint_wide_seg_run", a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_wide_run(const tpe_joint_wide_args* a, tpe_joint_wide_record* records, float* cand, double* l_out,
                       double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_wide_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_wide_mixed_run(const tpe_joint_wide_mixed_args* a, tpe_joint_wide_record* records, float* cand,
                             double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_wide_mixed_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_wide_quant_run(const tpe_joint_wide_quant_args* a, tpe_joint_wide_record* records, float* cand,
                             double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_wide_quant_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_wide_quant_profile(double* sample_ms) {
  if (!sample_ms || !g_wprof.valid)
    return fail("tpe_joint_wide_quant_profile", "no profiled sampling tpe_joint_wide_quant_run to read");
  return elapsed_ms(g_wprof.ev[0], g_wprof.ev[1], sample_ms);
}

int tpe_joint_mixed_run(const tpe_joint_mixed_args* a, tpe_joint_record* records, float* cand, double* l_out,
                        double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_mixed_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_quant_run(const tpe_joint_quant_args* a, tpe_joint_record* records, float* cand, double* l_out,
                        double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  return joint_quant_run_at(a, records, cand, l_out, g_out, scratch, scratch_bytes, stream, 0u);
}

int tpe_joint_run_shard(int32_t stage, const void* args, const tpe_joint_shard* shard, void* records, float* cand,
                        double* l_out, double* g_out, void* scratch, uint64_t scratch_bytes, void* stream) {
  constexpr const char* E = "tpe_joint_run_shard";
  tpe_internal_epoch_bump();
  if (!args) return fail(E, "null args");
  if (!shard) return fail(E, "null shard");
  // every stage's args hold n_cand and flags, read here by the stage's own type; then the stage itself runs
  auto go = [&](auto* a, auto* rec, auto run_at) -> int {
    const int64_t n_cand = a->n_cand;
    if (shard->cand_base < 0) return fail(E, "cand_base < 0");
    // the Philox counter word and the kernels' index arithmetic are 32-bit
    if (shard->n_cand_global >= ((int64_t)1 << 31)) return fail(E, "n_cand_global >= 2^31");
    if (n_cand > shard->n_cand_global || shard->cand_base > shard->n_cand_global - n_cand)
      return fail(E, "cand_base + n_cand > n_cand_global");
    if (((uint32_t)a->flags & TPE_JOINT_INJECT) && shard->cand_base != 0)
      return fail(E, "TPE_JOINT_INJECT with cand_base != 0");
    return run_at(a, rec, cand, l_out, g_out, scratch, scratch_bytes, stream, (uint32_t)shard->cand_base);
  };
  auto seg_at = [](auto* a, auto... rest) { return joint_seg_run_at("tpe_joint_seg_run", a, rest...); };
  auto mseg_at = [](auto* a, auto... rest) { return joint_seg_run_at("tpe_joint_mseg_run", a, rest...); };
  switch (stage) {
    case TPE_JOINT_STAGE_RUN: return go((const tpe_joint_args*)args, (tpe_joint_record*)records, joint_run_at);
    case TPE_JOINT_STAGE_WIDE:
      return go((const tpe_joint_wide_args*)args, (tpe_joint_wide_record*)records, joint_wide_run_at);
    case TPE_JOINT_STAGE_MIXED: return go((const tpe_joint_mixed_args*)args, (tpe_joint_record*)records, joint_mixed_run_at);
    case TPE_JOINT_STAGE_QUANT: return go((const tpe_joint_quant_args*)args, (tpe_joint_record*)records, joint_quant_run_at);
    case TPE_JOINT_STAGE_SEG: return go((const tpe_joint_seg_args*)args, (tpe_joint_record*)records, seg_at);
    case TPE_JOINT_STAGE_MSEG: return go((const tpe_joint_mseg_args*)args, (tpe_joint_record*)records, mseg_at);
    default: return fail(E, "stage outside [0, 5]");
  }
}

}  // extern "C"
