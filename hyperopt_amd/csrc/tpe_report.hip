// MI355X (gfx950) candidate report: the k best distinct candidate values and
// the score statistics of every problem of a batch, from the per-candidate
// buffers the scoring stages leave on the device (include/tpe_hip.h,
// "Candidate report").  Nothing on the suggest path runs through this file.
//
// k_report_chunk  one 256-thread workgroup per (problem, chunk of 4096
//                 candidates): 24 B per candidate read once (cand, l, g),
//                 the chunk's statistics by a fixed reduction tree, then up
//                 to k selection rounds over the 16 (value, score key) pairs
//                 each thread keeps in registers.
// k_report_merge  one workgroup per problem: a k-way merge of the chunk
//                 lists (each already ranked and distinct, so only list heads
//                 compete) and the chunk statistics merged in chunk order.
// k_joint_report_chunk / k_joint_report_merge  the same two passes over the
//                 f32 candidate ROWS a joint stage leaves ("Joint candidate
//                 report"): a score key and a row hash per candidate in
//                 registers, equality decided on the rows themselves.
// Every reduction has a fixed shape and no float atomics: the output bytes
// are a function of the input bytes.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/tpe_hip.h"

extern "C" int tpe_internal_fail(int code, const char* what);   // tpe_kernels.hip (hidden)
extern "C" void tpe_internal_epoch_bump(void);                    // tpe_kernels.hip (hidden): the device epoch

namespace {

constexpr int kThreads = 256;                              // 4 waves of 64
constexpr int kPer = TPE_REPORT_CHUNK / kThreads;          // candidates per thread
static_assert(kPer * kThreads == TPE_REPORT_CHUNK, "chunk = threads x candidates per thread");

// per-chunk record of pass 1 (scratch: n_chunks headers, then n_chunks * k entries)
struct ChunkHead {
  tpe_score_stats st;
  int32_t n_top;       // entries of the chunk's list
  int32_t head;        // pass 2: first entry whose value is not chosen yet
  int32_t pad[2];
};
static_assert(sizeof(ChunkHead) == 80 && sizeof(tpe_top_entry) == 32 && sizeof(tpe_score_stats) == 64, "layout");

// np.argmax order of a score as one unsigned key, larger = better, 0 = no
// candidate: every NaN the largest key (they compare equal), then the f64 bits
// made monotone (-0 as +0, which compares equal to it); -inf maps above 0
__device__ __forceinline__ uint64_t score_key(double s) {
  if (s != s) return ~0ull;
  const uint64_t b = (uint64_t)__double_as_longlong(s + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_score(uint64_t k) {   // inverse (not for NaN keys)
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// a competitor of a selection round: key, tie-break index (lower wins), value, payload
struct Pick {
  uint64_t key;
  int64_t idx;
  double val;
  int32_t loc;
};
__device__ __forceinline__ bool beats(const Pick& a, const Pick& b) {
  return a.key > b.key || (a.key == b.key && a.key != 0 && a.idx < b.idx);
}
__device__ __forceinline__ Pick shfl_xor(const Pick& p, int m) {
  Pick o;
  o.key = (uint64_t)__shfl_xor((unsigned long long)p.key, m, 64);
  o.idx = (int64_t)__shfl_xor((long long)p.idx, m, 64);
  o.val = __shfl_xor(p.val, m, 64);
  o.loc = __shfl_xor(p.loc, m, 64);
  return o;
}
// the block's best competitor, the same in every thread (two barriers: `slot`
// is free again on return)
__device__ __forceinline__ Pick block_best(Pick p, Pick* slot) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const Pick o = shfl_xor(p, m);
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

// (n, mean, m2, min, max) of finite scores + the counts of the others
struct Stat {
  double mean, m2, mn, mx;
  int32_t n, n_nan, n_pinf, n_ninf;
};
__device__ __forceinline__ Stat stat_empty() { return Stat{0.0, 0.0, INFINITY, -INFINITY, 0, 0, 0, 0}; }
// Chan's update, a then b (64-bit counts: a problem has < 2^31 candidates)
__device__ __forceinline__ void chan(double& mean, double& m2, double na, double mean_b, double m2_b, double nb) {
  if (nb == 0.0) return;
  if (na == 0.0) { mean = mean_b; m2 = m2_b; return; }
  const double n = na + nb, d = mean_b - mean;
  mean = mean + d * (nb / n);
  m2 = m2 + m2_b + d * d * (na * nb / n);
}
__device__ __forceinline__ Stat stat_merge(Stat a, const Stat& b) {
  chan(a.mean, a.m2, (double)a.n, b.mean, b.m2, (double)b.n);
  a.n += b.n; a.n_nan += b.n_nan; a.n_pinf += b.n_pinf; a.n_ninf += b.n_ninf;
  a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx);
  return a;
}
__device__ __forceinline__ Stat stat_shfl_xor(const Stat& s, int m) {
  Stat o;
  o.mean = __shfl_xor(s.mean, m, 64); o.m2 = __shfl_xor(s.m2, m, 64);
  o.mn = __shfl_xor(s.mn, m, 64); o.mx = __shfl_xor(s.mx, m, 64);
  o.n = __shfl_xor(s.n, m, 64); o.n_nan = __shfl_xor(s.n_nan, m, 64);
  o.n_pinf = __shfl_xor(s.n_pinf, m, 64); o.n_ninf = __shfl_xor(s.n_ninf, m, 64);
  return o;
}

// one score into a lane's record (the sum of the finite ones in `sum`)
__device__ __forceinline__ void stat_add(Stat& s, double& sum, double sc) {
  if (sc != sc) ++s.n_nan;
  else if (sc == INFINITY) ++s.n_pinf;
  else if (sc == -INFINITY) ++s.n_ninf;
  else { ++s.n; sum += sc; s.mn = fmin(s.mn, sc); s.mx = fmax(s.mx, sc); }
}
// the block's record in thread 0 by a fixed tree: a butterfly over the lanes
// (the lower lane's record first, so both lanes of a pair compute the same
// one), then the four waves in order
__device__ __forceinline__ Stat block_stat(Stat s, Stat* wstat) {
  const int t = threadIdx.x;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const Stat o = stat_shfl_xor(s, m);
    s = (t & m) ? stat_merge(o, s) : stat_merge(s, o);
  }
  if ((t & 63) == 0) wstat[t >> 6] = s;
  __syncthreads();
  Stat a = wstat[0];
  if (t == 0)
    for (int i = 1; i < kThreads / 64; ++i) a = stat_merge(a, wstat[i]);
  return a;
}
// pass 2: a problem's chunk records merged — thread t its run of consecutive
// chunks in chunk order, the threads' records in thread order (fixed for a
// given S) — and written as the problem's statistics
__device__ __forceinline__ void merge_chunk_stats(const ChunkHead* hd, int slots, Stat* wstat, tpe_score_stats& o) {
  const int t = threadIdx.x, per = (slots + kThreads - 1) / kThreads;
  Stat s = stat_empty();
  for (int c = t * per; c < min(slots, (t + 1) * per); ++c) {
    const tpe_score_stats& a = hd[c].st;
    Stat b{a.mean, a.m2, a.min, a.max, (int32_t)a.n_finite, (int32_t)a.n_nan, (int32_t)a.n_posinf,
           (int32_t)a.n_neginf};
    s = stat_merge(s, b);
  }
  const Stat a = block_stat(s, wstat);
  if (t == 0) {
    o.n_finite = a.n; o.n_nan = a.n_nan; o.n_posinf = a.n_pinf; o.n_neginf = a.n_ninf;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    o.mean = a.n ? a.mean : nan; o.m2 = a.n ? a.m2 : 0.0; o.min = a.n ? a.mn : nan; o.max = a.n ? a.mx : nan;
  }
}
// pass 1: a lane's record completed (per-lane two-pass: the keys keep the
// scores, so m2 needs no second read), the block's record written to the chunk head
template <int N>
__device__ __forceinline__ void chunk_stats(Stat s, double sum, const uint64_t (&key)[N], Stat* wstat, ChunkHead* hd) {
  if (s.n) {
    s.mean = sum / (double)s.n;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double sc = key_score(key[j]);
      if (key[j] != 0 && key[j] != ~0ull && fabs(sc) < INFINITY) s.m2 += (sc - s.mean) * (sc - s.mean);
    }
  }
  const Stat a = block_stat(s, wstat);
  if (threadIdx.x == 0) {
    hd->st.n_finite = a.n; hd->st.n_nan = a.n_nan; hd->st.n_posinf = a.n_pinf; hd->st.n_neginf = a.n_ninf;
    hd->st.mean = a.mean; hd->st.m2 = a.m2; hd->st.min = a.mn; hd->st.max = a.mx;
  }
}

// does the problem fit its chunk slots and the candidate buffers?
__device__ __forceinline__ bool problem_ok(const tpe_problem& pr, int slots, int64_t total_cand) {
  return pr.n_cand >= 0 && (int64_t)pr.n_cand <= (int64_t)slots * TPE_REPORT_CHUNK && pr.cand_off >= 0 &&
         pr.cand_off + pr.n_cand <= total_cand;
}

// ---------------------------------------------------------------- pass 1
__global__ __launch_bounds__(kThreads) void k_report_chunk(const tpe_problem* __restrict__ problems, int slots,
                                                           int64_t total_cand, const double* __restrict__ cand,
                                                           const double* __restrict__ l_out,
                                                           const double* __restrict__ g_out, int k,
                                                           ChunkHead* __restrict__ heads,
                                                           tpe_top_entry* __restrict__ entries) {
  __shared__ Pick slot[kThreads / 64];
  __shared__ Stat wstat[kThreads / 64];
  const int p = blockIdx.x / slots, c = blockIdx.x % slots, t = threadIdx.x;
  const tpe_problem& pr = problems[p];
  const int n_cand = problem_ok(pr, slots, total_cand) ? pr.n_cand : 0;
  const int64_t off = pr.cand_off, base = pr.cand_base;
  const int first = c * TPE_REPORT_CHUNK;       // < 2^31: c < slots, slots * CHUNK < 2^31 + CHUNK (host check)
  ChunkHead* hd = heads + blockIdx.x;
  tpe_top_entry* out = entries + (int64_t)blockIdx.x * k;

  // thread t holds candidates first + j * 256 + t (coalesced 8-B loads)
  double val[kPer];
  uint64_t key[kPer];
  Stat s = stat_empty();
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = first + j * kThreads + t;
    val[j] = 0.0;
    key[j] = 0;
    if (i < n_cand) {
      val[j] = cand[off + i];
      const double sc = l_out[off + i] - g_out[off + i];
      key[j] = score_key(sc);
      stat_add(s, sum, sc);
    }
  }
  chunk_stats(s, sum, key, wstat, hd);

  // selection rounds: the best remaining key wins, every candidate with its value leaves
  int n_top = 0;
  for (int r = 0; r < k; ++r) {
    Pick b{0, 0, 0.0, 0};
#pragma unroll
    for (int j = 0; j < kPer; ++j)            // ascending index: strict > keeps the first of a tie
      if (key[j] > b.key) b = Pick{key[j], (int64_t)(first + j * kThreads + t), val[j], 0};
    const Pick w = block_best(b, slot);
    if (w.key == 0) break;                    // (block-uniform) fewer than k distinct values
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (val[j] == w.val || (int64_t)(first + j * kThreads + t) == w.idx) key[j] = 0;
    if (t == 0) {
      out[r].value = w.val;
      out[r].l = l_out[off + w.idx];
      out[r].g = g_out[off + w.idx];
      out[r].global_idx = base + w.idx;
    }
    n_top = r + 1;
  }
  if (t == 0) { hd->n_top = n_top; hd->head = 0; hd->pad[0] = hd->pad[1] = 0; }
}

// ---------------------------------------------------------------- pass 2
__global__ __launch_bounds__(kThreads) void k_report_merge(const tpe_problem* __restrict__ problems, int slots,
                                                           int64_t total_cand, int k, ChunkHead* __restrict__ heads,
                                                           const tpe_top_entry* __restrict__ entries,
                                                           tpe_top_entry* __restrict__ top, int32_t* __restrict__ n_top,
                                                           tpe_score_stats* __restrict__ stats) {
  __shared__ Pick slot[kThreads / 64];
  __shared__ Stat wstat[kThreads / 64];
  __shared__ double chosen[TPE_REPORT_MAX_K];
  const int p = blockIdx.x, t = threadIdx.x;
  const tpe_problem& pr = problems[p];
  const bool ok = problem_ok(pr, slots, total_cand);
  ChunkHead* hd = heads + (int64_t)p * slots;
  const tpe_top_entry* ent = entries + (int64_t)p * slots * k;
  tpe_top_entry* out = top + (int64_t)p * k;

  merge_chunk_stats(hd, slots, wstat, stats[p]);

  // merge of the chunk lists: a list is ranked and distinct, so its best
  // entry with a value not chosen yet is the first such entry (its head)
  int n = 0;
  for (int r = 0; r < k; ++r) {
    Pick b{0, 0, 0.0, 0};
    for (int c = t; c < slots; c += kThreads) {
      const int nc = hd[c].n_top;
      int h = hd[c].head;
      for (; h < nc; ++h) {
        const double v = ent[(int64_t)c * k + h].value;
        bool seen = false;
        for (int q = 0; q < r; ++q) seen |= chosen[q] == v;
        if (!seen) break;
      }
      hd[c].head = h;
      if (h < nc) {
        const tpe_top_entry& e = ent[(int64_t)c * k + h];
        const Pick x{score_key(e.l - e.g), e.global_idx, e.value, c * k + h};
        if (beats(x, b)) b = x;
      }
    }
    const Pick w = block_best(b, slot);
    if (w.key == 0) break;
    const int wc = w.loc / k;
    if (t == wc % kThreads) hd[wc].head = w.loc % k + 1;     // (a NaN value equals nothing: step past it)
    if (t == 0) {
      out[r] = ent[w.loc];
      chosen[r] = w.val;
    }
    n = r + 1;
    __syncthreads();
  }
  if (t == 0) n_top[p] = ok ? n : -1;
  for (int r = n + t; r < k; r += kThreads) out[r] = tpe_top_entry{0.0, 0.0, 0.0, -1};
}

int64_t chunk_slots(const tpe_batch* b) {
  if (b->n_problems <= 0 || b->total_cand <= 0) return 0;
  const int64_t per = (b->total_cand + b->n_problems - 1) / b->n_problems;
  return (per + TPE_REPORT_CHUNK - 1) / TPE_REPORT_CHUNK;
}

// tpe_report_profile / tpe_joint_report_profile: start / stop events of the two
// launches (profiling only)
struct Prof {
  int on, valid;
  hipEvent_t ev[4];
};
Prof g_prof = {0, 0, {nullptr, nullptr, nullptr, nullptr}};
Prof g_jprof = {0, 0, {nullptr, nullptr, nullptr, nullptr}};

int prof_call(Prof& pf, int32_t enable, double* last_ms, const char* none) {
  if (last_ms) {
    if (!pf.valid) return tpe_internal_fail(TPE_E_ARG, none);
    for (int i = 0; i < 2; ++i) {
      float ms = 0.f;
      hipError_t e = hipEventSynchronize(pf.ev[2 * i + 1]);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, pf.ev[2 * i], pf.ev[2 * i + 1]);
      if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
      last_ms[i] = (double)ms;
    }
  }
  if (enable && !pf.ev[0])
    for (int i = 0; i < 4; ++i) {
      const hipError_t e = hipEventCreate(&pf.ev[i]);
      if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
    }
  pf.on = enable ? 1 : 0;
  pf.valid = 0;
  return TPE_OK;
}

// ---------------------------------------------------------------- joint report
// (include/tpe_hip.h "Joint candidate report"): the same two passes over rows
// of `width` floats.  A lane keeps a score key and a row hash per candidate;
// the rows themselves stay in `cand` and are re-read where a hash matches.
static_assert(TPE_JOINT_REPORT_CHUNK == TPE_REPORT_CHUNK, "the joint report shares kPer and ChunkHead");
static_assert(sizeof(tpe_joint_top_entry) == 32, "layout");
constexpr int kMaxW = TPE_JOINT_WIDE_MAX_DIMS;

// equal rows (all coordinates ==, so no NaN) have equal hashes: -0 hashes as +0
__device__ __forceinline__ uint32_t hash_step(uint32_t h, float x) {
  h = (h ^ __float_as_uint(x + 0.0f)) * 0x9E3779B1u;
  return h ^ (h >> 15);
}
__device__ __forceinline__ uint32_t row_hash(const float* __restrict__ r, int W, bool vec4) {
  uint32_t h = 0x811C9DC5u;
  if (vec4) {                                  // W % 4 == 0 and the row 16-B aligned
#pragma nounroll
    for (int d = 0; d < W; d += 4) {
      const float4 v = *reinterpret_cast<const float4*>(r + d);
      h = hash_step(hash_step(hash_step(hash_step(h, v.x), v.y), v.z), v.w);
    }
  } else {
#pragma nounroll
    for (int d = 0; d < W; ++d) h = hash_step(h, r[d]);
  }
  return h;
}
// all W coordinates == (a NaN anywhere: false)
__device__ __forceinline__ bool rows_equal(const float* __restrict__ r, const float* w, int W) {
  bool eq = true;
#pragma nounroll
  for (int d = 0; d < W; ++d) eq &= r[d] == w[d];
  return eq;
}
__device__ __forceinline__ int problem_width(const tpe_joint_report_args& a, int p) {
  const int W = a.widths ? a.widths[p] : a.width;
  return min(max(W, 1), kMaxW);               // (the host checked its copy: never clamps a valid call)
}
__device__ __forceinline__ int64_t problem_off(const tpe_joint_report_args& a, int p, int W) {
  return a.cand_off ? a.cand_off[p] : (int64_t)p * a.n_cand * W;
}

__global__ __launch_bounds__(kThreads) void k_joint_report_chunk(const tpe_joint_report_args a, int slots, int k,
                                                                 ChunkHead* __restrict__ heads,
                                                                 tpe_joint_top_entry* __restrict__ entries) {
  __shared__ Pick slot[kThreads / 64];
  __shared__ Stat wstat[kThreads / 64];
  __shared__ float wrow[kMaxW];
  const int p = blockIdx.x / slots, c = blockIdx.x % slots, t = threadIdx.x;
  const int n_cand = a.n_cand, W = problem_width(a, p);
  const float* __restrict__ rows = a.cand + problem_off(a, p, W);
  const double* __restrict__ lp = a.l_out + (int64_t)p * n_cand;
  const double* __restrict__ gp = a.g_out + (int64_t)p * n_cand;
  const bool vec4 = (W & 3) == 0 && ((uintptr_t)rows & 15) == 0;
  const int first = c * TPE_JOINT_REPORT_CHUNK;      // < 2^31: c < slots = ceil(n_cand / CHUNK)
  ChunkHead* hd = heads + blockIdx.x;
  tpe_joint_top_entry* out = entries + (int64_t)blockIdx.x * k;

  // thread t holds candidates first + j * 256 + t (coalesced 8-B loads of l and g)
  uint64_t key[kPer];
  uint32_t hash[kPer];
  Stat s = stat_empty();
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = (int64_t)first + j * kThreads + t;
    key[j] = 0;
    hash[j] = 0;
    if (i < n_cand) {
      hash[j] = row_hash(rows + i * W, W, vec4);
      const double sc = lp[i] - gp[i];
      key[j] = score_key(sc);
      stat_add(s, sum, sc);
    }
  }
  chunk_stats(s, sum, key, wstat, hd);

  // selection rounds: the best remaining key wins; the winner and every
  // candidate whose row equals its row leave
  int n_top = 0;
  for (int r = 0; r < k; ++r) {
    Pick b{0, 0, 0.0, 0};
#pragma unroll
    for (int j = 0; j < kPer; ++j)            // ascending index: strict > keeps the first of a tie
      if (key[j] > b.key) b = Pick{key[j], (int64_t)first + j * kThreads + t, 0.0, (int32_t)hash[j]};
    const Pick w = block_best(b, slot);
    if (w.key == 0) break;                    // (block-uniform) fewer than k distinct rows
    if (t < W) wrow[t] = rows[w.idx * W + t];
    __syncthreads();                          // (the next write of wrow lies behind block_best's barriers)
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t i = (int64_t)first + j * kThreads + t;
      if (key[j] == 0) continue;
      if (i == w.idx) key[j] = 0;
      else if (hash[j] == (uint32_t)w.loc && rows_equal(rows + i * W, wrow, W)) key[j] = 0;
    }
    if (t == 0) out[r] = tpe_joint_top_entry{w.idx, lp[w.idx], gp[w.idx], (int64_t)(uint32_t)w.loc};
    n_top = r + 1;
  }
  if (t == 0) { hd->n_top = n_top; hd->head = 0; hd->pad[0] = hd->pad[1] = 0; }
}

__global__ __launch_bounds__(kThreads) void k_joint_report_merge(const tpe_joint_report_args a, int slots, int k,
                                                                 ChunkHead* __restrict__ heads,
                                                                 const tpe_joint_top_entry* __restrict__ entries,
                                                                 tpe_joint_top_entry* __restrict__ top,
                                                                 float* __restrict__ top_z, int32_t* __restrict__ n_top,
                                                                 tpe_score_stats* __restrict__ stats) {
  __shared__ Pick slot[kThreads / 64];
  __shared__ Stat wstat[kThreads / 64];
  __shared__ float chosen[TPE_REPORT_MAX_K * kMaxW];     // row q at [q * W ..]
  __shared__ uint32_t chosen_hash[TPE_REPORT_MAX_K];
  const int p = blockIdx.x, t = threadIdx.x;
  const int W = problem_width(a, p), zs = a.z_stride;
  const float* __restrict__ rows = a.cand + problem_off(a, p, W);
  ChunkHead* hd = heads + (int64_t)p * slots;
  const tpe_joint_top_entry* ent = entries + (int64_t)p * slots * k;
  tpe_joint_top_entry* out = top + (int64_t)p * k;
  float* zout = top_z + (int64_t)p * k * zs;

  merge_chunk_stats(hd, slots, wstat, stats[p]);

  // merge of the chunk lists: a list's best entry with a row not chosen yet is
  // the first such entry (its head)
  int n = 0;
  for (int r = 0; r < k; ++r) {
    Pick b{0, 0, 0.0, 0};
    for (int c = t; c < slots; c += kThreads) {
      const int nc = hd[c].n_top;
      int h = hd[c].head;
      for (; h < nc; ++h) {
        const tpe_joint_top_entry& e = ent[(int64_t)c * k + h];
        bool seen = false;
        for (int q = 0; q < r && !seen; ++q)
          seen = chosen_hash[q] == (uint32_t)e.reserved && rows_equal(rows + e.idx * W, chosen + q * W, W);
        if (!seen) break;
      }
      hd[c].head = h;
      if (h < nc) {
        const tpe_joint_top_entry& e = ent[(int64_t)c * k + h];
        const Pick x{score_key(e.l - e.g), e.idx, 0.0, c * k + h};
        if (beats(x, b)) b = x;
      }
    }
    const Pick w = block_best(b, slot);
    if (w.key == 0) break;
    const int wc = w.loc / k;
    if (t == wc % kThreads) hd[wc].head = w.loc % k + 1;     // (a NaN row equals nothing: step past it)
    if (t == 0) {
      const tpe_joint_top_entry e = ent[w.loc];
      out[r] = tpe_joint_top_entry{e.idx, e.l, e.g, 0};
      chosen_hash[r] = (uint32_t)e.reserved;
    }
    for (int d = t; d < zs; d += kThreads) {
      const float x = d < W ? rows[w.idx * W + d] : 0.f;
      if (d < W) chosen[r * W + d] = x;
      zout[(int64_t)r * zs + d] = x;
    }
    n = r + 1;
    __syncthreads();
  }
  if (t == 0) n_top[p] = n;
  for (int r = n + t; r < k; r += kThreads) out[r] = tpe_joint_top_entry{-1, 0.0, 0.0, 0};
  for (int i = n * zs + t; i < k * zs; i += kThreads) zout[i] = 0.f;
}

// the host check of one call: the chunk slots per problem, or -1
int64_t joint_slots(int32_t n_probs, int32_t n_cand, int32_t k) {
  if (n_probs < 1 || n_cand < 1 || k < 1 || k > TPE_REPORT_MAX_K) return -1;
  const int64_t slots = ((int64_t)n_cand + TPE_JOINT_REPORT_CHUNK - 1) / TPE_JOINT_REPORT_CHUNK;
  return slots * n_probs > INT32_MAX ? -1 : slots;
}

}  // namespace

extern "C" {

int tpe_report_profile(int32_t enable, double* last_ms) {
  return prof_call(g_prof, enable, last_ms, "tpe_report_profile: no profiled tpe_report to read");
}

int tpe_report_scratch_bytes(int64_t n_chunks_total, int32_t k, uint64_t* bytes) {
  if (!bytes || n_chunks_total < 0 || k < 1 || k > TPE_REPORT_MAX_K)
    return tpe_internal_fail(TPE_E_ARG, "tpe_report_scratch_bytes: bad arguments");
  *bytes = (uint64_t)n_chunks_total * (sizeof(ChunkHead) + (uint64_t)k * sizeof(tpe_top_entry));
  return TPE_OK;
}

int tpe_report(const tpe_batch* b, int32_t k, tpe_top_entry* top, int32_t* n_top, tpe_score_stats* stats,
               void* scratch, uint64_t scratch_bytes, void* stream) {
  tpe_internal_epoch_bump();
  if (!b) return tpe_internal_fail(TPE_E_ARG, "tpe_report: null batch");
  if (k < 1 || k > TPE_REPORT_MAX_K) return tpe_internal_fail(TPE_E_ARG, "tpe_report: k outside [1, TPE_REPORT_MAX_K]");
  if (b->n_problems < 0 || b->total_cand < 0) return tpe_internal_fail(TPE_E_ARG, "tpe_report: negative count");
  if (!(b->flags & TPE_BATCH_WRITE_CAND))
    return tpe_internal_fail(TPE_E_ARG, "tpe_report: the batch did not store its candidates (TPE_BATCH_WRITE_CAND)");
  if (!b->cand || !b->l_out || !b->g_out) return tpe_internal_fail(TPE_E_ARG, "tpe_report: null cand / l_out / g_out");
  if (b->n_problems == 0) return TPE_OK;
  if (!b->problems || !top || !n_top || !stats) return tpe_internal_fail(TPE_E_ARG, "tpe_report: null problems / outputs");
  const int64_t slots = chunk_slots(b), chunks = slots * b->n_problems;
  if (slots * TPE_REPORT_CHUNK > (int64_t)INT32_MAX + TPE_REPORT_CHUNK || chunks > INT32_MAX)
    return tpe_internal_fail(TPE_E_ARG, "tpe_report: too many candidates");
  const uint64_t need = (uint64_t)chunks * (sizeof(ChunkHead) + (uint64_t)k * sizeof(tpe_top_entry));
  if (scratch_bytes < need || (need && !scratch)) return tpe_internal_fail(TPE_E_ARG, "tpe_report: scratch too small");
  ChunkHead* heads = (ChunkHead*)scratch;
  tpe_top_entry* entries = (tpe_top_entry*)((char*)scratch + (uint64_t)chunks * sizeof(ChunkHead));
  const bool timed = g_prof.on && chunks;
  if (timed) {
    hipExtLaunchKernelGGL(k_report_chunk, dim3((unsigned)chunks), dim3(kThreads), 0u, (hipStream_t)stream,
                          g_prof.ev[0], g_prof.ev[1], 0u, b->problems, (int)slots, b->total_cand, b->cand, b->l_out,
                          b->g_out, (int)k, heads, entries);
    hipExtLaunchKernelGGL(k_report_merge, dim3((unsigned)b->n_problems), dim3(kThreads), 0u, (hipStream_t)stream,
                          g_prof.ev[2], g_prof.ev[3], 0u, b->problems, (int)slots, b->total_cand, (int)k, heads,
                          entries, top, n_top, stats);
    g_prof.valid = 1;
  } else {
    if (chunks)
      hipLaunchKernelGGL(k_report_chunk, dim3((unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, b->problems,
                         (int)slots, b->total_cand, b->cand, b->l_out, b->g_out, (int)k, heads, entries);
    hipLaunchKernelGGL(k_report_merge, dim3((unsigned)b->n_problems), dim3(kThreads), 0, (hipStream_t)stream,
                       b->problems, (int)slots, b->total_cand, (int)k, heads, entries, top, n_top, stats);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

int tpe_joint_report_profile(int32_t enable, double* last_ms) {
  return prof_call(g_jprof, enable, last_ms, "tpe_joint_report_profile: no profiled tpe_joint_report to read");
}

int tpe_joint_report_scratch_bytes(int32_t n_probs, int32_t n_cand, int32_t k, uint64_t* bytes) {
  const int64_t slots = joint_slots(n_probs, n_cand, k);
  if (!bytes || slots < 0) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report_scratch_bytes: bad arguments");
  *bytes = (uint64_t)(slots * n_probs) * (sizeof(ChunkHead) + (uint64_t)k * sizeof(tpe_joint_top_entry));
  return TPE_OK;
}

int tpe_joint_report(const tpe_joint_report_args* a, int32_t k, tpe_joint_top_entry* top, float* top_z,
                     int32_t* n_top, tpe_score_stats* stats, void* scratch, uint64_t scratch_bytes, void* stream) {
  tpe_internal_epoch_bump();
  if (!a) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: null args");
  if (k < 1 || k > TPE_REPORT_MAX_K)
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: k outside [1, TPE_REPORT_MAX_K]");
  if (a->n_probs < 1 || a->n_cand < 1) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: n_probs / n_cand < 1");
  if (!a->cand || !a->l_out || !a->g_out) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: null cand / l_out / g_out");
  if (!top || !top_z || !n_top || !stats) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: null outputs");
  if (a->widths && !a->host_widths)
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: widths without host_widths");
  int32_t wmax = a->width;
  if (a->widths) {
    wmax = 0;
    for (int32_t p = 0; p < a->n_probs; ++p) {
      const int32_t w = a->host_widths[p];
      if (w < 1 || w > kMaxW) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: a width outside [1, 64]");
      wmax = w > wmax ? w : wmax;
    }
  } else if (wmax < 1 || wmax > kMaxW) {
    return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: width outside [1, 64]");
  }
  if (a->z_stride < wmax) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: z_stride below the largest width");
  const int64_t slots = joint_slots(a->n_probs, a->n_cand, k);
  if (slots < 0) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: too many chunks");
  const int64_t chunks = slots * a->n_probs;
  const uint64_t need = (uint64_t)chunks * (sizeof(ChunkHead) + (uint64_t)k * sizeof(tpe_joint_top_entry));
  if (!scratch || scratch_bytes < need) return tpe_internal_fail(TPE_E_ARG, "tpe_joint_report: scratch too small");
  ChunkHead* heads = (ChunkHead*)scratch;
  tpe_joint_top_entry* entries = (tpe_joint_top_entry*)((char*)scratch + (uint64_t)chunks * sizeof(ChunkHead));
  tpe_joint_report_args dev = *a;
  dev.host_widths = nullptr;
  if (g_jprof.on) {
    hipExtLaunchKernelGGL(k_joint_report_chunk, dim3((unsigned)chunks), dim3(kThreads), 0u, (hipStream_t)stream,
                          g_jprof.ev[0], g_jprof.ev[1], 0u, dev, (int)slots, (int)k, heads, entries);
    hipExtLaunchKernelGGL(k_joint_report_merge, dim3((unsigned)a->n_probs), dim3(kThreads), 0u, (hipStream_t)stream,
                          g_jprof.ev[2], g_jprof.ev[3], 0u, dev, (int)slots, (int)k, heads, entries, top, top_z, n_top,
                          stats);
    g_jprof.valid = 1;
  } else {
    hipLaunchKernelGGL(k_joint_report_chunk, dim3((unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, dev,
                       (int)slots, (int)k, heads, entries);
    hipLaunchKernelGGL(k_joint_report_merge, dim3((unsigned)a->n_probs), dim3(kThreads), 0, (hipStream_t)stream, dev,
                       (int)slots, (int)k, heads, entries, top, top_z, n_top, stats);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tpe_internal_fail(TPE_E_HIP, hipGetErrorString(e));
  return TPE_OK;
}

}  // extern "C"
