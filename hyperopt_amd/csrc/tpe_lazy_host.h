// Host selection of a lazy categorical problem (TPE_F_CAT_LAZY): what the
// device's select_cat_lazy (tpe_kernels.hip) computes, on the host.  Plain C++,
// no HIP runtime: included by tpe_kernels.hip (a resident level's fused hit,
// level_run_impl) and by tools/ubench/lazy_scan_ubench.cpp.
//
// A draw is one Philox-4x32-10 block of the candidate's global index (integer
// only), u01d of its first two words, and a binary search in the CDF — the
// device's draw_category, operation for operation in IEEE f64.  The scan keeps
// each category's first index and stops by the device's rule: once no undrawn
// drawable category could beat the best, in better()'s order (NaN first, then
// the score, then the smaller index).  The device applies the rule after every
// 4096 draws, the host whenever a category is drawn for the first time (the
// rule's inputs change at no other draw); both stop only when every later draw
// must lose, so both return the argmax of the full scan.
#ifndef TPE_LAZY_HOST_H
#define TPE_LAZY_HOST_H

#include <stdint.h>

#include "../../include/tpe_hip.h"
#include "tpe_device_rng.h"

// np.argmax order of (score, index): better() of the kernels
inline bool tpe_lazy_better(double s, int64_t i, double bs, int64_t bi) {
  if (bi < 0) return i >= 0;
  if (i < 0) return false;
  const bool n = s != s, bn = bs != bs;
  if (n || bn) return n && (!bn || i < bi);
  return s > bs || (s == bs && i < bi);
}

// category of local candidate i: the first k with u < cum[k * cs] (draw_category)
inline int tpe_lazy_category(uint32_t key0, uint32_t key1, uint32_t ctr2, uint32_t ctr3, int64_t cand_base, int64_t i,
                             int K, const double* cum, int cs) {
  const uint64_t g = (uint64_t)cand_base + (uint64_t)i;
  const U4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), ctr2, ctr3, key0, key1);
  const double u1 = u01d(r.x, r.y);
  int a = 0, b = K - 1;
  while (a < b) { const int m = (a + b) >> 1; if (u1 < cum[(int64_t)m * cs]) b = m; else a = m + 1; }
  return a;
}

// The problem's per-call words, its candidate range, its K <= 64 categories:
// the CDF cum[k * cs] (the sampler rows' first column: cs = 8), the scores' l
// and g (l[k * ls], g[k * ls]: the comp64 rows' first column: ls = 4).  Scans
// at most `budget` draws.  Returns the number of draws scanned and the full
// result in *out when the selection settled within them (0 draws: n_cand = 0,
// idx = -1), else -1 with *out untouched.
inline int64_t tpe_lazy_host_select(uint32_t key0, uint32_t key1, uint32_t ctr2, uint32_t ctr3, int64_t cand_base,
                                    int32_t n_cand, int K, const double* cum, int cs, const double* l, const double* g,
                                    int ls, int64_t budget, tpe_result* out) {
  if (K < 1 || K > 64) return -1;
  int64_t first[64];
  double score[64];
  for (int c = 0; c < K; ++c) { first[c] = -1; score[c] = l[(int64_t)c * ls] - g[(int64_t)c * ls]; }
  double bs = 0.0;
  int64_t bi = -1;
  int bc = -1;
  bool settled = n_cand <= 0;
  int64_t i = 0;
  const int64_t n = n_cand < budget ? n_cand : budget;
  for (; i < n && !settled; ++i) {
    const int c = tpe_lazy_category(key0, key1, ctr2, ctr3, cand_base, i, K, cum, cs);
    if (first[c] >= 0) continue;
    first[c] = i;
    if (tpe_lazy_better(score[c], i, bs, bi)) { bs = score[c]; bi = i; bc = c; }
    bool more = false;
    for (int k = 0; k < K && !more; ++k) {
      const bool drawable = cum[(int64_t)k * cs] > (k ? cum[(int64_t)(k - 1) * cs] : 0.0);
      more = first[k] < 0 && drawable && tpe_lazy_better(score[k], INT64_MAX, bs, bi);
    }
    settled = !more;
  }
  if (!settled && i < n_cand) return -1;          // (every candidate scanned settles it too)
  tpe_result r;
  r.score = bi >= 0 ? bs : 0.0;
  r.l = bi >= 0 ? l[(int64_t)bc * ls] : 0.0;
  r.g = bi >= 0 ? g[(int64_t)bc * ls] : 0.0;
  r.value = bi >= 0 ? (double)bc : 0.0;
  r.idx = bi;
  r.global_idx = bi >= 0 ? cand_base + bi : -1;
  *out = r;
  return i;
}

#endif  // TPE_LAZY_HOST_H
