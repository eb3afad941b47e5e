// lazy_scan_ubench.cpp — stand-alone check and timing of the host selection of
// a lazy categorical (hyperopt_amd/csrc/tpe_lazy_host.h), plain C++:
//   g++ -std=c++17 -O3 -I hyperopt_amd/csrc tools/ubench/lazy_scan_ubench.cpp -o lazy_scan_ubench
//   (checked build: -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all)
//
//   lazy_scan_ubench            the built-in cases against a full scan of every
//                               candidate, then the cost of a draw (the source of
//                               kLazyHostBudget in tpe_kernels.hip)
//   lazy_scan_ubench FILE       the cases of FILE (tests/test_lazy_host.py), one
//                               result line each:
//     case:   key0 key1 ctr2 ctr3 cand_base n_cand K budget  cum[K]  l[K]  g[K]
//     result: draws score l g value idx global_idx   (draws = -1: not settled;
//             floating-point numbers in C99 hexadecimal, "nan" for a NaN)
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "tpe_lazy_host.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct Case {
  uint32_t key0, key1, ctr2, ctr3;
  int64_t cand_base;
  int32_t n_cand;
  std::vector<double> cum, l, g;
};

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }
static bool same(const tpe_result& a, const tpe_result& b) {
  return same_bits(a.score, b.score) && same_bits(a.l, b.l) && same_bits(a.g, b.g) && same_bits(a.value, b.value) &&
         a.idx == b.idx && a.global_idx == b.global_idx;
}

// the selection by definition: every candidate drawn, the best by
// tpe_lazy_better; *need: the draws after which the stopping rule holds (the
// fewest a budget must allow), n_cand when it never does
static tpe_result full_scan(const Case& c, int64_t* need) {
  const int K = (int)c.cum.size();
  std::vector<int64_t> first((size_t)K, -1);
  tpe_result r{0, 0, 0, 0, -1, -1};
  *need = c.n_cand;
  bool settled = false;
  for (int64_t i = 0; i < c.n_cand; ++i) {
    const int k = tpe_lazy_category(c.key0, c.key1, c.ctr2, c.ctr3, c.cand_base, i, K, c.cum.data(), 1);
    if (first[(size_t)k] < 0) first[(size_t)k] = i;
    const double s = c.l[(size_t)k] - c.g[(size_t)k];
    if (tpe_lazy_better(s, i, r.score, r.idx)) r = tpe_result{s, c.l[(size_t)k], c.g[(size_t)k], (double)k, i, c.cand_base + i};
    if (settled) continue;
    bool more = false;
    for (int j = 0; j < K; ++j) {
      const bool drawable = c.cum[(size_t)j] > (j ? c.cum[(size_t)j - 1] : 0.0);
      more = more || (first[(size_t)j] < 0 && drawable &&
                      tpe_lazy_better(c.l[(size_t)j] - c.g[(size_t)j], INT64_MAX, r.score, r.idx));
    }
    if (!more) { settled = true; *need = i + 1; }
  }
  return r;
}

static int64_t run(const Case& c, int64_t budget, tpe_result* out) {
  return tpe_lazy_host_select(c.key0, c.key1, c.ctr2, c.ctr3, c.cand_base, c.n_cand, (int)c.cum.size(), c.cum.data(), 1,
                              c.l.data(), c.g.data(), 1, budget, out);
}

static void check_case(const char* name, const Case& c) {
  int64_t need = 0;
  const tpe_result ref = full_scan(c, &need);
  tpe_result got{9, 9, 9, 9, 9, 9};
  const int64_t d = run(c, INT64_MAX, &got);
  CHECK(d == need && same(got, ref));
  if (!(d == need && same(got, ref)))
    fprintf(stderr, "  case %s: draws %" PRId64 " (need %" PRId64 "), idx %" PRId64 " vs %" PRId64 "\n", name, d, need,
            got.idx, ref.idx);
  // the budget: settled exactly from `need` draws on, untouched output below
  if (need > 0) {
    tpe_result low{7, 7, 7, 7, 7, 7};
    CHECK(run(c, need - 1, &low) == -1 && low.idx == 7);
    CHECK(run(c, need, &got) == need && same(got, ref));
  }
}

static Case make(int K, uint32_t seed, int64_t base, int32_t n_cand) {
  Case c;
  c.key0 = 0x9E3779B9u * (seed + 1); c.key1 = 0x85EBCA6Bu ^ seed; c.ctr2 = 3 + seed; c.ctr3 = 2000 + seed;
  c.cand_base = base; c.n_cand = n_cand;
  double acc = 0;
  std::vector<double> w((size_t)K);
  for (int k = 0; k < K; ++k) { w[(size_t)k] = 1.0 + ((k * 7 + seed) % 5); acc += w[(size_t)k]; }
  double run_sum = 0;
  for (int k = 0; k < K; ++k) {
    run_sum += w[(size_t)k];
    c.cum.push_back(k == K - 1 ? 1.0 : run_sum / acc);
    c.l.push_back(std::log(w[(size_t)k] / acc));
    c.g.push_back(std::log((1.0 + ((k * 3 + seed) % 7)) / (4.0 * K)));
  }
  return c;
}

static void builtin_cases() {
  const int64_t bases[] = {0, 12345677, ((int64_t)1 << 32) + 5};
  for (int K : {2, 3, 64})
    for (int64_t base : bases)
      for (uint32_t seed = 0; seed < 3; ++seed) check_case("K", make(K, seed, base, 1 << 16));
  {                                           // equal scores: the earlier first index wins
    Case c = make(3, 1, 7, 4096);
    c.l = {0.5, 0.5, 0.5}; c.g = {0.25, 0.25, 0.25};
    check_case("equal", c);
  }
  {                                           // a NaN score comes first
    Case c = make(3, 2, 0, 4096);
    c.l[1] = std::numeric_limits<double>::quiet_NaN();
    check_case("nan", c);
  }
  {                                           // a zero-mass category with the best score never keeps the scan alive
    Case c = make(3, 0, 1, 4096);
    c.cum = {0.5, 0.5, 1.0};
    c.l = {0.0, 100.0, -1.0}; c.g = {0.0, 0.0, 0.0};
    int64_t need = 0;
    (void)full_scan(c, &need);
    CHECK(need < 64);
    check_case("zero mass", c);
  }
  for (int32_t n : {40, 5000}) {              // the best category rare (1/300): n_cand below and above its first draw
    Case c = make(2, 3, 9, n);
    c.cum = {1.0 - 1.0 / 300, 1.0};
    c.l = {0.0, 5.0}; c.g = {0.0, 0.0};
    check_case("rare", c);
  }
  check_case("one candidate", make(3, 4, 11, 1));
  check_case("no candidate", make(3, 4, 11, 0));
}

static void timing() {
  // the best category never drawn within the scan (mass 2^-40): every draw is
  // made and none settles, the budget's worst case
  for (int K : {3, 64}) {
    Case c = make(K, 5, 0, 1 << 22);
    for (int k = 0; k < K - 1; ++k) c.cum[(size_t)k] = (k + 1) * (1.0 - std::ldexp(1.0, -40)) / (K - 1);
    c.l[(size_t)K - 1] = 50.0;
    const int64_t budget = 1 << 20;
    tpe_result r{0, 0, 0, 0, 0, 0};
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      const int64_t d = run(c, budget, &r);
      const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
      CHECK(d == -1);
      best = ns < best ? ns : best;
    }
    printf("lazy_scan_ubench: K = %d: %.1f ns a draw (best of 5 scans of %" PRId64 " draws)\n", K,
           best / (double)budget, budget);
  }
}

static int run_file(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "lazy_scan_ubench: cannot open %s\n", path); return 2; }
  for (;;) {
    Case c;
    int K = 0;
    int64_t budget = 0;
    const int n = fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd64 " %" SCNd32 " %d %" SCNd64,
                         &c.key0, &c.key1, &c.ctr2, &c.ctr3, &c.cand_base, &c.n_cand, &K, &budget);
    if (n == EOF) break;
    if (n != 8 || K < 1 || K > 64) { fprintf(stderr, "lazy_scan_ubench: bad case header\n"); fclose(f); return 2; }
    for (std::vector<double>* v : {&c.cum, &c.l, &c.g})
      for (int k = 0; k < K; ++k) {
        char tok[64];
        if (fscanf(f, "%63s", tok) != 1) { fprintf(stderr, "lazy_scan_ubench: short case\n"); fclose(f); return 2; }
        v->push_back(strtod(tok, nullptr));
      }
    tpe_result r{0, 0, 0, 0, -1, -1};
    const int64_t d = run(c, budget, &r);
    printf("%" PRId64 " %a %a %a %a %" PRId64 " %" PRId64 "\n", d, r.score, r.l, r.g, r.value, (int64_t)r.idx,
           (int64_t)r.global_idx);
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return run_file(argv[1]);
  builtin_cases();
  if (g_fail) { printf("lazy_scan_ubench: %d checks failed\n", g_fail); return 1; }
  printf("lazy_scan_ubench: ok\n");
  timing();
  return g_fail ? 1 : 0;
}
