// keystore_test.cpp — stand-alone test of the fit keys' copy / compare / cap
// logic (hyperopt_amd/csrc/tpe_keystore.h).  Built with
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I hyperopt_amd/csrc tools/ubench/keystore_test.cpp -o tools/ubench/keystore_test
// and run as a plain executable (tests/test_resident_host.py does both).
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "tpe_keystore.h"

using tpe_keystore::Seg;
using tpe_keystore::Store;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

struct Head {
  int32_t family, flags;
  double low, high;
  int64_t n_obs;
};

static int segs_of(const Head& h, const std::vector<int64_t>& tids, const std::vector<double>& vals,
                   const std::vector<double>* prior, Seg* out) {
  int n = 0;
  out[n++] = Seg{&h, sizeof(h)};
  out[n++] = Seg{tids.data(), tids.size() * sizeof(int64_t)};
  out[n++] = Seg{vals.data(), vals.size() * sizeof(double)};
  out[n++] = Seg{prior ? prior->data() : nullptr, prior ? prior->size() * sizeof(double) : 0};
  return n;
}

int main() {
  std::atomic<int64_t> total{0};
  Seg s[8];
  {
    Store st(&total, tpe_keystore::kCapBytes);
    st.reserve_slots(3);
    CHECK(st.n_slots() == 3);
    Head h;
    memset(&h, 0, sizeof(h));
    h.family = 1; h.low = -1.0; h.high = 2.0; h.n_obs = 1000;
    std::vector<int64_t> tids(1000);
    std::iota(tids.begin(), tids.end(), 7);
    std::vector<double> vals(1000);
    for (size_t i = 0; i < vals.size(); ++i) vals[i] = 0.25 * (double)i;

    // an empty slot matches nothing; a slot past the end neither
    int n = segs_of(h, tids, vals, nullptr, s);
    CHECK(!st.match(0, s, n));
    CHECK(!st.match(99, s, n));
    CHECK(!st.store(99, s, n));
    CHECK(st.store(0, s, n));
    st.set_gen(0, 5);
    CHECK(st.match(0, s, n) && st.gen(0) == 5 && st.valid(0));
    CHECK(total.load() == st.bytes() && st.bytes() == (int64_t)(sizeof(h) + 16000));

    // the same content at other addresses matches; the key is a private copy
    {
      std::vector<int64_t> t2(tids);
      std::vector<double> v2(vals);
      Head h2 = h;
      Seg s2[8];
      const int n2 = segs_of(h2, t2, v2, nullptr, s2);
      CHECK(st.match(0, s2, n2));
    }
    // one element changed in place: the first, the last, of either array
    vals[0] = -3.0;
    CHECK(!st.match(0, s, n));
    vals[0] = 0.0;
    CHECK(st.match(0, s, n));
    vals[999] += 1.0;
    CHECK(!st.match(0, s, n));
    vals[999] -= 1.0;
    tids[0] = 6;
    CHECK(!st.match(0, s, n));
    tids[0] = 7;
    tids[999] += 1;
    CHECK(!st.match(0, s, n));
    tids[999] -= 1;
    CHECK(st.match(0, s, n));
    // a scalar of the head
    h.high = 2.5;
    CHECK(!st.match(0, s, n));
    h.high = 2.0;
    // unequal sizes: one element more, one less, an extra piece, a piece absent
    tids.push_back(2000); vals.push_back(1.0);
    n = segs_of(h, tids, vals, nullptr, s);
    CHECK(!st.match(0, s, n));
    // growth: the longer key replaces the shorter
    CHECK(st.store(0, s, n) && st.match(0, s, n));
    CHECK(total.load() == (int64_t)(sizeof(h) + 16016));
    tids.resize(10); vals.resize(10);
    n = segs_of(h, tids, vals, nullptr, s);
    CHECK(!st.match(0, s, n));
    // shrink
    CHECK(st.store(0, s, n) && st.match(0, s, n));
    CHECK(total.load() == (int64_t)(sizeof(h) + 160) && st.bytes() == total.load());
    std::vector<double> prior{0.25, 0.75};
    Seg sp[8];
    const int np = segs_of(h, tids, vals, &prior, sp);
    CHECK(!st.match(0, sp, np));            // the prior present, absent in the key
    CHECK(!st.match(0, s, n - 1));          // a piece fewer
    CHECK(st.store(1, sp, np) && st.match(1, sp, np) && !st.match(1, s, n));
    prior[1] = 0.5;
    CHECK(!st.match(1, sp, np));
    // zero-length arrays
    std::vector<int64_t> t0;
    std::vector<double> v0;
    n = segs_of(h, t0, v0, nullptr, s);
    CHECK(st.store(2, s, n) && st.match(2, s, n));
    // invalidate keeps the generation, drops the evidence
    st.set_gen(2, 9);
    st.invalidate(2);
    CHECK(!st.match(2, s, n) && st.gen(2) == 9 && !st.valid(2));
    st.clear();
    CHECK(total.load() == 0 && st.gen(0) == 0 && !st.match(1, sp, np));
  }
  {
    // the cap (a small one, and the real one): a key past it is refused and
    // leaves the slot empty; what was charged is given back
    Store st(&total, 1000);
    st.reserve_slots(2);
    std::vector<unsigned char> a(600, 1), b(600, 2), c(100, 3);
    Seg sa{a.data(), a.size()}, sb{b.data(), b.size()}, sc{c.data(), c.size()};
    CHECK(st.store(0, &sa, 1));
    CHECK(!st.store(1, &sb, 1) && !st.valid(1) && total.load() == 600);
    CHECK(st.store(1, &sc, 1) && total.load() == 700);
    CHECK(!st.store(1, &sb, 1) && total.load() == 600 && !st.match(1, &sc, 1));   // (the old key went too)
    CHECK(st.store(0, &sb, 1) && st.match(0, &sb, 1) && total.load() == 600);      // same size: replaced
    // two stores share the process-wide count
    Store other(&total, 1000);
    other.reserve_slots(1);
    CHECK(!other.store(0, &sa, 1) && total.load() == 600);
    CHECK(other.store(0, &sc, 1) && total.load() == 700);
  }
  CHECK(total.load() == 0);                 // (the destructors gave everything back)
  {
    Store st(&total, tpe_keystore::kCapBytes);
    st.reserve_slots(3);
    std::vector<unsigned char> big((size_t)40 << 20, 7);
    Seg sb{big.data(), big.size()};
    CHECK(st.store(0, &sb, 1) && st.match(0, &sb, 1));
    CHECK(!st.store(1, &sb, 1));            // 80 MB > 64 MB
    big[big.size() - 1] = 8;
    CHECK(!st.match(0, &sb, 1));
    CHECK(total.load() == (int64_t)big.size());
  }
  CHECK(total.load() == 0);
  if (g_fail) {
    fprintf(stderr, "keystore_test: %d failure(s)\n", g_fail);
    return 1;
  }
  puts("keystore_test: ok");
  return 0;
}
