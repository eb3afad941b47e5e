// Device helpers shared by the sampling kernels (tpe_kernels.hip, tpe_joint.hip):
// the Philox-4x32-10 block function, the open-interval uniforms made from its
// words, and the f32 inverse normal CDF every f32 draw inverts through.
// Include after <hip/hip_runtime.h>, outside any namespace.  The Philox block
// and u01d are integer and IEEE f64 code that the host runs too (a resident
// level's fused hit selects its lazy categoricals there, tpe_lazy_host.h): a
// plain C++ compiler sees only those two.
#ifndef TPE_DEVICE_RNG_H
#define TPE_DEVICE_RNG_H

#include <stdint.h>

#ifdef __HIPCC__
#define TPE_HD __host__ __device__ __forceinline__
#define TPE_UNROLL _Pragma("unroll")
#else
#define TPE_HD inline
#define TPE_UNROLL
#endif

// ---------------------------------------------------------------- Philox
struct U4 { uint32_t x, y, z, w; };

TPE_HD U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                        uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  TPE_UNROLL
  for (int r = 0; r < 10; ++r) {
    // one 32x32 -> 64-bit product per multiplier (v_mad_u64_u32) instead of a
    // mul_hi / mul_lo pair
    const uint64_t p0 = (uint64_t)M0 * (uint64_t)c0, p1 = (uint64_t)M1 * (uint64_t)c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return U4{c0, c1, c2, c3};
}

// open-interval uniforms
// (u01d: IEEE f64 operations only, the same value on the host and on the device)
TPE_HD double u01d(uint32_t a, uint32_t b) {
  const uint64_t m = ((uint64_t)a << 21) ^ (uint64_t)(b >> 11);   // 53 bits
  return ((double)m + 0.5) * 1.1102230246251565e-16;
}
#ifdef __HIPCC__
// 23-bit float uniform in [2^-24, 1 - 2^-24]: (k + 0.5) is exact, so never 0 or 1
__device__ __forceinline__ float u01f(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }
// 32-bit uniform as a double in (0, 1) (exact)
__device__ __forceinline__ double u01w(uint32_t a) { return ((double)a + 0.5) * 2.3283064365386963e-10; }

// Phi^-1(pr) in f32 = -sqrt2 erfinv(1 - 2 pr), erfinv by Giles' single-precision
// approximation ("Approximating the erfinv function", GPU Computing Gems 2010)
// with its log argument (1 - x)(1 + x) = 4 pr (1 - pr) formed from pr itself (no
// cancellation in the tails), and a third branch below the f32 uniforms (pr <
// 2.8e-8, see there).  Relative error <= 3e-7 for every normal f32 pr in
// [1e-38, 1 - 2^-24] (checked against scipy.special.ndtri; tests/draw_ref.py
// brackets every device draw by this bound); one v_log_f32, the tail branches
// add a sqrt.  Every f32 draw inverts through this one function.
__device__ __forceinline__ float ndtri_f32(float pr) {
  const float x = 1.f - 2.f * pr;
  float w = -__logf(4.f * pr * (1.f - pr));
  float q;
  if (w < 5.f) {
    w -= 2.5f;
    q = 2.81022636e-08f;
    q = __builtin_fmaf(q, w, 3.43273939e-07f); q = __builtin_fmaf(q, w, -3.5233877e-06f);
    q = __builtin_fmaf(q, w, -4.39150654e-06f); q = __builtin_fmaf(q, w, 0.00021858087f);
    q = __builtin_fmaf(q, w, -0.00125372503f); q = __builtin_fmaf(q, w, -0.00417768164f);
    q = __builtin_fmaf(q, w, 0.246640727f); q = __builtin_fmaf(q, w, 1.50140941f);
  } else if (w >= 16.f) {
    // pr < 2.8e-8: below every f32 uniform, past the range Giles' tail
    // polynomial was fitted on (it is 4e-4 off at pr = 1e-10 and 3e-2 at
    // 1e-14), but reached by pr = fa + u (fb - fa) of a truncated component
    // whose visible mass fb - fa is small.  q(s), s = sqrt(w), by a degree-9
    // least-squares fit on s in [3.95, 9.28] (pr from 4e-8 down to 1e-38)
    // against scipy.special.ndtri: 1.7e-7 in f32 arithmetic.  Below 1.2e-38 (pr
    // subnormal: fa rounded to 0 in f32 and fb - fa tiny) pr itself has lost
    // bits and the error grows to about 2e-6 of z; pr = 0 (a visible mass
    // under 1e-38: not drawn in practice) gives an infinite z of no meaning,
    // which only the callers' clip to the bounds catches.
    w = __builtin_sqrtf(w) - 6.5f;
    q = -4.196834879621747e-09f;
    q = __builtin_fmaf(q, w, 2.784403108080369e-08f); q = __builtin_fmaf(q, w, -9.715248694419643e-08f);
    q = __builtin_fmaf(q, w, 5.151761115484987e-07f); q = __builtin_fmaf(q, w, -2.931430344688124e-06f);
    q = __builtin_fmaf(q, w, 1.1722268027369864e-05f); q = __builtin_fmaf(q, w, -1.0785219274112023e-05f);
    q = __builtin_fmaf(q, w, -0.0005107762990519404f); q = __builtin_fmaf(q, w, 1.009109377861023f);
    q = __builtin_fmaf(q, w, 6.364593505859375f);
  } else {
    w = __builtin_sqrtf(w) - 3.f;
    q = -0.000200214257f;
    q = __builtin_fmaf(q, w, 0.000100950558f); q = __builtin_fmaf(q, w, 0.00134934322f);
    q = __builtin_fmaf(q, w, -0.00367342844f); q = __builtin_fmaf(q, w, 0.00573950773f);
    q = __builtin_fmaf(q, w, -0.0076224613f); q = __builtin_fmaf(q, w, 0.00943887047f);
    q = __builtin_fmaf(q, w, 1.00167406f); q = __builtin_fmaf(q, w, 2.83297682f);
  }
  return -1.41421356237309505f * (q * x);
}
#endif  // __HIPCC__

#endif  // TPE_DEVICE_RNG_H
