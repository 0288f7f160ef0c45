// rp_plan.hpp -- the arithmetic of librp_plan.so (include/plan/rp_plan.h), shared by its kernels, and the argument checks.
//
// Every float operation is a statement of its own: the library is built with -ffp-contract=on, which fuses a multiply
// and an add only inside one source expression, so nothing here is ever fused and a numpy restatement that rounds each
// operation separately gives the same bits.
#ifndef RP_PLAN_HPP_
#define RP_PLAN_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/plan/rp_plan.h"

#define RPPL_WAVE 64

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11) -------------------
struct RpplWords { uint32_t w[4]; };

__host__ __device__ inline RpplWords rppl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return RpplWords{{c0, c1, c2, c3}};
}

// z(seed, round, e, c): the sum of 12 words, centred and scaled; both conversions are exact (S < 2^36)
__host__ __device__ inline double rppl_z(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, uint32_t e, uint32_t c) {
  uint64_t S = 0;
  for (uint32_t j = 0; j < 3; ++j) {
    const RpplWords x = rppl_philox(round, e, c, j, seed_lo, seed_hi);
    S += (uint64_t)x.w[0] + x.w[1] + x.w[2] + x.w[3];
  }
  const int64_t centred = (int64_t)S - ((int64_t)6 << 32);
  return (double)centred * 2.3283064365386962890625e-10;   // 2^-32
}

// ---- splines -------------------------------------------------------------------------------------------------------------
// The control step knot p sits at.
__host__ __device__ inline int rppl_knot_step(int spline, int p, int H, int P) {
  if (P == 1) return 0;
  if (spline == RP_PLAN_LINEAR) return p * ((H - 1) / (P - 1));
  return (p * H + P - 1) / P;
}

// Entry of a plan at control step h; `knot(i)` reads knot i of that entry.
template <typename Read>
__host__ __device__ inline double rppl_spline(int spline, int h, int H, int P, Read knot) {
  if (P == 1) return knot(0);
  if (spline == RP_PLAN_ZERO) {
    int i = h * P / H;
    if (i > P - 1) i = P - 1;
    return knot(i);
  }
  const int Sd = (H - 1) / (P - 1);
  int i = h / Sd;
  if (i > P - 2) i = P - 2;
  const double k0 = knot(i), k1 = knot(i + 1);
  const double w = (double)(h - i * Sd) / (double)Sd;
  const double d = k1 - k0;
  const double m = d * w;
  const double a = k0 + m;
  return a;
}

// ---- argument checks (host) ----------------------------------------------------------------------------------------------
inline std::string rppl_check_range(const char* fn, const char* what, long long n, long long first, long long count) {
  if (first < 0 || count < 0 || first + count > n)
    return std::string(fn) + ": " + what + " [" + std::to_string(first) + ", " + std::to_string(first + count) +
           ") lies outside the batch of " + std::to_string(n);
  return "";
}

inline std::string rppl_check_spline(const char* fn, int spline, int H, int P) {
  if (spline != RP_PLAN_ZERO && spline != RP_PLAN_LINEAR) return std::string(fn) + ": spline must be RP_PLAN_ZERO or RP_PLAN_LINEAR";
  if (P < 1) return std::string(fn) + ": P must be >= 1";
  if (H < 1) return std::string(fn) + ": H must be >= 1";
  if (spline == RP_PLAN_LINEAR && P > 1 && (H - 1 < P - 1 || (H - 1) % (P - 1) != 0))
    return std::string(fn) + ": the linear spline needs (H - 1) % (P - 1) == 0 with H >= P (H = " + std::to_string(H) +
           ", P = " + std::to_string(P) + ")";
  return "";
}

// G K, P nu and E P nu must stay below 2^31: rows and plan entries are counted in int (and are Philox counter words)
inline std::string rppl_check_layout(const char* fn, int G, int K, int P, int nu) {
  if (G < 1) return std::string(fn) + ": G must be >= 1";
  if (K < 1) return std::string(fn) + ": K must be >= 1";
  if (P < 1) return std::string(fn) + ": P must be >= 1";
  if (nu < 1) return std::string(fn) + ": nu must be >= 1";
  if ((long long)G * K > 0x7fffffffLL || (long long)P * nu > 0x7fffffffLL) return std::string(fn) + ": G K and P nu must be < 2^31";
  return "";
}

#endif  // RP_PLAN_HPP_
