// rp_evolve.hpp -- the arithmetic of librp_evolve.so (include/learn/rp_evolve.h) and the argument checks.
//
// As in rp_plan.hpp, every float operation is a statement of its own: the library is built with -ffp-contract=on, which
// fuses a multiply and an add only inside one source expression, so nothing here is ever fused and a numpy restatement that
// rounds each operation separately gives the same bits.  The plan's draw is the planner's Philox (rp_plan.hpp).
#ifndef RP_EVOLVE_HPP_
#define RP_EVOLVE_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/learn/rp_evolve.h"
#include "rp_plan.hpp"

#define RPE_WAVE 64
#define RPE_COPY_BLOCK 256

// k of n eligible members at `percent`: the size of either end
__host__ __device__ inline int rpe_ends(int n, int percent) {
  const int a = n * percent / 100, b = n / 2;
  return a < b ? a : b;
}

// 1 - (1 - gamma) f, clamped
__host__ __device__ inline float rpe_explore_gamma(float gamma, float f, float lo, float hi) {
  const float d = 1.f - gamma;
  const float e = d * f;
  const float g = 1.f - e;
  return fminf(fmaxf(g, lo), hi);
}

// target_entropy f, clamped
__host__ __device__ inline float rpe_explore_entropy(float target_entropy, float f, float lo, float hi) {
  const float t = target_entropy * f;
  return fminf(fmaxf(t, lo), hi);
}

// ---- argument checks (host) ----------------------------------------------------------------------------------------------
inline std::string rpe_check_fold(const rp_evolve_fold_args& a) {
  const std::string fn = "rp_evolve_fold: ";
  if (!a.done_return || !a.done_count || !a.fit_sum || !a.fit_count) return fn + "a pointer is NULL";
  if (a.P < 1) return fn + "P must be >= 1, got " + std::to_string(a.P);
  if (a.E < 1 || a.E % a.P != 0)
    return fn + "E must be a positive multiple of P (E = " + std::to_string(a.E) + ", P = " + std::to_string(a.P) + ")";
  return "";
}

inline std::string rpe_check_plan(const rp_evolve_plan_args& a) {
  const std::string fn = "rp_evolve_plan: ";
  if (!a.fit_sum || !a.fit_count || !a.source) return fn + "a pointer is NULL";
  if (a.P < 1 || a.P > RP_EVOLVE_MAX_MEMBERS)
    return fn + "P must be 1 .. " + std::to_string(RP_EVOLVE_MAX_MEMBERS) + ", got " + std::to_string(a.P);
  if (a.percent < 0 || a.percent > 100) return fn + "percent must lie in [0, 100], got " + std::to_string(a.percent);
  if (a.min_episodes < 1) return fn + "min_episodes must be >= 1, got " + std::to_string(a.min_episodes);
  if (!(a.min_gap >= 0.0)) return fn + "min_gap must be >= 0";
  if (!(a.up > 0.f)) return fn + "up must be > 0";
  if (!(a.down > 0.f)) return fn + "down must be > 0";
  if (!(a.gamma_lo <= a.gamma_hi)) return fn + "gamma_lo must be <= gamma_hi";
  if (!(a.entropy_lo <= a.entropy_hi)) return fn + "entropy_lo must be <= entropy_hi";
  return "";
}

inline std::string rpe_check_copy(const rp_evolve_copy_args& a) {
  const std::string fn = "rp_evolve_copy: ";
  if (!a.source) return fn + "source is NULL";
  if (a.P < 1 || a.P > RP_EVOLVE_MAX_COPY_MEMBERS)
    return fn + "P must be 1 .. " + std::to_string(RP_EVOLVE_MAX_COPY_MEMBERS) + ", got " + std::to_string(a.P);
  if (a.n_fields < 0) return fn + "n_fields must be >= 0, got " + std::to_string(a.n_fields);
  if (a.n_fields > 0 && !a.fields) return fn + "fields is NULL";
  for (int i = 0; i < a.n_fields; ++i) {
    const rp_evolve_field& f = a.fields[i];
    const std::string which = fn + "field " + std::to_string(i);
    if (!f.base) return which + " has a NULL base";
    if (reinterpret_cast<uintptr_t>(f.base) & 3) return which + " has a base that is not 4-byte aligned";
    if (f.slice_words < 1) return which + " has slice_words < 1";
    if (f.slice_words > (1LL << 35)) return which + " has a slice of more than 2^35 words";
  }
  return "";
}

#endif  // RP_EVOLVE_HPP_
