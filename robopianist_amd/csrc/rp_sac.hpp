// rp_sac.hpp -- the argument checks of librp_sac.so (include/learn/rp_sac.h), and the device text of its sampler and
// policy, which librp_pop.so runs too.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// constants of the tile are the learner's (rp_learn.hpp), the noise is the planner's (rp_plan.hpp).
#ifndef RP_SAC_HPP_
#define RP_SAC_HPP_

#include <string>

#include "../../include/learn/rp_sac.h"
#include "rp_learn.hpp"
#include "rp_mlp_tile.hpp"

inline std::string rps_check_sample(const rp_sac_sample_args* a) {
  const std::string fn = "rp_sac_sample";
  if (!a->ring_obs || !a->ring_action || !a->ring_reward || !a->ring_discount || !a->ring_step_type || !a->obs ||
      !a->next_obs || !a->action || !a->reward || !a->discount || !a->mask)
    return fn + ": a pointer is NULL";
  if (a->C < 2) return fn + ": C must be >= 2";
  if (a->n_written < 2) return fn + ": n_written must be >= 2";
  if (a->E < 1) return fn + ": E must be >= 1";
  if (a->D < 1) return fn + ": D must be >= 1";
  if (a->A < 1) return fn + ": A must be >= 1";
  if (a->B < 1) return fn + ": B must be >= 1";
  const long long F = a->n_written < (long long)a->C ? a->n_written : (long long)a->C;
  if ((F - 1) * (long long)a->E >= (1LL << 32)) return fn + ": (min(n_written, C) - 1) E must be < 2^32";
  if (a->index && (long long)a->C * a->E > 0x7fffffffLL) return fn + ": C E must be < 2^31 where index is given";
  return rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
}

inline std::string rps_check_act(const rp_sac_act_args* a) {
  const std::string fn = "rp_sac_act";
  if (!a->obs || !a->mean || !a->inv_std || !a->action) return fn + ": a pointer is NULL";
  if (!a->actor) return fn + ": actor is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->log_std_min <= a->log_std_max)) return fn + ": log_std_min must be <= log_std_max";
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpl_check_hidden(fn, "H1", a->H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", a->H2);
  if (!err.empty()) return err;
  if (a->A < 1 || 2 * a->A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(a->A);
  err = rpl_check_mlp(fn, "actor", a->actor);
  if (!err.empty()) return err;
  if (!a->deterministic && !a->logp) return fn + ": a sampling actor needs logp";
  if (a->env_action && a->precision != 32 && a->precision != 64) return fn + ": precision must be 32 or 64";
  if (a->n_rows < 1) return fn + ": n_rows must be >= 1";
  return rpl_check_range(fn.c_str(), a->n_rows, a->row_first, a->row_count);
}

inline std::string rps_check_target(const rp_sac_target_args* a) {
  const std::string fn = "rp_sac_target";
  if (!a->next_obs || !a->action || !a->logp || !a->reward || !a->discount || !a->mean || !a->inv_std || !a->log_alpha || !a->y)
    return fn + ": a pointer is NULL";
  if (!a->critics) return fn + ": critics is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (a->n_critics < 1 || a->n_critics > RP_SAC_MAX_CRITICS)
    return fn + ": n_critics must be 1 .. " + std::to_string(RP_SAC_MAX_CRITICS) + ", got " + std::to_string(a->n_critics);
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpl_check_hidden(fn, "H1", a->H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", a->H2);
  if (!err.empty()) return err;
  if (a->A < 1 || 2 * a->A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(a->A);
  for (int i = 0; i < a->n_critics; ++i) {
    err = rpl_check_mlp(fn, ("critic " + std::to_string(i)).c_str(), &a->critics[i]);
    if (!err.empty()) return err;
  }
  if (a->B < 1) return fn + ": B must be >= 1";
  return rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
}

// ---- the device text of sample and act, shared with librp_pop.so (rp_pop.hip) -------------------------------------------
// Each body is parametrised by a map resolved at compile time: the kernels of librp_sac.so pass the identity, the
// population kernels their member's rows.  The weight set in use is the caller's argument block and RpsActor, by value.
namespace {

// (RplRowIdentity, row l of the caller's range is array row l, is rp_learn.hpp's.)  Row l is array row base + stride l (a member's rows, interleaved or blocked).
struct RplRowAffine {
  long long base, stride;
  __device__ long long operator()(long long l) const { return base + stride * l; }
};

// The envs a sampler row draws from: all E of the ring, in order.
struct RpsEnvsAll {
  long long count;   // E
  __device__ long long operator()(long long jj) const { return jj; }
};
// Member p's envs of P: count = E / P, env jj is p + P jj.
struct RpsEnvsMember {
  long long count, p, P;
  __device__ long long operator()(long long jj) const { return p + P * jj; }
};

// ---- sample ----------------------------------------------------------------------------------------------------------
__device__ inline void rps_zero_row(float* d, int width) {
  for (int i = (int)threadIdx.x; i < width; i += RPL_WAVE) d[i] = 0.f;
}

// Minibatch row b (the array row and the Philox counter), drawn over `envs`; one wave.
template <typename Envs>
__device__ inline void rps_sample_row(const rp_sac_sample_args& a, const long long b, const Envs envs) {
  const long long C = a.C, E = a.E;
  const long long F = a.n_written < C ? a.n_written : C;
  const uint64_t N = (uint64_t)((F - 1) * envs.count);   // (< 2^32, checked)
  long long slot = -1, next = -1, e = 0;
  for (uint32_t j = 0; j < RP_SAC_SAMPLE_TRIES; ++j) {
    const uint32_t w = rppl_philox(a.round, (uint32_t)b, 0u, 16u + j, a.seed_lo, a.seed_hi).w[0];
    const uint64_t i = ((uint64_t)w * N) >> 32;   // (< N)
    const long long t = (long long)(i / (uint64_t)envs.count);
    const long long ee = envs((long long)(i % (uint64_t)envs.count));
    const long long m = a.n_written - F + t;      // (<= n_written - 2)
    const long long s0 = m % C, s1 = (m + 1) % C;
    const int st0 = a.ring_step_type[s0 * E + ee], st1 = a.ring_step_type[s1 * E + ee];
    if (st0 != RP_LEARN_STEP_LAST && st1 != RP_LEARN_STEP_FIRST) {   // (wave-uniform)
      slot = s0; next = s1; e = ee;
      break;
    }
  }
  float* obs = a.obs + b * a.D;
  float* nobs = a.next_obs + b * a.D;
  float* act = a.action + b * a.A;
  if (slot < 0) {
    rps_zero_row(obs, a.D);
    rps_zero_row(nobs, a.D);
    rps_zero_row(act, a.A);
    if (threadIdx.x == 0) {
      a.reward[b] = 0.f;
      a.discount[b] = 0.f;
      a.mask[b] = 0.f;
      if (a.index) a.index[b] = -1;
    }
    return;
  }
  const long long r0 = slot * E + e, r1 = next * E + e;
  rpl_copy_row(a.ring_obs + r0 * a.D, obs, a.D);
  rpl_copy_row(a.ring_obs + r1 * a.D, nobs, a.D);
  rpl_copy_row(a.ring_action + r0 * a.A, act, a.A);
  if (threadIdx.x == 0) {
    a.reward[b] = a.ring_reward[r1];
    a.discount[b] = a.ring_discount[r1];
    a.mask[b] = 1.f;
    if (a.index) a.index[b] = (int32_t)r0;
  }
}

// ---- act -------------------------------------------------------------------------------------------------------------
struct RpsActor {
  rp_learn_mlp net;
  float logp_const;   // (float)(0.5 A ln 2 pi)
  float ln2;          // (float)ln 2
};

// The tile of the rows l0 .. l0 + 15 below l_end of the caller's range; `rows` gives their array rows (the noise's row
// too).  `sa`, `sw`, `sh`: the caller's LDS (rp_mlp_tile.hpp).  All 256 threads call it together.
// (__forceinline__: inlined last, as `inline` leaves it, the register allocation of rp_sac_act_kernel differs.)
template <typename Rows>
__device__ __forceinline__ void rps_act_tile(const rp_sac_act_args& a, const RpsActor& actor, const Rows rows, const long long e0,
                                    const long long e_end, float* sa, float* sw, float* sh) {
  const int tid = (int)threadIdx.x;
  const rp_learn_mlp net = actor.net;
  const int A = a.A, N3 = 2 * a.A;
  f32x4 acc[RPL_ACC];
  rpl_layer(
      [&](int r, int k) {
        const long long e = e0 + r;
        if (e >= e_end) return 0.f;
        return rpl_xn(a.obs, a.mean, a.inv_std, a.obs_clip, rows(e), a.D, k);
      },
      a.D, net.w1, a.H1, sa, sw, acc);
  rpl_store_layer<true>(acc, net.b1, a.H1, sh);
  rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, net.w2, a.H2, sa, sw, acc);
  rpl_store_layer<true>(acc, net.b2, a.H2, sh);
  rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H2, net.w3, N3, sa, sw, acc);
  rpl_store_layer<false>(acc, net.b3, N3, sh);
  float* sg = sw;   // [row][RP_LEARN_MAX_A]: the terms of the log-probability (the weight stage is dead)
  for (int idx = tid; idx < RPL_TILE_R * A; idx += RPL_BLOCK) {
    const int r = idx / A, u = idx - r * A;
    const long long l = e0 + r;
    if (l >= e_end) continue;
    const long long e = rows(l);
    const float m = sh[r * RPL_H_PITCH + u];
    float p = m;
    if (!a.deterministic) {
      const float l = sh[r * RPL_H_PITCH + A + u];
      const float lc = fmaxf(l, a.log_std_min);
      const float ls = fminf(lc, a.log_std_max);
      const float zf = (float)rppl_z(a.seed_lo, a.seed_hi, a.round, (uint32_t)e, (uint32_t)u);
      const float sd = expf(ls);
      const float t = sd * zf;
      p = m + t;
      sg[r * RP_LEARN_MAX_A + u] = rpl_logp_term(p, zf, ls, actor.ln2);
    }
    const float act = tanhf(p);
    const size_t o = (size_t)e * A + u;
    a.action[o] = act;
    if (a.pre) a.pre[o] = p;
    if (a.env_action) {
      if (a.precision == 32) static_cast<float*>(a.env_action)[o] = act;
      else static_cast<double*>(a.env_action)[o] = (double)act;
    }
  }
  if (a.deterministic) return;   // (block-uniform)
  __syncthreads();
  if (tid < RPL_TILE_R && e0 + tid < e_end) {
    float s = 0.f;
    for (int u = 0; u < A; u++) s = s + sg[tid * RP_LEARN_MAX_A + u];
    a.logp[rows(e0 + tid)] = s - actor.logp_const;
  }
}

}  // namespace

#endif  // RP_SAC_HPP_
