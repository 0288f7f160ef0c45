// rp_learn.hpp -- the constants and the argument checks of librp_learn.so (include/learn/rp_learn.h).
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// noise is the planner's (rp_plan.hpp: rppl_z), not a second Philox.
#ifndef RP_LEARN_HPP_
#define RP_LEARN_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/learn/rp_learn.h"
#include "rp_plan.hpp"

#define RPL_WAVE 64
#define RPL_BLOCK 256
// act: one workgroup of four waves owns RPL_TILE_R rows of one network
#define RPL_TILE_R 16
#define RPL_TK 32        // the k extent of one stage of the operands in LDS
#define RPL_S_PITCH 34   // floats per staged row: lane (r16, kq) reads bank (2 r16 + kq) % 32, all 32 of a half-wave differ
#define RPL_H_PITCH 260  // floats per row of the activations kept in LDS (RP_LEARN_MAX_H + 4)
// moments: RPL_MOMENT_COLS columns x RPL_MOMENT_LANES partial sums per workgroup
#define RPL_MOMENT_COLS 16
#define RPL_MOMENT_LANES 16

inline std::string rpl_check_range(const char* fn, long long n, long long first, long long count) {
  return rppl_check_range(fn, "the row range", n, first, count);
}

inline std::string rpl_check_pack(const rp_learn_pack_args* a) {
  const std::string fn = "rp_learn_pack";
  if (!a->fields) return fn + ": fields is NULL";
  if (a->n_fields < 1 || a->n_fields > RP_LEARN_MAX_FIELDS)
    return fn + ": n_fields must be 1 .. " + std::to_string(RP_LEARN_MAX_FIELDS) + ", got " + std::to_string(a->n_fields);
  if (a->precision != 32 && a->precision != 64) return fn + ": precision must be 32 or 64";
  if (!a->step_type || !a->obs || !a->slot_reward || !a->slot_discount || !a->slot_step_type) return fn + ": a pointer is NULL";
  const int n_stats = (a->ep_return != nullptr) + (a->ep_len != nullptr) + (a->done_return != nullptr) +
                      (a->done_len != nullptr) + (a->done_count != nullptr);
  if (n_stats != 0 && n_stats != 5) return fn + ": the five episode statistics arrays come together or not at all";
  if (a->E < 1) return fn + ": E must be >= 1";
  if (a->D < 1) return fn + ": D must be >= 1";
  long long sum = 0;
  for (int i = 0; i < a->n_fields; ++i) {
    const rp_learn_field& f = a->fields[i];
    if (!f.src) return fn + ": field " + std::to_string(i) + " has a NULL pointer";
    if (f.width < 1) return fn + ": field " + std::to_string(i) + " has width < 1";
    if (f.dtype != RP_LEARN_F32 && f.dtype != RP_LEARN_F64)
      return fn + ": field " + std::to_string(i) + " has a dtype other than RP_LEARN_F32 / RP_LEARN_F64";
    sum += f.width;
  }
  if (sum != a->D) return fn + ": the field widths sum to " + std::to_string(sum) + ", D is " + std::to_string(a->D);
  return rpl_check_range(fn.c_str(), a->E, a->env_first, a->env_count);
}

inline std::string rpl_check_mlp(const std::string& fn, const char* which, const rp_learn_mlp* m) {
  if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->w3 || !m->b3) return fn + ": the " + which + " has a NULL pointer";
  return "";
}

inline std::string rpl_check_hidden(const std::string& fn, const char* name, int H) {
  if (H < 16 || H > RP_LEARN_MAX_H || H % 16 != 0)
    return fn + ": " + name + " must be a multiple of 16 in [16, " + std::to_string(RP_LEARN_MAX_H) + "], got " + std::to_string(H);
  return "";
}

inline std::string rpl_check_act(const rp_learn_act_args* a) {
  const std::string fn = "rp_learn_act";
  if (!a->obs || !a->mean || !a->inv_std) return fn + ": a pointer is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!a->actor && !a->critic) return fn + ": neither an actor nor a critic";
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpl_check_hidden(fn, "H1", a->H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", a->H2);
  if (!err.empty()) return err;
  if (a->actor) {
    if (a->A < 1 || a->A > RP_LEARN_MAX_A) return fn + ": A must be 1 .. " + std::to_string(RP_LEARN_MAX_A) + ", got " + std::to_string(a->A);
    err = rpl_check_mlp(fn, "actor", a->actor);
    if (!err.empty()) return err;
    if (!a->action || !a->env_action) return fn + ": an actor needs action and env_action";
    if (!a->deterministic && (!a->logp || !a->log_std)) return fn + ": a sampling actor needs logp and log_std";
    if (a->precision != 32 && a->precision != 64) return fn + ": precision must be 32 or 64";
  }
  if (a->critic) {
    err = rpl_check_mlp(fn, "critic", a->critic);
    if (!err.empty()) return err;
    if (!a->value) return fn + ": a critic needs value";
  }
  if (a->n_rows < 1) return fn + ": n_rows must be >= 1";
  return rpl_check_range(fn.c_str(), a->n_rows, a->row_first, a->row_count);
}

inline std::string rpl_check_gae(const rp_learn_gae_args* a) {
  const std::string fn = "rp_learn_gae";
  if (!a->reward || !a->discount || !a->step_type || !a->value || !a->adv || !a->ret || !a->valid) return fn + ": a pointer is NULL";
  if (a->T < 1) return fn + ": T must be >= 1";
  if (a->E < 1) return fn + ": E must be >= 1";
  return rpl_check_range(fn.c_str(), a->E, a->env_first, a->env_count);
}

inline std::string rpl_check_moments(const rp_learn_moments_args* a) {
  const std::string fn = "rp_learn_moments";
  if (!a->obs || !a->mean || !a->M2 || !a->mean_f32 || !a->inv_std_f32) return fn + ": a pointer is NULL";
  if (a->D < 1) return fn + ": D must be >= 1";
  if (a->n_rows < 1) return fn + ": n_rows must be >= 1";
  if (!(a->count >= 0.0)) return fn + ": count must be >= 0";
  if (!(a->eps > 0.0)) return fn + ": eps must be > 0";
  return "";
}

// ---- the device text of moments, shared with librp_pop.so (rp_pop.hip) --------------------------------------------------
// Parametrised by a row map resolved at compile time: the kernel of librp_learn.so passes the identity.
namespace {

struct RplRowIdentity {   // row l of the caller's range is array row l
  __device__ long long operator()(long long l) const { return l; }
};

__device__ inline double rpl_lane_sum(double mine, double (*part)[RPL_MOMENT_COLS], int col, int l) {
  __syncthreads();   // (the previous reduction's reads)
  part[l][col] = mine;
  __syncthreads();
  double s = part[0][col];
  for (int i = 1; i < RPL_MOMENT_LANES; i++) s = s + part[i][col];
  return s;
}

// The merge of the caller's n_rows rows, `rows` giving the array row of each, into the moments `a` points to; `part`:
// the caller's LDS.  All 256 threads call it together.
template <typename Rows>
__device__ inline void rpl_moments_block(const rp_learn_moments_args& a, const Rows rows, double (*part)[RPL_MOMENT_COLS]) {
  const int col = (int)threadIdx.x & (RPL_MOMENT_COLS - 1), l = (int)threadIdx.x / RPL_MOMENT_COLS;
  const int j = (int)blockIdx.x * RPL_MOMENT_COLS + col;
  const bool live = j < a.D;
  const float* x = a.obs + (live ? j : 0);
  const double nb = (double)a.n_rows;
  double S = 0.0;
  if (live)
    for (long long i = l; i < a.n_rows; i += RPL_MOMENT_LANES) S = S + (double)x[rows(i) * a.D];
  S = rpl_lane_sum(S, part, col, l);
  const double mb = S / nb;
  double M = 0.0;
  if (live)
    for (long long i = l; i < a.n_rows; i += RPL_MOMENT_LANES) {
      const double d = (double)x[rows(i) * a.D] - mb;
      const double q = d * d;
      M = M + q;
    }
  M = rpl_lane_sum(M, part, col, l);
  if (!live || l != 0) return;
  const double n = a.count + nb;
  const double dl = mb - a.mean[j];
  const double w = nb / n;
  const double step = dl * w;
  const double mean = a.mean[j] + step;
  const double dd = dl * dl;
  const double dc = dd * a.count;
  const double cross = dc * w;
  const double m2ab = a.M2[j] + M;
  const double m2 = m2ab + cross;
  a.mean[j] = mean;
  a.M2[j] = m2;
  a.mean_f32[j] = (float)mean;
  const double var = m2 / n;
  const double ve = var + a.eps;
  const double sd = sqrt(ve);
  const double inv = 1.0 / sd;
  a.inv_std_f32[j] = (float)inv;
}

}  // namespace

#endif  // RP_LEARN_HPP_
