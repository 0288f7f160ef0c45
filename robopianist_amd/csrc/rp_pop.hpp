// rp_pop.hpp -- the argument checks of librp_pop.so (include/learn/rp_pop.h), and the single-learner argument blocks its
// kernels hand to the shared device text (rp_sac.hpp, rp_droq.hpp, rp_learn.hpp).
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  A
// population block is checked in two steps: what is the population's own (P, the member range, the layout, the sizes
// that must fit an int), then the single-learner block it becomes, by the single-learner check (rps_check_*,
// rpd_check_target, rpl_check_moments), whose message is returned under this library's entry point's name.
#ifndef RP_POP_HPP_
#define RP_POP_HPP_

#include <string>

#include "../../include/learn/rp_pop.h"
#include "rp_droq.hpp"
#include "rp_sac.hpp"

// `err` of a single-learner check ("rp_sac_act: ...") under the name `fn`.
inline std::string rpp_renamed(const std::string& fn, const std::string& err) {
  if (err.empty()) return err;
  const size_t colon = err.find(':');
  return fn + (colon == std::string::npos ? ": " + err : err.substr(colon));
}

inline std::string rpp_check_members(const std::string& fn, int P, int member_first, int member_count) {
  if (P < 1) return fn + ": P must be >= 1";
  if (member_first < 0 || member_count < 0 || (long long)member_first + member_count > P)
    return fn + ": the member range [" + std::to_string(member_first) + ", " +
           std::to_string((long long)member_first + member_count) + ") lies outside the " + std::to_string(P) + " members";
  return "";
}

// `rows` rows per member, P rows in all: the row range, and the total that the single-learner block holds in an int.
inline std::string rpp_check_rows(const std::string& fn, const char* name, int P, int rows, int row_first, int row_count) {
  if (rows < 1) return fn + ": " + name + " must be >= 1";
  if ((long long)P * rows > 0x7fffffffLL) return fn + ": P " + name + " must be < 2^31";
  return rppl_check_range(fn.c_str(), "the row range", rows, row_first, row_count);
}

inline std::string rpp_check_order(const std::string& fn, int order) {
  if (order != RP_POP_TILE_MAJOR && order != RP_POP_MEMBER_MAJOR)
    return fn + ": grid_order must be RP_POP_TILE_MAJOR or RP_POP_MEMBER_MAJOR";
  return "";
}

// ---- the single-learner blocks: all members' rows as one array, the stacked tensors' bases as the weight set ----------
inline rp_sac_act_args rpp_as_sac_act(const rp_pop_act_args* a) {
  rp_sac_act_args s = {};
  s.struct_size = sizeof(s);
  s.obs = a->obs; s.mean = a->mean; s.inv_std = a->inv_std;
  s.obs_clip = a->obs_clip; s.log_std_min = a->log_std_min; s.log_std_max = a->log_std_max;
  s.actor = a->actor;
  s.action = a->action; s.logp = a->logp; s.pre = a->pre; s.env_action = a->env_action;
  s.precision = a->precision; s.deterministic = a->deterministic;
  s.seed_lo = a->seed_lo; s.seed_hi = a->seed_hi; s.round = a->round;
  s.D = a->D; s.H1 = a->H1; s.H2 = a->H2; s.A = a->A;
  s.n_rows = a->P * a->rows;   // (row_first = row_count = 0: the kernel takes its range from the population block)
  s.hip_stream = a->hip_stream;
  return s;
}

inline rp_sac_sample_args rpp_as_sac_sample(const rp_pop_sample_args* a) {
  rp_sac_sample_args s = {};
  s.struct_size = sizeof(s);
  s.ring_obs = a->ring_obs; s.ring_action = a->ring_action; s.ring_reward = a->ring_reward;
  s.ring_discount = a->ring_discount; s.ring_step_type = a->ring_step_type;
  s.obs = a->obs; s.next_obs = a->next_obs; s.action = a->action; s.reward = a->reward; s.discount = a->discount;
  s.mask = a->mask; s.index = a->index;
  s.n_written = a->n_written;
  s.seed_lo = a->seed_lo; s.seed_hi = a->seed_hi; s.round = a->round;
  s.C = a->C; s.E = a->E; s.D = a->D; s.A = a->A;
  s.B = a->P * a->n;
  s.hip_stream = a->hip_stream;
  return s;
}

// (gamma and log_alpha are per member: the kernel fills them in; here they stand for "given")
inline rp_droq_target_args rpp_as_droq_target(const rp_pop_target_args* a) {
  rp_droq_target_args s = {};
  s.struct_size = sizeof(s);
  s.next_obs = a->next_obs; s.action = a->action; s.logp = a->logp; s.reward = a->reward; s.discount = a->discount;
  s.mean = a->mean; s.inv_std = a->inv_std;
  s.obs_clip = a->obs_clip; s.gamma = 0.f; s.log_alpha = a->log_alpha;
  s.critics = a->critics; s.n_critics = a->n_critics;
  s.y = a->y; s.q_min = a->q_min; s.q = a->q;
  s.drop_threshold = a->drop_threshold; s.keep_scale = a->keep_scale; s.ln_eps = a->ln_eps;
  s.seed_lo = a->seed_lo; s.seed_hi = a->seed_hi; s.round = a->round;
  s.D = a->D; s.H1 = a->H1; s.H2 = a->H2; s.A = a->A;
  s.B = a->P * a->n;
  s.hip_stream = a->hip_stream;
  return s;
}

inline rp_learn_moments_args rpp_as_learn_moments(const rp_pop_moments_args* a) {
  rp_learn_moments_args s = {};
  s.struct_size = sizeof(s);
  s.obs = a->obs; s.mean = a->mean; s.M2 = a->M2; s.mean_f32 = a->mean_f32; s.inv_std_f32 = a->inv_std_f32;
  s.count = a->count; s.eps = a->eps;
  s.n_rows = (long long)a->k * (a->P > 0 ? a->E / a->P : 0);
  s.D = a->D;
  s.hip_stream = a->hip_stream;
  return s;
}

// ---- the checks --------------------------------------------------------------------------------------------------------
inline std::string rpp_check_act(const rp_pop_act_args* a) {
  const std::string fn = "rp_pop_act";
  std::string err = rpp_check_members(fn, a->P, a->member_first, a->member_count);
  if (err.empty()) err = rpp_check_rows(fn, "rows", a->P, a->rows, a->row_first, a->row_count);
  if (!err.empty()) return err;
  if (a->layout != RP_POP_INTERLEAVED && a->layout != RP_POP_BLOCKED)
    return fn + ": layout must be RP_POP_INTERLEAVED or RP_POP_BLOCKED";
  err = rpp_check_order(fn, a->grid_order);
  if (!err.empty()) return err;
  const rp_sac_act_args s = rpp_as_sac_act(a);
  return rpp_renamed(fn, rps_check_act(&s));
}

inline std::string rpp_check_sample(const rp_pop_sample_args* a) {
  const std::string fn = "rp_pop_sample";
  std::string err = rpp_check_members(fn, a->P, a->member_first, a->member_count);
  if (err.empty()) err = rpp_check_rows(fn, "n", a->P, a->n, a->row_first, a->row_count);
  if (!err.empty()) return err;
  if (a->E < 1) return fn + ": E must be >= 1";
  if (a->E % a->P != 0) return fn + ": E = " + std::to_string(a->E) + " is not a multiple of P = " + std::to_string(a->P);
  if (a->C >= 2 && (long long)(a->C - 1) * (a->E / a->P) >= (1LL << 32)) return fn + ": (C - 1) E / P must be < 2^32";
  const rp_sac_sample_args s = rpp_as_sac_sample(a);
  return rpp_renamed(fn, rps_check_sample(&s));
}

inline std::string rpp_check_target(const rp_pop_target_args* a) {
  const std::string fn = "rp_pop_target";
  std::string err = rpp_check_members(fn, a->P, a->member_first, a->member_count);
  if (err.empty()) err = rpp_check_rows(fn, "n", a->P, a->n, a->row_first, a->row_count);
  if (err.empty()) err = rpp_check_order(fn, a->grid_order);
  if (!err.empty()) return err;
  if (!a->gamma) return fn + ": a pointer is NULL";
  const rp_droq_target_args s = rpp_as_droq_target(a);
  return rpp_renamed(fn, rpd_check_target(&s));
}

inline std::string rpp_check_moments(const rp_pop_moments_args* a) {
  const std::string fn = "rp_pop_moments";
  std::string err = rpp_check_members(fn, a->P, a->member_first, a->member_count);
  if (!err.empty()) return err;
  if (a->k < 1) return fn + ": k must be >= 1";
  if (a->E < 1) return fn + ": E must be >= 1";
  if (a->E % a->P != 0) return fn + ": E = " + std::to_string(a->E) + " is not a multiple of P = " + std::to_string(a->P);
  const rp_learn_moments_args s = rpp_as_learn_moments(a);
  return rpp_renamed(fn, rpl_check_moments(&s));
}

#endif  // RP_POP_HPP_
