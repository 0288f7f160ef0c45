// rp_pop_critic.hpp -- the argument checks of librp_pop_critic.so (include/learn/rp_pop_critic.h) and the single-learner
// argument block its kernels hand to the shared device text (rp_critic.hpp).
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  As in
// rp_pop.hpp a population block is checked in two steps: what is the population's own (P, the member range, the row
// range, the grid order, rp_pop.hpp's routines), then the single-learner block it becomes, by rpc_check_step, whose
// message is returned under this library's entry point's name; the workspace, which holds one segment per member, last.
#ifndef RP_POP_CRITIC_HPP_
#define RP_POP_CRITIC_HPP_

#include <string>

#include "../../include/learn/rp_pop_critic.h"
#include "rp_critic.hpp"
#include "rp_pop.hpp"

inline size_t rppc_workspace_bytes(int n_critics, int H1, int H2, int row_count, int member_count) {
  return rpc_workspace_bytes(n_critics, H1, H2, row_count) * (size_t)member_count;
}

// All members' rows as one array, the stacked tensors' bases as the weight sets.  (row_first, mean, inv_std and the
// workspace are per member: the kernel fills them in; here they are member 0's.)
inline rp_critic_step_args rppc_as_critic_step(const rp_pop_critic_step_args* a) {
  rp_critic_step_args s = {};
  s.struct_size = sizeof(s);
  s.obs = a->obs; s.action = a->action; s.y = a->y; s.mask = a->mask; s.mean = a->mean; s.inv_std = a->inv_std;
  s.obs_clip = a->obs_clip;
  s.p = a->p; s.m = a->m; s.v = a->v; s.target = a->target; s.grad = a->grad; s.n_critics = a->n_critics;
  s.q = a->q;
  s.workspace = a->workspace; s.workspace_bytes = a->workspace_bytes;
  s.drop_threshold = a->drop_threshold; s.keep_scale = a->keep_scale; s.ln_eps = a->ln_eps;
  s.seed_lo = a->seed_lo; s.seed_hi = a->seed_hi; s.round = a->round;
  s.one_minus_beta1 = a->one_minus_beta1; s.beta2 = a->beta2; s.one_minus_beta2 = a->one_minus_beta2;
  s.step_size = a->step_size; s.bc2_sqrt = a->bc2_sqrt; s.eps = a->eps; s.tau = a->tau;
  s.D = a->D; s.H1 = a->H1; s.H2 = a->H2; s.A = a->A;
  s.B = a->P * a->n;
  s.row_first = a->row_first; s.row_count = a->row_count;
  s.launches = a->launches;
  s.hip_stream = a->hip_stream;
  return s;
}

inline std::string rppc_check_workspace(const rp_pop_critic_workspace_args* a) {
  const std::string fn = "rp_pop_critic_workspace";
  const std::string err = rpd_check_sizes(fn, a->n_critics, a->H1, a->H2, 1);
  if (!err.empty()) return err;
  if (a->row_count < 0) return fn + ": row_count must be >= 0";
  if (a->member_count < 0) return fn + ": member_count must be >= 0";
  return "";
}

inline std::string rppc_check_step(const rp_pop_critic_step_args* a) {
  const std::string fn = "rp_pop_critic_step";
  std::string err = rpp_check_members(fn, a->P, a->member_first, a->member_count);
  if (err.empty()) err = rpp_check_rows(fn, "n", a->P, a->n, a->row_first, a->row_count);
  if (err.empty()) err = rpp_check_order(fn, a->grid_order);
  if (!err.empty()) return err;
  rp_critic_step_args s = rppc_as_critic_step(a);
  s.workspace_bytes = ~(size_t)0;   // (the size is this library's to check: member_count segments)
  err = rpp_renamed(fn, rpc_check_step(&s));
  if (!err.empty()) return err;
  const size_t need = rppc_workspace_bytes(a->n_critics, a->H1, a->H2, a->row_count, a->member_count);
  if (a->workspace_bytes < need)
    return fn + ": workspace of " + std::to_string(a->workspace_bytes) + " bytes is smaller than the " + std::to_string(need) +
           " this step needs";
  return "";
}

#endif  // RP_POP_CRITIC_HPP_
