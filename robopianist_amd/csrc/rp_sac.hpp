// rp_sac.hpp -- the argument checks of librp_sac.so (include/learn/rp_sac.h).
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// constants of the tile are the learner's (rp_learn.hpp), the noise is the planner's (rp_plan.hpp).
#ifndef RP_SAC_HPP_
#define RP_SAC_HPP_

#include <string>

#include "../../include/learn/rp_sac.h"
#include "rp_learn.hpp"

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

#endif  // RP_SAC_HPP_
