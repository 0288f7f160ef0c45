// rp_droq.hpp -- the argument checks of librp_droq.so (include/learn/rp_droq.h).
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  They
// are rp_sac.hpp's rps_check_target on the DroQ block, plus the LayerNorm pointers and the two positive scalars.
#ifndef RP_DROQ_HPP_
#define RP_DROQ_HPP_

#include <string>

#include "../../include/learn/rp_droq.h"
#include "rp_learn.hpp"

inline std::string rpd_check_target(const rp_droq_target_args* a) {
  const std::string fn = "rp_droq_target";
  if (!a->next_obs || !a->action || !a->logp || !a->reward || !a->discount || !a->mean || !a->inv_std || !a->log_alpha || !a->y)
    return fn + ": a pointer is NULL";
  if (!a->critics) return fn + ": critics is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->keep_scale > 0.f)) return fn + ": keep_scale must be > 0";
  if (!(a->ln_eps > 0.f)) return fn + ": ln_eps must be > 0";
  if (a->n_critics < 1 || a->n_critics > RP_DROQ_MAX_CRITICS)
    return fn + ": n_critics must be 1 .. " + std::to_string(RP_DROQ_MAX_CRITICS) + ", got " + std::to_string(a->n_critics);
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpl_check_hidden(fn, "H1", a->H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", a->H2);
  if (!err.empty()) return err;
  if (a->A < 1 || 2 * a->A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(a->A);
  for (int i = 0; i < a->n_critics; ++i) {
    const rp_droq_critic& c = a->critics[i];
    err = rpl_check_mlp(fn, ("critic " + std::to_string(i)).c_str(), &c.net);
    if (!err.empty()) return err;
    if (!c.g1 || !c.be1 || !c.g2 || !c.be2) return fn + ": the LayerNorm of critic " + std::to_string(i) + " has a NULL pointer";
  }
  if (a->B < 1) return fn + ": B must be >= 1";
  return rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
}

#endif  // RP_DROQ_HPP_
