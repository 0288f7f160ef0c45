/* learn/rp_droq.h — the TD target of DroQ: an ensemble of target critics whose hidden layers are
 * Linear -> Dropout -> LayerNorm -> ReLU, their minimum and the soft TD target in one launch (C ABI, gfx950,
 * librp_droq.so).
 *
 * DroQ (Hiroe et al. 2022: "Dropout Q-functions for doubly efficient reinforcement learning") is soft actor-critic
 * (learn/rp_sac.h) with dropout and layer normalisation in the critics and several critic updates per actor update.
 * The replay ring, its sampler and the policy are rp_sac.h's, unchanged (rp_sac_sample, rp_sac_act); this library adds
 * the one launch that rp_sac_target cannot do, because rp_sac_target reads two tanh layers.  Conventions are rp_sac.h's:
 * no handle, no allocation, every array is the caller's.
 *
 * A critic is (D + A) -> H1 -> H2 -> 1 on cat([xn, action]), xn being rp_sac_act's normaliser on next_obs:
 *     d = x - mean[k];  p = d * inv_std[k];  xn = fminf(fmaxf(p, -obs_clip), obs_clip)
 * For critic i = 0 .. n_critics - 1 (ascending), batch row b and hidden layer L in {0, 1} with H units, weights W [H][K],
 * bias bb, LayerNorm weight g and bias be:
 *     s[n]  = (fused-multiply-add chain over k ascending, from 0, of in[k] W[n][k]) + bb[n]
 *     words = philox(round, b, n >> 2, 32 + 2 i + L; seed_lo, seed_hi);   keep = words.w[n & 3] >= drop_threshold
 *     h[n]  = keep ? s[n] * keep_scale : 0
 *     mu    = SUM(h) / (float)H;   d[n] = h[n] - mu;   var = SUM(d d) / (float)H
 *     t     = var + ln_eps;  sq = sqrtf(t);  r = 1 / sq
 *     o = d[n] * r;  o = o * g[n];  o = o + be[n];  out[n] = fmaxf(o, 0)
 * then q_i = (W3 out) + b3 (the same chain), qm = fminf over i ascending, and rp_sac_target's epilogue, unchanged:
 *     al = expf(*log_alpha);  s = al logp;  v = qm - s;  nv = gamma discount;  tv = nv v;  y = reward + tv
 *
 * b is the ABSOLUTE batch row (not the row inside a tile or a range): a row gets the same masks whichever range it is
 * computed in.  philox is the planner's Philox4x32-10 (plan/rp_plan.h).  The last counter word is 32 .. 39 here; the
 * policy's z uses 0 .. 2 and the sampler 16 .. 19, so one (seed, round) serves all three.  One Philox call gives the
 * masks of four consecutive units.  drop_threshold = min((uint64)(p 2^32), 2^32 - 1) drops a unit with probability p;
 * drop_threshold == 0 keeps every unit, and with keep_scale == 1 that is dropout switched off.
 *
 * Every operation of the epilogue above is rounded on its own (float32, no fused multiply-add; the division and the
 * square root are correctly rounded).  SUM has a fixed order.  The H / 4 groups of four consecutive units are dealt to
 * sixteen lanes: lane j owns the groups j, j + 16, j + 32, j + 48 that exist.  A lane adds its terms, from 0, groups
 * ascending and the four units of a group ascending (a lane without a group holds 0); then the sixteen partial sums
 * are added pairwise in four levels, p[j] + p[j ^ 1], then ^ 2, ^ 4, ^ 8 (a balanced tree over the lanes in order).
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_droq_critic blocks (HOST; the arrays they
 * point to are device memory).  The entry point enqueues exactly one kernel on `hip_stream` (hipStream_t; NULL = default
 * stream): no host synchronisation, no allocation.  Returns 0, or a negative code with the message in
 * rp_droq_last_error(); a refused call launches nothing.  Refused: a struct_size mismatch, null pointers that are not
 * marked optional below (the LayerNorm pointers included), n_critics outside [1, RP_DROQ_MAX_CRITICS], D, A or B < 1,
 * 2 A > RP_SAC_MAX_HEAD, H1 or H2 not a multiple of 16 in [16, RP_LEARN_MAX_H], obs_clip, keep_scale or ln_eps not > 0,
 * a row range outside the batch.  A range of zero rows is accepted and launches nothing.
 */
#ifndef RP_DROQ_H_
#define RP_DROQ_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_sac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_DROQ_MAX_CRITICS RP_SAC_MAX_CRITICS
#define RP_DROQ_COUNTER 32 /* the last Philox counter word of critic i, layer L is RP_DROQ_COUNTER + 2 i + L */

typedef struct rp_droq_critic { /* HOST */
  rp_learn_mlp net;             /* w1 [H1][D + A], w2 [H2][H1], w3 [1][H2]; torch.nn.Linear layout, read in place */
  const float *g1, *be1;        /* [H1]: LayerNorm weight and bias of hidden layer 1 */
  const float *g2, *be2;        /* [H2] */
} rp_droq_critic;

/* The TD target of the rows b of [row_first, row_first + row_count) of a batch of B.  A workgroup owns 16 rows and
 * evaluates the critics one after the other, keeping the running minimum in LDS. */
typedef struct rp_droq_target_args {
  size_t struct_size;
  const float* next_obs;         /* [B][D] */
  const float* action;           /* [B][A]: the policy's action at next_obs */
  const float* logp;             /* [B] */
  const float* reward;           /* [B] */
  const float* discount;         /* [B] */
  const float* mean;             /* [D] */
  const float* inv_std;          /* [D] */
  float obs_clip;                /* > 0 */
  float gamma;
  const float* log_alpha;        /* DEVICE, one float: the live parameter */
  const rp_droq_critic* critics; /* HOST [n_critics], copied into the launch */
  int n_critics;                 /* 1 .. RP_DROQ_MAX_CRITICS */
  float* y;                      /* [B] */
  float* q_min;                  /* [B], optional */
  float* q;                      /* [n_critics][B], optional: every critic's own value */
  uint32_t drop_threshold;       /* a unit is kept iff its Philox word >= drop_threshold */
  float keep_scale;              /* > 0: 1 / (1 - p) */
  float ln_eps;                  /* > 0 */
  uint32_t seed_lo, seed_hi, round;
  int D, H1, H2, A;
  int B, row_first, row_count;
  void* hip_stream;
} rp_droq_target_args;

int rp_droq_target(const rp_droq_target_args* args);

/* "max_critics", "tile_rows" (the rows of one workgroup), "max_hidden" (RP_LEARN_MAX_H), "max_actions"
 * (RP_LEARN_MAX_A); -1 otherwise */
int rp_droq_dim(const char* name);

const char* rp_droq_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_DROQ_H_ */
