/* learn/rp_sac.h — the batched kernels of an on-device off-policy learner: a replay ring's sampler, the tanh-squashed
 * Gaussian policy and the TD target of soft actor-critic (C ABI, gfx950, librp_sac.so).
 *
 * Soft actor-critic (Haarnoja et al. 2018) over thousands of envs.  The replay buffer lives on the device, is written
 * by the step path itself and is never read back; the gradient step is the caller's (autograd).  This library is the
 * three launches without gradients: `sample` (a minibatch out of the ring), `act` (the policy, while collecting and on
 * the next observations of a minibatch) and `target` (the ensemble of target critics, their minimum and the TD target).
 * It has no handle and allocates nothing: every array is the caller's.  Conventions are learn/rp_learn.h's.
 *
 * The replay ring is rp_learn.h's rollout storage closed into a ring of C slots of E rows: obs [C][E][D] f32, reward
 * [C][E] f32, discount [C][E] f32, step_type [C][E] i32, and action [C][E][A] f32, the squashed action decided at that
 * slot.  TimeStep number m (counted from 0 since the first reset) lives in slot m mod C; the unchanged rp_learn_pack
 * writes it (there is no push kernel).  The host owns n_written, the number of TimeSteps written so far; it does not
 * depend on data.  With F = min(n_written, C), the candidate transitions are the TimeStep numbers m of
 * [n_written - F, n_written - 2]:
 *     (obs[m], action[m], reward[m+1], discount[m+1], obs[m+1]) of one env,
 *     valid iff step_type[m] != LAST and step_type[m+1] != FIRST                                   (rp_learn_gae's rule).
 * The newest slot has no successor and is never drawn; the pair (newest, oldest) across the wrap is not a transition and
 * is never drawn; the next observation is never stored twice.
 *
 * Networks are rp_learn_mlp: two tanh hidden layers, weights in torch.nn.Linear's layout [out][in], float32, contiguous,
 * read in place.  The actor is D -> H1 -> H2 -> 2 A (A means, then A log standard deviations); a critic is
 * (D + A) -> H1 -> H2 -> 1 on cat([normalised observation, action]).
 *
 * Noise.  z(seed, round, e, u) is the planner's (plan/rp_plan.h).  The sampler's words are
 * philox(round, b, 0, 16 + j; seed): their last counter word is 16 .. 19, z's is 0 .. 2.
 *
 * Every float operation of act's and target's normaliser and epilogue is rounded on its own (no fused multiply-add);
 * the matrix products are float32 fused-multiply-add chains over k ascending, starting from 0, the bias added
 * afterwards.  sample copies bits.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_learn_mlp blocks (HOST).  Every entry point
 * enqueues exactly one kernel on `hip_stream` (hipStream_t; NULL = default stream): no host synchronisation, no
 * allocation.  Returns 0, or a negative code with the message in rp_sac_last_error(); a refused call launches nothing.
 * Refused: a struct_size mismatch, null pointers that are not marked optional below, C < 2, n_written < 2, E, D, A or B
 * < 1, (min(n_written, C) - 1) E >= 2^32, a row range outside the batch, 2 A > RP_SAC_MAX_HEAD, H1 or H2 not a multiple
 * of 16 in [16, RP_LEARN_MAX_H], obs_clip <= 0, log_std_min > log_std_max, precision other than 32 / 64 where env_action
 * is given, n_critics outside [1, RP_SAC_MAX_CRITICS].  A range of zero rows is accepted and launches nothing.
 */
#ifndef RP_SAC_H_
#define RP_SAC_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_SAC_MAX_CRITICS 4
#define RP_SAC_SAMPLE_TRIES 4
#define RP_SAC_MAX_HEAD 256 /* 2 A <= RP_SAC_MAX_HEAD: A <= RP_LEARN_MAX_A */

/* One minibatch row per wave, for the rows b of [row_first, row_first + row_count) of a batch of B.  With
 * F = min(n_written, C) and N = (F - 1) E, for attempt j = 0 .. RP_SAC_SAMPLE_TRIES - 1:
 *     w = philox(round, b, 0, 16 + j; seed_lo, seed_hi).word[0];   i = ((uint64)w N) >> 32
 *     t = i / E;  e = i % E;  m = n_written - F + t
 * and the first valid attempt wins: obs[b] = ring obs[m mod C][e], next_obs[b] = ring obs[(m+1) mod C][e], action[b] =
 * ring action[m mod C][e], reward[b] and discount[b] those of slot (m+1) mod C, mask[b] = 1, index[b] = (m mod C) E + e.
 * A row with no valid attempt gets mask 0, index -1 and zeros everywhere else.  Copies are bit-exact and go in the
 * widest unit both rows allow (16, 8 or 4 bytes, after a head of single elements), as rp_learn_pack's. */
typedef struct rp_sac_sample_args {
  size_t struct_size;
  const float* ring_obs;         /* [C][E][D] */
  const float* ring_action;      /* [C][E][A] */
  const float* ring_reward;      /* [C][E] */
  const float* ring_discount;    /* [C][E] */
  const int32_t* ring_step_type; /* [C][E] */
  float* obs;                    /* [B][D] */
  float* next_obs;               /* [B][D] */
  float* action;                 /* [B][A] */
  float* reward;                 /* [B] */
  float* discount;               /* [B] */
  float* mask;                   /* [B] */
  int32_t* index;                /* [B], optional */
  long long n_written;           /* >= 2 */
  uint32_t seed_lo, seed_hi, round;
  int C, E, D, A;
  int B, row_first, row_count;
  void* hip_stream;
} rp_sac_sample_args;

/* The policy on the rows e of [row_first, row_first + row_count) of obs [n_rows][D]:
 *     d = x - mean[j];  p = d * inv_std[j];  xn = fmin(fmax(p, -obs_clip), obs_clip)
 *     h1 = tanhf(W1 xn + b1);  h2 = tanhf(W2 h1 + b2);  out = W3 h2 + b3                    (2 A entries)
 * and per entry u < A:
 *     m = out[u];  l = out[A+u];  ls = fminf(fmaxf(l, log_std_min), log_std_max)
 *     zf = (float)z(seed, round, e, u);  sd = expf(ls);  t = sd zf;  p = m + t               (deterministic: p = m)
 *     a = tanhf(p)
 *     w = -2 p;  sp = fmaxf(w, 0) + log1pf(expf(-fabsf(w)));  lg = 2 (((float)ln 2 - p) - sp)   (= log(1 - tanh^2 p))
 *     g = ((-0.5f (zf zf)) - ls) - lg;   logp = (sum of g over u ascending, from 0) - (float)(0.5 A ln 2 pi)
 * Writes action = a, logp (not when deterministic), pre = p where given, env_action = (precision)a where given (a lies
 * in [-1, 1]: no clamp). */
typedef struct rp_sac_act_args {
  size_t struct_size;
  const float* obs;          /* [n_rows][D] */
  const float* mean;         /* [D] */
  const float* inv_std;      /* [D] */
  float obs_clip;            /* > 0 */
  float log_std_min, log_std_max;
  const rp_learn_mlp* actor; /* HOST, copied into the launch; w3 [2 A][H2], b3 [2 A] */
  float* action;             /* [n_rows][A] */
  float* logp;               /* [n_rows] (deterministic == 0) */
  float* pre;                /* [n_rows][A], optional */
  void* env_action;          /* [n_rows][A] of `precision`, optional */
  int precision;             /* of env_action: 32 / 64 */
  int deterministic;
  uint32_t seed_lo, seed_hi, round;
  int D, H1, H2, A;
  int n_rows, row_first, row_count;
  void* hip_stream;
} rp_sac_act_args;

/* The TD target of the rows b of [row_first, row_first + row_count) of a batch of B.  A workgroup owns 16 rows and
 * evaluates the critics i = 0 .. n_critics - 1 one after the other on cat([xn, action]) (xn: act's normaliser on
 * next_obs), keeping the running minimum in LDS: qm = fminf over i ascending.  Then
 *     al = expf(*log_alpha);  s = al logp;  v = qm - s;  nv = gamma discount;  tv = nv v;  y = reward + tv */
typedef struct rp_sac_target_args {
  size_t struct_size;
  const float* next_obs;       /* [B][D] */
  const float* action;         /* [B][A]: the policy's action at next_obs */
  const float* logp;           /* [B] */
  const float* reward;         /* [B] */
  const float* discount;       /* [B] */
  const float* mean;           /* [D] */
  const float* inv_std;        /* [D] */
  float obs_clip;              /* > 0 */
  float gamma;
  const float* log_alpha;      /* DEVICE, one float: the live parameter */
  const rp_learn_mlp* critics; /* HOST [n_critics], copied into the launch; w1 [H1][D + A], w3 [1][H2] */
  int n_critics;               /* 1 .. RP_SAC_MAX_CRITICS */
  float* y;                    /* [B] */
  float* q_min;                /* [B], optional */
  int D, H1, H2, A;
  int B, row_first, row_count;
  void* hip_stream;
} rp_sac_target_args;

int rp_sac_sample(const rp_sac_sample_args* args);
int rp_sac_act(const rp_sac_act_args* args);
int rp_sac_target(const rp_sac_target_args* args);

/* "max_critics", "sample_tries", "tile_rows" (the rows of one workgroup of act and target), "max_hidden"
 * (RP_LEARN_MAX_H), "max_actions" (RP_LEARN_MAX_A); -1 otherwise */
int rp_sac_dim(const char* name);

const char* rp_sac_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_SAC_H_ */
