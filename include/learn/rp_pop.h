/* learn/rp_pop.h — populations: the kernels of P independent DroQ learners that share one environment batch (C ABI,
 * gfx950, librp_pop.so).
 *
 * There are P members.  Member p owns the envs e with e % P == p of a batch of E (the task's own song rule), its own
 * networks, temperature, observation normaliser and minibatches.  The four launches here are rp_sac_sample, rp_sac_act
 * (learn/rp_sac.h), rp_droq_target (learn/rp_droq.h) and rp_learn_moments (learn/rp_learn.h) over all members at once:
 * one device text with those kernels (the same arithmetic, statement by statement), run on a member's rows with that
 * member's weight set.  Conventions are rp_sac.h's: no handle, no allocation, every array is the caller's.
 *
 * Layouts.  An array of member rows has `rows` rows per member, P rows in all, in one of two layouts:
 *     RP_POP_INTERLEAVED   row j of member p is array row p + P j          (the env rows: rows = E / P)
 *     RP_POP_BLOCKED       row j of member p is array row p rows + j       (the minibatches)
 * Per-member parameters are stacked and contiguous: member p's tensor is the p-th slice of [P][...].  The ABI passes the
 * base pointers (in the blocks of the single-learner ABI: rp_learn_mlp, rp_droq_critic) and derives the strides from the
 * dimensions: w1 [P][H1][K], b1 [P][H1], w2 [P][H2][H1], b2 [P][H2], w3 [P][N3][H2], b3 [P][N3], g1, be1 [P][H1], g2,
 * be2 [P][H2], mean, inv_std [P][D], log_alpha, gamma [P].
 *
 * Every entry point takes a member range [member_first, member_first + member_count) and a row range within the
 * member, [row_first, row_first + row_count) of [0, rows) (moments: the whole of the k slots it is given).  Rows and
 * members outside the ranges are not touched.
 *
 * Noise.  All of it is keyed by the ARRAY row, whichever member owns it: act's z(seed, round, r, u) with r the array row
 * (interleaved: the env index), sample's philox(round, p n + b, 0, 16 + j; seed) and target's dropout words of the
 * absolute row p n + j.  So a member's launch here and the single-learner kernel on the same array rows give the same
 * bits.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_learn_mlp and rp_droq_critic blocks (HOST;
 * the arrays they point to are device memory).  Every entry point enqueues exactly one kernel on `hip_stream`
 * (hipStream_t; NULL = default stream): no host synchronisation, no allocation.  Returns 0, or a negative code with the
 * message in rp_pop_last_error(); a refused call launches nothing.  Refused: what the single-learner entry point
 * refuses, and P < 1, E % P != 0, a member range outside [0, P), a row range outside [0, rows), P rows > 2^31 - 1,
 * (C - 1) (E / P) >= 2^32, an unknown layout or grid order.  A range of zero rows or zero members is accepted and
 * launches nothing.
 *
 * Grid order (act and target: `grid_order`).  A 16-row tile belongs to one member and reads that member's whole weight
 * set.  With T tiles per member, workgroup b of the member_count x T is
 *     RP_POP_TILE_MAJOR     member b % member_count, tile b / member_count
 *     RP_POP_MEMBER_MAJOR   member b / T, tile b % T
 * This changes which workgroups run side by side and nothing else: the results do not depend on it.
 */
#ifndef RP_POP_H_
#define RP_POP_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_droq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_POP_INTERLEAVED 0
#define RP_POP_BLOCKED 1
#define RP_POP_TILE_MAJOR 0
#define RP_POP_MEMBER_MAJOR 1

/* rp_sac_act's policy and epilogue on the rows of the members in range, each with its member's actor, mean and inv_std.
 * Outputs go to the array row the input came from.  Grid: member_count x ceil(row_count / 16) workgroups. */
typedef struct rp_pop_act_args {
  size_t struct_size;
  const float* obs;          /* [P rows][D] in `layout` */
  const float* mean;         /* [P][D] */
  const float* inv_std;      /* [P][D] */
  float obs_clip;            /* > 0 */
  float log_std_min, log_std_max;
  const rp_learn_mlp* actor; /* HOST: the bases of the stacked tensors; w3 [P][2 A][H2], b3 [P][2 A] */
  float* action;             /* [P rows][A] */
  float* logp;               /* [P rows] (deterministic == 0) */
  float* pre;                /* [P rows][A], optional */
  void* env_action;          /* [P rows][A] of `precision`, optional */
  int precision;             /* of env_action: 32 / 64 */
  int deterministic;
  uint32_t seed_lo, seed_hi, round;
  int D, H1, H2, A;
  int P, rows;               /* members, rows per member */
  int layout;                /* RP_POP_INTERLEAVED / RP_POP_BLOCKED */
  int grid_order;            /* RP_POP_TILE_MAJOR / RP_POP_MEMBER_MAJOR */
  int member_first, member_count;
  int row_first, row_count;
  void* hip_stream;
} rp_pop_act_args;

/* rp_sac_sample per member: member p's rows b of [row_first, row_first + row_count) go to the blocked rows p n + b.
 * With Em = E / P, F = min(n_written, C) and N = (F - 1) Em, for attempt j = 0 .. RP_SAC_SAMPLE_TRIES - 1:
 *     w = philox(round, p n + b, 0, 16 + j; seed_lo, seed_hi).word[0];   i = ((uint64)w N) >> 32
 *     t = i / Em;  jj = i % Em;  e = p + P jj;  m = n_written - F + t
 * and rp_sac_sample's validity rule, copies, mask and zeros; index = (m mod C) E + e. */
typedef struct rp_pop_sample_args {
  size_t struct_size;
  const float* ring_obs;         /* [C][E][D] */
  const float* ring_action;      /* [C][E][A] */
  const float* ring_reward;      /* [C][E] */
  const float* ring_discount;    /* [C][E] */
  const int32_t* ring_step_type; /* [C][E] */
  float* obs;                    /* [P n][D], blocked */
  float* next_obs;               /* [P n][D] */
  float* action;                 /* [P n][A] */
  float* reward;                 /* [P n] */
  float* discount;               /* [P n] */
  float* mask;                   /* [P n] */
  int32_t* index;                /* [P n], optional */
  long long n_written;           /* >= 2 */
  uint32_t seed_lo, seed_hi, round;
  int C, E, D, A;
  int P, n;                      /* members, minibatch rows per member */
  int member_first, member_count;
  int row_first, row_count;
  void* hip_stream;
} rp_pop_sample_args;

/* rp_droq_target on the blocked rows p n + j of the members in range, with member p's critics, log_alpha[p], gamma[p],
 * mean[p] and inv_std[p].  The dropout words are keyed by the absolute row p n + j.  drop_threshold == 0 with
 * keep_scale == 1 is dropout switched off. */
typedef struct rp_pop_target_args {
  size_t struct_size;
  const float* next_obs;         /* [P n][D] */
  const float* action;           /* [P n][A] */
  const float* logp;             /* [P n] */
  const float* reward;           /* [P n] */
  const float* discount;         /* [P n] */
  const float* mean;             /* [P][D] */
  const float* inv_std;          /* [P][D] */
  float obs_clip;                /* > 0 */
  const float* gamma;            /* DEVICE [P] */
  const float* log_alpha;        /* DEVICE [P]: the live parameters */
  const rp_droq_critic* critics; /* HOST [n_critics]: the bases of the stacked tensors of critic i */
  int n_critics;                 /* 1 .. RP_DROQ_MAX_CRITICS */
  float* y;                      /* [P n] */
  float* q_min;                  /* [P n], optional */
  float* q;                      /* [n_critics][P n], optional */
  uint32_t drop_threshold;
  float keep_scale;              /* > 0 */
  float ln_eps;                  /* > 0 */
  uint32_t seed_lo, seed_hi, round;
  int D, H1, H2, A;
  int P, n;
  int grid_order;                /* RP_POP_TILE_MAJOR / RP_POP_MEMBER_MAJOR */
  int member_first, member_count;
  int row_first, row_count;
  void* hip_stream;
} rp_pop_target_args;

/* rp_learn_moments per member over k consecutive ring slots [k][E][D] starting at `obs`: with Em = E / P, member p's
 * logical row r = t Em + jj of n_rows = k Em is obs[(t E + p + P jj) D]; the lane rule and the merge are
 * rp_learn_moments' over r.  `count` is the host's, the same for every member.  Grid: ceil(D / 16) x member_count. */
typedef struct rp_pop_moments_args {
  size_t struct_size;
  const float* obs;   /* [k][E][D] */
  double* mean;       /* [P][D] */
  double* M2;         /* [P][D] */
  float* mean_f32;    /* [P][D] */
  float* inv_std_f32; /* [P][D] */
  double count;       /* rows merged so far, per member; >= 0 */
  double eps;         /* > 0 */
  int k, E, D, P;     /* k >= 1 slots */
  int member_first, member_count;
  void* hip_stream;
} rp_pop_moments_args;

int rp_pop_act(const rp_pop_act_args* args);
int rp_pop_sample(const rp_pop_sample_args* args);
int rp_pop_target(const rp_pop_target_args* args);
int rp_pop_moments(const rp_pop_moments_args* args);

/* "interleaved", "blocked", "tile_major", "member_major" (the codes above), "default_grid_order" (what a caller that
 * does not care passes), "tile_rows", "max_critics", "sample_tries", "max_hidden", "max_actions", "moment_lanes"; -1
 * otherwise */
int rp_pop_dim(const char* name);

const char* rp_pop_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_POP_H_ */
