/* learn/rp_pop_critic.h — the fused DroQ critic step of a population: rp_critic_step (learn/rp_critic.h) for every member
 * of a range in the same two launches (C ABI, gfx950, librp_pop_critic.so).
 *
 * Conventions are rp_critic.h's and rp_pop.h's: argument blocks with struct_size, no handle, no allocation, every array
 * is the caller's (the workspace too: rp_pop_critic_workspace reports its size), one stream, no host synchronisation,
 * nothing read back.
 *
 * MEANING.  There are P members with n minibatch rows each, blocked (rp_pop.h: row j of member p is array row p n + j).
 * For every member p of [member_first, member_first + member_count) the call is rp_critic_step with
 *     obs, action, y, mask, q            the arrays of P n rows (q [n_critics][P n]), B = P n,
 *                                        row_first = p n + row_first, row_count = row_count;
 *     p, m, v, target, grad              member p's slices of the stacked tensors [P][...] whose bases the rp_critic_set
 *                                        blocks hold; the strides are derived from the dimensions, as in rp_pop.h:
 *                                        w1 [P][H1][D + A], b1, g1, be1 [P][H1], w2 [P][H2][H1], b2, w3, g2, be2 [P][H2],
 *                                        b3 [P][1];
 *     mean, inv_std                      mean[p], inv_std[p] of [P][D];
 *     the workspace                      segment p - member_first of the caller's workspace, each segment being
 *                                        rp_critic_workspace's size for (n_critics, H1, H2, row_count);
 *     everything else                    as given: the Adam and Polyak scalars and (seed, round) are shared, the members
 *                                        step together and one step count serves them all.
 * So M = fmaxf(MSUM(mask over the member's range), 1) is the member's own, and the dropout words are keyed by the
 * absolute row p n + j, as rp_pop_target's are.  Statement by statement the arithmetic is rp_critic.h's and is not
 * restated here: member p's q rows, gradients, p, m, v and target have the bits rp_critic_step gives when called as
 * above.  Rows and members outside the ranges are not touched.
 *
 * LAUNCHES: exactly two per call, whatever P, the sizes and n_critics are; the members are flattened into grid x.
 *   1. rows:  grid (member_count x tiles of 16 rows, critics).
 *   2. apply: grid (member_count x (16-column tiles of w1 + of w2 + blocks of 256 vector elements), critics).
 * `grid_order` is rp_pop.h's rule for both, with a member's tiles (rows) or blocks (apply) as T:
 *     RP_POP_TILE_MAJOR     member b % member_count, tile b / member_count
 *     RP_POP_MEMBER_MAJOR   member b / T, tile b % T
 * It changes which workgroups run side by side and nothing else.  Both reductions have one order: no atomics, and no
 * block reads what another block of the same launch wrote.  `launches` takes rp_critic.h's three values.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_critic_set blocks (HOST; the arrays they
 * point to are device memory).  Returns 0, or a negative code with the message in rp_pop_critic_last_error(); a refused
 * call launches nothing.  Refused: what rp_critic_step refuses; what rp_pop_target refuses about P, the member range,
 * the row range within [0, n), P n > 2^31 - 1 and the grid order; a workspace smaller than rp_pop_critic_workspace's
 * answer (or not 16-byte aligned).  A range of zero rows or zero members is accepted and launches nothing.
 */
#ifndef RP_POP_CRITIC_H_
#define RP_POP_CRITIC_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_critic.h"
#include "rp_pop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rp_pop_critic_step_args {
  size_t struct_size;
  const float* obs;            /* [P n][D], blocked */
  const float* action;         /* [P n][A] */
  const float* y;              /* [P n] */
  const float* mask;           /* [P n] */
  const float* mean;           /* [P][D] */
  const float* inv_std;        /* [P][D] */
  float obs_clip;              /* > 0 */
  const rp_critic_set* p;      /* HOST [n_critics]: the bases of the stacked live critics, updated in place */
  const rp_critic_set* m;      /* HOST [n_critics]: of Adam's stacked first moments */
  const rp_critic_set* v;      /* HOST [n_critics]: of Adam's stacked second moments */
  const rp_critic_set* target; /* HOST [n_critics]: of the stacked target critics */
  const rp_critic_set* grad;   /* HOST [n_critics], optional, and each of its pointers optional: of stacked gradients */
  int n_critics;               /* 1 .. RP_DROQ_MAX_CRITICS */
  float* q;                    /* [n_critics][P n]: the critics' values before the step */
  void* workspace;             /* at least rp_pop_critic_workspace's answer; 16-byte aligned */
  size_t workspace_bytes;
  uint32_t drop_threshold;
  float keep_scale;            /* > 0 */
  float ln_eps;                /* > 0 */
  uint32_t seed_lo, seed_hi, round;
  float one_minus_beta1, beta2, one_minus_beta2;
  float step_size;             /* > 0: lr / (1 - beta1^t) */
  float bc2_sqrt;              /* > 0: sqrt(1 - beta2^t) */
  float eps;                   /* > 0 */
  float tau;                   /* in [0, 1] */
  int D, H1, H2, A;
  int P, n;                    /* members, minibatch rows per member */
  int grid_order;              /* RP_POP_TILE_MAJOR / RP_POP_MEMBER_MAJOR */
  int member_first, member_count;
  int row_first, row_count;    /* within the member */
  int launches;                /* RP_CRITIC_STEP, RP_CRITIC_ROWS_ONLY or RP_CRITIC_APPLY_ONLY */
  void* hip_stream;
} rp_pop_critic_step_args;

int rp_pop_critic_step(const rp_pop_critic_step_args* args);

/* The size query: sets `bytes` to member_count times rp_critic_workspace's answer for (n_critics, H1, H2, row_count). */
typedef struct rp_pop_critic_workspace_args {
  size_t struct_size;
  int n_critics, H1, H2, row_count, member_count;
  size_t bytes; /* out */
} rp_pop_critic_workspace_args;

int rp_pop_critic_workspace(rp_pop_critic_workspace_args* args);

/* rp_critic_dim's names ("max_critics", "tile_rows", "stage_rows", "launches", "counter", "max_hidden", "max_actions")
 * and "tile_major", "member_major", "default_grid_order" of rp_pop_dim; -1 otherwise */
int rp_pop_critic_dim(const char* name);

const char* rp_pop_critic_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_POP_CRITIC_H_ */
