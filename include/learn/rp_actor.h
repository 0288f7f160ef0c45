/* learn/rp_actor.h — the actor's and the temperature's step of DroQ in two launches: the policy at the rows' observations,
 * every live critic at the policy's action, the minimum over the ensemble, the gradient through the selected critic's
 * action input, the squashed-Gaussian head and the two tanh layers, Adam on the actor's six tensors and on log_alpha, and
 * the step's statistics (C ABI, gfx950, librp_actor.so).
 *
 * Conventions are rp_critic.h's: argument blocks with struct_size, no handle, no allocation, every array is the caller's
 * (the workspace too: rp_actor_workspace reports its size), one stream, no host synchronisation, nothing read back.
 *
 * The actor is rp_sac.h's: D -> H1 -> H2 -> 2 A, two tanh layers, torch.nn.Linear's layout; its six tensors are numbered
 * RP_ACTOR_W1 .. RP_ACTOR_B3.  A critic is rp_critic.h's, as an rp_critic_set, read only.  The step covers the rows b of
 * [row_first, row_first + row_count) of a batch of B.  SUM, MSUM, FORWARD, BACKWARD and ADAM below are rp_critic.h's.
 *
 * 1. POLICY, row b.  rp_sac_act's normaliser xn, layers and epilogue (the products: fused-multiply-add chains over k
 *    ascending, from 0, then the bias; h1 = tanhf(s1), h2 = tanhf(s2); the head out = [m[0 .. A), l[0 .. A)]):
 *        lc = fmaxf(l[u], log_std_min);  ls = fminf(lc, log_std_max);  inside[u] = l[u] > log_std_min && l[u] < log_std_max
 *        zf = (float) za(seed, round, b, u);  sd = expf(ls);  t[u] = sd zf;  p = m[u] + t[u];  a[u] = tanhf(p)
 *        w = -2 p;  aw = fabsf(w);  ex = expf(-aw);  l1 = log1pf(ex);  wp = fmaxf(w, 0);  sp = wp + l1
 *        c1 = ln2 - p;  c2 = c1 - sp;  lg = 2 c2;  q = zf zf;  h = -0.5 q;  g0 = h - ls;  term[u] = g0 - lg
 *        logp = (the sum over u ascending, from 0, of term[u]) - (float)(0.5 A ln 2 pi)
 *    za is the planner's z (plan/rp_plan.h) with the last Philox counter word moved: its three words are
 *    philox(round, b, u, RP_ACTOR_NOISE_COUNTER + j; seed), j = 0, 1, 2.  (rp_sac_act has used z itself, counter words
 *    0 .. 2, on these rows for the next observations' actions.)  b is the ABSOLUTE batch row.
 * 2. CRITICS.  Critic i, ascending, on x = cat([xn, a]) by FORWARD, its dropout words being
 *    philox(round, b, n >> 2, RP_ACTOR_COUNTER + 2 i + L; seed).  qm = q_0, best = 0; a later critic replaces them only
 *    when its q is strictly smaller: qm is the q of the first critic, ascending, that attains the minimum.
 *    The counter words: 64 .. 66 (noise) and 80 .. 87 (dropout), clear of the policy (0 .. 2), the sampler (16 .. 19), the
 *    targets (32 .. 39) and the critic step (48 .. 55): one (seed, round) serves all six.
 * 3. LOSS and HEAD GRADIENT.  M = fmaxf(MSUM(mask), 1);  w = mask[b] / M;  al = expf(*log_alpha) as it is before the step.
 *        s1 = al logp;  s2 = s1 - qm;  la[b] = w s2                          (L_actor = the sum over b of la[b])
 *    dqa[u] = d qm / d a[u] from critic `best` alone: BACKWARD with dq = 1 (dout2[n] = w3[n]), then
 *        dqa[u] = the chain over n ascending, from 0, of ds1[n] W1[n][D + u]
 *    Only these A columns of W1 are read; no parameter gradient of a critic is formed.  Then (d logp / d p = 2 tanh p)
 *        wa = al w;  e1 = 2 a[u];  e2 = wa e1;  aa = a[u] a[u];  om = 1 - aa;  f1 = w dqa[u];  f2 = f1 om;  dp = e2 - f2
 *        dm[u] = dp;   dt = dp t[u];  dl[u] = inside[u] ? dt - wa : 0
 * 4. ACTOR BACKWARD, row-local.  dout3 = [dm, dl];
 *        dh2[k] = the chain over n ascending of dout3[n] W3[n][k];  hh = h2[k] h2[k];  om = 1 - hh;  ds2[k] = dh2[k] om
 *        dh1[k] = the chain over n ascending of ds2[n] W2[n][k];    hh = h1[k] h1[k];  om = 1 - hh;  ds1[k] = dh1[k] om
 *    PARAMETER GRADIENTS in the critic step's fixed order (no atomics): db1 += ds1, db2 += ds2, db3 += dout3 over a tile of
 *    16 consecutive rows ascending, from 0, then the tiles ascending, from 0; dW1[n][k] = the chain over the rows b of the
 *    range ascending, from 0, of ds1[b][n] xn[b][k] (MFMA; xn read from obs and normalised in place), dW2 of ds2[b][n]
 *    h1[b][k], dW3 of dout3[b][n] h2[b][k].  Then ADAM per element with `actor_adam`'s scalars; no Polyak step (the actor
 *    has no target).
 * 5. TEMPERATURE.  lt = logp + target_entropy;  gt[b] = w lt;  g = -(the sum over b of gt[b]);  ADAM on log_alpha's one
 *    element with `alpha_adam`'s scalars.
 * 6. STATISTICS.  stats[0] = actor_loss = sum la[b];  stats[1] = alpha_loss = log_alpha_before g;  stats[2] = alpha =
 *    expf(log_alpha after the step);  en[b] = w logp;  stats[3] = entropy = -(sum en[b]);  stats[4] = masked =
 *    1 - (sum mask[b]) / (float)row_count.  Every "sum over b" here: a tile's rows ascending, from 0, then the tiles
 *    ascending, from 0.
 * 7. An all-masked range (M = 1, every w = 0) is ADAM on a zero gradient.  A range of zero rows launches nothing.
 *
 * LAUNCHES: exactly two per call, whatever B, the sizes and n_critics are.
 *   1. rows:  grid (tiles of 16 rows).  The policy, the critics one after the other with the selection, the head gradient
 *             and the actor's row-local backward; writes the optional per-row outputs, and into the workspace h1, h2, ds1,
 *             ds2, dout3 and the tile's partial sums of the biases and of the four scalar sums.
 *   2. apply: grid (16-column tiles of w1, then of w2, then of w3, then blocks of 256 bias elements, then one block for the
 *             temperature and the statistics).  The batch reduction, then Adam, in the epilogue.  A gradient reaches memory
 *             only where its pointer asks for it.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_critic_set blocks (HOST; the arrays they
 * point to are device memory).  Returns 0, or a negative code with the message in rp_actor_last_error(); a refused call
 * launches nothing.  Refused: a struct_size mismatch, NULL pointers not marked optional (log_alpha, stats, every m and v
 * among them), n_critics outside [1, RP_DROQ_MAX_CRITICS], D, A or B < 1, 2 A > RP_SAC_MAX_HEAD, H1 or H2 not a multiple of
 * 16 in [16, RP_LEARN_MAX_H], obs_clip, keep_scale or ln_eps not > 0, log_std_min > log_std_max, a row range outside the
 * batch, a workspace smaller than rp_actor_workspace's answer (or not 16-byte aligned), step_size, bc2_sqrt or eps of
 * either optimiser not > 0, `launches` not one of its three values.  A range of zero rows is accepted and launches nothing.
 */
#ifndef RP_ACTOR_H_
#define RP_ACTOR_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_ACTOR_NOISE_COUNTER 64 /* the last Philox counter words of the step's draw are RP_ACTOR_NOISE_COUNTER + 0 .. 2 */
#define RP_ACTOR_COUNTER 80       /* the last Philox counter word of critic i, layer L is RP_ACTOR_COUNTER + 2 i + L */
#define RP_ACTOR_PARAMS 6
#define RP_ACTOR_STATS 5
enum { RP_ACTOR_W1, RP_ACTOR_B1, RP_ACTOR_W2, RP_ACTOR_B2, RP_ACTOR_W3, RP_ACTOR_B3 };
enum { RP_ACTOR_LOSS, RP_ACTOR_ALPHA_LOSS, RP_ACTOR_ALPHA, RP_ACTOR_ENTROPY, RP_ACTOR_MASKED };

enum { RP_ACTOR_STEP = 0, RP_ACTOR_ROWS_ONLY = 1, RP_ACTOR_APPLY_ONLY = 2 };

typedef struct rp_actor_set { /* the six tensors of the actor (or of its m, v or gradient): device pointers */
  float* t[RP_ACTOR_PARAMS];
} rp_actor_set;

typedef struct rp_actor_adam { /* Adam's scalars of one optimiser at its own step count, as rp_critic_step_args has them */
  float one_minus_beta1, beta2, one_minus_beta2;
  float step_size; /* > 0: lr / (1 - beta1^t) */
  float bc2_sqrt;  /* > 0: sqrt(1 - beta2^t) */
  float eps;       /* > 0 */
} rp_actor_adam;

typedef struct rp_actor_step_args {
  size_t struct_size;
  const float* obs;             /* [B][D] */
  const float* mask;            /* [B] */
  const float* mean;            /* [D] */
  const float* inv_std;         /* [D] */
  float obs_clip;               /* > 0 */
  rp_actor_set p;               /* the actor, updated in place */
  rp_actor_set m;               /* Adam's first moments, updated in place */
  rp_actor_set v;               /* Adam's second moments, updated in place */
  rp_actor_set grad;            /* each pointer optional: the gradients */
  const rp_critic_set* critics; /* HOST [n_critics]: the live critics, read only */
  int n_critics;                /* 1 .. RP_DROQ_MAX_CRITICS */
  float* log_alpha;             /* [1], updated in place */
  float* log_alpha_m;           /* [1] */
  float* log_alpha_v;           /* [1] */
  float* log_alpha_grad;        /* [1], optional */
  float target_entropy;
  float log_std_min, log_std_max;
  void* workspace;              /* at least rp_actor_workspace's answer; 16-byte aligned */
  size_t workspace_bytes;
  uint32_t drop_threshold;      /* a unit is kept iff its Philox word >= drop_threshold */
  float keep_scale;             /* > 0: 1 / (1 - p) */
  float ln_eps;                 /* > 0 */
  uint32_t seed_lo, seed_hi, round;
  rp_actor_adam actor_adam;     /* the actor's optimiser */
  rp_actor_adam alpha_adam;     /* the temperature's optimiser */
  float* action;                /* [B][A], optional: a */
  float* logp;                  /* [B], optional */
  float* q_min;                 /* [B], optional: qm */
  float* stats;                 /* [RP_ACTOR_STATS] */
  int D, H1, H2, A;
  int B, row_first, row_count;
  int launches;                 /* RP_ACTOR_STEP: both launches, a step; the other two values run one launch alone, for
                                   measurement (the apply launch then reads whatever the workspace holds) */
  void* hip_stream;
} rp_actor_step_args;

int rp_actor_step(const rp_actor_step_args* args);

/* The size query: sets `bytes` to what rp_actor_step needs for these sizes (a pure function of them):
 * 4 ((2 H1 + 2 H2 + 2 A) row_count + ceil(row_count / 16) (H1 + H2 + 2 A + 4)) bytes, rounded up to a multiple of 16. */
typedef struct rp_actor_workspace_args {
  size_t struct_size;
  int H1, H2, A, row_count;
  size_t bytes; /* out */
} rp_actor_workspace_args;

int rp_actor_workspace(rp_actor_workspace_args* args);

/* "max_critics", "tile_rows" (the rows of one workgroup of the rows launch), "stage_rows" (the rows one stage of the
 * apply launch's reduction holds), "launches" (2), "noise_counter", "counter", "max_hidden", "max_actions", "stats";
 * -1 otherwise */
int rp_actor_dim(const char* name);

const char* rp_actor_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_ACTOR_H_ */
