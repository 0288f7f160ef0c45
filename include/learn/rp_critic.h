/* learn/rp_critic.h — one critic step of DroQ in two launches: the forward pass of every critic of the ensemble, the
 * backward pass, the parameter gradients, Adam and the targets' Polyak step (C ABI, gfx950, librp_critic.so).
 *
 * Conventions are rp_droq.h's: argument blocks with struct_size, no handle, no allocation, every array is the caller's
 * (the workspace too: rp_critic_workspace reports its size), one stream, no host synchronisation, nothing read back.
 *
 * A critic is rp_droq.h's: (D + A) -> H1 -> H2 -> 1 on x = cat([xn(obs), action]), xn being rp_sac_act's normaliser.  Its
 * ten parameter tensors are numbered as rp_droq_critic lists them (RP_CRITIC_W1 ..): w1 [H1][D + A], b1, w2 [H2][H1], b2,
 * w3 [1][H2], b3, g1, be1, g2, be2.  The step covers the rows b of [row_first, row_first + row_count) of a batch of B.
 *
 * FORWARD, for critic i, row b, hidden layer L in {0, 1} (rp_droq.h's statements; SUM is rp_droq.h's SUM: sixteen lanes,
 * lane j owning the groups j, j + 16, .. of four units, then a balanced tree):
 *     s[n]  = (fused-multiply-add chain over k ascending, from 0, of in[k] W[n][k]) + bb[n]
 *     words = philox(round, b, n >> 2, RP_CRITIC_COUNTER + 2 i + L; seed_lo, seed_hi);  keep = words.w[n & 3] >= drop_threshold
 *     h[n]  = keep ? s[n] * keep_scale : 0
 *     mu = SUM(h) / (float)H;  d[n] = h[n] - mu;  var = SUM(d d) / (float)H;  t = var + ln_eps;  r = 1 / sqrtf(t)
 *     o[n]  = d[n] * r;  u = o[n] * g[n];  u = u + be[n];  out[n] = fmaxf(u, 0)
 *     q     = SUM(out2[n] * w3[n]) + b3            (the head: the products in SUM's order, not a chain)
 * b is the ABSOLUTE batch row.  The last counter word is 48 .. 55: clear of the policy (0 .. 2), the sampler (16 .. 19) and
 * the target critics (32 .. 39), so one (seed, round) serves all four.
 *
 * LOSS.  L = sum_i sum_b mask[b] 0.5 (q[i][b] - y[b])^2 / M over the range, M = fmaxf(MSUM(mask), 1); MSUM: thread t of 256
 * adds mask[row_first + t + 256 j], j ascending, from 0; the 256 partial sums are added in a balanced tree (p[t] + p[t + 128],
 * then + 64, .. + 1).  e = q - y;  f = mask e;  dq = f / M.
 *
 * BACKWARD, row-local, layer 2 then layer 1 (dout2[n] = dq w3[n]; dout1[k] = the chain over n ascending of ds2[n] W2[n][k]):
 *     dz[n] = out[n] > 0 ? dout[n] : 0;   c[n] = dz[n] g[n];   m1 = SUM(c) / (float)H;   m2 = SUM(c o) / (float)H
 *     t1 = c[n] - m1;  t2 = o[n] m2;  t3 = t1 - t2;  dh = r t3;   ds[n] = keep ? dh keep_scale : 0
 * The gradient with respect to x is never formed.
 *
 * PARAMETER GRADIENTS, in a fixed order that does not depend on how many workgroups run at a time (no atomics):
 *     vectors: a tile of 16 consecutive rows of the range (the last one may be short) adds its rows ascending, from 0:
 *              db[n] += ds[n], dg[n] += dz[n] o[n], dbe[n] += dz[n], dw3[n] += dq out2[n], db3 += dq
 *              (each product rounded, then added); the tiles' partial sums are then added ascending, from 0.
 *     matrices: dW1[n][k] = the chain over the rows b of the range ascending, from 0, of ds1[b][n] x[b][k] (MFMA, four rows
 *              per instruction; x is read from obs / action and normalised in place); dW2[n][k] likewise of ds2[b][n]
 *              out1[b][k].
 *
 * ADAM and POLYAK, per parameter element, every operation rounded on its own (no fused multiply-add; correctly rounded
 * square root and divisions), as torch's Adam with its defaults computes them:
 *     a = g - m;  a = a one_minus_beta1;  m = m + a
 *     c = g one_minus_beta2;  c = c g;  v = v beta2;  v = v + c
 *     den = sqrtf(v) / bc2_sqrt;  den = den + eps;  u = m / den;  u = u step_size;  p = p - u
 *     w = p - t;  w = w tau;  t = t + w                         (the matching target parameter)
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) are the caller's, computed in double.
 *
 * LAUNCHES: exactly two per call, whatever B, the sizes and n_critics are.
 *   1. rows:  grid (tiles of 16 rows, critics).  Forward, loss gradient, row-local backward; writes q, and into the
 *             workspace ds1, out1, ds2 and the tile's partial sums of the vector parameters.
 *   2. apply: grid (16-column tiles of w1, then of w2, then blocks of 256 vector elements; critics).  The batch reduction,
 *             then Adam, then Polyak, in the epilogue.  A gradient reaches memory only where `grad` asks for it.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except the rp_critic_set blocks (HOST; the arrays they
 * point to are device memory).  Returns 0, or a negative code with the message in rp_critic_last_error(); a refused call
 * launches nothing.  Refused: what rp_droq_target refuses (a struct_size mismatch, NULL pointers not marked optional,
 * n_critics outside [1, RP_DROQ_MAX_CRITICS], D, A or B < 1, 2 A > RP_SAC_MAX_HEAD, H1 or H2 not a multiple of 16 in
 * [16, RP_LEARN_MAX_H], obs_clip, keep_scale or ln_eps not > 0, a row range outside the batch), and a NULL m, v, target or
 * workspace, a workspace smaller than rp_critic_workspace's answer (or not 16-byte aligned), tau outside [0, 1],
 * step_size, bc2_sqrt or eps not > 0, `launches` not one of its three values.  A range of zero rows is accepted and launches nothing.
 */
#ifndef RP_CRITIC_H_
#define RP_CRITIC_H_

#include <stddef.h>
#include <stdint.h>

#include "rp_droq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RP_CRITIC_COUNTER 48 /* the last Philox counter word of critic i, layer L is RP_CRITIC_COUNTER + 2 i + L */
#define RP_CRITIC_PARAMS 10
enum { RP_CRITIC_W1, RP_CRITIC_B1, RP_CRITIC_W2, RP_CRITIC_B2, RP_CRITIC_W3, RP_CRITIC_B3, RP_CRITIC_G1, RP_CRITIC_BE1,
       RP_CRITIC_G2, RP_CRITIC_BE2 };

enum { RP_CRITIC_STEP = 0, RP_CRITIC_ROWS_ONLY = 1, RP_CRITIC_APPLY_ONLY = 2 };

typedef struct rp_critic_set { /* HOST: the ten tensors of one critic (or of its m, v, target or gradient) */
  float* t[RP_CRITIC_PARAMS];
} rp_critic_set;

typedef struct rp_critic_step_args {
  size_t struct_size;
  const float* obs;            /* [B][D] */
  const float* action;         /* [B][A] */
  const float* y;              /* [B]: the TD target */
  const float* mask;           /* [B] */
  const float* mean;           /* [D] */
  const float* inv_std;        /* [D] */
  float obs_clip;              /* > 0 */
  const rp_critic_set* p;      /* HOST [n_critics]: the live critics, updated in place */
  const rp_critic_set* m;      /* HOST [n_critics]: Adam's first moments, updated in place */
  const rp_critic_set* v;      /* HOST [n_critics]: Adam's second moments, updated in place */
  const rp_critic_set* target; /* HOST [n_critics]: the target critics, updated in place */
  const rp_critic_set* grad;   /* HOST [n_critics], optional, and each of its pointers optional: the gradients */
  int n_critics;               /* 1 .. RP_DROQ_MAX_CRITICS */
  float* q;                    /* [n_critics][B]: the critics' values before the step */
  void* workspace;             /* at least rp_critic_workspace's answer; 16-byte aligned */
  size_t workspace_bytes;
  uint32_t drop_threshold;     /* a unit is kept iff its Philox word >= drop_threshold */
  float keep_scale;            /* > 0: 1 / (1 - p) */
  float ln_eps;                /* > 0 */
  uint32_t seed_lo, seed_hi, round;
  float one_minus_beta1, beta2, one_minus_beta2;
  float step_size;             /* > 0: lr / (1 - beta1^t) */
  float bc2_sqrt;              /* > 0: sqrt(1 - beta2^t) */
  float eps;                   /* > 0 */
  float tau;                   /* in [0, 1] */
  int D, H1, H2, A;
  int B, row_first, row_count;
  int launches;                /* RP_CRITIC_STEP: both launches, a step; the other two values run one launch alone, for
                                  measurement (the apply launch then reads whatever the workspace holds) */
  void* hip_stream;
} rp_critic_step_args;

int rp_critic_step(const rp_critic_step_args* args);

/* The size query: sets `bytes` to what rp_critic_step needs for these sizes (a pure function of them). */
typedef struct rp_critic_workspace_args {
  size_t struct_size;
  int n_critics, H1, H2, row_count;
  size_t bytes; /* out */
} rp_critic_workspace_args;

int rp_critic_workspace(rp_critic_workspace_args* args);

/* "max_critics", "tile_rows" (the rows of one workgroup of the rows launch), "stage_rows" (the rows one stage of the
 * apply launch's reduction holds), "launches" (2), "counter", "max_hidden", "max_actions"; -1 otherwise */
int rp_critic_dim(const char* name);

const char* rp_critic_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_CRITIC_H_ */
