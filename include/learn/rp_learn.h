/* learn/rp_learn.h — the batched kernels of an on-device PPO learner (C ABI, gfx950, librp_learn.so).
 *
 * Proximal policy optimisation over thousands of envs: a rollout of T control steps of E envs is collected with the
 * policy evaluated on the device, advantages are estimated (GAE), the observation normaliser learns, and the gradient
 * step is the caller's (autograd).  This library is the four launches around the environment's step: `pack` (a
 * TimeStep into the rollout storage), `act` (the fused actor / critic evaluation and the draw), `gae` and `moments`.
 * It has no handle and allocates nothing: every array is the caller's.
 *
 * Rollout storage, T + 1 slots of E rows.  Slot t holds TimeStep t verbatim -- obs [T+1][E][D] f32, reward [T+1][E]
 * f32, discount [T+1][E] f32, step_type [T+1][E] i32 -- and what was decided at it: action [T][E][A] f32, logp [T][E]
 * f32, value [T+1][E] f32.  The entry points take pointers to ONE slot (pack, act) or to the whole storage (gae,
 * moments), so the slot's address arithmetic is the caller's.
 *
 * Networks.  The actor and the critic are multilayer perceptrons with two tanh hidden layers, D -> H1 -> H2 -> A (actor)
 * or 1 (critic), weights in torch.nn.Linear's layout [out][in], float32, contiguous, read in place.
 *
 * Noise.  z(seed, round, e, u) is the planner's (plan/rp_plan.h): Philox4x32-10, the sum of 12 words.
 *
 * Every float operation of pack, gae, moments and of act's normaliser and epilogue is rounded on its own (no fused
 * multiply-add).  act's three matrix products are float32 fused-multiply-add chains over k ascending, starting from 0,
 * the bias added afterwards.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except rp_learn_pack_args.fields (HOST).  Every entry
 * point enqueues exactly one kernel on `hip_stream` (hipStream_t; NULL = default stream): no host synchronisation, no
 * allocation.  Returns 0, or a negative code with the message in rp_learn_last_error(); a refused call launches
 * nothing.  Refused: a struct_size mismatch, null pointers that are not marked optional below, E < 1, D < 1, T < 1,
 * A outside [1, RP_LEARN_MAX_A], H1 or H2 not a multiple of 16 in [16, RP_LEARN_MAX_H], a row range outside the batch,
 * n_fields outside [1, RP_LEARN_MAX_FIELDS], a field of width < 1 or of a dtype other than RP_LEARN_F32 / RP_LEARN_F64,
 * field widths that do not sum to D, precision other than 32 / 64, act without a network, an actor without its outputs,
 * n_rows < 1 or count < 0 or eps <= 0 (moments), statistics arrays given only in part (pack).  A range of zero rows is
 * accepted and launches nothing.
 */
#ifndef RP_LEARN_H_
#define RP_LEARN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_LEARN_MAX_FIELDS 64
#define RP_LEARN_MAX_H 256
#define RP_LEARN_MAX_A 128
#define RP_LEARN_F32 0
#define RP_LEARN_F64 1
#define RP_LEARN_STEP_FIRST 0 /* dm_env StepType, as rp_task writes it */
#define RP_LEARN_STEP_MID 1
#define RP_LEARN_STEP_LAST 2

typedef struct rp_learn_field {
  const void* src; /* [E] rows of `width` elements, aligned to the element size */
  int width;       /* >= 1 */
  int dtype;       /* RP_LEARN_F32 / RP_LEARN_F64 */
} rp_learn_field;

/* One TimeStep into one slot, for the rows e of [env_first, env_first + env_count): field f (the observation dict's
 * tensors in sorted key order) lands at off_f = the sum of the widths before it, obs[e][off_f + j] = (float)src_f[e][j];
 * step_type is copied; reward and discount are cast to float32 (a NULL reward writes 0, a NULL discount 1: reset()
 * returns None for both).  Copies go in the widest unit both rows allow: where the two addresses agree modulo 16 (8)
 * bytes, single float32 up to the first boundary, then units of 16 (8) bytes, then single ones; float64 in pairs (16
 * bytes in, 8 out), after one single element where that aligns both rows.
 * Episode statistics per env, without atomics (all five arrays, or none):
 *     FIRST        ep_return[e] = 0, ep_len[e] = 0
 *     otherwise    ep_return[e] += (double)reward (of the source's precision), ep_len[e] += 1
 *     LAST, then   done_return[e] += ep_return[e], done_len[e] += ep_len[e], done_count[e] += 1 */
typedef struct rp_learn_pack_args {
  size_t struct_size;
  const rp_learn_field* fields; /* HOST [n_fields], copied into the launch */
  int n_fields;                 /* 1 .. RP_LEARN_MAX_FIELDS */
  int precision;                /* of reward and discount: 32 / 64 */
  const int32_t* step_type;     /* [E] */
  const void* reward;           /* [E] of `precision`, or NULL */
  const void* discount;         /* [E] of `precision`, or NULL */
  float* obs;                   /* the slot: [E][D] */
  float* slot_reward;           /* [E] */
  float* slot_discount;         /* [E] */
  int32_t* slot_step_type;      /* [E] */
  double* ep_return;            /* [E], optional (with the four below) */
  int32_t* ep_len;              /* [E] */
  double* done_return;          /* [E] */
  long long* done_len;          /* [E] */
  int32_t* done_count;          /* [E] */
  int E, D;
  int env_first, env_count;
  void* hip_stream;
} rp_learn_pack_args;

typedef struct rp_learn_mlp {
  const float* w1; /* [H1][D] */
  const float* b1; /* [H1] */
  const float* w2; /* [H2][H1] */
  const float* b2; /* [H2] */
  const float* w3; /* [A][H2] (actor), [1][H2] (critic) */
  const float* b3; /* [A], [1] */
} rp_learn_mlp;

/* The actor and the critic on the rows e of [row_first, row_first + row_count) of one slot:
 *     d = x - mean[j];  p = d * inv_std[j];  xn = fmin(fmax(p, -obs_clip), obs_clip)
 *     h1 = tanhf(W1 xn + b1);  h2 = tanhf(W2 h1 + b2);  out = W3 h2 + b3          (mu, or the value)
 *     zf = (float)z(seed, round, e, u);  sd = expf(log_std[u]);  t = sd * zf;  a = mu + t
 *     q = zf * zf;  h = -0.5f * q;  g = h - log_std[u];  logp = (sum of g over u ascending, from 0) - (float)(0.5 A ln 2 pi)
 *     env_action = (precision)fmin(fmax(a, -1), 1)
 * Writes action, logp, env_action (and mu where given) from the actor and value from the critic.  deterministic != 0:
 * a = mu, logp is not written.  actor == NULL: the value alone (the bootstrap evaluation at slot T); critic == NULL:
 * the actor's outputs alone. */
typedef struct rp_learn_act_args {
  size_t struct_size;
  const float* obs;           /* [n_rows][D] */
  const float* mean;          /* [D] */
  const float* inv_std;       /* [D] */
  float obs_clip;             /* > 0 */
  const rp_learn_mlp* actor;  /* HOST, copied into the launch; or NULL */
  const rp_learn_mlp* critic; /* HOST, copied into the launch; or NULL */
  const float* log_std;       /* [A] (actor) */
  float* action;              /* [n_rows][A] (actor) */
  float* logp;                /* [n_rows] (actor, deterministic == 0) */
  float* mu;                  /* [n_rows][A], optional */
  void* env_action;           /* [n_rows][A] of `precision` (actor) */
  float* value;               /* [n_rows] (critic) */
  int precision;              /* of env_action: 32 / 64 */
  int deterministic;
  uint32_t seed_lo, seed_hi, round;
  int D, H1, H2, A;
  int n_rows, row_first, row_count;
  void* hip_stream;
} rp_learn_act_args;

/* Generalised advantage estimation, one thread per env e of [env_first, env_first + env_count), float64, every
 * operation rounded on its own.  carry = 0; for t = T - 1 down to 0:
 *     step_type[t][e] == LAST or step_type[t+1][e] == FIRST: slot t made no transition (the env discards the action at
 *         a LAST; a forced reset yields a FIRST with no LAST before it):  A = 0, valid = 0
 *     otherwise, r = reward[t+1][e], d = discount[t+1][e]:
 *         nv = gamma d;  tv = nv V[t+1];  s = r + tv;  delta = s - V[t];  gl = nv lambda;  c = gl carry;  A = delta + c;
 *         valid = 1
 *     adv[t][e] = (float)A;  ret[t][e] = (float)(A + V[t]);  carry = A (unrounded) */
typedef struct rp_learn_gae_args {
  size_t struct_size;
  const float* reward;      /* [T+1][E] */
  const float* discount;    /* [T+1][E] */
  const int32_t* step_type; /* [T+1][E] */
  const float* value;       /* [T+1][E] */
  float* adv;               /* [T][E] */
  float* ret;               /* [T][E] */
  unsigned char* valid;     /* [T][E] */
  double gamma, lambda;
  int T, E;
  int env_first, env_count;
  void* hip_stream;
} rp_learn_gae_args;

/* The per-column moments of obs[0 .. n_rows) in float64, merged into the caller's running (count, mean[D], M2[D]) and
 * published for act.  `count` is the number of rows merged so far; it is the host's (it grows by n_rows per call).
 * Column j, with L = RP_LEARN_MOMENT_LANES ("moment_lanes") partial sums: lane l sums the rows l, l + L, ... in
 * ascending order, the lanes are summed in ascending order:
 *     S = sum x;  mb = S / n_rows;  Mb = sum (x - mb)^2        (each difference, square and sum rounded on its own)
 *     n = count + n_rows;  dl = mb - mean[j];  w = n_rows / n;  mean[j] += dl w
 *     M2[j] = (M2[j] + Mb) + ((dl dl) count) w
 *     mean_f32[j] = (float)mean[j];  inv_std_f32[j] = (float)(1 / sqrt(M2[j] / n + eps))
 * The order is fixed and there are no atomics: two runs give the same bits. */
typedef struct rp_learn_moments_args {
  size_t struct_size;
  const float* obs; /* [n_rows][D] */
  double* mean;     /* [D] */
  double* M2;       /* [D] */
  float* mean_f32;  /* [D] */
  float* inv_std_f32; /* [D] */
  double count;     /* >= 0 */
  double eps;       /* > 0 */
  long long n_rows; /* >= 1 */
  int D;
  void* hip_stream;
} rp_learn_moments_args;

int rp_learn_pack(const rp_learn_pack_args* args);
int rp_learn_act(const rp_learn_act_args* args);
int rp_learn_gae(const rp_learn_gae_args* args);
int rp_learn_moments(const rp_learn_moments_args* args);

/* "max_fields", "max_hidden" (RP_LEARN_MAX_H), "hidden_multiple" (16), "min_hidden" (16), "max_actions"
 * (RP_LEARN_MAX_A), "min_obs" (1), "tile_rows" (the rows of one workgroup of act), "moment_lanes"; -1 otherwise */
int rp_learn_dim(const char* name);

const char* rp_learn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_LEARN_H_ */
