/* plan/rp_plan.h — the batched kernels of a predictive-sampling planner (C ABI, gfx950, librp_plan.so).
 *
 * Predictive sampling (MJPC): fork the state of every real env into K candidates, roll each candidate out H control
 * steps under a perturbed action spline, keep the best.  The rollouts are the engine's; this library is the six
 * launches around them.  It has no handle and allocates nothing: every array is the caller's.
 *
 * Layout.  G real envs ("groups"), K candidates each.  The planning batch has E = G K rows; row e belongs to group
 * e / K and is candidate e % K.  Candidate 0 always carries the unperturbed nominal plan.  A plan is P knots of nu
 * action entries over a horizon of H control steps: knots [E][P][nu], nominal [G][P][nu], both float64.
 *
 * Splines (RP_PLAN_ZERO, RP_PLAN_LINEAR), value of entry u at control step h of a plan with knots k_0 .. k_{P-1}:
 *     P == 1        k_0
 *     zero-order    k_i, i = min(h P / H, P - 1)                                     (integer division)
 *     linear        requires (H - 1) % (P - 1) == 0;  Sd = (H - 1) / (P - 1), i = min(h / Sd, P - 2),
 *                   w = (double)(h - i Sd) / (double)Sd,  d = k_{i+1} - k_i,  m = d w,  a = k_i + m
 * Knot p sits at control step s_p = p Sd (linear), ceil(p H / P) (zero-order), 0 (P == 1).
 * Every float operation of this library is rounded on its own (no fused multiply-add): a restatement that rounds each
 * product and each sum separately in float64 reproduces every output bit for bit.
 *
 * Noise.  z(seed, round, e, c) is defined in integers: Philox4x32-10 with key (seed_lo, seed_hi) and counter
 * (round, e, c, j) for j = 0, 1, 2 gives 12 words of 32 bits; S = their sum as an unsigned 64-bit integer;
 *     z = (double)((int64)S - 6 * 2^32) * 2^-32
 * (Irwin-Hall of 12 uniforms: mean 0 up to 6 * 2^-32, unit variance, support [-6, 6)).  c = p nu + u.
 *
 * Array pointers are DEVICE pointers into caller-owned memory, except rp_plan_fork_args.fields (HOST).  Every entry
 * point enqueues exactly one kernel on `hip_stream` (hipStream_t; NULL = default stream): no host synchronisation, no
 * allocation.  Returns 0, or a negative code with the message in rp_plan_last_error(); a refused call launches nothing.
 * Refused: a struct_size mismatch, null pointers, G < 1, K < 1, P < 1, nu < 1, H < 1, h outside [0, H), linear with
 * (H - 1) % (P - 1) != 0, a row range outside the batch, more than RP_PLAN_MAX_FIELDS fields, a field of
 * row_bytes < 1, precision other than 32 / 64.  A range of zero rows is accepted and launches nothing.
 */
#ifndef RP_PLAN_H_
#define RP_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_PLAN_MAX_FIELDS 64
#define RP_PLAN_ZERO 0
#define RP_PLAN_LINEAR 1
#define RP_PLAN_STEP_LAST 2 /* dm_env StepType.LAST, as rp_task writes it */

typedef struct rp_plan_field {
  const void* src;     /* [G] rows of row_bytes bytes: a per-env array of the real environment */
  void* dst;           /* [E] rows of row_bytes bytes: the same array of the planning environment (another allocation) */
  long long row_bytes; /* >= 1 */
} rp_plan_field;

/* dst row e <- src row e / K for the rows e of [env_first, env_first + env_count), every field.  16-byte copies where
 * both rows are 16-aligned, else the widest of 8 / 4 / 2 / 1 bytes both rows are aligned to, plus a byte tail. */
typedef struct rp_plan_fork_args {
  size_t struct_size;
  const rp_plan_field* fields; /* HOST [n_fields], copied into the launch */
  int n_fields;                /* 1 .. RP_PLAN_MAX_FIELDS */
  int G, K;
  int env_first, env_count; /* rows of the planning batch */
  void* hip_stream;
} rp_plan_fork_args;

/* knots[e][p][u] = clamp(nominal[e / K][p][u] + sigma[u] z(seed, round, e, p nu + u), lo[u], hi[u]) for e % K > 0,
 * clamp(nominal[e / K][p][u], lo[u], hi[u]) for e % K == 0.  t = sigma z and nominal + t are rounded separately;
 * clamp(x, lo, hi) = fmin(fmax(x, lo), hi). */
typedef struct rp_plan_sample_args {
  size_t struct_size;
  const double* nominal; /* [G][P][nu] */
  const double* sigma;   /* [nu] */
  const double* lo;      /* [nu] */
  const double* hi;      /* [nu] */
  double* knots;         /* [E][P][nu] */
  uint32_t seed_lo, seed_hi, round;
  int G, K, P, nu;
  int env_first, env_count;
  void* hip_stream;
} rp_plan_sample_args;

/* out[r][u] = the spline of knots[r] at control step h, computed in float64 and rounded once to `precision`, for the
 * rows r of [row_first, row_first + row_count) of a batch of n_rows plans (the E candidates, or the G nominals). */
typedef struct rp_plan_action_args {
  size_t struct_size;
  const double* knots; /* [n_rows][P][nu] */
  void* out;           /* [n_rows][nu] of `precision` */
  int precision;       /* 32 / 64 */
  int spline;          /* RP_PLAN_ZERO / RP_PLAN_LINEAR */
  int h, H, P, nu;
  int n_rows, row_first, row_count;
  void* hip_stream;
} rp_plan_action_args;

/* For the rows that are still alive (alive[e] != 0): t = weight * (double)reward[e]; ret[e] = ret[e] + t; then
 * alive[e] = 0 if step_type[e] == RP_PLAN_STEP_LAST.  A dead row is left alone: the step that ends an episode still
 * counts, nothing after it does.  A NaN reward makes the row's return NaN.  The caller zeroes ret and sets alive to 1
 * before the first step of a rollout; weight = gamma^h is the host's. */
typedef struct rp_plan_accumulate_args {
  size_t struct_size;
  double* ret;              /* [E] */
  unsigned char* alive;     /* [E] */
  const void* reward;       /* [E] of `precision` */
  const int32_t* step_type; /* [E] */
  int precision;
  double weight;
  int E, env_first, env_count;
  void* hip_stream;
} rp_plan_accumulate_args;

/* One wave per group g of [group_first, group_first + group_count): best = the argmax of ret[g K .. g K + K) where NaN
 * never wins, ties go to the lowest candidate and all-NaN gives 0 (-inf is a value like any other).  Writes
 * best_k[g] = best, best_return[g] = ret[g K + best] and nominal[g] <- knots[g K + best]. */
typedef struct rp_plan_select_args {
  size_t struct_size;
  const double* ret;   /* [E] */
  const double* knots; /* [E][P][nu] */
  double* nominal;     /* [G][P][nu] */
  int32_t* best_k;     /* [G] */
  double* best_return; /* [G] */
  int G, K, P, nu;
  int group_first, group_count;
  void* hip_stream;
} rp_plan_select_args;

/* Advances the nominal by one control step, in place: knot p of every group becomes the OLD spline's value at control
 * step min(s_p + 1, H - 1) (s_p above).  P == 1 changes nothing. */
typedef struct rp_plan_shift_args {
  size_t struct_size;
  double* nominal; /* [G][P][nu] */
  int spline;
  int H, P, nu;
  int G, group_first, group_count;
  void* hip_stream;
} rp_plan_shift_args;

int rp_plan_fork(const rp_plan_fork_args* args);
int rp_plan_sample(const rp_plan_sample_args* args);
int rp_plan_action(const rp_plan_action_args* args);
int rp_plan_accumulate(const rp_plan_accumulate_args* args);
int rp_plan_select(const rp_plan_select_args* args);
int rp_plan_shift(const rp_plan_shift_args* args);

/* "max_fields" (RP_PLAN_MAX_FIELDS), "wave_size" (the lanes of the select kernel's reduction: 64); -1 otherwise */
int rp_plan_dim(const char* name);

const char* rp_plan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_PLAN_H_ */
