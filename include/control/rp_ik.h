/* control/rp_ik.h — batched fingertip inverse kinematics on the engine's state (C ABI, gfx950, librp_ik.so).
 *
 * One call turns fingertip targets of `env_count` environments into actuator-space position targets (the task's
 * action, without the sustain entry) by damped-least-squares steps on the hands' kinematic trees, straight from the
 * engine's qpos array (rp_field_ptr(RP_QPOS)).
 *
 * Definition.  A scene has H hands (1 or 2; right before left).  A hand has n <= 32 dofs (hinge or slide, the forearm's
 * included), a <= 32 position actuators of gear 1 (each on a joint or on a fixed tendon sum_j coef_j q_j) and 5 fingertip
 * sites (th..lf).  Tips are numbered in fingering order, right 0-4, left 5-9 (0-4 in a one-hand scene); T = 5H.
 * For every env and hand, q^0 = the hand's dofs of qpos; for it = 0 .. K-1:
 *     p_i      world position of tip i at q^it (the hand root carries the env's tree_offset)
 *     d_i      = p*_i - p_i, p* fixed over the iterations; delta mode: p*_i = p_i(q^0) + target_i
 *     e_i      = w_i d_i min(1, s / |d_i|), 0 where d_i = 0 or w_i = 0
 *     J        15 x n, rows 3i..3i+2 = w_i dp_i/dq: axis_w x (p_i - anchor_w) for a hinge above the tip in the tree,
 *              axis_w for a slide above it, 0 for any other dof
 *     A        = J D J^T + lambda^2 I,  D = diag(dof_weight)     (eigenvalues >= lambda^2: Cholesky, no pivoting)
 *     dq       = D J^T A^-1 e
 *     q^{it+1} = clamp(q^it + dq, jnt_range)                      (limited joints only)
 * Outputs: out_k = clamp(sum_j coef_kj q^K_j, ctrlrange_k) in the task's action order (the right hand's actuators,
 * then the left's); optionally q_target = q^K, residual_i = |p*_i - p_i(q^K)| and tips_i = p_i(q^0).
 * All IK arithmetic is float64, whatever the engine's precision; of the engine's state only qpos and tree_offset
 * are read.
 *
 * Array pointers of rp_ik_args are DEVICE pointers into caller-owned memory, except `dof_weight` (HOST).  rp_ik_solve
 * only enqueues one kernel on `hip_stream` (hipStream_t; NULL = default stream): no host synchronisation, no
 * allocation after create.  Returns 0, or a negative code with the message in rp_ik_last_error(); a refused call
 * launches nothing.  Refused: lambda <= 0, max_step <= 0, iterations < 1 (or > 1024), a negative or non-finite
 * dof_weight, an env range outside the batch, out_stride < n_act.  The tip weights live on the device and cannot be
 * inspected without a read-back: they must be >= 0 (the Python binding refuses negative host-side weights).
 */
#ifndef RP_IK_H_
#define RP_IK_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rp_ik rp_ik;

typedef struct rp_ik_args {
  size_t struct_size;        /* sizeof(rp_ik_args) of the caller: a mismatch is refused */
  const void* qpos;          /* [E][nv] of the solver's precision */
  const void* tree_offset;   /* [E][ntree][3] of the solver's precision (RP_TREE_OFFSET), or NULL */
  const double* target;      /* [E][T][3]: world targets, or displacements of the current tips in delta mode */
  const double* weight;      /* [E][T] tip weights >= 0, or NULL = 1 */
  const double* dof_weight;  /* HOST [n_dof] >= 0 in q_target's order, or NULL = 1 */
  int delta;                 /* 0 = absolute targets, 1 = delta mode */
  int iterations;            /* K >= 1 */
  double lambda;             /* damping > 0 */
  double max_step;           /* s > 0: clip of every tip's error, metres */
  void* out;                 /* [E] rows of `out_stride` elements of the solver's precision; columns >= n_act stay */
  long long out_stride;      /* >= n_act */
  double* q_target;          /* [E][n_dof] or NULL: q^K, the right hand's dofs (HandInfo.joint_ids order), then the left's */
  double* residual;          /* [E][T] or NULL */
  double* tips;              /* [E][T][3] or NULL: p(q^0) */
  int env_first, env_count;  /* envs [env_first, env_first + env_count) are solved; every array is indexed by the
                                ABSOLUTE env: the other envs' rows stay */
  void* hip_stream;
} rp_ik_args;

/* `blob` = robopianist_amd.model.ik_tables.make_ik_blob; precision 32 / 64 = element type of qpos, tree_offset and
 * out.  Uploads the tables; allocates nothing per env. */
int rp_ik_create(const void* blob, size_t bytes, int n_envs, int device, int precision, rp_ik** out);
void rp_ik_destroy(rp_ik* h);

int rp_ik_solve(rp_ik* h, const rp_ik_args* args);

/* "n_hands", "n_tips", "n_act", "n_dof", "nv", "ntree", "n_envs" */
int rp_ik_dim(const rp_ik* h, const char* name);

const char* rp_ik_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_IK_H_ */
