// rp_ik.hpp -- the fingertip inverse kinematics' tables and per-env solve (include/control/rp_ik.h).
//
// Plain C++ behind RPIK_HD, free of wave intrinsics: rp_ik.hip compiles it for gfx950, and the CPU tests compile the same
// source with a host compiler.  The solve is written as PHASES: within a phase every (hand, lane) pair works on its own
// item (a body, a dof column, a matrix row, an actuator) and touches no item another lane writes in that phase; phases
// are separated by ctx.sync().  On the device a workgroup is one wave, lanes 0-31 = hand 0, 32-63 = hand 1, each lane
// runs its own pair and sync() is the workgroup barrier; on the host one thread runs every pair of a phase in turn
// and sync() does nothing.  Everything that lives across a phase boundary is in RpikWork (LDS on the device).
#ifndef RP_IK_HPP_
#define RP_IK_HPP_

#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/control/rp_ik.h"

#if defined(__HIPCC__)
#define RPIK_HD __host__ __device__
#else
#define RPIK_HD
#endif

enum { RPIK_JNT_SLIDE = 2, RPIK_JNT_HINGE = 3 };
#define RPIK_MAX_HANDS 2
#define RPIK_LANES 32        // dofs, bodies and actuators of one hand: one lane each
#define RPIK_TIPS 5
#define RPIK_ROWS 15         // 3 rows per tip
#define RPIK_LD 17           // leading dimension of the 15-wide arrays (odd: a lane per row reads without LDS bank conflicts)
#define RPIK_MAX_TERMS 4     // joints of one fixed tendon
#define RPIK_MAX_ITERATIONS 1024

// The tables, exactly as model/ik_tables.py lays them out (every array padded to the fixed sizes).
struct RpikModel {
  int nhand, nv, ntree, maxlevel, ndof, nact, pad_[2];
  int hand[RPIK_MAX_HANDS][8];                       // n, nbody, nact, nlevel, tree, qoff, aoff, -
  int body_i[RPIK_MAX_HANDS][RPIK_LANES][4];         // parent (-1 = the hand root), level, first joint, joint count
  int jnt_i[RPIK_MAX_HANDS][RPIK_LANES][2];          // walk order: type, column
  int col_i[RPIK_MAX_HANDS][RPIK_LANES];             // qpos address of the column
  uint32_t tip_i[RPIK_MAX_HANDS][RPIK_TIPS][2];      // body, mask of the columns above the tip
  int act_i[RPIK_MAX_HANDS][RPIK_LANES][1 + RPIK_MAX_TERMS];   // term count, columns
  double body_d[RPIK_MAX_HANDS][RPIK_LANES][7];      // local position, local quaternion
  double jnt_d[RPIK_MAX_HANDS][RPIK_LANES][6];       // walk order: axis, anchor (body frame)
  double col_d[RPIK_MAX_HANDS][RPIK_LANES][2];       // range (-inf, +inf: not limited)
  double tip_d[RPIK_MAX_HANDS][RPIK_TIPS][3];        // site position (body frame)
  double act_d[RPIK_MAX_HANDS][RPIK_LANES][RPIK_MAX_TERMS + 2];   // coefficients, ctrlrange
};

// One call, as the per-env solve sees it (pointers of the side that runs it).
struct RpikCall {
  const void *qpos, *tree_offset;
  const double *target, *weight;
  void* out;
  long long out_stride;
  double *q_target, *residual, *tips;
  double lambda2, max_step;
  int delta, iterations;
  double dof_weight[RPIK_MAX_HANDS][RPIK_LANES];
};

// Per-hand state that crosses phase boundaries.
struct RpikWork {
  double q[RPIK_LANES];
  double bpos[RPIK_LANES][3], bquat[RPIK_LANES][4];        // world frames of the bodies
  double axis[RPIK_LANES][3], anchor[RPIK_LANES][3];       // per column, world frame
  double tip[RPIK_TIPS][3], goal[RPIK_TIPS][3], w[RPIK_TIPS];
  double J[RPIK_LANES][RPIK_LD];                           // [column][row]
  double A[RPIK_ROWS][RPIK_LD];                            // lower triangle: A, then its Cholesky factor
  double r[RPIK_LD], piv[RPIK_LD];
  int jtype[RPIK_LANES];                                   // per column
};

// ---------------------------------------------------------------------------------------------------------------
// host side: blob -> tables
// ---------------------------------------------------------------------------------------------------------------
struct RpikBlobEntry { char name[40]; int32_t dtype, ndim; int64_t count, offset; };

// Fills M from an IK blob; returns "" or an error message.  Every index the solve follows is checked here, once.
inline std::string rpik_parse(const void* blob, size_t nb, RpikModel& M) {
  const unsigned char* p = (const unsigned char*)blob;
  if (!p || nb < 12) return "ik blob: too short";
  uint32_t h[3]; memcpy(h, p, 12);
  if (h[0] != 0x52504D42u) return "ik blob: bad magic";
  const int n = (int)h[2];
  if (n < 0 || 12 + (size_t)n * sizeof(RpikBlobEntry) > nb) return "ik blob: truncated table";
  std::string err;
  auto get = [&](const char* name, int dtype, size_t count, void* dst) {
    for (int i = 0; i < n; i++) {
      RpikBlobEntry e;
      memcpy(&e, p + 12 + (size_t)i * sizeof(e), sizeof(e));
      if (strncmp(e.name, name, 40)) continue;
      const size_t es = e.dtype == 0 ? 8 : 4;
      if (e.dtype != dtype || e.count < 0 || (size_t)e.count != count) { err = std::string("ik blob: bad shape: ") + name; return false; }
      if (e.offset < 0 || (size_t)e.offset > nb || count * es > nb - (size_t)e.offset) { err = std::string("ik blob: entry out of range: ") + name; return false; }
      memcpy(dst, p + e.offset, count * es);
      return true;
    }
    err = std::string("ik blob: entry missing: ") + name + " (not an IK blob? build it with model/ik_tables.py)";
    return false;
  };
  memset(&M, 0, sizeof(M));
  int dims[8];
  const size_t HL = RPIK_MAX_HANDS * RPIK_LANES, HT = RPIK_MAX_HANDS * RPIK_TIPS;
  if (!get("ik_dims", 1, 8, dims) || !get("ik_hand_i", 1, RPIK_MAX_HANDS * 8, M.hand) || !get("ik_body_i", 1, HL * 4, M.body_i) ||
      !get("ik_jnt_i", 1, HL * 2, M.jnt_i) || !get("ik_col_i", 1, HL, M.col_i) || !get("ik_tip_i", 1, HT * 2, M.tip_i) ||
      !get("ik_act_i", 1, HL * (1 + RPIK_MAX_TERMS), M.act_i) || !get("ik_body_d", 0, HL * 7, M.body_d) ||
      !get("ik_jnt_d", 0, HL * 6, M.jnt_d) || !get("ik_col_d", 0, HL * 2, M.col_d) || !get("ik_tip_d", 0, HT * 3, M.tip_d) ||
      !get("ik_act_d", 0, HL * (RPIK_MAX_TERMS + 2), M.act_d))
    return err;
  M.nhand = dims[0]; M.nv = dims[1]; M.ntree = dims[2];
  if (M.nhand < 1 || M.nhand > RPIK_MAX_HANDS) return "ik blob: " + std::to_string(M.nhand) + " hands (1 or 2)";
  if (M.nv < 1 || M.ntree < 0) return "ik blob: bad counts";
  int qoff = 0, aoff = 0, maxlevel = 0;
  for (int hd = 0; hd < M.nhand; hd++) {
    int* H = M.hand[hd];
    const int nd = H[0], nbody = H[1], na = H[2], nlevel = H[3], tree = H[4];
    if (nd < 1 || nd > RPIK_LANES) return "ik blob: a hand has " + std::to_string(nd) + " dofs (1 to " + std::to_string(RPIK_LANES) + ")";
    if (nbody < 1 || nbody > RPIK_LANES || na < 0 || na > RPIK_LANES) return "ik blob: bad body / actuator count";
    if (tree < -1 || tree >= M.ntree) return "ik blob: bad tree index";
    if (H[5] != qoff || H[6] != aoff) return "ik blob: bad offsets";
    int njoint = 0, lvl_max = 0;
    uint32_t seen = 0;
    for (int b = 0; b < nbody; b++) {
      const int par = M.body_i[hd][b][0], lvl = M.body_i[hd][b][1], ja = M.body_i[hd][b][2], jn = M.body_i[hd][b][3];
      if (b == 0 ? (par != -1 || lvl != 0) : (par < 0 || par >= b || lvl != M.body_i[hd][par][1] + 1)) return "ik blob: bad body tree";
      if (jn < 0 || ja != njoint || ja + jn > nd) return "ik blob: bad body joints";
      njoint += jn;
      if (lvl > lvl_max) lvl_max = lvl;
      for (int k = 0; k < 7; k++) if (!std::isfinite(M.body_d[hd][b][k])) return "ik blob: body pose is not finite";
    }
    if (njoint != nd || nlevel != lvl_max + 1) return "ik blob: joints / levels do not match the tree";
    for (int j = 0; j < nd; j++) {
      const int ty = M.jnt_i[hd][j][0], col = M.jnt_i[hd][j][1];
      if (ty != RPIK_JNT_SLIDE && ty != RPIK_JNT_HINGE) return "ik blob: joint type (hinge and slide only)";
      if (col < 0 || col >= nd || (seen >> col & 1u)) return "ik blob: the joints' columns are not a permutation";
      seen |= 1u << col;
      if (M.col_i[hd][j] < 0 || M.col_i[hd][j] >= M.nv) return "ik blob: bad qpos address";
      if (!(M.col_d[hd][j][0] <= M.col_d[hd][j][1])) return "ik blob: bad joint range";
      for (int k = 0; k < 6; k++) if (!std::isfinite(M.jnt_d[hd][j][k])) return "ik blob: joint axis / anchor is not finite";
    }
    for (int i = 0; i < RPIK_TIPS; i++) {
      if (M.tip_i[hd][i][0] >= (uint32_t)nbody) return "ik blob: bad tip body";
      if (nd < 32 && (M.tip_i[hd][i][1] >> nd) != 0) return "ik blob: bad tip column mask";
    }
    for (int k = 0; k < na; k++) {
      const int nt = M.act_i[hd][k][0];
      if (nt < 1 || nt > RPIK_MAX_TERMS) return "ik blob: bad transmission";
      for (int i = 0; i < nt; i++) if (M.act_i[hd][k][1 + i] < 0 || M.act_i[hd][k][1 + i] >= nd) return "ik blob: bad transmission column";
      if (!(M.act_d[hd][k][RPIK_MAX_TERMS] <= M.act_d[hd][k][RPIK_MAX_TERMS + 1])) return "ik blob: bad ctrlrange";
    }
    qoff += nd; aoff += na;
    if (nlevel > maxlevel) maxlevel = nlevel;
  }
  M.ndof = qoff; M.nact = aoff; M.maxlevel = maxlevel;
  return "";
}

// Host-side refusals, shared by rp_ik_solve and the CPU build.  Returns "" or the message.
inline std::string rpik_check_args(const rp_ik_args* a, int n_envs, const RpikModel& M) {
  if (!a) return "rp_ik_solve: args is NULL";
  if (a->struct_size != sizeof(rp_ik_args))
    return "rp_ik_solve: args->struct_size = " + std::to_string(a->struct_size) + ", this library's rp_ik_args has " +
           std::to_string(sizeof(rp_ik_args)) + " bytes (header / library mismatch)";
  if (!a->qpos || !a->target || !a->out) return "rp_ik_solve: qpos, target and out must not be NULL";
  if (!(a->lambda > 0.0) || !std::isfinite(a->lambda)) return "rp_ik_solve: lambda must be positive";
  if (!(a->max_step > 0.0) || !std::isfinite(a->max_step)) return "rp_ik_solve: max_step must be positive";
  if (a->iterations < 1 || a->iterations > RPIK_MAX_ITERATIONS)
    return "rp_ik_solve: iterations must be in [1, " + std::to_string(RPIK_MAX_ITERATIONS) + "]";
  if (a->delta != 0 && a->delta != 1) return "rp_ik_solve: delta must be 0 or 1";
  if (a->out_stride < M.nact) return "rp_ik_solve: out_stride = " + std::to_string(a->out_stride) + " < " + std::to_string(M.nact) + " actuators";
  if (a->env_count <= 0 || a->env_first < 0 || a->env_first > n_envs - a->env_count)
    return "rp_ik_solve: envs [" + std::to_string(a->env_first) + ", " + std::to_string((long long)a->env_first + a->env_count) +
           ") are outside the batch of " + std::to_string(n_envs);
  if (a->dof_weight)
    for (int k = 0; k < M.ndof; k++)
      if (!(a->dof_weight[k] >= 0.0) || !std::isfinite(a->dof_weight[k])) return "rp_ik_solve: dof_weight must be finite and >= 0";
  return "";
}

inline RpikCall rpik_call(const rp_ik_args* a, const RpikModel& M) {
  RpikCall c;
  memset(&c, 0, sizeof(c));
  c.qpos = a->qpos; c.tree_offset = a->tree_offset; c.target = a->target; c.weight = a->weight;
  c.out = a->out; c.out_stride = a->out_stride; c.q_target = a->q_target; c.residual = a->residual; c.tips = a->tips;
  c.lambda2 = a->lambda * a->lambda; c.max_step = a->max_step; c.delta = a->delta; c.iterations = a->iterations;
  for (int h = 0; h < M.nhand; h++)
    for (int l = 0; l < M.hand[h][0]; l++) c.dof_weight[h][l] = a->dof_weight ? a->dof_weight[M.hand[h][5] + l] : 1.0;
  return c;
}

// ---------------------------------------------------------------------------------------------------------------
// the per-env solve
// ---------------------------------------------------------------------------------------------------------------
RPIK_HD inline void rpik_quat_mat(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

RPIK_HD inline void rpik_quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

RPIK_HD inline void rpik_rot(const double* R, const double* v, double* o) {
  o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}

// World frame of body b of hand h from its parent's (already in W), and the world axis / anchor of its joints' columns.
// `off` = the env's offset of this hand's root, or null.
RPIK_HD inline void rpik_body(const RpikModel& M, int h, int b, const double* off, RpikWork& W) {
  const int par = M.body_i[h][b][0];
  double pp[3] = {0, 0, 0}, pq[4] = {1, 0, 0, 0};
  if (par >= 0)
    for (int k = 0; k < 4; k++) { if (k < 3) pp[k] = W.bpos[par][k]; pq[k] = W.bquat[par][k]; }
  const double* bd = M.body_d[h][b];
  double lp[3] = {bd[0], bd[1], bd[2]};
  if (par < 0 && off) { lp[0] += off[0]; lp[1] += off[1]; lp[2] += off[2]; }
  double R[9], t[3], p[3], q[4];
  rpik_quat_mat(pq, R);
  rpik_rot(R, lp, t);
  p[0] = pp[0] + t[0]; p[1] = pp[1] + t[1]; p[2] = pp[2] + t[2];
  rpik_quat_mul(pq, bd + 3, q);
  const int j0 = M.body_i[h][b][2], j1 = j0 + M.body_i[h][b][3];
  for (int j = j0; j < j1; j++) {
    const int col = M.jnt_i[h][j][1];
    const double* jd = M.jnt_d[h][j];
    const double ang = W.q[col];
    double ax[3], an[3];
    rpik_quat_mat(q, R);
    rpik_rot(R, jd, ax);
    rpik_rot(R, jd + 3, t);
    an[0] = p[0] + t[0]; an[1] = p[1] + t[1]; an[2] = p[2] + t[2];
    if (M.jnt_i[h][j][0] == RPIK_JNT_SLIDE) {
      p[0] += ax[0] * ang; p[1] += ax[1] * ang; p[2] += ax[2] * ang;
    } else {
      // hinge: rotate about the axis through the anchor, which stays where it is
      const double s = sin(0.5 * ang), c = cos(0.5 * ang);
      const double dq[4] = {c, jd[0] * s, jd[1] * s, jd[2] * s};
      double nq[4];
      rpik_quat_mul(q, dq, nq);
      q[0] = nq[0]; q[1] = nq[1]; q[2] = nq[2]; q[3] = nq[3];
      rpik_quat_mat(q, R);
      rpik_rot(R, jd + 3, t);
      p[0] = an[0] - t[0]; p[1] = an[1] - t[1]; p[2] = an[2] - t[2];
    }
    for (int k = 0; k < 3; k++) { W.axis[col][k] = ax[k]; W.anchor[col][k] = an[k]; }
    W.jtype[col] = M.jnt_i[h][j][0];
  }
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 3; k++) W.bpos[b][k] = p[k];
  for (int k = 0; k < 4; k++) W.bquat[b][k] = q[k] * inv;
}

RPIK_HD inline double rpik_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

#define RPIK_EACH(h, l) \
  for (int h = ctx.h0; h < ctx.h1; h++) if (h < M.nhand) for (int l = ctx.l0; l < ctx.l1; l++)

// Solves env `env` of the call.  T = element type of qpos, tree_offset and out.  W: RPIK_MAX_HANDS work areas.
template <typename T, typename Ctx>
RPIK_HD inline void rpik_solve_env(const RpikModel& M, const RpikCall& c, int env, RpikWork* Wh, Ctx& ctx) {
  const T* qpos = (const T*)c.qpos + (size_t)env * M.nv;
  const T* offs = c.tree_offset ? (const T*)c.tree_offset + (size_t)env * M.ntree * 3 : nullptr;
  const int ntip = RPIK_TIPS * M.nhand;
  RPIK_EACH(h, l) {
    RpikWork& W = Wh[h];
    if (l < M.hand[h][0]) W.q[l] = (double)qpos[M.col_i[h][l]];
    if (l < RPIK_TIPS) W.w[l] = c.weight ? c.weight[(size_t)env * ntip + RPIK_TIPS * h + l] : 1.0;
  }
  ctx.sync();
  // (the pass after the last update only measures the residual)
  const int passes = c.iterations + (c.residual ? 1 : 0);
  for (int it = 0; it < passes; it++) {
    // ---- tree walk, level by level: lane = body ------------------------------------------------------------
    for (int lev = 0; lev < M.maxlevel; lev++) {
      RPIK_EACH(h, l) {
        if (l < M.hand[h][1] && M.body_i[h][l][1] == lev) {
          const int tr = M.hand[h][4];
          double off[3];
          const bool has = offs && tr >= 0;
          if (has) { off[0] = (double)offs[3 * tr]; off[1] = (double)offs[3 * tr + 1]; off[2] = (double)offs[3 * tr + 2]; }
          rpik_body(M, h, l, has ? off : nullptr, Wh[h]);
        }
      }
      ctx.sync();
    }
    // ---- tips, goals, clipped errors: lane = tip ----------------------------------------------------------------
    RPIK_EACH(h, l) {
      if (l < RPIK_TIPS) {
        RpikWork& W = Wh[h];
        const int b = (int)M.tip_i[h][l][0];
        const size_t ti = (size_t)env * ntip + RPIK_TIPS * h + l;
        double R[9], t[3], p[3];
        rpik_quat_mat(W.bquat[b], R);
        rpik_rot(R, M.tip_d[h][l], t);
        for (int k = 0; k < 3; k++) { p[k] = W.bpos[b][k] + t[k]; W.tip[l][k] = p[k]; }
        if (it == 0) {
          for (int k = 0; k < 3; k++) W.goal[l][k] = c.delta ? p[k] + c.target[3 * ti + k] : c.target[3 * ti + k];
          if (c.tips) for (int k = 0; k < 3; k++) c.tips[3 * ti + k] = p[k];
        }
        const double d[3] = {W.goal[l][0] - p[0], W.goal[l][1] - p[1], W.goal[l][2] - p[2]};
        const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (it == c.iterations) {
          c.residual[ti] = nrm;
        } else {
          const double w = W.w[l];
          const double scale = nrm > c.max_step ? c.max_step / nrm : 1.0;
          // (a weightless tip contributes +0 whatever its target: no bit of the outputs depends on it)
          for (int k = 0; k < 3; k++) W.r[3 * l + k] = (w == 0.0 || nrm == 0.0) ? 0.0 : w * d[k] * scale;
        }
      }
    }
    ctx.sync();
    if (it == c.iterations) break;
    // ---- Jacobian: lane = column ----------------------------------------------------------------------------------
    RPIK_EACH(h, l) {
      RpikWork& W = Wh[h];
      if (l < M.hand[h][0]) {
        const int jt = W.jtype[l];
        const double* ax = W.axis[l];
        for (int i = 0; i < RPIK_TIPS; i++) {
          double v[3] = {0, 0, 0};
          if (M.tip_i[h][i][1] >> l & 1u) {
            if (jt == RPIK_JNT_SLIDE) {
              v[0] = ax[0]; v[1] = ax[1]; v[2] = ax[2];
            } else {
              const double rx = W.tip[i][0] - W.anchor[l][0], ry = W.tip[i][1] - W.anchor[l][1], rz = W.tip[i][2] - W.anchor[l][2];
              v[0] = ax[1] * rz - ax[2] * ry; v[1] = ax[2] * rx - ax[0] * rz; v[2] = ax[0] * ry - ax[1] * rx;
            }
          }
          for (int k = 0; k < 3; k++) W.J[l][3 * i + k] = W.w[i] * v[k];
        }
      }
    }
    ctx.sync();
    // ---- A = J D J^T + lambda^2 I, lower triangle: lanes share the 120 entries ------------------------------------
    RPIK_EACH(h, l) {
      RpikWork& W = Wh[h];
      const int nd = M.hand[h][0];
      for (int idx = l; idx < RPIK_ROWS * RPIK_ROWS; idx += RPIK_LANES) {
        const int r = idx / RPIK_ROWS, cc = idx - r * RPIK_ROWS;
        if (cc > r) continue;
        double s = 0.0;
        for (int k = 0; k < nd; k++) s += c.dof_weight[h][k] * W.J[k][r] * W.J[k][cc];
        W.A[r][cc] = r == cc ? s + c.lambda2 : s;
      }
    }
    ctx.sync();
    // ---- Cholesky factor, column by column (left-looking): lane = row ---------------------------------------------
    for (int j = 0; j < RPIK_ROWS; j++) {
      RPIK_EACH(h, l) {
        RpikWork& W = Wh[h];
        if (l >= j && l < RPIK_ROWS) {
          double s = W.A[l][j];
          for (int k = 0; k < j; k++) s -= W.A[l][k] * W.A[j][k];
          W.piv[l] = s;
        }
      }
      ctx.sync();
      RPIK_EACH(h, l) {
        RpikWork& W = Wh[h];
        if (l >= j && l < RPIK_ROWS) {
          const double d = sqrt(W.piv[j]);
          W.A[l][j] = l == j ? d : W.piv[l] / d;
        }
      }
      ctx.sync();
    }
    // ---- L y = e (y into piv), then L^T x = y (x into r): lane = row ----------------------------------------------
    for (int j = 0; j < RPIK_ROWS; j++) {
      RPIK_EACH(h, l) {
        RpikWork& W = Wh[h];
        const double y = W.r[j] / W.A[j][j];          // (r[j] is final, and nobody writes it in this phase)
        if (l > j && l < RPIK_ROWS) W.r[l] -= W.A[l][j] * y;
        if (l == j) W.piv[j] = y;
      }
      ctx.sync();
    }
    for (int j = RPIK_ROWS - 1; j >= 0; j--) {
      RPIK_EACH(h, l) {
        RpikWork& W = Wh[h];
        const double x = W.piv[j] / W.A[j][j];
        if (l < j) W.piv[l] -= W.A[j][l] * x;
        if (l == j) W.r[j] = x;
      }
      ctx.sync();
    }
    // ---- dq = D J^T x, update and clamp: lane = column -------------------------------------------------------------
    RPIK_EACH(h, l) {
      RpikWork& W = Wh[h];
      if (l < M.hand[h][0]) {
        double s = 0.0;
        for (int r = 0; r < RPIK_ROWS; r++) s += W.J[l][r] * W.r[r];
        W.q[l] = rpik_clamp(W.q[l] + c.dof_weight[h][l] * s, M.col_d[h][l][0], M.col_d[h][l][1]);
      }
    }
    ctx.sync();
  }
  // ---- transmission: lane = actuator ----------------------------------------------------------------------------------
  RPIK_EACH(h, l) {
    RpikWork& W = Wh[h];
    if (l < M.hand[h][2]) {
      double s = 0.0;
      for (int i = 0; i < M.act_i[h][l][0]; i++) s += M.act_d[h][l][i] * W.q[M.act_i[h][l][1 + i]];
      s = rpik_clamp(s, M.act_d[h][l][RPIK_MAX_TERMS], M.act_d[h][l][RPIK_MAX_TERMS + 1]);
      ((T*)c.out)[(size_t)env * (size_t)c.out_stride + M.hand[h][6] + l] = (T)s;
    }
    if (c.q_target && l < M.hand[h][0]) c.q_target[(size_t)env * M.ndof + M.hand[h][5] + l] = W.q[l];
  }
}

// Host executor: one thread runs every (hand, lane) pair of a phase in turn.
struct RpikHostCtx {
  int h0 = 0, h1 = RPIK_MAX_HANDS, l0 = 0, l1 = RPIK_LANES;
  void sync() const {}
};

// The whole call on the host (CPU tests, and the definition of what rp_ik_solve computes).  Pointers are host pointers.
inline std::string rpik_solve_host(const RpikModel& M, const rp_ik_args* a, int n_envs, int precision) {
  const std::string err = rpik_check_args(a, n_envs, M);
  if (!err.empty()) return err;
  const RpikCall c = rpik_call(a, M);
  RpikWork* W = new RpikWork[RPIK_MAX_HANDS];
  RpikHostCtx ctx;
  for (int e = a->env_first; e < a->env_first + a->env_count; e++) {
    memset(W, 0, sizeof(RpikWork) * RPIK_MAX_HANDS);
    if (precision == 32) rpik_solve_env<float>(M, c, e, W, ctx);
    else rpik_solve_env<double>(M, c, e, W, ctx);
  }
  delete[] W;
  return "";
}

#endif  // RP_IK_HPP_
