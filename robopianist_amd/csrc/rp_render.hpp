// rp_render.hpp -- the camera renderer's tables, kinematics and per-ray routine (include/render/rp_render.h).
//
// Plain C++ behind RPR_HD, free of wave intrinsics: rp_render.hip compiles it for gfx950, and the CPU tests compile
// the same source with a host compiler (rpr_render_host below walks the same routines pixel by pixel).
#ifndef RP_RENDER_HPP_
#define RP_RENDER_HPP_

#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/render/rp_render.h"

#if defined(__HIPCC__)
#define RPR_HD __host__ __device__
#else
#define RPR_HD
#endif

// geom types (mjtGeom, model/spec.py) and their order in the sorted geom list (model/render_tables.py: TYPE_ORDER)
enum { RPR_BOX = 0, RPR_CAPSULE = 1, RPR_CYLINDER = 2, RPR_SPHERE = 3, RPR_MESH = 4, RPR_NTYPE = 5 };
enum { RPR_JNT_SLIDE = 2, RPR_JNT_HINGE = 3 };
#define RPR_MAX_BODIES 256
#define RPR_MAX_GEOMS 1024
#define RPR_N_KEYS 88
#define RPR_MAX_GRID_Y 65535   // the device's limit on a grid's y extent (rp_render_kernel: y = env)
#define RPR_FRAME 12   // floats per geom frame: world position, row-major rotation

// The tables as the kernels see them: pointers into three flat arrays (int, double, float).
struct RprModel {
  int nbody, nlevel, njnt, nv, ntree, ngeom, nplane, nkey;
  int type_end[RPR_NTYPE];
  float floor_half, floor_rgb[3], bg_rgb[3], light[6];
  // body tree (kinematics run in the engine's precision: constants are kept as double and converted on load)
  const int *body_parentid, *body_level, *body_jntadr, *body_jntnum, *body_tree;
  const double *body_pos, *body_quat;
  const int *jnt_type, *jnt_qposadr;
  const double *jnt_axis, *jnt_pos, *jnt_qpos0;
  // geoms, sorted by type
  const int *geom_id, *geom_bodyid, *geom_key, *geom_planeadr, *geom_planenum;
  const double *geom_pos, *geom_mat;
  const float *geom_size, *geom_rbound, *geom_rgb, *planes;
};

struct RprCamera {
  float pos[3], rot[9];   // rot: row-major, columns = camera axes in the world frame
  float tan_half, aspect; // tan(fovy / 2), W / H
  int height, width;
};

// ---------------------------------------------------------------------------------------------------------------
// host side: blob -> tables
// ---------------------------------------------------------------------------------------------------------------
struct RprBlobEntry { char name[40]; int32_t dtype, ndim; int64_t count, offset; };

struct RprTables {
  std::vector<int> I;
  std::vector<double> D;
  std::vector<float> F;
  RprModel M;           // counts filled; pointers hold OFFSETS until view() rebases them
  size_t o_int[16], o_dbl[8], o_flt[4];

  // returns "" or an error message
  std::string parse(const void* blob, size_t nb) {
    const unsigned char* p = (const unsigned char*)blob;
    if (!p || nb < 12) return "render blob: too short";
    uint32_t h[3]; memcpy(h, p, 12);
    if (h[0] != 0x52504D42u) return "render blob: bad magic";
    const int n = (int)h[2];
    if (12 + (size_t)n * sizeof(RprBlobEntry) > nb) return "render blob: truncated table";
    std::string err;
    auto find = [&](const char* name, RprBlobEntry& e) {
      for (int i = 0; i < n; i++) {
        memcpy(&e, p + 12 + (size_t)i * sizeof(RprBlobEntry), sizeof(e));
        if (!strncmp(e.name, name, 40)) {
          const size_t es = e.dtype == 0 ? 8 : 4;
          if (e.offset < 0 || e.count < 0 || (size_t)e.offset + (size_t)e.count * es > nb) { err = std::string("render blob: entry out of range: ") + name; return false; }
          return true;
        }
      }
      err = std::string("render blob: entry missing: ") + name + " (not a render blob? build it with model/render_tables.py)";
      return false;
    };
    auto geti = [&](const char* name, size_t want, size_t& off) {
      RprBlobEntry e;
      if (!find(name, e)) return false;
      if (e.dtype != 1 || (size_t)e.count != want) { err = std::string("render blob: bad shape: ") + name; return false; }
      off = I.size(); I.resize(off + want);
      if (want) memcpy(&I[off], p + e.offset, 4 * want);
      return true;
    };
    auto getd = [&](const char* name, size_t want, std::vector<double>& v) {
      RprBlobEntry e;
      if (!find(name, e)) return false;
      if (e.dtype != 0 || (size_t)e.count != want) { err = std::string("render blob: bad shape: ") + name; return false; }
      v.resize(want);
      if (want) memcpy(v.data(), p + e.offset, 8 * want);
      return true;
    };
    auto get1 = [&](const char* name, int& v) {
      size_t off;
      if (!geti(name, 1, off)) return false;
      v = I[off]; I.resize(off);
      return true;
    };
    memset(&M, 0, sizeof(M));
    if (!get1("rnd_nbody", M.nbody) || !get1("rnd_nlevel", M.nlevel) || !get1("rnd_njnt", M.njnt) || !get1("rnd_nv", M.nv) ||
        !get1("rnd_ntree", M.ntree) || !get1("rnd_ngeom", M.ngeom) || !get1("rnd_nplane", M.nplane) || !get1("rnd_nkey", M.nkey))
      return err;
    if (M.nbody < 1 || M.nbody > RPR_MAX_BODIES) return "render blob: nbody = " + std::to_string(M.nbody) + " (the body tree is walked by one workgroup: at most " + std::to_string(RPR_MAX_BODIES) + ")";
    if (M.ngeom < 0 || M.ngeom > RPR_MAX_GEOMS) return "render blob: ngeom = " + std::to_string(M.ngeom) + " (at most " + std::to_string(RPR_MAX_GEOMS) + ")";
    if (M.nkey < 0 || M.nkey > RPR_N_KEYS || M.njnt < 0 || M.nv < M.njnt || M.ntree < 0 || M.nplane < 0 || M.nlevel < 1)
      return "render blob: bad counts";
    const size_t nb_ = M.nbody, nj = M.njnt, ng = M.ngeom;
    const char* inames[] = {"rnd_body_parentid", "rnd_body_level", "rnd_body_jntadr", "rnd_body_jntnum", "rnd_body_tree",
                            "rnd_jnt_type", "rnd_jnt_qposadr", "rnd_geom_id", "rnd_geom_bodyid", "rnd_geom_key",
                            "rnd_geom_planeadr", "rnd_geom_planenum", "rnd_geom_type"};
    const size_t icount[] = {nb_, nb_, nb_, nb_, nb_, nj, nj, ng, ng, ng, ng, ng, ng};
    for (int k = 0; k < 13; k++) if (!geti(inames[k], icount[k], o_int[k])) return err;
    size_t te;
    if (!geti("rnd_type_end", RPR_NTYPE, te)) return err;
    for (int k = 0; k < RPR_NTYPE; k++) M.type_end[k] = I[te + k];
    I.resize(te);
    const char* dnames[] = {"rnd_body_pos", "rnd_body_quat", "rnd_jnt_axis", "rnd_jnt_pos", "rnd_jnt_qpos0", "rnd_geom_pos", "rnd_geom_mat"};
    const size_t dcount[] = {3 * nb_, 4 * nb_, 3 * nj, 3 * nj, nj, 3 * ng, 9 * ng};
    for (int k = 0; k < 7; k++) {
      std::vector<double> v;
      if (!getd(dnames[k], dcount[k], v)) return err;
      o_dbl[k] = D.size(); D.insert(D.end(), v.begin(), v.end());
    }
    const char* fnames[] = {"rnd_geom_size", "rnd_geom_rbound", "rnd_geom_rgb", "rnd_planes"};
    const size_t fcount[] = {3 * ng, ng, 3 * ng, 4 * (size_t)M.nplane};
    for (int k = 0; k < 4; k++) {
      std::vector<double> v;
      if (!getd(fnames[k], fcount[k], v)) return err;
      o_flt[k] = F.size();
      for (double x : v) F.push_back((float)x);
    }
    std::vector<double> fl, bg, li;
    if (!getd("rnd_floor", 4, fl) || !getd("rnd_background", 3, bg) || !getd("rnd_lights", 6, li)) return err;
    M.floor_half = (float)fl[0];
    for (int k = 0; k < 3; k++) { M.floor_rgb[k] = (float)fl[1 + k]; M.bg_rgb[k] = (float)bg[k]; }
    for (int k = 0; k < 6; k++) M.light[k] = (float)li[k];
    // every index the kernels follow is checked here, once
    const int* ip = I.data();
    int prev_end = 0;
    for (int k = 0; k < RPR_NTYPE; k++) { if (M.type_end[k] < prev_end) return "render blob: bad type ranges"; prev_end = M.type_end[k]; }
    if (prev_end != M.ngeom) return "render blob: type ranges do not cover the geoms";
    static const int mj_type[RPR_NTYPE] = {6, 3, 5, 2, 7};
    for (int b = 0; b < M.nbody; b++) {
      const int par = ip[o_int[0] + b], lvl = ip[o_int[1] + b], ja = ip[o_int[2] + b], jn = ip[o_int[3] + b], tr = ip[o_int[4] + b];
      if (b == 0 ? lvl != 0 : (par < 0 || par >= b || lvl != ip[o_int[1] + par] + 1 || lvl >= M.nlevel)) return "render blob: bad body tree";
      if (jn < 0 || (jn > 0 && (ja < 0 || ja + jn > M.njnt)) || tr < -1 || tr >= M.ntree) return "render blob: bad body joints";
    }
    for (int j = 0; j < M.njnt; j++) {
      const int ty = ip[o_int[5] + j], qa = ip[o_int[6] + j];
      if ((ty != RPR_JNT_SLIDE && ty != RPR_JNT_HINGE) || qa < 0 || qa >= M.nv) return "render blob: bad joint";
    }
    for (int g = 0, k = 0; g < M.ngeom; g++) {
      while (g >= M.type_end[k]) k++;
      const int id = ip[o_int[7] + g], bd = ip[o_int[8] + g], ky = ip[o_int[9] + g], pa = ip[o_int[10] + g], pn = ip[o_int[11] + g];
      if (ip[o_int[12] + g] != mj_type[k]) return "render blob: geoms are not sorted by type";
      if (id < 0 || id >= M.ngeom || bd < 0 || bd >= M.nbody || ky < -1 || ky >= RPR_N_KEYS) return "render blob: bad geom";
      if (k == RPR_MESH && (pn < 4 || pa < 0 || pa + pn > M.nplane)) return "render blob: bad hull planes";
    }
    return "";
  }

  RprModel view(const int* i, const double* d, const float* f) const {
    RprModel m = M;
    m.body_parentid = i + o_int[0]; m.body_level = i + o_int[1]; m.body_jntadr = i + o_int[2]; m.body_jntnum = i + o_int[3];
    m.body_tree = i + o_int[4]; m.jnt_type = i + o_int[5]; m.jnt_qposadr = i + o_int[6]; m.geom_id = i + o_int[7];
    m.geom_bodyid = i + o_int[8]; m.geom_key = i + o_int[9]; m.geom_planeadr = i + o_int[10]; m.geom_planenum = i + o_int[11];
    m.body_pos = d + o_dbl[0]; m.body_quat = d + o_dbl[1]; m.jnt_axis = d + o_dbl[2]; m.jnt_pos = d + o_dbl[3];
    m.jnt_qpos0 = d + o_dbl[4]; m.geom_pos = d + o_dbl[5]; m.geom_mat = d + o_dbl[6];
    m.geom_size = f + o_flt[0]; m.geom_rbound = f + o_flt[1]; m.geom_rgb = f + o_flt[2]; m.planes = f + o_flt[3];
    return m;
  }
  RprModel host_view() const { return view(I.data(), D.data(), F.data()); }
};

// Host-side refusals, shared by rp_render and the CPU build.  Returns "" or the message.
inline std::string rpr_check_args(const rp_render_args* a, int n_envs) {
  if (!a) return "rp_render: args is NULL";
  if (a->struct_size != sizeof(rp_render_args))
    return "rp_render: args->struct_size = " + std::to_string(a->struct_size) + ", this library's rp_render_args has " +
           std::to_string(sizeof(rp_render_args)) + " bytes (header / library mismatch)";
  if (!a->qpos) return "rp_render: qpos is NULL";
  if (a->height <= 0 || a->width <= 0 || a->height > 16384 || a->width > 16384)
    return "rp_render: bad image size " + std::to_string(a->height) + " x " + std::to_string(a->width);
  if (a->env_count <= 0 || a->env_first < 0 || a->env_first > n_envs - a->env_count)
    return "rp_render: envs [" + std::to_string(a->env_first) + ", " + std::to_string((long long)a->env_first + a->env_count) +
           ") are outside the batch of " + std::to_string(n_envs);
  if (!(a->fovy_deg > 0.0 && a->fovy_deg < 180.0)) return "rp_render: fovy_deg must be in (0, 180)";
  for (int k = 0; k < 3; k++) if (!std::isfinite(a->cam_pos[k])) return "rp_render: cam_pos is not finite";
  for (int k = 0; k < 9; k++) if (!std::isfinite(a->cam_rot[k])) return "rp_render: cam_rot is not finite";
  return "";
}

// rp_render_kernel takes the env from the grid's y index: a batch of more than RPR_MAX_GRID_Y envs goes out in slices.
// Number of envs of the slice that starts `first` envs into a call of `env_count` envs.
inline int rpr_slice_count(int env_count, int first) {
  const int left = env_count - first;
  return left < RPR_MAX_GRID_Y ? left : RPR_MAX_GRID_Y;
}

inline RprCamera rpr_camera(const rp_render_args* a) {
  RprCamera c;
  for (int k = 0; k < 3; k++) c.pos[k] = (float)a->cam_pos[k];
  for (int k = 0; k < 9; k++) c.rot[k] = (float)a->cam_rot[k];
  c.tan_half = (float)tan(0.5 * a->fovy_deg * 3.14159265358979323846 / 180.0);
  c.aspect = (float)a->width / (float)a->height;
  c.height = a->height; c.width = a->width;
  return c;
}

// ---------------------------------------------------------------------------------------------------------------
// kinematics (in T)
// ---------------------------------------------------------------------------------------------------------------
RPR_HD inline void rpr_sincos(float x, float& s, float& c) { s = sinf(x); c = cosf(x); }
RPR_HD inline void rpr_sincos(double x, double& s, double& c) { s = sin(x); c = cos(x); }
RPR_HD inline float rpr_sqrt(float x) { return sqrtf(x); }
RPR_HD inline double rpr_sqrt(double x) { return sqrt(x); }

template <typename T>
RPR_HD inline void rpr_quat_mat(const T* q, T* R) {
  const T w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

template <typename T>
RPR_HD inline void rpr_quat_mul(const T* a, const T* b, T* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// World frame (position p, unit quaternion q) of body b from its parent's frame.  `off` = this env's tree offsets
// [ntree][3] or null: added to the position of the hand roots (children of the world body).
template <typename T>
RPR_HD inline void rpr_body_frame(const RprModel& M, int b, const T* pp, const T* pq, const T* qpos, const T* off, T* p, T* q) {
  T R[9];
  rpr_quat_mat(pq, R);
  T lp[3] = {(T)M.body_pos[3 * b], (T)M.body_pos[3 * b + 1], (T)M.body_pos[3 * b + 2]};
  const int tr = M.body_tree[b];
  if (off && tr >= 0) { lp[0] += off[3 * tr]; lp[1] += off[3 * tr + 1]; lp[2] += off[3 * tr + 2]; }
  p[0] = pp[0] + (R[0] * lp[0] + R[1] * lp[1] + R[2] * lp[2]);
  p[1] = pp[1] + (R[3] * lp[0] + R[4] * lp[1] + R[5] * lp[2]);
  p[2] = pp[2] + (R[6] * lp[0] + R[7] * lp[1] + R[8] * lp[2]);
  const T lq[4] = {(T)M.body_quat[4 * b], (T)M.body_quat[4 * b + 1], (T)M.body_quat[4 * b + 2], (T)M.body_quat[4 * b + 3]};
  rpr_quat_mul(pq, lq, q);
  const int j0 = M.body_jntadr[b], j1 = j0 + M.body_jntnum[b];
  for (int j = j0; j < j1; j++) {
    const T ang = qpos[M.jnt_qposadr[j]] - (T)M.jnt_qpos0[j];
    const T ax[3] = {(T)M.jnt_axis[3 * j], (T)M.jnt_axis[3 * j + 1], (T)M.jnt_axis[3 * j + 2]};
    rpr_quat_mat(q, R);
    if (M.jnt_type[j] == RPR_JNT_SLIDE) {
      p[0] += (R[0] * ax[0] + R[1] * ax[1] + R[2] * ax[2]) * ang;
      p[1] += (R[3] * ax[0] + R[4] * ax[1] + R[5] * ax[2]) * ang;
      p[2] += (R[6] * ax[0] + R[7] * ax[1] + R[8] * ax[2]) * ang;
    } else {
      // hinge: rotate about the axis through the anchor, which stays where it is
      const T jp[3] = {(T)M.jnt_pos[3 * j], (T)M.jnt_pos[3 * j + 1], (T)M.jnt_pos[3 * j + 2]};
      const T an[3] = {p[0] + (R[0] * jp[0] + R[1] * jp[1] + R[2] * jp[2]),
                       p[1] + (R[3] * jp[0] + R[4] * jp[1] + R[5] * jp[2]),
                       p[2] + (R[6] * jp[0] + R[7] * jp[1] + R[8] * jp[2])};
      T s, c;
      rpr_sincos(ang * (T)0.5, s, c);
      const T dq[4] = {c, ax[0] * s, ax[1] * s, ax[2] * s};
      T nq[4];
      rpr_quat_mul(q, dq, nq);
      q[0] = nq[0]; q[1] = nq[1]; q[2] = nq[2]; q[3] = nq[3];
      rpr_quat_mat(q, R);
      p[0] = an[0] - (R[0] * jp[0] + R[1] * jp[1] + R[2] * jp[2]);
      p[1] = an[1] - (R[3] * jp[0] + R[4] * jp[1] + R[5] * jp[2]);
      p[2] = an[2] - (R[6] * jp[0] + R[7] * jp[1] + R[8] * jp[2]);
    }
  }
  const T inv = (T)1 / rpr_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
}

// Frame of (sorted) geom g from its body's frame: 12 floats, world position then row-major rotation.
template <typename T>
RPR_HD inline void rpr_geom_frame(const RprModel& M, int g, const T* bp, const T* bq, float* out) {
  T R[9];
  rpr_quat_mat(bq, R);
  const T gp[3] = {(T)M.geom_pos[3 * g], (T)M.geom_pos[3 * g + 1], (T)M.geom_pos[3 * g + 2]};
  out[0] = (float)(bp[0] + (R[0] * gp[0] + R[1] * gp[1] + R[2] * gp[2]));
  out[1] = (float)(bp[1] + (R[3] * gp[0] + R[4] * gp[1] + R[5] * gp[2]));
  out[2] = (float)(bp[2] + (R[6] * gp[0] + R[7] * gp[1] + R[8] * gp[2]));
  const double* G = M.geom_mat + 9 * g;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      out[3 + 3 * r + c] = (float)(R[3 * r] * (T)G[c] + R[3 * r + 1] * (T)G[3 + c] + R[3 * r + 2] * (T)G[6 + c]);
}

// ---------------------------------------------------------------------------------------------------------------
// the per-ray routine (float)
// ---------------------------------------------------------------------------------------------------------------
#define RPR_INF (__builtin_huge_valf())

// A convex shape cuts the ray's parameter line in an interval [t0, t1]; n0 / n1 = outward normals (geom frame) at
// its two ends.  rpr_pick turns that into the visible hit: the entry if it lies in front of the origin, the exit if
// the origin is inside, nothing if the shape lies behind.
struct RprSpan { float t0, t1, n0[3], n1[3]; };

RPR_HD inline bool rpr_box(const float* o, const float* d, const float* s, RprSpan& h) {
  float t0 = -RPR_INF, t1 = RPR_INF;
  int a0 = 0, a1 = 0;
#define RPR_SLAB(i)                                                                        \
  if (d[i] == 0.0f) { if (fabsf(o[i]) > s[i]) return false; }                              \
  else {                                                                                   \
    const float inv = 1.0f / d[i];                                                         \
    float ta = (-s[i] - o[i]) * inv, tb = (s[i] - o[i]) * inv;                             \
    if (ta > tb) { const float x = ta; ta = tb; tb = x; }                                  \
    if (ta > t0) { t0 = ta; a0 = i; }                                                      \
    if (tb < t1) { t1 = tb; a1 = i; }                                                      \
  }
  RPR_SLAB(0) RPR_SLAB(1) RPR_SLAB(2)
#undef RPR_SLAB
  if (t0 > t1) return false;
  const float d0 = a0 == 0 ? d[0] : (a0 == 1 ? d[1] : d[2]), d1 = a1 == 0 ? d[0] : (a1 == 1 ? d[1] : d[2]);
  const float s0 = d0 > 0.0f ? -1.0f : 1.0f, s1 = d1 > 0.0f ? 1.0f : -1.0f;
  h.t0 = t0; h.t1 = t1;
  h.n0[0] = a0 == 0 ? s0 : 0.0f; h.n0[1] = a0 == 1 ? s0 : 0.0f; h.n0[2] = a0 == 2 ? s0 : 0.0f;
  h.n1[0] = a1 == 0 ? s1 : 0.0f; h.n1[1] = a1 == 1 ? s1 : 0.0f; h.n1[2] = a1 == 2 ? s1 : 0.0f;
  return true;
}

RPR_HD inline bool rpr_sphere(const float* o, const float* d, float r, RprSpan& h) {
  const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const float b = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
  const float c = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - r * r;
  const float disc = b * b - a * c;
  if (disc < 0.0f) return false;
  const float sq = sqrtf(disc), ia = 1.0f / a, ir = 1.0f / r;
  h.t0 = (-b - sq) * ia; h.t1 = (-b + sq) * ia;
  for (int k = 0; k < 3; k++) { h.n0[k] = (o[k] + h.t0 * d[k]) * ir; h.n1[k] = (o[k] + h.t1 * d[k]) * ir; }
  return true;
}

// cylinder along z: radius r, half height hh, flat caps
RPR_HD inline bool rpr_cylinder(const float* o, const float* d, float r, float hh, RprSpan& h) {
  const float a = d[0] * d[0] + d[1] * d[1];
  const float b = o[0] * d[0] + o[1] * d[1];
  const float c = o[0] * o[0] + o[1] * o[1] - r * r;
  float s0 = -RPR_INF, s1 = RPR_INF;
  if (a == 0.0f) { if (c > 0.0f) return false; }
  else {
    const float disc = b * b - a * c;
    if (disc < 0.0f) return false;
    const float sq = sqrtf(disc), ia = 1.0f / a;
    s0 = (-b - sq) * ia; s1 = (-b + sq) * ia;
  }
  float z0 = -RPR_INF, z1 = RPR_INF, zn0 = 0.0f, zn1 = 0.0f;
  if (d[2] == 0.0f) { if (fabsf(o[2]) > hh) return false; }
  else {
    const float inv = 1.0f / d[2];
    z0 = (-hh - o[2]) * inv; z1 = (hh - o[2]) * inv;
    if (z0 > z1) { const float x = z0; z0 = z1; z1 = x; }
    zn0 = d[2] > 0.0f ? -1.0f : 1.0f; zn1 = -zn0;
  }
  const bool side0 = s0 >= z0, side1 = s1 <= z1;
  h.t0 = side0 ? s0 : z0; h.t1 = side1 ? s1 : z1;
  if (h.t0 > h.t1) return false;
  const float ir = 1.0f / r;
  h.n0[0] = side0 ? (o[0] + h.t0 * d[0]) * ir : 0.0f; h.n0[1] = side0 ? (o[1] + h.t0 * d[1]) * ir : 0.0f; h.n0[2] = side0 ? 0.0f : zn0;
  h.n1[0] = side1 ? (o[0] + h.t1 * d[0]) * ir : 0.0f; h.n1[1] = side1 ? (o[1] + h.t1 * d[1]) * ir : 0.0f; h.n1[2] = side1 ? 0.0f : zn1;
  return true;
}

// capsule along z: cylinder of radius r between z = -hh and hh, closed by two half spheres.  The surface is the
// union of three parts; a root of a part counts where it lies on that part (to RPR_CAP_EPS: at the seam both parts
// describe the same point, and rounding must not leave a root to neither).  The shape is convex: the smallest and the
// largest valid root are its entry and exit.
#define RPR_CAP_EPS 1e-5f
RPR_HD inline void rpr_capsule_root(float t, float nx, float ny, float nz, RprSpan& h) {
  if (t < h.t0) { h.t0 = t; h.n0[0] = nx; h.n0[1] = ny; h.n0[2] = nz; }
  if (t > h.t1) { h.t1 = t; h.n1[0] = nx; h.n1[1] = ny; h.n1[2] = nz; }
}
RPR_HD inline bool rpr_capsule(const float* o, const float* d, float r, float hh, RprSpan& h) {
  h.t0 = RPR_INF; h.t1 = -RPR_INF;
  const float ir = 1.0f / r;
  const float a2 = d[0] * d[0] + d[1] * d[1];
  const float b2 = o[0] * d[0] + o[1] * d[1];
  const float c2 = o[0] * o[0] + o[1] * o[1] - r * r;
  if (a2 > 0.0f) {
    const float disc = b2 * b2 - a2 * c2;
    if (disc < 0.0f) return false;      // misses the infinite cylinder: misses the capsule inside it
    const float sq = sqrtf(disc), ia = 1.0f / a2;
    for (int k = 0; k < 2; k++) {
      const float t = (-b2 + (k ? sq : -sq)) * ia, z = o[2] + t * d[2];
      if (fabsf(z) <= hh + RPR_CAP_EPS) rpr_capsule_root(t, (o[0] + t * d[0]) * ir, (o[1] + t * d[1]) * ir, 0.0f, h);
    }
  } else if (c2 > 0.0f) return false;
  const float a = a2 + d[2] * d[2];
  const float ia = 1.0f / a;
  for (int e = 0; e < 2; e++) {
    const float cz = e ? hh : -hh, oz = o[2] - cz;
    const float b = b2 + oz * d[2], c = c2 + oz * oz;
    const float disc = b * b - a * c;
    if (disc < 0.0f) continue;
    const float sq = sqrtf(disc);
    for (int k = 0; k < 2; k++) {
      const float t = (-b + (k ? sq : -sq)) * ia, z = oz + t * d[2];
      if (e ? z >= -RPR_CAP_EPS : z <= RPR_CAP_EPS) rpr_capsule_root(t, (o[0] + t * d[0]) * ir, (o[1] + t * d[1]) * ir, z * ir, h);
    }
  }
  return h.t0 <= h.t1;
}

// convex hull: clip of the parameter interval against the face planes n.x <= d
RPR_HD inline bool rpr_hull(const float* o, const float* d, const float* planes, int n, RprSpan& h) {
  float t0 = -RPR_INF, t1 = RPR_INF;
  int i0 = 0, i1 = 0;
  for (int i = 0; i < n; i++) {
    const float* p = planes + 4 * i;
    const float den = p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
    const float num = p[3] - (p[0] * o[0] + p[1] * o[1] + p[2] * o[2]);
    if (den == 0.0f) { if (num < 0.0f) return false; continue; }
    const float t = num / den;
    if (den < 0.0f) { if (t > t0) { t0 = t; i0 = i; } }
    else if (t < t1) { t1 = t; i1 = i; }
  }
  if (t0 > t1) return false;
  h.t0 = t0; h.t1 = t1;
  for (int k = 0; k < 3; k++) { h.n0[k] = planes[4 * i0 + k]; h.n1[k] = planes[4 * i1 + k]; }
  return true;
}

struct RprHit {
  float t;      // ray parameter of the nearest hit = its depth along the camera's -z axis (the ray's camera-frame z is -1)
  int gi;       // sorted geom index; ngeom = floor; -1 = nothing
  int id;       // segmentation id
  float n[3];   // outward normal, world frame
};

RPR_HD inline void rpr_pixel_ray(const RprCamera& cam, int r, int c, float* d) {
  const float x = (2.0f * ((float)c + 0.5f) / (float)cam.width - 1.0f) * cam.tan_half * cam.aspect;
  const float y = (1.0f - 2.0f * ((float)r + 0.5f) / (float)cam.height) * cam.tan_half;
  d[0] = cam.rot[0] * x + cam.rot[1] * y - cam.rot[2];
  d[1] = cam.rot[3] * x + cam.rot[4] * y - cam.rot[5];
  d[2] = cam.rot[6] * x + cam.rot[7] * y - cam.rot[8];
}

// One geom against the ray (o, d), world frame; `fr` = its frame.  Updates `best` when the geom is hit nearer (or as
// near, with a lower model id).
RPR_HD inline void rpr_test_geom(const RprModel& M, int type, int g, const float* fr, const float* o, const float* d, float dd, RprHit& best) {
  // bounding sphere
  const float cx = fr[0] - o[0], cy = fr[1] - o[1], cz = fr[2] - o[2];
  const float rb = M.geom_rbound[g];
  const float b = cx * d[0] + cy * d[1] + cz * d[2];
  const float c = cx * cx + cy * cy + cz * cz - rb * rb;
  if (c > 0.0f && b <= 0.0f) return;
  if (b * b - dd * c < 0.0f) return;
  // the ray in the geom frame
  const float ol[3] = {-(fr[3] * cx + fr[6] * cy + fr[9] * cz), -(fr[4] * cx + fr[7] * cy + fr[10] * cz), -(fr[5] * cx + fr[8] * cy + fr[11] * cz)};
  const float dl[3] = {fr[3] * d[0] + fr[6] * d[1] + fr[9] * d[2], fr[4] * d[0] + fr[7] * d[1] + fr[10] * d[2], fr[5] * d[0] + fr[8] * d[1] + fr[11] * d[2]};
  const float* s = M.geom_size + 3 * g;
  RprSpan h;
  bool hit;
  if (type == RPR_BOX) hit = rpr_box(ol, dl, s, h);
  else if (type == RPR_CAPSULE) hit = rpr_capsule(ol, dl, s[0], s[1], h);
  else if (type == RPR_CYLINDER) hit = rpr_cylinder(ol, dl, s[0], s[1], h);
  else if (type == RPR_SPHERE) hit = rpr_sphere(ol, dl, s[0], h);
  else hit = rpr_hull(ol, dl, M.planes + 4 * M.geom_planeadr[g], M.geom_planenum[g], h);
  if (!hit || !(h.t1 > 0.0f)) return;
  const bool entry = h.t0 >= 0.0f;
  const float t = entry ? h.t0 : h.t1;
  const int id = M.geom_id[g];
  if (t < best.t || (t == best.t && id < best.id)) {
    const float nx = entry ? h.n0[0] : h.n1[0], ny = entry ? h.n0[1] : h.n1[1], nz = entry ? h.n0[2] : h.n1[2];
    best.t = t; best.gi = g; best.id = id;
    best.n[0] = fr[3] * nx + fr[4] * ny + fr[5] * nz;
    best.n[1] = fr[6] * nx + fr[7] * ny + fr[8] * nz;
    best.n[2] = fr[9] * nx + fr[10] * ny + fr[11] * nz;
  }
}

// Nearest hit of the ray (o, d) among the env's geoms (`frames` [ngeom][12], sorted order) and the floor square.
RPR_HD inline void rpr_trace(const RprModel& M, const float* frames, const float* o, const float* d, RprHit& best) {
  best.t = RPR_INF; best.gi = -1; best.id = -1; best.n[0] = best.n[1] = best.n[2] = 0.0f;
  const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  int g = 0;
  for (int type = 0; type < RPR_NTYPE; type++)   // one loop per type: every lane of a wave runs the same test
    for (; g < M.type_end[type]; g++)
      rpr_test_geom(M, type, g, frames + RPR_FRAME * g, o, d, dd, best);
  // the floor: the square |x|, |y| <= floor_half of the plane z = 0; id ngeom, so it loses every exact tie
  if (d[2] != 0.0f) {
    const float t = -o[2] / d[2];
    const float x = o[0] + t * d[0], y = o[1] + t * d[1];
    if (t > 0.0f && t < best.t && fabsf(x) <= M.floor_half && fabsf(y) <= M.floor_half) {
      best.t = t; best.gi = M.ngeom; best.id = M.ngeom;
      best.n[0] = 0.0f; best.n[1] = 0.0f; best.n[2] = 1.0f;
    }
  }
}

RPR_HD inline unsigned char rpr_u8(float x) {
  x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
  return (unsigned char)(int)(255.0f * x + 0.5f);
}

// Colour of the pixel whose ray (o, d) ended in `hit`.  key_rgb = this env's [88][3] key colours or null.
RPR_HD inline void rpr_shade(const RprModel& M, const RprHit& hit, const float* o, const float* d, const unsigned char* key_rgb, unsigned char* out) {
  if (hit.gi < 0) { for (int k = 0; k < 3; k++) out[k] = rpr_u8(M.bg_rgb[k]); return; }
  float col[3];
  if (hit.gi >= M.ngeom) { col[0] = M.floor_rgb[0]; col[1] = M.floor_rgb[1]; col[2] = M.floor_rgb[2]; }
  else {
    const int key = M.geom_key[hit.gi];
    if (key_rgb && key >= 0) for (int k = 0; k < 3; k++) col[k] = (float)key_rgb[3 * key + k] * (1.0f / 255.0f);
    else for (int k = 0; k < 3; k++) col[k] = M.geom_rgb[3 * hit.gi + k];
  }
  const float p[3] = {o[0] + hit.t * d[0], o[1] + hit.t * d[1], o[2] + hit.t * d[2]};
  float shade = 0.4f;
  for (int i = 0; i < 2; i++) {
    const float lx = M.light[3 * i] - p[0], ly = M.light[3 * i + 1] - p[1], lz = M.light[3 * i + 2] - p[2];
    const float ndl = (hit.n[0] * lx + hit.n[1] * ly + hit.n[2] * lz) / sqrtf(lx * lx + ly * ly + lz * lz);
    shade += 0.3f * (ndl > 0.0f ? ndl : 0.0f);
  }
  for (int k = 0; k < 3; k++) out[k] = rpr_u8(col[k] * shade);
}

// One pixel, start to end: what a thread of rp_render_kernel does.
RPR_HD inline void rpr_pixel(const RprModel& M, const RprCamera& cam, const float* frames, const unsigned char* key_rgb,
                             int pix, unsigned char* rgb, float* depth, int* seg) {
  const int r = pix / cam.width, c = pix - r * cam.width;
  float d[3];
  rpr_pixel_ray(cam, r, c, d);
  RprHit hit;
  rpr_trace(M, frames, cam.pos, d, hit);
  if (depth) depth[pix] = hit.t;
  if (seg) seg[pix] = hit.id;
  if (rgb) rpr_shade(M, hit, cam.pos, d, key_rgb, rgb + 3 * (size_t)pix);
}

// ---------------------------------------------------------------------------------------------------------------
// The whole call on the host (CPU tests): same refusals, same routines, pointers of `a` are HOST pointers.
// `frames` [n_envs][ngeom][12] is the caller's frame buffer.
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
inline void rpr_frames_host(const RprModel& M, const T* qpos, const T* off, float* frames) {
  std::vector<T> p(3 * (size_t)M.nbody), q(4 * (size_t)M.nbody);
  p[0] = p[1] = p[2] = 0; q[0] = 1; q[1] = q[2] = q[3] = 0;
  for (int b = 1; b < M.nbody; b++) {   // (a parent precedes its children)
    const int par = M.body_parentid[b];
    rpr_body_frame<T>(M, b, &p[3 * par], &q[4 * par], qpos, off, &p[3 * b], &q[4 * b]);
  }
  for (int g = 0; g < M.ngeom; g++) {
    const int b = M.geom_bodyid[g];
    rpr_geom_frame<T>(M, g, &p[3 * b], &q[4 * b], frames + RPR_FRAME * (size_t)g);
  }
}

inline std::string rpr_render_host(const RprTables& tab, int n_envs, int precision, const rp_render_args* a, float* frames) {
  std::string err = rpr_check_args(a, n_envs);
  if (!err.empty()) return err;
  const RprModel M = tab.host_view();
  const RprCamera cam = rpr_camera(a);
  const size_t npix = (size_t)a->height * a->width;
  for (int e = a->env_first; e < a->env_first + a->env_count; e++) {
    float* fr = frames + (size_t)e * M.ngeom * RPR_FRAME;
    if (precision == 32)
      rpr_frames_host<float>(M, (const float*)a->qpos + (size_t)e * M.nv,
                             a->tree_offset ? (const float*)a->tree_offset + (size_t)e * M.ntree * 3 : nullptr, fr);
    else
      rpr_frames_host<double>(M, (const double*)a->qpos + (size_t)e * M.nv,
                              a->tree_offset ? (const double*)a->tree_offset + (size_t)e * M.ntree * 3 : nullptr, fr);
    for (size_t pix = 0; pix < npix; pix++)
      rpr_pixel(M, cam, fr, a->key_rgb ? a->key_rgb + (size_t)e * RPR_N_KEYS * 3 : nullptr, (int)pix,
                a->rgb ? a->rgb + e * npix * 3 : nullptr, a->depth ? a->depth + e * npix : nullptr,
                a->segmentation ? a->segmentation + e * npix : nullptr);
  }
  return "";
}

#endif  // RP_RENDER_HPP_
