// rp_critic.hpp -- the argument checks of librp_critic.so (include/learn/rp_critic.h), the layout of its workspace and the
// device text of its two launches.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// device text takes the weight sets in use by value, so that a population can run it on a member's rows and slices: the
// member's rows through row_first, and `member` (0 in librp_critic.so, where the compiler folds it away) selects the slice
// of stacked tensors [P][...] whose bases the sets hold.  The critic itself -- forward with saved activations, the head,
// backward to ds1 -- is rp_droq.hpp's (rpd_critic_forward, rpd_critic_backward); the layer, its store, the normalised
// read, the mask sum and Adam are rp_mlp_tile.hpp's.  What is here is the step's own: the loss gradient, the column sums
// of the vector parameters and the apply launch.
#ifndef RP_CRITIC_HPP_
#define RP_CRITIC_HPP_

#include <string>

#include "../../include/learn/rp_critic.h"
#include "rp_droq.hpp"
#include "rp_mlp_tile.hpp"

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// Per critic, in floats: ds1 [R][H1], out1 [R][H1], ds2 [R][H2], part [T][V]; R = row_count, T = its tiles of 16 rows,
// V = 3 H1 + 4 H2 + 1 vector elements in the order b1, g1, be1, b2, g2, be2, w3, b3.
struct RpcLayout {
  size_t ds1, a1, ds2, part, per_critic;   // offsets and the size of one critic's part, in floats (multiples of 4)
  int T, V;
};

__host__ __device__ inline RpcLayout rpc_layout(int H1, int H2, int R) {
  RpcLayout w;
  w.T = (R + RPL_TILE_R - 1) / RPL_TILE_R;
  w.V = 3 * H1 + 4 * H2 + 1;
  w.ds1 = 0;
  w.a1 = w.ds1 + (size_t)R * H1;
  w.ds2 = w.a1 + (size_t)R * H1;
  w.part = w.ds2 + (size_t)R * H2;
  w.per_critic = (w.part + (size_t)w.T * w.V + 3) & ~(size_t)3;
  return w;
}

inline size_t rpc_workspace_bytes(int n_critics, int H1, int H2, int R) {
  return rpc_layout(H1, H2, R).per_critic * (size_t)n_critics * sizeof(float);
}

inline std::string rpc_check_workspace(const rp_critic_workspace_args* a) {
  const std::string fn = "rp_critic_workspace";
  const std::string err = rpd_check_sizes(fn, a->n_critics, a->H1, a->H2, 1);
  if (!err.empty()) return err;
  if (a->row_count < 0) return fn + ": row_count must be >= 0";
  return "";
}

inline std::string rpc_check_step(const rp_critic_step_args* a) {
  const std::string fn = "rp_critic_step";
  if (!a->obs || !a->action || !a->y || !a->mask || !a->mean || !a->inv_std || !a->q) return fn + ": a pointer is NULL";
  if (!a->p) return fn + ": critics is NULL";
  if (!a->m || !a->v) return fn + ": the moments m and v must not be NULL";
  if (!a->target) return fn + ": target is NULL";
  if (!a->workspace) return fn + ": workspace is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->keep_scale > 0.f)) return fn + ": keep_scale must be > 0";
  if (!(a->ln_eps > 0.f)) return fn + ": ln_eps must be > 0";
  if (!(a->tau >= 0.f && a->tau <= 1.f)) return fn + ": tau must lie in [0, 1]";
  if (!(a->step_size > 0.f)) return fn + ": step_size must be > 0";
  if (!(a->bc2_sqrt > 0.f)) return fn + ": bc2_sqrt must be > 0";
  if (!(a->eps > 0.f)) return fn + ": eps must be > 0";
  if (a->launches != RP_CRITIC_STEP && a->launches != RP_CRITIC_ROWS_ONLY && a->launches != RP_CRITIC_APPLY_ONLY)
    return fn + ": launches must be RP_CRITIC_STEP, RP_CRITIC_ROWS_ONLY or RP_CRITIC_APPLY_ONLY";
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpd_check_sizes(fn, a->n_critics, a->H1, a->H2, a->A);
  if (!err.empty()) return err;
  const struct { const rp_critic_set* s; const char* what; } sets[4] = {{a->p, "critic"}, {a->m, "m of critic"}, {a->v, "v of critic"},
                                                                       {a->target, "target of critic"}};
  for (int i = 0; i < a->n_critics; ++i)
    for (const auto& s : sets)
      for (int k = 0; k < RP_CRITIC_PARAMS; ++k)
        if (!s.s[i].t[k]) return fn + ": the " + s.what + " " + std::to_string(i) + " has a NULL pointer";
  if (a->B < 1) return fn + ": B must be >= 1";
  err = rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
  if (!err.empty()) return err;
  if ((uintptr_t)a->workspace & 15) return fn + ": workspace must be 16-byte aligned";
  const size_t need = rpc_workspace_bytes(a->n_critics, a->H1, a->H2, a->row_count);
  if (a->workspace_bytes < need)
    return fn + ": workspace of " + std::to_string(a->workspace_bytes) + " bytes is smaller than the " + std::to_string(need) + " this step needs";
  return "";
}

// ---- the device text ---------------------------------------------------------------------------------------------------------
namespace {

// The weight sets of a launch: critic i's ten tensors, its moments, its target and (optional, zero) where its gradients go.
struct RpcSets {
  rp_critic_set p[RP_DROQ_MAX_CRITICS], m[RP_DROQ_MAX_CRITICS], v[RP_DROQ_MAX_CRITICS], t[RP_DROQ_MAX_CRITICS], g[RP_DROQ_MAX_CRITICS];
};

// The elements of tensor `which` of a critic: what lies between two members' slices of a stacked tensor.
__device__ inline size_t rpc_elems(int which, int K, int H1, int H2) {
  switch (which) {
    case RP_CRITIC_W1: return (size_t)H1 * K;
    case RP_CRITIC_W2: return (size_t)H2 * H1;
    case RP_CRITIC_B1: case RP_CRITIC_G1: case RP_CRITIC_BE1: return (size_t)H1;
    case RP_CRITIC_B3: return 1;
    default: return (size_t)H2;   // b2, w3, g2, be2
  }
}

// Member `member`'s slices of the stacked tensors of `s`, as the critic rp_droq.hpp's routines read (K = D + A).
__device__ inline rp_droq_critic rpc_critic_of(const rp_critic_set& s, size_t member, int K, int H1, int H2) {
  auto at = [&](int which) -> const float* { return s.t[which] + member * rpc_elems(which, K, H1, H2); };
  rp_droq_critic c;
  c.net.w1 = at(RP_CRITIC_W1); c.net.b1 = at(RP_CRITIC_B1);
  c.net.w2 = at(RP_CRITIC_W2); c.net.b2 = at(RP_CRITIC_B2);
  c.net.w3 = at(RP_CRITIC_W3); c.net.b3 = at(RP_CRITIC_B3);
  c.g1 = at(RP_CRITIC_G1); c.be1 = at(RP_CRITIC_BE1);
  c.g2 = at(RP_CRITIC_G2); c.be2 = at(RP_CRITIC_BE2);
  return c;
}

// The x = cat([xn(obs), action]) of array row e, column k < D + A, read and normalised in place.
__device__ inline float rpc_x(const rp_critic_step_args& a, long long e, int k) {
  return rpl_xn_action(a.obs, a.action, a.mean, a.inv_std, a.obs_clip, e, a.D, a.A, k);
}

// The tile's partial sums of a hidden layer's vector gradients, rows ascending from 0: db <- ds, dg <- dz o, dbe <- dz.
__device__ inline void rpc_column_sums(const float* dsh, const float* act, const float* nrm, int H, float* db, float* dg, float* dbe) {
  const int n = (int)threadIdx.x;
  if (n >= H) return;
  float sb = 0.f, sg = 0.f, se = 0.f;
#pragma unroll 4
  for (int r = 0; r < RPL_TILE_R; r++) {
    const float dz = act[r * RPL_H_PITCH + n];
    const float zo = dz * nrm[r * RPL_H_PITCH + n];
    sb = sb + dsh[r * RPL_H_PITCH + n];
    sg = sg + zo;
    se = se + dz;
  }
  db[n] = sb;
  dg[n] = sg;
  dbe[n] = se;
}

#define RPC_ROWS_LDS_FLOATS (RPD_CRITIC_LDS_FLOATS + RPL_TILE_R)   // rp_droq.hpp's tile, then dq per row

// The rows launch on tile `tile` of critic i.  `lds`: RPC_ROWS_LDS_FLOATS floats, 16-byte aligned.  Row l of the range is
// array row row_first + l (the masks' row too).  All 256 threads call it together.
__device__ __forceinline__ void rpc_rows_tile(const rp_critic_step_args& a, const RpcSets& sets, int tile, int i, float* ws, float* lds,
                                              const size_t member = 0) {
  const RpdTile t = rpd_tile(lds);
  float* sdq = lds + RPD_CRITIC_LDS_FLOATS;
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  const int D = a.D, A = a.A, H1 = a.H1, H2 = a.H2, R = a.row_count;
  const RpcLayout lay = rpc_layout(H1, H2, R);
  float* wsc = ws + lay.per_critic * (size_t)i;
  float* part = wsc + lay.part + (size_t)tile * lay.V;
  const int l0 = tile * RPL_TILE_R;
  const bool valid = l0 + r < R;
  const long long e = valid ? (long long)a.row_first + l0 + r : 0;
  const rp_droq_critic C = rpc_critic_of(sets.p[i], member, D + A, H1, H2);
  const float M = rpl_mask_sum(a.mask + a.row_first, R, t.sw);   // the header's MSUM

  RpdKept k1, k2;
  const float q = rpd_critic_forward(
      [&](int rr, int k) {
        if (l0 + rr >= R) return 0.f;
        return rpc_x(a, (long long)a.row_first + l0 + rr, k);
      },
      D + A, H1, H2, C, (uint32_t)e, RP_CRITIC_COUNTER + 2u * (uint32_t)i, rpd_drop_of(a), t, k1, k2,
      valid ? wsc + lay.a1 + (size_t)(l0 + r) * H1 : nullptr);
  // the loss gradient; st <- dout2
  {
    const float* w3 = C.net.w3;
    const int groups = H2 >> 2;
    float dq = 0.f;
    if (valid) {
      const float er = q - a.y[e];
      const float f = a.mask[e] * er;
      dq = f / M;
      if (j == 0) a.q[(size_t)i * a.B + (size_t)e] = q;
    }
    if (j == 0) sdq[r] = dq;
#pragma unroll
    for (int g = 0; g < RPD_GROUPS; g++) {
      const int grp = j + RPD_ROW_LANES * g;
      if (grp < groups) {
#pragma unroll
        for (int c = 0; c < 4; c++) t.st[r * RPL_H_PITCH + 4 * grp + c] = dq * w3[4 * grp + c];
      }
    }
    __syncthreads();
  }
  // dw3 and db3 of the tile, rows ascending
  if (tid < H2) {
    float s = 0.f;
    for (int rr = 0; rr < RPL_TILE_R; rr++) {
      const float x = sdq[rr] * t.a2[rr * RPL_H_PITCH + tid];
      s = s + x;
    }
    part[3 * H1 + 3 * H2 + tid] = s;
  }
  if (tid == RPL_BLOCK - 1) {
    float s = 0.f;
    for (int rr = 0; rr < RPL_TILE_R; rr++) s = s + sdq[rr];
    part[3 * H1 + 4 * H2] = s;
  }
  __syncthreads();
  rpd_critic_backward(H1, H2, C, a.keep_scale, t, k1, k2, valid ? wsc + lay.ds2 + (size_t)(l0 + r) * H2 : nullptr,
                      valid ? wsc + lay.ds1 + (size_t)(l0 + r) * H1 : nullptr,
                      [&] { rpc_column_sums(t.st, t.a2, t.n2, H2, part + 3 * H1, part + 3 * H1 + H2, part + 3 * H1 + 2 * H2); });
  rpc_column_sums(t.st, t.a1, t.n1, H1, part, part + H1, part + 2 * H1);
}

// Adam on element `idx` of tensor `which` of critic i with the gradient g, then the target's Polyak step (the header's
// statements).
__device__ inline void rpc_adam(const rp_critic_step_args& a, const RpcSets& sets, int i, int which, size_t idx, float g) {
  const RplAdam o = {a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.step_size, a.bc2_sqrt, a.eps};
  float* pp = sets.p[i].t[which] + idx;
  float* pm = sets.m[i].t[which] + idx;
  float* pv = sets.v[i].t[which] + idx;
  float* pt = sets.t[i].t[which] + idx;
  float* pg = sets.g[i].t[which];
  if (pg) pg[idx] = g;
  float m = *pm, v = *pv, p = *pp, t = *pt;
  rpl_adam(o, g, m, v, p);
  t = rpl_polyak(t, p, a.tau);
  *pm = m;
  *pv = v;
  *pp = p;
  *pt = t;
}

// The apply launch: block `blk` of critic i.  `lds`: the two staging arrays of the layer.
__device__ __forceinline__ void rpc_apply_block(const rp_critic_step_args& a, const RpcSets& sets, int blk, int i, const float* ws,
                                                float* lds, const size_t member = 0) {
  float* sa = lds;
  float* sw = sa + RPL_TILE_R * RPL_S_PITCH;
  const int D = a.D, A = a.A, H1 = a.H1, H2 = a.H2, R = a.row_count;
  const RpcLayout lay = rpc_layout(H1, H2, R);
  const float* wsc = ws + lay.per_critic * (size_t)i;
  const int tiles1 = (D + A + 15) >> 4, tiles2 = H1 >> 4;
  f32x4 acc[RPL_ACC];
  if (blk < tiles1) {   // (block-uniform, as the two below)
    const int k0 = blk * 16;
    const float* ds1 = wsc + lay.ds1;
    rpl_layer_of<true>(
        [&](int rr, int l) {
          if (k0 + rr >= D + A) return 0.f;
          return rpc_x(a, (long long)a.row_first + l, k0 + rr);
        },
        [&](int n, int l) { return ds1[(size_t)l * H1 + n]; }, R, H1, sa, sw, acc);
    const size_t base = member * rpc_elems(RP_CRITIC_W1, D + A, H1, H2);
    rpl_adam_tile(acc, k0, D + A, H1, [&a, &sets, i, base](size_t idx, float g) { rpc_adam(a, sets, i, RP_CRITIC_W1, base + idx, g); });
    return;
  }
  blk -= tiles1;
  if (blk < tiles2) {
    const int k0 = blk * 16;
    const float* out1 = wsc + lay.a1;
    const float* ds2 = wsc + lay.ds2;
    rpl_layer_of<true>([&](int rr, int l) { return out1[(size_t)l * H1 + k0 + rr]; },
                       [&](int n, int l) { return ds2[(size_t)l * H2 + n]; }, R, H2, sa, sw, acc);
    const size_t base = member * rpc_elems(RP_CRITIC_W2, D + A, H1, H2);
    rpl_adam_tile(acc, k0, H1, H2, [&a, &sets, i, base](size_t idx, float g) { rpc_adam(a, sets, i, RP_CRITIC_W2, base + idx, g); });
    return;
  }
  blk -= tiles2;
  const int el = blk * RPL_BLOCK + (int)threadIdx.x;
  if (el >= lay.V) return;
  const float* part = wsc + lay.part + el;
  float g = 0.f;
  for (int t = 0; t < lay.T; t++) g = g + part[(size_t)t * lay.V];
  int which, idx = el;
  if (idx < H1) which = RP_CRITIC_B1;
  else if ((idx -= H1) < H1) which = RP_CRITIC_G1;
  else if ((idx -= H1) < H1) which = RP_CRITIC_BE1;
  else if ((idx -= H1) < H2) which = RP_CRITIC_B2;
  else if ((idx -= H2) < H2) which = RP_CRITIC_G2;
  else if ((idx -= H2) < H2) which = RP_CRITIC_BE2;
  else if ((idx -= H2) < H2) which = RP_CRITIC_W3;
  else { idx -= H2; which = RP_CRITIC_B3; }
  rpc_adam(a, sets, i, which, member * rpc_elems(which, D + A, H1, H2) + (size_t)idx, g);
}

}  // namespace

#endif  // RP_CRITIC_HPP_
