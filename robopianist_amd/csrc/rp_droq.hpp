// rp_droq.hpp -- the argument checks of librp_droq.so (include/learn/rp_droq.h), and the device text of its target, which
// librp_pop.so runs too.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  They
// are rp_sac.hpp's rps_check_target on the DroQ block, plus the LayerNorm pointers and the two positive scalars.
#ifndef RP_DROQ_HPP_
#define RP_DROQ_HPP_

#include <string>

#include "../../include/learn/rp_droq.h"
#include "rp_sac.hpp"

inline std::string rpd_check_target(const rp_droq_target_args* a) {
  const std::string fn = "rp_droq_target";
  if (!a->next_obs || !a->action || !a->logp || !a->reward || !a->discount || !a->mean || !a->inv_std || !a->log_alpha || !a->y)
    return fn + ": a pointer is NULL";
  if (!a->critics) return fn + ": critics is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->keep_scale > 0.f)) return fn + ": keep_scale must be > 0";
  if (!(a->ln_eps > 0.f)) return fn + ": ln_eps must be > 0";
  if (a->n_critics < 1 || a->n_critics > RP_DROQ_MAX_CRITICS)
    return fn + ": n_critics must be 1 .. " + std::to_string(RP_DROQ_MAX_CRITICS) + ", got " + std::to_string(a->n_critics);
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpl_check_hidden(fn, "H1", a->H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", a->H2);
  if (!err.empty()) return err;
  if (a->A < 1 || 2 * a->A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(a->A);
  for (int i = 0; i < a->n_critics; ++i) {
    const rp_droq_critic& c = a->critics[i];
    err = rpl_check_mlp(fn, ("critic " + std::to_string(i)).c_str(), &c.net);
    if (!err.empty()) return err;
    if (!c.g1 || !c.be1 || !c.g2 || !c.be2) return fn + ": the LayerNorm of critic " + std::to_string(i) + " has a NULL pointer";
  }
  if (a->B < 1) return fn + ": B must be >= 1";
  return rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
}

// ---- the device text of the target, shared with librp_pop.so (rp_pop.hip) -----------------------------------------------
// Parametrised as rp_sac.hpp's bodies: a row map resolved at compile time (the kernel of librp_droq.so passes the
// identity) and the weight set in use, by value.
namespace {

#define RPD_ROW_LANES 16                                   // the lanes that own one row of the tile
#define RPD_GROUPS (RP_LEARN_MAX_H / 4 / RPD_ROW_LANES)    // groups of four units per lane at 256 units

// The weight set of a launch: critic i's pointers.  (The population's set gives a member's slices instead.)
struct RpdCritics {
  rp_droq_critic c[RP_DROQ_MAX_CRITICS];
  __device__ rp_droq_critic operator()(int i) const { return c[i]; }
};

// The sum of `p` over the sixteen lanes of a row: p[j] + p[j ^ 1], then ^ 2, ^ 4, ^ 8.  Every lane gets the same bits.
__device__ inline float rpd_row_sum(float p) {
#pragma unroll
  for (int m = 1; m < RPD_ROW_LANES; m <<= 1) {
    const float o = __shfl_xor(p, m, RPD_ROW_LANES);
    p = p + o;
  }
  return p;
}

// Dropout, LayerNorm and ReLU on the tile's sums `sh` [16][RPL_H_PITCH], in place (the header's epilogue, statement by
// statement).  `e0`: the tile's first row, `rows` its map to the absolute batch row that keys the masks; `ctr`: the last
// Philox counter word.  All 256 threads call it together, behind the barrier of rpl_store_layer; it ends with a barrier.
template <typename Rows>
__device__ inline void rpd_drop_norm_relu(float* sh, int H, const float* __restrict__ g, const float* __restrict__ be,
                                          long long e0, const Rows rows, uint32_t ctr, const rp_droq_target_args& a) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  float* row = sh + r * RPL_H_PITCH;
  const uint32_t b = (uint32_t)rows(e0 + r);
  const int groups = H >> 2;
  const float fH = (float)H;
  float h[RPD_GROUPS][4];
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      const float4 s = *reinterpret_cast<const float4*>(row + 4 * grp);   // (sh is 16-byte aligned, the pitch 1040 bytes)
      const RpplWords w = rppl_philox(a.round, b, (uint32_t)grp, ctr, a.seed_lo, a.seed_hi);
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float v = sv[c] * a.keep_scale;
        h[i][c] = w.w[c] >= a.drop_threshold ? v : 0.f;
        p = p + h[i][c];
      }
    }
  }
  const float sum = rpd_row_sum(p);
  const float mu = sum / fH;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    if (j + RPD_ROW_LANES * i < groups) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        h[i][c] = h[i][c] - mu;
        const float dd = h[i][c] * h[i][c];
        q = q + dd;
      }
    }
  }
  const float sq = rpd_row_sum(q);
  const float var = sq / fH;
  const float t = var + a.ln_eps;
  const float root = sqrtf(t);
  const float rr = 1.f / root;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int n = 4 * grp + c;
        const float o1 = h[i][c] * rr;
        const float o2 = o1 * g[n];
        const float o3 = o2 + be[n];
        o[c] = fmaxf(o3, 0.f);
      }
      *reinterpret_cast<float4*>(row + 4 * grp) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();
}

// The tile of the rows e0 .. e0 + 15 below e_end of the caller's range; `rows` gives their array rows (the masks' row
// too).  `sa`, `sw`, `sh` (16-byte aligned), `sq`: the caller's LDS.  All 256 threads call it together.
// (__forceinline__: inlined last, as `inline` leaves it, the register allocation of rp_droq_target_kernel differs.)
template <typename Rows, typename Critics>
__device__ __forceinline__ void rpd_target_tile(const rp_droq_target_args& a, const Critics& critics, const Rows rows,
                                       const long long e0, const long long e_end, float* sa, float* sw, float* sh, float* sq) {
  const int tid = (int)threadIdx.x;
  const int D = a.D, A = a.A;
  f32x4 acc[RPL_ACC];
  const float clip = a.obs_clip, nclip = -a.obs_clip;
#pragma unroll 1
  for (int i = 0; i < a.n_critics; ++i) {   // (block-uniform)
    const rp_droq_critic cr = critics(i);
    const uint32_t ctr = RP_DROQ_COUNTER + 2u * (uint32_t)i;
    rpl_layer(
        [&](int r, int k) {
          const long long l = e0 + r;
          if (l >= e_end) return 0.f;
          const long long e = rows(l);
          if (k >= D) return a.action[(size_t)e * A + (k - D)];
          const float x = a.next_obs[(size_t)e * D + k];
          const float d = x - a.mean[k];
          const float p = d * a.inv_std[k];
          const float lo = fmaxf(p, nclip);
          return fminf(lo, clip);
        },
        D + A, cr.net.w1, a.H1, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b1, a.H1, sh);
    rpd_drop_norm_relu(sh, a.H1, cr.g1, cr.be1, e0, rows, ctr, a);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, cr.net.w2, a.H2, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b2, a.H2, sh);
    rpd_drop_norm_relu(sh, a.H2, cr.g2, cr.be2, e0, rows, ctr + 1u, a);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H2, cr.net.w3, 1, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b3, 1, sh);
    // (thread r alone reads and writes sq[r]; sh[r][0] is rewritten only behind the next layers' barriers)
    if (tid < RPL_TILE_R) {
      const float q = sh[tid * RPL_H_PITCH];
      sq[tid] = i == 0 ? q : fminf(sq[tid], q);
      if (a.q && e0 + tid < e_end) a.q[(size_t)i * a.B + (size_t)rows(e0 + tid)] = q;
    }
  }
  if (tid < RPL_TILE_R && e0 + tid < e_end) {
    const long long e = rows(e0 + tid);
    const float qm = sq[tid];
    const float al = expf(*a.log_alpha);
    const float s = al * a.logp[e];
    const float v = qm - s;
    const float nv = a.gamma * a.discount[e];
    const float tv = nv * v;
    a.y[e] = a.reward[e] + tv;
    if (a.q_min) a.q_min[e] = qm;
  }
}

}  // namespace

#endif  // RP_DROQ_HPP_
