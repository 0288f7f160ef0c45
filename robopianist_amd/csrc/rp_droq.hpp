// rp_droq.hpp -- the argument checks of librp_droq.so (include/learn/rp_droq.h), the device text of its target, which
// librp_pop.so runs too, and the one DroQ critic on the tile: the row epilogue, the forward pass that keeps what the
// backward pass reads, and the backward pass down to ds1, which the critic step (rp_critic.hpp) and the actor step
// (rp_actor.hpp) both call.  The tile's primitives (the layer, its store, the normalised read) are rp_mlp_tile.hpp's.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  They
// are rp_sac.hpp's rps_check_target on the DroQ block, plus the LayerNorm pointers and the two positive scalars.
#ifndef RP_DROQ_HPP_
#define RP_DROQ_HPP_

#include <string>

#include "../../include/learn/rp_droq.h"
#include "rp_sac.hpp"

// The sizes every DroQ critic kernel is compiled for: n_critics, H1, H2 and A in range.  (A caller whose block lacks
// one of them, as a workspace query, passes 1.)
inline std::string rpd_check_sizes(const std::string& fn, int n_critics, int H1, int H2, int A) {
  if (n_critics < 1 || n_critics > RP_DROQ_MAX_CRITICS)
    return fn + ": n_critics must be 1 .. " + std::to_string(RP_DROQ_MAX_CRITICS) + ", got " + std::to_string(n_critics);
  std::string err = rpl_check_hidden(fn, "H1", H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", H2);
  if (!err.empty()) return err;
  if (A < 1 || 2 * A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(A);
  return "";
}

inline std::string rpd_check_target(const rp_droq_target_args* a) {
  const std::string fn = "rp_droq_target";
  if (!a->next_obs || !a->action || !a->logp || !a->reward || !a->discount || !a->mean || !a->inv_std || !a->log_alpha || !a->y)
    return fn + ": a pointer is NULL";
  if (!a->critics) return fn + ": critics is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->keep_scale > 0.f)) return fn + ": keep_scale must be > 0";
  if (!(a->ln_eps > 0.f)) return fn + ": ln_eps must be > 0";
  if (a->D < 1) return fn + ": D must be >= 1";
  std::string err = rpd_check_sizes(fn, a->n_critics, a->H1, a->H2, a->A);
  if (!err.empty()) return err;
  for (int i = 0; i < a->n_critics; ++i) {
    const rp_droq_critic& c = a->critics[i];
    err = rpl_check_mlp(fn, ("critic " + std::to_string(i)).c_str(), &c.net);
    if (!err.empty()) return err;
    if (!c.g1 || !c.be1 || !c.g2 || !c.be2) return fn + ": the LayerNorm of critic " + std::to_string(i) + " has a NULL pointer";
  }
  if (a->B < 1) return fn + ": B must be >= 1";
  return rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
}

// ---- the device text ---------------------------------------------------------------------------------------------------------
namespace {

#define RPD_ROW_LANES 16                                   // the lanes that own one row of the tile
#define RPD_GROUPS (RP_LEARN_MAX_H / 4 / RPD_ROW_LANES)    // groups of four units per lane at 256 units

// The weight set of a launch: critic i's pointers.  (The population's set gives a member's slices instead.)
struct RpdCritics {
  rp_droq_critic c[RP_DROQ_MAX_CRITICS];
  __device__ rp_droq_critic operator()(int i) const { return c[i]; }
};

// What the row epilogue reads from a launch's argument block.
struct RpdDrop {
  uint32_t round, seed_lo, seed_hi, drop_threshold;
  float keep_scale, ln_eps;
};
template <typename Args>
__device__ inline RpdDrop rpd_drop_of(const Args& a) {
  return RpdDrop{a.round, a.seed_lo, a.seed_hi, a.drop_threshold, a.keep_scale, a.ln_eps};
}

// What the epilogue of a hidden layer keeps in the registers of the sixteen lanes that own a row: the keep mask of this
// lane's units (bit 4 i + c: unit c of the lane's i-th group) and 1 / sigma.
struct RpdKept {
  uint32_t bits;
  float rinv;
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

// Dropout, LayerNorm and ReLU on the tile's sums `sh` [16][RPL_H_PITCH] (the header's epilogue, statement by statement):
// the output -> `act` (which may be `sh`: in place).  `b`: the absolute batch row of this thread's row, which keys the
// masks; `ctr`: the last Philox counter word.  kKeep: the form that keeps what the backward pass reads -- the normalised
// value o -> `nrm`, the mask and 1 / sigma -> the return value, and the output of a valid row (`out` not NULL) to out [H].
// All 256 threads call it together, behind the barrier of rpl_store_layer; it ends with a barrier.
template <bool kKeep>
__device__ inline RpdKept rpd_drop_norm_relu(const float* sh, float* act, float* nrm, int H, const float* __restrict__ g,
                                             const float* __restrict__ be, uint32_t b, uint32_t ctr, const RpdDrop& a, float* out) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  const int groups = H >> 2;
  const float fH = (float)H;
  float h[RPD_GROUPS][4];
  float p = 0.f;
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      const float4 s = *reinterpret_cast<const float4*>(sh + r * RPL_H_PITCH + 4 * grp);   // (16-byte aligned, the pitch 1040 bytes)
      const RpplWords w = rppl_philox(a.round, b, (uint32_t)grp, ctr, a.seed_lo, a.seed_hi);
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float v = sv[c] * a.keep_scale;
        const bool keep = w.w[c] >= a.drop_threshold;
        if (kKeep) bits |= keep ? 1u << (4 * i + c) : 0u;
        h[i][c] = keep ? v : 0.f;
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
      float o[4], u[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int n = 4 * grp + c;
        o[c] = h[i][c] * rr;
        const float o2 = o[c] * g[n];
        const float o3 = o2 + be[n];
        u[c] = fmaxf(o3, 0.f);
      }
      if (kKeep) *reinterpret_cast<float4*>(nrm + r * RPL_H_PITCH + 4 * grp) = make_float4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<float4*>(act + r * RPL_H_PITCH + 4 * grp) = make_float4(u[0], u[1], u[2], u[3]);
      if (kKeep && out) *reinterpret_cast<float4*>(out + 4 * grp) = make_float4(u[0], u[1], u[2], u[3]);
    }
  }
  __syncthreads();
  return RpdKept{bits, rr};
}

// The backward row pass of one hidden layer (rp_critic.h's statements).  In: `dsh` the gradient of the layer's output,
// `act` the output, `nrm` the normalised value.  Out: `act` <- dz, `dsh` <- ds, and ds of a valid row (`ds_out` not NULL) to
// ds_out [H].  All 256 threads call it together; it ends with a barrier.
__device__ inline void rpd_backward_rows(float* dsh, float* act, const float* nrm, int H, const float* __restrict__ g, const RpdKept kept,
                                         float keep_scale, float* ds_out) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  const int groups = H >> 2;
  const float fH = (float)H;
  float cc[RPD_GROUPS][4], oo[RPD_GROUPS][4];
  float p1 = 0.f, p2 = 0.f;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      const int at = r * RPL_H_PITCH + 4 * grp;
      const float4 d4 = *reinterpret_cast<const float4*>(dsh + at);
      const float4 a4 = *reinterpret_cast<const float4*>(act + at);
      const float4 n4 = *reinterpret_cast<const float4*>(nrm + at);
      const float dv[4] = {d4.x, d4.y, d4.z, d4.w}, av[4] = {a4.x, a4.y, a4.z, a4.w}, nv[4] = {n4.x, n4.y, n4.z, n4.w};
      float dz[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        dz[c] = av[c] > 0.f ? dv[c] : 0.f;
        cc[i][c] = dz[c] * g[4 * grp + c];
        oo[i][c] = nv[c];
        p1 = p1 + cc[i][c];
        const float co = cc[i][c] * oo[i][c];
        p2 = p2 + co;
      }
      *reinterpret_cast<float4*>(act + at) = make_float4(dz[0], dz[1], dz[2], dz[3]);
    }
  }
  const float s1 = rpd_row_sum(p1);
  const float m1 = s1 / fH;
  const float s2 = rpd_row_sum(p2);
  const float m2 = s2 / fH;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      float ds[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float t1 = cc[i][c] - m1;
        const float t2 = oo[i][c] * m2;
        const float t3 = t1 - t2;
        const float dh = kept.rinv * t3;
        const float sc = dh * keep_scale;
        ds[c] = (kept.bits >> (4 * i + c)) & 1u ? sc : 0.f;
      }
      *reinterpret_cast<float4*>(dsh + r * RPL_H_PITCH + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      if (ds_out) *reinterpret_cast<float4*>(ds_out + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
    }
  }
  __syncthreads();
}

// ---- the critic with saved activations: the tile of the critic step and of the actor step ---------------------------------
// The two staging arrays of the layer, then five [16][RPL_H_PITCH] arrays (16 x 34 and 256 x 34 floats: 16-byte multiples).
#define RPD_CRITIC_LDS_FLOATS (RPL_TILE_R * RPL_S_PITCH + RP_LEARN_MAX_H * RPL_S_PITCH + 5 * RPL_TILE_R * RPL_H_PITCH)

struct RpdTile {
  float *sa, *sw;   // the staged operands
  float* st;        // sums, then gradients
  float *a1, *n1;   // out1, then dz1; o1
  float *a2, *n2;   // out2, then dz2; o2
};
__device__ inline RpdTile rpd_tile(float* lds) {   // `lds`: RPD_CRITIC_LDS_FLOATS floats, 16-byte aligned
  RpdTile t;
  t.sa = lds;
  t.sw = t.sa + RPL_TILE_R * RPL_S_PITCH;
  t.st = t.sw + RP_LEARN_MAX_H * RPL_S_PITCH;
  t.a1 = t.st + RPL_TILE_R * RPL_H_PITCH;
  t.n1 = t.a1 + RPL_TILE_R * RPL_H_PITCH;
  t.a2 = t.n1 + RPL_TILE_R * RPL_H_PITCH;
  t.n2 = t.a2 + RPL_TILE_R * RPL_H_PITCH;
  return t;
}

// Forward: layer 1 on x = load_x(row of the tile, k < K), its epilogue, layer 2, its epilogue, then the head as the row
// sum over the sixteen lanes of this thread's row.  -> q of that row (every lane of the row the same bits).  Leaves
// out1, o1, out2, o2 in the tile and the two layers' masks and 1 / sigma in k1 and k2.  `b`: the absolute batch row of this
// thread's row; `out1`: where the row's out1 [H1] goes, or NULL.  All 256 threads call it together.
template <typename LoadX>
__device__ inline float rpd_critic_forward(LoadX load_x, int K, int H1, int H2, const rp_droq_critic& c, uint32_t b, uint32_t ctr,
                                           const RpdDrop& drop, const RpdTile& t, RpdKept& k1, RpdKept& k2, float* out1) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  f32x4 acc[RPL_ACC];
  rpl_layer(load_x, K, c.net.w1, H1, t.sa, t.sw, acc);
  rpl_store_layer<false>(acc, c.net.b1, H1, t.st);
  k1 = rpd_drop_norm_relu<true>(t.st, t.a1, t.n1, H1, c.g1, c.be1, b, ctr, drop, out1);
  rpl_layer([&](int rr, int k) { return t.a1[rr * RPL_H_PITCH + k]; }, H1, c.net.w2, H2, t.sa, t.sw, acc);
  rpl_store_layer<false>(acc, c.net.b2, H2, t.st);
  k2 = rpd_drop_norm_relu<true>(t.st, t.a2, t.n2, H2, c.g2, c.be2, b, ctr + 1u, drop, nullptr);
  const int groups = H2 >> 2;
  float p = 0.f;
#pragma unroll
  for (int g = 0; g < RPD_GROUPS; g++) {
    const int grp = j + RPD_ROW_LANES * g;
    if (grp < groups) {
#pragma unroll
      for (int cc = 0; cc < 4; cc++) {
        const float x = t.a2[r * RPL_H_PITCH + 4 * grp + cc] * c.net.w3[4 * grp + cc];
        p = p + x;
      }
    }
  }
  const float s = rpd_row_sum(p);
  return s + c.net.b3[0];
}

// Backward from dout2, which the caller left in t.st behind a barrier: layer 2's row pass, W2 transposed, layer 1's row
// pass.  Leaves ds1 in t.st, dz1 in t.a1, dz2 in t.a2; ds2 and ds1 of this thread's row also to `ds2_out` [H2] and
// `ds1_out` [H1] where given.  `after2()` runs behind layer 2's row pass, while t.st still holds ds2 (the critic step's
// column sums).  All 256 threads call it together; it ends with a barrier.
template <typename After2>
__device__ inline void rpd_critic_backward(int H1, int H2, const rp_droq_critic& c, float keep_scale, const RpdTile& t, const RpdKept k1,
                                           const RpdKept k2, float* ds2_out, float* ds1_out, After2 after2) {
  f32x4 acc[RPL_ACC];
  rpd_backward_rows(t.st, t.a2, t.n2, H2, c.g2, k2, keep_scale, ds2_out);
  after2();
  rpl_layer_of<true>([&](int rr, int k) { return t.st[rr * RPL_H_PITCH + k]; },
                     [&](int n, int k) { return c.net.w2[(size_t)k * H1 + n]; }, H2, H1, t.sa, t.sw, acc);
  rpl_store_layer<false, false>(acc, nullptr, H1, t.st);
  rpd_backward_rows(t.st, t.a1, t.n1, H1, c.g1, k1, keep_scale, ds1_out);
}

// ---- the target, shared with librp_pop.so (rp_pop.hip) --------------------------------------------------------------------
// Parametrised as rp_sac.hpp's bodies: a row map resolved at compile time (the kernel of librp_droq.so passes the
// identity) and the weight set in use, by value.
// The tile of the rows e0 .. e0 + 15 below e_end of the caller's range; `rows` gives their array rows (the masks' row
// too).  `sa`, `sw`, `sh` (16-byte aligned), `sq`: the caller's LDS.  All 256 threads call it together.  The head stays
// the N = 1 layer: the row sum of rpd_critic_forward adds in another order.
// (__forceinline__: inlined last, as `inline` leaves it, the register allocation of rp_droq_target_kernel differs.)
template <typename Rows, typename Critics>
__device__ __forceinline__ void rpd_target_tile(const rp_droq_target_args& a, const Critics& critics, const Rows rows,
                                       const long long e0, const long long e_end, float* sa, float* sw, float* sh, float* sq) {
  const int tid = (int)threadIdx.x;
  const int D = a.D, A = a.A;
  f32x4 acc[RPL_ACC];
  const RpdDrop drop = rpd_drop_of(a);
  const uint32_t b = (uint32_t)rows(e0 + (tid >> 4));   // the batch row of the row this thread's sixteen lanes own
#pragma unroll 1
  for (int i = 0; i < a.n_critics; ++i) {   // (block-uniform)
    const rp_droq_critic cr = critics(i);
    const uint32_t ctr = RP_DROQ_COUNTER + 2u * (uint32_t)i;
    rpl_layer(
        [&](int r, int k) {
          const long long l = e0 + r;
          if (l >= e_end) return 0.f;
          return rpl_xn_action(a.next_obs, a.action, a.mean, a.inv_std, a.obs_clip, rows(l), D, A, k);
        },
        D + A, cr.net.w1, a.H1, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b1, a.H1, sh);
    rpd_drop_norm_relu<false>(sh, sh, nullptr, a.H1, cr.g1, cr.be1, b, ctr, drop, nullptr);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, cr.net.w2, a.H2, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b2, a.H2, sh);
    rpd_drop_norm_relu<false>(sh, sh, nullptr, a.H2, cr.g2, cr.be2, b, ctr + 1u, drop, nullptr);
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
