// rp_critic.hpp -- the argument checks of librp_critic.so (include/learn/rp_critic.h), the layout of its workspace and the
// device text of its two launches.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// device text is parametrised as rp_droq.hpp's: a row map resolved at compile time (the kernels of librp_critic.so pass
// the identity) and the weight sets in use, by value, so that a population can run it on a member's rows and slices:
// `member` (0 in librp_critic.so, where the compiler folds it away) selects the slice of stacked tensors [P][...] whose
// bases the sets hold.
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

inline std::string rpc_check_sizes(const std::string& fn, int n_critics, int H1, int H2) {
  if (n_critics < 1 || n_critics > RP_DROQ_MAX_CRITICS)
    return fn + ": n_critics must be 1 .. " + std::to_string(RP_DROQ_MAX_CRITICS) + ", got " + std::to_string(n_critics);
  std::string err = rpl_check_hidden(fn, "H1", H1);
  if (err.empty()) err = rpl_check_hidden(fn, "H2", H2);
  return err;
}

inline std::string rpc_check_workspace(const rp_critic_workspace_args* a) {
  const std::string fn = "rp_critic_workspace";
  const std::string err = rpc_check_sizes(fn, a->n_critics, a->H1, a->H2);
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
  std::string err = rpc_check_sizes(fn, a->n_critics, a->H1, a->H2);
  if (!err.empty()) return err;
  if (a->A < 1 || 2 * a->A > RP_SAC_MAX_HEAD) return fn + ": A must be 1 .. " + std::to_string(RP_SAC_MAX_HEAD / 2) + ", got " + std::to_string(a->A);
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

// rpl_layer (rp_mlp_tile.hpp) with the weights behind a loader too: acc[i] (column tile wave + 4 i) = the chain over k
// ascending, from 0, of load_a(r, k) load_w(n, k).  kColFast says which index is consecutive in memory and so which one
// the staging threads run along: k (false: the forward layers, W [N][K]) or r and n (true: W2 transposed, and the
// parameter gradients, whose k is the batch row).
template <bool kColFast, typename LoadA, typename LoadW>
__device__ inline void rpc_layer(LoadA load_a, LoadW load_w, int K, int N, float* sa, float* sw, f32x4 (&acc)[RPL_ACC]) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  const int tiles = (N + 15) >> 4;
  const int w_rounds = tiles * 16 * RPL_TK / RPL_BLOCK;
  // this thread's staged elements: A (ar + a_dr i, ak + a_dk i), W (wn + w_dn i, wk + w_dk i)
  const int ar = kColFast ? (tid & 15) : tid / RPL_TK, ak = kColFast ? (tid >> 4) : (tid & (RPL_TK - 1));
  constexpr int a_dr = kColFast ? 0 : RPL_BLOCK / RPL_TK, a_dk = kColFast ? 16 : 0;
  const int wn = kColFast ? tid : tid / RPL_TK, wk = kColFast ? 0 : (tid & (RPL_TK - 1));
  constexpr int w_dn = kColFast ? 0 : RPL_BLOCK / RPL_TK, w_dk = kColFast ? 1 : 0;
#pragma unroll
  for (int i = 0; i < RPL_ACC; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float pa[RPL_A_ROUNDS], pw[RPL_W_ROUNDS];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < RPL_A_ROUNDS; i++) {
      const int k = k0 + ak + a_dk * i;
      pa[i] = k < K ? load_a(ar + a_dr * i, k) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < RPL_W_ROUNDS; i++) {
      const int n = wn + w_dn * i, k = k0 + wk + w_dk * i;
      pw[i] = ((kColFast || i < w_rounds) && n < N && k < K) ? load_w(n, k) : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += RPL_TK) {
#pragma unroll
    for (int i = 0; i < RPL_A_ROUNDS; i++) sa[(ar + a_dr * i) * RPL_S_PITCH + ak + a_dk * i] = pa[i];
#pragma unroll
    for (int i = 0; i < RPL_W_ROUNDS; i++)
      if (kColFast ? wn < tiles * 16 : i < w_rounds) sw[(wn + w_dn * i) * RPL_S_PITCH + wk + w_dk * i] = pw[i];
    __syncthreads();
    if (k0 + RPL_TK < K) fetch(k0 + RPL_TK);   // (block-uniform)
#pragma unroll 2
    for (int kk = 0; kk < RPL_TK; kk += 4) {
      const float av = sa[r16 * RPL_S_PITCH + kk + kq];
#pragma unroll
      for (int i = 0; i < RPL_ACC; i++) {
        const int c = wave + 4 * i;
        if (c < tiles)   // (wave-uniform)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sw[(c * 16 + r16) * RPL_S_PITCH + kk + kq], acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

// The x = cat([xn(obs), action]) of array row e, column k < D + A, read and normalised in place.
__device__ inline float rpc_x(const rp_critic_step_args& a, long long e, int k) {
  if (k >= a.D) return a.action[(size_t)e * a.A + (k - a.D)];
  const float x = a.obs[(size_t)e * a.D + k];
  const float d = x - a.mean[k];
  const float p = d * a.inv_std[k];
  const float lo = fmaxf(p, -a.obs_clip);
  return fminf(lo, a.obs_clip);
}

// The forward row epilogue that keeps what the backward pass reads: rpd_drop_norm_relu's statements on the sums `sh`, with
// out -> `act`, the normalised value o -> `nrm`, 1 / sigma -> `rinv` and the keep mask of this lane's units -> the return
// value (bit 4 i + c: unit c of the lane's i-th group).  Valid rows (`out1` not NULL) also go to out1 [l][H].
// All 256 threads call it together, behind the barrier of rpl_store_layer; it ends with a barrier.
__device__ inline uint32_t rpc_forward_rows(const float* sh, float* act, float* nrm, int H, const float* __restrict__ g,
                                            const float* __restrict__ be, uint32_t b, uint32_t ctr, const rp_critic_step_args& a,
                                            float& rinv, float* out1) {
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
      const float4 s = *reinterpret_cast<const float4*>(sh + r * RPL_H_PITCH + 4 * grp);
      const RpplWords w = rppl_philox(a.round, b, (uint32_t)grp, ctr, a.seed_lo, a.seed_hi);
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float v = sv[c] * a.keep_scale;
        const bool keep = w.w[c] >= a.drop_threshold;
        bits |= keep ? 1u << (4 * i + c) : 0u;
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
      *reinterpret_cast<float4*>(nrm + r * RPL_H_PITCH + 4 * grp) = make_float4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<float4*>(act + r * RPL_H_PITCH + 4 * grp) = make_float4(u[0], u[1], u[2], u[3]);
      if (out1) *reinterpret_cast<float4*>(out1 + 4 * grp) = make_float4(u[0], u[1], u[2], u[3]);
    }
  }
  rinv = rr;
  __syncthreads();
  return bits;
}

// The backward row pass of one hidden layer (the header's statements).  In: `dsh` the gradient of the layer's output,
// `act` the output, `nrm` the normalised value.  Out: `act` <- dz, `dsh` <- ds, and ds of a valid row (`ds_out` not NULL) to
// ds_out [H].  All 256 threads call it together; it ends with a barrier.
__device__ inline void rpc_backward_rows(float* dsh, float* act, const float* nrm, int H, const float* __restrict__ g, uint32_t bits,
                                         float rinv, float keep_scale, float* ds_out) {
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
        const float dh = rinv * t3;
        const float sc = dh * keep_scale;
        ds[c] = (bits >> (4 * i + c)) & 1u ? sc : 0.f;
      }
      *reinterpret_cast<float4*>(dsh + r * RPL_H_PITCH + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      if (ds_out) *reinterpret_cast<float4*>(ds_out + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
    }
  }
  __syncthreads();
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

// The layer's sums (plus bias, where there is one) into the tile's array `sh`; ends with a barrier.
__device__ inline void rpc_store(const f32x4 (&acc)[RPL_ACC], const float* __restrict__ b, int N, float* sh) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < RPL_ACC; i++) {
    const int n = (wave + 4 * i) * 16 + r16;
    if (n < N) {
      const float bias = b ? b[n] : 0.f;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) sh[(4 * kq + reg) * RPL_H_PITCH + n] = b ? acc[i][reg] + bias : acc[i][reg];
    }
  }
  __syncthreads();
}

#define RPC_ROWS_LDS_FLOATS (RPL_TILE_R * RPL_S_PITCH + RP_LEARN_MAX_H * RPL_S_PITCH + 5 * RPL_TILE_R * RPL_H_PITCH + RPL_TILE_R)

// The rows launch on tile `tile` of critic i.  `lds`: RPC_ROWS_LDS_FLOATS floats, 16-byte aligned.  `rows`: range row ->
// array row (the masks' row too).  All 256 threads call it together.
template <typename Rows>
__device__ __forceinline__ void rpc_rows_tile(const rp_critic_step_args& a, const RpcSets& sets, const Rows rows, int tile, int i,
                                              float* ws, float* lds, const size_t member = 0) {
  float* sa = lds;
  float* sw = sa + RPL_TILE_R * RPL_S_PITCH;
  float* st = sw + RP_LEARN_MAX_H * RPL_S_PITCH;    // sums, then gradients   (16 x 34 and 256 x 34 floats: 16-byte multiples)
  float* a1 = st + RPL_TILE_R * RPL_H_PITCH;        // out1, then dz1
  float* n1 = a1 + RPL_TILE_R * RPL_H_PITCH;        // o1
  float* a2 = n1 + RPL_TILE_R * RPL_H_PITCH;        // out2, then dz2
  float* n2 = a2 + RPL_TILE_R * RPL_H_PITCH;        // o2
  float* sdq = n2 + RPL_TILE_R * RPL_H_PITCH;       // dq per row
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  const int D = a.D, A = a.A, H1 = a.H1, H2 = a.H2, R = a.row_count;
  const RpcLayout lay = rpc_layout(H1, H2, R);
  float* wsc = ws + lay.per_critic * (size_t)i;
  float* part = wsc + lay.part + (size_t)tile * lay.V;
  const int l0 = tile * RPL_TILE_R;
  const bool valid = l0 + r < R;
  const long long e = valid ? rows((long long)a.row_first + l0 + r) : 0;
  rp_critic_set P = sets.p[i];
#pragma unroll
  for (int k = 0; k < RP_CRITIC_PARAMS; k++) P.t[k] += member * rpc_elems(k, D + A, H1, H2);
  const uint32_t ctr = RP_CRITIC_COUNTER + 2u * (uint32_t)i;

  // M: the header's MSUM
  float pm = 0.f;
  for (int l = tid; l < R; l += RPL_BLOCK) pm = pm + a.mask[rows((long long)a.row_first + l)];
  sw[tid] = pm;
  __syncthreads();
  for (int s = RPL_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) sw[tid] = sw[tid] + sw[tid + s];
    __syncthreads();
  }
  const float M = fmaxf(sw[0], 1.f);
  __syncthreads();

  f32x4 acc[RPL_ACC];
  float r1, r2;
  // forward
  rpc_layer<false>(
      [&](int rr, int k) {
        if (l0 + rr >= R) return 0.f;
        return rpc_x(a, rows((long long)a.row_first + l0 + rr), k);
      },
      [&](int n, int k) { return P.t[RP_CRITIC_W1][(size_t)n * (D + A) + k]; }, D + A, H1, sa, sw, acc);
  rpc_store(acc, P.t[RP_CRITIC_B1], H1, st);
  const uint32_t bits1 = rpc_forward_rows(st, a1, n1, H1, P.t[RP_CRITIC_G1], P.t[RP_CRITIC_BE1], (uint32_t)e, ctr, a, r1,
                                          valid ? wsc + lay.a1 + (size_t)(l0 + r) * H1 : nullptr);
  rpc_layer<false>([&](int rr, int k) { return a1[rr * RPL_H_PITCH + k]; },
                   [&](int n, int k) { return P.t[RP_CRITIC_W2][(size_t)n * H1 + k]; }, H1, H2, sa, sw, acc);
  rpc_store(acc, P.t[RP_CRITIC_B2], H2, st);
  const uint32_t bits2 = rpc_forward_rows(st, a2, n2, H2, P.t[RP_CRITIC_G2], P.t[RP_CRITIC_BE2], (uint32_t)e, ctr + 1u, a, r2, nullptr);
  // the head and the loss gradient; st <- dout2
  {
    const float* w3 = P.t[RP_CRITIC_W3];
    const int groups = H2 >> 2;
    float p = 0.f;
#pragma unroll
    for (int g = 0; g < RPD_GROUPS; g++) {
      const int grp = j + RPD_ROW_LANES * g;
      if (grp < groups) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const float t = a2[r * RPL_H_PITCH + 4 * grp + c] * w3[4 * grp + c];
          p = p + t;
        }
      }
    }
    const float s = rpd_row_sum(p);
    const float q = s + P.t[RP_CRITIC_B3][0];
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
        for (int c = 0; c < 4; c++) st[r * RPL_H_PITCH + 4 * grp + c] = dq * w3[4 * grp + c];
      }
    }
    __syncthreads();
  }
  // dw3 and db3 of the tile, rows ascending
  if (tid < H2) {
    float s = 0.f;
    for (int rr = 0; rr < RPL_TILE_R; rr++) {
      const float t = sdq[rr] * a2[rr * RPL_H_PITCH + tid];
      s = s + t;
    }
    part[3 * H1 + 3 * H2 + tid] = s;
  }
  if (tid == RPL_BLOCK - 1) {
    float s = 0.f;
    for (int rr = 0; rr < RPL_TILE_R; rr++) s = s + sdq[rr];
    part[3 * H1 + 4 * H2] = s;
  }
  __syncthreads();
  // backward
  rpc_backward_rows(st, a2, n2, H2, P.t[RP_CRITIC_G2], bits2, r2, a.keep_scale, valid ? wsc + lay.ds2 + (size_t)(l0 + r) * H2 : nullptr);
  rpc_column_sums(st, a2, n2, H2, part + 3 * H1, part + 3 * H1 + H2, part + 3 * H1 + 2 * H2);
  rpc_layer<true>([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; },
                  [&](int n, int k) { return P.t[RP_CRITIC_W2][(size_t)k * H1 + n]; }, H2, H1, sa, sw, acc);
  rpc_store(acc, nullptr, H1, st);
  rpc_backward_rows(st, a1, n1, H1, P.t[RP_CRITIC_G1], bits1, r1, a.keep_scale, valid ? wsc + lay.ds1 + (size_t)(l0 + r) * H1 : nullptr);
  rpc_column_sums(st, a1, n1, H1, part, part + H1, part + 2 * H1);
}

// Adam on element `idx` of tensor `which` of critic i with the gradient g, then the target's Polyak step (the header's
// statements).
__device__ inline void rpc_adam(const rp_critic_step_args& a, const RpcSets& sets, int i, int which, size_t idx, float g) {
  float* pp = sets.p[i].t[which] + idx;
  float* pm = sets.m[i].t[which] + idx;
  float* pv = sets.v[i].t[which] + idx;
  float* pt = sets.t[i].t[which] + idx;
  float* pg = sets.g[i].t[which];
  if (pg) pg[idx] = g;
  float m = *pm, v = *pv, p = *pp, t = *pt;
  float x = g - m;
  x = x * a.one_minus_beta1;
  m = m + x;
  float c = g * a.one_minus_beta2;
  c = c * g;
  v = v * a.beta2;
  v = v + c;
  float den = sqrtf(v);
  den = den / a.bc2_sqrt;
  den = den + a.eps;
  float u = m / den;
  u = u * a.step_size;
  p = p - u;
  float w = p - t;
  w = w * a.tau;
  t = t + w;
  *pm = m;
  *pv = v;
  *pp = p;
  *pt = t;
}

// Adam on the 16 x N tile of a weight matrix [N][K] whose gradient `acc` holds: row 4 kq + reg is column k0 + .. of the
// matrix, the accumulator's column its row n.  `base`: the matrix's first element in the tensor (a member's slice).
__device__ inline void rpc_adam_tile(const rp_critic_step_args& a, const RpcSets& sets, int i, int which, const f32x4 (&acc)[RPL_ACC],
                                     int k0, int K, int N, size_t base) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < RPL_ACC; t++) {
    const int n = (wave + 4 * t) * 16 + r16;
    if (n < N) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int k = k0 + 4 * kq + reg;
        if (k < K) rpc_adam(a, sets, i, which, base + (size_t)n * K + k, acc[t][reg]);
      }
    }
  }
}

// The apply launch: block `blk` of critic i.  `lds`: the two staging arrays of rpc_layer.
template <typename Rows>
__device__ __forceinline__ void rpc_apply_block(const rp_critic_step_args& a, const RpcSets& sets, const Rows rows, int blk, int i,
                                                const float* ws, float* lds, const size_t member = 0) {
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
    rpc_layer<true>(
        [&](int rr, int l) {
          if (k0 + rr >= D + A) return 0.f;
          return rpc_x(a, rows((long long)a.row_first + l), k0 + rr);
        },
        [&](int n, int l) { return ds1[(size_t)l * H1 + n]; }, R, H1, sa, sw, acc);
    rpc_adam_tile(a, sets, i, RP_CRITIC_W1, acc, k0, D + A, H1, member * rpc_elems(RP_CRITIC_W1, D + A, H1, H2));
    return;
  }
  blk -= tiles1;
  if (blk < tiles2) {
    const int k0 = blk * 16;
    const float* out1 = wsc + lay.a1;
    const float* ds2 = wsc + lay.ds2;
    rpc_layer<true>([&](int rr, int l) { return out1[(size_t)l * H1 + k0 + rr]; },
                    [&](int n, int l) { return ds2[(size_t)l * H2 + n]; }, R, H2, sa, sw, acc);
    rpc_adam_tile(a, sets, i, RP_CRITIC_W2, acc, k0, H1, H2, member * rpc_elems(RP_CRITIC_W2, D + A, H1, H2));
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
