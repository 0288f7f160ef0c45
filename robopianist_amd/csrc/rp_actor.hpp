// rp_actor.hpp -- the argument checks of librp_actor.so (include/learn/rp_actor.h), the layout of its workspace and the
// device text of its two launches.
//
// The checks are host code and touch no device: a refused call returns its message before anything is launched.  The
// device text is parametrised as rp_critic.hpp's: the weight sets in use by value, the rows through row_first, and
// `member` (0 in librp_actor.so, where the compiler folds it away) selects the slice of stacked tensors [P][...] whose
// bases the sets hold, so that a population can run it on a member's rows and slices.  The critics are the critic
// step's: rp_droq.hpp's rpd_critic_forward and rpd_critic_backward on rp_critic.hpp's slices (rpc_critic_of).  The
// layer, its store, the normalised read, the mask sum, Adam and the log-probability's per-unit term are
// rp_mlp_tile.hpp's.  What is here is the step's own: the policy with its noise, the selection of the minimum, the dqa layer,
// the head gradient, the tanh layers' backward pass and the apply launch.
#ifndef RP_ACTOR_HPP_
#define RP_ACTOR_HPP_

#include <string>

#include "../../include/learn/rp_actor.h"
#include "rp_critic.hpp"
#include "rp_droq.hpp"
#include "rp_mlp_tile.hpp"
#include "rp_sac.hpp"

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// In floats: h1 [R][H1], h2 [R][H2], ds1 [R][H1], ds2 [R][H2], dout3 [R][2 A], part [T][V]; R = row_count, T = its tiles of
// 16 rows, V = H1 + H2 + 2 A + 4: the tile's sums of db1, db2, db3, then of la, gt, en and mask.
struct RpaLayout {
  size_t h1, h2, ds1, ds2, dout, part, total;   // offsets and the size, in floats
  int T, V;
};

__host__ __device__ inline RpaLayout rpa_layout(int H1, int H2, int A, int R) {
  RpaLayout w;
  w.T = (R + RPL_TILE_R - 1) / RPL_TILE_R;
  w.V = H1 + H2 + 2 * A + 4;
  w.h1 = 0;
  w.h2 = w.h1 + (size_t)R * H1;
  w.ds1 = w.h2 + (size_t)R * H2;
  w.ds2 = w.ds1 + (size_t)R * H1;
  w.dout = w.ds2 + (size_t)R * H2;
  w.part = w.dout + (size_t)R * 2 * A;
  w.total = (w.part + (size_t)w.T * w.V + 3) & ~(size_t)3;
  return w;
}

inline size_t rpa_workspace_bytes(int H1, int H2, int A, int R) { return rpa_layout(H1, H2, A, R).total * sizeof(float); }

inline std::string rpa_check_workspace(const rp_actor_workspace_args* a) {
  const std::string fn = "rp_actor_workspace";
  const std::string err = rpd_check_sizes(fn, 1, a->H1, a->H2, a->A);
  if (!err.empty()) return err;
  if (a->row_count < 0) return fn + ": row_count must be >= 0";
  return "";
}

inline std::string rpa_check_adam(const std::string& fn, const char* which, const rp_actor_adam& o) {
  if (!(o.step_size > 0.f)) return fn + ": step_size of " + which + " must be > 0";
  if (!(o.bc2_sqrt > 0.f)) return fn + ": bc2_sqrt of " + which + " must be > 0";
  if (!(o.eps > 0.f)) return fn + ": eps of " + which + " must be > 0";
  return "";
}

inline std::string rpa_check_step(const rp_actor_step_args* a) {
  const std::string fn = "rp_actor_step";
  if (!a->obs || !a->mask || !a->mean || !a->inv_std) return fn + ": a pointer is NULL";
  if (!a->critics) return fn + ": critics is NULL";
  if (!a->log_alpha) return fn + ": log_alpha is NULL";
  if (!a->log_alpha_m || !a->log_alpha_v) return fn + ": the moments m and v of log_alpha must not be NULL";
  if (!a->stats) return fn + ": stats is NULL";
  if (!a->workspace) return fn + ": workspace is NULL";
  if (!(a->obs_clip > 0.f)) return fn + ": obs_clip must be > 0";
  if (!(a->keep_scale > 0.f)) return fn + ": keep_scale must be > 0";
  if (!(a->ln_eps > 0.f)) return fn + ": ln_eps must be > 0";
  if (!(a->log_std_min <= a->log_std_max)) return fn + ": log_std_min must be <= log_std_max";
  std::string err = rpa_check_adam(fn, "the actor's optimiser", a->actor_adam);
  if (err.empty()) err = rpa_check_adam(fn, "the temperature's optimiser", a->alpha_adam);
  if (!err.empty()) return err;
  if (a->launches != RP_ACTOR_STEP && a->launches != RP_ACTOR_ROWS_ONLY && a->launches != RP_ACTOR_APPLY_ONLY)
    return fn + ": launches must be RP_ACTOR_STEP, RP_ACTOR_ROWS_ONLY or RP_ACTOR_APPLY_ONLY";
  if (a->D < 1) return fn + ": D must be >= 1";
  err = rpd_check_sizes(fn, a->n_critics, a->H1, a->H2, a->A);
  if (!err.empty()) return err;
  const struct { const rp_actor_set* s; const char* what; } sets[3] = {{&a->p, "actor"}, {&a->m, "m of the actor"}, {&a->v, "v of the actor"}};
  for (const auto& s : sets)
    for (int k = 0; k < RP_ACTOR_PARAMS; ++k)
      if (!s.s->t[k]) return fn + ": the " + s.what + " has a NULL pointer";
  for (int i = 0; i < a->n_critics; ++i)
    for (int k = 0; k < RP_CRITIC_PARAMS; ++k)
      if (!a->critics[i].t[k]) return fn + ": the critic " + std::to_string(i) + " has a NULL pointer";
  if (a->B < 1) return fn + ": B must be >= 1";
  err = rpl_check_range(fn.c_str(), a->B, a->row_first, a->row_count);
  if (!err.empty()) return err;
  if ((uintptr_t)a->workspace & 15) return fn + ": workspace must be 16-byte aligned";
  const size_t need = rpa_workspace_bytes(a->H1, a->H2, a->A, a->row_count);
  if (a->workspace_bytes < need)
    return fn + ": workspace of " + std::to_string(a->workspace_bytes) + " bytes is smaller than the " + std::to_string(need) + " this step needs";
  return "";
}

// ---- the device text ---------------------------------------------------------------------------------------------------------
namespace {

// The critics of a launch (read only) and the two constants of the log-probability.
struct RpaCritics {
  rp_critic_set c[RP_DROQ_MAX_CRITICS];
  float logp_const;   // (float)(0.5 A ln 2 pi)
  float ln2;          // (float)ln 2
};

// The elements of tensor `which` of the actor: what lies between two members' slices of a stacked tensor.
__device__ inline size_t rpa_elems(int which, int D, int H1, int H2, int A) {
  switch (which) {
    case RP_ACTOR_W1: return (size_t)H1 * D;
    case RP_ACTOR_B1: return (size_t)H1;
    case RP_ACTOR_W2: return (size_t)H2 * H1;
    case RP_ACTOR_B2: return (size_t)H2;
    case RP_ACTOR_W3: return (size_t)2 * A * H2;
    default: return (size_t)2 * A;
  }
}

// The header's za: rppl_z with the last counter word moved by RP_ACTOR_NOISE_COUNTER.
__device__ inline double rpa_z(uint32_t seed_lo, uint32_t seed_hi, uint32_t round, uint32_t e, uint32_t c) {
  uint64_t S = 0;
  for (uint32_t j = 0; j < 3; ++j) {
    const RpplWords x = rppl_philox(round, e, c, RP_ACTOR_NOISE_COUNTER + j, seed_lo, seed_hi);
    S += (uint64_t)x.w[0] + x.w[1] + x.w[2] + x.w[3];
  }
  const int64_t centred = (int64_t)S - ((int64_t)6 << 32);
  return (double)centred * 2.3283064365386962890625e-10;   // 2^-32
}

// xn of array row e, column k < D, read and normalised in place.
__device__ inline float rpa_x(const rp_actor_step_args& a, long long e, int k) {
  return rpl_xn(a.obs, a.mean, a.inv_std, a.obs_clip, e, a.D, k);
}

// The tile's rows of `sh` [16][RPL_H_PITCH] (H a multiple of 16) to `out` [.][H]; `out`: this thread's row, or NULL.
__device__ inline void rpa_rows_out(const float* sh, int H, float* out) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  if (!out) return;
  for (int grp = j; grp < (H >> 2); grp += RPD_ROW_LANES)
    *reinterpret_cast<float4*>(out + 4 * grp) = *reinterpret_cast<const float4*>(sh + r * RPL_H_PITCH + 4 * grp);
}

// The backward pass of a tanh layer on the tile: dsh [r][k] <- dh [r][k] (1 - h^2), h being this thread's row of the
// workspace (`h`; NULL: a row past the range, whose ds is 0); ds also to `ds_out` [H].  Ends with a barrier.
__device__ inline void rpa_tanh_backward(const float* dh, float* dsh, int H, const float* h, float* ds_out) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  for (int grp = j; grp < (H >> 2); grp += RPD_ROW_LANES) {
    const float4 d4 = *reinterpret_cast<const float4*>(dh + r * RPL_H_PITCH + 4 * grp);
    float4 h4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (h) h4 = *reinterpret_cast<const float4*>(h + 4 * grp);
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w}, hv[4] = {h4.x, h4.y, h4.z, h4.w};
    float ds[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const float hh = hv[c] * hv[c];
      const float om = 1.f - hh;
      const float s = dv[c] * om;
      ds[c] = h ? s : 0.f;
    }
    *reinterpret_cast<float4*>(dsh + r * RPL_H_PITCH + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
    if (ds_out) *reinterpret_cast<float4*>(ds_out + 4 * grp) = make_float4(ds[0], ds[1], ds[2], ds[3]);
  }
  __syncthreads();
}

// The tile's partial sum of a bias gradient, rows ascending from 0: db[n] = sum of sh[r][n].
__device__ inline void rpa_column_sum(const float* sh, int N, float* db) {
  const int n = (int)threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 4
  for (int r = 0; r < RPL_TILE_R; r++) s = s + sh[r * RPL_H_PITCH + n];
  db[n] = s;
}

#define RPA_HEAD_PITCH RP_LEARN_MAX_A
// rp_droq.hpp's tile (the critics run in it), then six rows of 16 per-row scalars, then a, t and dqa of the selected
// critic [16][RPA_HEAD_PITCH] and `inside` (bytes)
#define RPA_ROWS_LDS_FLOATS (RPD_CRITIC_LDS_FLOATS + 6 * RPL_TILE_R + 3 * RPL_TILE_R * RPA_HEAD_PITCH + RPL_TILE_R * RPA_HEAD_PITCH / 4)

// The rows launch on tile `tile`.  `lds`: RPA_ROWS_LDS_FLOATS floats, 16-byte aligned.  Row l of the range is array row
// row_first + l (the noise's and the masks' row too).  All 256 threads call it together.
__device__ __forceinline__ void rpa_rows_tile(const rp_actor_step_args& a, const RpaCritics& cs, int tile, float* ws, float* lds,
                                              const size_t member = 0) {
  const RpdTile tl = rpd_tile(lds);                 // a1 is the actor's dh too, a2 a critic's dqa
  float *sa = tl.sa, *sw = tl.sw, *st = tl.st, *a1 = tl.a1, *a2 = tl.a2;
  float* slp = lds + RPD_CRITIC_LDS_FLOATS;         // per row: logp
  float* swt = slp + RPL_TILE_R;                    // w
  float* sla = swt + RPL_TILE_R;                    // la
  float* sgt = sla + RPL_TILE_R;                    // gt
  float* sen = sgt + RPL_TILE_R;                    // en
  float* smk = sen + RPL_TILE_R;                    // mask
  float* sact = smk + RPL_TILE_R;                   // a
  float* stt = sact + RPL_TILE_R * RPA_HEAD_PITCH;  // t
  float* sdqa = stt + RPL_TILE_R * RPA_HEAD_PITCH;  // dqa of the selected critic
  unsigned char* sins = reinterpret_cast<unsigned char*>(sdqa + RPL_TILE_R * RPA_HEAD_PITCH);
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  const int D = a.D, A = a.A, H1 = a.H1, H2 = a.H2, R = a.row_count, N3 = 2 * a.A;
  const RpaLayout lay = rpa_layout(H1, H2, A, R);
  float* part = ws + lay.part + (size_t)tile * lay.V;
  const int l0 = tile * RPL_TILE_R;
  const bool valid = l0 + r < R;
  const long long e = valid ? (long long)a.row_first + l0 + r : 0;
  rp_actor_set P = a.p;
#pragma unroll
  for (int k = 0; k < RP_ACTOR_PARAMS; k++) P.t[k] += member * rpa_elems(k, D, H1, H2, A);

  const float M = rpl_mask_sum(a.mask + a.row_first, R, sw);   // the header's MSUM
  const float al = expf(a.log_alpha[member]);
  const float mk = valid ? a.mask[e] : 0.f;
  const float wt = mk / M;
  if (j == 0) {
    swt[r] = wt;
    smk[r] = mk;
  }

  f32x4 acc[RPL_ACC];
  auto xn = [&](int rr, int k) {
    if (l0 + rr >= R) return 0.f;
    return rpa_x(a, (long long)a.row_first + l0 + rr, k);
  };
  // 1. the policy
  rpl_layer(xn, D, P.t[RP_ACTOR_W1], H1, sa, sw, acc);
  rpl_store_layer<true>(acc, P.t[RP_ACTOR_B1], H1, st);
  rpa_rows_out(st, H1, valid ? ws + lay.h1 + (size_t)(l0 + r) * H1 : nullptr);
  rpl_layer([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; }, H1, P.t[RP_ACTOR_W2], H2, sa, sw, acc);
  rpl_store_layer<true>(acc, P.t[RP_ACTOR_B2], H2, st);
  rpa_rows_out(st, H2, valid ? ws + lay.h2 + (size_t)(l0 + r) * H2 : nullptr);
  rpl_layer([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; }, H2, P.t[RP_ACTOR_W3], N3, sa, sw, acc);
  rpl_store_layer<false>(acc, P.t[RP_ACTOR_B3], N3, st);
  {
    float* sg = sw;   // [row][RPA_HEAD_PITCH]: the terms of the log-probability (the weight stage is dead)
    for (int idx = tid; idx < RPL_TILE_R * A; idx += RPL_BLOCK) {
      const int rr = idx / A, u = idx - rr * A;
      const bool ok = l0 + rr < R;
      const long long ee = ok ? (long long)a.row_first + l0 + rr : 0;
      const float m = st[rr * RPL_H_PITCH + u];
      const float l = st[rr * RPL_H_PITCH + A + u];
      const float lc = fmaxf(l, a.log_std_min);
      const float ls = fminf(lc, a.log_std_max);
      const float zf = (float)rpa_z(a.seed_lo, a.seed_hi, a.round, (uint32_t)ee, (uint32_t)u);
      const float sd = expf(ls);
      const float t = sd * zf;
      const float p = m + t;
      const float act = tanhf(p);
      sg[rr * RPA_HEAD_PITCH + u] = rpl_logp_term(p, zf, ls, cs.ln2);
      sact[rr * RPA_HEAD_PITCH + u] = ok ? act : 0.f;
      stt[rr * RPA_HEAD_PITCH + u] = t;
      sins[rr * RPA_HEAD_PITCH + u] = (l > a.log_std_min && l < a.log_std_max) ? 1 : 0;
      if (ok && a.action) a.action[(size_t)ee * A + u] = act;
    }
    __syncthreads();
    if (tid < RPL_TILE_R) {
      float s = 0.f;
      for (int u = 0; u < A; u++) s = s + sg[tid * RPA_HEAD_PITCH + u];
      const float lp = s - cs.logp_const;
      slp[tid] = lp;
      if (l0 + tid < R && a.logp) a.logp[(long long)a.row_first + l0 + tid] = lp;
    }
    __syncthreads();
  }

  // 2. the critics, ascending, and the selection
  const RpdDrop drop = rpd_drop_of(a);
  float qm = 0.f;
  for (int i = 0; i < a.n_critics; i++) {
    const rp_droq_critic C = rpc_critic_of(cs.c[i], member, D + A, H1, H2);
    RpdKept k1, k2;
    const float q = rpd_critic_forward([&](int rr, int k) { return k < D ? xn(rr, k) : sact[rr * RPA_HEAD_PITCH + (k - D)]; }, D + A, H1, H2,
                                       C, (uint32_t)e, RP_ACTOR_COUNTER + 2u * (uint32_t)i, drop, tl, k1, k2, nullptr);
    const bool take = i == 0 || q < qm;
    if (take) qm = q;
    // st <- dout2 = w3 (dq = 1)
#pragma unroll
    for (int g = 0; g < RPD_GROUPS; g++) {
      const int grp = j + RPD_ROW_LANES * g;
      if (grp < (H2 >> 2)) {
#pragma unroll
        for (int c = 0; c < 4; c++) st[r * RPL_H_PITCH + 4 * grp + c] = C.net.w3[4 * grp + c];
      }
    }
    __syncthreads();
    rpd_critic_backward(H1, H2, C, a.keep_scale, tl, k1, k2, nullptr, nullptr, [] {});
    // dqa: the A action columns of W1, transposed
    rpl_layer_of<true>([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; },
                       [&](int n, int k) { return C.net.w1[(size_t)k * (D + A) + D + n]; }, H1, A, sa, sw, acc);
    rpl_store_layer<false, false>(acc, nullptr, A, a2);
    if (take)
      for (int u = j; u < A; u += RPD_ROW_LANES) sdqa[r * RPA_HEAD_PITCH + u] = a2[r * RPL_H_PITCH + u];
  }

  // 3. the loss's terms of the row, and the head gradient; st <- dout3
  if (j == 0) {
    const float lp = slp[r];
    const float s1 = al * lp;
    const float s2 = s1 - qm;
    sla[r] = wt * s2;
    const float lt = lp + a.target_entropy;
    sgt[r] = wt * lt;
    sen[r] = wt * lp;
    if (valid && a.q_min) a.q_min[e] = qm;
  }
  __syncthreads();
  for (int idx = tid; idx < RPL_TILE_R * A; idx += RPL_BLOCK) {
    const int rr = idx / A, u = idx - rr * A;
    const float w = swt[rr];
    const float av = sact[rr * RPA_HEAD_PITCH + u];
    const float wa = al * w;
    const float e1 = 2.f * av;
    const float e2 = wa * e1;
    const float aa = av * av;
    const float om = 1.f - aa;
    const float f1 = w * sdqa[rr * RPA_HEAD_PITCH + u];
    const float f2 = f1 * om;
    const float dp = e2 - f2;
    const float dt = dp * stt[rr * RPA_HEAD_PITCH + u];
    const float dl = dt - wa;
    const bool ok = l0 + rr < R;
    st[rr * RPL_H_PITCH + u] = ok ? dp : 0.f;
    st[rr * RPL_H_PITCH + A + u] = (ok && sins[rr * RPA_HEAD_PITCH + u]) ? dl : 0.f;
  }
  __syncthreads();
  // the tile's sums of the four scalars, rows ascending
  if (tid >= RPL_BLOCK - 4) {
    const float* src = tid == RPL_BLOCK - 4 ? sla : tid == RPL_BLOCK - 3 ? sgt : tid == RPL_BLOCK - 2 ? sen : smk;
    float s = 0.f;
    for (int rr = 0; rr < RPL_TILE_R; rr++) s = s + src[rr];
    part[H1 + H2 + N3 + (tid - (RPL_BLOCK - 4))] = s;
  }

  // 4. the actor's row-local backward pass
  if (valid)
    for (int n = j; n < N3; n += RPD_ROW_LANES) ws[lay.dout + (size_t)(l0 + r) * N3 + n] = st[r * RPL_H_PITCH + n];
  rpa_column_sum(st, N3, part + H1 + H2);
  rpl_layer_of<true>([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; },
                     [&](int n, int k) { return P.t[RP_ACTOR_W3][(size_t)k * H2 + n]; }, N3, H2, sa, sw, acc);
  rpl_store_layer<false, false>(acc, nullptr, H2, a1);
  rpa_tanh_backward(a1, st, H2, valid ? ws + lay.h2 + (size_t)(l0 + r) * H2 : nullptr,
                    valid ? ws + lay.ds2 + (size_t)(l0 + r) * H2 : nullptr);
  rpa_column_sum(st, H2, part + H1);
  rpl_layer_of<true>([&](int rr, int k) { return st[rr * RPL_H_PITCH + k]; },
                     [&](int n, int k) { return P.t[RP_ACTOR_W2][(size_t)k * H1 + n]; }, H2, H1, sa, sw, acc);
  rpl_store_layer<false, false>(acc, nullptr, H1, a1);
  rpa_tanh_backward(a1, st, H1, valid ? ws + lay.h1 + (size_t)(l0 + r) * H1 : nullptr,
                    valid ? ws + lay.ds1 + (size_t)(l0 + r) * H1 : nullptr);
  rpa_column_sum(st, H1, part);
}

__device__ inline RplAdam rpa_adam_of(const rp_actor_adam& o) {
  return RplAdam{o.one_minus_beta1, o.beta2, o.one_minus_beta2, o.step_size, o.bc2_sqrt, o.eps};
}

// Adam (rp_mlp_tile.hpp) on element `idx` of the actor's tensor `which` with the gradient g.
__device__ inline void rpa_step(const rp_actor_step_args& a, int which, size_t idx, float g) {
  rpl_adam_at(rpa_adam_of(a.actor_adam), a.p.t[which] + idx, a.m.t[which] + idx, a.v.t[which] + idx,
           a.grad.t[which] ? a.grad.t[which] + idx : nullptr, g);
}

// The blocks of the apply launch: the column tiles of w1, w2 and w3, the blocks of bias elements, the scalar block.
__host__ __device__ inline int rpa_apply_blocks(int D, int H1, int H2, int A) {
  return ((D + 15) >> 4) + (H1 >> 4) + (H2 >> 4) + (H1 + H2 + 2 * A + RPL_BLOCK - 1) / RPL_BLOCK + 1;
}

// The apply launch: block `blk`.  `lds`: the two staging arrays of the layer.
__device__ __forceinline__ void rpa_apply_block(const rp_actor_step_args& a, int blk, const float* ws, float* lds, const size_t member = 0) {
  float* sa = lds;
  float* sw = sa + RPL_TILE_R * RPL_S_PITCH;
  const int D = a.D, A = a.A, H1 = a.H1, H2 = a.H2, R = a.row_count, N3 = 2 * a.A;
  const RpaLayout lay = rpa_layout(H1, H2, A, R);
  const int tiles1 = (D + 15) >> 4, tiles2 = H1 >> 4, tiles3 = H2 >> 4, vblocks = (H1 + H2 + N3 + RPL_BLOCK - 1) / RPL_BLOCK;
  f32x4 acc[RPL_ACC];
  if (blk < tiles1) {   // (block-uniform, as those below)
    const int k0 = blk * 16;
    const float* ds1 = ws + lay.ds1;
    rpl_layer_of<true>(
        [&](int rr, int l) {
          if (k0 + rr >= D) return 0.f;
          return rpa_x(a, (long long)a.row_first + l, k0 + rr);
        },
        [&](int n, int l) { return ds1[(size_t)l * H1 + n]; }, R, H1, sa, sw, acc);
    const size_t base = member * rpa_elems(RP_ACTOR_W1, D, H1, H2, A);
    rpl_adam_tile(acc, k0, D, H1, [&a, base](size_t idx, float g) { rpa_step(a, RP_ACTOR_W1, base + idx, g); });
    return;
  }
  blk -= tiles1;
  if (blk < tiles2) {
    const int k0 = blk * 16;
    const float* h1 = ws + lay.h1;
    const float* ds2 = ws + lay.ds2;
    rpl_layer_of<true>([&](int rr, int l) { return h1[(size_t)l * H1 + k0 + rr]; },
                       [&](int n, int l) { return ds2[(size_t)l * H2 + n]; }, R, H2, sa, sw, acc);
    const size_t base = member * rpa_elems(RP_ACTOR_W2, D, H1, H2, A);
    rpl_adam_tile(acc, k0, H1, H2, [&a, base](size_t idx, float g) { rpa_step(a, RP_ACTOR_W2, base + idx, g); });
    return;
  }
  blk -= tiles2;
  if (blk < tiles3) {
    const int k0 = blk * 16;
    const float* h2 = ws + lay.h2;
    const float* dout = ws + lay.dout;
    rpl_layer_of<true>([&](int rr, int l) { return h2[(size_t)l * H2 + k0 + rr]; },
                       [&](int n, int l) { return dout[(size_t)l * N3 + n]; }, R, N3, sa, sw, acc);
    const size_t base = member * rpa_elems(RP_ACTOR_W3, D, H1, H2, A);
    rpl_adam_tile(acc, k0, H2, N3, [&a, base](size_t idx, float g) { rpa_step(a, RP_ACTOR_W3, base + idx, g); });
    return;
  }
  blk -= tiles3;
  if (blk < vblocks) {
    const int el = blk * RPL_BLOCK + (int)threadIdx.x;
    if (el >= H1 + H2 + N3) return;
    const float* part = ws + lay.part + el;
    float g = 0.f;
    for (int t = 0; t < lay.T; t++) g = g + part[(size_t)t * lay.V];
    int which, idx = el;
    if (idx < H1) which = RP_ACTOR_B1;
    else if ((idx -= H1) < H2) which = RP_ACTOR_B2;
    else { idx -= H2; which = RP_ACTOR_B3; }
    rpa_step(a, which, member * rpa_elems(which, D, H1, H2, A) + (size_t)idx, g);
    return;
  }
  // the temperature and the statistics: one thread
  if (threadIdx.x != 0) return;
  const float* part = ws + lay.part + (H1 + H2 + N3);
  float sl = 0.f, sg = 0.f, se = 0.f, sm = 0.f;
  for (int t = 0; t < lay.T; t++) {
    const float* pt = part + (size_t)t * lay.V;
    sl = sl + pt[0];
    sg = sg + pt[1];
    se = se + pt[2];
    sm = sm + pt[3];
  }
  const float g = -sg;
  const float before = a.log_alpha[member];
  rpl_adam_at(rpa_adam_of(a.alpha_adam), a.log_alpha + member, a.log_alpha_m + member, a.log_alpha_v + member,
           a.log_alpha_grad ? a.log_alpha_grad + member : nullptr, g);
  float* stats = a.stats + member * RP_ACTOR_STATS;
  stats[RP_ACTOR_LOSS] = sl;
  stats[RP_ACTOR_ALPHA_LOSS] = before * g;
  stats[RP_ACTOR_ALPHA] = expf(a.log_alpha[member]);
  stats[RP_ACTOR_ENTROPY] = -se;
  const float f = sm / (float)R;
  stats[RP_ACTOR_MASKED] = 1.f - f;
}

}  // namespace

#endif  // RP_ACTOR_HPP_
