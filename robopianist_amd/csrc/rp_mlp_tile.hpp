// rp_mlp_tile.hpp -- the 16-row MFMA multilayer-perceptron tile in LDS, shared by the kernels of librp_learn.so
// (rp_learn.hip: the PPO policy), of librp_sac.so (rp_sac.hip: the SAC policy and TD target), of librp_droq.so and of
// librp_pop.so (the same bodies, through rp_sac.hpp and rp_droq.hpp), of librp_critic.so, librp_pop_critic.so and
// librp_actor.so (rp_critic.hpp, rp_actor.hpp), and the one-wave row copy: the sampler's rows through rpl_copy_row,
// rp_learn_pack_kernel's float32 fields through its parts.
//
// This is the one home of the tile's primitives: the layer (rpl_layer_of, with loaders for both operands; rpl_layer, the
// forward form on W [N][K]), its store (rpl_store_layer), the normalised observation read (rpl_xn, rpl_xn_action), the
// mask sum of the masked means (rpl_mask_sum), the squashed Gaussian's per-unit term (rpl_logp_term) and Adam (rpl_adam,
// rpl_polyak, rpl_adam_tile).
//
// A workgroup of RPL_BLOCK = 256 threads (four waves) owns RPL_TILE_R = 16 rows.  A layer runs on
// v_mfma_f32_16x16x4_f32; both operands go through LDS RPL_TK = 32 k at a time (the caller's `sa` [16][RPL_S_PITCH] and
// `sw` [RP_LEARN_MAX_H][RPL_S_PITCH]), the activations stay in the caller's `sh` [16][RPL_H_PITCH].  The operand maps and
// the staging are described at the head of rp_learn.hip.  The routines are device code with internal linkage: each
// library compiles its own copy from this one text.
#ifndef RP_MLP_TILE_HPP_
#define RP_MLP_TILE_HPP_

#include <hip/hip_runtime.h>

#include "rp_learn.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RPL_MAX_TILES (RP_LEARN_MAX_H / 16)                 // column tiles of a layer
#define RPL_ACC (RPL_MAX_TILES / 4)                         // accumulators per wave
#define RPL_W_ROUNDS (RP_LEARN_MAX_H * RPL_TK / RPL_BLOCK)  // weight values per thread and stage at 256 outputs
#define RPL_A_ROUNDS (RPL_TILE_R * RPL_TK / RPL_BLOCK)

// One layer of the tile: acc[i] (column tile wave + 4 i) = the chain over k ascending, from 0, of load_a(r, k) load_w(n, k).
// `load_a(r, k)` is the input of row r, `load_w(n, k)` the weight of output n, k < K.  kColFast says which index is
// consecutive in memory and so which one the staging threads run along: k (false: the forward layers, W [N][K]) or r and
// n (true: a transposed W, and the parameter gradients, whose k is the batch row).  All 256 threads call it together.
template <bool kColFast, typename LoadA, typename LoadW>
__device__ inline void rpl_layer_of(LoadA load_a, LoadW load_w, int K, int N, float* sa, float* sw, f32x4 (&acc)[RPL_ACC]) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  const int tiles = (N + 15) >> 4;
  const int w_rounds = tiles * 16 * RPL_TK / RPL_BLOCK;   // (2 per column tile)
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

// The forward layer on the matrix W [N][K] as torch keeps it.
template <typename LoadA>
__device__ inline void rpl_layer(LoadA load_a, int K, const float* __restrict__ W, int N, float* sa, float* sw, f32x4 (&acc)[RPL_ACC]) {
  rpl_layer_of<false>(load_a, [W, K](int n, int k) { return W[(size_t)n * K + k]; }, K, N, sa, sw, acc);
}

// The layer's sums plus bias (kBias false, `b` NULL: the sums as they are; kTanh: through tanhf, a hidden layer) into the
// tile's array `sh`, in place; ends with a barrier.
template <bool kTanh, bool kBias = true>
__device__ inline void rpl_store_layer(const f32x4 (&acc)[RPL_ACC], const float* __restrict__ b, int N, float* sh) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < RPL_ACC; i++) {
    const int n = (wave + 4 * i) * 16 + r16;
    if (n < N) {
      const float bias = kBias ? b[n] : 0.f;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const float s = kBias ? acc[i][reg] + bias : acc[i][reg];
        sh[(4 * kq + reg) * RPL_H_PITCH + n] = kTanh ? tanhf(s) : s;
      }
    }
  }
  __syncthreads();
}

// xn: column k < D of row e of `obs` [.][D], normalised and clipped as it is read.
__device__ inline float rpl_xn(const float* __restrict__ obs, const float* __restrict__ mean, const float* __restrict__ inv_std,
                               float clip, long long e, int D, int k) {
  const float x = obs[(size_t)e * D + k];
  const float d = x - mean[k];
  const float p = d * inv_std[k];
  const float lo = fmaxf(p, -clip);
  return fminf(lo, clip);
}

// Column k < D + A of cat([xn(obs), action]) of row e: a critic's input.
__device__ inline float rpl_xn_action(const float* __restrict__ obs, const float* __restrict__ action, const float* __restrict__ mean,
                                      const float* __restrict__ inv_std, float clip, long long e, int D, int A, int k) {
  if (k >= D) return action[(size_t)e * A + (k - D)];
  return rpl_xn(obs, mean, inv_std, clip, e, D, k);
}

// max(the sum of mask[0 .. R), 1): a strided sum per thread, then the halving tree in `red` (RPL_BLOCK floats of LDS).
// All 256 threads call it together; it ends with a barrier.
__device__ inline float rpl_mask_sum(const float* __restrict__ mask, int R, float* red) {
  const int tid = (int)threadIdx.x;
  float pm = 0.f;
  for (int l = tid; l < R; l += RPL_BLOCK) pm = pm + mask[l];
  red[tid] = pm;
  __syncthreads();
  for (int s = RPL_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const float M = fmaxf(red[0], 1.f);
  __syncthreads();
  return M;
}

// The term of unit u in the squashed Gaussian's log-probability (rp_sac.h's statements): the pre-activation p = m + t, the
// noise zf, the clamped log std ls; `ln2`: (float)ln 2.  For rp_sac.hpp's policy and the actor step (rp_actor.hpp).
__device__ inline float rpl_logp_term(float p, float zf, float ls, float ln2) {
  const float w = -2.f * p;
  const float aw = fabsf(w);
  const float ex = expf(-aw);
  const float l1 = log1pf(ex);
  const float wp = fmaxf(w, 0.f);
  const float sp = wp + l1;
  const float c1 = ln2 - p;
  const float c2 = c1 - sp;
  const float lg = 2.f * c2;
  const float q = zf * zf;
  const float h = -0.5f * q;
  const float g0 = h - ls;
  return g0 - lg;
}

// ---- Adam --------------------------------------------------------------------------------------------------------------
struct RplAdam {   // one optimiser's scalars at its step count (rp_critic.h)
  float one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
};

// Adam's statements (rp_critic.h) on one element's values: the gradient g moves the moments m and v and the parameter p.
__device__ inline void rpl_adam(const RplAdam& o, float g, float& m, float& v, float& p) {
  float x = g - m;
  x = x * o.one_minus_beta1;
  m = m + x;
  float c = g * o.one_minus_beta2;
  c = c * g;
  v = v * o.beta2;
  v = v + c;
  float den = sqrtf(v);
  den = den / o.bc2_sqrt;
  den = den + o.eps;
  float u = m / den;
  u = u * o.step_size;
  p = p - u;
}

// The same on an element in memory; the gradient to `pg` if given.
__device__ inline void rpl_adam_at(const RplAdam& o, float* pp, float* pm, float* pv, float* pg, float g) {
  if (pg) *pg = g;
  float m = *pm, v = *pv, p = *pp;
  rpl_adam(o, g, m, v, p);
  *pm = m;
  *pv = v;
  *pp = p;
}

// The Polyak step of a target parameter t towards p.  -> the new target parameter.
__device__ inline float rpl_polyak(float t, float p, float tau) {
  float w = p - t;
  w = w * tau;
  t = t + w;
  return t;
}

// The 16 x N tile of the gradient of a matrix [N][K] that `acc` holds: row 4 kq + reg is column k0 + .. of the matrix, the
// accumulator's column its row n.  Calls step(n K + k, g) on every element inside the matrix.
// (__forceinline__, and `step` capturing its scalars by value: as `inline` with a by-reference lambda leaves it, the apply
// kernels recompute the tensors' addresses per element.)
template <typename Step>
__device__ __forceinline__ void rpl_adam_tile(const f32x4 (&acc)[RPL_ACC], int k0, int K, int N, Step step) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < RPL_ACC; t++) {
    const int n = (wave + 4 * t) * 16 + r16;
    if (n < N) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int k = k0 + 4 * kq + reg;
        if (k < K) step((size_t)n * K + k, acc[t][reg]);
      }
    }
  }
}

// ---- the aligned row copy of one wave (RPL_WAVE lanes): the sampler's rows, and the parts of the pack kernel's copy ------
// Copies floats [from, width) of a row in units of U (whole units only); returns the first float it left.
template <typename U>
__device__ inline int rpl_copy_units(const float* s, float* d, int from, int width) {
  constexpr int per = (int)(sizeof(U) / sizeof(float));
  const int n = (width - from) / per;
  const U* su = reinterpret_cast<const U*>(s + from);
  U* du = reinterpret_cast<U*>(d + from);
  for (int i = threadIdx.x; i < n; i += RPL_WAVE) du[i] = su[i];
  return from + n * per;
}

// The floats in front of the first address that is a multiple of `unit` bytes (a is 4-aligned), at most `width`.
__device__ inline int rpl_head(uintptr_t a, int unit, int width) {
  const int h = (int)(((uintptr_t)unit - (a & (uintptr_t)(unit - 1))) & (uintptr_t)(unit - 1)) >> 2;
  return h < width ? h : width;
}

// Copies the `width` floats of row s into row d: where the two addresses agree modulo 16 (8) bytes, single floats up to
// the first 16- (8-) byte boundary, whole units from there, single floats for the rest.
__device__ inline void rpl_copy_row(const float* s, float* d, int width) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
  const int lane = (int)threadIdx.x;
  int head = 0, done = 0;
  if (((sa ^ da) & 15) == 0) {
    head = rpl_head(sa, 16, width);
    done = rpl_copy_units<uint4>(s, d, head, width);
  } else if (((sa ^ da) & 7) == 0) {
    head = rpl_head(sa, 8, width);
    done = rpl_copy_units<uint2>(s, d, head, width);
  }
  if (lane < head) d[lane] = s[lane];                                     // (head <= 3)
  for (int i = done + lane; i < width; i += RPL_WAVE) d[i] = s[i];        // (the tail: < 4 floats, or all)
}

}  // namespace

#endif  // RP_MLP_TILE_HPP_
