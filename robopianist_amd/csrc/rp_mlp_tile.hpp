// rp_mlp_tile.hpp -- the 16-row MFMA multilayer-perceptron tile in LDS, shared by the kernels of librp_learn.so
// (rp_learn.hip: the PPO policy), of librp_sac.so (rp_sac.hip: the SAC policy and TD target), of librp_droq.so and of
// librp_pop.so (the same bodies, through rp_sac.hpp and rp_droq.hpp), and the one-wave row copy: the sampler's rows
// through rpl_copy_row, rp_learn_pack_kernel's float32 fields through its parts.
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

// One layer of the tile: acc[i] (column tile wave + 4 i) = sum over k ascending of in[row][k] W[n][k], from 0.
// `load_a(r, k)` is the input of row r, k < K.  All 256 threads call it together.
template <typename LoadA>
__device__ inline void rpl_layer(LoadA load_a, int K, const float* __restrict__ W, int N, float* sa, float* sw, f32x4 (&acc)[RPL_ACC]) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
  const int tiles = (N + 15) >> 4;
  const int w_rounds = tiles * 16 * RPL_TK / RPL_BLOCK;   // (2 per column tile)
  const int tk = tid & (RPL_TK - 1), tn = tid / RPL_TK;   // this thread's k and first row of the staged tiles
#pragma unroll
  for (int i = 0; i < RPL_ACC; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float pa[RPL_A_ROUNDS], pw[RPL_W_ROUNDS];
  auto fetch = [&](int k0) {
    const int k = k0 + tk;
#pragma unroll
    for (int i = 0; i < RPL_A_ROUNDS; i++) pa[i] = k < K ? load_a(tn + (RPL_BLOCK / RPL_TK) * i, k) : 0.f;
#pragma unroll
    for (int i = 0; i < RPL_W_ROUNDS; i++) {
      const int n = tn + (RPL_BLOCK / RPL_TK) * i;
      pw[i] = (i < w_rounds && n < N && k < K) ? W[(size_t)n * K + k] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += RPL_TK) {
#pragma unroll
    for (int i = 0; i < RPL_A_ROUNDS; i++) sa[(tn + (RPL_BLOCK / RPL_TK) * i) * RPL_S_PITCH + tk] = pa[i];
#pragma unroll
    for (int i = 0; i < RPL_W_ROUNDS; i++)
      if (i < w_rounds) sw[(tn + (RPL_BLOCK / RPL_TK) * i) * RPL_S_PITCH + tk] = pw[i];
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

// The layer's sums plus bias (through tanhf for a hidden layer) into the tile's activations, in place.
template <bool kTanh>
__device__ inline void rpl_store_layer(const f32x4 (&acc)[RPL_ACC], const float* __restrict__ b, int N, float* sh) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < RPL_ACC; i++) {
    const int n = (wave + 4 * i) * 16 + r16;
    if (n < N) {
      const float bias = b[n];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const float s = acc[i][reg] + bias;
        sh[(4 * kq + reg) * RPL_H_PITCH + n] = kTanh ? tanhf(s) : s;
      }
    }
  }
  __syncthreads();
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
