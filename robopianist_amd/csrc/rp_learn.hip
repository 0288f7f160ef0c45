// rp_learn.hip -- librp_learn.so: the kernels of the on-device PPO learner (include/learn/rp_learn.h).
//
// One launch per call:
//   rp_learn_pack_kernel     grid (row, field + 1), one wave: field f of the TimeStep into its columns of the slot's obs
//                            row, cast to float32, in the widest unit both rows allow after a head of single elements; the last y index is the
//                            row's step type, reward, discount and episode statistics (lane 0).
//   rp_learn_act_kernel      the fused policy: grid (row tile, network), four waves.  A workgroup owns RPL_TILE_R = 16
//                            rows of ONE network (the actor or the critic), so 4096 rows are 256 tiles x 2 networks =
//                            512 workgroups on 256 CUs.  The three layers run on v_mfma_f32_16x16x4_f32 with the operand
//                            maps of rp_hear.hip's analysis GEMM (A[lane & 15][lane >> 4], B[lane >> 4][lane & 15], C/D
//                            column = lane & 15, row = 4 (lane >> 4) + register); wave w owns the column tiles w, w + 4,
//                            w + 8, w + 12 (four accumulators at 256 outputs).  Both operands go through LDS RPL_TK = 32
//                            k at a time -- the normalised input (layer 1) or the previous activations, and the rows
//                            [out][k .. k + 32) of the weight matrix as torch keeps it -- with the next stage's global
//                            loads in flight under the current stage's MFMAs.  The activations of the tile stay in LDS
//                            ([16][RPL_H_PITCH], overwritten in place once a layer's sums are complete); nothing
//                            intermediate goes to global memory.  The epilogue draws the planner's noise.
//                            Resources of the shipped binary (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see
//                            the table under the kernel.
//   rp_learn_gae_kernel      one thread per env, backwards over the slots, float64.
//   rp_learn_moments_kernel  grid (column block of 16): 16 columns x 16 partial sums per workgroup, two passes (sum, then
//                            squared deviations), lanes reduced through LDS in ascending order, merged by Chan's formula.
//                            Its body is rpl_moments_block of rp_learn.hpp, which librp_pop.so runs per member too.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_learn.hpp"
#include "rp_mlp_tile.hpp"

namespace {

// ---- pack ------------------------------------------------------------------------------------------------------------
struct RplField {
  const void* src;
  int width, dtype, off, pad_;
};
struct RplFieldTable {
  RplField f[RP_LEARN_MAX_FIELDS];
};

template <typename T>
__device__ inline void rpl_pack_meta(const rp_learn_pack_args& a, long long e) {
  const int st = a.step_type[e];
  const T r = a.reward ? static_cast<const T*>(a.reward)[e] : (T)0;
  const T d = a.discount ? static_cast<const T*>(a.discount)[e] : (T)1;
  a.slot_step_type[e] = st;
  a.slot_reward[e] = (float)r;
  a.slot_discount[e] = (float)d;
  if (!a.ep_return) return;
  if (st == RP_LEARN_STEP_FIRST) {
    a.ep_return[e] = 0.0;
    a.ep_len[e] = 0;
    return;
  }
  const double ret = a.ep_return[e] + (double)r;
  const int len = a.ep_len[e] + 1;
  a.ep_return[e] = ret;
  a.ep_len[e] = len;
  if (st == RP_LEARN_STEP_LAST) {
    const double dr = a.done_return[e] + ret;
    a.done_return[e] = dr;
    a.done_len[e] = a.done_len[e] + len;
    a.done_count[e] = a.done_count[e] + 1;
  }
}

__global__ __launch_bounds__(RPL_WAVE) void rp_learn_pack_kernel(const RplFieldTable tab, const rp_learn_pack_args a) {
  const long long e = (long long)a.env_first + blockIdx.x;
  if ((int)blockIdx.y == a.n_fields) {
    if (threadIdx.x == 0) {
      if (a.precision == 32) rpl_pack_meta<float>(a, e);
      else rpl_pack_meta<double>(a, e);
    }
    return;
  }
  const RplField f = tab.f[blockIdx.y];
  float* d = a.obs + e * a.D + f.off;
  const uintptr_t da = reinterpret_cast<uintptr_t>(d);
  const int lane = (int)threadIdx.x;
  if (f.dtype == RP_LEARN_F32) {
    // rows whose addresses agree modulo 16 (or 8) bytes: single floats up to the first 16- (8-) byte boundary, whole
    // units from there, single floats for the rest (rpl_copy_row of rp_mlp_tile.hpp, written out: through the call
    // the kernel is two instructions longer)
    const float* s = static_cast<const float*>(f.src) + e * f.width;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s);
    int head = 0, done = 0;
    if (((sa ^ da) & 15) == 0) {
      head = rpl_head(sa, 16, f.width);
      done = rpl_copy_units<uint4>(s, d, head, f.width);
    } else if (((sa ^ da) & 7) == 0) {
      head = rpl_head(sa, 8, f.width);
      done = rpl_copy_units<uint2>(s, d, head, f.width);
    }
    if (lane < head) d[lane] = s[lane];                                          // (head <= 3)
    for (int i = done + lane; i < f.width; i += RPL_WAVE) d[i] = s[i];           // (the tail: < 4 floats, or all)
  } else {
    // pairs: two float64 (16 bytes) into two float32 (8 bytes), after one single element where that aligns both rows
    const double* s = static_cast<const double*>(f.src) + e * f.width;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(s);
    int head = 0, done = 0;
    const bool s_off = (sa & 15) != 0, d_off = (da & 7) != 0;
    if (s_off == d_off) {
      head = s_off && f.width > 0 ? 1 : 0;
      const int n = (f.width - head) / 2;
      const double2* s2 = reinterpret_cast<const double2*>(s + head);
      float2* d2 = reinterpret_cast<float2*>(d + head);
      for (int i = lane; i < n; i += RPL_WAVE) {
        const double2 v = s2[i];
        d2[i] = make_float2((float)v.x, (float)v.y);
      }
      done = head + 2 * n;
    }
    if (lane < head) d[lane] = (float)s[lane];
    for (int i = done + lane; i < f.width; i += RPL_WAVE) d[i] = (float)s[i];
  }
}

// ---- act -------------------------------------------------------------------------------------------------------------
struct RplNets {
  rp_learn_mlp net[2];
  int is_actor[2];
  float logp_const;   // (float)(0.5 A ln 2 pi)
};

// (rpl_layer and rpl_store_layer, one layer of the tile and its store, are rp_mlp_tile.hpp's: librp_sac.so runs them too)
// Row tile: 16 rows per workgroup and one network per workgroup, so 4096 rows launch 256 x 2 = 512 workgroups, two per
// CU of the 256.  Resources (gfx950, -O3 -ffp-contract=on, the compiler's kernel-resource-usage remark for this binary):
//     VGPRs 178 + AGPRs 16 = 194 of the unified file -> 2 waves per SIMD, i.e. two 4-wave workgroups per CU
//     SGPRs 106 (204 spilled to VGPR lanes: the argument block and the six weight pointers), scratch 0 bytes per lane
//     LDS 53,632 bytes per workgroup, static (2,176 input stage + 34,816 weight stage + 16,640 activations): three
//     workgroups would fit the 160 KiB of a CU, the registers admit two
// so all 512 workgroups of a 4096-row launch are resident at once.  Measured: 237 us per launch at 4096 rows, D = 1130,
// 256 x 256 hidden units, 45 actions (profiles/learn_bench.json); by count (1,472 MFMAs of 32 cycles per wave) the matrix
// pipe is busy for about 40 us of it at two workgroups per CU; the rest is the latency of the staged loads, which one
// stage of prefetch does not cover.
__global__ __launch_bounds__(RPL_BLOCK) void rp_learn_act_kernel(const rp_learn_act_args a, const RplNets nets) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];        // the staged input: [row][k]
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];    // the staged weights: [out][k]; the epilogue's log-probability terms
  __shared__ float sh[RPL_TILE_R * RPL_H_PITCH];        // the tile's activations: [row][unit]
  const int tid = (int)threadIdx.x;
  const rp_learn_mlp net = nets.net[blockIdx.y];
  const bool is_actor = nets.is_actor[blockIdx.y] != 0;
  const int N3 = is_actor ? a.A : 1;
  const long long e0 = (long long)a.row_first + (long long)blockIdx.x * RPL_TILE_R;
  const long long e_end = (long long)a.row_first + a.row_count;
  f32x4 acc[RPL_ACC];
  rpl_layer(
      [&](int r, int k) {
        const long long e = e0 + r;
        if (e >= e_end) return 0.f;
        return rpl_xn(a.obs, a.mean, a.inv_std, a.obs_clip, e, a.D, k);
      },
      a.D, net.w1, a.H1, sa, sw, acc);
  rpl_store_layer<true>(acc, net.b1, a.H1, sh);
  rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, net.w2, a.H2, sa, sw, acc);
  rpl_store_layer<true>(acc, net.b2, a.H2, sh);
  rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H2, net.w3, N3, sa, sw, acc);
  rpl_store_layer<false>(acc, net.b3, N3, sh);
  if (!is_actor) {   // (block-uniform)
    if (tid < RPL_TILE_R && e0 + tid < e_end) a.value[e0 + tid] = sh[tid * RPL_H_PITCH];
    return;
  }
  const int A = a.A;
  float* sg = sw;   // [row][RP_LEARN_MAX_A]: the terms of the log-probability (the weight stage is dead)
  for (int idx = tid; idx < RPL_TILE_R * A; idx += RPL_BLOCK) {
    const int r = idx / A, u = idx - r * A;
    const long long e = e0 + r;
    if (e >= e_end) continue;
    const float mu = sh[r * RPL_H_PITCH + u];
    float act = mu;
    if (!a.deterministic) {
      const float zf = (float)rppl_z(a.seed_lo, a.seed_hi, a.round, (uint32_t)e, (uint32_t)u);
      const float ls = a.log_std[u];
      const float sd = expf(ls);
      const float t = sd * zf;
      act = mu + t;
      const float q = zf * zf;
      const float h = -0.5f * q;
      sg[r * RP_LEARN_MAX_A + u] = h - ls;
    }
    const size_t o = (size_t)e * A + u;
    a.action[o] = act;
    if (a.mu) a.mu[o] = mu;
    const float lo = fmaxf(act, -1.f);
    const float env = fminf(lo, 1.f);
    if (a.precision == 32) static_cast<float*>(a.env_action)[o] = env;
    else static_cast<double*>(a.env_action)[o] = (double)env;
  }
  if (a.deterministic) return;   // (block-uniform)
  __syncthreads();
  if (tid < RPL_TILE_R && e0 + tid < e_end) {
    float s = 0.f;
    for (int u = 0; u < A; u++) s = s + sg[tid * RP_LEARN_MAX_A + u];
    a.logp[e0 + tid] = s - nets.logp_const;
  }
}

// ---- gae -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RPL_BLOCK) void rp_learn_gae_kernel(const rp_learn_gae_args a) {
  const long long idx = (long long)blockIdx.x * RPL_BLOCK + threadIdx.x;
  if (idx >= a.env_count) return;
  const long long e = (long long)a.env_first + idx, E = a.E;
  double carry = 0.0;
  int st_next = a.step_type[(long long)a.T * E + e];
  double v_next = (double)a.value[(long long)a.T * E + e];
  for (int t = a.T - 1; t >= 0; --t) {
    const long long i = (long long)t * E + e;
    const int st = a.step_type[i];
    const double v = (double)a.value[i];
    double A = 0.0;
    unsigned char valid = 0;
    if (st != RP_LEARN_STEP_LAST && st_next != RP_LEARN_STEP_FIRST) {
      const double r = (double)a.reward[i + E], d = (double)a.discount[i + E];
      const double nv = a.gamma * d;
      const double tv = nv * v_next;
      const double s = r + tv;
      const double delta = s - v;
      const double gl = nv * a.lambda;
      const double c = gl * carry;
      A = delta + c;
      valid = 1;
    }
    const double rt = A + v;
    a.adv[i] = (float)A;
    a.ret[i] = (float)rt;
    a.valid[i] = valid;
    carry = A;
    st_next = st;
    v_next = v;
  }
}

// ---- moments ---------------------------------------------------------------------------------------------------------
// The body is rp_learn.hpp's, on the identity map.
__global__ __launch_bounds__(RPL_MOMENT_COLS * RPL_MOMENT_LANES) void rp_learn_moments_kernel(const rp_learn_moments_args a) {
  __shared__ double part[RPL_MOMENT_LANES][RPL_MOMENT_COLS];
  rpl_moments_block(a, RplRowIdentity{}, part);
}

}  // namespace

extern "C" {

const char* rp_learn_last_error(void) { return g_err.c_str(); }

int rp_learn_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_fields")) return RP_LEARN_MAX_FIELDS;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "min_hidden")) return 16;
  if (!strcmp(name, "hidden_multiple")) return 16;
  if (!strcmp(name, "max_actions")) return RP_LEARN_MAX_A;
  if (!strcmp(name, "min_obs")) return 1;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "moment_lanes")) return RPL_MOMENT_LANES;
  return -1;
}

int rp_learn_pack(const rp_learn_pack_args* a) {
  RP_ARGS_HEAD("rp_learn_pack", rp_learn_pack_args);
  RP_ARGS_CHECK(rpl_check_pack(a));
  if (a->env_count == 0) return 0;
  RplFieldTable tab;
  memset(&tab, 0, sizeof(tab));
  int off = 0;
  for (int i = 0; i < a->n_fields; ++i) {
    tab.f[i].src = a->fields[i].src;
    tab.f[i].width = a->fields[i].width;
    tab.f[i].dtype = a->fields[i].dtype;
    tab.f[i].off = off;
    off += a->fields[i].width;
  }
  // the row is the grid's x index (< 2^31), the field the y index (<= 65)
  hipLaunchKernelGGL(rp_learn_pack_kernel, dim3((unsigned)a->env_count, (unsigned)a->n_fields + 1), dim3(RPL_WAVE), 0,
                     (hipStream_t)a->hip_stream, tab, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_learn_act(const rp_learn_act_args* a) {
  RP_ARGS_HEAD("rp_learn_act", rp_learn_act_args);
  RP_ARGS_CHECK(rpl_check_act(a));
  if (a->row_count == 0) return 0;
  RplNets nets;
  memset(&nets, 0, sizeof(nets));
  int n = 0;
  if (a->actor) { nets.net[n] = *a->actor; nets.is_actor[n] = 1; ++n; }
  if (a->critic) { nets.net[n] = *a->critic; nets.is_actor[n] = 0; ++n; }
  nets.logp_const = (float)(0.5 * (double)a->A * 1.8378770664093453);   // ln 2 pi
  hipLaunchKernelGGL(rp_learn_act_kernel, dim3(blocks_for(a->row_count, RPL_TILE_R), (unsigned)n), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, *a, nets);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_learn_gae(const rp_learn_gae_args* a) {
  RP_ARGS_HEAD("rp_learn_gae", rp_learn_gae_args);
  RP_ARGS_CHECK(rpl_check_gae(a));
  if (a->env_count == 0) return 0;
  hipLaunchKernelGGL(rp_learn_gae_kernel, dim3(blocks_for(a->env_count, RPL_BLOCK)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_learn_moments(const rp_learn_moments_args* a) {
  RP_ARGS_HEAD("rp_learn_moments", rp_learn_moments_args);
  RP_ARGS_CHECK(rpl_check_moments(a));
  hipLaunchKernelGGL(rp_learn_moments_kernel, dim3(blocks_for(a->D, RPL_MOMENT_COLS)), dim3(RPL_MOMENT_COLS * RPL_MOMENT_LANES),
                     0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
