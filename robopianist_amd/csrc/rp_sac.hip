// rp_sac.hip -- librp_sac.so: the kernels of the on-device off-policy learner (include/learn/rp_sac.h).
//
// One launch per call:
//   rp_sac_sample_kernel   grid (row), one wave: the wave draws up to RP_SAC_SAMPLE_TRIES transitions (every lane the
//                          same Philox words and the same two step types: wave-uniform), then copies the winner's two obs
//                          rows and its action row out of the ring in the widest unit both rows allow (rpl_copy_row of
//                          rp_mlp_tile.hpp, rp_learn_pack_kernel's); a row without a valid attempt is zeroed.
//   rp_sac_act_kernel      grid (row tile), four waves: the tile of rp_mlp_tile.hpp on the actor D -> H1 -> H2 -> 2 A, then
//                          the squashed Gaussian's epilogue with the planner's noise.
//   rp_sac_target_kernel   grid (row tile), four waves: the same tile on each target critic in turn, the first layer
//                          reading cat([normalised next obs, action]); the running minimum of the tile's 16 rows stays
//                          in LDS, so the ensemble needs neither atomics nor a second launch.
// The bodies of sample and act are device functions of rp_sac.hpp (rps_sample_row, rps_act_tile), which librp_pop.so runs
// on a member's rows too; the kernels here call them with the identity map.
// Resources (gfx950, -O3 -ffp-contract=on, the compiler's kernel-resource-usage remark): sample 14 VGPRs, no LDS; act
// 178 VGPRs + 16 AGPRs, 0 scratch, 53,632 bytes of LDS (rp_learn_act_kernel's figures: two workgroups per CU); target 256
// VGPRs + 72 AGPRs, 0 scratch, 53,696 bytes (the learner's three arrays and 64 bytes of minima): one workgroup per CU,
// which is what the 256 tiles of a 4096-row batch occupy anyway.  Measured at 4096 rows, D = 1130, 256 x 256 hidden units,
// 45 actions, two critics (profiles/sac_bench.json): sample 20.6 us, act + target 660 us.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_sac.hpp"
#include "rp_mlp_tile.hpp"

namespace {

// ---- sample and act: the bodies are rp_sac.hpp's, on the identity map ------------------------------------------------
__global__ __launch_bounds__(RPL_WAVE) void rp_sac_sample_kernel(const rp_sac_sample_args a) {
  rps_sample_row(a, (long long)a.row_first + blockIdx.x, RpsEnvsAll{a.E});
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_sac_act_kernel(const rp_sac_act_args a, const RpsActor actor) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];        // the staged input: [row][k]
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];    // the staged weights: [out][k]; the epilogue's log-probability terms
  __shared__ float sh[RPL_TILE_R * RPL_H_PITCH];        // the tile's activations: [row][unit]
  rps_act_tile(a, actor, RplRowIdentity{}, (long long)a.row_first + (long long)blockIdx.x * RPL_TILE_R,
               (long long)a.row_first + a.row_count, sa, sw, sh);
}

// ---- target ----------------------------------------------------------------------------------------------------------
struct RpsCritics {
  rp_learn_mlp net[RP_SAC_MAX_CRITICS];
};

__global__ __launch_bounds__(RPL_BLOCK) void rp_sac_target_kernel(const rp_sac_target_args a, const RpsCritics critics) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];
  __shared__ float sh[RPL_TILE_R * RPL_H_PITCH];
  __shared__ float sq[RPL_TILE_R];                      // the running minimum over the critics, per row
  const int tid = (int)threadIdx.x;
  const int D = a.D, A = a.A;
  const long long e0 = (long long)a.row_first + (long long)blockIdx.x * RPL_TILE_R;
  const long long e_end = (long long)a.row_first + a.row_count;
  f32x4 acc[RPL_ACC];
#pragma unroll 1
  for (int i = 0; i < a.n_critics; ++i) {   // (block-uniform)
    const rp_learn_mlp net = critics.net[i];
    rpl_layer(
        [&](int r, int k) {
          const long long e = e0 + r;
          if (e >= e_end) return 0.f;
          return rpl_xn_action(a.next_obs, a.action, a.mean, a.inv_std, a.obs_clip, e, D, A, k);
        },
        D + A, net.w1, a.H1, sa, sw, acc);
    rpl_store_layer<true>(acc, net.b1, a.H1, sh);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, net.w2, a.H2, sa, sw, acc);
    rpl_store_layer<true>(acc, net.b2, a.H2, sh);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H2, net.w3, 1, sa, sw, acc);
    rpl_store_layer<false>(acc, net.b3, 1, sh);
    // (thread r alone reads and writes sq[r]; sh[r][0] is rewritten only behind the next layers' barriers)
    if (tid < RPL_TILE_R) {
      const float q = sh[tid * RPL_H_PITCH];
      sq[tid] = i == 0 ? q : fminf(sq[tid], q);
    }
  }
  if (tid < RPL_TILE_R && e0 + tid < e_end) {
    const long long e = e0 + tid;
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

extern "C" {

const char* rp_sac_last_error(void) { return g_err.c_str(); }

int rp_sac_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_critics")) return RP_SAC_MAX_CRITICS;
  if (!strcmp(name, "sample_tries")) return RP_SAC_SAMPLE_TRIES;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  return -1;
}

int rp_sac_sample(const rp_sac_sample_args* a) {
  RP_ARGS_HEAD("rp_sac_sample", rp_sac_sample_args);
  RP_ARGS_CHECK(rps_check_sample(a));
  if (a->row_count == 0) return 0;
  hipLaunchKernelGGL(rp_sac_sample_kernel, dim3((unsigned)a->row_count), dim3(RPL_WAVE), 0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_sac_act(const rp_sac_act_args* a) {
  RP_ARGS_HEAD("rp_sac_act", rp_sac_act_args);
  RP_ARGS_CHECK(rps_check_act(a));
  if (a->row_count == 0) return 0;
  RpsActor actor;
  memset(&actor, 0, sizeof(actor));
  actor.net = *a->actor;
  actor.logp_const = (float)(0.5 * (double)a->A * 1.8378770664093453);   // ln 2 pi
  actor.ln2 = (float)0.6931471805599453;
  hipLaunchKernelGGL(rp_sac_act_kernel, dim3(blocks_for(a->row_count, RPL_TILE_R)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, *a, actor);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_sac_target(const rp_sac_target_args* a) {
  RP_ARGS_HEAD("rp_sac_target", rp_sac_target_args);
  RP_ARGS_CHECK(rps_check_target(a));
  if (a->row_count == 0) return 0;
  RpsCritics critics;
  memset(&critics, 0, sizeof(critics));
  for (int i = 0; i < a->n_critics; ++i) critics.net[i] = a->critics[i];
  hipLaunchKernelGGL(rp_sac_target_kernel, dim3(blocks_for(a->row_count, RPL_TILE_R)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, *a, critics);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
