// rp_actor.hip -- librp_actor.so: the actor's and the temperature's step of DroQ (include/learn/rp_actor.h).
//
// The decomposition that ships: two launches per call.
//   rp_actor_rows_kernel   grid (tiles of 16 rows), four waves.  The policy on the tile of rp_mlp_tile.hpp (h1 and h2 go to
//                          the workspace as they are made: the critics need the tile's arrays), its epilogue keeping a, t,
//                          `inside` and logp in LDS; then the critics one after the other in the critic step's tile
//                          (rp_droq.hpp: forward with saved activations, the head, backward with dq = 1), each followed
//                          by one more transposed layer through the A action columns of its W1, whose result a row copies
//                          only if this critic's q is the smallest so far; then the head gradient and the actor's
//                          backward pass (W3 and W2 transposed through the same tile, h2 and h1 read back from the
//                          workspace).  To the workspace: h1, h2, ds1, ds2 [R][H], dout3 [R][2 A] and the tile's partial
//                          sums of the three biases and the four scalar sums.
//   rp_actor_apply_kernel  grid (ceil(D / 16) + H1 / 16 + H2 / 16 + ceil((H1 + H2 + 2 A) / 256) + 1).  A block of the first
//                          three kinds owns 16 columns of w1, w2 or w3 for all units: dW = ds^T in on
//                          v_mfma_f32_16x16x4_f32, the batch rows being the reduction (stages of 32 rows in LDS,
//                          ascending); the fourth adds the tiles' partial sums of 256 bias elements, tiles ascending; each
//                          then applies Adam to what it owns.  The last block's first thread adds the tiles' scalar sums,
//                          takes the temperature's Adam step and writes the five statistics.
// Both reductions have one order whatever the device runs at a time: there are no atomics and no block reads what another
// block of the same launch wrote.
// Resources: profiles/actor_resources.txt.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_actor.hpp"

namespace {

__global__ __launch_bounds__(RPL_BLOCK) void rp_actor_rows_kernel(const rp_actor_step_args a, const RpaCritics cs) {
  __shared__ __attribute__((aligned(16))) float lds[RPA_ROWS_LDS_FLOATS];
  rpa_rows_tile(a, cs, (int)blockIdx.x, (float*)a.workspace, lds);
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_actor_apply_kernel(const rp_actor_step_args a) {
  __shared__ __attribute__((aligned(16))) float lds[RPL_TILE_R * RPL_S_PITCH + RP_LEARN_MAX_H * RPL_S_PITCH];
  rpa_apply_block(a, (int)blockIdx.x, (const float*)a.workspace, lds);
}

}  // namespace

extern "C" {

const char* rp_actor_last_error(void) { return g_err.c_str(); }

int rp_actor_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_critics")) return RP_DROQ_MAX_CRITICS;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "stage_rows")) return RPL_TK;
  if (!strcmp(name, "launches")) return 2;
  if (!strcmp(name, "noise_counter")) return RP_ACTOR_NOISE_COUNTER;
  if (!strcmp(name, "counter")) return RP_ACTOR_COUNTER;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  if (!strcmp(name, "stats")) return RP_ACTOR_STATS;
  return -1;
}

int rp_actor_workspace(rp_actor_workspace_args* a) {
  RP_ARGS_HEAD("rp_actor_workspace", rp_actor_workspace_args);
  RP_ARGS_CHECK(rpa_check_workspace(a));
  a->bytes = rpa_workspace_bytes(a->H1, a->H2, a->A, a->row_count);
  return 0;
}

int rp_actor_step(const rp_actor_step_args* a) {
  RP_ARGS_HEAD("rp_actor_step", rp_actor_step_args);
  RP_ARGS_CHECK(rpa_check_step(a));
  if (a->row_count == 0) return 0;
  RpaCritics cs;
  memset(&cs, 0, sizeof(cs));
  for (int i = 0; i < a->n_critics; ++i) cs.c[i] = a->critics[i];
  cs.logp_const = (float)(0.5 * (double)a->A * 1.8378770664093453);   // ln 2 pi
  cs.ln2 = (float)0.6931471805599453;
  const RpaLayout lay = rpa_layout(a->H1, a->H2, a->A, a->row_count);
  const hipStream_t stream = (hipStream_t)a->hip_stream;
  if (a->launches != RP_ACTOR_APPLY_ONLY) {
    hipLaunchKernelGGL(rp_actor_rows_kernel, dim3((unsigned)lay.T), dim3(RPL_BLOCK), 0, stream, *a, cs);
    HIP_OK(hipGetLastError());
  }
  if (a->launches == RP_ACTOR_ROWS_ONLY) return 0;
  const unsigned blocks = (unsigned)rpa_apply_blocks(a->D, a->H1, a->H2, a->A);
  hipLaunchKernelGGL(rp_actor_apply_kernel, dim3(blocks), dim3(RPL_BLOCK), 0, stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
