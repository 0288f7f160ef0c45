// rp_critic.hip -- librp_critic.so: one critic step of DroQ (include/learn/rp_critic.h).
//
// The decomposition that ships: two launches per call, both with the critics side by side in grid.y.
//   rp_critic_rows_kernel   grid (tiles of 16 rows, critics), four waves.  The tile of rp_mlp_tile.hpp, the critic of
//                           rp_droq.hpp (rpd_critic_forward, rpd_critic_backward, which the actor step runs too):
//                           layer 1 and layer 2 forward, each followed by a row epilogue that keeps what the backward pass needs -- the output and the normalised value in LDS, 1 / sigma
//                           and the keep mask (16 bits: the lane's units) in registers of the sixteen lanes that own the
//                           row.  The head is a row sum over those lanes.  Backward: layer 2's row pass, W2 transposed
//                           through the same tile (staged along its contiguous index), layer 1's row pass.  Five [16][260]
//                           arrays hold sums / gradients, out1, o1, out2, o2; a row pass rewrites `out` with dz and the
//                           gradient array with ds, so the column sums of the vector parameters (thread n: rows 0 .. 15
//                           ascending) read LDS only.  To the workspace: ds1, out1, ds2 [R][H] and the tile's partial sums.
//   rp_critic_apply_kernel  grid (ceil((D + A) / 16) + H1 / 16 + ceil(V / 256), critics).  A block of the first kind owns
//                           the columns k0 .. k0 + 15 of w1 for all H1 units: dW1 = ds1^T x on v_mfma_f32_16x16x4_f32, the
//                           batch rows being the reduction (stages of 32 rows in LDS, ascending; x read from obs / action
//                           and normalised in place); the second kind does the same for w2 from ds2 and out1; the third
//                           adds the tiles' partial sums of 256 vector elements, tiles ascending.  Each then applies Adam
//                           and the Polyak step to what it owns, straight from the accumulators: no gradient is stored
//                           unless the caller gave a pointer for it.
// Both reductions have one order whatever the device runs at a time: there are no atomics and no block reads what another
// block of the same launch wrote.
// Resources: profiles/critic_resources.txt.  Measured times: DESIGN 6m (profiles/critic_bench.json).
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_critic.hpp"

namespace {

__global__ __launch_bounds__(RPL_BLOCK) void rp_critic_rows_kernel(const rp_critic_step_args a, const RpcSets sets) {
  __shared__ __attribute__((aligned(16))) float lds[RPC_ROWS_LDS_FLOATS];
  rpc_rows_tile(a, sets, (int)blockIdx.x, (int)blockIdx.y, (float*)a.workspace, lds);
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_critic_apply_kernel(const rp_critic_step_args a, const RpcSets sets) {
  __shared__ __attribute__((aligned(16))) float lds[RPL_TILE_R * RPL_S_PITCH + RP_LEARN_MAX_H * RPL_S_PITCH];
  rpc_apply_block(a, sets, (int)blockIdx.x, (int)blockIdx.y, (const float*)a.workspace, lds);
}

}  // namespace

extern "C" {

const char* rp_critic_last_error(void) { return g_err.c_str(); }

int rp_critic_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_critics")) return RP_DROQ_MAX_CRITICS;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "stage_rows")) return RPL_TK;
  if (!strcmp(name, "launches")) return 2;
  if (!strcmp(name, "counter")) return RP_CRITIC_COUNTER;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  return -1;
}

int rp_critic_workspace(rp_critic_workspace_args* a) {
  RP_ARGS_HEAD("rp_critic_workspace", rp_critic_workspace_args);
  RP_ARGS_CHECK(rpc_check_workspace(a));
  a->bytes = rpc_workspace_bytes(a->n_critics, a->H1, a->H2, a->row_count);
  return 0;
}

int rp_critic_step(const rp_critic_step_args* a) {
  RP_ARGS_HEAD("rp_critic_step", rp_critic_step_args);
  RP_ARGS_CHECK(rpc_check_step(a));
  if (a->row_count == 0) return 0;
  RpcSets sets;
  memset(&sets, 0, sizeof(sets));
  for (int i = 0; i < a->n_critics; ++i) {
    sets.p[i] = a->p[i];
    sets.m[i] = a->m[i];
    sets.v[i] = a->v[i];
    sets.t[i] = a->target[i];
    if (a->grad) sets.g[i] = a->grad[i];
  }
  const RpcLayout lay = rpc_layout(a->H1, a->H2, a->row_count);
  const hipStream_t stream = (hipStream_t)a->hip_stream;
  if (a->launches != RP_CRITIC_APPLY_ONLY) {
    hipLaunchKernelGGL(rp_critic_rows_kernel, dim3((unsigned)lay.T, (unsigned)a->n_critics), dim3(RPL_BLOCK), 0, stream, *a, sets);
    HIP_OK(hipGetLastError());
  }
  if (a->launches == RP_CRITIC_ROWS_ONLY) return 0;
  const unsigned blocks = blocks_for(a->D + a->A, 16) + (unsigned)(a->H1 / 16) + blocks_for(lay.V, RPL_BLOCK);
  hipLaunchKernelGGL(rp_critic_apply_kernel, dim3(blocks, (unsigned)a->n_critics), dim3(RPL_BLOCK), 0, stream, *a, sets);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
