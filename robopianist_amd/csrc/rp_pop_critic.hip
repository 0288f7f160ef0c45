// rp_pop_critic.hip -- librp_pop_critic.so: the fused critic step of a population of DroQ learners
// (include/learn/rp_pop_critic.h).
//
// Both kernels are callers of the device text of librp_critic.so's two (rp_critic.hpp: rpc_rows_tile, rpc_apply_block).
// A workgroup derives its member p and its tile (rows) or block (apply) from its index, moves mean, inv_std, row_first
// and the workspace in its copy of the single-learner argument block to the member's (scalar arithmetic: p is uniform
// over the workgroup) and hands p to the shared body, which adds p slices to the bases of the weight sets where it
// reads them.  (The sets stay where the launch put them, in the kernel's argument segment: critic i and, in the apply
// launch's vector blocks, the tensor are indexed there at run time, and a moved copy of the fifty pointers per critic
// would have to live in scratch memory for that.)  Nothing else is computed here, so a member's step has the bits
// rp_critic_step gives on the same array rows with that member's slices.
//
// Two launches per call, the members flattened into grid.x, the critics side by side in grid.y:
//   rp_pop_critic_rows_kernel   grid (member_count x tiles of 16 rows, critics), four waves: rpc_rows_tile.
//   rp_pop_critic_apply_kernel  grid (member_count x (ceil((D + A) / 16) + H1 / 16 + ceil(V / 256)), critics):
//                               rpc_apply_block on the member's segment of the workspace.
// The workgroup -> (member, tile) rule is rp_pop.h's, one expression per order.
// Resources: profiles/pop_critic_resources.txt.  Measured times: DESIGN 6n (profiles/pop_critic_bench.json).
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_pop_critic.hpp"

namespace {

// The members of a launch and what each of them has in grid.x.
struct RppcGrid {
  int member_first, member_count;
  int per_member;          // rows: tiles of 16 rows; apply: blocks
  int order;               // RP_POP_TILE_MAJOR / RP_POP_MEMBER_MAJOR
  int n, row_first;        // rows per member; the range's first row within the member
  size_t segment;          // floats of one member's workspace
};

// Workgroup b of member_count x per_member -> its member (absolute) and its tile or block; the argument block becomes
// the member's.  Returns the member's workspace.
__device__ inline float* rppc_member(rp_critic_step_args& a, const RppcGrid& g, int& p, int& t) {
  const int b = (int)blockIdx.x;
  const bool tile_major = g.order == RP_POP_TILE_MAJOR;   // (uniform over the grid)
  const int m = tile_major ? b % g.member_count : b / g.per_member;
  t = tile_major ? b / g.member_count : b % g.per_member;
  p = g.member_first + m;
  a.mean += (size_t)p * a.D;
  a.inv_std += (size_t)p * a.D;
  a.row_first = p * g.n + g.row_first;   // (P n fits an int: checked)
  return (float*)a.workspace + (size_t)m * g.segment;
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_pop_critic_rows_kernel(rp_critic_step_args a, const RpcSets sets, const RppcGrid g) {
  __shared__ __attribute__((aligned(16))) float lds[RPC_ROWS_LDS_FLOATS];
  int p, t;
  float* ws = rppc_member(a, g, p, t);
  rpc_rows_tile(a, sets, t, (int)blockIdx.y, ws, lds, (size_t)p);
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_pop_critic_apply_kernel(rp_critic_step_args a, const RpcSets sets, const RppcGrid g) {
  __shared__ __attribute__((aligned(16))) float lds[RPL_TILE_R * RPL_S_PITCH + RP_LEARN_MAX_H * RPL_S_PITCH];
  int p, t;
  const float* ws = rppc_member(a, g, p, t);
  rpc_apply_block(a, sets, t, (int)blockIdx.y, ws, lds, (size_t)p);
}

}  // namespace

extern "C" {

const char* rp_pop_critic_last_error(void) { return g_err.c_str(); }

int rp_pop_critic_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_critics")) return RP_DROQ_MAX_CRITICS;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "stage_rows")) return RPL_TK;
  if (!strcmp(name, "launches")) return 2;
  if (!strcmp(name, "counter")) return RP_CRITIC_COUNTER;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  if (!strcmp(name, "tile_major")) return RP_POP_TILE_MAJOR;
  if (!strcmp(name, "member_major")) return RP_POP_MEMBER_MAJOR;
  if (!strcmp(name, "default_grid_order")) return RP_POP_TILE_MAJOR;
  return -1;
}

int rp_pop_critic_workspace(rp_pop_critic_workspace_args* a) {
  RP_ARGS_HEAD("rp_pop_critic_workspace", rp_pop_critic_workspace_args);
  RP_ARGS_CHECK(rppc_check_workspace(a));
  a->bytes = rppc_workspace_bytes(a->n_critics, a->H1, a->H2, a->row_count, a->member_count);
  return 0;
}

int rp_pop_critic_step(const rp_pop_critic_step_args* a) {
  RP_ARGS_HEAD("rp_pop_critic_step", rp_pop_critic_step_args);
  RP_ARGS_CHECK(rppc_check_step(a));
  if (a->row_count == 0 || a->member_count == 0) return 0;
  const RpcLayout lay = rpc_layout(a->H1, a->H2, a->row_count);
  const long long blocks = (long long)blocks_for(a->D + a->A, 16) + a->H1 / 16 + blocks_for(lay.V, RPL_BLOCK);
  if ((long long)lay.T * a->member_count > 0x7fffffffLL || blocks * a->member_count > 0x7fffffffLL)
    return fail("rp_pop_critic_step: more than 2^31 - 1 workgroups");
  RpcSets sets;
  memset(&sets, 0, sizeof(sets));
  for (int i = 0; i < a->n_critics; ++i) {
    sets.p[i] = a->p[i];
    sets.m[i] = a->m[i];
    sets.v[i] = a->v[i];
    sets.t[i] = a->target[i];
    if (a->grad) sets.g[i] = a->grad[i];
  }
  const rp_critic_step_args s = rppc_as_critic_step(a);
  RppcGrid g;
  g.member_first = a->member_first; g.member_count = a->member_count;
  g.order = a->grid_order;
  g.n = a->n; g.row_first = a->row_first;
  g.segment = lay.per_critic * (size_t)a->n_critics;
  const hipStream_t stream = (hipStream_t)a->hip_stream;
  if (a->launches != RP_CRITIC_APPLY_ONLY) {
    g.per_member = lay.T;
    hipLaunchKernelGGL(rp_pop_critic_rows_kernel, dim3((unsigned)(lay.T * a->member_count), (unsigned)a->n_critics), dim3(RPL_BLOCK),
                       0, stream, s, sets, g);
    HIP_OK(hipGetLastError());
  }
  if (a->launches == RP_CRITIC_ROWS_ONLY) return 0;
  g.per_member = (int)blocks;
  hipLaunchKernelGGL(rp_pop_critic_apply_kernel, dim3((unsigned)(blocks * a->member_count), (unsigned)a->n_critics), dim3(RPL_BLOCK),
                     0, stream, s, sets, g);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
