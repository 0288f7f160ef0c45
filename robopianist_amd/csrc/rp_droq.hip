// rp_droq.hip -- librp_droq.so: the TD target of DroQ's dropout / LayerNorm critics (include/learn/rp_droq.h).
//
// One launch per call:
//   rp_droq_target_kernel  grid (row tile), four waves: rp_sac_target_kernel's loop over the critics on the tile of
//                          rp_mlp_tile.hpp, with a row epilogue of its own behind each hidden layer.  The layer's sums plus
//                          bias go to `sh` [16][RPL_H_PITCH] untouched (rpl_store_layer<false>); then sixteen lanes own a
//                          row (thread t: row t >> 4, lane t & 15; a row's lanes are sixteen consecutive lanes of one
//                          wave).  Lane j owns the groups j, j + 16, j + 32, j + 48 of four consecutive units: one 16-byte
//                          LDS read and one Philox call per group.  The mean and the centred squares are two passes over
//                          the lane's registers, each reduced over the sixteen lanes with __shfl_xor of width 16 (1, 2, 4,
//                          8: every lane ends with the same bits).  Only units n < H are ever read, so the padding columns
//                          of `sh` enter neither sum.  The result is written back in place and is the next layer's input.
//                          LDS banking of the epilogue: a row's lanes read consecutive 16-byte slots; the four rows of a
//                          wave start RPL_H_PITCH = 260 floats = one slot (mod 64 banks) apart, so ds_read_b128's
//                          16-lane groups meet a two-way conflict on one slot at most.  The epilogue is 2 x 16 rows x H
//                          values per critic next to (D + A + H1) H MFMA columns: it is not where the time goes.
// The body and its epilogue are device functions of rp_droq.hpp (rpd_target_tile, rpd_drop_norm_relu), which librp_pop.so
// runs on a member's rows too; the kernel here calls them with the identity map.
// Resources (gfx950, -O3 -ffp-contract=on, the compiler's kernel-resource-usage remark): 256 VGPRs + 94 AGPRs, 0 scratch,
// 53,696 bytes of LDS (rp_sac_target_kernel's arrays: the learner's three and 64 bytes of minima): one workgroup per CU,
// as rp_sac_target_kernel.  Measured times: DESIGN 6k (profiles/droq_bench.json).
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_droq.hpp"
#include "rp_mlp_tile.hpp"

namespace {

// The body is rp_droq.hpp's, on the identity map.
__global__ __launch_bounds__(RPL_BLOCK) void rp_droq_target_kernel(const rp_droq_target_args a, const RpdCritics critics) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];
  __shared__ __attribute__((aligned(16))) float sh[RPL_TILE_R * RPL_H_PITCH];
  __shared__ float sq[RPL_TILE_R];                      // the running minimum over the critics, per row
  rpd_target_tile(a, critics, RplRowIdentity{}, (long long)a.row_first + (long long)blockIdx.x * RPL_TILE_R,
                  (long long)a.row_first + a.row_count, sa, sw, sh, sq);
}

}  // namespace

extern "C" {

const char* rp_droq_last_error(void) { return g_err.c_str(); }

int rp_droq_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_critics")) return RP_DROQ_MAX_CRITICS;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  return -1;
}

int rp_droq_target(const rp_droq_target_args* a) {
  RP_ARGS_HEAD("rp_droq_target", rp_droq_target_args);
  RP_ARGS_CHECK(rpd_check_target(a));
  if (a->row_count == 0) return 0;
  RpdCritics critics;
  memset(&critics, 0, sizeof(critics));
  for (int i = 0; i < a->n_critics; ++i) critics.c[i] = a->critics[i];
  hipLaunchKernelGGL(rp_droq_target_kernel, dim3(blocks_for(a->row_count, RPL_TILE_R)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, *a, critics);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
