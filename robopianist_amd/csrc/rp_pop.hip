// rp_pop.hip -- librp_pop.so: the kernels of a population of DroQ learners on one env batch (include/learn/rp_pop.h).
//
// Every kernel is a caller of the device text of a single-learner kernel (rp_sac.hpp: rps_sample_row, rps_act_tile;
// rp_droq.hpp: rpd_target_tile; rp_learn.hpp: rpl_moments_block) with two things of its own: the map from a member's
// logical row to the array row, and the member's slices of the stacked tensors as the weight set.  A workgroup derives
// its member p from its index, moves the bases in its copy of the single-learner argument block by p slices (scalar
// arithmetic: p is uniform over the workgroup) and calls the shared body.  Nothing else is computed here, so a member's
// rows get the bits the single-learner kernel gives on the same array rows with that member's tensors.
//
// One launch per call:
//   rp_pop_sample_kernel   grid (row_count, member_count), one wave: rps_sample_row on the blocked row p n + b, drawing
//                          over the member's envs p + P jj (RpsEnvsMember).
//   rp_pop_act_kernel      grid (member_count x tiles), four waves: rps_act_tile on RplRowAffine{p member_stride,
//                          row_stride}, which is (p, P) interleaved and (p rows, 1) blocked -- the host resolves the
//                          layout into the two strides, the kernel has no branch on it.
//   rp_pop_target_kernel   grid (member_count x tiles), four waves: rpd_target_tile on the blocked rows.
//   rp_pop_moments_kernel  grid (column block of 16, member_count): rpl_moments_block on RppRowSlots.
// The workgroup -> (member, tile) rule of act and target is rpp_member_tile, one expression per order (rp_pop.h).
// Resources (gfx950, -O3 -ffp-contract=on, the compiler's kernel-resource-usage remark): profiles/pop_resources_new.txt.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_pop.hpp"
#include "rp_mlp_tile.hpp"

namespace {

// The members and tiles of a launch of act or target, and the layout as two strides.
struct RppGrid {
  int member_first, member_count;
  int tiles;                 // per member: ceil(row_count / 16)
  int order;                 // RP_POP_TILE_MAJOR / RP_POP_MEMBER_MAJOR
  int row_first, row_count;  // within the member
  long long member_stride;   // array rows between row j of member p and of member p + 1: 1 interleaved, rows blocked
  long long row_stride;      // array rows between rows j and j + 1 of a member: P interleaved, 1 blocked
};

// Workgroup b of member_count x tiles -> its member (absolute) and its tile.
__device__ inline void rpp_member_tile(const RppGrid& g, int& p, int& t) {
  const int b = (int)blockIdx.x;
  const bool tile_major = g.order == RP_POP_TILE_MAJOR;   // (uniform over the grid)
  p = g.member_first + (tile_major ? b % g.member_count : b / g.tiles);
  t = tile_major ? b / g.member_count : b % g.tiles;
}

// Member p's slices of a stacked network whose layers are [H1][K], [H2][H1], [N3][H2].
__device__ inline rp_learn_mlp rpp_slice(rp_learn_mlp m, size_t p, size_t K, size_t H1, size_t H2, size_t N3) {
  m.w1 += p * H1 * K; m.b1 += p * H1;
  m.w2 += p * H2 * H1; m.b2 += p * H2;
  m.w3 += p * N3 * H2; m.b3 += p * N3;
  return m;
}

// ---- sample ----------------------------------------------------------------------------------------------------------
struct RppSample {
  int P, n, member_first, row_first;
};

__global__ __launch_bounds__(RPL_WAVE) void rp_pop_sample_kernel(const rp_sac_sample_args a, const RppSample g) {
  const long long p = (long long)g.member_first + blockIdx.y;
  const long long b = p * g.n + g.row_first + blockIdx.x;
  rps_sample_row(a, b, RpsEnvsMember{(long long)(a.E / g.P), p, (long long)g.P});
}

// ---- act -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RPL_BLOCK) void rp_pop_act_kernel(rp_sac_act_args a, RpsActor actor, const RppGrid g) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];
  __shared__ float sh[RPL_TILE_R * RPL_H_PITCH];
  int p, t;
  rpp_member_tile(g, p, t);
  actor.net = rpp_slice(actor.net, (size_t)p, (size_t)a.D, (size_t)a.H1, (size_t)a.H2, 2 * (size_t)a.A);
  a.mean += (size_t)p * a.D;
  a.inv_std += (size_t)p * a.D;
  rps_act_tile(a, actor, RplRowAffine{(long long)p * g.member_stride, g.row_stride},
               (long long)g.row_first + (long long)t * RPL_TILE_R, (long long)g.row_first + g.row_count, sa, sw, sh);
}

// ---- target ----------------------------------------------------------------------------------------------------------
// Member p's slices of the stacked critics (the bases stay where the launch put them: critic i is indexed there).
struct RppCritics {
  const RpdCritics& base;
  size_t p, K, H1, H2;
  __device__ rp_droq_critic operator()(int i) const {
    rp_droq_critic c = base.c[i];
    c.net = rpp_slice(c.net, p, K, H1, H2, 1);
    c.g1 += p * H1; c.be1 += p * H1;
    c.g2 += p * H2; c.be2 += p * H2;
    return c;
  }
};

__global__ __launch_bounds__(RPL_BLOCK) void rp_pop_target_kernel(rp_droq_target_args a, const RpdCritics critics,
                                                                  const float* __restrict__ gamma, const RppGrid g) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];
  __shared__ __attribute__((aligned(16))) float sh[RPL_TILE_R * RPL_H_PITCH];
  __shared__ float sq[RPL_TILE_R];
  int p, t;
  rpp_member_tile(g, p, t);
  a.mean += (size_t)p * a.D;
  a.inv_std += (size_t)p * a.D;
  a.log_alpha += p;
  a.gamma = gamma[p];
  rpd_target_tile(a, RppCritics{critics, (size_t)p, (size_t)a.D + (size_t)a.A, (size_t)a.H1, (size_t)a.H2},
                  RplRowAffine{(long long)p * g.member_stride, g.row_stride},
                  (long long)g.row_first + (long long)t * RPL_TILE_R, (long long)g.row_first + g.row_count, sa, sw, sh, sq);
}

// ---- moments ---------------------------------------------------------------------------------------------------------
// Member p's logical row r = t Em + jj of k slots of E envs is array row t E + p + P jj.
struct RppRowSlots {
  long long Em, E, P, p;
  __device__ long long operator()(long long r) const {
    const long long t = r / Em, jj = r - t * Em;
    return t * E + p + P * jj;
  }
};

struct RppMoments {
  int E, P, member_first;
};

__global__ __launch_bounds__(RPL_MOMENT_COLS * RPL_MOMENT_LANES) void rp_pop_moments_kernel(rp_learn_moments_args a,
                                                                                           const RppMoments g) {
  __shared__ double part[RPL_MOMENT_LANES][RPL_MOMENT_COLS];
  const long long p = (long long)g.member_first + blockIdx.y;
  const size_t off = (size_t)p * a.D;
  a.mean += off; a.M2 += off; a.mean_f32 += off; a.inv_std_f32 += off;
  rpl_moments_block(a, RppRowSlots{(long long)(g.E / g.P), (long long)g.E, (long long)g.P, p}, part);
}

RppGrid grid_of(int order, int member_first, int member_count, int row_first, int row_count, long long member_stride,
                long long row_stride) {
  RppGrid g;
  g.member_first = member_first; g.member_count = member_count;
  g.tiles = (int)blocks_for(row_count, RPL_TILE_R);
  g.order = order;
  g.row_first = row_first; g.row_count = row_count;
  g.member_stride = member_stride; g.row_stride = row_stride;
  return g;
}

}  // namespace

extern "C" {

const char* rp_pop_last_error(void) { return g_err.c_str(); }

int rp_pop_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "interleaved")) return RP_POP_INTERLEAVED;
  if (!strcmp(name, "blocked")) return RP_POP_BLOCKED;
  if (!strcmp(name, "tile_major")) return RP_POP_TILE_MAJOR;
  if (!strcmp(name, "member_major")) return RP_POP_MEMBER_MAJOR;
  if (!strcmp(name, "default_grid_order")) return RP_POP_TILE_MAJOR;
  if (!strcmp(name, "tile_rows")) return RPL_TILE_R;
  if (!strcmp(name, "max_critics")) return RP_DROQ_MAX_CRITICS;
  if (!strcmp(name, "sample_tries")) return RP_SAC_SAMPLE_TRIES;
  if (!strcmp(name, "max_hidden")) return RP_LEARN_MAX_H;
  if (!strcmp(name, "max_actions")) return RP_SAC_MAX_HEAD / 2;
  if (!strcmp(name, "moment_lanes")) return RPL_MOMENT_LANES;
  return -1;
}

int rp_pop_sample(const rp_pop_sample_args* a) {
  RP_ARGS_HEAD("rp_pop_sample", rp_pop_sample_args);
  RP_ARGS_CHECK(rpp_check_sample(a));
  if (a->row_count == 0 || a->member_count == 0) return 0;
  if (a->member_count > 65535) return fail("rp_pop_sample: more than 65535 members in one launch");
  const RppSample g = {a->P, a->n, a->member_first, a->row_first};
  hipLaunchKernelGGL(rp_pop_sample_kernel, dim3((unsigned)a->row_count, (unsigned)a->member_count), dim3(RPL_WAVE), 0,
                     (hipStream_t)a->hip_stream, rpp_as_sac_sample(a), g);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_pop_act(const rp_pop_act_args* a) {
  RP_ARGS_HEAD("rp_pop_act", rp_pop_act_args);
  RP_ARGS_CHECK(rpp_check_act(a));
  if (a->row_count == 0 || a->member_count == 0) return 0;
  const bool interleaved = a->layout == RP_POP_INTERLEAVED;
  const RppGrid g = grid_of(a->grid_order, a->member_first, a->member_count, a->row_first, a->row_count,
                            interleaved ? 1 : a->rows, interleaved ? a->P : 1);
  if ((long long)g.tiles * a->member_count > 0x7fffffffLL) return fail("rp_pop_act: more than 2^31 - 1 workgroups");
  RpsActor actor;
  memset(&actor, 0, sizeof(actor));
  actor.net = *a->actor;
  actor.logp_const = (float)(0.5 * (double)a->A * 1.8378770664093453);   // ln 2 pi
  actor.ln2 = (float)0.6931471805599453;
  hipLaunchKernelGGL(rp_pop_act_kernel, dim3((unsigned)(g.tiles * a->member_count)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, rpp_as_sac_act(a), actor, g);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_pop_target(const rp_pop_target_args* a) {
  RP_ARGS_HEAD("rp_pop_target", rp_pop_target_args);
  RP_ARGS_CHECK(rpp_check_target(a));
  if (a->row_count == 0 || a->member_count == 0) return 0;
  const RppGrid g = grid_of(a->grid_order, a->member_first, a->member_count, a->row_first, a->row_count, a->n, 1);
  if ((long long)g.tiles * a->member_count > 0x7fffffffLL) return fail("rp_pop_target: more than 2^31 - 1 workgroups");
  RpdCritics critics;
  memset(&critics, 0, sizeof(critics));
  for (int i = 0; i < a->n_critics; ++i) critics.c[i] = a->critics[i];
  hipLaunchKernelGGL(rp_pop_target_kernel, dim3((unsigned)(g.tiles * a->member_count)), dim3(RPL_BLOCK), 0,
                     (hipStream_t)a->hip_stream, rpp_as_droq_target(a), critics, a->gamma, g);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_pop_moments(const rp_pop_moments_args* a) {
  RP_ARGS_HEAD("rp_pop_moments", rp_pop_moments_args);
  RP_ARGS_CHECK(rpp_check_moments(a));
  if (a->member_count == 0) return 0;
  if (a->member_count > 65535) return fail("rp_pop_moments: more than 65535 members in one launch");
  const RppMoments g = {a->E, a->P, a->member_first};
  hipLaunchKernelGGL(rp_pop_moments_kernel, dim3(blocks_for(a->D, RPL_MOMENT_COLS), (unsigned)a->member_count),
                     dim3(RPL_MOMENT_COLS * RPL_MOMENT_LANES), 0, (hipStream_t)a->hip_stream, rpp_as_learn_moments(a), g);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
