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

#define RPD_ROW_LANES 16                                   // the lanes that own one row of the tile
#define RPD_GROUPS (RP_LEARN_MAX_H / 4 / RPD_ROW_LANES)    // groups of four units per lane at 256 units

struct RpdCritics {
  rp_droq_critic c[RP_DROQ_MAX_CRITICS];
};

// The sum of `p` over the sixteen lanes of a row: p[j] + p[j ^ 1], then ^ 2, ^ 4, ^ 8.  Every lane gets the same bits.
__device__ inline float rpd_row_sum(float p) {
#pragma unroll
  for (int m = 1; m < RPD_ROW_LANES; m <<= 1) {
    const float o = __shfl_xor(p, m, RPD_ROW_LANES);
    p = p + o;
  }
  return p;
}

// Dropout, LayerNorm and ReLU on the tile's sums `sh` [16][RPL_H_PITCH], in place (the header's epilogue, statement by
// statement).  `e0`: the tile's first absolute batch row; `ctr`: the last Philox counter word.  All 256 threads call it
// together, behind the barrier of rpl_store_layer; it ends with a barrier.
__device__ inline void rpd_drop_norm_relu(float* sh, int H, const float* __restrict__ g, const float* __restrict__ be,
                                          long long e0, uint32_t ctr, const rp_droq_target_args& a) {
  const int tid = (int)threadIdx.x, r = tid >> 4, j = tid & (RPD_ROW_LANES - 1);
  float* row = sh + r * RPL_H_PITCH;
  const uint32_t b = (uint32_t)(e0 + r);
  const int groups = H >> 2;
  const float fH = (float)H;
  float h[RPD_GROUPS][4];
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      const float4 s = *reinterpret_cast<const float4*>(row + 4 * grp);   // (sh is 16-byte aligned, the pitch 1040 bytes)
      const RpplWords w = rppl_philox(a.round, b, (uint32_t)grp, ctr, a.seed_lo, a.seed_hi);
      const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float v = sv[c] * a.keep_scale;
        h[i][c] = w.w[c] >= a.drop_threshold ? v : 0.f;
        p = p + h[i][c];
      }
    }
  }
  const float sum = rpd_row_sum(p);
  const float mu = sum / fH;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    if (j + RPD_ROW_LANES * i < groups) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        h[i][c] = h[i][c] - mu;
        const float dd = h[i][c] * h[i][c];
        q = q + dd;
      }
    }
  }
  const float sq = rpd_row_sum(q);
  const float var = sq / fH;
  const float t = var + a.ln_eps;
  const float root = sqrtf(t);
  const float rr = 1.f / root;
#pragma unroll
  for (int i = 0; i < RPD_GROUPS; i++) {
    const int grp = j + RPD_ROW_LANES * i;
    if (grp < groups) {
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const int n = 4 * grp + c;
        const float o1 = h[i][c] * rr;
        const float o2 = o1 * g[n];
        const float o3 = o2 + be[n];
        o[c] = fmaxf(o3, 0.f);
      }
      *reinterpret_cast<float4*>(row + 4 * grp) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(RPL_BLOCK) void rp_droq_target_kernel(const rp_droq_target_args a, const RpdCritics critics) {
  __shared__ float sa[RPL_TILE_R * RPL_S_PITCH];
  __shared__ float sw[RP_LEARN_MAX_H * RPL_S_PITCH];
  __shared__ __attribute__((aligned(16))) float sh[RPL_TILE_R * RPL_H_PITCH];
  __shared__ float sq[RPL_TILE_R];                      // the running minimum over the critics, per row
  const int tid = (int)threadIdx.x;
  const int D = a.D, A = a.A;
  const long long e0 = (long long)a.row_first + (long long)blockIdx.x * RPL_TILE_R;
  const long long e_end = (long long)a.row_first + a.row_count;
  f32x4 acc[RPL_ACC];
  const float clip = a.obs_clip, nclip = -a.obs_clip;
#pragma unroll 1
  for (int i = 0; i < a.n_critics; ++i) {   // (block-uniform)
    const rp_droq_critic cr = critics.c[i];
    const uint32_t ctr = RP_DROQ_COUNTER + 2u * (uint32_t)i;
    rpl_layer(
        [&](int r, int k) {
          const long long e = e0 + r;
          if (e >= e_end) return 0.f;
          if (k >= D) return a.action[(size_t)e * A + (k - D)];
          const float x = a.next_obs[(size_t)e * D + k];
          const float d = x - a.mean[k];
          const float p = d * a.inv_std[k];
          const float lo = fmaxf(p, nclip);
          return fminf(lo, clip);
        },
        D + A, cr.net.w1, a.H1, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b1, a.H1, sh);
    rpd_drop_norm_relu(sh, a.H1, cr.g1, cr.be1, e0, ctr, a);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H1, cr.net.w2, a.H2, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b2, a.H2, sh);
    rpd_drop_norm_relu(sh, a.H2, cr.g2, cr.be2, e0, ctr + 1u, a);
    rpl_layer([&](int r, int k) { return sh[r * RPL_H_PITCH + k]; }, a.H2, cr.net.w3, 1, sa, sw, acc);
    rpl_store_layer<false>(acc, cr.net.b3, 1, sh);
    // (thread r alone reads and writes sq[r]; sh[r][0] is rewritten only behind the next layers' barriers)
    if (tid < RPL_TILE_R) {
      const float q = sh[tid * RPL_H_PITCH];
      sq[tid] = i == 0 ? q : fminf(sq[tid], q);
      if (a.q && e0 + tid < e_end) a.q[(size_t)i * a.B + (size_t)(e0 + tid)] = q;
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
