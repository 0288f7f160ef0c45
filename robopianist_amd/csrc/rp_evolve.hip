// rp_evolve.hip -- librp_evolve.so: population-based training on the stacked tensors of a population
// (include/learn/rp_evolve.h).
//
//   rp_evolve_fold_kernel   one wave per member: the ended-episode counters of its envs into its fitness window, in a fixed
//                           summation order (a lane's envs ascending, then the lanes ascending)
//   rp_evolve_plan_kernel   one workgroup, one thread per member: eligibility, rank, the two ends, the losers' draw of a
//                           winner, the perturbed hyper-parameters, the cleared windows
//   rp_evolve_copy_kernel   grid (chunks of a slice, members, fields): slice p <- slice source[p] in the widest of 16 / 8 / 4
//                           bytes both addresses allow (rpl_copy_row's rule of rp_mlp_tile.hpp, over a grid); a workgroup
//                           whose member keeps itself returns on a uniform read of `source`
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_evolve.hpp"

namespace {

struct RpeFieldTable {
  rp_evolve_field f[RP_EVOLVE_MAX_FIELDS];
};

__global__ __launch_bounds__(RPE_WAVE) void rp_evolve_fold_kernel(const rp_evolve_fold_args a) {
  __shared__ double lane_sum[RPE_WAVE];
  __shared__ long long lane_count[RPE_WAVE];
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  const long long P = a.P, Em = a.E / a.P;
  double s = 0.0;
  long long c = 0;
  for (long long j = lane; j < Em; j += RPE_WAVE) {
    const long long e = p + P * j;
    s = s + a.done_return[e];
    c += (long long)a.done_count[e];
  }
  lane_sum[lane] = s;
  lane_count[lane] = c;
  __syncthreads();
  if (lane != 0) return;
  double t = 0.0;
  long long n = 0;
  for (int l = 0; l < RPE_WAVE; ++l) {
    t = t + lane_sum[l];
    n += lane_count[l];
  }
  a.fit_sum[p] = a.fit_sum[p] + t;
  a.fit_count[p] += n;
}

__global__ __launch_bounds__(RP_EVOLVE_MAX_MEMBERS) void rp_evolve_plan_kernel(const rp_evolve_plan_args a) {
  __shared__ double score[RP_EVOLVE_MAX_MEMBERS];
  __shared__ int eligible[RP_EVOLVE_MAX_MEMBERS];
  __shared__ int winner[RP_EVOLVE_MAX_MEMBERS];   // by rank
  const int p = (int)threadIdx.x, P = a.P;
  double sc = 0.0;
  int el = 0;
  if (p < P) {
    const long long c = a.fit_count[p];
    sc = a.fit_sum[p] / (double)c;
    el = c >= a.min_episodes && !isnan(sc);
  }
  score[p] = sc;
  eligible[p] = el;
  __syncthreads();
  int n = 0, rank = 0;
  for (int q = 0; q < P; ++q) {
    if (!eligible[q]) continue;
    ++n;
    const double o = score[q];
    if (o > sc || (o == sc && q < p)) ++rank;
  }
  const int k = rpe_ends(n, a.percent);
  if (el && rank < k) winner[rank] = p;
  __syncthreads();
  if (p >= P) return;
  int src = p;
  if (el && k > 0 && rank >= n - k) {
    const RpplWords x = rppl_philox(a.generation, (uint32_t)p, 0u, (uint32_t)RP_EVOLVE_COUNTER, a.seed_lo, a.seed_hi);
    const int w = winner[x.w[0] % (uint32_t)k];
    const double gap = score[w] - sc;
    if (gap > a.min_gap) {
      src = w;
      if (a.gamma) a.gamma[p] = rpe_explore_gamma(a.gamma[w], (x.w[1] & 1u) ? a.up : a.down, a.gamma_lo, a.gamma_hi);
      if (a.target_entropy)
        a.target_entropy[p] = rpe_explore_entropy(a.target_entropy[w], (x.w[1] & 2u) ? a.up : a.down, a.entropy_lo, a.entropy_hi);
    }
  }
  a.source[p] = src;
  a.fit_sum[p] = 0.0;
  a.fit_count[p] = 0;
}

// The units [lo, hi) (word offsets; hi - lo is a multiple of the unit) of slice s into slice d.
template <typename U>
__device__ inline void rpe_copy_units(const uint32_t* s, uint32_t* d, long long lo, long long hi) {
  constexpr int per = (int)(sizeof(U) / sizeof(uint32_t));
  const long long n = (hi - lo) / per;
  const U* su = reinterpret_cast<const U*>(s + lo);
  U* du = reinterpret_cast<U*>(d + lo);
  for (long long i = threadIdx.x; i < n; i += RPE_COPY_BLOCK) du[i] = su[i];
}

__global__ __launch_bounds__(RPE_COPY_BLOCK) void rp_evolve_copy_kernel(const RpeFieldTable tab, const int32_t* source, int P) {
  const int p = (int)blockIdx.y;
  const int s = source[p];                               // (uniform: one scalar read per workgroup)
  if (s == p || s < 0 || s >= P) return;
  if (source[s] != s) return;
  const rp_evolve_field f = tab.f[blockIdx.z];
  const long long width = f.slice_words;
  const long long first = (long long)blockIdx.x * RP_EVOLVE_CHUNK_WORDS;
  if (first >= width) return;
  const uint32_t* sp = static_cast<const uint32_t*>(f.base) + (long long)s * width;
  uint32_t* dp = static_cast<uint32_t*>(f.base) + (long long)p * width;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(sp), da = reinterpret_cast<uintptr_t>(dp);
  const int unit = ((sa ^ da) & 15) == 0 ? 16 : ((sa ^ da) & 7) == 0 ? 8 : 4;   // bytes
  const int per = unit >> 2;
  long long head = (long long)((((uintptr_t)unit - (sa & (uintptr_t)(unit - 1))) & (uintptr_t)(unit - 1)) >> 2);   // <= 3
  if (head > width) head = width;
  const long long body_end = head + (width - head) / per * per;
  const long long lo = head + first;
  long long hi = lo + RP_EVOLVE_CHUNK_WORDS;
  if (hi > body_end) hi = body_end;
  if (unit == 16) rpe_copy_units<uint4>(sp, dp, lo, hi);
  else if (unit == 8) rpe_copy_units<uint2>(sp, dp, lo, hi);
  else rpe_copy_units<uint32_t>(sp, dp, lo, hi);
  if (blockIdx.x == 0) {   // the single words in front of the first unit and after the last one: < 4 each
    const int lane = (int)threadIdx.x;
    if (lane < head) dp[lane] = sp[lane];
    for (long long i = body_end + lane; i < width; i += RPE_COPY_BLOCK) dp[i] = sp[i];
  }
}

}  // namespace

extern "C" {

const char* rp_evolve_last_error(void) { return g_err.c_str(); }

int rp_evolve_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_members")) return RP_EVOLVE_MAX_MEMBERS;
  if (!strcmp(name, "max_fields")) return RP_EVOLVE_MAX_FIELDS;
  if (!strcmp(name, "chunk_words")) return RP_EVOLVE_CHUNK_WORDS;
  if (!strcmp(name, "counter")) return RP_EVOLVE_COUNTER;
  if (!strcmp(name, "wave_size")) return RPE_WAVE;
  return -1;
}

int rp_evolve_fold(const rp_evolve_fold_args* a) {
  RP_ARGS_HEAD("rp_evolve_fold", rp_evolve_fold_args);
  RP_ARGS_CHECK(rpe_check_fold(*a));
  hipLaunchKernelGGL(rp_evolve_fold_kernel, dim3((unsigned)a->P), dim3(RPE_WAVE), 0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_evolve_plan(const rp_evolve_plan_args* a) {
  RP_ARGS_HEAD("rp_evolve_plan", rp_evolve_plan_args);
  RP_ARGS_CHECK(rpe_check_plan(*a));
  hipLaunchKernelGGL(rp_evolve_plan_kernel, dim3(1), dim3(RP_EVOLVE_MAX_MEMBERS), 0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_evolve_copy(rp_evolve_copy_args* a) {
  RP_ARGS_HEAD("rp_evolve_copy", rp_evolve_copy_args);
  RP_ARGS_CHECK(rpe_check_copy(*a));
  a->launches = 0;
  if (a->n_fields == 0 || a->P == 1) return 0;
  for (int first = 0; first < a->n_fields; first += RP_EVOLVE_MAX_FIELDS) {
    const int count = a->n_fields - first < RP_EVOLVE_MAX_FIELDS ? a->n_fields - first : RP_EVOLVE_MAX_FIELDS;
    RpeFieldTable tab;
    memset(&tab, 0, sizeof(tab));
    long long widest = 0;
    for (int i = 0; i < count; ++i) {
      tab.f[i] = a->fields[first + i];
      if (tab.f[i].slice_words > widest) widest = tab.f[i].slice_words;
    }
    hipLaunchKernelGGL(rp_evolve_copy_kernel, dim3(blocks_for(widest, RP_EVOLVE_CHUNK_WORDS), (unsigned)a->P, (unsigned)count),
                       dim3(RPE_COPY_BLOCK), 0, (hipStream_t)a->hip_stream, tab, a->source, a->P);
    HIP_OK(hipGetLastError());
    ++a->launches;
  }
  return 0;
}

}  // extern "C"
