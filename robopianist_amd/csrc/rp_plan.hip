// rp_plan.hip -- librp_plan.so: the kernels of the predictive-sampling planner (include/plan/rp_plan.h).
//
// One launch per call:
//   rp_plan_fork_kernel        one workgroup of one wave per (row, field): dst row e <- src row e / K, in the widest
//                              unit both rows are aligned to (16 / 8 / 4 / 2 / 1 bytes) plus a byte tail
//   rp_plan_sample_kernel      one thread per knot entry (e, p nu + u): Philox noise around the group's nominal
//   rp_plan_action_kernel<T>   one thread per (row, u): the spline at control step h, float64, rounded once to T
//   rp_plan_accumulate_kernel<T>  one thread per row: the discounted return of the rows that are still alive
//   rp_plan_select_kernel      one wave per group: argmax over the K returns, the winner's knots into the nominal
//   rp_plan_shift_kernel       one thread per (group, u): the nominal one control step later, in place
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "rp_abi_host.hpp"
#include "rp_plan.hpp"

namespace {

#define RPPL_BLOCK 256

struct RpplFieldTable {
  rp_plan_field f[RP_PLAN_MAX_FIELDS];
};

template <typename U>
__device__ inline long long rppl_copy_units(const unsigned char* s, unsigned char* d, long long bytes) {
  const long long n = bytes / (long long)sizeof(U);
  const U* su = reinterpret_cast<const U*>(s);
  U* du = reinterpret_cast<U*>(d);
  for (long long i = threadIdx.x; i < n; i += RPPL_WAVE) du[i] = su[i];
  return n * (long long)sizeof(U);
}

__global__ __launch_bounds__(RPPL_WAVE) void rp_plan_fork_kernel(const RpplFieldTable tab, int K, int env_first) {
  const rp_plan_field f = tab.f[blockIdx.y];
  const long long e = (long long)env_first + blockIdx.x, g = e / K;
  const unsigned char* s = static_cast<const unsigned char*>(f.src) + g * f.row_bytes;
  unsigned char* d = static_cast<unsigned char*>(f.dst) + e * f.row_bytes;
  const uintptr_t both = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d);
  long long done;
  if ((both & 15) == 0) done = rppl_copy_units<uint4>(s, d, f.row_bytes);
  else if ((both & 7) == 0) done = rppl_copy_units<uint2>(s, d, f.row_bytes);
  else if ((both & 3) == 0) done = rppl_copy_units<uint32_t>(s, d, f.row_bytes);
  else if ((both & 1) == 0) done = rppl_copy_units<uint16_t>(s, d, f.row_bytes);
  else done = 0;
  for (long long i = done + threadIdx.x; i < f.row_bytes; i += RPPL_WAVE) d[i] = s[i];   // (the tail: < 16 bytes, or all)
}

__global__ __launch_bounds__(RPPL_BLOCK) void rp_plan_sample_kernel(const rp_plan_sample_args a, long long total) {
  const long long idx = (long long)blockIdx.x * RPPL_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const int PN = a.P * a.nu;
  const long long e = (long long)a.env_first + idx / PN;
  const int c = (int)(idx % PN), u = c % a.nu;
  const long long g = e / a.K;
  const int k = (int)(e % a.K);
  double v = a.nominal[g * PN + c];
  if (k > 0) {
    const double z = rppl_z(a.seed_lo, a.seed_hi, a.round, (uint32_t)e, (uint32_t)c);
    const double t = a.sigma[u] * z;
    v = v + t;
  }
  v = fmax(v, a.lo[u]);
  v = fmin(v, a.hi[u]);
  a.knots[e * PN + c] = v;
}

template <typename T>
__global__ __launch_bounds__(RPPL_BLOCK) void rp_plan_action_kernel(const rp_plan_action_args a, long long total) {
  const long long idx = (long long)blockIdx.x * RPPL_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long long r = (long long)a.row_first + idx / a.nu;
  const int u = (int)(idx % a.nu);
  const double* row = a.knots + r * a.P * a.nu + u;
  const int nu = a.nu;
  const double v = rppl_spline(a.spline, a.h, a.H, a.P, [&](int i) { return row[(long long)i * nu]; });
  static_cast<T*>(a.out)[r * a.nu + u] = (T)v;
}

template <typename T>
__global__ __launch_bounds__(RPPL_BLOCK) void rp_plan_accumulate_kernel(const rp_plan_accumulate_args a) {
  const long long idx = (long long)blockIdx.x * RPPL_BLOCK + threadIdx.x;
  if (idx >= a.env_count) return;
  const long long e = (long long)a.env_first + idx;
  if (!a.alive[e]) return;
  const double r = (double)static_cast<const T*>(a.reward)[e];
  const double t = a.weight * r;
  const double sum = a.ret[e] + t;
  a.ret[e] = sum;
  if (a.step_type[e] == RP_PLAN_STEP_LAST) a.alive[e] = 0;
}

// (value, candidate) pairs; candidate -1 = none yet.  `b` beats `a` if it is a number and a is none, or larger, or equal
// with the lower candidate.
__device__ inline void rppl_better(double& av, int& ak, double bv, int bk) {
  if (bk < 0) return;
  if (ak < 0 || bv > av || (bv == av && bk < ak)) { av = bv; ak = bk; }
}

__global__ __launch_bounds__(RPPL_WAVE) void rp_plan_select_kernel(const rp_plan_select_args a) {
  const long long g = (long long)a.group_first + blockIdx.x;
  const int lane = (int)threadIdx.x;
  const double* ret = a.ret + g * a.K;
  double bv = 0.0;
  int bk = -1;
  for (int k = lane; k < a.K; k += RPPL_WAVE) {   // K > 64: every lane keeps the best of its candidates
    const double v = ret[k];
    if (v == v) rppl_better(bv, bk, v, k);        // (NaN never enters)
  }
  for (int off = RPPL_WAVE / 2; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off, RPPL_WAVE);
    const int ok = __shfl_down(bk, off, RPPL_WAVE);
    rppl_better(bv, bk, ov, ok);
  }
  bk = __shfl(bk, 0, RPPL_WAVE);
  if (bk < 0) bk = 0;                             // all NaN
  if (lane == 0) {
    a.best_k[g] = bk;
    a.best_return[g] = ret[bk];
  }
  const long long PN = (long long)a.P * a.nu;
  const double* src = a.knots + (g * a.K + bk) * PN;
  double* dst = a.nominal + g * PN;
  for (long long i = lane; i < PN; i += RPPL_WAVE) dst[i] = src[i];
}

__global__ __launch_bounds__(RPPL_BLOCK) void rp_plan_shift_kernel(const rp_plan_shift_args a, long long total) {
  const long long idx = (long long)blockIdx.x * RPPL_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const long long g = (long long)a.group_first + idx / a.nu;
  const int u = (int)(idx % a.nu), nu = a.nu;
  double* col = a.nominal + g * a.P * a.nu + u;
  // ascending p, in place: the new knot p reads old knots p - 1 (linear, last knot only) .. p + 2; knot p - 1 has been
  // overwritten by then, so its old value is carried in a register
  double before = 0.0;
  for (int p = 0; p < a.P; ++p) {
    int h = rppl_knot_step(a.spline, p, a.H, a.P) + 1;
    if (h > a.H - 1) h = a.H - 1;
    const double v = rppl_spline(a.spline, h, a.H, a.P,
                                 [&](int i) { return i == p - 1 ? before : col[(long long)i * nu]; });
    before = col[(long long)p * nu];
    col[(long long)p * nu] = v;
  }
}

}  // namespace

extern "C" {

const char* rp_plan_last_error(void) { return g_err.c_str(); }

int rp_plan_dim(const char* name) {
  if (!name) return -1;
  if (!strcmp(name, "max_fields")) return RP_PLAN_MAX_FIELDS;
  if (!strcmp(name, "wave_size")) return RPPL_WAVE;
  return -1;
}

int rp_plan_fork(const rp_plan_fork_args* a) {
  RP_ARGS_HEAD("rp_plan_fork", rp_plan_fork_args);
  if (!a->fields) return fail("rp_plan_fork: fields is NULL");
  if (a->n_fields < 1 || a->n_fields > RP_PLAN_MAX_FIELDS)
    return fail("rp_plan_fork: n_fields must be 1 .. " + std::to_string(RP_PLAN_MAX_FIELDS) + ", got " + std::to_string(a->n_fields));
  RP_ARGS_CHECK(rppl_check_layout("rp_plan_fork", a->G, a->K, 1, 1));
  RP_ARGS_CHECK(rppl_check_range("rp_plan_fork", "the row range", (long long)a->G * a->K, a->env_first, a->env_count));
  RpplFieldTable tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 0; i < a->n_fields; ++i) {
    const rp_plan_field& f = a->fields[i];
    if (!f.src || !f.dst) return fail("rp_plan_fork: field " + std::to_string(i) + " has a NULL pointer");
    if (f.row_bytes < 1) return fail("rp_plan_fork: field " + std::to_string(i) + " has row_bytes < 1");
    tab.f[i] = f;
  }
  if (a->env_count == 0) return 0;
  hipLaunchKernelGGL(rp_plan_fork_kernel, dim3((unsigned)a->env_count, (unsigned)a->n_fields), dim3(RPPL_WAVE), 0,
                     (hipStream_t)a->hip_stream, tab, a->K, a->env_first);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_plan_sample(const rp_plan_sample_args* a) {
  RP_ARGS_HEAD("rp_plan_sample", rp_plan_sample_args);
  if (!a->nominal || !a->sigma || !a->lo || !a->hi || !a->knots) return fail("rp_plan_sample: a pointer is NULL");
  RP_ARGS_CHECK(rppl_check_layout("rp_plan_sample", a->G, a->K, a->P, a->nu));
  RP_ARGS_CHECK(rppl_check_range("rp_plan_sample", "the row range", (long long)a->G * a->K, a->env_first, a->env_count));
  const long long total = (long long)a->env_count * a->P * a->nu;
  if (total == 0) return 0;
  if ((total + RPPL_BLOCK - 1) / RPPL_BLOCK > 0x7fffffffLL) return fail("rp_plan_sample: too many entries for one launch");
  hipLaunchKernelGGL(rp_plan_sample_kernel, dim3(blocks_for(total, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a, total);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_plan_action(const rp_plan_action_args* a) {
  RP_ARGS_HEAD("rp_plan_action", rp_plan_action_args);
  if (!a->knots || !a->out) return fail("rp_plan_action: a pointer is NULL");
  if (a->precision != 32 && a->precision != 64) return fail("rp_plan_action: precision must be 32 or 64");
  if (a->nu < 1) return fail("rp_plan_action: nu must be >= 1");
  RP_ARGS_CHECK(rppl_check_spline("rp_plan_action", a->spline, a->H, a->P));
  if (a->h < 0 || a->h >= a->H) return fail("rp_plan_action: h must lie in [0, H)");
  if (a->n_rows < 1) return fail("rp_plan_action: n_rows must be >= 1");
  RP_ARGS_CHECK(rppl_check_range("rp_plan_action", "the row range", a->n_rows, a->row_first, a->row_count));
  const long long total = (long long)a->row_count * a->nu;
  if (total == 0) return 0;
  if (a->precision == 32)
    hipLaunchKernelGGL(rp_plan_action_kernel<float>, dim3(blocks_for(total, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a, total);
  else
    hipLaunchKernelGGL(rp_plan_action_kernel<double>, dim3(blocks_for(total, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a, total);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_plan_accumulate(const rp_plan_accumulate_args* a) {
  RP_ARGS_HEAD("rp_plan_accumulate", rp_plan_accumulate_args);
  if (!a->ret || !a->alive || !a->reward || !a->step_type) return fail("rp_plan_accumulate: a pointer is NULL");
  if (a->precision != 32 && a->precision != 64) return fail("rp_plan_accumulate: precision must be 32 or 64");
  if (a->E < 1) return fail("rp_plan_accumulate: E must be >= 1");
  RP_ARGS_CHECK(rppl_check_range("rp_plan_accumulate", "the row range", a->E, a->env_first, a->env_count));
  if (a->env_count == 0) return 0;
  if (a->precision == 32)
    hipLaunchKernelGGL(rp_plan_accumulate_kernel<float>, dim3(blocks_for(a->env_count, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a);
  else
    hipLaunchKernelGGL(rp_plan_accumulate_kernel<double>, dim3(blocks_for(a->env_count, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_plan_select(const rp_plan_select_args* a) {
  RP_ARGS_HEAD("rp_plan_select", rp_plan_select_args);
  if (!a->ret || !a->knots || !a->nominal || !a->best_k || !a->best_return) return fail("rp_plan_select: a pointer is NULL");
  RP_ARGS_CHECK(rppl_check_layout("rp_plan_select", a->G, a->K, a->P, a->nu));
  RP_ARGS_CHECK(rppl_check_range("rp_plan_select", "the group range", a->G, a->group_first, a->group_count));
  if (a->group_count == 0) return 0;
  hipLaunchKernelGGL(rp_plan_select_kernel, dim3((unsigned)a->group_count), dim3(RPPL_WAVE), 0, (hipStream_t)a->hip_stream, *a);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_plan_shift(const rp_plan_shift_args* a) {
  RP_ARGS_HEAD("rp_plan_shift", rp_plan_shift_args);
  if (!a->nominal) return fail("rp_plan_shift: nominal is NULL");
  RP_ARGS_CHECK(rppl_check_layout("rp_plan_shift", a->G, 1, a->P, a->nu));
  RP_ARGS_CHECK(rppl_check_spline("rp_plan_shift", a->spline, a->H, a->P));
  RP_ARGS_CHECK(rppl_check_range("rp_plan_shift", "the group range", a->G, a->group_first, a->group_count));
  const long long total = (long long)a->group_count * a->nu;
  if (total == 0) return 0;
  hipLaunchKernelGGL(rp_plan_shift_kernel, dim3(blocks_for(total, RPPL_BLOCK)), dim3(RPPL_BLOCK), 0, (hipStream_t)a->hip_stream, *a, total);
  HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
