// rp_ik.hip -- librp_ik.so: batched fingertip inverse kinematics on the engine's state (include/control/rp_ik.h).
//
// One launch per call:
//   rp_ik_kernel<T>  one workgroup of one wave per env; lanes 0-31 work for hand 0, lanes 32-63 for hand 1.  A lane is
//                    a body in the tree walk, a dof column in the Jacobian and the update, a row in the 15 x 15
//                    Cholesky solve and an actuator in the transmission (rp_ik.hpp: rpik_solve_env).  The hand's
//                    frames, J, A and its factor sit in LDS; the K iterations run inside the launch.
#include "rp_abi_host.hpp"
#include "rp_ik.hpp"

namespace {

#define RPIK_BLOCK (RPIK_MAX_HANDS * RPIK_LANES)   // 64: one wave

struct RpikWaveCtx {
  int h0, h1, l0, l1;
  __device__ void sync() const { __syncthreads(); }
};

template <typename T>
__global__ __launch_bounds__(RPIK_BLOCK) void rp_ik_kernel(const RpikModel* __restrict__ Mp, const RpikCall c, int env_first) {
  __shared__ RpikWork W[RPIK_MAX_HANDS];
  const int h = (int)threadIdx.x / RPIK_LANES, l = (int)threadIdx.x % RPIK_LANES;
  RpikWaveCtx ctx = {h, h + 1, l, l + 1};
  // (every thread of the workgroup runs every phase of its env: the barriers inside are met by all 64)
  rpik_solve_env<T>(*Mp, c, env_first + (int)blockIdx.x, W, ctx);
}

}  // namespace

struct rp_ik {
  RpikModel M;            // host copy
  RpikModel* d_M = nullptr;
  int n_envs = 0, device = 0, precision = 64;
};

extern "C" {

const char* rp_ik_last_error(void) { return g_err.c_str(); }

int rp_ik_create(const void* blob, size_t bytes, int n_envs, int device, int precision, rp_ik** out) {
  if (!out) return fail("rp_ik_create: out is NULL");
  *out = nullptr;
  if (n_envs <= 0) return fail("rp_ik_create: n_envs must be positive");
  if (precision != 32 && precision != 64) return fail("rp_ik_create: precision must be 32 or 64");
  rp_ik* r = new rp_ik();
  const std::string err = rpik_parse(blob, bytes, r->M);
  if (!err.empty()) { delete r; return fail("rp_ik_create: " + err); }
  r->n_envs = n_envs; r->device = device; r->precision = precision;
  CreateGuard<rp_ik> guard{r, rp_ik_destroy};
  HIP_OK_AS("rp_ik_create", "hipSetDevice", hipSetDevice(device));
  if (upload("rp_ik_create", &r->d_M, &r->M, 1)) return -1;
  *out = guard.release();
  return 0;
}

void rp_ik_destroy(rp_ik* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  free_all({r->d_M});
  delete r;
}

int rp_ik_solve(rp_ik* r, const rp_ik_args* a) {
  RP_HANDLE_HEAD(r, "rp_ik_solve: solver is NULL");
  RP_ARGS_CHECK(rpik_check_args(a, r->n_envs, r->M));
  HIP_OK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)a->hip_stream;
  const RpikCall c = rpik_call(a, r->M);
  const dim3 grid((unsigned)a->env_count), block(RPIK_BLOCK);
  if (r->precision == 32)
    hipLaunchKernelGGL(rp_ik_kernel<float>, grid, block, 0, st, (const RpikModel*)r->d_M, c, a->env_first);
  else
    hipLaunchKernelGGL(rp_ik_kernel<double>, grid, block, 0, st, (const RpikModel*)r->d_M, c, a->env_first);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_ik_dim(const rp_ik* r, const char* name) {
  if (!r || !name) return -1;
  if (!strcmp(name, "n_hands")) return r->M.nhand;
  if (!strcmp(name, "n_tips")) return RPIK_TIPS * r->M.nhand;
  if (!strcmp(name, "n_act")) return r->M.nact;
  if (!strcmp(name, "n_dof")) return r->M.ndof;
  if (!strcmp(name, "nv")) return r->M.nv;
  if (!strcmp(name, "ntree")) return r->M.ntree;
  if (!strcmp(name, "n_envs")) return r->n_envs;
  return -1;
}

}  // extern "C"
