// rp_render.hip -- librp_render.so: batched camera rendering of the engine's state (include/render/rp_render.h).
//
// Two launches per call:
//   rp_render_frames_kernel<T>  one workgroup per env, thread = body: the body tree is walked level by level with the
//                               parents' frames in LDS (kinematics in the engine's T), then the threads write the
//                               world frame of every geom as 12 floats.
//   rp_render_kernel            grid (ceil(H W / 256), env), thread = pixel: the workgroup stages its env's geom
//                               frames in LDS, every thread casts its ray (rp_render.hpp: rpr_pixel).
#include "rp_abi_host.hpp"
#include "rp_render.hpp"

namespace {

template <typename T>
__global__ __launch_bounds__(RPR_MAX_BODIES) void rp_render_frames_kernel(
    const RprModel M, const T* __restrict__ qpos, const T* __restrict__ tree_offset, float* __restrict__ frames, int env_first) {
  __shared__ T sp[RPR_MAX_BODIES * 3];
  __shared__ T sq[RPR_MAX_BODIES * 4];
  const int env = env_first + (int)blockIdx.x;
  const int b = (int)threadIdx.x;
  const T* q = qpos + (size_t)env * M.nv;
  const T* off = tree_offset ? tree_offset + (size_t)env * M.ntree * 3 : nullptr;
  const int level = b < M.nbody ? M.body_level[b] : -1;
  if (b == 0) { sp[0] = sp[1] = sp[2] = 0; sq[0] = 1; sq[1] = sq[2] = sq[3] = 0; }
  __syncthreads();
  for (int l = 1; l < M.nlevel; l++) {   // (nlevel is uniform: every thread meets every barrier)
    if (level == l) {
      const int par = M.body_parentid[b];
      const T pp[3] = {sp[3 * par], sp[3 * par + 1], sp[3 * par + 2]};
      const T pq[4] = {sq[4 * par], sq[4 * par + 1], sq[4 * par + 2], sq[4 * par + 3]};
      T p[3], r[4];
      rpr_body_frame<T>(M, b, pp, pq, q, off, p, r);
      sp[3 * b] = p[0]; sp[3 * b + 1] = p[1]; sp[3 * b + 2] = p[2];
      sq[4 * b] = r[0]; sq[4 * b + 1] = r[1]; sq[4 * b + 2] = r[2]; sq[4 * b + 3] = r[3];
    }
    __syncthreads();
  }
  float* out = frames + (size_t)env * M.ngeom * RPR_FRAME;
  for (int g = b; g < M.ngeom; g += RPR_MAX_BODIES) {
    const int gb = M.geom_bodyid[g];
    const T bp[3] = {sp[3 * gb], sp[3 * gb + 1], sp[3 * gb + 2]};
    const T bq[4] = {sq[4 * gb], sq[4 * gb + 1], sq[4 * gb + 2], sq[4 * gb + 3]};
    float f[RPR_FRAME];
    rpr_geom_frame<T>(M, g, bp, bq, f);
#pragma unroll
    for (int k = 0; k < RPR_FRAME; k++) out[(size_t)g * RPR_FRAME + k] = f[k];
  }
}

__global__ __launch_bounds__(256) void rp_render_kernel(
    const RprModel M, const RprCamera cam, const float* __restrict__ frames, const unsigned char* __restrict__ key_rgb,
    unsigned char* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ seg, int env_first) {
  extern __shared__ float sfr[];   // [ngeom][12]
  const int env = env_first + (int)blockIdx.y;
  const int n = M.ngeom * RPR_FRAME;
  const float* src = frames + (size_t)env * n;
  for (int i = (int)threadIdx.x; i < n; i += 256) sfr[i] = src[i];
  __syncthreads();
  // the last workgroup of an image is partial: its spare threads leave after the only barrier
  const int npix = cam.height * cam.width;
  const int pix = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (pix >= npix) return;
  const size_t base = (size_t)env * npix;
  rpr_pixel(M, cam, sfr, key_rgb ? key_rgb + (size_t)env * RPR_N_KEYS * 3 : nullptr, pix,
            rgb ? rgb + base * 3 : nullptr, depth ? depth + base : nullptr, seg ? seg + base : nullptr);
}

}  // namespace

struct rp_renderer {
  RprTables tab;
  RprModel M;   // device view
  int n_envs = 0, device = 0, precision = 64;
  int* d_int = nullptr;
  double* d_dbl = nullptr;
  float* d_flt = nullptr;
  float* d_frames = nullptr;
  hipStream_t last_stream = nullptr;
};

extern "C" {

const char* rp_render_last_error(void) { return g_err.c_str(); }

int rp_render_create(const void* blob, size_t bytes, int n_envs, int device, int precision, rp_renderer** out) {
  if (!out) return fail("rp_render_create: out is NULL");
  *out = nullptr;
  if (n_envs <= 0) return fail("rp_render_create: n_envs must be positive");
  if (precision != 32 && precision != 64) return fail("rp_render_create: precision must be 32 or 64");
  rp_renderer* r = new rp_renderer();
  const std::string err = r->tab.parse(blob, bytes);
  if (!err.empty()) { delete r; return fail("rp_render_create: " + err); }
  r->n_envs = n_envs; r->device = device; r->precision = precision;
  CreateGuard<rp_renderer> guard{r, rp_render_destroy};
  HIP_OK_AS("rp_render_create", "hipSetDevice", hipSetDevice(device));
  const RprTables& t = r->tab;
  if (upload("rp_render_create", &r->d_int, t.I.data(), t.I.size())) return -1;
  if (upload("rp_render_create", &r->d_dbl, t.D.data(), t.D.size())) return -1;
  if (upload("rp_render_create", &r->d_flt, t.F.data(), t.F.size())) return -1;
  const size_t nfr = (size_t)n_envs * (size_t)(t.M.ngeom ? t.M.ngeom : 1) * RPR_FRAME;
  HIP_OK_AS("rp_render_create", "hipMalloc (geom frames)", hipMalloc(&r->d_frames, sizeof(float) * nfr));
  HIP_OK_AS("rp_render_create", "hipMemset", hipMemset(r->d_frames, 0, sizeof(float) * nfr));
  r->M = t.view(r->d_int, r->d_dbl, r->d_flt);
  *out = guard.release();
  return 0;
}

void rp_render_destroy(rp_renderer* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  free_all({r->d_int, r->d_dbl, r->d_flt, r->d_frames});
  delete r;
}

int rp_render(rp_renderer* r, const rp_render_args* a) {
  RP_HANDLE_HEAD(r, "rp_render: renderer is NULL");
  RP_ARGS_CHECK(rpr_check_args(a, r->n_envs));
  const long long npix = (long long)a->height * a->width;
  // (rpr_check_args bounds height and width by 16384: a pixel index fits an int; per-env bases are size_t)
  HIP_OK(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)a->hip_stream;
  const RprCamera cam = rpr_camera(a);
  const dim3 fgrid((unsigned)a->env_count), fblock(RPR_MAX_BODIES);
  if (r->precision == 32)
    hipLaunchKernelGGL(rp_render_frames_kernel<float>, fgrid, fblock, 0, st, r->M, (const float*)a->qpos,
                       (const float*)a->tree_offset, r->d_frames, a->env_first);
  else
    hipLaunchKernelGGL(rp_render_frames_kernel<double>, fgrid, fblock, 0, st, r->M, (const double*)a->qpos,
                       (const double*)a->tree_offset, r->d_frames, a->env_first);
  HIP_OK(hipGetLastError());
  r->last_stream = st;
  if (a->rgb || a->depth || a->segmentation) {
    const size_t lds = sizeof(float) * RPR_FRAME * (size_t)(r->M.ngeom ? r->M.ngeom : 1);
    // the env is the grid's y index, which the device limits to 65535: larger batches go out in slices
    for (int first = 0; first < a->env_count; first += RPR_MAX_GRID_Y) {
      const int count = rpr_slice_count(a->env_count, first);   // (tests: the arithmetic on the host; 65540 envs in two launches on the GPU)
      const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)count), block(256);
      hipLaunchKernelGGL(rp_render_kernel, grid, block, lds, st, r->M, cam, (const float*)r->d_frames, a->key_rgb, a->rgb,
                         a->depth, a->segmentation, a->env_first + first);
      HIP_OK(hipGetLastError());
    }
  }
  return 0;
}

int rp_render_geom_frames(rp_renderer* r, float* dst) {
  if (!r || !dst) return fail("rp_render_geom_frames: NULL argument");
  HIP_OK(hipSetDevice(r->device));
  const size_t nb = sizeof(float) * (size_t)r->n_envs * r->M.ngeom * RPR_FRAME;
  if (nb) HIP_OK(hipMemcpyAsync(dst, r->d_frames, nb, hipMemcpyDeviceToHost, r->last_stream));
  HIP_OK(hipStreamSynchronize(r->last_stream));
  return 0;
}

int rp_render_dim(const rp_renderer* r, const char* name) {
  if (!r || !name) return -1;
  if (!strcmp(name, "ngeom")) return r->M.ngeom;
  if (!strcmp(name, "nbody")) return r->M.nbody;
  if (!strcmp(name, "nv")) return r->M.nv;
  if (!strcmp(name, "ntree")) return r->M.ntree;
  if (!strcmp(name, "n_envs")) return r->n_envs;
  return -1;
}

}  // extern "C"
