// rp_hear.hip -- librp_hear.so: what every environment hears, per step (include/audio/rp_hear.h).
//
// Three kernels:
//   rp_hear_track_kernel     one wave per env, lane = key (lane l also carries key 64 + l for l < 24), as the
//                            synthesiser's notes kernel.  A lane keeps its keys' two slots and the rule's two bits in
//                            registers over the rows of the call; the state words are ballots, `forgotten` a wave sum.
//   rp_hear_window_kernel    grid (sample block of the window, env), one wave.  The 176 bank entries are staged in
//                            three rounds of 64: the ones that can sound in the block are compacted into LDS in
//                            summation order (ballot + prefix popcount) and accumulated by rpa_accumulate.
//   rp_hear_analysis_kernel  the GEMM [E x W] x [W x 2B] on v_mfma_f32_16x16x4_f32 with the magnitude as epilogue.  A
//                            workgroup of four waves owns RPH_TILE_E envs x RPH_TILE_B bins; a wave owns 16 envs and
//                            four accumulators (cos and sin of two column tiles of 16 bins), so that the cosine and the
//                            sine sum of one (env, bin) meet in the same lane and register.  The window and both
//                            tables go through LDS RPH_TILE_K samples at a time, the next stage's loads in flight under the
//                            current stage's MFMAs; rows past the env window and bins past B are loaded as zeros and
//                            never stored.
#include "rp_abi_host.hpp"
#include "rp_hear.hpp"

namespace {

#define RPH_ANALYSIS_THREADS 256

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(RPA_THREADS) void rp_hear_track_kernel(
    double rel_tail, const unsigned int* __restrict__ trace, int n_sub, const int* __restrict__ pedal,
    const int* __restrict__ restart, double dt, double* __restrict__ t_on, double* __restrict__ t_off,
    int* __restrict__ state, int env_first) {
  const int env = env_first + (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  const bool two = lane < RPA_N_KEYS - 64;
  int* st = state + (size_t)env * RPH_STATE;
  if (restart && restart[env] != 0) {   // (wave-uniform)
    RphKey E;
    E.on0 = E.off0 = E.on1 = E.off1 = -1.0;
    rph_store_key(t_on, t_off, env, lane, E);
    if (two) rph_store_key(t_on, t_off, env, 64 + lane, E);
    if (lane < RPH_STATE) st[lane] = 0;
    return;
  }
  const int env_pedal = pedal ? (pedal[env] != 0 ? 1 : 0) : 0;
  const unsigned int* tr = trace + (size_t)env * n_sub * 4;
  const int T0 = st[6];
  RphKey K0, K1;
  rph_load_key(t_on, t_off, st, env, lane, K0);
  if (two) {
    rph_load_key(t_on, t_off, st, env, 64 + lane, K1);
  } else {
    K1.on0 = K1.off0 = K1.on1 = K1.off1 = -1.0;
    K1.prev = K1.held = 0;
  }
  int forgot = 0;
  for (int s = 0; s < n_sub; s++) {
    const unsigned int w0 = tr[4 * s], w1 = tr[4 * s + 1], w2 = tr[4 * s + 2];
    const int ped = (int)((w2 >> (RPA_PEDAL_BIT - 64)) & 1u) | env_pedal;
    const int act0 = (int)(((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u);
    const int act1 = two ? (int)((w2 >> lane) & 1u) : 0;
    const double t = (double)(T0 + s + 1) * dt;
    forgot += rph_key_row(K0, act0, ped, t, rel_tail);
    forgot += rph_key_row(K1, act1, ped, t, rel_tail);
  }
  const double t_end = (double)(T0 + n_sub) * dt;
  rph_key_end(K0, t_end);
  rph_key_end(K1, t_end);
  const int forgotten = st[7];   // (read before any lane writes the state)
  const unsigned long long a0 = __ballot(K0.prev), a1 = __ballot(K1.prev);
  const unsigned long long h0 = __ballot(K0.held), h1 = __ballot(K1.held);
  for (int d = 32; d >= 1; d >>= 1) forgot += __shfl_xor(forgot, d);
  rph_store_key(t_on, t_off, env, lane, K0);
  if (two) rph_store_key(t_on, t_off, env, 64 + lane, K1);
  if (lane == 0) {
    st[0] = (int)(unsigned)(a0 & 0xFFFFFFFFull); st[1] = (int)(unsigned)(a0 >> 32); st[2] = (int)(unsigned)(a1 & 0xFFFFFFull);
    st[3] = (int)(unsigned)(h0 & 0xFFFFFFFFull); st[4] = (int)(unsigned)(h0 >> 32); st[5] = (int)(unsigned)(h1 & 0xFFFFFFull);
    st[6] = T0 + n_sub;
    st[7] = forgotten + forgot;
  }
}

__global__ __launch_bounds__(RPA_THREADS) void rp_hear_window_kernel(
    const RpaModel M, int W, const double* __restrict__ t_on, const double* __restrict__ t_off,
    const int* __restrict__ state, double dt, float* __restrict__ window, int env_first) {
  __shared__ RpaVoice sv[RPA_CHUNK];
  const int env = env_first + (int)blockIdx.y;
  const int lane = (int)threadIdx.x;
  const int off = (int)blockIdx.x * RPA_BLOCK;   // (< W: the grid has ceil(W / RPA_BLOCK) blocks)
  const int b0 = rph_last_sample(M.sr, state[(size_t)env * RPH_STATE + 6], dt) - W + 1 + off;
  const int b1 = b0 + (W - off < RPA_BLOCK ? W - off : RPA_BLOCK);
  const unsigned long long below = (1ull << lane) - 1ull;
  float acc[RPA_R];
#pragma unroll
  for (int j = 0; j < RPA_R; j++) acc[j] = 0.f;
  for (int base = 0; base < RPH_VOICES; base += RPA_CHUNK) {
    RpaVoice v;
    const bool audible = base + lane < RPH_VOICES && rph_stage(M, t_on, t_off, env, base + lane, b0, b1, v);
    const unsigned long long m = __ballot(audible);
    if (m == 0ull) continue;   // (wave-uniform)
    if (audible) sv[__popcll(m & below)] = v;
    __syncthreads();
    rpa_accumulate(M, sv, __popcll(m), b0 + lane, acc);
    __syncthreads();
  }
  float* row = window + (size_t)env * W;
#pragma unroll
  for (int j = 0; j < RPA_R; j++) {
    const int i = off + lane + j * RPA_THREADS;
    if (i < W) row[i] = acc[j];
  }
}

__global__ __launch_bounds__(RPH_ANALYSIS_THREADS) void rp_hear_analysis_kernel(
    const float* __restrict__ window, const float* __restrict__ C, const float* __restrict__ S, int W, int B,
    int env_first, int env_end, float* __restrict__ spectrum) {
  __shared__ float sx[RPH_TILE_E * RPH_X_PITCH];            // [env][k]
  __shared__ float st[2][RPH_TILE_B / 16][RPH_TILE_K][16];  // [cos | sin][column tile][k][bin]
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e0 = env_first + (int)blockIdx.y * RPH_TILE_E;
  const int b0 = (int)blockIdx.x * RPH_TILE_B;
  const int r16 = lane & 15, kq = lane >> 4;   // the operand maps of the 16x16x4 form: A[r16][kq], B[kq][r16]
  f32x4 acc[2][RPH_TILE_B / 16];
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int c = 0; c < RPH_TILE_B / 16; c++) acc[q][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tb = tid & (RPH_TILE_B - 1), tk = tid / RPH_TILE_B;   // this thread's bin and first k of the table tiles
  const bool bin_ok = b0 + tb < B;
  // The next stage's values are loaded into registers before the MFMAs of the current one, so that the loads' latency
  // runs under them; the order of the sums does not change.
  float px[RPH_TILE_E / 4], pc[RPH_TILE_K * RPH_TILE_B / RPH_ANALYSIS_THREADS], ps[RPH_TILE_K * RPH_TILE_B / RPH_ANALYSIS_THREADS];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < RPH_TILE_E / 4; i++) {
      const int env = e0 + wave + 4 * i;
      px[i] = env < env_end ? window[(size_t)env * W + k0 + lane] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < RPH_TILE_K * RPH_TILE_B / RPH_ANALYSIS_THREADS; i++) {
      const size_t g = (size_t)(k0 + tk + (RPH_ANALYSIS_THREADS / RPH_TILE_B) * i) * B + b0 + tb;
      pc[i] = bin_ok ? C[g] : 0.f;
      ps[i] = bin_ok ? S[g] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < W; k0 += RPH_TILE_K) {   // (W is a multiple of RPH_TILE_K = 64)
#pragma unroll
    for (int i = 0; i < RPH_TILE_E / 4; i++) sx[(wave + 4 * i) * RPH_X_PITCH + lane] = px[i];
#pragma unroll
    for (int i = 0; i < RPH_TILE_K * RPH_TILE_B / RPH_ANALYSIS_THREADS; i++) {
      const int k = tk + (RPH_ANALYSIS_THREADS / RPH_TILE_B) * i;
      st[0][tb >> 4][k][tb & 15] = pc[i];
      st[1][tb >> 4][k][tb & 15] = ps[i];
    }
    __syncthreads();
    if (k0 + RPH_TILE_K < W) fetch(k0 + RPH_TILE_K);   // (block-uniform)
#pragma unroll 4
    for (int kk = 0; kk < RPH_TILE_K; kk += 4) {
      const float a = sx[(wave * 16 + r16) * RPH_X_PITCH + kk + kq];
#pragma unroll
      for (int c = 0; c < RPH_TILE_B / 16; c++) {
        acc[0][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, st[0][c][kk + kq][r16], acc[0][c], 0, 0, 0);
        acc[1][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, st[1][c][kk + kq][r16], acc[1][c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // C/D map: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int c = 0; c < RPH_TILE_B / 16; c++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int env = e0 + wave * 16 + 4 * kq + reg, b = b0 + 16 * c + r16;
      if (env < env_end && b < B) spectrum[(size_t)env * B + b] = rph_magnitude(acc[0][c][reg], acc[1][c][reg]);
    }
}

}  // namespace

struct rp_hear {
  RpaTables tab;
  RphAnalysis ana;
  RpaModel M;   // device view
  int n_envs = 0, max_substeps = 0, device = 0;
  RpaPartial* d_part = nullptr;
  float* d_C = nullptr;
  float* d_S = nullptr;
  float* d_window = nullptr;   // [n_envs][W], for calls without a window of their own
};

extern "C" {

const char* rp_hear_last_error(void) { return g_err.c_str(); }

int rp_hear_create(const void* audio_blob, size_t audio_bytes, const void* analysis_blob, size_t analysis_bytes,
                   int n_envs, int max_substeps_per_call, int device, rp_hear** out) {
  if (!out) return fail("rp_hear_create: out is NULL");
  *out = nullptr;
  if (n_envs <= 0 || n_envs > (1 << 21)) return fail("rp_hear_create: n_envs must be in 1..2^21");
  if (max_substeps_per_call <= 0 || max_substeps_per_call > (1 << 20)) return fail("rp_hear_create: max_substeps_per_call must be in 1..2^20");
  rp_hear* h = new rp_hear();
  std::string err = h->tab.parse(audio_blob, audio_bytes);
  if (err.empty()) err = h->ana.parse(analysis_blob, analysis_bytes);
  if (!err.empty()) { delete h; return fail("rp_hear_create: " + err); }
  h->n_envs = n_envs; h->max_substeps = max_substeps_per_call; h->device = device;
  CreateGuard<rp_hear> guard{h, rp_hear_destroy};
  HIP_OK_AS("rp_hear_create", "hipSetDevice", hipSetDevice(device));
  if (upload("rp_hear_create", &h->d_part, h->tab.part.data(), h->tab.part.size())) return -1;
  if (upload("rp_hear_create", &h->d_C, h->ana.C.data(), h->ana.C.size())) return -1;
  if (upload("rp_hear_create", &h->d_S, h->ana.S.data(), h->ana.S.size())) return -1;
  HIP_OK_AS("rp_hear_create", "hipMalloc", hipMalloc(&h->d_window, sizeof(float) * (size_t)n_envs * h->ana.W));
  h->M = h->tab.view(h->d_part);
  *out = guard.release();
  return 0;
}

void rp_hear_destroy(rp_hear* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  free_all({h->d_part, h->d_C, h->d_S, h->d_window});
  delete h;
}

int rp_hear_track(rp_hear* h, const rp_hear_track_args* args) {
  RP_HANDLE_HEAD(h, "rp_hear_track: handle is NULL");
  RP_ARGS_CHECK(rph_check_track_args(args, h->n_envs, h->max_substeps));
  HIP_OK(hipSetDevice(h->device));
  hipLaunchKernelGGL(rp_hear_track_kernel, dim3((unsigned)args->env_count), dim3(RPA_THREADS), 0,
                     (hipStream_t)args->hip_stream, h->M.rel_tail, args->trace, args->n_sub, args->pedal, args->restart,
                     args->dt, args->bank.t_on, args->bank.t_off, args->bank.state, args->env_first);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_hear_spectrum(rp_hear* h, const rp_hear_spectrum_args* args) {
  RP_HANDLE_HEAD(h, "rp_hear_spectrum: handle is NULL");
  RP_ARGS_CHECK(rph_check_spectrum_args(args, h->n_envs));
  HIP_OK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)args->hip_stream;
  const int W = h->ana.W, B = h->ana.B;
  float* window = args->window ? args->window : h->d_window;
  const unsigned nblk = (unsigned)((W + RPA_BLOCK - 1) / RPA_BLOCK);
  // the env is the grid's y index, which the device limits to 65535: larger batches go out in slices
  for (int first = 0; first < args->env_count; first += RPA_MAX_GRID_Y) {
    const int cnt = rpa_slice_count(args->env_count, first);
    hipLaunchKernelGGL(rp_hear_window_kernel, dim3(nblk, (unsigned)cnt), dim3(RPA_THREADS), 0, st, h->M, W,
                       (const double*)args->bank.t_on, (const double*)args->bank.t_off, (const int*)args->bank.state,
                       args->dt, window, args->env_first + first);
    HIP_OK(hipGetLastError());
  }
  const unsigned gx = (unsigned)((B + RPH_TILE_B - 1) / RPH_TILE_B);
  const unsigned gy = (unsigned)((args->env_count + RPH_TILE_E - 1) / RPH_TILE_E);   // (<= 2^21 / 64: create checked n_envs)
  hipLaunchKernelGGL(rp_hear_analysis_kernel, dim3(gx, gy), dim3(RPH_ANALYSIS_THREADS), 0, st, (const float*)window,
                     (const float*)h->d_C, (const float*)h->d_S, W, B, args->env_first,
                     args->env_first + args->env_count, args->spectrum);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_hear_dim(const rp_hear* h, const char* name) {
  if (!h || !name) return -1;
  if (!strcmp(name, "n_envs")) return h->n_envs;
  if (!strcmp(name, "max_substeps_per_call")) return h->max_substeps;
  if (!strcmp(name, "W")) return h->ana.W;
  if (!strcmp(name, "B")) return h->ana.B;
  if (!strcmp(name, "H")) return h->tab.H;
  if (!strcmp(name, "sample_rate")) return (int)(h->tab.sr + 0.5);
  if (!strcmp(name, "tile_envs")) return RPH_TILE_E;
  if (!strcmp(name, "tile_bins")) return RPH_TILE_B;
  return -1;
}

}  // extern "C"
