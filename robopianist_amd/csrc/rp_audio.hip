// rp_audio.hip -- librp_audio.so: batched piano synthesis from the engine's key trace (include/audio/rp_audio.h).
//
// Three kernels, every workgroup one wave:
//   rp_audio_notes_kernel  one wave per env, lane = key (lane l also carries key 64 + l for l < 24).  The wave walks
//                          the substeps; per substep it ballots the onsets and allots list slots in (time, key) order
//                          with a prefix popcount; a lane keeps its open note's slot to patch t_off.  No atomics: the
//                          list order, and with it the summation order, is deterministic.
//   rp_audio_synth_kernel  grid (sample block, env).  The wave walks the env's list in chunks of RPA_CHUNK entries,
//                          compacts the ones audible in its block into LDS in list order (ballot + prefix popcount)
//                          and accumulates them (rp_audio.hpp: rpa_accumulate); a list with more audible notes than a
//                          chunk simply takes more rounds.  Rows are written coalesced.
//   rp_audio_pcm_kernel    one workgroup per env: max |wave| of the row (wave shuffles, then LDS), then the int16 row.
//                          No float atomics.
#include "rp_abi_host.hpp"
#include "rp_audio.hpp"

namespace {

#define RPA_PCM_THREADS 256

__global__ __launch_bounds__(RPA_THREADS) void rp_audio_notes_kernel(
    const unsigned int* __restrict__ trace, const int* __restrict__ lengths, int trace_substeps, double dt, int max_notes,
    int* __restrict__ key, double* __restrict__ t_on, double* __restrict__ t_off, int* __restrict__ velocity,
    int* __restrict__ count, int* __restrict__ dropped, int env_first) {
  const int env = env_first + (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  const int T = rpa_clamp_len(lengths[env], trace_substeps);
  const unsigned int* tr = trace + (size_t)env * trace_substeps * 4;
  const size_t nb = (size_t)env * max_notes;
  const unsigned long long below = (1ull << lane) - 1ull;
  const double t_end = (double)T * dt;
  int prev0 = 0, held0 = 0, slot0 = -1;   // key `lane`
  int prev1 = 0, held1 = 0, slot1 = -1;   // key 64 + lane (lanes 0..23)
  int n = 0, drop = 0;                    // wave-uniform
  for (int s = 0; s < T; s++) {
    const unsigned int w0 = tr[4 * s], w1 = tr[4 * s + 1], w2 = tr[4 * s + 2];
    const int pedal = (int)((w2 >> (RPA_PEDAL_BIT - 64)) & 1u);
    const int act0 = (int)(((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u);
    const int act1 = lane < RPA_N_KEYS - 64 ? (int)((w2 >> lane) & 1u) : 0;
    const double t = (double)(s + 1) * dt;
    const int ev0 = rpa_key_step(act0, pedal, prev0, held0);
    const int ev1 = rpa_key_step(act1, pedal, prev1, held1);
    if ((ev0 & 2) && slot0 >= 0) { t_off[nb + slot0] = t; slot0 = -1; }
    if ((ev1 & 2) && slot1 >= 0) { t_off[nb + slot1] = t; slot1 = -1; }
    const unsigned long long b0 = __ballot(ev0 & 1), b1 = __ballot(ev1 & 1);
    if (b0 | b1) {
      const int c0 = __popcll(b0), c1 = __popcll(b1);
      if (ev0 & 1) {
        const int i = n + __popcll(b0 & below);
        slot0 = i < max_notes ? i : -1;
        if (slot0 >= 0) { key[nb + i] = lane; t_on[nb + i] = t; t_off[nb + i] = t_end; velocity[nb + i] = 127; }
      }
      if (ev1 & 1) {
        const int i = n + c0 + __popcll(b1 & below);
        slot1 = i < max_notes ? i : -1;
        if (slot1 >= 0) { key[nb + i] = 64 + lane; t_on[nb + i] = t; t_off[nb + i] = t_end; velocity[nb + i] = 127; }
      }
      const int room = max_notes - n;
      const int kept = c0 + c1 < room ? c0 + c1 : room;
      drop += c0 + c1 - kept;
      n += kept;
    }
  }
  if (lane == 0) { count[env] = n; dropped[env] = drop; }
}

__global__ __launch_bounds__(RPA_THREADS) void rp_audio_synth_kernel(
    const RpaModel M, const int* __restrict__ key, const double* __restrict__ t_on, const double* __restrict__ t_off,
    const int* __restrict__ velocity, const int* __restrict__ count, const int* __restrict__ lengths, int substeps_cap,
    double dt, int n_cap, int max_notes, float* __restrict__ wave, int env_first) {
  __shared__ RpaVoice sv[RPA_CHUNK];
  const int env = env_first + (int)blockIdx.y;
  const int lane = (int)threadIdx.x;
  const int b0 = (int)blockIdx.x * RPA_BLOCK;   // (< n_cap <= 2e9: the host checked)
  const int ns = rpa_n_samples(M.sr, rpa_clamp_len(lengths[env], substeps_cap), dt, n_cap);
  float acc[RPA_R];
#pragma unroll
  for (int j = 0; j < RPA_R; j++) acc[j] = 0.f;
  if (b0 < ns) {   // (block-uniform: every lane meets every barrier)
    const int b1 = ns - b0 < RPA_BLOCK ? ns : b0 + RPA_BLOCK;
    const int cnt = rpa_clamp_len(count[env], max_notes);
    const size_t nb = (size_t)env * max_notes;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < cnt; base += RPA_CHUNK) {
      const int i = base + lane;
      bool audible = false;
      RpaVoice v;
      if (i < cnt) {
        const int k = key[nb + i];
        const double on = t_on[nb + i], off = t_off[nb + i];
        if (rpa_valid_note(k, on, off) && rpa_maybe_audible(M, on, off, b0, b1)) {
          rpa_stage(M, k, on, off, velocity[nb + i], v);
          audible = v.n_on < b1 && b0 < v.n_cut;
        }
      }
      const unsigned long long m = __ballot(audible);
      if (m == 0ull) continue;   // (wave-uniform)
      if (audible) sv[__popcll(m & below)] = v;
      __syncthreads();
      rpa_accumulate(M, sv, __popcll(m), b0 + lane, acc);
      __syncthreads();
    }
  }
  float* row = wave + (size_t)env * n_cap;
#pragma unroll
  for (int j = 0; j < RPA_R; j++) {
    const long long n = (long long)b0 + lane + j * RPA_THREADS;
    if (n < n_cap) row[n] = n < ns ? acc[j] : 0.f;
  }
}

__global__ __launch_bounds__(RPA_PCM_THREADS) void rp_audio_pcm_kernel(
    double sr, const int* __restrict__ lengths, int substeps_cap, double dt, int n_cap, const float* __restrict__ wave,
    short* __restrict__ pcm, int env_first) {
  __shared__ float part[RPA_PCM_THREADS / 64];
  const int env = env_first + (int)blockIdx.x;
  const int tid = (int)threadIdx.x;
  const int ns = rpa_n_samples(sr, rpa_clamp_len(lengths[env], substeps_cap), dt, n_cap);
  const float* row = wave + (size_t)env * n_cap;
  float m = 0.f;
  for (int n = tid; n < ns; n += RPA_PCM_THREADS) m = fmaxf(m, fabsf(row[n]));
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((tid & 63) == 0) part[tid >> 6] = m;
  __syncthreads();
  float peak = part[0];
#pragma unroll
  for (int w = 1; w < RPA_PCM_THREADS / 64; w++) peak = fmaxf(peak, part[w]);
  short* prow = pcm + (size_t)env * n_cap;
  for (int n = tid; n < n_cap; n += RPA_PCM_THREADS) prow[n] = n < ns ? rpa_pcm(row[n], peak) : (short)0;
}

}  // namespace

struct rp_audio {
  RpaTables tab;
  RpaModel M;   // device view
  int n_envs = 0, max_substeps = 0, max_notes = 0, device = 0;
  RpaPartial* d_part = nullptr;
};

extern "C" {

const char* rp_audio_last_error(void) { return g_err.c_str(); }

int rp_audio_create(const void* blob, size_t bytes, int n_envs, int max_substeps, int max_notes, int device,
                    rp_audio** out) {
  if (!out) return fail("rp_audio_create: out is NULL");
  *out = nullptr;
  if (n_envs <= 0) return fail("rp_audio_create: n_envs must be positive");
  if (max_substeps <= 0 || max_substeps > (1 << 26)) return fail("rp_audio_create: max_substeps must be in 1..2^26");
  if (max_notes <= 0 || max_notes > (1 << 24)) return fail("rp_audio_create: max_notes must be in 1..2^24");
  rp_audio* a = new rp_audio();
  const std::string err = a->tab.parse(blob, bytes);
  if (!err.empty()) { delete a; return fail("rp_audio_create: " + err); }
  a->n_envs = n_envs; a->max_substeps = max_substeps; a->max_notes = max_notes; a->device = device;
  CreateGuard<rp_audio> guard{a, rp_audio_destroy};
  HIP_OK_AS("rp_audio_create", "hipSetDevice", hipSetDevice(device));
  if (upload("rp_audio_create", &a->d_part, a->tab.part.data(), a->tab.part.size())) return -1;
  a->M = a->tab.view(a->d_part);
  *out = guard.release();
  return 0;
}

void rp_audio_destroy(rp_audio* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  free_all({a->d_part});
  delete a;
}

int rp_audio_notes_from_trace(rp_audio* a, const rp_audio_notes_args* args) {
  RP_HANDLE_HEAD(a, "rp_audio_notes_from_trace: handle is NULL");
  RP_ARGS_CHECK(rpa_check_notes_args(args, a->n_envs, a->max_substeps));
  HIP_OK(hipSetDevice(a->device));
  const rp_audio_notes& n = args->notes;
  hipLaunchKernelGGL(rp_audio_notes_kernel, dim3((unsigned)args->env_count), dim3(RPA_THREADS), 0,
                     (hipStream_t)args->hip_stream, args->trace, args->lengths, args->trace_substeps, args->dt,
                     a->max_notes, n.key, n.t_on, n.t_off, n.velocity, n.count, n.dropped, args->env_first);
  HIP_OK(hipGetLastError());
  return 0;
}

int rp_audio_synthesize(rp_audio* a, const rp_audio_synth_args* args) {
  RP_HANDLE_HEAD(a, "rp_audio_synthesize: handle is NULL");
  RP_ARGS_CHECK(rpa_check_synth_args(args, a->n_envs, a->max_substeps, a->tab.sr));
  HIP_OK(hipSetDevice(a->device));
  hipStream_t st = (hipStream_t)args->hip_stream;
  const rp_audio_notes& n = args->notes;
  const unsigned nblk = (unsigned)(((long long)args->n_cap + RPA_BLOCK - 1) / RPA_BLOCK);
  // the env is the grid's y index, which the device limits to 65535: larger batches go out in slices
  for (int first = 0; first < args->env_count; first += RPA_MAX_GRID_Y) {
    const int cnt = rpa_slice_count(args->env_count, first);
    hipLaunchKernelGGL(rp_audio_synth_kernel, dim3(nblk, (unsigned)cnt), dim3(RPA_THREADS), 0, st, a->M,
                       (const int*)n.key, (const double*)n.t_on, (const double*)n.t_off, (const int*)n.velocity,
                       (const int*)n.count, args->lengths, args->substeps_cap, args->dt, args->n_cap, a->max_notes,
                       args->wave, args->env_first + first);
    HIP_OK(hipGetLastError());
  }
  if (args->pcm) {
    hipLaunchKernelGGL(rp_audio_pcm_kernel, dim3((unsigned)args->env_count), dim3(RPA_PCM_THREADS), 0, st, a->M.sr,
                       args->lengths, args->substeps_cap, args->dt, args->n_cap, (const float*)args->wave, args->pcm,
                       args->env_first);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

int rp_audio_dim(const rp_audio* a, const char* name) {
  if (!a || !name) return -1;
  if (!strcmp(name, "n_envs")) return a->n_envs;
  if (!strcmp(name, "max_substeps")) return a->max_substeps;
  if (!strcmp(name, "max_notes")) return a->max_notes;
  if (!strcmp(name, "H")) return a->tab.H;
  if (!strcmp(name, "sample_rate")) return (int)(a->tab.sr + 0.5);
  if (!strcmp(name, "block_samples")) return RPA_BLOCK;
  if (!strcmp(name, "chunk_notes")) return RPA_CHUNK;
  return -1;
}

}  // extern "C"
