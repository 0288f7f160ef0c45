// rp_audio.hpp -- the synthesiser's routines (include/audio/rp_audio.h has the definition of the sound).
//
// Plain C++ behind RPA_HD, free of wave intrinsics: rp_audio.hip compiles it for gfx950, and the CPU tests compile
// the same text with g++ (tests/audio_reference.py), where rpa_notes_host / rpa_synthesize_host walk environments,
// sample blocks, threads and note chunks in the kernels' order.
//
// How a block is computed.  A block is RPA_BLOCK = RPA_THREADS x RPA_R samples; thread i owns the samples
// b0 + i + j RPA_THREADS, j < RPA_R, so a row is written coalesced.  For every voice-partial the thread evaluates the
// closed form once, at its first sample (phase frac(f_h u) in float64, one sincos, one exp), and then steps a damped
// phasor z <- z w, w = exp(-RPA_THREADS/(tau_h sr)) e^{i 2 pi f_h RPA_THREADS/sr}: four FMAs per sample.  The
// attack and release factors apply per voice.  Whether a sample lies before the onset, in the release or past the
// cut-off is decided by integer sample thresholds (rpa_stage) that reproduce the float64 comparisons of the
// definition exactly, so the silent stretches are exact zeros.
#pragma once

#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/audio/rp_audio.h"

#if defined(__HIPCC__)
#define RPA_HD __host__ __device__
#else
#define RPA_HD
#endif
#define RPA_INLINE RPA_HD inline __attribute__((always_inline))

#define RPA_N_KEYS 88
#define RPA_MAX_H 8
#define RPA_THREADS 64                      /* one wave per workgroup */
#define RPA_R 16                            /* samples per thread and block = length of one recurrence run */
#define RPA_BLOCK (RPA_THREADS * RPA_R)     /* samples per block */
#define RPA_CHUNK 64                        /* list entries staged per LDS chunk */
#define RPA_PEDAL_BIT 88
#define RPA_MAX_GRID_Y 65535
#define RPA_BLOB_MAGIC 0x55415052u          /* "RPAU" */
#define RPA_BLOB_VERSION 1u
#define RPA_MAX_TIME 1.0e6                  /* seconds: later notes do not sound (sample indices stay ints) */

struct RpaPartial {
  double f;        // f_h, Hz
  float amp;       // a_h, or 0 for a partial at or above 0.45 sr
  float inv_tau;   // 1/tau_h
  float wr, wi;    // the phasor step over RPA_THREADS samples
};

struct RpaModel {   // by value into the kernels; `part` is a device (or host) pointer
  int H;
  double sr;
  double rel_tail;        // 8 tau_rel
  float inv_tau_att, inv_tau_rel;
  float att_done;         // 18 tau_att: from there on 1 - exp(-u/tau_att) is 1 in float32
  float du;               // RPA_THREADS / sr
  const RpaPartial* part; // [88][RPA_MAX_H]
};

struct RpaTables {
  int H = 0;
  double sr = 0, tau_att = 0, tau_rel = 0;
  std::vector<RpaPartial> part;

  // blob: u32 magic, u32 version, i32 H, i32 0, then doubles: sr, tau_att, tau_rel, a[8], B[88], tau[88][8]
  std::string parse(const void* blob, size_t nb) {
    const size_t nd = 3 + RPA_MAX_H + RPA_N_KEYS + RPA_N_KEYS * RPA_MAX_H;
    if (!blob || nb != 16 + sizeof(double) * nd) return "audio blob has the wrong size";
    uint32_t head[4];
    memcpy(head, blob, 16);
    if (head[0] != RPA_BLOB_MAGIC || head[1] != RPA_BLOB_VERSION) return "not an audio blob of this version";
    H = (int)head[2];
    if (H < 1 || H > RPA_MAX_H) return "audio blob: H must be in 1..8";
    std::vector<double> d(nd);
    memcpy(d.data(), (const char*)blob + 16, sizeof(double) * nd);
    sr = d[0]; tau_att = d[1]; tau_rel = d[2];
    const double* a = &d[3];
    const double* B = a + RPA_MAX_H;
    const double* tau = B + RPA_N_KEYS;
    if (!(sr >= 1000.0 && sr <= 1.0e6)) return "audio blob: sample rate out of range";
    if (!(tau_att > 0 && tau_rel > 0 && std::isfinite(tau_att) && std::isfinite(tau_rel))) return "audio blob: tau_att and tau_rel must be positive";
    part.assign((size_t)RPA_N_KEYS * RPA_MAX_H, RpaPartial{0.0, 0.f, 1.f, 0.f, 0.f});
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < RPA_N_KEYS; k++) {
      if (!(B[k] >= 0 && std::isfinite(B[k]))) return "audio blob: B must be non-negative";
      const double f0 = 440.0 * std::pow(2.0, ((k + 21) - 69) / 12.0);
      for (int h = 1; h <= H; h++) {
        const double t = tau[k * RPA_MAX_H + h - 1];
        if (!(t > 0 && std::isfinite(t)) || !std::isfinite(a[h - 1])) return "audio blob: tau_h must be positive and a_h finite";
        RpaPartial& p = part[(size_t)k * RPA_MAX_H + h - 1];
        p.f = h * f0 * std::sqrt(1.0 + B[k] * h * h);
        p.amp = p.f >= 0.45 * sr ? 0.f : (float)a[h - 1];
        p.inv_tau = (float)(1.0 / t);
        const double dec = std::exp(-(double)RPA_THREADS / (t * sr));
        double cyc = p.f * RPA_THREADS / sr;
        cyc -= std::floor(cyc);
        p.wr = (float)(dec * std::cos(two_pi * cyc));
        p.wi = (float)(dec * std::sin(two_pi * cyc));
      }
    }
    return "";
  }

  RpaModel view(const RpaPartial* p) const {
    RpaModel M;
    M.H = H; M.sr = sr; M.rel_tail = 8.0 * tau_rel;
    M.inv_tau_att = (float)(1.0 / tau_att); M.inv_tau_rel = (float)(1.0 / tau_rel);
    M.att_done = (float)(18.0 * tau_att);
    M.du = (float)((double)RPA_THREADS / sr);
    M.part = p;
    return M;
  }
};

// ---- samples per environment -----------------------------------------------------------------------------------
RPA_INLINE int rpa_clamp_len(int T, int cap) { return T < 0 ? 0 : (T > cap ? cap : T); }

// ceil(sr (T dt + 1.0)), at most n_cap
RPA_INLINE int rpa_n_samples(double sr, int T, double dt, int n_cap) {
  const double n = ceil(sr * ((double)T * dt + 1.0));
  return n >= (double)n_cap ? n_cap : (int)n;
}

// ---- argument checks (host) ------------------------------------------------------------------------------------
inline std::string rpa_check_window(const char* who, int env_first, int env_count, int n_envs) {
  if (env_first < 0 || env_count < 1 || env_first > n_envs - env_count)
    return std::string(who) + ": env window [" + std::to_string(env_first) + ", +" + std::to_string(env_count) +
           ") is outside the " + std::to_string(n_envs) + " environments";
  return "";
}

inline std::string rpa_check_notes_args(const rp_audio_notes_args* a, int n_envs, int max_substeps) {
  const char* who = "rp_audio_notes_from_trace";
  if (!a) return std::string(who) + ": args is NULL";
  if (a->struct_size != sizeof(rp_audio_notes_args)) return std::string(who) + ": struct_size does not match this library's rp_audio_notes_args";
  if (!a->trace || !a->lengths) return std::string(who) + ": trace and lengths must not be NULL";
  const rp_audio_notes& n = a->notes;
  if (!n.key || !n.t_on || !n.t_off || !n.velocity || !n.count || !n.dropped) return std::string(who) + ": every array of the note list must be given";
  if (a->trace_substeps < 0 || a->trace_substeps > max_substeps)
    return std::string(who) + ": trace_substeps " + std::to_string(a->trace_substeps) + " exceeds max_substeps " + std::to_string(max_substeps);
  if (!(a->dt > 0) || !std::isfinite(a->dt)) return std::string(who) + ": dt must be positive";
  return rpa_check_window(who, a->env_first, a->env_count, n_envs);
}

inline std::string rpa_check_synth_args(const rp_audio_synth_args* a, int n_envs, int max_substeps, double sr) {
  const char* who = "rp_audio_synthesize";
  if (!a) return std::string(who) + ": args is NULL";
  if (a->struct_size != sizeof(rp_audio_synth_args)) return std::string(who) + ": struct_size does not match this library's rp_audio_synth_args";
  const rp_audio_notes& n = a->notes;
  if (!n.key || !n.t_on || !n.t_off || !n.velocity || !n.count) return std::string(who) + ": key, t_on, t_off, velocity and count of the note list must be given";
  if (!a->lengths || !a->wave) return std::string(who) + ": lengths and wave must not be NULL";
  if (a->substeps_cap < 0 || a->substeps_cap > max_substeps)
    return std::string(who) + ": substeps_cap " + std::to_string(a->substeps_cap) + " exceeds max_substeps " + std::to_string(max_substeps);
  if (!(a->dt > 0) || !std::isfinite(a->dt)) return std::string(who) + ": dt must be positive";
  const double need = ceil(sr * ((double)a->substeps_cap * a->dt + 1.0));
  if (!(need < 2.0e9)) return std::string(who) + ": the episode is too long for 32-bit sample indices";
  if (a->n_cap < (int)need) return std::string(who) + ": n_cap " + std::to_string(a->n_cap) + " is smaller than the " + std::to_string((long long)need) + " samples of substeps_cap substeps";
  if ((double)a->n_cap > 2.0e9) return std::string(who) + ": n_cap is too large for 32-bit sample indices";
  return rpa_check_window(who, a->env_first, a->env_count, n_envs);
}

inline int rpa_slice_count(int env_count, int first) {
  return env_count - first < RPA_MAX_GRID_Y ? env_count - first : RPA_MAX_GRID_Y;
}

// ---- notes from the trace ----------------------------------------------------------------------------------------
// One key, one substep.  Returns bit 0: a note starts, bit 1: the open note (if any) is released now.
RPA_INLINE int rpa_key_step(int act, int pedal, int& prev_act, int& held) {
  const int onset = act & (prev_act ^ 1);
  const int now = act | (held & pedal);
  const int close = held & (onset | (now ^ 1));
  prev_act = act;
  held = now;
  return onset | (close << 1);
}

RPA_INLINE int rpa_trace_bit(const unsigned int* w, int bit) { return (int)((w[bit >> 5] >> (bit & 31)) & 1u); }

// The notes of one environment on the host, in the kernel's order.
inline void rpa_notes_host(const unsigned int* trace, int T, double dt, int max_notes, int* key, double* t_on,
                           double* t_off, int* velocity, int* count, int* dropped) {
  int prev[RPA_N_KEYS] = {0}, held[RPA_N_KEYS] = {0}, slot[RPA_N_KEYS];
  for (int k = 0; k < RPA_N_KEYS; k++) slot[k] = -1;
  int n = 0, drop = 0;
  for (int s = 0; s < T; s++) {
    const unsigned int* w = trace + (size_t)s * 4;
    const int pedal = rpa_trace_bit(w, RPA_PEDAL_BIT);
    const double t = (double)(s + 1) * dt;
    for (int k = 0; k < RPA_N_KEYS; k++) {
      const int ev = rpa_key_step(rpa_trace_bit(w, k), pedal, prev[k], held[k]);
      if ((ev & 2) && slot[k] >= 0) { t_off[slot[k]] = t; slot[k] = -1; }
      if (ev & 1) {
        if (n < max_notes) {
          key[n] = k; t_on[n] = t; t_off[n] = (double)T * dt; velocity[n] = 127;
          slot[k] = n++;
        } else {
          slot[k] = -1; drop++;
        }
      }
    }
  }
  *count = n;
  *dropped = drop;
}

// ---- one voice, staged for a block -----------------------------------------------------------------------------
struct RpaVoice {
  double t_on;
  double u_off;     // t_off - t_on
  int n_on;         // first sample with u >= 0
  int n_off;        // first sample with u >= u_off (the release has begun)
  int n_cut;        // first sample with u >= u_off + 8 tau_rel (silent from here on)
  int key;
  float g;
  int pad_;
};

// The smallest n >= 0 with fl(fl(n/sr) - t_on) >= lim: the left side does not decrease with n, so the threshold
// states the float64 comparison of the definition for every sample at once.
RPA_INLINE int rpa_first_sample(double sr, double t_on, double lim) {
  double e = ceil((t_on + lim) * sr);
  if (!(e >= 0.0)) e = 0.0;
  if (e > 2.0e9) e = 2.0e9;
  int n = (int)e;
  for (int i = 0; i < 4 && n > 0 && ((double)(n - 1) / sr - t_on) >= lim; i++) n--;
  for (int i = 0; i < 4 && !(((double)n / sr - t_on) >= lim); i++) n++;
  return n;
}

// false: the note never sounds (see the header)
RPA_INLINE bool rpa_valid_note(int key, double t_on, double t_off) {
  return key >= 0 && key < RPA_N_KEYS && t_on >= 0.0 && t_off >= t_on && t_off < RPA_MAX_TIME;
}

// cheap superset of "audible in samples [b0, b1)", before the thresholds are worked out
RPA_INLINE bool rpa_maybe_audible(const RpaModel& M, double t_on, double t_off, int b0, int b1) {
  return t_on * M.sr < (double)b1 + 2.0 && (t_off + M.rel_tail) * M.sr > (double)b0 - 2.0;
}

RPA_INLINE void rpa_stage(const RpaModel& M, int key, double t_on, double t_off, int velocity, RpaVoice& v) {
  v.t_on = t_on;
  v.u_off = t_off - t_on;
  v.n_on = rpa_first_sample(M.sr, t_on, 0.0);
  v.n_off = rpa_first_sample(M.sr, t_on, v.u_off);
  v.n_cut = rpa_first_sample(M.sr, t_on, v.u_off + M.rel_tail);
  v.key = key;
  const float q = (float)velocity / 127.0f;
  v.g = q * q;
  v.pad_ = 0;
}

RPA_INLINE void rpa_sincos_cycles(float ph, float& s, float& c) {   // of 2 pi ph, ph in [0, 1]
#if defined(__HIP_DEVICE_COMPILE__)
  sincospif(2.0f * ph, &s, &c);   // (no large-argument reduction, which would cost scratch)
#else
  const float x = 6.2831855f * ph;
  s = sinf(x); c = cosf(x);
#endif
}

// Adds the voices vs[0..nv) to acc[j], the samples n0 + j RPA_THREADS, in list order.
RPA_INLINE void rpa_accumulate(const RpaModel& M, const RpaVoice* vs, int nv, int n0, float* acc) {
  const double t0 = (double)n0 / M.sr;
  const int n_last = n0 + (RPA_R - 1) * RPA_THREADS;
  for (int i = 0; i < nv; i++) {
    const RpaVoice v = vs[i];
    if (n_last < v.n_on || n0 >= v.n_cut) continue;
    const double u0d = t0 - v.t_on;
    const float u0 = (float)u0d;
    float S[RPA_R];
#pragma unroll
    for (int j = 0; j < RPA_R; j++) S[j] = 0.f;
    const RpaPartial* P = M.part + (size_t)v.key * RPA_MAX_H;
    for (int h = 0; h < M.H; h++) {
      const RpaPartial p = P[h];
      if (p.amp == 0.f) continue;
      const double x = p.f * u0d;
      float s, c;
      rpa_sincos_cycles((float)(x - floor(x)), s, c);
      const float A = p.amp * expf(-u0 * p.inv_tau);
      float zr = A * c, zi = A * s;
      S[0] += zi;
#pragma unroll
      for (int j = 1; j < RPA_R; j++) {
        const float nr = zr * p.wr - zi * p.wi;
        zi = zr * p.wi + zi * p.wr;
        zr = nr;
        S[j] += zi;
      }
    }
    const bool attack = u0 < M.att_done;           // the run's first sample decides for the run: u only grows
    const bool release = n_last >= v.n_off;
    const float x0 = (float)(u0d - v.u_off);
#pragma unroll
    for (int j = 0; j < RPA_R; j++) {
      const int n = n0 + j * RPA_THREADS;
      float gain = v.g;
      if (attack) {   // (u is small here: formed in float64 like the definition's, a float32 sum would lose its bits)
        const float u = (float)((double)n / M.sr - v.t_on);
        if (u < M.att_done) gain *= 1.0f - expf(-u * M.inv_tau_att);
      }
      if (release && n >= v.n_off) gain *= expf(-fmaf((float)j, M.du, x0) * M.inv_tau_rel);
      if (n >= v.n_on && n < v.n_cut) acc[j] += gain * S[j];
    }
  }
}

// The quotient first: w / peak is exactly +-1 at the peak, so the loudest sample is exactly +-32767 (the product first,
// 32767 w rounded and then divided by peak, can come out just below 32767 and truncate to 32766).
RPA_INLINE short rpa_pcm(float w, float peak) {
  return peak > 0.f ? (short)truncf(32767.0f * (w / peak)) : (short)0;
}

// ---- the whole call on the host (tests) -------------------------------------------------------------------------
inline void rpa_synthesize_host(const RpaModel& M, const rp_audio_synth_args* a, int max_notes) {
  for (int env = a->env_first; env < a->env_first + a->env_count; env++) {
    const int ns = rpa_n_samples(M.sr, rpa_clamp_len(a->lengths[env], a->substeps_cap), a->dt, a->n_cap);
    const size_t nb = (size_t)env * max_notes;
    const int cnt = rpa_clamp_len(a->notes.count[env], max_notes);
    float* row = a->wave + (size_t)env * a->n_cap;
    float peak = 0.f;
    for (int b0 = 0; b0 < a->n_cap; b0 += RPA_BLOCK) {
      const int b1 = b0 + RPA_BLOCK < ns ? b0 + RPA_BLOCK : ns;
      std::vector<float> acc((size_t)RPA_BLOCK, 0.f);   // [thread][j]
      if (b0 < ns) {
        for (int base = 0; base < cnt; base += RPA_CHUNK) {
          RpaVoice sv[RPA_CHUNK];
          int nv = 0;
          for (int i = base; i < cnt && i < base + RPA_CHUNK; i++) {
            const int key = a->notes.key[nb + i];
            const double on = a->notes.t_on[nb + i], off = a->notes.t_off[nb + i];
            if (!rpa_valid_note(key, on, off) || !rpa_maybe_audible(M, on, off, b0, b1)) continue;
            RpaVoice v;
            rpa_stage(M, key, on, off, a->notes.velocity[nb + i], v);
            if (v.n_on < b1 && b0 < v.n_cut) sv[nv++] = v;
          }
          for (int t = 0; t < RPA_THREADS; t++) rpa_accumulate(M, sv, nv, b0 + t, &acc[(size_t)t * RPA_R]);
        }
      }
      for (int t = 0; t < RPA_THREADS; t++)
        for (int j = 0; j < RPA_R; j++) {
          const int n = b0 + t + j * RPA_THREADS;
          if (n >= a->n_cap) continue;
          const float w = n < ns ? acc[(size_t)t * RPA_R + j] : 0.f;
          row[n] = w;
          peak = fmaxf(peak, fabsf(w));
        }
    }
    if (a->pcm) {
      short* prow = a->pcm + (size_t)env * a->n_cap;
      for (int n = 0; n < a->n_cap; n++) prow[n] = n < ns ? rpa_pcm(row[n], peak) : (short)0;
    }
  }
}
