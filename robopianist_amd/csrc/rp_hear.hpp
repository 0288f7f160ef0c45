// rp_hear.hpp -- the routines of the audio observation (include/audio/rp_hear.h has the definition).
//
// Plain C++ behind RPA_HD, free of wave intrinsics, on top of rp_audio.hpp: the blob parser, the partial table, the note
// rule of one key (rpa_key_step) and the evaluation of a voice (rpa_stage, rpa_accumulate) are the synthesiser's and
// are not restated here.  rp_hear.hip compiles this for gfx950, and the CPU tests compile the same text with g++
// (tests/hear_reference.py), where rph_track_host / rph_window_host / rph_analysis_host walk environments, sample
// blocks, threads and voices in the kernels' order.
//
// The window.  Its W samples start at n_start = N - W + 1 (negative early in an episode) and are cut into the
// synthesiser's blocks of RPA_BLOCK samples from there: thread i of block b owns n_start + b RPA_BLOCK + i +
// j RPA_THREADS, j < RPA_R, and evaluates them exactly as the synthesiser does (closed form at its first sample, then
// the damped phasor; integer thresholds from rpa_stage, so silent stretches are exact zeros).  The candidates are
// the 176 slots of the bank in the order key ascending, slot 1 then slot 0; the ones that cannot sound in the block
// are skipped before any arithmetic.
//
// The analysis.  spectrum = |[x C, x S]| is a GEMM [E x W] x [W x 2B]; per output element it is the fma chain
// c <- fma(x_j, C[j][b], c) over j ascending from c = 0, which is what v_mfma_f32_16x16x4_f32 computes and what
// rph_analysis_host restates.
#pragma once

#include "rp_audio.hpp"

#include "../../include/audio/rp_hear.h"

#define RPH_SLOTS 2
#define RPH_VOICES (RPA_N_KEYS * RPH_SLOTS)   /* bank entries per environment */
#define RPH_STATE 8                           /* state words per environment */
#define RPH_MIN_W 64
#define RPH_MAX_W 4096
#define RPH_MAX_B 128
#define RPH_BLOB_MAGIC 0x41485052u            /* "RPHA" */
#define RPH_BLOB_VERSION 1u
#define RPH_MAX_SAMPLE 2.0e9                  /* N is capped here (sample indices stay ints) */
#define RPH_TILE_E 64                         /* analysis: environments per workgroup (4 waves x 16 rows) */
#define RPH_TILE_B 32                         /* bins per workgroup (2 column tiles of 16) */
#define RPH_TILE_K 64                         /* window samples per LDS stage */
#define RPH_X_PITCH 68                        /* floats per row of the staged window: 16 rows x 4 k hit 64 distinct banks */

struct RphAnalysis {
  int W = 0, B = 0;
  std::vector<float> C, S;   // [W][B]

  // blob: u32 magic, u32 version, i32 W, i32 B, then float32 C[W][B], S[W][B]
  std::string parse(const void* blob, size_t nb) {
    if (!blob || nb < 16) return "analysis blob has the wrong size";
    uint32_t head[4];
    memcpy(head, blob, 16);
    if (head[0] != RPH_BLOB_MAGIC || head[1] != RPH_BLOB_VERSION) return "not an analysis blob of this version";
    const int w = (int)head[2], b = (int)head[3];
    if (w < RPH_MIN_W || w > RPH_MAX_W || w % 64 != 0) return "analysis blob: W must be a multiple of 64 in 64..4096, got " + std::to_string(w);
    if (b < 1 || b > RPH_MAX_B) return "analysis blob: B must be in 1..128, got " + std::to_string(b);
    const size_t n = (size_t)w * b;
    if (nb != 16 + 2 * n * sizeof(float)) return "analysis blob has the wrong size";
    W = w; B = b;
    C.resize(n); S.resize(n);
    memcpy(C.data(), (const char*)blob + 16, n * sizeof(float));
    memcpy(S.data(), (const char*)blob + 16 + n * sizeof(float), n * sizeof(float));
    return "";
  }
};

// ---- argument checks (host) ------------------------------------------------------------------------------------
inline std::string rph_check_bank(const char* who, const rp_hear_bank& b) {
  if (!b.t_on || !b.t_off || !b.state) return std::string(who) + ": t_on, t_off and state of the bank must be given";
  return "";
}

inline std::string rph_check_track_args(const rp_hear_track_args* a, int n_envs, int max_substeps) {
  const char* who = "rp_hear_track";
  if (!a) return std::string(who) + ": args is NULL";
  if (a->struct_size != sizeof(rp_hear_track_args)) return std::string(who) + ": struct_size does not match this library's rp_hear_track_args";
  if (a->n_sub < 0 || a->n_sub > max_substeps)
    return std::string(who) + ": n_sub " + std::to_string(a->n_sub) + " exceeds max_substeps_per_call " + std::to_string(max_substeps);
  if (!a->trace && a->n_sub > 0) return std::string(who) + ": trace must not be NULL";
  const std::string err = rph_check_bank(who, a->bank);
  if (!err.empty()) return err;
  if (!(a->dt > 0) || !std::isfinite(a->dt)) return std::string(who) + ": dt must be positive";
  return rpa_check_window(who, a->env_first, a->env_count, n_envs);
}

inline std::string rph_check_spectrum_args(const rp_hear_spectrum_args* a, int n_envs) {
  const char* who = "rp_hear_spectrum";
  if (!a) return std::string(who) + ": args is NULL";
  if (a->struct_size != sizeof(rp_hear_spectrum_args)) return std::string(who) + ": struct_size does not match this library's rp_hear_spectrum_args";
  const std::string err = rph_check_bank(who, a->bank);
  if (!err.empty()) return err;
  if (!a->spectrum) return std::string(who) + ": spectrum must not be NULL";
  if (!(a->dt > 0) || !std::isfinite(a->dt)) return std::string(who) + ": dt must be positive";
  return rpa_check_window(who, a->env_first, a->env_count, n_envs);
}

// ---- the tracker -------------------------------------------------------------------------------------------------
struct RphKey {        // one key of the bank, in registers
  double on0, off0;    // slot 0: the newest note
  double on1, off1;    // slot 1: the one before
  int prev, held;      // rpa_key_step's state
};

RPA_INLINE size_t rph_slot(int env, int key, int slot) { return ((size_t)env * RPA_N_KEYS + key) * RPH_SLOTS + slot; }

RPA_INLINE void rph_load_key(const double* t_on, const double* t_off, const int* st, int env, int key, RphKey& K) {
  K.on0 = t_on[rph_slot(env, key, 0)]; K.off0 = t_off[rph_slot(env, key, 0)];
  K.on1 = t_on[rph_slot(env, key, 1)]; K.off1 = t_off[rph_slot(env, key, 1)];
  K.prev = (int)(((unsigned)st[key >> 5] >> (key & 31)) & 1u);
  K.held = (int)(((unsigned)st[3 + (key >> 5)] >> (key & 31)) & 1u);
}

RPA_INLINE void rph_store_key(double* t_on, double* t_off, int env, int key, const RphKey& K) {
  t_on[rph_slot(env, key, 0)] = K.on0; t_off[rph_slot(env, key, 0)] = K.off0;
  t_on[rph_slot(env, key, 1)] = K.on1; t_off[rph_slot(env, key, 1)] = K.off1;
}

// One key, one row, at event time t.  A note is open exactly while `held` is set (it is set by an onset and cleared by
// the release), so the open note is always slot 0.  Returns 1 if a voice that would still sound was pushed out.
RPA_INLINE int rph_key_row(RphKey& K, int act, int pedal, double t, double rel_tail) {
  const int ev = rpa_key_step(act, pedal, K.prev, K.held);
  int forgot = 0;
  if (ev & 2) K.off0 = t;
  if (ev & 1) {
    forgot = (K.on1 >= 0.0 && K.off1 + rel_tail > t) ? 1 : 0;
    K.on1 = K.on0; K.off1 = K.off0;
    K.on0 = t; K.off0 = t;
  }
  return forgot;
}

// after the last row: an open note is released at T dt, as a note still open at T_e in rp_audio.h
RPA_INLINE void rph_key_end(RphKey& K, double t_end) { if (K.held) K.off0 = t_end; }

RPA_INLINE int rph_row_pedal(const unsigned int* w) { return (int)((w[RPA_PEDAL_BIT >> 5] >> (RPA_PEDAL_BIT & 31)) & 1u); }

inline void rph_track_host(const RpaModel& M, const rp_hear_track_args* a) {
  for (int env = a->env_first; env < a->env_first + a->env_count; env++) {
    int* st = a->bank.state + (size_t)env * RPH_STATE;
    if (a->restart && a->restart[env] != 0) {
      for (int k = 0; k < RPA_N_KEYS; k++)
        for (int s = 0; s < RPH_SLOTS; s++) a->bank.t_on[rph_slot(env, k, s)] = a->bank.t_off[rph_slot(env, k, s)] = -1.0;
      for (int i = 0; i < RPH_STATE; i++) st[i] = 0;
      continue;
    }
    const int env_pedal = a->pedal && a->pedal[env] != 0;
    const unsigned int* tr = a->trace + (size_t)env * a->n_sub * 4;
    const int T0 = st[6];
    int forgotten = st[7];
    unsigned int act_w[3] = {0, 0, 0}, held_w[3] = {0, 0, 0};
    for (int k = 0; k < RPA_N_KEYS; k++) {
      RphKey K;
      rph_load_key(a->bank.t_on, a->bank.t_off, st, env, k, K);
      for (int s = 0; s < a->n_sub; s++) {
        const unsigned int* w = tr + (size_t)s * 4;
        forgotten += rph_key_row(K, rpa_trace_bit(w, k), rph_row_pedal(w) | env_pedal, (double)(T0 + s + 1) * a->dt, M.rel_tail);
      }
      rph_key_end(K, (double)(T0 + a->n_sub) * a->dt);
      rph_store_key(a->bank.t_on, a->bank.t_off, env, k, K);
      act_w[k >> 5] |= (unsigned)K.prev << (k & 31);
      held_w[k >> 5] |= (unsigned)K.held << (k & 31);
    }
    for (int i = 0; i < 3; i++) { st[i] = (int)act_w[i]; st[3 + i] = (int)held_w[i]; }
    st[6] = T0 + a->n_sub;
    st[7] = forgotten;
  }
}

// ---- the window --------------------------------------------------------------------------------------------------
// N = floor(sr ((double)T dt)), the newest sample of the window
RPA_INLINE int rph_last_sample(double sr, int T, double dt) {
  const double n = floor(sr * ((double)(T < 0 ? 0 : T) * dt));
  return n > RPH_MAX_SAMPLE ? (int)RPH_MAX_SAMPLE : (int)n;
}

// bank entry v of the summation order: key ascending, slot 1 then slot 0
RPA_INLINE int rph_voice_key(int v) { return v >> 1; }
RPA_INLINE int rph_voice_slot(int v) { return 1 - (v & 1); }

// Stages entry v if it can sound in the samples [b0, b1); false otherwise.
RPA_INLINE bool rph_stage(const RpaModel& M, const double* t_on, const double* t_off, int env, int v, int b0, int b1,
                          RpaVoice& out) {
  const int key = rph_voice_key(v);
  const size_t i = rph_slot(env, key, rph_voice_slot(v));
  const double on = t_on[i], off = t_off[i];
  if (!rpa_valid_note(key, on, off) || !rpa_maybe_audible(M, on, off, b0, b1)) return false;
  rpa_stage(M, key, on, off, 127, out);
  return out.n_on < b1 && b0 < out.n_cut;
}

inline void rph_window_host(const RpaModel& M, int W, const rp_hear_spectrum_args* a, float* window) {
  for (int env = a->env_first; env < a->env_first + a->env_count; env++) {
    const int n_start = rph_last_sample(M.sr, a->bank.state[(size_t)env * RPH_STATE + 6], a->dt) - W + 1;
    float* row = window + (size_t)env * W;
    for (int off = 0; off < W; off += RPA_BLOCK) {
      const int b0 = n_start + off;
      const int b1 = b0 + (W - off < RPA_BLOCK ? W - off : RPA_BLOCK);
      RpaVoice sv[RPH_VOICES];
      int nv = 0;
      for (int v = 0; v < RPH_VOICES; v++)
        if (rph_stage(M, a->bank.t_on, a->bank.t_off, env, v, b0, b1, sv[nv])) nv++;
      for (int t = 0; t < RPA_THREADS; t++) {
        float acc[RPA_R];
        for (int j = 0; j < RPA_R; j++) acc[j] = 0.f;
        rpa_accumulate(M, sv, nv, b0 + t, acc);
        for (int j = 0; j < RPA_R; j++) {
          const int i = off + t + j * RPA_THREADS;
          if (i < W) row[i] = acc[j];
        }
      }
    }
  }
}

// ---- the analysis ------------------------------------------------------------------------------------------------
RPA_INLINE float rph_magnitude(float c, float s) { return sqrtf(fmaf(c, c, s * s)); }

inline void rph_analysis_host(const RphAnalysis& A, const rp_hear_spectrum_args* a, const float* window) {
  for (int env = a->env_first; env < a->env_first + a->env_count; env++) {
    const float* x = window + (size_t)env * A.W;
    for (int b = 0; b < A.B; b++) {
      float c = 0.f, s = 0.f;
      for (int j = 0; j < A.W; j++) {
        c = fmaf(x[j], A.C[(size_t)j * A.B + b], c);
        s = fmaf(x[j], A.S[(size_t)j * A.B + b], s);
      }
      a->spectrum[(size_t)env * A.B + b] = rph_magnitude(c, s);
    }
  }
}
