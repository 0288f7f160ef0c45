/* audio/rp_audio.h — batched piano synthesis from the engine's key trace (C ABI, gfx950, librp_audio.so).
 *
 * Two calls: rp_audio_notes_from_trace turns the per-substep activation bit masks of a batch of environments
 * (rp_step(key_trace), accumulated over an episode) into one note list per environment; rp_audio_synthesize turns
 * note lists into sound.  The note list lives in caller-owned device memory, so a list made on the host can be
 * synthesised as well.
 *
 * Sound definition.
 *
 * Inputs per environment: a trace [T][4] of uint32 (bits 0..87 = key activations of substep s, bit 88 = sustain
 * pedal; the engine leaves bit 88 at 0, a recorder sets it), a length T_e <= T, the physics timestep dt, and the
 * sample rate sr of the timbre blob.
 *
 * Notes from the trace.  The activation before substep 0 is 0; an event of substep s has time (s+1) dt.  Per key
 *     held[s] = act[s] | (held[s-1] & pedal[s]).
 * A rising edge of act starts a note; if the key is still held at that moment (a re-strike under the pedal) the
 * open note is released at that same time.  A falling edge of held releases the open note.  A note still open at
 * T_e is released at T_e dt.  Velocity is 127.  The list is ordered by onset time, then key, and capped at
 * max_notes: later notes are dropped and counted in `dropped`.
 *
 * A voice.  With p = key + 21, f0 = 440 2^((p-69)/12), f_h = h f0 sqrt(1 + B(p) h^2), u = t - t_on,
 * u_off = t_off - t_on and g = (velocity/127)^2, a note sounds
 *     g att(u) rel(u) sum_{h=1..H} a_h exp(-u/tau_h(p)) sin(2 pi f_h u)        for u >= 0, and 0 before,
 *     att(u) = 1 - exp(-u/tau_att),
 *     rel(u) = 1 for u < u_off, exp(-(u-u_off)/tau_rel) after, and exactly 0 from u_off + 8 tau_rel on.
 * A partial with f_h >= 0.45 sr has amplitude 0.  H <= 8, a_h, tau_h(p), B(p), tau_att and tau_rel are the timbre
 * table of the create blob (robopianist_amd.music.synthesizer.make_audio_blob): data, not code.
 * A note whose key is outside 0..87, or whose times are not 0 <= t_on <= t_off < 1e6, does not sound.
 *
 * Output.  Sample n is at t = n/sr; n_samples_e = ceil(sr (T_e dt + 1.0)) (one second of tail).
 *   wave  float32 [E][n_cap]: the plain sum of the voices in list order; samples from n_samples_e on are 0.
 *   pcm   int16   [E][n_cap], optional: trunc(32767 (wave / peak_e)), peak_e = max |wave| of that environment, the
 *         quotient formed first, so the loudest sample is exactly +-32767; peak_e == 0 gives all zeros.
 * All per-sample arithmetic is float32; t, u and u - u_off are formed in float64 and then rounded, and a phase is
 * reduced as frac(f_h u) in float64 before any float32 sine.
 *
 * All array pointers are DEVICE pointers into caller-owned memory, rows indexed by the ABSOLUTE environment:
 * environments outside [env_first, env_first + env_count) stay untouched.  Both calls only enqueue on `hip_stream`
 * (hipStream_t; NULL = default stream): no host synchronisation, no allocation after create.  They return 0, or a
 * negative code with the message in rp_audio_last_error(); a refused call launches nothing.  The lengths are
 * device data, so the host checks the capacity they are clamped to (`trace_substeps` / `substeps_cap`) instead.
 */
#ifndef RP_AUDIO_H_
#define RP_AUDIO_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rp_audio rp_audio;

typedef struct rp_audio_notes {
  int* key;          /* [E][max_notes] key number 0..87 */
  double* t_on;      /* [E][max_notes] seconds */
  double* t_off;     /* [E][max_notes] seconds */
  int* velocity;     /* [E][max_notes] 1..127 */
  int* count;        /* [E] notes in the list (<= max_notes) */
  int* dropped;      /* [E] notes beyond max_notes; written by rp_audio_notes_from_trace only, may be NULL for synthesis */
} rp_audio_notes;

typedef struct rp_audio_notes_args {
  size_t struct_size;            /* sizeof(rp_audio_notes_args) of the caller: a mismatch is refused */
  const unsigned int* trace;     /* [E][trace_substeps][4] */
  const int* lengths;            /* [E] T_e; clamped to [0, trace_substeps] on the device */
  int trace_substeps;            /* rows per environment of `trace`; <= max_substeps */
  int env_first, env_count;
  double dt;                     /* physics timestep, seconds */
  rp_audio_notes notes;          /* out */
  void* hip_stream;
} rp_audio_notes_args;

typedef struct rp_audio_synth_args {
  size_t struct_size;            /* sizeof(rp_audio_synth_args) of the caller: a mismatch is refused */
  rp_audio_notes notes;          /* in */
  const int* lengths;            /* [E] T_e; clamped to [0, substeps_cap] on the device */
  int substeps_cap;              /* <= max_substeps */
  int n_cap;                     /* samples per row of wave and pcm; >= ceil(sr (substeps_cap dt + 1.0)) */
  int env_first, env_count;
  double dt;
  float* wave;                   /* [E][n_cap] */
  short* pcm;                    /* [E][n_cap] or NULL */
  void* hip_stream;
} rp_audio_synth_args;

/* `blob` = robopianist_amd.music.synthesizer.make_audio_blob (timbre table and sample rate).  max_notes is the row
 * length of the note arrays.  Uploads the per-key partial table. */
int rp_audio_create(const void* blob, size_t bytes, int n_envs, int max_substeps, int max_notes, int device,
                    rp_audio** out);
void rp_audio_destroy(rp_audio* a);

int rp_audio_notes_from_trace(rp_audio* a, const rp_audio_notes_args* args);
int rp_audio_synthesize(rp_audio* a, const rp_audio_synth_args* args);

/* "n_envs", "max_substeps", "max_notes", "H", "sample_rate" (rounded), "block_samples", "chunk_notes" */
int rp_audio_dim(const rp_audio* a, const char* name);

const char* rp_audio_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RP_AUDIO_H_ */
