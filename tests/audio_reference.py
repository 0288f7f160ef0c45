"""Reference for the synthesiser's tests: a numpy restatement of the sound definition (include/audio/rp_audio.h), the
shared test cases, the tolerance, and the g++ build of csrc/rp_audio.hpp.

`reference_wave` evaluates the definition in closed form per sample, with no recurrence: in float64, or in float32
with t, u and u - u_off formed in float64 and then rounded and the phase frac(f_h u) reduced in float64, which is what
the header asks of an implementation.  The tolerance of every wave comparison is 4 x the largest difference between the
two over the test cases, relative to the case's peak (test_audio_host.py measures it).
"""

from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = 0.005
SR = 44100
T_CAP = 64
N_KEYS = 88
PEDAL = 88

# max |float32 - float64| / peak of the reference over the cases below (measure_reference_rounding, on the CPU)
MEASURED_WAVE_ROUNDING = 4.85e-7
WAVE_TOL = 4 * MEASURED_WAVE_ROUNDING   # absolute, as a fraction of the case's peak


def n_samples(T, dt=DT, sr=SR):
    return int(math.ceil(sr * (T * dt + 1.0)))


# ---- timbres -----------------------------------------------------------------------------------------------------
def pure_sine_timbre(tau_att=0.002, tau_rel=0.05):
    """H = 1, B = 0, tau so large that the decay is invisible: a voice is sin(2 pi f0 u) att rel."""
    return dict(H=1, a=np.ones(1), tau=np.full((N_KEYS, 1), 1e12), B=np.zeros(N_KEYS), tau_att=tau_att, tau_rel=tau_rel)


def partials(timbre, sr=SR):
    """(f [88][H] Hz, amp [88][H] with the partials at or above 0.45 sr silenced, tau [88][H])."""
    H = int(timbre["H"])
    p = np.arange(N_KEYS) + 21
    h = np.arange(1, H + 1)
    f0 = 440.0 * 2.0 ** ((p - 69) / 12.0)
    B = np.broadcast_to(np.asarray(timbre["B"], np.float64), (N_KEYS,))
    f = h[None, :] * f0[:, None] * np.sqrt(1.0 + B[:, None] * h[None, :] ** 2)
    amp = np.where(f >= 0.45 * sr, 0.0, np.broadcast_to(np.asarray(timbre["a"], np.float64), (N_KEYS, H)))
    tau = np.broadcast_to(np.asarray(timbre["tau"], np.float64), (N_KEYS, H))
    return f, amp, tau


# ---- the definition ------------------------------------------------------------------------------------------------
def reference_wave(notes, T, timbre, dt=DT, sr=SR, n_cap=None, dtype=np.float64):
    """wave [n_cap] of one environment: `notes` = [(key, t_on, t_off, velocity)] in list order."""
    ns = n_samples(T, dt, sr)
    n_cap = ns if n_cap is None else n_cap
    out = np.zeros(n_cap, dtype)
    t = np.arange(ns, dtype=np.float64) / sr
    f, amp, tau = partials(timbre, sr)
    tau_att, tau_rel = float(timbre["tau_att"]), float(timbre["tau_rel"])
    F = dtype
    for key, t_on, t_off, vel in notes:
        u_all = t - t_on
        u_off = t_off - t_on
        idx = np.flatnonzero((u_all >= 0) & ~(u_all >= u_off + 8.0 * tau_rel))
        if not len(idx):
            continue
        u64 = u_all[idx]
        u = u64.astype(F)
        S = np.zeros(len(idx), F)
        for h in range(int(timbre["H"])):
            if amp[key, h] == 0.0:
                continue
            x = f[key, h] * u64
            ph = (x - np.floor(x)).astype(F)
            S += F(amp[key, h]) * np.exp(-u / F(tau[key, h])) * np.sin(F(2.0 * np.pi) * ph)
        att = F(1.0) - np.exp(-u / F(tau_att))
        rel = np.where(u64 >= u_off, np.exp(-(u64 - u_off).astype(F) / F(tau_rel)), F(1.0)).astype(F)
        g = F(vel / 127.0) ** 2
        out[idx] += (g * att * rel * S).astype(F)
    return out


def reference_pcm(wave64):
    peak = np.abs(wave64).max() if len(wave64) else 0.0
    if peak == 0:
        return np.zeros(len(wave64), np.int16)
    return np.trunc(32767.0 * wave64 / peak).astype(np.int16)


# ---- traces and cases ------------------------------------------------------------------------------------------------
def make_trace(T, presses=(), pedal=()):
    """[T][4] uint32: `presses` = (key, first substep, last substep) inclusive, `pedal` = (first, last) spans."""
    tr = np.zeros((T, 4), np.uint32)
    for key, a, b in presses:
        tr[a:b + 1, key // 32] |= np.uint32(1 << (key % 32))
    for a, b in pedal:
        tr[a:b + 1, PEDAL // 32] |= np.uint32(1 << (PEDAL % 32))
    return tr


def case_a():
    """Three environments of lengths 64, 37 and 0 in a [3][64][4] trace.  Key bits 0, 31, 32, 63, 64, 87 (word and
    wave-pass boundaries), the pedal bit; every onset (s+1) 220.5 samples falls mid-block and mid-run; keys 63 / 64
    are released under the pedal and ring from 0.065 s to the pedal-up at 0.21 s plus the 0.4 s release (> 20 blocks
    of 1024); key 87 is struck again under the pedal; key 40 is still down at the end; the rows past an
    environment's length are set bits that must be ignored."""
    e0 = make_trace(T_CAP, presses=[(0, 2, 9), (31, 4, 6), (32, 4, 20), (63, 12, 15), (64, 12, 15), (87, 20, 22),
                                    (87, 30, 31), (40, 50, 63), (45, 50, 55)], pedal=[(14, 40)])
    e1 = make_trace(T_CAP, presses=[(0, 0, 3), (87, 1, 30), (64, 5, 8), (31, 35, 63), (12, 37, 63)], pedal=[(6, 63)])
    e2 = np.full((T_CAP, 4), 0xFFFFFFFF, np.uint32)
    return np.stack([e0, e1, e2]), np.array([64, 37, 0], np.int32)


def case_b():
    """More audible notes than one LDS chunk (64): all 88 keys struck in one substep, under the pedal."""
    tr = make_trace(T_CAP, presses=[(k, 3, 5) for k in range(N_KEYS)], pedal=[(0, 50)])
    return tr[None], np.array([T_CAP], np.int32)


def host_notes(trace, T, dt=DT, max_notes=None):
    """(notes, dropped) of one environment by the Python twin: MidiModule events, then notes_from_events."""
    from robopianist_amd.music import synthesizer
    ev = synthesizer.events_from_substep_trace(np.asarray(trace)[:T], dt)
    notes = synthesizer.notes_from_events(ev, T * dt)
    if max_notes is not None and len(notes) > max_notes:
        return notes[:max_notes], len(notes) - max_notes
    return notes, 0


@functools.lru_cache(maxsize=None)
def case_references(name):
    """Per environment of case `name` ("a" / "b"), with the default timbre: (notes, float64 wave); computed once."""
    from robopianist_amd.music import synthesizer
    trace, lengths = case_a() if name == "a" else case_b()
    out = []
    for e in range(len(lengths)):
        notes, _ = host_notes(trace[e], int(lengths[e]))
        w = reference_wave(notes, int(lengths[e]), synthesizer.DEFAULT_TIMBRE, n_cap=n_samples(T_CAP))
        w.setflags(write=False)
        out.append((notes, w))
    return out


def measure_reference_rounding():
    """max |float32 - float64| / peak of the reference over the environments of the cases."""
    from robopianist_amd.music import synthesizer
    worst = 0.0
    for name in ("a", "b"):
        trace, lengths = case_a() if name == "a" else case_b()
        for e, (notes, w64) in enumerate(case_references(name)):
            if not notes:
                continue
            w32 = reference_wave(notes, int(lengths[e]), synthesizer.DEFAULT_TIMBRE, n_cap=len(w64), dtype=np.float32)
            worst = max(worst, float(np.abs(w32.astype(np.float64) - w64).max() / np.abs(w64).max()))
    return worst


def compare_wave(got, ref64, label=""):
    """|got - ref| <= WAVE_TOL x peak(ref), and exact zeros where the reference is exactly zero."""
    got = np.asarray(got, np.float64)
    peak = float(np.abs(ref64).max())
    err = float(np.abs(got - ref64).max())
    print(f"{label}: max |wave - ref| = {err:.3e} = {err / peak if peak else 0:.3e} of the peak {peak:.4f} (tolerance {WAVE_TOL:.2e})")
    assert np.isfinite(got).all()
    assert err <= WAVE_TOL * peak, f"{label}: {err:.3e} > {WAVE_TOL * peak:.3e}"


def compare_pcm(got, ref64, label=""):
    d = np.abs(np.asarray(got, np.int64) - reference_pcm(ref64).astype(np.int64)).max() if len(ref64) else 0
    print(f"{label}: max |pcm - ref| = {d}")
    assert d <= 1, f"{label}: pcm differs by {d}"


def notes_from_arrays(key, t_on, t_off, vel, count):
    return [(int(key[i]), float(t_on[i]), float(t_off[i]), int(vel[i])) for i in range(int(count))]


# ---- the g++ build of csrc/rp_audio.hpp ---------------------------------------------------------------------------
_HOST_SRC = r"""
#include "rp_audio.hpp"
struct rp_audio { RpaTables tab; RpaModel M; int n_envs, max_substeps, max_notes; };
static thread_local std::string g_err;
static int fail(const std::string& s) { g_err = s; return -1; }
extern "C" {
const char* rpah_last_error(void) { return g_err.c_str(); }
int rpah_create(const void* blob, size_t bytes, int n_envs, int max_substeps, int max_notes, int device, rp_audio** out) {
  (void)device;
  rp_audio* a = new rp_audio();
  const std::string err = a->tab.parse(blob, bytes);
  if (!err.empty()) { delete a; return fail(err); }
  a->n_envs = n_envs; a->max_substeps = max_substeps; a->max_notes = max_notes;
  a->M = a->tab.view(a->tab.part.data());
  *out = a;
  return 0;
}
void rpah_destroy(rp_audio* a) { delete a; }
int rpah_notes_from_trace(rp_audio* a, const rp_audio_notes_args* g) {
  const std::string err = rpa_check_notes_args(g, a->n_envs, a->max_substeps);
  if (!err.empty()) return fail(err);
  for (int env = g->env_first; env < g->env_first + g->env_count; env++) {
    const size_t nb = (size_t)env * a->max_notes;
    rpa_notes_host(g->trace + (size_t)env * g->trace_substeps * 4, rpa_clamp_len(g->lengths[env], g->trace_substeps), g->dt,
                   a->max_notes, g->notes.key + nb, g->notes.t_on + nb, g->notes.t_off + nb, g->notes.velocity + nb,
                   g->notes.count + env, g->notes.dropped + env);
  }
  return 0;
}
int rpah_synthesize(rp_audio* a, const rp_audio_synth_args* g) {
  const std::string err = rpa_check_synth_args(g, a->n_envs, a->max_substeps, a->tab.sr);
  if (!err.empty()) return fail(err);
  rpa_synthesize_host(a->M, g, a->max_notes);
  return 0;
}
int rpah_dim(const rp_audio* a, const char* name) { return !strcmp(name, "block_samples") ? RPA_BLOCK : !strcmp(name, "chunk_notes") ? RPA_CHUNK : -1; }
}
"""

_host_lib = None
_host_dir = None


def host_library():
    """Compiles csrc/rp_audio.hpp with g++ (once per process) and loads the result."""
    global _host_lib, _host_dir
    if _host_lib is None:
        from robopianist_amd.music import synthesizer
        _host_dir = tempfile.TemporaryDirectory(prefix="rp_audio_host_")
        src = os.path.join(_host_dir.name, "rp_audio_host.cpp")
        so = os.path.join(_host_dir.name, "librp_audio_host.so")
        with open(src, "w") as fh:
            fh.write(_HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "robopianist_amd", "csrc"), src, "-o", so])
        L = ctypes.CDLL(so)
        synthesizer.declare(L, "rpah_")
        _host_lib = L
    return _host_lib


class HostAudio:
    """The library's two calls on the CPU (rpa_notes_host, rpa_synthesize_host), numpy arrays in and out."""

    def __init__(self, n_envs=1, max_substeps=T_CAP, max_notes=256, timbre=None, sr=SR):
        from robopianist_amd.music import synthesizer
        self._S = synthesizer
        self._L = host_library()
        self.n_envs, self.max_substeps, self.max_notes, self.sr = n_envs, max_substeps, max_notes, sr
        self.blob = synthesizer.make_audio_blob(timbre, sr)
        self._h = ctypes.c_void_p()
        if self._L.rpah_create(self.blob, len(self.blob), n_envs, max_substeps, max_notes, 0, ctypes.byref(self._h)) != 0:
            raise RuntimeError(self._L.rpah_last_error().decode())
        E, N = n_envs, max_notes
        self.notes = dict(key=np.zeros((E, N), np.int32), t_on=np.zeros((E, N)), t_off=np.zeros((E, N)),
                          velocity=np.zeros((E, N), np.int32), count=np.zeros(E, np.int32), dropped=np.zeros(E, np.int32))

    def __del__(self):
        try:
            self._L.rpah_destroy(self._h)
        except Exception:
            pass

    def _notes_struct(self):
        return self._S.Notes(*[self.notes[k].ctypes.data for k in ("key", "t_on", "t_off", "velocity", "count", "dropped")])

    def notes_from_trace(self, trace, lengths, dt=DT, env_first=0, env_count=None):
        trace = np.ascontiguousarray(trace, np.uint32)
        lengths = np.ascontiguousarray(lengths, np.int32)
        a = self._S.NotesArgs()
        a.struct_size = ctypes.sizeof(a)
        a.trace, a.lengths, a.trace_substeps = trace.ctypes.data, lengths.ctypes.data, trace.shape[1]
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        a.dt, a.notes = dt, self._notes_struct()
        if self._L.rpah_notes_from_trace(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rpah_last_error().decode())
        return [notes_from_arrays(self.notes["key"][e], self.notes["t_on"][e], self.notes["t_off"][e],
                                  self.notes["velocity"][e], self.notes["count"][e]) for e in range(self.n_envs)]

    def set_notes(self, env, notes):
        for i, (k, on, off, v) in enumerate(notes):
            self.notes["key"][env, i], self.notes["t_on"][env, i] = k, on
            self.notes["t_off"][env, i], self.notes["velocity"][env, i] = off, v
        self.notes["count"][env] = len(notes)

    def synthesize(self, lengths, substeps_cap, dt=DT, pcm=True, env_first=0, env_count=None):
        lengths = np.ascontiguousarray(lengths, np.int32)
        n_cap = n_samples(substeps_cap, dt, self.sr)
        wave = np.zeros((self.n_envs, n_cap), np.float32)
        out = np.zeros((self.n_envs, n_cap), np.int16)
        a = self._S.SynthArgs()
        a.struct_size = ctypes.sizeof(a)
        a.notes, a.lengths, a.substeps_cap, a.n_cap = self._notes_struct(), lengths.ctypes.data, substeps_cap, n_cap
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        a.dt, a.wave, a.pcm = dt, wave.ctypes.data, out.ctypes.data if pcm else None
        if self._L.rpah_synthesize(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rpah_last_error().decode())
        return wave, out
