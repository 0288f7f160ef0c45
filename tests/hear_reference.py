"""Reference for the tests of the audio observation (include/audio/rp_hear.h): a numpy restatement of the tracker, of
the window and of the analysis, the shared cases, the tolerances, and the g++ build of csrc/rp_hear.hpp.

The tracker twin is plain Python over boolean arrays.  The window is a slice of `audio_reference.reference_wave` (the
closed form per sample, no recurrence) on the bank's voices, in float64 or in float32 under the header's rules; the
analysis is a matrix product in float64, or a sequential float32 chain.  The tolerances follow the project's rule: 4 x
the largest difference between the float32 and the float64 restatement over the test cases (`measure_rounding`),
relative to the peak of the float64 sound of the rows consumed so far; a spectrum is in the sound's units (a unit sine
at a bin's frequency reads 1), so it is measured against the same peak.
"""

from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

import audio_reference as ar

ROOT = ar.ROOT
DT = ar.DT
SR = 16000
N_KEYS = ar.N_KEYS
N_SUB = 4

# max |float32 - float64| / peak over every call of the stream of case_a and the five analyses (measure_rounding, on
# the CPU: 4.724e-07 and 3.563e-07)
MEASURED_WINDOW_ROUNDING = 4.73e-7
MEASURED_SPECTRUM_ROUNDING = 3.57e-7
WINDOW_TOL = 4 * MEASURED_WINDOW_ROUNDING       # absolute, as a fraction of the peak of the sound so far
SPECTRUM_TOL = 4 * MEASURED_SPECTRUM_ROUNDING


def default_timbre():
    from robopianist_amd.music import synthesizer
    return synthesizer.DEFAULT_TIMBRE


# ---- the tracker ---------------------------------------------------------------------------------------------------
class TrackerTwin:
    """One environment's voice bank by the rule of rp_hear.h, in Python."""

    def __init__(self, tau_rel=None):
        self.tail = 8.0 * float(default_timbre()["tau_rel"] if tau_rel is None else tau_rel)
        self.restart()

    def restart(self):
        self.t_on = np.full((N_KEYS, 2), -1.0)
        self.t_off = np.full((N_KEYS, 2), -1.0)
        self.act = np.zeros(N_KEYS, bool)
        self.held = np.zeros(N_KEYS, bool)
        self.T = 0
        self.forgotten = 0

    def track(self, rows, dt=DT, pedal=False, restart=False):
        """rows: [n_sub][4] uint32."""
        if restart:
            self.restart()
            return
        rows = np.asarray(rows, np.uint32).reshape(-1, 4)
        for w in rows:
            act = np.array([(int(w[k // 32]) >> (k % 32)) & 1 for k in range(N_KEYS)], bool)
            ped = bool((int(w[ar.PEDAL // 32]) >> (ar.PEDAL % 32)) & 1) or bool(pedal)
            self.T += 1
            t = float(self.T) * dt
            onset = act & ~self.act
            now = act | (self.held & ped)
            close = self.held & (onset | ~now)
            self.t_off[close, 0] = t
            for k in np.flatnonzero(onset):
                if self.t_on[k, 1] >= 0 and self.t_off[k, 1] + self.tail > t:
                    self.forgotten += 1
                self.t_on[k, 1], self.t_off[k, 1] = self.t_on[k, 0], self.t_off[k, 0]
                self.t_on[k, 0] = self.t_off[k, 0] = t
            self.act, self.held = act, now
        self.t_off[self.held, 0] = float(self.T) * dt

    def state(self):
        """int32 [8] as rp_hear.h lays it out."""
        def words(bits):
            out = np.zeros(3, np.uint32)
            for k in np.flatnonzero(bits):
                out[k // 32] |= np.uint32(1) << np.uint32(k % 32)
            return out
        return np.concatenate([words(self.act), words(self.held), np.array([self.T, self.forgotten], np.uint32)]).view(np.int32)


def bank_of_notes(notes):
    """(t_on, t_off) [88][2] that the invariant asks for: per key the last two notes of `notes` (ordered by onset),
    newest first."""
    t_on = np.full((N_KEYS, 2), -1.0)
    t_off = np.full((N_KEYS, 2), -1.0)
    for k in range(N_KEYS):
        mine = [n for n in notes if n[0] == k][-2:][::-1]
        for s, n in enumerate(mine):
            t_on[k, s], t_off[k, s] = n[1], n[2]
    return t_on, t_off


def notes_of_bank(t_on, t_off):
    """The bank's voices in summation order: key ascending, slot 1 then slot 0; empty slots left out."""
    return [(k, float(t_on[k, s]), float(t_off[k, s]), 127) for k in range(N_KEYS) for s in (1, 0) if t_on[k, s] >= 0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ---- the window and the analysis -----------------------------------------------------------------------------------------
def last_sample(T, dt=DT, sr=SR):
    return int(math.floor(float(sr) * (float(T) * dt)))


def reference_sound(t_on, t_off, T, timbre=None, dt=DT, sr=SR, dtype=np.float64):
    """The bank's sound from sample 0 to past N, by audio_reference.reference_wave."""
    return ar.reference_wave(notes_of_bank(t_on, t_off), T, default_timbre() if timbre is None else timbre, dt, sr, dtype=dtype)


def window_of(sound, T, W, dt=DT, sr=SR):
    """Samples N - W + 1 .. N of `sound`, zeros before sample 0."""
    N = last_sample(T, dt, sr)
    out = np.zeros(W, sound.dtype)
    lo = N - W + 1
    out[max(0, -lo):] = sound[max(0, lo):N + 1]
    return out


def reference_spectrum(x, C, S, dtype=np.float64):
    """sqrt(c^2 + s^2): in float64 a matrix product, in float32 the sequential chain over j."""
    if dtype == np.float64:
        x64 = np.asarray(x, np.float64)
        return np.hypot(x64 @ np.asarray(C, np.float64), x64 @ np.asarray(S, np.float64))
    x, C, S = np.asarray(x, np.float32), np.asarray(C, np.float32), np.asarray(S, np.float32)
    c = np.zeros(C.shape[1], np.float32)
    s = np.zeros(C.shape[1], np.float32)
    for j in range(len(x)):
        c = c + x[j] * C[j]
        s = s + x[j] * S[j]
    return np.sqrt(c * c + s * s)


@functools.lru_cache(maxsize=None)
def analysis(name):
    """The analyses of the tests: (C, S) float32 [W][B]."""
    from robopianist_amd.music import hearing
    f = hearing.key_frequencies()
    if name == "small":      # W 128, B 5
        C, S = hearing.make_analysis(SR, 128, freqs=f[[0, 31, 40, 63, 87]])
    elif name == "default":  # W 2048, B 88: 2B = 176 is no multiple of a tile
        C, S = hearing.make_analysis(SR, 2048)
    elif name == "one":      # B = 1
        C, S = hearing.make_analysis(SR, 256, freqs=f[[40]])
    elif name == "wide":     # B = 128
        C, S = hearing.make_analysis(SR, 512, freqs=np.geomspace(60.0, 7000.0, 128))
    elif name == "short":    # W = 64
        C, S = hearing.make_analysis(SR, 64, freqs=f[[45, 60, 75, 87]], cycles=4.0)
    else:
        raise KeyError(name)
    for a in (C, S):
        a.setflags(write=False)
    return C, S


MAIN_ANALYSES = ("small", "default")
ALL_ANALYSES = ("small", "default", "one", "wide", "short")


@functools.lru_cache(maxsize=None)
def stream_reference(case="a", n_sub=N_SUB):
    """case_a fed `n_sub` rows at a time to every environment (all 64 rows of each: the environments' own lengths do not
    apply to a stream).  Per call a list over environments of dict(t_on, t_off, state, T, forgotten, sound64, peak):
    the twin's bank after the call and the float64 sound of it; computed once."""
    trace, _ = ar.case_a()
    twins = [TrackerTwin() for _ in range(len(trace))]
    calls = []
    for c in range(trace.shape[1] // n_sub):
        envs = []
        for e, tw in enumerate(twins):
            tw.track(trace[e, c * n_sub:(c + 1) * n_sub])
            sound = reference_sound(tw.t_on, tw.t_off, tw.T)
            sound.setflags(write=False)
            envs.append(dict(t_on=tw.t_on.copy(), t_off=tw.t_off.copy(), state=tw.state(), T=tw.T, forgotten=tw.forgotten,
                             sound64=sound, peak=float(np.abs(sound).max())))
        calls.append(envs)
    return calls


def measure_rounding(names=ALL_ANALYSES):
    """(window, spectrum): max |float32 - float64| / peak of the restatements over every call of the stream of case_a,
    for the analyses `names`."""
    worst_w = worst_s = 0.0
    for envs in stream_reference():
        for r in envs:
            if r["peak"] == 0.0:
                continue
            sound32 = reference_sound(r["t_on"], r["t_off"], r["T"], dtype=np.float32)
            for name in names:
                C, S = analysis(name)
                W = C.shape[0]
                x64, x32 = window_of(r["sound64"], r["T"], W), window_of(sound32, r["T"], W)
                worst_w = max(worst_w, float(np.abs(x32.astype(np.float64) - x64).max()) / r["peak"])
                s64, s32 = reference_spectrum(x64, C, S), reference_spectrum(x32, C, S, np.float32)
                worst_s = max(worst_s, float(np.abs(s32.astype(np.float64) - s64).max()) / r["peak"])
    return worst_w, worst_s


def compare(got, ref64, peak, tol, label):
    """|got - ref| <= tol x peak; exact zeros where the reference is exactly zero."""
    got = np.asarray(got, np.float64)
    err = float(np.abs(got - ref64).max())
    print(f"{label}: max |got - ref| = {err:.3e} = {err / peak if peak else 0:.3e} of the peak {peak:.4f} (tolerance {tol:.2e})")
    assert np.isfinite(got).all()
    assert err <= tol * peak, f"{label}: {err:.3e} > {tol * peak:.3e}"
    assert (got[ref64 == 0] == 0).all(), f"{label}: silent stretches must be exact zeros"


def check_observation(r, name, window, spectrum, label):
    """One environment after one call: `r` of stream_reference (or a dict of the same keys), against analysis `name`."""
    C, S = analysis(name) if isinstance(name, str) else name
    x64 = window_of(r["sound64"], r["T"], C.shape[0])
    if window is not None:
        compare(window, x64, r["peak"], WINDOW_TOL, label + " window")
    s64 = reference_spectrum(x64, C, S)
    compare(spectrum, s64, r["peak"], SPECTRUM_TOL, label + " spectrum")
    if not x64.any():
        assert not np.asarray(spectrum).any(), f"{label}: a silent window must read exact zeros"


def reference_of_rows(rows, sustain=None, n_sub=N_SUB, dt=DT):
    """dict(t_on, t_off, state, T, forgotten, sound64, peak) of one environment after its rows [T][4] were consumed
    `n_sub` at a time, `sustain[i]` being call i's pedal flag."""
    tw = TrackerTwin()
    rows = np.asarray(rows, np.uint32).reshape(-1, 4)
    for i in range(len(rows) // n_sub):
        tw.track(rows[i * n_sub:(i + 1) * n_sub], dt, pedal=bool(sustain[i]) if sustain is not None else False)
    sound = reference_sound(tw.t_on, tw.t_off, tw.T, dt=dt)
    return dict(t_on=tw.t_on, t_off=tw.t_off, state=tw.state(), T=tw.T, forgotten=tw.forgotten, sound64=sound,
                peak=float(np.abs(sound).max()))


# ---- the g++ build of csrc/rp_hear.hpp -------------------------------------------------------------------------------
_HOST_SRC = r"""
#include "rp_hear.hpp"
struct rp_hear { RpaTables tab; RphAnalysis ana; RpaModel M; int n_envs, max_substeps; std::vector<float> window; };
static thread_local std::string g_err;
static int fail(const std::string& s) { g_err = s; return -1; }
extern "C" {
const char* rphh_last_error(void) { return g_err.c_str(); }
int rphh_create(const void* ab, size_t an, const void* bb, size_t bn, int n_envs, int max_substeps, int device, rp_hear** out) {
  (void)device;
  rp_hear* h = new rp_hear();
  std::string err = h->tab.parse(ab, an);
  if (err.empty()) err = h->ana.parse(bb, bn);
  if (!err.empty()) { delete h; return fail(err); }
  h->n_envs = n_envs; h->max_substeps = max_substeps;
  h->M = h->tab.view(h->tab.part.data());
  h->window.assign((size_t)n_envs * h->ana.W, 0.f);
  *out = h;
  return 0;
}
void rphh_destroy(rp_hear* h) { delete h; }
int rphh_track(rp_hear* h, const rp_hear_track_args* g) {
  const std::string err = rph_check_track_args(g, h->n_envs, h->max_substeps);
  if (!err.empty()) return fail(err);
  rph_track_host(h->M, g);
  return 0;
}
int rphh_spectrum(rp_hear* h, const rp_hear_spectrum_args* g) {
  const std::string err = rph_check_spectrum_args(g, h->n_envs);
  if (!err.empty()) return fail(err);
  float* w = g->window ? g->window : h->window.data();
  rph_window_host(h->M, h->ana.W, g, w);
  rph_analysis_host(h->ana, g, w);
  return 0;
}
int rphh_dim(const rp_hear* h, const char* name) { return !strcmp(name, "W") ? h->ana.W : !strcmp(name, "B") ? h->ana.B : -1; }
}
"""

_host_lib = None
_host_dir = None


def host_library():
    """Compiles csrc/rp_hear.hpp with g++ (once per process) and loads the result."""
    global _host_lib, _host_dir
    if _host_lib is None:
        from robopianist_amd.music import hearing
        _host_dir = tempfile.TemporaryDirectory(prefix="rp_hear_host_")
        src = os.path.join(_host_dir.name, "rp_hear_host.cpp")
        so = os.path.join(_host_dir.name, "librp_hear_host.so")
        with open(src, "w") as fh:
            fh.write(_HOST_SRC)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", os.path.join(ROOT, "robopianist_amd", "csrc"), src, "-o", so])
        L = ctypes.CDLL(so)
        hearing.declare(L, "rphh_")
        _host_lib = L
    return _host_lib


class HostHearing:
    """The library's two calls on the CPU (rph_track_host, rph_window_host, rph_analysis_host), numpy arrays in and out."""

    def __init__(self, n_envs=1, analysis_tables=None, timbre=None, sr=SR, max_substeps_per_call=64):
        from robopianist_amd.music import hearing, synthesizer
        self._H = hearing
        self._L = host_library()
        self.n_envs = n_envs
        C, S = analysis("default") if analysis_tables is None else analysis_tables
        self.W, self.B = C.shape
        ab, bb = synthesizer.make_audio_blob(timbre, sr), hearing.make_analysis_blob(C, S)
        self._h = ctypes.c_void_p()
        if self._L.rphh_create(ab, len(ab), bb, len(bb), n_envs, max_substeps_per_call, 0, ctypes.byref(self._h)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())
        self.t_on = np.full((n_envs, N_KEYS, 2), -1.0)
        self.t_off = np.full((n_envs, N_KEYS, 2), -1.0)
        self.state = np.zeros((n_envs, 8), np.int32)

    def __del__(self):
        try:
            self._L.rphh_destroy(self._h)
        except Exception:
            pass

    def _bank(self):
        return self._H.Bank(self.t_on.ctypes.data, self.t_off.ctypes.data, self.state.ctypes.data)

    def track(self, trace, pedal=None, restart=None, dt=DT, env_first=0, env_count=None):
        trace = np.ascontiguousarray(trace, np.uint32)
        pedal = None if pedal is None else np.ascontiguousarray(pedal, np.int32)
        restart = None if restart is None else np.ascontiguousarray(restart, np.int32)
        a = self._H.TrackArgs()
        a.struct_size = ctypes.sizeof(a)
        a.trace, a.n_sub = trace.ctypes.data, trace.shape[1]
        a.pedal = None if pedal is None else pedal.ctypes.data
        a.restart = None if restart is None else restart.ctypes.data
        a.dt, a.bank = dt, self._bank()
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        if self._L.rphh_track(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())

    def spectrum(self, dt=DT, env_first=0, env_count=None):
        """(spectrum [E][B], window [E][W])"""
        window = np.zeros((self.n_envs, self.W), np.float32)
        spec = np.zeros((self.n_envs, self.B), np.float32)
        a = self._H.SpectrumArgs()
        a.struct_size = ctypes.sizeof(a)
        a.bank, a.dt = self._bank(), dt
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        a.window, a.spectrum = window.ctypes.data, spec.ctypes.data
        if self._L.rphh_spectrum(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())
        return spec, window
