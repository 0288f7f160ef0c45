"""Reference for the tests of the audio observation (include/audio/rp_hear.h): a numpy restatement of the tracker, of
the window and of the analysis, the shared cases, the tolerances, and the g++ build of csrc/rp_hear.hpp.

The tracker twin is plain Python over boolean arrays.  The window is a slice of `audio_reference.reference_wave` (the
closed form per sample, no recurrence) on the bank's voices, in float64 or in float32 under the header's rules; the
analysis is a matrix product in float64, or a sequential float32 chain.  The tolerances follow the project's rule: 4 x
the largest difference between the float32 and the float64 restatement over the test cases (`measure_rounding`),
relative to the peak of the float64 sound of the rows consumed so far; a spectrum is in the sound's units (a unit sine
at a bin's frequency reads 1), so it is measured against the same peak.

The wider cases (call shapes, forgotten voices, other rates, timesteps and timbres, late episodes) are defined below the
references; twin, restatements and checks take `dt`, `sr`, `timbre` and a start count `T0`.  Late in an episode the float64
reference is `reference_window`, which evaluates the window's samples alone.  The wider cases have a constant pair of
their own, measured over them by the same rule (`measure_wide_rounding`, WIDE_TOLS).
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


def timbre_of(timbre):
    """None (the default), a timbre dict, or one of the names the cached references are keyed by."""
    from robopianist_amd.music import synthesizer
    if timbre is None or timbre == "default":
        return default_timbre()
    if isinstance(timbre, str):
        if timbre == "harsh":
            return ar.harsh_timbre()
        if timbre == "sine":
            return ar.pure_sine_timbre()
        if timbre.startswith("tau_rel="):
            return synthesizer.make_timbre(tau_rel=float(timbre[len("tau_rel="):]))
        raise KeyError(timbre)
    return timbre


# ---- the tracker ---------------------------------------------------------------------------------------------------
class TrackerTwin:
    """One environment's voice bank by the rule of rp_hear.h, in Python."""

    def __init__(self, tau_rel=None, T0=0):
        self.tail = 8.0 * float(default_timbre()["tau_rel"] if tau_rel is None else tau_rel)
        self.restart()
        self.T = int(T0)     # (an empty bank whose count starts late; a restart goes back to 0, as the library's does)

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
    return ar.reference_wave(notes_of_bank(t_on, t_off), T, timbre_of(timbre), dt, sr, dtype=dtype)


def ranged_sound(notes, lo, hi, timbre=None, sr=SR, dtype=np.float64):
    """Samples lo..hi (0 <= lo, both inclusive) of the sound of `notes`: the closed form of
    audio_reference.reference_wave, statement for statement, with t = n / sr in float64, on that range alone; late in
    an episode nothing from sample 0 is needed."""
    timbre = timbre_of(timbre)
    out = np.zeros(max(0, hi - lo + 1), dtype)
    t = np.arange(lo, hi + 1, dtype=np.float64) / sr
    f, amp, tau = ar.partials(timbre, sr)
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
        rel = np.exp(-np.where(u64 >= u_off, u64 - u_off, 0.0).astype(F) / F(tau_rel))
        g = F(vel / 127.0) ** 2
        out[idx] += (g * att * rel * S).astype(F)
    return out


def reference_window(t_on, t_off, T, W, timbre=None, dt=DT, sr=SR, dtype=np.float64):
    """Samples N - W + 1 .. N of the bank's sound, zeros before sample 0: window_of(reference_sound(...)) to the bit
    (test_hearing_host.py asserts it), without the samples before the window."""
    N = last_sample(T, dt, sr)
    lo = N - W + 1
    out = np.zeros(W, dtype)
    out[max(0, -lo):] = ranged_sound(notes_of_bank(t_on, t_off), max(0, lo), N, timbre, sr, dtype)
    return out


def peak_so_far(t_on, t_off, T, timbre=None, dt=DT, sr=SR):
    """The largest |sample| of the bank's float64 sound from its earliest onset to N: the peak of a late case."""
    notes = notes_of_bank(t_on, t_off)
    N = last_sample(T, dt, sr)
    if not notes:
        return 0.0
    lo = max(0, int(math.floor(min(n[1] for n in notes) * sr)) - 1)
    sound = ranged_sound(notes, lo, N, timbre, sr)
    return float(np.abs(sound).max()) if len(sound) else 0.0


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


def bank_entry(tw, timbre=None, dt=DT, sr=SR, T0=0):
    """dict(t_on, t_off, state, T, forgotten, sound64, peak) of a twin's bank.  With T0 == 0 `sound64` is the float64
    sound from sample 0 and `peak` its largest |sample|; late in an episode (T0 > 0) there is no such array: `sound64` is
    None, check_observation evaluates the window alone, and the peak is peak_so_far's."""
    if T0:
        sound, peak = None, peak_so_far(tw.t_on, tw.t_off, tw.T, timbre, dt, sr)
    else:
        sound = reference_sound(tw.t_on, tw.t_off, tw.T, timbre, dt, sr)
        sound.setflags(write=False)
        peak = float(np.abs(sound).max())
    return dict(t_on=tw.t_on.copy(), t_off=tw.t_off.copy(), state=tw.state(), T=tw.T, forgotten=tw.forgotten,
                sound64=sound, peak=peak)


@functools.lru_cache(maxsize=None)
def stream_reference(case="a", n_sub=N_SUB, dt=DT, sr=SR, timbre=None, T0=0):
    """case_a fed `n_sub` rows at a time to every environment (all 64 rows of each: the environments' own lengths do not
    apply to a stream), on banks that are empty with the count at T0.  `timbre` is None or a name of timbre_of (the result
    is cached).  Per call a list over environments of bank_entry dicts: the twin's bank after the call and the float64
    sound of it; computed once."""
    trace, _ = ar.case_a()
    twins = [TrackerTwin(timbre_of(timbre)["tau_rel"], T0) for _ in range(len(trace))]
    calls = []
    for c in range(trace.shape[1] // n_sub):
        envs = []
        for e, tw in enumerate(twins):
            tw.track(trace[e, c * n_sub:(c + 1) * n_sub], dt)
            envs.append(bank_entry(tw, timbre, dt, sr, T0))
        calls.append(envs)
    return calls


def window64_of(r, W, timbre=None, dt=DT, sr=SR):
    """The float64 window of a bank_entry."""
    if r["sound64"] is not None:
        return window_of(r["sound64"], r["T"], W, dt, sr)
    return reference_window(r["t_on"], r["t_off"], r["T"], W, timbre, dt, sr)


def rounding_of(entries, tables, timbre=None, dt=DT, sr=SR):
    """(window, spectrum): max |float32 - float64| / peak of the restatements over the bank_entry dicts `entries`, for
    the analyses `tables` (names or (C, S) pairs)."""
    worst_w = worst_s = 0.0
    for r in entries:
        if r["peak"] == 0.0:
            continue
        for name in tables:
            C, S = analysis(name) if isinstance(name, str) else name
            W = C.shape[0]
            x64 = window64_of(r, W, timbre, dt, sr)
            x32 = reference_window(r["t_on"], r["t_off"], r["T"], W, timbre, dt, sr, np.float32)
            worst_w = max(worst_w, float(np.abs(x32.astype(np.float64) - x64).max()) / r["peak"])
            s64, s32 = reference_spectrum(x64, C, S), reference_spectrum(x32, C, S, np.float32)
            worst_s = max(worst_s, float(np.abs(s32.astype(np.float64) - s64).max()) / r["peak"])
    return worst_w, worst_s


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


def check_observation(r, name, window, spectrum, label, dt=DT, sr=SR, timbre=None, T0=0, tols=None):
    """One environment after one call: `r` of stream_reference (or a bank_entry of the same keys), against analysis
    `name` (a name of analysis() or a (C, S) pair).  `tols` = (window, spectrum) tolerances: the stream of case_a's by
    default, WIDE_TOLS for the wider cases.  With T0 > 0 the reference is the windowed one."""
    C, S = analysis(name) if isinstance(name, str) else name
    assert (r["sound64"] is None) == bool(T0)
    wtol, stol = (WINDOW_TOL, SPECTRUM_TOL) if tols is None else tols
    x64 = window64_of(r, C.shape[0], timbre, dt, sr)
    if window is not None:
        compare(window, x64, r["peak"], wtol, label + " window")
    s64 = reference_spectrum(x64, C, S)
    compare(spectrum, s64, r["peak"], stol, label + " spectrum")
    if not x64.any():
        assert not np.asarray(spectrum).any(), f"{label}: a silent window must read exact zeros"


def reference_of_rows(rows, sustain=None, n_sub=N_SUB, dt=DT, sr=SR, timbre=None, T0=0):
    """bank_entry of one environment after its rows [T][4] were consumed `n_sub` at a time, `sustain[i]` being call i's
    pedal flag, from an empty bank with the count at T0."""
    tw = TrackerTwin(timbre_of(timbre)["tau_rel"], T0)
    rows = np.asarray(rows, np.uint32).reshape(-1, 4)
    for i in range(len(rows) // n_sub):
        tw.track(rows[i * n_sub:(i + 1) * n_sub], dt, pedal=bool(sustain[i]) if sustain is not None else False)
    return bank_entry(tw, timbre, dt, sr, T0)


# ---- the wider cases: call shapes, forgotten voices, rates, timbres, late episodes ------------------------------------
FUZZ_CALLS = (1, 0, 3, 10, 0, 32)     # rows per call, repeated until a trace is used up (46 rows: exactly once)


def fuzz_traces():
    """The traces [5][T][4] of the first 10 of audio_reference.notes_fuzz_batches(); T is 46 in the first and between 30
    and 91 in the others."""
    return [b["trace"] for b in ar.notes_fuzz_batches()[:10]]


def call_spans(T, pattern=FUZZ_CALLS):
    """[(first row, end row)] of the calls that feed T rows `pattern` rows at a time, the last one cut at T."""
    spans, a, i = [], 0, 0
    while a < T:
        n = min(pattern[i % len(pattern)], T - a)
        spans.append((a, a + n))
        a, i = a + n, i + 1
    return spans


FORGET_KEYS = (0, 31, 32, 63, 64, 87)   # word boundaries, and both of the two keys a lane of the tracker carries


@functools.lru_cache(maxsize=None)
def forget_trace():
    """[3][16][4]: env 0 strikes each of FORGET_KEYS at substeps 2, 6 and 10 (0.02 s apart; 8 tau_rel = 0.4 s, so the
    third strike pushes out a voice that still sounds), env 1 does so on key 50 alone, env 2 plays nothing."""
    strikes = lambda k: [(k, 2, 3), (k, 6, 7), (k, 10, 11)]
    tr = np.stack([ar.make_trace(16, presses=[p for k in FORGET_KEYS for p in strikes(k)]),
                   ar.make_trace(16, presses=strikes(50)), ar.make_trace(16)])
    tr.setflags(write=False)
    return tr


@functools.lru_cache(maxsize=None)
def forget_reference():
    """forget_trace fed twice, one call each: per call, per env the bank_entry of the twin.  The sound is the bank's,
    whatever was forgotten."""
    twins = [TrackerTwin() for _ in range(3)]
    calls = []
    for _ in range(2):
        for tw, rows in zip(twins, forget_trace()):
            tw.track(rows)
        calls.append([bank_entry(tw) for tw in twins])
    assert [r["forgotten"] for r in calls[0]] == [6, 1, 0] and calls[1][0]["forgotten"] > 6
    return calls


def far_strikes():
    """Three strikes 100 substeps (0.5 s) apart on key 50: whether the first still sounds at the third is tau_rel's say."""
    return ar.make_trace(300, presses=[(50, 2, 3), (50, 102, 103), (50, 202, 203)])


RATES = ((44100, 0.005), (22050, 0.002), (8000, 0.0025))    # (sr, dt): 220.5, 44.1 and 20 samples per substep
LATE_T0 = (2_000_000, 24_999_900)                           # 10 000 s; N ends at 1 999 997 120, under the cap of 2e9
RATES_N_SUB = 3     # rows per call of the rates cases: T is odd after every other call (44.1 kHz: sr T dt = 220.5 T)
SINE_KEYS = (0, 40, 87)
SINE_SUBSTEPS = 60


@functools.lru_cache(maxsize=None)
def rate_analysis(sr):
    """Five bins at W = 512 for the sample rate `sr`."""
    from robopianist_amd.music import hearing
    C, S = hearing.make_analysis(sr, 512, freqs=hearing.key_frequencies()[[0, 31, 40, 63, 87]])
    for a in (C, S):
        a.setflags(write=False)
    return C, S


@functools.lru_cache(maxsize=None)
def sine_analysis(key):
    """One bin at the key's own fundamental, W = 2048, 16 kHz."""
    from robopianist_amd.music import hearing
    C, S = hearing.make_analysis(SR, 2048, freqs=hearing.key_frequencies()[[key]])
    for a in (C, S):
        a.setflags(write=False)
    return C, S


def sine_rows(key):
    return ar.make_trace(SINE_SUBSTEPS, presses=[(key, 0, SINE_SUBSTEPS - 1)])


@functools.lru_cache(maxsize=None)
def sine_reference(key):
    """bank_entry of one env that has held `key` for SINE_SUBSTEPS substeps, pure sine timbre."""
    return reference_of_rows(sine_rows(key), timbre="sine")


def rates_reference(sr):
    """The stream of case_a at the rate `sr` of RATES and its dt, RATES_N_SUB rows per call (21 calls)."""
    dt = next(x[1] for x in RATES if x[0] == sr)
    return stream_reference(n_sub=RATES_N_SUB, dt=dt, sr=sr)


def wide_case(name):
    """dict(dt, sr, timbre, T0, groups = [(bank_entry dicts, analyses)]) of a wider case: what the kernels are checked
    on under that name, and what measure_wide_rounding measures."""
    flat = lambda calls: [r for envs in calls for r in envs]
    kind, _, arg = name.partition("/")
    if kind == "rates":
        sr, dt = next(x for x in RATES if x[0] == int(arg))
        return dict(dt=dt, sr=sr, timbre=None, T0=0, groups=[(flat(rates_reference(sr)), [rate_analysis(sr)])])
    if kind == "late":
        return dict(dt=DT, sr=SR, timbre=None, T0=int(arg), groups=[(flat(stream_reference(T0=int(arg))), ["default"])])
    if name == "harsh":
        return dict(dt=DT, sr=SR, timbre="harsh", T0=0, groups=[(flat(stream_reference(timbre="harsh")), ["small"])])
    if name == "sine":
        return dict(dt=DT, sr=SR, timbre="sine", T0=0, groups=[([sine_reference(k)], [sine_analysis(k)]) for k in SINE_KEYS])
    if name == "forget":
        return dict(dt=DT, sr=SR, timbre=None, T0=0, groups=[(flat(forget_reference()), list(MAIN_ANALYSES))])
    raise KeyError(name)


WIDE_CASES = ("rates/44100", "rates/22050", "rates/8000", "harsh", "sine", "late/2000000", "late/24999900", "forget")


def measure_wide_rounding(names=WIDE_CASES):
    """((window, spectrum), per case): rounding_of over the groups of every wider case, the largest and, for the record,
    each case's own."""
    per_case = {}
    for name in names:
        case = wide_case(name)
        pairs = [rounding_of(entries, tables, case["timbre"], case["dt"], case["sr"]) for entries, tables in case["groups"]]
        per_case[name] = (max(p[0] for p in pairs), max(p[1] for p in pairs))
    return (max(v[0] for v in per_case.values()), max(v[1] for v in per_case.values())), per_case


# max |float32 - float64| / peak over the wider cases (measure_wide_rounding, on the CPU: 6.991e-07, the harsh timbre, and
# 6.348e-07, 44.1 kHz; window / spectrum per case: rates 5.7e-07 / 6.3e-07, 6.4e-07 / 2.4e-07 and 3.9e-07 / 2.6e-07, harsh
# 7.0e-07 / 1.1e-07, sine 5.9e-07 / 5.9e-07, late 4.7e-07 / 2.7e-07 and 5.3e-07 / 2.5e-07, forget 3.6e-07 / 8.1e-08)
MEASURED_WIDE_WINDOW_ROUNDING = 7.00e-7
MEASURED_WIDE_SPECTRUM_ROUNDING = 6.36e-7
WIDE_TOLS = (4 * MEASURED_WIDE_WINDOW_ROUNDING, 4 * MEASURED_WIDE_SPECTRUM_ROUNDING)   # (window, spectrum) of the wider cases


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
int rphh_analysis(rp_hear* h, const rp_hear_spectrum_args* g) {   // the analysis alone, on the caller's window
  const std::string err = rph_check_spectrum_args(g, h->n_envs);
  if (!err.empty()) return fail(err);
  if (!g->window) return fail("rphh_analysis: window must be given");
  rph_analysis_host(h->ana, g, g->window);
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
        L.rphh_analysis.argtypes = L.rphh_spectrum.argtypes
        _host_lib = L
    return _host_lib


class HostHearing:
    """The library's two calls on the CPU (rph_track_host, rph_window_host, rph_analysis_host), numpy arrays in and out."""

    def __init__(self, n_envs=1, analysis_tables=None, timbre=None, sr=SR, max_substeps_per_call=64, dt=DT, T0=0):
        from robopianist_amd.music import hearing, synthesizer
        self._H = hearing
        self._L = host_library()
        self.n_envs = n_envs
        C, S = analysis("default") if analysis_tables is None else analysis_tables
        self.W, self.B = C.shape
        self.dt = dt
        ab, bb = synthesizer.make_audio_blob(timbre_of(timbre), sr), hearing.make_analysis_blob(C, S)
        self._h = ctypes.c_void_p()
        if self._L.rphh_create(ab, len(ab), bb, len(bb), n_envs, max_substeps_per_call, 0, ctypes.byref(self._h)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())
        self.t_on = np.full((n_envs, N_KEYS, 2), -1.0)
        self.t_off = np.full((n_envs, N_KEYS, 2), -1.0)
        self.state = np.zeros((n_envs, 8), np.int32)
        self.state[:, 6] = T0

    def __del__(self):
        try:
            self._L.rphh_destroy(self._h)
        except Exception:
            pass

    def _bank(self):
        return self._H.Bank(self.t_on.ctypes.data, self.t_off.ctypes.data, self.state.ctypes.data)

    def track(self, trace, pedal=None, restart=None, dt=None, env_first=0, env_count=None):
        trace = np.ascontiguousarray(trace, np.uint32)
        pedal = None if pedal is None else np.ascontiguousarray(pedal, np.int32)
        restart = None if restart is None else np.ascontiguousarray(restart, np.int32)
        a = self._H.TrackArgs()
        a.struct_size = ctypes.sizeof(a)
        a.trace, a.n_sub = trace.ctypes.data, trace.shape[1]
        a.pedal = None if pedal is None else pedal.ctypes.data
        a.restart = None if restart is None else restart.ctypes.data
        a.dt, a.bank = self.dt if dt is None else dt, self._bank()
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        if self._L.rphh_track(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())

    def spectrum(self, dt=None, env_first=0, env_count=None, of_window=None):
        """(spectrum [E][B], window [E][W]); with `of_window` [E][W] float32 only rph_analysis_host runs, on that window."""
        window = np.zeros((self.n_envs, self.W), np.float32) if of_window is None else np.ascontiguousarray(of_window, np.float32)
        assert window.shape == (self.n_envs, self.W)
        spec = np.zeros((self.n_envs, self.B), np.float32)
        a = self._H.SpectrumArgs()
        a.struct_size = ctypes.sizeof(a)
        a.bank, a.dt = self._bank(), self.dt if dt is None else dt
        a.env_first, a.env_count = env_first, self.n_envs - env_first if env_count is None else env_count
        a.window, a.spectrum = window.ctypes.data, spec.ctypes.data
        if (self._L.rphh_spectrum if of_window is None else self._L.rphh_analysis)(self._h, ctypes.byref(a)) != 0:
            raise RuntimeError(self._L.rphh_last_error().decode())
        return spec, window
