"""CPU tests of the audio observation (include/audio/rp_hear.h): the tracker twin against the note rule's Python twin,
the g++ build of csrc/rp_hear.hpp against the twin and the float64 definition, the analysis table, the blobs.

Tolerances (tests/hear_reference.py): the float32 restatement against the float64 one over every call of the stream of
case_a and the five analyses differs by at most 4.73e-07 of the peak of the sound so far in the window and 3.57e-07 in the
spectrum; WINDOW_TOL and SPECTRUM_TOL are 4 x that.  Over the wider cases (other rates, timesteps and timbres, forgetting
banks, late episodes) it differs by at most 7.00e-07 and 6.36e-07; WIDE_TOLS is 4 x that.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import audio_reference as ar
import hear_reference as hr
from robopianist_amd.music import hearing, synthesizer


def _invariant(tw, rows, label):
    """The twin's bank equals the last two notes per key of the note list of the rows so far, to the bit."""
    notes, _ = ar.host_notes(rows, len(rows))
    want_on, want_off = hr.bank_of_notes(notes)
    assert tw.T == len(rows)
    assert hr.same_bits(tw.t_on, want_on) and hr.same_bits(tw.t_off, want_off), label


def _streams():
    """(label, rows [T][4]) of every environment of the fuzz batches and of case_a."""
    out = []
    for b, batch in enumerate(ar.notes_fuzz_batches()):
        for e in range(len(batch["trace"])):
            out.append((f"fuzz {b}/{e}", batch["trace"][e]))
    trace, _ = ar.case_a()
    return out + [(f"case_a/{e}", trace[e]) for e in range(len(trace))]


def test_tracker_twin_keeps_the_last_two_notes_for_every_prefix():
    n = 0
    for label, rows in _streams():
        tw = hr.TrackerTwin()
        for s in range(len(rows)):
            tw.track(rows[s:s + 1])
            _invariant(tw, rows[:s + 1], f"{label} after {s + 1} rows")
            n += 1
    assert n > 5000


@pytest.mark.parametrize("chunk", [1, 3, 10])
def test_tracker_twin_in_chunks_equals_one_shot(chunk):
    for label, rows in _streams():
        one = hr.TrackerTwin()
        one.track(rows)
        tw = hr.TrackerTwin()
        for s in range(0, len(rows), chunk):
            tw.track(rows[s:s + chunk])
        assert hr.same_bits(tw.t_on, one.t_on) and hr.same_bits(tw.t_off, one.t_off), label
        assert (tw.state() == one.state()).all(), label


def test_restart_mid_stream():
    trace, _ = ar.case_a()
    tw = hr.TrackerTwin()
    tw.track(trace[0, :20])
    assert (tw.t_on >= 0).any() and tw.T == 20
    tw.track(trace[0, 20:24], restart=True)   # the rows of a restarting call are not consumed
    assert (tw.t_on == -1).all() and (tw.t_off == -1).all() and (tw.state() == 0).all()
    tw.track(trace[1, :30])
    _invariant(tw, trace[1, :30], "after the restart")


def test_the_call_pedal_equals_bit_88_in_the_rows():
    for label, rows in _streams()[::7]:
        rows = rows.copy()
        rows[:, 2] &= ~np.uint32(1 << (ar.PEDAL % 32))
        flags = [bool((i // 2) % 2) for i in range((len(rows) + 3) // 4)]
        a, b = hr.TrackerTwin(), hr.TrackerTwin()
        for i, s in enumerate(range(0, len(rows), 4)):
            a.track(rows[s:s + 4], pedal=flags[i])
            marked = rows[s:s + 4].copy()
            if flags[i]:
                marked[:, 2] |= np.uint32(1 << (ar.PEDAL % 32))
            b.track(marked)
        assert hr.same_bits(a.t_on, b.t_on) and hr.same_bits(a.t_off, b.t_off) and (a.state() == b.state()).all(), label


def _three_strikes():
    """Key 50 struck at substeps 2, 6 and 10 (0.02 s apart, 8 tau_rel = 0.4 s), key 51 once."""
    return ar.make_trace(16, presses=[(50, 2, 3), (50, 6, 7), (50, 10, 11), (51, 4, 12)])


def test_three_strikes_forget_the_oldest():
    rows = _three_strikes()
    tw = hr.TrackerTwin()
    tw.track(rows)
    notes, _ = ar.host_notes(rows, 16)
    mine = [n for n in notes if n[0] == 50]
    assert len(mine) == 3 and tw.forgotten == 1
    assert [tw.t_on[50, 0], tw.t_on[50, 1]] == [mine[2][1], mine[1][1]]
    _invariant(tw, rows, "three strikes")
    # three strikes far apart forget nothing that sounds: 100 substeps = 0.5 s > 0.4 s + the note
    far = ar.make_trace(300, presses=[(50, 2, 3), (50, 102, 103), (50, 202, 203)])
    tw = hr.TrackerTwin()
    tw.track(far)
    assert tw.forgotten == 0


# ---- the g++ build of rp_hear.hpp ------------------------------------------------------------------------------------
def test_host_build_equals_the_twin_to_the_bit():
    """The bank and the state after every call of the stream, and the fuzz batches in one call each."""
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis("small"))
    for c, envs in enumerate(hr.stream_reference()):
        h.track(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB])
        for e, r in enumerate(envs):
            assert r["forgotten"] == 0
            assert hr.same_bits(h.t_on[e], r["t_on"]) and hr.same_bits(h.t_off[e], r["t_off"]), f"call {c} env {e}"
            assert (h.state[e] == r["state"]).all(), f"call {c} env {e}"
    for b, batch in enumerate(ar.notes_fuzz_batches()[:10]):
        tr = batch["trace"]
        h = hr.HostHearing(len(tr), hr.analysis("small"), max_substeps_per_call=ar.FUZZ_T_CAP)
        h.track(tr[:, :tr.shape[1] // 2])
        h.track(tr[:, tr.shape[1] // 2:])
        for e in range(len(tr)):
            tw = hr.TrackerTwin()
            tw.track(tr[e])
            assert hr.same_bits(h.t_on[e], tw.t_on) and hr.same_bits(h.t_off[e], tw.t_off), f"fuzz {b}/{e}"
            assert (h.state[e] == tw.state()).all(), f"fuzz {b}/{e}"


def test_host_build_forgets_restarts_and_takes_the_pedal():
    rows = _three_strikes()
    h = hr.HostHearing(2, hr.analysis("small"))
    both = np.stack([rows, rows])
    h.track(both, pedal=[0, 1])
    tw0, tw1 = hr.TrackerTwin(), hr.TrackerTwin()
    tw0.track(rows)
    tw1.track(rows, pedal=True)
    assert h.state[0, 7] == 1 and (h.state[0] == tw0.state()).all() and (h.state[1] == tw1.state()).all()
    assert hr.same_bits(h.t_off[1], tw1.t_off) and not hr.same_bits(h.t_off[0], h.t_off[1])
    h.track(both, restart=[1, 0])
    assert (h.t_on[0] == -1).all() and (h.t_off[0] == -1).all() and (h.state[0] == 0).all()
    tw1.track(rows, pedal=False)
    assert hr.same_bits(h.t_on[1], tw1.t_on) and (h.state[1] == tw1.state()).all()


@pytest.mark.parametrize("name", hr.ALL_ANALYSES)
def test_host_build_window_and_spectrum_match_the_definition(name):
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis(name))
    leading = 0
    for c, envs in enumerate(hr.stream_reference()):
        h.track(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB])
        spec, window = h.spectrum()
        for e, r in enumerate(envs):
            assert r["forgotten"] == 0
            hr.check_observation(r, name, window[e], spec[e], f"host {name} call {c} env {e}")
        leading += hr.last_sample(envs[0]["T"]) - h.W + 1 < 0
    assert name != "default" or leading >= 5, "no call with leading zeros"


def test_measured_rounding_is_what_the_constants_say():
    """The tolerance's source: the float32 restatement against the float64 one, over the calls and analyses above."""
    w, s = hr.measure_rounding()
    print(f"float32 vs float64 restatement: window {w:.3e}, spectrum {s:.3e} of the peak")
    assert w <= hr.MEASURED_WINDOW_ROUNDING and w >= 0.5 * hr.MEASURED_WINDOW_ROUNDING
    assert s <= hr.MEASURED_SPECTRUM_ROUNDING and s >= 0.5 * hr.MEASURED_SPECTRUM_ROUNDING
    (w, s), per_case = hr.measure_wide_rounding()
    for name, (cw, cs) in per_case.items():
        print(f"{name}: window {cw:.3e}, spectrum {cs:.3e} of the peak")
    assert set(per_case) == set(hr.WIDE_CASES) and all(cw > 0 and cs > 0 for cw, cs in per_case.values())
    assert 0.5 * hr.MEASURED_WIDE_WINDOW_ROUNDING <= w <= hr.MEASURED_WIDE_WINDOW_ROUNDING
    assert 0.5 * hr.MEASURED_WIDE_SPECTRUM_ROUNDING <= s <= hr.MEASURED_WIDE_SPECTRUM_ROUNDING
    assert hr.WIDE_TOLS == (4 * hr.MEASURED_WIDE_WINDOW_ROUNDING, 4 * hr.MEASURED_WIDE_SPECTRUM_ROUNDING)


def test_env_window_on_the_host_leaves_other_rows_alone():
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis("small"))
    h.track(trace[:, :8], env_first=1, env_count=1)
    assert (h.t_on[[0, 2]] == -1).all() and (h.state[[0, 2]] == 0).all() and h.state[1, 6] == 8
    with pytest.raises(RuntimeError, match="env window"):
        h.track(trace[:, :8], env_first=2, env_count=2)
    with pytest.raises(RuntimeError, match="exceeds max_substeps_per_call"):
        hr.HostHearing(3, hr.analysis("small"), max_substeps_per_call=4).track(trace[:, :8])


# ---- the wider cases (hear_reference.py), on the host build ------------------------------------------------------------
def test_windowed_reference_equals_the_full_one():
    """reference_window evaluates samples N - W + 1 .. N alone; on case_a it is the slice of the sound from sample 0, to
    the bit, in float64 and in the float32 restatement, with and without leading zeros."""
    n = 0
    for envs in hr.stream_reference():
        for r in envs:
            sound32 = hr.reference_sound(r["t_on"], r["t_off"], r["T"], dtype=np.float32)
            for W in (64, 128, 2048):
                assert hr.same_bits(hr.reference_window(r["t_on"], r["t_off"], r["T"], W), hr.window_of(r["sound64"], r["T"], W))
                assert hr.same_bits(hr.reference_window(r["t_on"], r["t_off"], r["T"], W, dtype=np.float32),
                                    hr.window_of(sound32, r["T"], W))
                n += bool(r["peak"])
            if r["peak"]:
                near = abs(hr.peak_so_far(r["t_on"], r["t_off"], r["T"]) - float(np.abs(r["sound64"][:hr.last_sample(r["T"]) + 1]).max()))
                assert near == 0.0
    assert n >= 90


def _same_bank(h, e, tw, label):
    assert hr.same_bits(h.t_on[e], tw.t_on) and hr.same_bits(h.t_off[e], tw.t_off), label
    assert (h.state[e] == tw.state()).all(), label


def test_host_build_on_the_fuzz_traces_in_every_call_shape():
    """One call of n_sub = max_substeps_per_call, and calls of 1, 0, 3, 10, 0, 32 rows: t_on, t_off and the 8 state words."""
    lengths, some_forgotten = set(), 0
    for b, tr in enumerate(hr.fuzz_traces()):
        E, T = tr.shape[:2]
        one = hr.HostHearing(E, hr.analysis("small"), max_substeps_per_call=T)
        one.track(tr)
        twins = [hr.TrackerTwin() for _ in range(E)]
        cut = hr.HostHearing(E, hr.analysis("small"), max_substeps_per_call=32)
        for a, z in hr.call_spans(T):
            before = (cut.t_on.copy(), cut.t_off.copy(), cut.state.copy())
            cut.track(tr[:, a:z])
            lengths.add(z - a)
            for e, tw in enumerate(twins):
                tw.track(tr[e, a:z])
                _same_bank(cut, e, tw, f"fuzz {b}/{e} rows {a}..{z}")
                held = tw.held
                assert (tw.t_off[held, 0] == tw.T * hr.DT).all()
            if z == a:
                assert all(hr.same_bits(x, y) for x, y in zip(before, (cut.t_on, cut.t_off, cut.state)))
        for e, tw in enumerate(twins):
            _same_bank(one, e, tw, f"fuzz {b}/{e} in one call")
            some_forgotten += tw.forgotten > 0
    assert hr.fuzz_traces()[0].shape == (5, 46, 4) and hr.call_spans(46) == [(0, 1), (1, 1), (1, 4), (4, 14), (14, 14), (14, 46)]
    assert {0, 1, 3, 10, 32} <= lengths and some_forgotten >= 5


def test_host_build_forgets_six_keys_in_one_call():
    tr = hr.forget_trace()
    h = hr.HostHearing(3, hr.analysis("small"))
    for c, envs in enumerate(hr.forget_reference()):
        h.track(tr)
        assert [int(x) for x in h.state[:, 7]] == [r["forgotten"] for r in envs]
        for e, r in enumerate(envs):
            assert hr.same_bits(h.t_on[e], r["t_on"]) and hr.same_bits(h.t_off[e], r["t_off"]) and (h.state[e] == r["state"]).all()
    assert [r["forgotten"] for r in hr.forget_reference()[0]] == [6, 1, 0]
    h.track(tr, restart=[1, 0, 0])
    assert (h.state[0] == 0).all() and h.state[1, 7] > hr.forget_reference()[1][1]["forgotten"]


@pytest.mark.parametrize("timbre, want", [(None, 0), ("tau_rel=0.2", 1), ("tau_rel=0.1", 0)])
def test_the_release_tail_decides_what_is_forgotten(timbre, want):
    """Three strikes 0.5 s apart: with 8 tau_rel = 1.6 s the first still sounds at the third, with 0.4 s or 0.8 s not."""
    rows = hr.far_strikes()
    tw = hr.TrackerTwin(hr.timbre_of(timbre)["tau_rel"])
    h = hr.HostHearing(1, hr.analysis("small"), timbre=timbre)
    for a in range(0, len(rows), 64):
        tw.track(rows[a:a + 64])
        h.track(rows[None, a:a + 64])
    assert tw.forgotten == want and tw.T == 300
    _same_bank(h, 0, tw, f"{timbre}")


@pytest.mark.parametrize("name", hr.MAIN_ANALYSES)
def test_host_build_on_forgetting_banks(name):
    """The definition is the bank's sound, whatever was forgotten."""
    h = hr.HostHearing(3, hr.analysis(name))
    for c, envs in enumerate(hr.forget_reference()):
        h.track(hr.forget_trace())
        spec, window = h.spectrum()
        for e, r in enumerate(envs):
            hr.check_observation(r, name, window[e], spec[e], f"host forget {name} call {c} env {e}", tols=hr.WIDE_TOLS)
    assert np.abs(spec[0]).max() > 0.01


@pytest.mark.parametrize("sr", [x[0] for x in hr.RATES])
def test_host_build_at_other_rates_and_timesteps(sr):
    case = hr.wide_case(f"rates/{sr}")
    dt, tables = case["dt"], hr.rate_analysis(sr)
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, tables, sr=sr, dt=dt)
    fractional = 0
    for c, envs in enumerate(hr.rates_reference(sr)):
        h.track(trace[:, c * hr.RATES_N_SUB:(c + 1) * hr.RATES_N_SUB])
        spec, window = h.spectrum()
        fractional += hr.last_sample(envs[0]["T"], dt, sr) != round(sr * envs[0]["T"] * dt)
        for e, r in enumerate(envs):
            assert hr.same_bits(h.t_on[e], r["t_on"]) and hr.same_bits(h.t_off[e], r["t_off"]) and (h.state[e] == r["state"]).all()
            hr.check_observation(r, tables, window[e], spec[e], f"host {sr} Hz call {c} env {e}", dt=dt, sr=sr,
                                 tols=hr.WIDE_TOLS)
    assert c == 20
    assert (fractional > 0) == (sr != 8000), "floor() must decide some N at a non-integer sr dt"
    if sr == 8000:    # key 87's partials at or above 0.45 sr are silenced
        assert (ar.partials(hr.default_timbre(), sr)[1][87] == 0).any() and (ar.partials(hr.default_timbre(), hr.SR)[1][87] != 0).any()


def test_host_build_with_the_harsh_timbre():
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis("small"), timbre="harsh")
    for c, envs in enumerate(hr.stream_reference(timbre="harsh")):
        h.track(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB])
        spec, window = h.spectrum()
        for e, r in enumerate(envs):
            assert hr.same_bits(h.t_on[e], r["t_on"]) and (h.state[e] == r["state"]).all()
            hr.check_observation(r, "small", window[e], spec[e], f"host harsh call {c} env {e}", timbre="harsh", tols=hr.WIDE_TOLS)


@pytest.mark.parametrize("key", hr.SINE_KEYS)
def test_host_build_reads_a_held_pure_sine_as_one(key):
    """The one check that a table that is transposed or scaled cannot pass while tracker and window are right."""
    tables, r = hr.sine_analysis(key), hr.sine_reference(key)
    h = hr.HostHearing(1, tables, timbre="sine")
    h.track(hr.sine_rows(key)[None])
    spec, window = h.spectrum()
    want = float(hr.reference_spectrum(hr.window64_of(r, 2048, "sine"), *tables)[0])
    print(f"key {key}: the float64 reference reads {want:.6f}, the host build {float(spec[0, 0]):.6f}")
    assert abs(want - 1.0) <= 1.5e-3
    hr.check_observation(r, tables, window[0], spec[0], f"host sine key {key}", timbre="sine", tols=hr.WIDE_TOLS)


@pytest.mark.parametrize("T0", hr.LATE_T0)
def test_host_build_late_in_an_episode(T0):
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis("default"), T0=T0)
    for c, envs in enumerate(hr.stream_reference(T0=T0)):
        h.track(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB])
        spec, window = h.spectrum()
        for e, r in enumerate(envs):
            assert r["T"] == T0 + hr.N_SUB * (c + 1)
            assert hr.same_bits(h.t_on[e], r["t_on"]) and hr.same_bits(h.t_off[e], r["t_off"]) and (h.state[e] == r["state"]).all()
            hr.check_observation(r, "default", window[e], spec[e], f"host T0 {T0} call {c} env {e}", T0=T0, tols=hr.WIDE_TOLS)
    N = hr.last_sample(envs[0]["T"])
    assert N <= 2.0e9 and (T0 != hr.LATE_T0[1] or N == 1_999_997_120)


def test_host_analysis_entry_is_the_analysis_of_the_spectrum_call():
    trace, _ = ar.case_a()
    h = hr.HostHearing(3, hr.analysis("wide"))
    h.track(trace[:, :40])
    spec, window = h.spectrum()
    again, _ = h.spectrum(of_window=window)
    assert spec.any() and hr.same_bits(spec, again)
    assert not h.spectrum(of_window=np.zeros_like(window))[0].any()


# ---- the analysis table -------------------------------------------------------------------------------------------------
def test_default_analysis_reads_a_unit_sine_as_one():
    """A unit sine at each of the 88 fundamentals, eight phases: the float64 definition reads 1 within 1.5e-3 (the worst of
    these 88 x 8 is 7.2e-4; the bound is twice that, because eight phases do not find the worst one)."""
    C, S = hearing.make_analysis(16000, 2048)
    assert C.shape == S.shape == (2048, 88) and C.dtype == S.dtype == np.float32
    t = np.arange(2048) / 16000.0
    worst = 0.0
    for b, f in enumerate(hearing.key_frequencies()):
        for p in range(8):
            x = np.sin(2.0 * np.pi * f * t + 2.0 * np.pi * p / 8.0 + 0.1)
            worst = max(worst, abs(float(hr.reference_spectrum(x, C[:, b:b + 1], S[:, b:b + 1])[0]) - 1.0))
    print(f"unit sines through the default table: worst |reading - 1| = {worst:.3e}")
    assert worst <= 1.5e-3
    # a bin's taps cover its newest L_b samples only
    L87 = int(np.ceil(16.0 * 16000 / hearing.key_frequencies()[87]))
    assert not C[:2048 - L87, 87].any() and not S[:2048 - L87, 87].any() and C[2048 - L87, 87] != 0


def test_blob_refusals():
    C, S = hr.analysis("small")
    good = hearing.make_analysis_blob(C, S)
    audio = synthesizer.make_audio_blob(None, hr.SR)
    L = hr.host_library()

    def create(ab, bb):
        out = ctypes.c_void_p()
        rc = L.rphh_create(ab, len(ab), bb, len(bb), 1, 8, 0, ctypes.byref(out))
        if rc == 0:
            L.rphh_destroy(out)
        return rc, L.rphh_last_error().decode()
    assert create(audio, good)[0] == 0
    rc, msg = create(audio, good[:-4])
    assert rc != 0 and "wrong size" in msg
    rc, msg = create(audio[:-8], good)
    assert rc != 0 and "wrong size" in msg
    import struct
    w100 = struct.pack("<IIii", 0x41485052, 1, 100, 5) + bytes(2 * 100 * 5 * 4)
    rc, msg = create(audio, w100)
    assert rc != 0 and "multiple of 64" in msg
    b129 = struct.pack("<IIii", 0x41485052, 1, 128, 129) + bytes(2 * 128 * 129 * 4)
    rc, msg = create(audio, b129)
    assert rc != 0 and "B must be in 1..128" in msg
    rc, msg = create(audio, b"XXXX" + good[4:])
    assert rc != 0 and "not an analysis blob" in msg
    with pytest.raises(ValueError, match="multiple of 64"):
        hearing.make_analysis_blob(np.zeros((100, 5), np.float32), np.zeros((100, 5), np.float32))
    with pytest.raises(ValueError, match="bins"):
        hearing.make_analysis_blob(np.zeros((128, 129), np.float32), np.zeros((128, 129), np.float32))


# ---- library ------------------------------------------------------------------------------------------------------------
def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        for part in stmt.strip().split(",") if stmt.strip() else []:
            names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", part)[-1])
    return names


def test_hear_abi_structs_and_symbols_match_the_header():
    src = open(os.path.join(hr.ROOT, "include", "audio", "rp_hear.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for cname, mirror in (("rp_hear_bank", hearing.Bank), ("rp_hear_track_args", hearing.TrackArgs),
                          ("rp_hear_spectrum_args", hearing.SpectrumArgs)):
        assert _struct_fields(src, cname) == [f[0] for f in mirror._fields_], cname
    assert sorted(set(re.findall(r"\b(rp_hear_[a-z_0-9]*)\s*\(", src))) == sorted(hearing.EXPORTED_SYMBOLS)
    hip = open(os.path.join(hr.ROOT, "robopianist_amd", "csrc", "rp_hear.hip")).read()
    for name in hearing.EXPORTED_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hip), name


def test_binding_raises_without_a_library():
    with pytest.raises(hearing.HearingError, match="not found"):
        hearing.load_library(os.path.join(hr.ROOT, "no_such_dir", "librp_hear.so"))


def test_the_library_is_one_of_its_own():
    """build() keeps rp_hear.* out of librp_engine.so's source list and rebuilds librp_hear.so when rp_audio.hpp changes;
    rp_hear.hpp is built on rp_audio.hpp."""
    src = open(os.path.join(hr.ROOT, "__graft_entry__.py")).read()
    assert "rp_hear." in eval(re.search(r"own = (.*)\n", src).group(1))
    block = src[src.index("librp_hear.so"):]
    assert "rp_audio.hpp" in block[:block.index("check_call")]
    csrc = os.path.join(hr.ROOT, "robopianist_amd", "csrc")
    assert '#include "rp_audio.hpp"' in open(os.path.join(csrc, "rp_hear.hpp")).read()
    for f in ("rp_engine.hip", "rp_task.hip", "rp_render.hip", "rp_audio.hip", "rp_video.hip"):
        assert "rp_hear" not in open(os.path.join(csrc, f)).read()
