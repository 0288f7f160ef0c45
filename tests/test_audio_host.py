"""The synthesiser without a GPU: the notes rule, known answers of the g++ build of csrc/rp_audio.hpp, that build against
the numpy reference on the GPU tests' cases, the ABI mirror and the file formats."""

import ctypes
import os
import re
import types
import wave

import numpy as np
import pytest

import audio_reference as ar
from robopianist_amd.music import audio, midi_file, midi_module, synthesizer

DT = ar.DT


def _both(trace, T=None, max_notes=64):
    """(Python twin's notes, host build's notes) of a one-environment trace."""
    T = len(trace) if T is None else T
    py, _ = ar.host_notes(trace, T)
    h = ar.HostAudio(n_envs=1, max_substeps=len(trace), max_notes=max_notes)
    cc = h.notes_from_trace(trace[None], [T])[0]
    return py, cc


# ---- the notes rule --------------------------------------------------------------------------------------------------
def test_press_and_release_without_the_pedal():
    py, cc = _both(ar.make_trace(20, presses=[(48, 3, 9)]))
    assert py == [(48, 4 * DT, 11 * DT, 127)]   # substep s has time (s+1) dt; the falling edge is substep 10
    assert cc == py


def test_release_under_the_pedal_is_deferred_to_pedal_up():
    py, cc = _both(ar.make_trace(30, presses=[(10, 2, 5)], pedal=[(4, 19)]))
    assert py == [(10, 3 * DT, 21 * DT, 127)]
    assert cc == py


def test_restrike_under_the_pedal_closes_the_old_note_at_the_new_onset():
    py, cc = _both(ar.make_trace(40, presses=[(87, 2, 4), (87, 10, 12)], pedal=[(0, 29)]))
    assert py == [(87, 3 * DT, 11 * DT, 127), (87, 11 * DT, 31 * DT, 127)]
    assert cc == py


def test_pedal_only_trace_gives_no_notes():
    py, cc = _both(ar.make_trace(16, pedal=[(2, 9)]))
    assert py == [] and cc == []
    ev = synthesizer.events_from_substep_trace(ar.make_trace(16, pedal=[(2, 9)]), DT)
    assert [type(e) for e in ev] == [midi_module.SustainOn, midi_module.SustainOff]


def test_key_still_down_at_the_end_is_released_at_T_dt():
    tr = ar.make_trace(16, presses=[(0, 5, 15), (64, 7, 15)])
    py, cc = _both(tr)
    assert py == [(0, 6 * DT, 16 * DT, 127), (64, 8 * DT, 16 * DT, 127)]
    assert cc == py
    py, cc = _both(tr, T=10)     # a shorter episode in the same buffer: the rows past it do not count
    assert py == [(0, 6 * DT, 10 * DT, 127), (64, 8 * DT, 10 * DT, 127)] and cc == py


def test_pedal_and_release_in_the_same_substep_keep_the_note():
    """held[s] = act[s] | (held[s-1] & pedal[s]): the pedal of the substep in which the key comes up already holds."""
    py, cc = _both(ar.make_trace(20, presses=[(30, 1, 4)], pedal=[(5, 9)]))
    assert py == [(30, 2 * DT, 11 * DT, 127)] and cc == py


def test_host_build_gives_the_identical_list_on_the_gpu_cases():
    for name in ("a", "b"):
        trace, lengths = ar.case_a() if name == "a" else ar.case_b()
        h = ar.HostAudio(n_envs=len(lengths), max_notes=128)
        got = h.notes_from_trace(trace, lengths)
        for e, (notes, _) in enumerate(ar.case_references(name)):
            assert got[e] == notes, f"case {name} env {e}"       # order included
            assert h.notes["dropped"][e] == 0
    keys = [n[0] for n in ar.case_references("b")[0][0]]
    assert keys == list(range(88))                                  # one substep: ordered by key


def test_max_notes_overflow_is_counted():
    trace, lengths = ar.case_a()
    full, _ = ar.host_notes(trace[0], 64)
    assert len(full) == 9
    h = ar.HostAudio(n_envs=3, max_notes=4)
    got = h.notes_from_trace(trace, lengths)
    kept, dropped = ar.host_notes(trace[0], 64, max_notes=4)
    assert dropped == 5 and h.notes["dropped"][0] == 5 and h.notes["count"][0] == 4
    assert got[0] == kept
    assert h.notes["dropped"][2] == 0 and h.notes["count"][2] == 0


# ---- known answers -----------------------------------------------------------------------------------------------------
def _a4_wave(timbre):
    trace = ar.make_trace(ar.T_CAP, presses=[(48, 3, 20)])
    h = ar.HostAudio(n_envs=1, max_notes=8, timbre=timbre)
    (notes,) = h.notes_from_trace(trace[None], [ar.T_CAP])
    w, _ = h.synthesize([ar.T_CAP], ar.T_CAP)
    return notes, w[0]


def test_pure_sine_a4_known_answer():
    tb = ar.pure_sine_timbre()
    notes, w = _a4_wave(tb)
    assert notes == [(48, 4 * DT, 22 * DT, 127)]
    _, t_on, t_off, _ = notes[0]
    t = np.arange(len(w)) / ar.SR
    u = t - t_on
    u_off = t_off - t_on
    att = 1 - np.exp(-u / tb["tau_att"])
    rel = np.where(u >= u_off, np.exp(-(u - u_off) / tb["tau_rel"]), 1.0)
    want = np.where((u >= 0) & (u < u_off + 8 * tb["tau_rel"]), np.sin(2 * np.pi * 440.0 * u) * att * rel, 0.0)
    err = np.abs(w - want).max()
    print(f"A4 pure sine: max error {err:.3e}, peak {np.abs(want).max():.4f}")
    assert err <= ar.WAVE_TOL * np.abs(want).max()
    before = t < t_on
    after = u >= u_off + 8 * tb["tau_rel"]
    assert before.sum() > 800 and after.sum() > 10000
    assert (w[before] == 0).all(), "samples before the onset must be exactly zero"
    assert (w[after] == 0).all(), "samples from t_off + 8 tau_rel on must be exactly zero"
    assert w[np.flatnonzero(~before)[1]] != 0 and w[np.flatnonzero(after)[0] - 1] != 0   # and only those


def test_partials_above_0p45_sr_contribute_exactly_zero():
    """C8 (4186 Hz): its partials 5..8 lie at or above 0.45 x 44100 Hz.  A table that gives only those an amplitude is
    silent, and the default table sounds like its first four partials alone."""
    f, amp, _ = ar.partials(synthesizer.DEFAULT_TIMBRE)
    assert (amp[87] != 0).tolist() == [True] * 4 + [False] * 4
    trace = ar.make_trace(ar.T_CAP, presses=[(87, 3, 20)])
    waves = {}
    for name, a in (("high", [0, 0, 0, 0, 1, 1, 1, 1]), ("all", 1 / np.arange(1, 9)), ("low", [1, 1 / 2, 1 / 3, 1 / 4, 0, 0, 0, 0])):
        tb = dict(synthesizer.DEFAULT_TIMBRE, a=np.asarray(a, float))
        h = ar.HostAudio(n_envs=1, max_notes=8, timbre=tb)
        h.notes_from_trace(trace[None], [ar.T_CAP])
        waves[name] = h.synthesize([ar.T_CAP], ar.T_CAP)[0][0]
    assert (waves["high"] == 0).all()
    assert np.abs(waves["all"]).max() > 0.5 and (waves["all"] == waves["low"]).all()


def test_empty_episode_is_all_zeros_and_never_divides_by_zero():
    h = ar.HostAudio(n_envs=1, max_notes=8)
    h.notes_from_trace(np.zeros((1, ar.T_CAP, 4), np.uint32), [ar.T_CAP])
    w, p = h.synthesize([ar.T_CAP], ar.T_CAP)
    assert (w == 0).all() and (p == 0).all()


# ---- the host build against the reference --------------------------------------------------------------------------------
def test_reference_rounding_supports_the_tolerance():
    """The float32 evaluation of the reference against its float64 evaluation over the cases: the wave tolerance is 4 x
    the largest difference (relative to the case's peak)."""
    worst = ar.measure_reference_rounding()
    print(f"reference rounding: {worst:.4e} of the peak")
    assert worst <= ar.MEASURED_WAVE_ROUNDING * 1.0005, "the recorded measurement no longer holds: re-measure"
    assert worst >= ar.MEASURED_WAVE_ROUNDING * 0.5, "the recorded measurement is padded: re-measure"
    assert ar.WAVE_TOL == 4 * ar.MEASURED_WAVE_ROUNDING
    assert 4 * ar.MEASURED_WAVE_ROUNDING * 32767 < 0.5      # so pcm differs from the reference's by at most one step


@pytest.mark.parametrize("name", ["a", "b"])
def test_host_build_matches_the_reference(name):
    trace, lengths = ar.case_a() if name == "a" else ar.case_b()
    h = ar.HostAudio(n_envs=len(lengths), max_notes=128)
    h.notes_from_trace(trace, lengths)
    wave_, pcm = h.synthesize(lengths, ar.T_CAP)
    for e, (notes, ref) in enumerate(ar.case_references(name)):
        ns = ar.n_samples(int(lengths[e]))
        assert (wave_[e, ns:] == 0).all() and (pcm[e, ns:] == 0).all()
        if not notes:
            assert (wave_[e] == 0).all() and (pcm[e] == 0).all()
            continue
        ar.compare_wave(wave_[e], ref, f"host {name}/{e}")
        ar.compare_pcm(pcm[e], ref, f"host {name}/{e}")
    if name == "b":
        assert len(ar.case_references("b")[0][0]) > h._L.rpah_dim(h._h, b"chunk_notes")


# ---- the wider cases (audio_reference.py), the CPU twins of the GPU tests ---------------------------------------------
def test_wide_reference_rounding_supports_the_wide_tolerance():
    """The same rule over the wider cases alone: WIDE_TOL is 4 x the reference's own float32 rounding on them."""
    worst, per_run = ar.measure_wide_reference_rounding()
    for label, r in per_run.items():
        print(f"reference rounding, {label}: {r:.4e} of the peak")
    assert worst <= ar.MEASURED_WIDE_ROUNDING * 1.0005, "the recorded measurement no longer holds: re-measure"
    assert worst >= ar.MEASURED_WIDE_ROUNDING * 0.5, "the recorded measurement is padded: re-measure"
    assert ar.WIDE_TOL == 4 * ar.MEASURED_WIDE_ROUNDING
    assert 4 * ar.MEASURED_WIDE_ROUNDING * 32767 < 0.5      # so pcm differs from the reference's by at most one step


def _host_run(run, max_notes=None):
    E = len(run["lists"])
    h = ar.HostAudio(n_envs=E, max_substeps=run["T"], max_notes=run["max_notes"] if max_notes is None else max_notes,
                     timbre=run["timbre"], sr=run["sr"])
    for e, notes in enumerate(run["lists"]):
        h.set_notes(e, notes)
    return h


@pytest.mark.parametrize("name", ar.WIDE_CASES)
def test_host_build_matches_the_reference_on_the_wide_cases(name):
    for run, refs in zip(ar.wide_case(name), ar.wide_references(name)):
        h = _host_run(run)
        w, p = h.synthesize([run["T"]] * len(refs), run["T"], dt=run["dt"])
        ar.check_rows(run, refs, w, p, "host")
    if name == "crowd":
        busiest, silent = ar.crowd_presence(h._L.rpah_dim(h._h, b"block_samples"))
        print(f"crowd: up to {busiest} notes audible in one block, {silent:.1%} of the entries do not sound")
        assert busiest > h._L.rpah_dim(h._h, b"chunk_notes")
        assert silent >= 0.2
    if name == "long":
        assert ar.n_samples(run["T"]) > 900 * h._L.rpah_dim(h._h, b"block_samples")
    if name == "rates":
        assert [ar.n_samples(r["T"], r["dt"], r["sr"]) for r in ar.case_rates()][3] == 1320      # 1000 Hz: two blocks


def test_edges_are_what_they_claim_and_count_is_clamped_on_the_host():
    """The edge list's times are sample times to the bit; count > max_notes reads max_notes entries, count < 0 none."""
    for (run, (ref,)), (tau_rel, cut) in zip(zip(ar.case_edges(), ar.wide_references("edges")), ((0.05, 5 * 4096), (0.01, 4096))):
        full, valid = ar.edges_lists(tau_rel, cut)
        assert ar.sounding(full) == valid and len(full) == 2 * len(valid) == 16 == run["max_notes"]
        t = np.arange(len(ref)) / ar.SR
        for n in (1023, 1024, 1025, 2047, 2048, 2049, 3072):
            assert sum(x[1] == t[n] for x in valid) + sum(x[2] == t[n] for x in valid) >= 1
        assert sorted(x[3] for x in valid if x[3] != 127)[:1] == [1] and {1, 64, 100, 127} <= {x[3] for x in valid}
        k25 = [x for x in valid if x[0] == 25][0]
        last = int(np.flatnonzero(ar.reference_wave([k25], run["T"], run["timbre"]))[-1])
        print(f"{run['label']}: key 25's cut-off was put on sample {cut}, its last sounding sample is {last}")
        assert abs(k25[2] + 8 * tau_rel - cut / ar.SR) < 1e-12 and last in (cut - 1, cut) and cut % 1024 == 0
        h = _host_run(run)
        w, p = h.synthesize([run["T"]], run["T"])
        h.notes["count"][0] = run["max_notes"] + 7
        w2, p2 = h.synthesize([run["T"]], run["T"])
        assert (w2.view(np.uint32) == w.view(np.uint32)).all() and (p2 == p).all()
        h.notes["count"][0] = -3
        w3, p3 = h.synthesize([run["T"]], run["T"])
        assert (w3 == 0).all() and (p3 == 0).all()


def test_notes_fuzz_on_the_host():
    """Random traces through rpa_notes_host against the Python twin, the cap included."""
    batches = ar.notes_fuzz_batches()
    for b, batch in enumerate(batches):
        h = ar.HostAudio(n_envs=5, max_substeps=ar.FUZZ_T_CAP, max_notes=batch["max_notes"])
        got = h.notes_from_trace(batch["trace"], batch["lengths"])
        for e, (notes, dropped) in enumerate(batch["want"]):
            assert got[e] == notes, f"batch {b} env {e}"
            assert h.notes["dropped"][e] == dropped, f"batch {b} env {e}"
    _fuzz_presence(batches)


def _fuzz_presence(batches):
    crossing = sum(sum(b["crossing"]) for b in batches)
    print(f"notes fuzz: {crossing} environments whose cap falls inside a substep with onsets on both sides of key 64")
    assert len(batches) == 40 and crossing >= 1
    assert {b["max_notes"] for b in batches} == {1, 7, 64, 4096}
    assert all(int(b["lengths"].max()) == b["trace"].shape[1] for b in batches)
    assert any(d == 0 and len(n) > 64 for b in batches for n, d in b["want"])      # and long lists that fit


def test_peak_rows_on_the_host():
    run, targets = ar.case_peak()
    refs = ar.peak_references()
    h = _host_run(run)
    w, p = h.synthesize(ar.PEAK_LENGTHS, ar.T_CAP)
    ar.check_rows(run, refs, w, p, "host")
    assert [i % 256 for i, _ in targets][1] == 255 and targets[0][0] == ar.n_samples(ar.PEAK_LENGTHS[0]) - 1 and targets[2][1] == -1
    for e, (index, sign) in enumerate(targets):
        assert p[e, index] == sign * 32767 and int(np.abs(p[e].astype(np.int32)).argmax()) == index


def test_slices_rows_on_the_host():
    """The 48 distinct rows of the GPU suite's 65 537-environment run."""
    S = ar.SLICES
    E = S["n_keys"]
    h = ar.HostAudio(n_envs=E, max_substeps=1, max_notes=S["max_notes"], sr=S["sr"])
    got = h.notes_from_trace(ar.slices_trace(np.arange(E)), np.ones(E, np.int32), dt=S["dt"])
    w, p = h.synthesize(np.ones(E, np.int32), 1, dt=S["dt"])
    assert w.shape == (E, 1005)
    run = dict(label="slices")
    assert [g for g in got] == [n for n, _ in ar.slices_references()] and all(len(g) == 1 for g in got)
    ar.check_rows(run, [r for _, r in ar.slices_references()], w, p, "host")
    f, amp, _ = ar.partials(synthesizer.DEFAULT_TIMBRE, S["sr"])
    assert (amp[:E, 0] != 0).all() and f[E - 1, 0] < 450.0


def test_env_window_leaves_other_rows_alone_on_the_host():
    trace, lengths = ar.case_a()
    h = ar.HostAudio(n_envs=3, max_notes=32)
    h.notes["key"][:] = -7
    h.notes_from_trace(trace, lengths, env_first=1, env_count=1)
    assert (h.notes["key"][[0, 2]] == -7).all() and h.notes["count"][1] == 4


def test_refused_arguments_on_the_host():
    h = ar.HostAudio(n_envs=1, max_substeps=ar.T_CAP, max_notes=8)
    with pytest.raises(RuntimeError, match="exceeds max_substeps"):
        h.notes_from_trace(np.zeros((1, ar.T_CAP + 1, 4), np.uint32), [ar.T_CAP + 1])
    with pytest.raises(RuntimeError, match="exceeds max_substeps"):
        h.synthesize([ar.T_CAP + 1], ar.T_CAP + 1)
    with pytest.raises(RuntimeError, match="env window"):
        h.synthesize([1], 1, env_first=1, env_count=1)
    blob = synthesizer.make_audio_blob()
    out = ctypes.c_void_p()
    assert h._L.rpah_create(blob[:-8], len(blob) - 8, 1, 8, 8, 0, ctypes.byref(out)) != 0
    assert b"wrong size" in h._L.rpah_last_error()


# ---- library and file formats ----------------------------------------------------------------------------------------------
def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        for part in stmt.strip().split(",") if stmt.strip() else []:
            names.append(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", re.sub(r"\[\d+\]", "", part))[-1])
    return names


def test_audio_abi_structs_and_symbols_match_the_header():
    src = open(os.path.join(ar.ROOT, "include", "audio", "rp_audio.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for cname, mirror in (("rp_audio_notes", synthesizer.Notes), ("rp_audio_notes_args", synthesizer.NotesArgs),
                          ("rp_audio_synth_args", synthesizer.SynthArgs)):
        assert _struct_fields(src, cname) == [f[0] for f in mirror._fields_], cname
    assert synthesizer.NotesArgs._fields_[0][0] == "struct_size" and synthesizer.SynthArgs._fields_[0][0] == "struct_size"
    assert sorted(set(re.findall(r"\b(rp_audio_[a-z_0-9]*)\s*\(", src))) == sorted(synthesizer.EXPORTED_SYMBOLS)


def test_missing_library_raises():
    with pytest.raises(synthesizer.AudioError, match="not found"):
        synthesizer.load_library(os.path.join(ar.ROOT, "no_such_dir", "librp_audio.so"))


def test_the_engine_library_does_not_depend_on_the_audio_sources():
    """build() keeps rp_audio.* out of librp_engine.so's staleness list, like rp_render.*."""
    src = open(os.path.join(ar.ROOT, "__graft_entry__.py")).read()
    assert '("rp_render.", "rp_audio.")' in src
    for f in ("rp_engine.hip", "rp_task.hip"):
        assert "rp_audio" not in open(os.path.join(ar.ROOT, "robopianist_amd", "csrc", f)).read()


def test_write_wav_reads_back_bit_exact(tmp_path):
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, 5000).astype(np.int16)
    audio.write_wav(tmp_path / "x.wav", pcm, 22050)
    with wave.open(str(tmp_path / "x.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (1, 2, 22050, 5000)
        back = np.frombuffer(wf.readframes(5000), "<i2")
    assert (back == pcm).all()
    with pytest.raises(ValueError):
        audio.write_wav(tmp_path / "y.wav", pcm.astype(np.float32))


def test_mid_round_trip(tmp_path):
    trace, _ = ar.case_a()
    events = synthesizer.events_from_substep_trace(trace[0], DT)
    song = midi_file.MidiFile.from_events(events)
    assert len(song.seq.notes) == 9 and len(song.seq.control_changes) == 2
    song.save(tmp_path / "played.mid")
    back = midi_file.MidiFile.from_file(tmp_path / "played.mid")
    key = lambda n: (round(n.start_time, 6), n.pitch)
    a, b = sorted(song.seq.notes, key=key), sorted(back.seq.notes, key=key)
    assert [(n.pitch, n.velocity) for n in a] == [(n.pitch, n.velocity) for n in b]
    np.testing.assert_allclose([(n.start_time, n.end_time) for n in b], [(n.start_time, n.end_time) for n in a], atol=1e-9)
    cc = lambda s: [(c.control_number, c.control_value) for c in s.seq.control_changes]
    assert cc(back) == cc(song) == [(64, 127), (64, 0)]
    np.testing.assert_allclose([c.time for c in back.seq.control_changes], [c.time for c in song.seq.control_changes], atol=1e-9)
    # a note that ends where the next one of its pitch begins stays two notes
    ev = [midi_module.NoteOn(60, 127, 0.1), midi_module.NoteOn(60, 100, 0.2), midi_module.NoteOff(60, 0.3)]
    midi_file.MidiFile.from_events(ev).save(tmp_path / "twice.mid")
    twice = midi_file.MidiFile.from_file(tmp_path / "twice.mid").seq.notes
    assert [(n.pitch, n.velocity, round(n.start_time, 9), round(n.end_time, 9)) for n in twice] == \
           [(60, 127, 0.1, 0.2), (60, 100, 0.2, 0.3)]


def test_save_proto_is_unchanged(tmp_path):
    from robopianist_amd import music
    song = music.load("TwinkleTwinkleRousseau")
    song.save(tmp_path / "t.proto")
    back = midi_file.MidiFile.from_file(tmp_path / "t.proto")
    assert [(n.pitch, n.start_time, n.end_time, n.velocity) for n in back.seq.notes] == \
           [(n.pitch, n.start_time, n.end_time, n.velocity) for n in song.seq.notes]
    with pytest.raises(ValueError):
        song.save(tmp_path / "t.txt")


def test_blob_layout():
    blob = synthesizer.make_audio_blob(ar.pure_sine_timbre(), 48000)
    assert len(blob) == 16 + 8 * (3 + 8 + 88 + 88 * 8)
    assert np.frombuffer(blob[:16], "<i4").tolist()[2:] == [1, 0]
    assert np.frombuffer(blob[16:40], "<f8").tolist() == [48000.0, 0.002, 0.05]
    with pytest.raises(ValueError):
        synthesizer.make_audio_blob(dict(synthesizer.DEFAULT_TIMBRE, H=9))


def test_sound_wrapper_refuses_environments_it_cannot_record(tmp_path):
    from robopianist_amd.wrappers import PianoSoundWrapper
    with pytest.raises(ValueError, match="piano"):
        PianoSoundWrapper(types.SimpleNamespace(task=types.SimpleNamespace()), tmp_path)
    with pytest.raises(ValueError, match="record_key_trace"):
        PianoSoundWrapper(types.SimpleNamespace(task=types.SimpleNamespace(piano=object()), key_trace=None), tmp_path)
