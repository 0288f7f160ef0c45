"""GPU tests of the synthesiser (include/audio/rp_audio.h, librp_audio.so) and the sound-recording wrapper.

dt = 0.005, 44.1 kHz, 64 substeps per row: 58 212 samples with the tail, 57 sample blocks of 1024.  The numpy reference,
the cases and the tolerance are the CPU suite's (tests/audio_reference.py: the reference in float32 against itself in
float64 differs by 4.84e-07 of the peak on these cases; WAVE_TOL = 4 x 4.85e-07 = 1.94e-06 of the peak; pcm within 1).
The wider cases further down (other timbres, rates and row lengths, host-made note lists, 65 537 environments, the
recorder on a scripted environment) have their own measured tolerance, WIDE_TOL, by the same rule.
"""
import os
import warnings
import wave

import numpy as np
import pytest
import torch

import audio_reference as ar
from robopianist_amd.music import midi_file, midi_module, synthesizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAP = ar.n_samples(ar.T_CAP)


def _np(x):
    return x.detach().cpu().numpy()


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda:0").to(dtype)


def _trace(tr):
    return _dev(tr.view(np.int32))


def _synth(n_envs, max_notes=128, **kw):
    return synthesizer.Synthesizer(n_envs=n_envs, sample_rate=ar.SR, max_substeps=ar.T_CAP, max_notes=max_notes,
                                   physics_timestep=ar.DT, **kw)


def _lists(s):
    n = {k: _np(v) for k, v in s.notes.items()}
    return [ar.notes_from_arrays(n["key"][e], n["t_on"][e], n["t_off"][e], n["velocity"][e], n["count"][e])
            for e in range(s.n_envs)], n["dropped"]


@pytest.fixture(scope="module")
def run_a():
    trace, lengths = ar.case_a()
    s = _synth(3)
    w, p = s.synthesize_trace(_trace(trace), lengths)
    torch.cuda.synchronize()
    return s, _np(w).copy(), _np(p).copy(), _lists(s)


def test_case_a_matches_the_reference(run_a):
    """(a) three environments of lengths 64, 37 and 0."""
    s, w, p, (lists, dropped) = run_a
    _, lengths = ar.case_a()
    assert w.shape == p.shape == (3, N_CAP) and N_CAP == 58212
    assert s._L.rp_audio_dim(s._h, b"block_samples") * 10 < N_CAP
    for e, (notes, ref) in enumerate(ar.case_references("a")):
        assert lists[e] == notes, f"env {e}: the device note list differs from the host twin"
        assert dropped[e] == 0
        ns = ar.n_samples(int(lengths[e]))
        assert (w[e, ns:] == 0).all() and (p[e, ns:] == 0).all(), "samples past n_samples_e must be zero"
        if notes:
            ar.compare_wave(w[e], ref, f"gpu a/{e}")
            ar.compare_pcm(p[e], ref, f"gpu a/{e}")
            assert (w[e][ref == 0] == 0).all(), "silent stretches must be exact zeros"
    assert len(ar.case_references("a")[0][0]) == 9 and len(ar.case_references("a")[1][0]) == 4
    assert np.isfinite(w).all() and (w[2] == 0).all() and (p[2] == 0).all()      # the empty episode
    # a note of env 0 sounds across more than 10 blocks
    key63 = [n for n in lists[0] if n[0] == 63][0]
    assert (key63[2] + 0.4 - key63[1]) * ar.SR > 10 * 1024


def test_more_audible_notes_than_one_chunk():
    """(b) all 88 keys struck in one substep, under the pedal."""
    trace, lengths = ar.case_b()
    s = _synth(1)
    assert s._L.rp_audio_dim(s._h, b"chunk_notes") < 88
    w, p = s.synthesize_trace(_trace(trace), lengths)
    (notes, ref), = ar.case_references("b")
    lists, dropped = _lists(s)
    assert lists[0] == notes and len(notes) == 88 and dropped[0] == 0
    ar.compare_wave(_np(w)[0], ref, "gpu b")
    ar.compare_pcm(_np(p)[0], ref, "gpu b")


def test_env_window_leaves_other_rows_bit_identical(run_a):
    """(c) env_first=1, env_count=1."""
    _, w_all, p_all, _ = run_a
    trace, lengths = ar.case_a()
    s = _synth(3)
    w, p = s.outputs(N_CAP)
    w.fill_(-123.25); p.fill_(-77)
    for k, v in s.notes.items():
        v.fill_(-5)
    w2, p2 = s.synthesize_trace(_trace(trace), lengths, env_first=1, env_count=1)
    assert w2 is w and p2 is p
    w, p = _np(w), _np(p)
    assert (w[[0, 2]] == -123.25).all() and (p[[0, 2]] == -77).all()
    for k, v in s.notes.items():
        assert (_np(v)[[0, 2]] == -5).all(), k
    assert (w[1] == w_all[1]).all() and (p[1] == p_all[1]).all()


def test_note_cap_drops_and_counts(run_a):
    """(d) max_notes smaller than the trace needs."""
    trace, lengths = ar.case_a()
    s = _synth(3, max_notes=4)
    w, _ = s.synthesize_trace(_trace(trace), lengths)
    lists, dropped = _lists(s)
    kept, host_dropped = ar.host_notes(trace[0], 64, max_notes=4)
    assert host_dropped == 5 and dropped.tolist() == [5, 0, 0] and _np(s.dropped).tolist() == [5, 0, 0]
    assert lists[0] == kept and lists[1] == ar.case_references("a")[1][0]
    ref = ar.reference_wave(kept, 64, synthesizer.DEFAULT_TIMBRE, n_cap=N_CAP)
    ar.compare_wave(_np(w)[0], ref, "gpu capped")


def test_two_runs_are_bitwise_equal(run_a):
    """(e)"""
    _, w1, p1, (lists1, _) = run_a
    trace, lengths = ar.case_a()
    s = _synth(3)
    w, p = s.synthesize_trace(_trace(trace), lengths)
    lists, _ = _lists(s)
    assert lists == lists1
    assert (_np(w).view(np.uint32) == w1.view(np.uint32)).all() and (_np(p) == p1).all()


def test_refusals_launch_nothing():
    """(f) host-side argument checks: nothing is launched, the buffers keep their contents, the error text is set."""
    trace, lengths = ar.case_a()
    s = _synth(3)
    w, p = s.outputs(N_CAP)
    w.fill_(9.5); p.fill_(11)
    for v in s.notes.values():
        v.fill_(-5)
    tr, ln = _trace(trace), _dev(lengths)
    long_tr = _trace(np.zeros((3, ar.T_CAP + 1, 4), np.uint32))
    long_ln = _dev(np.full(3, ar.T_CAP + 1, np.int32))
    torch.cuda.synchronize()

    bad = s.notes_args(tr, ln, ar.DT); bad.struct_size -= 8
    assert s.notes_raw(bad) != 0 and "struct_size" in s.last_error()
    assert s.notes_raw(s.notes_args(long_tr, long_ln, ar.DT)) != 0 and "exceeds max_substeps" in s.last_error()
    assert s.notes_raw(s.notes_args(tr, ln, ar.DT, env_first=2, env_count=2)) != 0 and "env window" in s.last_error()
    bad = s.synth_args(ln, ar.DT, ar.T_CAP, w, p); bad.struct_size += 8
    assert s.synthesize_raw(bad) != 0 and "struct_size" in s.last_error()
    assert s.synthesize_raw(s.synth_args(long_ln, ar.DT, ar.T_CAP + 1, w, p)) != 0 and "exceeds max_substeps" in s.last_error()
    assert s.synthesize_raw(s.synth_args(ln, ar.DT, ar.T_CAP, w[:, :1000].contiguous(), None)) != 0 and "n_cap" in s.last_error()
    with pytest.raises(synthesizer.AudioError, match="lengths must lie"):
        s.synthesize_trace(tr, [ar.T_CAP + 1, 0, 0])
    with pytest.raises(synthesizer.AudioError, match="exceeds max_substeps"):
        s.synthesize_trace(long_tr, long_ln)
    torch.cuda.synchronize()
    assert bool((w == 9.5).all()) and bool((p == 11).all())
    for k, v in s.notes.items():
        assert bool((v == -5).all()), k
    assert s.notes_raw(s.notes_args(tr, ln, ar.DT)) == 0 and s.synthesize_raw(s.synth_args(ln, ar.DT, ar.T_CAP, w, p)) == 0
    torch.cuda.synchronize()
    assert not bool((w == 9.5).any()) and int(s.notes["count"][0]) == 9


def test_get_samples_of_an_event_list():
    """The reference's Synthesizer.get_samples: events in, int16 samples with one second of tail out."""
    trace, _ = ar.case_a()
    events = synthesizer.events_from_substep_trace(trace[0], ar.DT)
    end = events[-1].time
    s = _synth(1)
    got = s.get_samples(events)
    assert got.dtype == np.int16 and got.shape == (int(np.ceil(ar.SR * (end + 1.0))),)
    ref = ar.reference_wave(synthesizer.notes_from_events(events, end), 1, synthesizer.DEFAULT_TIMBRE, dt=end)
    ar.compare_pcm(got, ref, "get_samples")
    assert np.abs(got).max() >= 32766


def test_sound_wrapper_end_to_end(tmp_path):
    """(g) PianoWithShadowHands on the Twinkle replay, 2 envs, env 0 recorded."""
    from robopianist_amd import suite
    from robopianist_amd.suite.scripted import ScriptedActions
    from robopianist_amd.wrappers import CanonicalSpecWrapper, PianoSoundWrapper
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))

    def load(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=2, seed=11,
                              task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                               primitive_fingertip_collisions=True), **kw)
    with pytest.raises(ValueError, match="record_key_trace"):
        PianoSoundWrapper(load(), tmp_path / "none")
    base = load(record_key_trace=True)
    env = PianoSoundWrapper(CanonicalSpecWrapper(base), tmp_path / "rec", record_envs=(0,), export_midi=True)
    dev, dtype = base.physics.device, base.physics.dtype
    script = ScriptedActions(torch.as_tensor(actions, dtype=dtype, device=dev), torch.zeros(2, dtype=torch.long, device=dev))
    dt = base.task.physics_timestep
    env.reset()
    traces, sustain, times = [], [], []
    for t in range(len(actions) + 5):
        ts = env.step(script)
        traces.append(_np(base.key_trace).view(np.uint32).copy())
        sustain.append(bool(base.task.piano.sustain_activation[0, 0]))
        times.append(float(base.physics.time[0]))
        if bool(ts.last()[0]):
            break
    print(f"episode: {len(traces)} control steps")
    assert bool(ts.last()[0]) and len(actions) == 158 and len(traces) >= 150
    events = midi_module.events_from_trace(np.stack(traces), sustain, times, dt, env=0)
    # The definition puts the event of substep s at (s+1) dt.  events_from_trace derives its times from the accumulated
    # physics time, which is that to ~1e-14 s; where (s+1) dt sr is a whole number (every even s+1), so is the sample
    # at which a voice's 8 tau_rel cut-off falls, and a time that is off in the last bit moves that cut-off by a sample
    # (e^-8 of the voice: 2 pcm steps between two float64 references on such times).  The times are therefore checked
    # against the grid and put on it.
    for e in events:
        k = round(e.time / dt)
        assert abs(e.time - k * dt) < 1e-9, "the physics time is not the definition's (s+1) dt"
        e.time = k * dt
    n_on = sum(isinstance(e, midi_module.NoteOn) for e in events)
    assert n_on >= 1, "the replay pressed no key: the test shows nothing"
    wavs, mids = sorted((tmp_path / "rec").glob("*.wav")), sorted((tmp_path / "rec").glob("*.mid"))
    assert [p.name for p in wavs] == ["0000_00000.wav"] and [p.name for p in mids] == ["0000_00000.mid"]
    T = len(traces) * traces[0].shape[1]
    with wave.open(str(wavs[0]), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate()) == (1, 2, ar.SR)
        got = np.frombuffer(wf.readframes(wf.getnframes()), "<i2")
    assert len(got) == ar.n_samples(T, dt)
    notes = synthesizer.notes_from_events(events, T * dt)
    assert len(notes) == n_on
    ref = ar.reference_wave(notes, T, synthesizer.DEFAULT_TIMBRE, dt=dt)
    ar.compare_pcm(got, ref, "wrapper wav")
    # the exported MIDI file loads to the notes as played
    played = midi_file.MidiFile.from_events(events).seq.notes
    back = sorted(midi_file.MidiFile.from_file(mids[0]).seq.notes, key=lambda n: (round(n.start_time, 6), n.pitch))
    assert [n.pitch for n in back] == [n.pitch for n in played]
    np.testing.assert_allclose([(n.start_time, n.end_time) for n in back], [(n.start_time, n.end_time) for n in played], atol=3e-4)
    # an episode without a note writes nothing: the hands hold their reset pose
    quiet = load(record_key_trace=True)
    qenv = PianoSoundWrapper(quiet, tmp_path / "quiet", record_envs=(0, 1))
    zero = torch.zeros((2,) + tuple(quiet.action_spec().shape), dtype=dtype, device=dev)
    qenv.reset()
    pressed = 0
    for t in range(len(actions) + 5):
        ts = qenv.step(zero)
        pressed += int((quiet.key_trace.view(torch.int32)[..., :3] != 0).sum())
        if bool(ts.last().all()):
            break
    assert bool(ts.last().all())
    assert pressed == 0, "the zero action pressed a key: the check below shows nothing"
    assert list((tmp_path / "quiet").iterdir()) == [] and qenv.written == []


# ---- the wider cases (tests/audio_reference.py): other timbres, rates, host note lists, many environments ---------------
# Their tolerance is the same rule measured on them alone: the reference in float32 against itself in float64 differs by
# at most 5.95e-07 of the peak on these cases (the 20 s undamped sine), WIDE_TOL = 4 x 5.95e-07 = 2.38e-06; pcm within 1.
def _wide_synth(run, n_envs=None, **kw):
    return synthesizer.Synthesizer(n_envs=len(run["lists"]) if n_envs is None else n_envs, sample_rate=run["sr"],
                                   max_substeps=run["T"], max_notes=run["max_notes"], physics_timestep=run["dt"],
                                   timbre=run["timbre"], **kw)


def _run_lists(run):
    """The run's lists through set_notes / synthesize_notes; (synthesiser, wave, pcm) on the device."""
    s = _wide_synth(run)
    for e, notes in enumerate(run["lists"]):
        s.set_notes(e, notes)
    w, p = s.synthesize_notes([run["T"]] * s.n_envs, run["T"])
    torch.cuda.synchronize()
    return s, w, p


@pytest.mark.parametrize("name", ar.WIDE_CASES)
def test_wide_cases_match_the_reference(name):
    """long, harsh, rates, edges, crowd: every run's rows against the numpy reference of sounding(list)."""
    for run, refs in zip(ar.wide_case(name), ar.wide_references(name)):
        s, w, p = _run_lists(run)
        assert tuple(w.shape) == tuple(p.shape) == (len(refs), ar.n_samples(run["T"], run["dt"], run["sr"]))
        assert int(s.dropped.sum()) == 0
        for e, ref in enumerate(refs):                      # (one copy of a row at a time: a row of `long` is 3.9 MB)
            ar.check_rows(run, [ref], [_np(w[e])], [_np(p[e])], f"gpu[{e}]")
    if name == "crowd":
        busiest, silent = ar.crowd_presence(s._L.rp_audio_dim(s._h, b"block_samples"))
        print(f"crowd: up to {busiest} notes audible in one block, {silent:.1%} of the entries do not sound")
        assert busiest > s._L.rp_audio_dim(s._h, b"chunk_notes")
        assert silent >= 0.2
    if name == "long":
        assert ar.n_samples(run["T"]) > 900 * s._L.rp_audio_dim(s._h, b"block_samples")


def test_edges_count_above_max_notes_and_below_zero():
    """The edge list again: count > max_notes gives the bits of count = max_notes, count < 0 an all-zero wave and pcm."""
    for run in ar.case_edges():
        s, w, p = _run_lists(run)
        assert s.max_notes == len(run["lists"][0]) == 16
        w1, p1 = w.clone(), p.clone()
        s.notes["count"][0] = s.max_notes + 7
        w.fill_(7.5); p.fill_(7)
        w2, p2 = s.synthesize_notes([run["T"]], run["T"])
        assert bool((w2.view(torch.int32) == w1.view(torch.int32)).all()) and bool((p2 == p1).all())
        s.notes["count"][0] = -3
        w.fill_(7.5); p.fill_(7)
        w3, p3 = s.synthesize_notes([run["T"]], run["T"])
        assert bool((w3 == 0).all()) and bool((p3 == 0).all())


def test_notes_fuzz_matches_the_python_twin():
    """Random traces through the note builder alone: 40 batches of 5 environments, the cap falling inside substeps."""
    batches = ar.notes_fuzz_batches()
    crossing = 0
    for b, batch in enumerate(batches):
        s = synthesizer.Synthesizer(n_envs=5, max_substeps=ar.FUZZ_T_CAP, max_notes=batch["max_notes"], physics_timestep=ar.DT)
        for v in s.notes.values():
            v.fill_(-5)
        s.notes_from_trace(_trace(batch["trace"]), batch["lengths"])
        lists, dropped = _lists(s)
        for e, (notes, want_dropped) in enumerate(batch["want"]):
            assert lists[e] == notes, f"batch {b} env {e}: the device note list differs from the host twin"
            assert dropped[e] == want_dropped, f"batch {b} env {e}"
            assert (_np(s.notes["key"])[e, len(notes):] == -5).all(), "entries past count must stay untouched"
        crossing += sum(batch["crossing"])
    print(f"notes fuzz: {crossing} environments whose cap falls inside a substep with onsets on both sides of key 64")
    assert len(batches) == 40 and crossing >= 1


def test_more_environments_than_one_launch_takes():
    """65 537 environments: the synthesis goes out in two launches, the second of 2 rows.  Row e repeats row e % 48."""
    S = ar.SLICES
    E, K = S["n_envs"], S["n_keys"]
    s = synthesizer.Synthesizer(n_envs=E, sample_rate=S["sr"], max_substeps=S["T"], max_notes=S["max_notes"],
                                physics_timestep=S["dt"])
    n_cap = ar.n_samples(S["T"], S["dt"], S["sr"])
    assert E > 65535 + 1 and n_cap == 1005
    trace = _trace(ar.slices_trace(np.arange(E)))
    lengths = torch.ones(E, dtype=torch.int32, device="cuda:0")
    w, p = s.outputs(n_cap)
    w.fill_(-123.25); p.fill_(-32768)          # sentinels that are no sample: |wave| stays below 2, |pcm| <= 32767
    w2, p2 = s.synthesize_trace(trace, lengths)
    assert w2 is w and p2 is p
    torch.cuda.synchronize()
    refs = ar.slices_references()
    key, count = _np(s.notes["key"]), _np(s.notes["count"])
    assert (count == 1).all() and (key[:, 0] == np.arange(E) % K).all() and int(s.dropped.sum()) == 0
    ar.check_rows(dict(label="slices"), [r for _, r in refs], _np(w[:K]), _np(p[:K]), "gpu")
    idx = torch.arange(E, device="cuda:0") % K
    same_w = (w.view(torch.int32) == w.view(torch.int32)[idx]).all(dim=1)
    same_p = (p == p[idx]).all(dim=1)
    bad = torch.nonzero(~(same_w & same_p)).flatten().tolist()
    assert not bad, f"rows {bad[:8]} differ from row e % {K}"
    assert bool(same_w[[65534, 65535, 65536]].all()) and bool((w[65536] != 0).any())      # the second launch wrote
    assert not bool((w == -123.25).any()) and not bool((p == -32768).any()), "a sentinel survived"
    # a window across the same rows, on re-filled buffers, writes those rows and nothing else
    first = w[:K].clone(), p[:K].clone()
    w.fill_(-123.25); p.fill_(-32768)
    for v in s.notes.values():
        v.fill_(-5)
    s.synthesize_trace(trace, lengths, env_first=65530, env_count=7)
    torch.cuda.synchronize()
    assert bool((w[:65530] == -123.25).all()) and bool((p[:65530] == -32768).all())
    assert bool((s.notes["count"][:65530] == -5).all()) and bool((s.notes["count"][65530:] == 1).all())
    rows = torch.arange(65530, E, device="cuda:0") % K
    assert bool((w[65530:].view(torch.int32) == first[0].view(torch.int32)[rows]).all()) and bool((p[65530:] == first[1][rows]).all())


def test_pcm_peak_in_the_last_sample_in_lane_255_and_negative():
    """The pcm kernel's peak reduction: the row's largest |sample| is the last one before n_samples_e, one with index
    = 255 (mod 256), a negative one.  The wave buffer holds larger values, which the call overwrites, past n_samples_e."""
    run, targets = ar.case_peak()
    refs = ar.peak_references()
    s = _wide_synth(run)
    for e, notes in enumerate(run["lists"]):
        s.set_notes(e, notes)
    w = torch.full((3, N_CAP), 1.0e9, dtype=torch.float32, device="cuda:0")
    p = torch.full((3, N_CAP), -77, dtype=torch.int16, device="cuda:0")
    lengths = _dev(np.asarray(ar.PEAK_LENGTHS, np.int32))
    assert s.synthesize_raw(s.synth_args(lengths, ar.DT, ar.T_CAP, w, p)) == 0, s.last_error()
    torch.cuda.synchronize()
    w, p = _np(w), _np(p)
    ar.check_rows(run, refs, w, p, "gpu")
    assert targets[0][0] == ar.n_samples(ar.PEAK_LENGTHS[0]) - 1 and targets[1][0] % 256 == 255 and targets[2][1] == -1
    for e, (index, sign) in enumerate(targets):
        ns = ar.n_samples(ar.PEAK_LENGTHS[e])
        assert index < ns and (w[e, ns:] == 0).all() and (p[e, ns:] == 0).all()
        print(f"peak row {e}: pcm[{index}] = {p[e, index]}, the row's extreme is at {int(np.abs(p[e].astype(np.int32)).argmax())}")
        assert p[e, index] == sign * 32767 and int(np.abs(p[e].astype(np.int32)).argmax()) == index
        assert (p[e] == ar.reference_pcm(refs[e]))[index]
    assert ar.n_samples(ar.PEAK_LENGTHS[0]) < ar.n_samples(ar.PEAK_LENGTHS[2]) < N_CAP


class _ScriptedPianoEnv:
    """No physics: `step` installs the scripted key trace and sustain activation and returns the scripted step types."""
    n_envs = 4

    def __init__(self, script, dt=ar.DT):
        import types
        dev = torch.device("cuda", 0)
        self._script, self._t = script, 0
        self.key_trace = torch.zeros((4, 4, 4), dtype=torch.int32, device=dev)
        self.physics = types.SimpleNamespace(device=dev)
        self.task = types.SimpleNamespace(physics_timestep=dt, piano=types.SimpleNamespace(
            sustain_activation=torch.zeros((4, 1), dtype=torch.bool, device=dev)))

    def reset(self):
        import types
        return types.SimpleNamespace(step_type=torch.zeros(4, dtype=torch.long, device=self.physics.device))

    def step(self, action):
        import types
        step_type, trace, sustain = self._script[self._t]
        self._t += 1
        self.key_trace.copy_(_trace(trace))
        self.task.piano.sustain_activation[:, 0] = _dev(np.asarray(sustain, bool))
        return types.SimpleNamespace(step_type=_dev(np.asarray(step_type, np.int64)))


def _recorder_script(rng):
    """Per env a list of episodes, each a list of recorded steps (rows [4][4] uint32, sustain); then the step script.
    An env's first episode starts right after reset(); every later one starts with a FIRST step whose rows are junk."""
    def keys(n_steps, lo, hi):
        steps = []
        for _ in range(n_steps):
            rows = np.zeros((4, 4), np.uint32)
            for k in rng.integers(lo, hi, 3):
                a = int(rng.integers(0, 3))
                rows[a:int(rng.integers(a + 1, 5)), k // 32] |= np.uint32(1) << np.uint32(k % 32)
            steps.append((rows, bool(rng.integers(0, 2))))
        return steps
    pedal_only = [(np.zeros((4, 4), np.uint32), True), (np.zeros((4, 4), np.uint32), False)]
    episodes = {0: [keys(2, 0, 88), keys(3, 0, 88), keys(2, 0, 88), keys(9, 0, 88)],
                1: [pedal_only, keys(4, 0, 88), keys(6, 0, 88), keys(2, 0, 88)],        # the third: 24 substeps > 16
                2: [keys(5, 0, 88), keys(4, 0, 88), keys(8, 0, 88)],
                3: [keys(3, 0, 88), keys(2, 0, 88), keys(4, 60, 88), keys(6, 0, 88)]}
    FIRST, MID, LAST = 0, 1, 2
    lanes = {}
    for e, eps in episodes.items():
        lane = []
        for i, ep in enumerate(eps):
            if i:
                lane.append((FIRST, np.full((4, 4), 0xFFFFFFFF, np.uint32), True))
            lane += [(LAST if j == len(ep) - 1 else MID, rows, sus) for j, (rows, sus) in enumerate(ep)]
        lanes[e] = lane
    n_steps = 15                                                   # env 1's three episodes: 2 + 1 + 4 + 1 + 6 + 1
    assert all(len(lane) >= n_steps for lane in lanes.values())
    script = [([lanes[e][t][0] for e in range(4)], np.stack([lanes[e][t][1] for e in range(4)]),
               [lanes[e][t][2] for e in range(4)]) for t in range(n_steps)]
    return episodes, lanes, script


def _episode_trace(steps):
    """[4 len(steps)][4] uint32 of recorded steps: their rows, with the step's sustain as bit 88 of its four substeps."""
    rows = np.concatenate([r for r, _ in steps])
    for j, (_, sus) in enumerate(steps):
        if sus:
            rows[4 * j:4 * j + 4, ar.PEDAL // 32] |= np.uint32(1 << (ar.PEDAL % 32))
    return rows


def test_sound_wrapper_tracked_index_is_not_the_env_index(tmp_path):
    """record_envs=(3, 1), record_every=2, three episodes per tracked env on a scripted environment."""
    from robopianist_amd.wrappers import PianoSoundWrapper
    episodes, lanes, script = _recorder_script(np.random.default_rng(7))
    ends = {e: [t for t in range(len(script)) if lanes[e][t][0] == 2] for e in (1, 3)}
    assert len(ends[1]) == len(ends[3]) == 3 and not set(ends[1]) & set(ends[3]), "the episodes must end at different steps"
    assert any(lanes[e][t][0] == 2 for e in (0, 2) for t in range(len(script)))      # the untracked envs finish episodes too
    base = _ScriptedPianoEnv(script)
    env = PianoSoundWrapper(base, tmp_path / "rec", record_envs=(3, 1), record_every=2, max_substeps=16, max_notes=64)
    env.reset()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in script:
            env.step(None)
    truncated = [str(c.message) for c in caught if "truncated" in str(c.message)]
    assert len(truncated) == 1 and "env 1's" in truncated[0], truncated
    names = sorted(q.name for q in (tmp_path / "rec").iterdir())
    # env 3: episodes 0 and 2; env 1: episode 0 has pedal bits only (no file, but it counts), episode 2 is truncated
    assert names == ["0001_00002.wav", "0003_00000.wav", "0003_00002.wav"]
    assert sorted(q.name for q in env.written) == names
    for name, e, ep, n_rec in (("0003_00000.wav", 3, 0, 3), ("0003_00002.wav", 3, 2, 4), ("0001_00002.wav", 1, 2, 4)):
        rows = _episode_trace(episodes[e][ep][:n_rec])
        T = len(rows)
        notes, _ = ar.host_notes(rows, T)
        assert notes, "the scripted episode has no note: the check shows nothing"
        with wave.open(str(tmp_path / "rec" / name), "rb") as wf:
            assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate()) == (1, 2, ar.SR)
            got = np.frombuffer(wf.readframes(wf.getnframes()), "<i2")
        assert len(got) == ar.n_samples(T)
        ar.compare_pcm(got, ar.reference_wave(notes, T, synthesizer.DEFAULT_TIMBRE), f"recorder {name}")
    assert len(episodes[1][2]) * 4 > 16 and len(episodes[3][1]) != len(episodes[3][0]) != len(episodes[3][2])
    silent = _episode_trace(episodes[1][0])
    assert ar.host_notes(silent, 8) == ([], 0) and silent.any()
