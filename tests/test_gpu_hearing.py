"""GPU tests of the audio observation (include/audio/rp_hear.h, librp_hear.so) and of AudioObservationWrapper.

dt = 0.005, 16 kHz, four substeps per call: the stream of case_a is 16 calls, N = 320 (c + 1) after call c, so a window of
2048 samples starts before sample 0 in the first six of them and has leading zeros there.  The twin, the float64 restatement and the tolerances
are the CPU suite's (tests/hear_reference.py: the float32 restatement against the float64 one differs by 4.73e-07 of the
peak of the sound so far in the window and 3.57e-07 in the spectrum; the tolerances are 4 x that).

The wider cases (the second half of this file; their definitions, twins and references are hear_reference.py's, and
test_hearing_host.py checks the host build on the same ones): call shapes n_sub = 0, 1, uneven and max, voices forgotten on
the device, more environments than one tile row of the analysis and than one launch of the window kernel, other sample
rates, timesteps and timbres, episodes that are thousands of seconds old, and the summation order of the analysis.  Their
tolerances are hr.WIDE_TOLS: 4 x (7.00e-07, 6.36e-07), the float32 restatement against the float64 one over those cases.
"""
import collections
import os
import types
import warnings

import numpy as np
import pytest
import torch

import audio_reference as ar
import hear_reference as hr
from robopianist_amd.music import hearing, synthesizer
from robopianist_amd.suite import specs
from robopianist_amd.suite.specs import StepType, TimeStep

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CALLS = ar.T_CAP // hr.N_SUB


def _np(x):
    return x.detach().cpu().numpy()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _trace(tr):
    return _dev(np.ascontiguousarray(tr).view(np.int32))


def _hearing(n_envs, name, **kw):
    kw.setdefault("max_substeps_per_call", 8)
    return hearing.Hearing(n_envs, sample_rate=hr.SR, analysis=hr.analysis(name), physics_timestep=hr.DT, **kw)


def _stream(name, n_envs=3, env_map=None, **window):
    """Feeds case_a four rows at a time; per call (t_on, t_off, state, spectrum, window) on the host."""
    trace, _ = ar.case_a()
    if env_map is not None:
        trace = trace[env_map]
    h = _hearing(n_envs, name)
    out = []
    for c in range(N_CALLS):
        spec, wave = h.observe(_trace(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB]), window=True, **window)
        out.append(tuple(_np(x).copy() for x in (h.t_on, h.t_off, h.state, spec, wave)))
    return h, out


@pytest.fixture(scope="module")
def main_runs():
    return {name: _stream(name)[1] for name in hr.MAIN_ANALYSES}


@pytest.mark.parametrize("name", hr.MAIN_ANALYSES)
def test_stream_of_case_a_matches_the_reference(main_runs, name):
    """E = 3, n_sub = 4, checked after every call: the bank to the bit, window and spectrum within tolerance, exact zeros."""
    C, _ = hr.analysis(name)
    leading = 0
    for c, (envs, got) in enumerate(zip(hr.stream_reference(), main_runs[name])):
        t_on, t_off, state, spec, wave = got
        assert spec.shape == (3, C.shape[1]) and wave.shape == (3, C.shape[0])
        for e, r in enumerate(envs):
            assert r["forgotten"] == 0, "the case must not hide behind forgotten voices"
            assert hr.same_bits(t_on[e], r["t_on"]) and hr.same_bits(t_off[e], r["t_off"]), f"call {c} env {e}: the bank"
            assert (state[e] == r["state"]).all(), f"call {c} env {e}: the state"
            hr.check_observation(r, name, wave[e], spec[e], f"gpu {name} call {c} env {e}")
        n_lead = max(0, C.shape[0] - 1 - hr.last_sample(envs[0]["T"]))
        leading += n_lead > 0
        assert (wave[:, :n_lead] == 0).all(), "samples before sample 0 must be exact zeros"
    assert leading == (6 if name == "default" else 0)
    assert 2 * hr.analysis("default")[0].shape[1] % 32 != 0     # 2B = 176 is no multiple of the tile
    assert len(hr.notes_of_bank(hr.stream_reference()[-1][2]["t_on"], hr.stream_reference()[-1][2]["t_off"])) == 88   # > one chunk


def test_window_is_the_slice_of_the_synthesiser(main_runs):
    """The same sound from the existing kernel: rp_audio_synthesize on the accumulated trace, sliced to [N - W + 1, N]."""
    trace, _ = ar.case_a()
    s = synthesizer.Synthesizer(n_envs=3, sample_rate=hr.SR, max_substeps=ar.T_CAP, max_notes=128, physics_timestep=hr.DT)
    for name in hr.MAIN_ANALYSES:
        W = hr.analysis(name)[0].shape[0]
        for c in (0, 3, 6, 10, 15):
            T = hr.N_SUB * (c + 1)
            wave, _ = s.synthesize_trace(_trace(trace[:, :T]), [T] * 3, pcm=False)
            wave = _np(wave)
            assert int(_np(s.dropped).max()) == 0
            for e, r in enumerate(hr.stream_reference()[c]):
                want = hr.window_of(wave[e], T, W)
                got = main_runs[name][c][4][e]
                err = float(np.abs(got.astype(np.float64) - want).max())
                print(f"{name} call {c} env {e}: max |window - synthesiser| = {err:.3e}, peak {r['peak']:.4f}")
                assert err <= (ar.WAVE_TOL + hr.WINDOW_TOL) * r["peak"]
                assert (got[want == 0] == 0).all()


@pytest.mark.parametrize("name", ["one", "wide", "short"])
def test_other_shapes(name):
    """B = 1, B = 128 and W = 64."""
    C, _ = hr.analysis(name)
    assert C.shape == dict(one=(256, 1), wide=(512, 128), short=(64, 4))[name]
    _, runs = _stream(name)
    for c, (envs, got) in enumerate(zip(hr.stream_reference(), runs)):
        for e, r in enumerate(envs):
            assert hr.same_bits(got[0][e], r["t_on"]) and hr.same_bits(got[1][e], r["t_off"])
            hr.check_observation(r, name, got[4][e], got[3][e], f"gpu {name} call {c} env {e}")


def test_env_window_leaves_other_rows_bit_identical():
    """E = 65 with the env window [1, 64): the rows 0 and 64 keep their prefilled bank, state, window and spectrum."""
    trace, _ = ar.case_a()
    env_map = np.arange(65) % 3
    h = _hearing(65, "small")
    spec, wave = h.outputs()
    outside = [0, 64]
    h.t_on[outside] = -7.5; h.t_off[outside] = 3.25; h.state[outside] = -5
    spec.fill_(9.5); wave.fill_(-123.25)
    for c in range(6):
        got = h.observe(_trace(trace[env_map][:, c * hr.N_SUB:(c + 1) * hr.N_SUB]), window=True, env_first=1, env_count=63)
        assert got[0] is spec and got[1] is wave
    t_on, t_off, state, spec, wave = (_np(x) for x in (h.t_on, h.t_off, h.state, spec, wave))
    assert (t_on[outside] == -7.5).all() and (t_off[outside] == 3.25).all() and (state[outside] == -5).all()
    assert (spec[outside] == 9.5).all() and (wave[outside] == -123.25).all()
    for e in range(1, 64):
        r = hr.stream_reference()[5][env_map[e]]
        assert hr.same_bits(t_on[e], r["t_on"]) and hr.same_bits(t_off[e], r["t_off"]) and (state[e] == r["state"]).all()
        hr.check_observation(r, "small", wave[e], spec[e], f"gpu window env {e}")
    assert h._L.rp_hear_dim(h._h, b"tile_envs") == 64


def test_two_runs_are_bitwise_equal(main_runs):
    for name in hr.MAIN_ANALYSES:
        _, again = _stream(name)
        for first, second in zip(main_runs[name], again):
            for a, b in zip(first, second):
                assert hr.same_bits(a, b)


def test_internal_window_buffer_gives_the_same_spectrum(main_runs):
    trace, _ = ar.case_a()
    h = _hearing(3, "default")
    for c in range(N_CALLS):
        spec = h.observe(_trace(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB]))
        assert hr.same_bits(_np(spec), main_runs["default"][c][3])


def test_refusals_launch_nothing():
    """Host-side argument checks: nothing is launched, the buffers keep their contents, the error text is set."""
    trace, _ = ar.case_a()
    h = _hearing(3, "small")
    spec, wave = h.outputs()
    spec.fill_(9.5); wave.fill_(11.0)
    h.t_on.fill_(-7.5); h.t_off.fill_(3.25); h.state.fill_(-5)
    tr, long_tr = _trace(trace[:, :4]), _trace(trace[:, :9])
    torch.cuda.synchronize()

    assert h.spectrum_raw(h.spectrum_args(None, wave)) != 0 and "spectrum must not be NULL" in h.last_error()
    bad = h.spectrum_args(spec, wave); bad.struct_size -= 8
    assert h.spectrum_raw(bad) != 0 and "struct_size" in h.last_error()
    bad = h.track_args(tr); bad.struct_size += 8
    assert h.track_raw(bad) != 0 and "struct_size" in h.last_error()
    assert h.track_raw(h.track_args(tr, env_first=2, env_count=2)) != 0 and "env window" in h.last_error()
    assert h.spectrum_raw(h.spectrum_args(spec, wave, env_first=-1, env_count=2)) != 0 and "env window" in h.last_error()
    assert h.spectrum_raw(h.spectrum_args(spec, wave, env_first=3, env_count=1)) != 0 and "env window" in h.last_error()
    assert h.track_raw(h.track_args(long_tr)) != 0 and "exceeds max_substeps_per_call" in h.last_error()
    with pytest.raises(hearing.HearingError, match="exceeds max_substeps_per_call"):
        h.track(long_tr)
    with pytest.raises(hearing.HearingError, match="trace"):
        h.track(_trace(trace[:2, :4]))
    torch.cuda.synchronize()
    assert bool((spec == 9.5).all()) and bool((wave == 11.0).all())
    assert bool((h.t_on == -7.5).all()) and bool((h.t_off == 3.25).all()) and bool((h.state == -5).all())
    restart = torch.ones(3, dtype=torch.int32, device="cuda:0")
    assert h.track_raw(h.track_args(tr, restart=restart)) == 0 and h.spectrum_raw(h.spectrum_args(spec, wave)) == 0
    torch.cuda.synchronize()
    assert bool((spec == 0).all()) and bool((wave == 0).all()) and bool((h.t_on == -1).all()) and bool((h.state == 0).all())


# ---- the wider cases ------------------------------------------------------------------------------------------------------
def _make(n_envs, tables, sr=hr.SR, dt=hr.DT, timbre=None, max_sub=64, T0=0):
    h = hearing.Hearing(n_envs, sample_rate=sr, analysis=hr.analysis(tables) if isinstance(tables, str) else tables,
                        timbre=hr.timbre_of(timbre), physics_timestep=dt, max_substeps_per_call=max_sub)
    if T0:
        h.state[:, 6] = T0     # an empty bank late in an episode
    return h


def _bank(h):
    return tuple(_np(x).copy() for x in (h.t_on, h.t_off, h.state))


def _same_bank(bank, e, want, label):
    """`want`: a TrackerTwin or a bank_entry."""
    t_on, t_off, state = (want.t_on, want.t_off, want.state()) if isinstance(want, hr.TrackerTwin) else (want["t_on"], want["t_off"], want["state"])
    assert hr.same_bits(bank[0][e], t_on) and hr.same_bits(bank[1][e], t_off), f"{label}: the bank"
    assert (bank[2][e] == state).all(), f"{label}: the state is {bank[2][e].tolist()}, the twin's {state.tolist()}"


def test_tracker_on_the_fuzz_traces_in_every_call_shape():
    """The first 10 fuzz batches ([5][T][4], T = 46 in the first, 30..91 in the others), each in one call of n_sub = T =
    max_substeps_per_call, and in calls of 1, 0, 3, 10, 0 and 32 rows (repeated while rows are left): t_on, t_off and all 8
    state words against the twin after every call.  A call of no rows changes nothing."""
    lengths, at_max, forgotten = set(), 0, 0
    for b, tr in enumerate(hr.fuzz_traces()):
        E, T = tr.shape[:2]
        one = _make(E, "short", max_sub=T)
        one.track(_trace(tr))
        at_max += one._L.rp_hear_dim(one._h, b"max_substeps_per_call") == T == int(_np(one.substeps)[0])
        cut = _make(E, "short", max_sub=32)
        twins = [hr.TrackerTwin() for _ in range(E)]
        before = _bank(cut)
        for a, z in hr.call_spans(T):
            cut.track(_trace(tr[:, a:z]))
            after = _bank(cut)
            lengths.add(z - a)
            for e, tw in enumerate(twins):
                tw.track(tr[e, a:z])
                _same_bank(after, e, tw, f"fuzz {b}/{e} rows {a}..{z}")
                assert (after[1][e][tw.held, 0] == tw.T * hr.DT).all(), "a held key's note ends at T dt"
            if z == a:
                assert all(hr.same_bits(x, y) for x, y in zip(before, after)), "a call of no rows changed the bank"
            before = after
        got = _bank(one)
        for e, tw in enumerate(twins):
            _same_bank(got, e, tw, f"fuzz {b}/{e} in one call")
            forgotten += tw.forgotten
    print(f"fuzz: call lengths {sorted(lengths)}, {forgotten} voices forgotten in all")
    assert at_max == 10 and {0, 1, 3, 10, 32} <= lengths and forgotten >= 10
    assert hr.fuzz_traces()[0].shape == (5, 46, 4) and hr.call_spans(46) == [(0, 1), (1, 1), (1, 4), (4, 14), (14, 14), (14, 46)]


@pytest.mark.parametrize("name", hr.MAIN_ANALYSES)
def test_six_keys_forget_in_one_call(name):
    """Keys 0, 31, 32, 63, 64 and 87 struck three times in one 16-row call: `forgotten` is 6 (the wave sum, the keys 64 and
    87 from the lanes' second key), 1 in the env that strikes key 50 alone, 0 in the silent one; a second call of the same
    rows adds the twin's count; a restart zeroes it.  Window and spectrum are the bank's sound, whatever was forgotten."""
    tr = _trace(hr.forget_trace().copy())
    h = _make(3, name)
    for c, envs in enumerate(hr.forget_reference()):
        spec, wave = h.observe(tr, window=True)
        bank, spec, wave = _bank(h), _np(spec), _np(wave)
        assert _np(h.forgotten).tolist() == [r["forgotten"] for r in envs]
        if c == 0:
            assert _np(h.forgotten).tolist() == [6, 1, 0]
        for e, r in enumerate(envs):
            _same_bank(bank, e, r, f"forget call {c} env {e}")
            hr.check_observation(r, name, wave[e], spec[e], f"gpu forget {name} call {c} env {e}", tols=hr.WIDE_TOLS)
    assert envs[0]["forgotten"] == 6 + 18 and np.abs(spec[0]).max() > 0.01
    h.track(tr, restart=_dev(np.array([1, 0, 0], np.int32)))
    bank = _bank(h)
    assert (bank[2][0] == 0).all() and (bank[0][0] == -1).all() and (bank[1][0] == -1).all()
    assert bank[2][1, 7] == envs[1]["forgotten"] + 3 and bank[2][2, 7] == 0 and bank[2][1, 6] == 48


@pytest.mark.parametrize("timbre, want", [(None, 0), ("tau_rel=0.2", 1), ("tau_rel=0.1", 0)])
def test_the_release_tail_decides_what_is_forgotten(timbre, want):
    """Three strikes 0.5 s apart in calls of at most 64 rows: 8 tau_rel = 1.6 s forgets the first, 0.4 s and 0.8 s do not."""
    rows = hr.far_strikes()
    tw = hr.TrackerTwin(hr.timbre_of(timbre)["tau_rel"])
    h = _make(1, "short", timbre=timbre)
    for a in range(0, len(rows), 64):
        tw.track(rows[a:a + 64])
        h.track(_trace(rows[None, a:a + 64]))
    assert tw.forgotten == want and tw.T == 300
    _same_bank(_bank(h), 0, tw, f"timbre {timbre}")
    assert int(_np(h.forgotten)[0]) == want


def test_pedal_and_restart_mixed_in_one_call():
    """Per-env flags of one device call: pedal [0, 1, 1], restart [0, 0, 1]."""
    rows = ar.make_trace(16, presses=[(50, 2, 3), (50, 6, 7), (50, 10, 11), (51, 4, 12), (87, 1, 2)])
    tr = _trace(np.stack([rows] * 3))
    h = _make(3, "short")
    twins = [hr.TrackerTwin() for _ in range(3)]
    h.track(tr)
    for tw in twins:
        tw.track(rows)
    h.track(tr, pedal=_dev(np.array([0, 1, 1], np.int32)), restart=_dev(np.array([False, False, True])))
    twins[0].track(rows)
    twins[1].track(rows, pedal=True)
    twins[2].track(rows, pedal=True, restart=True)
    bank = _bank(h)
    for e, tw in enumerate(twins):
        _same_bank(bank, e, tw, f"env {e}")
    assert (bank[2][2] == 0).all() and (bank[0][2] == -1).all()
    assert not hr.same_bits(bank[1][0], bank[1][1]) and bank[2][0, 7] > 1


@pytest.mark.parametrize("name, n_envs, first, count", [("small", 131, 1, 129), ("default", 66, 0, 66)])
def test_more_environments_than_one_tile_row(name, n_envs, first, count):
    """The analysis kernel with blockIdx.y > 0 and a partial last tile row: env e replays pattern e % 3 of case_a, six
    calls; every env of the window against the reference, the envs outside it keep their sentinels."""
    trace, _ = ar.case_a()
    env_map = np.arange(n_envs) % 3
    h = _make(n_envs, name, max_sub=8)
    tile = h._L.rp_hear_dim(h._h, b"tile_envs")
    assert tile == 64 and count > tile and count % tile != 0, "more than one tile row, the last one partial"
    refs = hr.stream_reference()[5]
    # the row maps of the kernel stride by 1, 4, 16 and 64 envs: envs that far apart must have different references
    assert all(d % 3 != 0 for d in (1, 4, 16, 64))
    C, S = hr.analysis(name)
    specs = [hr.reference_spectrum(hr.window64_of(r, C.shape[0]), C, S) for r in refs]
    for i in range(3):
        for j in range(i):
            assert np.abs(specs[i] - specs[j]).max() > 1e-3 * max(r["peak"] for r in refs) and not hr.same_bits(refs[i]["t_on"], refs[j]["t_on"])
    spec, wave = h.outputs()
    outside = [e for e in range(n_envs) if not first <= e < first + count]
    assert outside == ([0, 130] if name == "small" else [])
    if outside:
        h.t_on[outside] = -7.5; h.t_off[outside] = 3.25; h.state[outside] = -5
    spec.fill_(9.5); wave.fill_(-123.25)
    for c in range(6):
        h.observe(_trace(trace[env_map][:, c * hr.N_SUB:(c + 1) * hr.N_SUB]), window=True, env_first=first, env_count=count)
    bank, spec, wave = _bank(h), _np(spec), _np(wave)
    assert (bank[0][outside] == -7.5).all() and (bank[1][outside] == 3.25).all() and (bank[2][outside] == -5).all()
    assert (spec[outside] == 9.5).all() and (wave[outside] == -123.25).all()
    for e in range(first, first + count):
        _same_bank(bank, e, refs[e % 3], f"env {e}")
        hr.check_observation(refs[e % 3], name, wave[e], spec[e], f"gpu {name} tile rows env {e}")


def test_more_environments_than_one_window_launch():
    """E = 65537, W 64, B 4: the second turn of rp_hear_spectrum's slicing loop, an analysis grid of 1025 tile rows, a
    tracker grid of 65537 blocks.  Rows 0..2 against the reference; every row e bit-identical to row e % 3, compared on
    the device."""
    E = 65537
    trace, _ = ar.case_a()
    idx = torch.arange(E, device="cuda:0") % 3
    h = _make(E, "short", max_sub=4)
    assert h.n_envs > 65535, "more environments than the grid's y index takes"
    for c in range(5):
        spec, wave = h.observe(_trace(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB])[idx].contiguous(), window=True)
    for name, x in (("t_on", h.t_on), ("t_off", h.t_off), ("state", h.state), ("window", wave), ("spectrum", spec)):
        bits = x.view(torch.int64 if x.element_size() == 8 else torch.int32)
        assert bool((bits == bits[idx]).all()), f"{name}: a row differs from the row of its pattern"
    last = [E - 3, E - 2, E - 1]
    assert bool((wave[last].abs().amax(dim=1) > 0).all()) and bool((spec[last].abs().amax(dim=1) > 0).all())
    bank = tuple(_np(x[:3]) for x in (h.t_on, h.t_off, h.state))
    for e, r in enumerate(hr.stream_reference()[4]):
        _same_bank(bank, e, r, f"env {e}")
        hr.check_observation(r, "short", _np(wave[e]), _np(spec[e]), f"gpu slices env {e}")


@pytest.mark.parametrize("sr", [x[0] for x in hr.RATES])
def test_other_rates_and_timesteps(sr):
    """(44100, 0.005), (22050, 0.002), (8000, 0.0025), five bins at W = 512, the stream of case_a three rows at a time:
    sr T dt has a fraction after the calls that leave T odd (44.1 kHz) or no multiple of 10 (22.05 kHz), so
    rph_last_sample's floor decides N and the window's blocks start off the substep grid."""
    case = hr.wide_case(f"rates/{sr}")
    dt, tables = case["dt"], hr.rate_analysis(sr)
    trace, _ = ar.case_a()
    h = _make(3, tables, sr=sr, dt=dt, max_sub=hr.RATES_N_SUB)
    assert h._L.rp_hear_dim(h._h, b"sample_rate") == sr
    fractional = 0
    for c, envs in enumerate(hr.rates_reference(sr)):
        spec, wave = h.observe(_trace(trace[:, c * hr.RATES_N_SUB:(c + 1) * hr.RATES_N_SUB]), window=True)
        bank, spec, wave = _bank(h), _np(spec), _np(wave)
        fractional += hr.last_sample(envs[0]["T"], dt, sr) != round(sr * envs[0]["T"] * dt)
        for e, r in enumerate(envs):
            _same_bank(bank, e, r, f"{sr} Hz call {c} env {e}")
            hr.check_observation(r, tables, wave[e], spec[e], f"gpu {sr} Hz call {c} env {e}", dt=dt, sr=sr, tols=hr.WIDE_TOLS)
    assert c == 20 and (sr * dt != round(sr * dt)) == (sr != 8000)
    assert (fractional > 0) == (sr != 8000), "floor() must decide some N where sr dt is no integer"
    if sr == 8000:    # the 0.45 sr cut silences partials of key 87 that sound at 16 kHz
        assert (ar.partials(hr.default_timbre(), sr)[1][87] == 0).any() and (ar.partials(hr.default_timbre(), hr.SR)[1][87] != 0).any()


def test_harsh_timbre():
    """H = 8, amplitudes of mixed sign, partials gone in a few ms, 8 tau_rel = 0.08 s."""
    trace, _ = ar.case_a()
    h = _make(3, "small", timbre="harsh", max_sub=8)
    for c, envs in enumerate(hr.stream_reference(timbre="harsh")):
        spec, wave = h.observe(_trace(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB]), window=True)
        bank, spec, wave = _bank(h), _np(spec), _np(wave)
        for e, r in enumerate(envs):
            _same_bank(bank, e, r, f"harsh call {c} env {e}")
            hr.check_observation(r, "small", wave[e], spec[e], f"gpu harsh call {c} env {e}", timbre="harsh", tols=hr.WIDE_TOLS)


@pytest.mark.parametrize("key", hr.SINE_KEYS)
def test_a_held_pure_sine_reads_one(key):
    """One bin at the key's own fundamental, the key held for 60 substeps with the pure sine timbre: the float64 reference
    reads 1 within 1.5e-3 and the device reads what the reference reads.  A table uploaded transposed or scaled fails
    here even if tracker and window are right."""
    tables, r = hr.sine_analysis(key), hr.sine_reference(key)
    h = _make(1, tables, timbre="sine")
    spec, wave = h.observe(_trace(hr.sine_rows(key)[None]), window=True)
    want = float(hr.reference_spectrum(hr.window64_of(r, 2048, "sine"), *tables)[0])
    print(f"key {key}: the float64 reference reads {want:.6f}, the device {float(spec[0, 0]):.6f}")
    assert abs(want - 1.0) <= 1.5e-3
    _same_bank(_bank(h), 0, r, f"sine key {key}")
    hr.check_observation(r, tables, _np(wave)[0], _np(spec)[0], f"gpu sine key {key}", timbre="sine", tols=hr.WIDE_TOLS)


@pytest.mark.parametrize("T0", hr.LATE_T0)
def test_late_in_an_episode(T0):
    """The stream of case_a on an empty bank whose count starts at T0: T dt is 10 000 s, and 125 000 s with N just under
    the cap of 2e9.  The bank to the bit; window and spectrum against the windowed float64 reference."""
    trace, _ = ar.case_a()
    h = _make(3, "default", max_sub=8, T0=T0)
    for c, envs in enumerate(hr.stream_reference(T0=T0)):
        spec, wave = h.observe(_trace(trace[:, c * hr.N_SUB:(c + 1) * hr.N_SUB]), window=True)
        bank, spec, wave = _bank(h), _np(spec), _np(wave)
        for e, r in enumerate(envs):
            assert r["T"] == T0 + hr.N_SUB * (c + 1)
            _same_bank(bank, e, r, f"T0 {T0} call {c} env {e}")
            hr.check_observation(r, "default", wave[e], spec[e], f"gpu T0 {T0} call {c} env {e}", T0=T0, tols=hr.WIDE_TOLS)
    N = hr.last_sample(envs[0]["T"])
    assert N <= 2.0e9 and np.abs(spec).max() > 0.01
    if T0 == hr.LATE_T0[1]:
        assert N == 1_999_997_120 and N > 1.9e9


@pytest.mark.parametrize("name", ["default", "wide"])
def test_the_analysis_sums_in_the_order_the_header_promises(main_runs, name):
    """rp_hear.h: c_b is one fused multiply-add per term, j ascending from 0.  rph_analysis_host is that sentence in C; run
    on the device's own window it must give the device's spectrum, bit for bit."""
    runs = main_runs[name] if name in main_runs else _stream(name)[1]
    host = hr.HostHearing(3, hr.analysis(name))
    n = differ = 0
    worst = 0.0
    for c, got in enumerate(runs):
        spec, wave = got[3], got[4]
        want, _ = host.spectrum(of_window=wave)
        differ += int((want.view(np.uint32) != spec.view(np.uint32)).sum())
        n += spec.size
        worst = max(worst, float(np.abs(want.astype(np.float64) - spec).max()))
    print(f"{name}: {differ} of {n} magnitudes differ from the host chain on the device's window, by at most {worst:.3e}")
    assert np.abs(runs[-1][3]).max() > 0.01
    assert differ == 0


# ---- the wrapper --------------------------------------------------------------------------------------------------------
class _ScriptedHearingEnv:
    """No physics: `step` installs the scripted key trace and sustain activation and returns the scripted step types with
    a small observation of its own."""
    n_envs = 4

    def __init__(self, script, dt=hr.DT, key_trace=True):
        dev = torch.device("cuda", 0)
        self._script, self._t = script, 0
        self.key_trace = torch.zeros((4, hr.N_SUB, 4), dtype=torch.int32, device=dev) if key_trace else None
        self.physics = types.SimpleNamespace(device=dev)
        self.task = types.SimpleNamespace(physics_timestep=dt, piano=types.SimpleNamespace(
            sustain_activation=torch.zeros((4, 1), dtype=torch.bool, device=dev)))

    def observation_spec(self):
        return collections.OrderedDict(goal=specs.Array((3,), np.dtype(np.float32), name="goal"))

    def _timestep(self, step_type):
        obs = collections.OrderedDict(goal=torch.full((4, 3), float(self._t), dtype=torch.float32, device=self.physics.device))
        return TimeStep(_dev(np.asarray(step_type, np.int32)), None, None, obs)

    def reset(self):
        return self._timestep([int(StepType.FIRST)] * 4)

    def step(self, action):
        step_type, trace, sustain = self._script[self._t]
        self._t += 1
        self.key_trace.copy_(_trace(trace))
        self.task.piano.sustain_activation[:, 0] = _dev(np.asarray(sustain, bool))
        return self._timestep(step_type)

    def state_dict(self):
        return {"t": self._t}

    def load_state_dict(self, sd):
        self._t = sd["t"]


def _hearing_script(rng):
    """Per env a list of (step type, rows [4][4] uint32, sustain); an env's later episodes start with a FIRST step whose
    rows are junk.  Within an episode a key is struck at most twice, so nothing that sounds is forgotten."""
    FIRST, MID, LAST = int(StepType.FIRST), int(StepType.MID), int(StepType.LAST)

    def episode(n_steps):
        perm = rng.permutation(ar.N_KEYS)
        steps = []
        for i in range(n_steps):
            rows = np.zeros((hr.N_SUB, 4), np.uint32)
            keys = list(perm[3 * i:3 * i + 3]) + ([perm[3 * (i - 1)]] if i else [])
            for k in keys:
                a = int(rng.integers(0, 3))
                rows[a:int(rng.integers(a + 1, 5)), k // 32] |= np.uint32(1) << np.uint32(k % 32)
            steps.append((LAST if i == n_steps - 1 else MID, rows, bool(rng.integers(0, 2))))
        return steps
    lengths = {0: [3, 4, 9], 1: [6, 2, 7], 2: [12, 5], 3: [1, 1, 5, 8]}
    lanes = {}
    for e, eps in lengths.items():
        lane = []
        for i, n in enumerate(eps):
            if i:
                lane.append((FIRST, np.full((hr.N_SUB, 4), 0xFFFFFFFF, np.uint32), True))
            lane += episode(n)
        lanes[e] = lane
    n_steps = min(len(lane) for lane in lanes.values())
    script = [([lanes[e][t][0] for e in range(4)], np.stack([lanes[e][t][1] for e in range(4)]),
               [lanes[e][t][2] for e in range(4)]) for t in range(n_steps)]
    return lanes, script


def _episode_so_far(lane, t):
    """(rows, sustain flags) of the steps of the env's current episode up to step t; None at a FIRST step."""
    if lane[t][0] == int(StepType.FIRST):
        return None
    first = t
    while first > 0 and lane[first - 1][0] == int(StepType.MID):
        first -= 1
    return np.concatenate([lane[i][1] for i in range(first, t + 1)]), [lane[i][2] for i in range(first, t + 1)]


def test_audio_observation_wrapper_on_a_scripted_env():
    from robopianist_amd.wrappers import AudioObservationWrapper
    lanes, script = _hearing_script(np.random.default_rng(5))
    assert len(script) >= 15 and any(lanes[e][t][0] == 0 for e in range(4) for t in range(len(script)))
    with pytest.raises(ValueError, match="record_key_trace"):
        AudioObservationWrapper(_ScriptedHearingEnv(script, key_trace=False))
    with pytest.raises(ValueError, match="already part"):
        AudioObservationWrapper(_ScriptedHearingEnv(script), observation_key="goal")
    base = _ScriptedHearingEnv(script)
    env = AudioObservationWrapper(base, sample_rate=hr.SR, analysis=hr.analysis("default"), include_waveform=True)
    spec = env.observation_spec()
    assert list(spec) == ["goal", "audio", "audio_waveform"]
    assert spec["audio"].shape == (88,) and spec["audio"].dtype == np.float32
    assert spec["audio_waveform"].shape == (2048,) and spec["audio_waveform"].dtype == np.float32
    assert env.n_envs == 4 and env.key_trace is base.key_trace            # passthrough
    plain = AudioObservationWrapper(_ScriptedHearingEnv(script), sample_rate=hr.SR, window=128)
    assert list(plain.observation_spec()) == ["goal", "audio"] and plain.observation_spec()["audio"].shape == (88,)

    ts = env.reset()
    assert list(ts.observation) == ["goal", "audio", "audio_waveform"]
    assert ts.observation["audio"].shape == (4, 88) and ts.observation["audio"].dtype == torch.float32
    assert not bool(ts.observation["audio"].any()) and not bool(ts.observation["audio_waveform"].any())
    saved = after_saved = None
    restarts = 0
    for t in range(len(script)):
        if t == 8:
            saved = env.state_dict()
        ts = env.step(None)
        audio, wave = _np(ts.observation["audio"]), _np(ts.observation["audio_waveform"])
        if t == 8:
            after_saved = (audio.copy(), wave.copy())
        assert (_np(ts.observation["goal"]) == t + 1).all()
        for e in range(4):
            so_far = _episode_so_far(lanes[e], t)
            if so_far is None:
                restarts += 1
                assert not audio[e].any() and not wave[e].any(), f"step {t} env {e}: a FIRST step must read silence"
                assert not _np(env.hearing.state[e]).any()
                continue
            r = hr.reference_of_rows(*so_far)
            assert r["forgotten"] == 0 and int(env.hearing.forgotten[e]) == 0
            assert hr.same_bits(_np(env.hearing.t_on[e]), r["t_on"]) and hr.same_bits(_np(env.hearing.t_off[e]), r["t_off"])
            hr.check_observation(r, "default", wave[e], audio[e], f"wrapper step {t} env {e}")
    assert restarts >= 6 and np.abs(audio).max() > 0.01
    # the snapshot taken before step 8 replays step 8 to the bit, from a bank that has moved on since
    env.load_state_dict(saved)
    assert base._t == 8
    ts = env.step(None)
    assert hr.same_bits(_np(ts.observation["audio"]), after_saved[0]) and hr.same_bits(_np(ts.observation["audio_waveform"]), after_saved[1])
    ts = env.reset()
    assert not bool(ts.observation["audio"].any()) and not bool(ts.observation["audio_waveform"].any())
    assert not bool(env.hearing.state.any()) and bool((env.hearing.t_on == -1).all())


def test_audio_observation_end_to_end():
    """PianoWithShadowHands on the Twinkle replay, 2 envs: the observation equals Hearing.observe run by hand."""
    from robopianist_amd import suite
    from robopianist_amd.suite.scripted import ScriptedActions
    from robopianist_amd.wrappers import AudioObservationWrapper, CanonicalSpecWrapper
    actions = np.load(os.path.join(ROOT, "tests", "golden", "twinkle_twinkle_actions.npy"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = suite.load("RoboPianist-debug-TwinkleTwinkleRousseau-v0", n_envs=2, seed=11, record_key_trace=True,
                          task_kwargs=dict(trim_silence=True, control_timestep=0.05, gravity_compensation=True,
                                           primitive_fingertip_collisions=True))
    env = AudioObservationWrapper(CanonicalSpecWrapper(base))
    dev, dtype = base.physics.device, base.physics.dtype
    n_sub = int(base.key_trace.shape[1])
    by_hand = hearing.Hearing(2, physics_timestep=base.task.physics_timestep, max_substeps_per_call=n_sub)
    assert env.observation_spec()["audio"].shape == (88,) and "audio" not in base.observation_spec()
    script = ScriptedActions(torch.as_tensor(actions, dtype=dtype, device=dev), torch.zeros(2, dtype=torch.long, device=dev))
    ts = env.reset()
    assert not bool(ts.observation["audio"].any())
    sounded_at = None
    for t in range(40):
        ts = env.step(script)
        audio = ts.observation["audio"]
        want = by_hand.observe(base.key_trace, pedal=base.task.piano.sustain_activation[:, 0],
                               restart=ts.step_type == int(StepType.FIRST))
        assert audio.shape == (2, 88) and bool(torch.isfinite(audio).all())
        assert hr.same_bits(_np(audio), _np(want)), f"step {t}"
        if sounded_at is None and bool((base.key_trace[..., :3] != 0).any()):
            sounded_at = t
        if sounded_at is not None:
            assert bool(audio.any()), f"step {t}: a key has sounded since step {sounded_at}, the observation is all zeros"
    assert sounded_at is not None, "the replay pressed no key in 40 steps: the test shows nothing"
    assert int(by_hand.substeps[0]) == 40 * n_sub
    # (no reference sound is compared here, so forgotten voices hide nothing: a fingertip that chatters on a key strikes
    # it more than twice within 8 tau_rel, and the count says so)
    assert hr.same_bits(_np(env.hearing.state), _np(by_hand.state))
    loud = int(audio[0].argmax())
    print(f"first key activation at step {sounded_at}; after 40 steps the loudest bin of env 0 is key {loud} at "
          f"{float(audio[0, loud]):.4f}; forgotten voices: {_np(env.hearing.forgotten).tolist()}")
