"""PianoSoundWrapper records what the tracked envs play and writes it as WAV files; PianoSoundVideoWrapper films them
as well and writes AVI files with picture and sound (counterparts of robopianist/wrappers/sound.py's
PianoSoundVideoWrapper, built there on FluidSynth and ffmpeg; here on the batched HIP synthesiser, include/audio/
rp_audio.h, the batched HIP renderer, include/render/rp_render.h, and the batched HIP JPEG encoder, include/video/
rp_video.h)."""

from __future__ import annotations

import warnings
from fractions import Fraction
from pathlib import Path
from typing import Sequence

import torch

from robopianist_amd.music import audio, constants as consts, midi_file, synthesizer
from robopianist_amd.suite.specs import StepType


class PianoSoundWrapper:
    """Every step, the `env.key_trace` rows of the envs in `record_envs` are appended to a device buffer
    [n_tracked, max_substeps, 4], with the step's latched sustain activation (`task.piano.sustain_activation`) as
    bit 88 of every substep.  A FIRST step restarts an env's buffer (a resetting env is not simulated in that step),
    MID and LAST append, and LAST finalises the episode: it is synthesised on the device and written to
    `record_dir/{env:04d}_{counter:05d}.wav` (and `.mid` with `export_midi`).  An episode with no note -- silence, or
    pedal events only -- writes nothing, as in the reference.  Every `record_every`-th episode of an env is written.

    The environment must have been built with `record_key_trace=True`.  This is a recording tool, not the training
    path: it reads the tracked envs' step types back to the host every step (one small copy).

    PianoSoundVideoWrapper (below) records the picture as well.
    """

    def __init__(self, environment, record_dir, record_envs: Sequence[int] = (0,), record_every: int = 1,
                 sample_rate: int = consts.SAMPLING_RATE, export_midi: bool = False, max_substeps: int = 0,
                 max_notes: int = 4096):
        if not hasattr(environment.task, "piano"):
            raise ValueError("PianoSoundWrapper only works with piano environments.")
        if getattr(environment, "key_trace", None) is None:
            raise ValueError("PianoSoundWrapper needs an environment built with record_key_trace=True.")
        self._environment = environment
        self._record_dir = Path(record_dir)
        self._record_dir.mkdir(parents=True, exist_ok=True)
        self._envs = [int(e) for e in record_envs]
        if not self._envs or min(self._envs) < 0 or max(self._envs) >= environment.n_envs:
            raise ValueError(f"record_envs must name envs in [0, {environment.n_envs})")
        self._record_every = int(record_every)
        self._export_midi = bool(export_midi)
        self._dt = float(environment.task.physics_timestep)
        self._n_sub = int(environment.key_trace.shape[1])
        # default capacity: two minutes of playing
        self._cap = int(max_substeps) if max_substeps else int(round(120.0 / self._dt))
        dev = environment.physics.device
        self._synth = synthesizer.Synthesizer(n_envs=len(self._envs), sample_rate=sample_rate, max_substeps=self._cap,
                                              max_notes=max_notes, device_id=dev.index or 0,
                                              physics_timestep=self._dt)
        self._index = torch.as_tensor(self._envs, dtype=torch.long, device=dev)
        self._buffer = torch.zeros((len(self._envs), self._cap, 4), dtype=torch.int32, device=dev)
        self._length = [0] * len(self._envs)
        self._truncated = [False] * len(self._envs)
        self._counter = [0] * len(self._envs)
        self.written = []   # paths of the files written so far

    def __getattr__(self, name):
        return getattr(self._environment, name)

    def reset(self):
        timestep = self._environment.reset()
        for i in range(len(self._envs)):
            self._length[i], self._truncated[i] = 0, False
        return timestep

    def step(self, action):
        timestep = self._environment.step(action)
        step_type = timestep.step_type[self._index].cpu().tolist()   # the one read-back
        env, piano = self._environment, self._environment.task.piano
        for i, e in enumerate(self._envs):
            if step_type[i] == int(StepType.FIRST):
                self._length[i], self._truncated[i] = 0, False
                continue
            n = self._length[i]
            if n + self._n_sub > self._cap:
                if not self._truncated[i]:
                    warnings.warn(f"PianoSoundWrapper: env {e}'s episode is longer than max_substeps={self._cap}; "
                                  "the recording is truncated")
                self._truncated[i] = True
            else:
                rows = self._buffer[i, n:n + self._n_sub]
                rows.copy_(env.key_trace[e])
                pedal = piano.sustain_activation[e, 0].to(torch.int32) << (synthesizer.PEDAL_BIT % 32)
                rows[:, synthesizer.PEDAL_BIT // 32] |= pedal
                self._length[i] = n + self._n_sub
            if step_type[i] == int(StepType.LAST):
                self._finalize(i)
        return timestep

    def _finalize(self, i: int) -> None:
        counter, self._counter[i] = self._counter[i], self._counter[i] + 1
        if counter % self._record_every != 0:
            return
        s, e = self._synth, self._envs[i]
        s.notes_from_trace(self._buffer, self._length, env_first=i, env_count=1)
        count, dropped = int(s.notes["count"][i]), int(s.dropped[i])
        if count == 0:   # no events, or sustain events only
            return
        if dropped:
            warnings.warn(f"PianoSoundWrapper: env {e}: {dropped} notes beyond max_notes={s.max_notes} were dropped")
        # (rows as long as this episode, not as long as the buffer: the other envs' lengths do not matter here)
        length = self._length[i]
        lengths = [length if j == i else 0 for j in range(len(self._envs))]
        _, pcm = s.synthesize_notes(lengths, length, pcm=True, env_first=i, env_count=1, cache=False)
        stem = self._record_dir / f"{e:04d}_{counter:05d}"
        audio.write_wav(stem.with_suffix(".wav"), pcm[i].cpu().numpy(), s.sample_rate)
        self.written.append(stem.with_suffix(".wav"))
        if self._export_midi:
            trace = self._buffer[i, :self._length[i]].cpu().numpy()
            events = synthesizer.events_from_substep_trace(trace, self._dt)
            midi_file.MidiFile.from_events(events).save(stem.with_suffix(".mid"))
            self.written.append(stem.with_suffix(".mid"))


class PianoSoundVideoWrapper(PianoSoundWrapper):
    """PianoSoundWrapper that also films the tracked envs: the reference's class name and recording keywords
    (record_dir, record_every, camera_id, height, width, playback_speed), plus `record_envs` and `quality`; the
    remaining keywords are PianoSoundWrapper's (sample_rate, export_midi, max_substeps, max_notes).

    One frame is taken per control step, the FIRST step's (reset, or the step in which an env restarts) being the first
    of an episode.  Only the tracked envs are rendered (the renderer's env window, one launch per tracked env), with the
    task's key colours and fingertip colours; the images are encoded on the device (include/video/rp_video.h) and
    the JPEG files kept on the host.  LAST writes `record_dir/{env:04d}_{counter:05d}.avi`: a Motion-JPEG stream with one
    frame every control_timestep / playback_speed seconds (an exact rational) and, if the episode has a note, the
    synthesised sound as 16-bit PCM at sample_rate x playback_speed; an episode without a note is written as picture
    only.  An episode of n steps has n + 1 frames and n control_timestep + 1 seconds of sound, so picture and sound
    stay in step by construction.  No `.wav` is written.

    This is a recording tool, not the training path: next to PianoSoundWrapper's read-back of the step types, every
    step reads the tracked envs' JPEG lengths (with their step types, in one small copy) and then copies exactly
    those bytes to the host."""

    def __init__(self, environment, record_dir, record_envs: Sequence[int] = (0,), record_every: int = 1,
                 camera_id="piano/back", height: int = 480, width: int = 640, playback_speed: float = 1.0,
                 quality: int = 90, **sound_kwargs):
        super().__init__(environment, record_dir, record_envs=record_envs, record_every=record_every, **sound_kwargs)
        self._camera_id, self._height, self._width = camera_id, int(height), int(width)
        if not playback_speed > 0:
            raise ValueError("playback_speed must be positive")
        period = (Fraction(float(environment.task.control_timestep)).limit_denominator(10 ** 6)
                  / Fraction(float(playback_speed)).limit_denominator(10 ** 6))
        self._frame_period = (period.numerator, period.denominator)
        self._audio_rate = int(round(self._synth.sample_rate * float(playback_speed)))
        self._encoder = environment.physics.jpeg_encoder(self._height, self._width, len(self._envs), quality)
        self._frames = [[] for _ in self._envs]
        self._pending = []

    def _film(self, timestep):
        """Renders and encodes the tracked envs; returns their step types and appends their JPEG files."""
        env = self._environment
        task, physics = env.task, env.physics
        kw = dict(height=self._height, width=self._width, camera_id=self._camera_id)
        if hasattr(task, "key_rgb"):
            kw.update(key_rgb=task.key_rgb(physics), colorize_fingertips=bool(getattr(task, "colorize_fingertips", False)))
        for e in self._envs:
            rgb = physics.render(env_first=e, env_count=1, **kw)
        with torch.cuda.device(physics.device):
            data, length = self._encoder.encode(rgb.index_select(0, self._index).contiguous())
        # the one read-back of this wrapper: lengths and step types together
        both = torch.stack([length, timestep.step_type[self._index].to(torch.int32)]).cpu().tolist()
        for i, (n, st) in enumerate(zip(*both)):
            if st == int(StepType.FIRST):
                self._frames[i] = []
            self._frames[i].append(data[i, :n].cpu().numpy().tobytes())
        return both[1]

    def reset(self):
        timestep = super().reset()
        self._film(timestep)
        return timestep

    def step(self, action):
        self._pending = []
        timestep = super().step(action)   # appends the key trace; LAST calls _finalize, which defers to here
        self._film(timestep)
        for i in self._pending:
            self._write_episode(i)
        return timestep

    def _finalize(self, i: int) -> None:
        self._pending.append(i)

    def _write_episode(self, i: int) -> None:
        from robopianist_amd import video
        counter, self._counter[i] = self._counter[i], self._counter[i] + 1
        if counter % self._record_every != 0:
            return
        s, e = self._synth, self._envs[i]
        s.notes_from_trace(self._buffer, self._length, env_first=i, env_count=1)
        count, dropped = int(s.notes["count"][i]), int(s.dropped[i])
        if dropped:
            warnings.warn(f"PianoSoundVideoWrapper: env {e}: {dropped} notes beyond max_notes={s.max_notes} were dropped")
        pcm = None
        if count:   # (no events, or sustain events only: picture only)
            length = self._length[i]
            lengths = [length if j == i else 0 for j in range(len(self._envs))]
            _, out = s.synthesize_notes(lengths, length, pcm=True, env_first=i, env_count=1, cache=False)
            pcm = out[i].cpu().numpy()
        stem = self._record_dir / f"{e:04d}_{counter:05d}"
        video.write_avi(stem.with_suffix(".avi"), self._frames[i], self._frame_period, self._height, self._width,
                        pcm=pcm, sample_rate=self._audio_rate if pcm is not None else None)
        self.written.append(stem.with_suffix(".avi"))
        if self._export_midi and count:
            trace = self._buffer[i, :self._length[i]].cpu().numpy()
            events = synthesizer.events_from_substep_trace(trace, self._dt)
            midi_file.MidiFile.from_events(events).save(stem.with_suffix(".mid"))
            self.written.append(stem.with_suffix(".mid"))
