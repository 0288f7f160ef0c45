"""PianoSoundWrapper: records what the tracked envs play and writes it as WAV files (counterpart of
robopianist/wrappers/sound.py's PianoSoundVideoWrapper, built there on FluidSynth and ffmpeg; here on the batched HIP
synthesiser, include/audio/rp_audio.h)."""

from __future__ import annotations

import warnings
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

    Video is out of scope (there is no encoder to rely on); frames can be taken alongside the recording:

        env = PianoSoundWrapper(PixelWrapper(base, dict(height=240, width=320)), "recordings")
        ts = env.step(action); frame = ts.observation["pixels"][0].cpu().numpy()   # or base.physics.render(...)
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
