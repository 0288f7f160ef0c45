"""AudioObservationWrapper: adds what every env hears to the observation, on the batched HIP audio observation
(include/audio/rp_hear.h).  The reference has no counterpart: its synthesiser only records finished episodes."""

from __future__ import annotations

import collections

import numpy as np
import torch

from robopianist_amd.music import hearing
from robopianist_amd.suite import specs
from robopianist_amd.suite.specs import StepType


class AudioObservationWrapper:
    """The wrapped observation mapping gains `observation_key`: a device tensor [E, B] float32, the magnitudes of the
    newest `window` samples (at `sample_rate`) of what the env has played since its episode began, one per bin of
    `analysis` (default: the 88 key fundamentals, music.hearing.make_analysis); with `include_waveform` also
    `observation_key + "_waveform"`: those samples, [E, window] float32.

    Every step, `env.key_trace` and the step's latched sustain activation (`task.piano.sustain_activation`) are
    consumed into a per-env voice bank and the window is synthesised from it; a FIRST step restarts an env's bank (a
    resetting env is not simulated in that step), so its observation is silence.  All of it runs on the device with no
    read-back: this is the training path.  The tensors are the cached buffers of `music.hearing.Hearing`: they are
    overwritten by the next step.

    The environment must have been built with `record_key_trace=True`."""

    def __init__(self, environment, observation_key: str = "audio", sample_rate: int = 16000, window: int = 2048,
                 analysis=None, include_waveform: bool = False):
        if not hasattr(environment.task, "piano"):
            raise ValueError("AudioObservationWrapper only works with piano environments.")
        if getattr(environment, "key_trace", None) is None:
            raise ValueError("AudioObservationWrapper needs an environment built with record_key_trace=True.")
        self._environment = environment
        self._observation_key = observation_key
        self._waveform_key = observation_key + "_waveform" if include_waveform else None
        wrapped = environment.observation_spec()
        for key in filter(None, (observation_key, self._waveform_key)):
            if key in wrapped:
                raise ValueError(f"observation key {key!r} is already part of the wrapped observation")
        dev = environment.physics.device
        self._hearing = hearing.Hearing(
            n_envs=environment.n_envs, sample_rate=sample_rate, window=window, analysis=analysis,
            physics_timestep=float(environment.task.physics_timestep),
            max_substeps_per_call=int(environment.key_trace.shape[1]), device_id=dev.index or 0)
        self._all = torch.ones(environment.n_envs, dtype=torch.int32, device=dev)
        self._observation_spec = collections.OrderedDict(wrapped)
        self._observation_spec[observation_key] = specs.Array(
            (self._hearing.n_bins,), np.dtype(np.float32), name=observation_key)
        if self._waveform_key:
            self._observation_spec[self._waveform_key] = specs.Array(
                (self._hearing.window,), np.dtype(np.float32), name=self._waveform_key)

    def __getattr__(self, name):
        return getattr(self._environment, name)

    @property
    def hearing(self):
        """The music.hearing.Hearing behind the observation (its bank, `forgotten`, the analysis tables)."""
        return self._hearing

    def observation_spec(self):
        return self._observation_spec

    def _add_audio(self, timestep, restart):
        env = self._environment
        with torch.cuda.device(env.physics.device):
            out = self._hearing.observe(env.key_trace, pedal=env.task.piano.sustain_activation[:, 0], restart=restart,
                                        window=self._waveform_key is not None)
        obs = collections.OrderedDict(timestep.observation)
        if self._waveform_key:
            obs[self._observation_key], obs[self._waveform_key] = out
        else:
            obs[self._observation_key] = out
        return timestep._replace(observation=obs)

    def reset(self):
        return self._add_audio(self._environment.reset(), self._all)

    def step(self, action):
        timestep = self._environment.step(action)
        return self._add_audio(timestep, timestep.step_type == int(StepType.FIRST))

    def state_dict(self):
        """The wrapped env's snapshot plus the voice bank: `load_state_dict` continues the observations bit for bit."""
        return {"environment": self._environment.state_dict(), "hearing": self._hearing.state_dict()}

    def load_state_dict(self, sd):
        self._environment.load_state_dict(sd["environment"])
        self._hearing.load_state_dict(sd["hearing"])
