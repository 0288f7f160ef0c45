"""MIDI events from the engine's per-substep activation trace.

The reference's MidiModule (robopianist/models/piano/midi_module.py:47-98) runs inside
`after_substep`: it XORs the current key activation with the previous one and emits timed
NoteOn / NoteOff / SustainOn / SustainOff messages.  The batched engine instead records
the activation of every substep as bit masks on the device (`rp_step(key_trace)`,
`Environment(record_key_trace=True)`); this module applies the same edge detection to
that trace, lazily and per env, on the host.  Its consumers are the MIDI export (`MidiFile.from_events(...).save("x.mid")`)
and the host side of the synthesiser (music/synthesizer.py: `notes_from_events`, `Synthesizer.get_samples`); the
synthesiser's device path reads the trace itself (include/audio/rp_audio.h) and follows this module's conventions."""

from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Union

import numpy as np

from robopianist_amd.music import midi_file


@dataclasses.dataclass
class NoteOn:
    note: int
    velocity: int
    time: float


@dataclasses.dataclass
class NoteOff:
    note: int
    time: float


@dataclasses.dataclass
class SustainOn:
    time: float


@dataclasses.dataclass
class SustainOff:
    time: float


MidiMessage = Union[NoteOn, NoteOff, SustainOn, SustainOff]


class MidiModule:
    """Edge detector over an activation trace of ONE environment."""

    def __init__(self, n_keys: int = 88) -> None:
        self._n_keys = n_keys
        self.initialize_episode()

    def initialize_episode(self) -> None:
        self._prev_activation = np.zeros(self._n_keys, dtype=bool)
        self._prev_sustain_activation = False
        self._midi_messages: List[List[MidiMessage]] = []

    def after_substep(self, time: float, activation: np.ndarray, sustain_activation: bool) -> None:
        """Same message order as the reference: note-ons, note-offs, sustain on, sustain off."""
        activation = np.asarray(activation, dtype=bool)
        sustain_activation = bool(np.asarray(sustain_activation).reshape(-1)[0])
        events: List[MidiMessage] = []
        change = activation ^ self._prev_activation
        for key_id in np.flatnonzero(change & ~self._prev_activation):
            # the reference hard-codes the maximum velocity (midi_module.py:66-69)
            events.append(NoteOn(note=midi_file.key_number_to_midi_number(int(key_id)), velocity=127, time=time))
        for key_id in np.flatnonzero(change & ~activation):
            events.append(NoteOff(note=midi_file.key_number_to_midi_number(int(key_id)), time=time))
        if sustain_activation and not self._prev_sustain_activation:
            events.append(SustainOn(time=time))
        if self._prev_sustain_activation and not sustain_activation:
            events.append(SustainOff(time=time))
        self._midi_messages.append(events)
        self._prev_activation = activation.copy()
        self._prev_sustain_activation = sustain_activation

    def consume_step(self, key_bits: np.ndarray, sustain_activation: bool, time_after_step: float,
                     physics_timestep: float) -> None:
        """One control step: `key_bits` is [n_substeps, n_keys] (engine.decode_key_trace of
        this env's slab), the sustain activation is the one latched for the step, and
        `time_after_step` is physics.time after the last substep."""
        n_sub = key_bits.shape[0]
        for s in range(n_sub):
            t = time_after_step - (n_sub - 1 - s) * physics_timestep
            self.after_substep(t, key_bits[s], sustain_activation)

    def get_latest_midi_messages(self) -> List[MidiMessage]:
        return self._midi_messages[-1]

    def get_all_midi_messages(self) -> List[MidiMessage]:
        return [m for step in self._midi_messages for m in step]


def events_from_trace(key_trace: np.ndarray, sustain: Sequence[bool], times: Sequence[float],
                      physics_timestep: float, env: int = 0, n_keys: int = 88) -> List[MidiMessage]:
    """All events of env `env` for a rollout: `key_trace` is [n_steps, n_envs, n_substeps, 4]
    uint32 (one `Environment.key_trace` per control step), `sustain[t]` / `times[t]` the
    sustain activation and physics time after step t."""
    from robopianist_amd import engine
    mod = MidiModule(n_keys)
    for t in range(len(times)):
        bits = engine.decode_key_trace(np.asarray(key_trace[t])[env:env + 1], n_keys)[0]
        mod.consume_step(bits, bool(sustain[t]), float(times[t]), physics_timestep)
    return mod.get_all_midi_messages()
