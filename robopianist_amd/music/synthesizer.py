"""Piano synthesis on the GPU: ctypes binding of include/audio/rp_audio.h (librp_audio.so).

The reference synthesises with FluidSynth and a soundfont (robopianist/music/synthesizer.py); here the sound is an
additive synthesiser defined in closed form in rp_audio.h -- damped, slightly inharmonic partials with an attack and a
release -- and computed for a whole batch of environments straight from the device-resident key trace.  The timbre is
the table below: data that is packed into the create blob, not code.  Like the engine and the renderer, the
synthesiser has no CPU fallback: a missing library is an error.
"""

from __future__ import annotations

import ctypes
import math
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from robopianist_amd import _abi
from robopianist_amd.music import constants as consts
from robopianist_amd.music import midi_module

EXPORTED_SYMBOLS = ("rp_audio_create", "rp_audio_destroy", "rp_audio_notes_from_trace", "rp_audio_synthesize",
                    "rp_audio_dim", "rp_audio_last_error")

N_KEYS = consts.NUM_KEYS
MAX_PARTIALS = 8
PEDAL_BIT = 88           # bit of the trace that carries the sustain pedal
TAIL_SECONDS = 1.0       # the reference's second of silence after the last event
_BLOB_MAGIC, _BLOB_VERSION = 0x55415052, 1


class AudioError(RuntimeError):
    pass


# --------------------------------------------------------------------------------------------------------- timbre
def make_timbre(n_partials: int = 8, tau_att: float = 0.002, tau_rel: float = 0.05) -> dict:
    """The default timbre: a_h = 1/h, tau_1(p) = 3 s * 2^(-(p-21)/24), tau_h = tau_1 / (1 + 0.25 (h-1)),
    B(p) = 1e-4 * 2^((p-21)/16).  Keys: H, a [H], tau [88][H] seconds, B [88], tau_att, tau_rel."""
    p = np.arange(N_KEYS) + consts.MIN_MIDI_PITCH_PIANO
    h = np.arange(1, n_partials + 1)
    tau1 = 3.0 * 2.0 ** (-(p - 21) / 24.0)
    return dict(H=int(n_partials), a=1.0 / h, tau=tau1[:, None] / (1.0 + 0.25 * (h[None, :] - 1)),
                B=1e-4 * 2.0 ** ((p - 21) / 16.0), tau_att=float(tau_att), tau_rel=float(tau_rel))


DEFAULT_TIMBRE = make_timbre()


def make_audio_blob(timbre: Optional[dict] = None, sample_rate: float = consts.SAMPLING_RATE) -> bytes:
    """The create blob of rp_audio_create: u32 magic, u32 version, i32 H, i32 0, then float64 sample rate, tau_att,
    tau_rel, a[8], B[88], tau[88][8] (rows beyond H padded)."""
    t = DEFAULT_TIMBRE if timbre is None else timbre
    H = int(t["H"])
    if not 1 <= H <= MAX_PARTIALS:
        raise ValueError(f"H must be in 1..{MAX_PARTIALS}, got {H}")
    a = np.zeros(MAX_PARTIALS)
    a[:H] = np.asarray(t["a"], np.float64).reshape(H)
    tau = np.ones((N_KEYS, MAX_PARTIALS))
    tau[:, :H] = np.broadcast_to(np.asarray(t["tau"], np.float64), (N_KEYS, H))
    B = np.broadcast_to(np.asarray(t["B"], np.float64), (N_KEYS,))
    body = np.concatenate([[float(sample_rate), float(t["tau_att"]), float(t["tau_rel"])], a, B, tau.reshape(-1)])
    return struct.pack("<IIii", _BLOB_MAGIC, _BLOB_VERSION, H, 0) + body.astype("<f8").tobytes()


# ------------------------------------------------------------------------------------------------- the notes rule
Note = Tuple[int, float, float, int]   # (key, t_on, t_off, velocity)


def events_from_substep_trace(trace: np.ndarray, dt: float) -> List[midi_module.MidiMessage]:
    """MidiModule's events of one environment's episode trace [T][4] uint32 (bits 0..87 keys, bit 88 the pedal): the
    event of substep s has time (s+1) dt."""
    from robopianist_amd import engine
    trace = np.ascontiguousarray(trace).view(np.uint32).reshape(-1, 4)
    bits = engine.decode_key_trace(trace[None], N_KEYS)[0]
    pedal = (trace[:, PEDAL_BIT // 32] >> (PEDAL_BIT % 32)) & 1
    mod = midi_module.MidiModule(N_KEYS)
    for s in range(trace.shape[0]):
        mod.after_substep((s + 1) * dt, bits[s], bool(pedal[s]))
    return mod.get_all_midi_messages()


def notes_from_events(events: Sequence[midi_module.MidiMessage], end_time: float) -> List[Note]:
    """The host twin of rp_audio_notes_from_trace over MidiModule messages (rp_audio.h, "Notes from the trace").
    Events that share a time are one substep: the rule sees the activation and the pedal after all of them.  A note
    still open at the end is released at `end_time`.  Ordered by onset, then key; not capped."""
    act = np.zeros(N_KEYS, bool)
    held = np.zeros(N_KEYS, bool)
    pedal = False
    open_note = {}
    notes: List[list] = []
    i, n = 0, len(events)
    while i < n:
        t = events[i].time
        prev = act.copy()
        velocity = {}
        while i < n and events[i].time == t:
            e = events[i]
            if isinstance(e, midi_module.NoteOn):
                k = e.note - consts.MIN_MIDI_PITCH_PIANO
                act[k] = True
                velocity[k] = e.velocity
            elif isinstance(e, midi_module.NoteOff):
                act[e.note - consts.MIN_MIDI_PITCH_PIANO] = False
            elif isinstance(e, midi_module.SustainOn):
                pedal = True
            elif isinstance(e, midi_module.SustainOff):
                pedal = False
            else:
                raise ValueError(f"Unknown event type: {e}")
            i += 1
        onset = act & ~prev
        now = act | (held & pedal)
        for k in np.flatnonzero(held & (onset | ~now)):
            if k in open_note:
                open_note.pop(k)[2] = t
        for k in np.flatnonzero(onset):
            open_note[k] = [int(k), t, None, int(velocity.get(k, consts.MAX_VELOCITY))]
            notes.append(open_note[k])
        held = now
    for note in open_note.values():
        note[2] = end_time
    notes.sort(key=lambda x: (x[1], x[0]))
    return [tuple(x) for x in notes]


# ------------------------------------------------------------------------------------------------------- binding
class Notes(ctypes.Structure):
    """rp_audio_notes (include/audio/rp_audio.h)."""
    _fields_ = [
        ("key", ctypes.c_void_p),
        ("t_on", ctypes.c_void_p),
        ("t_off", ctypes.c_void_p),
        ("velocity", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("dropped", ctypes.c_void_p),
    ]


class NotesArgs(ctypes.Structure):
    """rp_audio_notes_args."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("trace", ctypes.c_void_p),
        ("lengths", ctypes.c_void_p),
        ("trace_substeps", ctypes.c_int),
        ("env_first", ctypes.c_int), ("env_count", ctypes.c_int),
        ("dt", ctypes.c_double),
        ("notes", Notes),
        ("hip_stream", ctypes.c_void_p),
    ]


class SynthArgs(ctypes.Structure):
    """rp_audio_synth_args."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("notes", Notes),
        ("lengths", ctypes.c_void_p),
        ("substeps_cap", ctypes.c_int),
        ("n_cap", ctypes.c_int),
        ("env_first", ctypes.c_int), ("env_count", ctypes.c_int),
        ("dt", ctypes.c_double),
        ("wave", ctypes.c_void_p),
        ("pcm", ctypes.c_void_p),
        ("hip_stream", ctypes.c_void_p),
    ]


def n_samples(sample_rate: float, substeps: int, dt: float) -> int:
    """ceil(sr (T dt + 1.0)): the samples of an episode of T substeps, with the tail."""
    return int(math.ceil(float(sample_rate) * (float(substeps) * float(dt) + TAIL_SECONDS)))


_table = _abi.HandleTable("rp_audio_", {"notes_from_trace": NotesArgs, "synthesize": SynthArgs}, AudioError, "RP_AUDIO_LIB",
                          "librp_audio.so", "audio",
                          create=[ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int])
LIB_PATH = _table.path
load_library, declare = _table.load, _table.declare


class Synthesizer(_abi.Owner):
    """Batched synthesiser.  `physics_timestep` is the dt of the traces it is given (synthesize_trace can override
    it per call); `timbre` defaults to DEFAULT_TIMBRE.  The note lists live in device tensors of this object
    (`notes`): rp_audio_notes_from_trace fills them, `set_notes` writes one from the host."""

    def __init__(self, n_envs: int = 1, sample_rate: int = consts.SAMPLING_RATE, max_substeps: int = 8192,
                 max_notes: int = 2048, device_id: int = 0, physics_timestep: float = 0.005,
                 timbre: Optional[dict] = None):
        import torch
        self.n_envs, self.sample_rate = int(n_envs), sample_rate
        self.max_substeps, self.max_notes, self.device_id = int(max_substeps), int(max_notes), int(device_id)
        self.physics_timestep = float(physics_timestep)
        self.timbre = DEFAULT_TIMBRE if timbre is None else timbre
        self.blob = make_audio_blob(self.timbre, sample_rate)
        self._handle = _abi.Handle(_table, self.blob, len(self.blob), self.n_envs, self.max_substeps, self.max_notes,
                                   self.device_id)
        dev = self.device = torch.device("cuda", self.device_id)
        E, N = self.n_envs, self.max_notes
        self.notes = dict(key=torch.zeros((E, N), dtype=torch.int32, device=dev),
                          t_on=torch.zeros((E, N), dtype=torch.float64, device=dev),
                          t_off=torch.zeros((E, N), dtype=torch.float64, device=dev),
                          velocity=torch.zeros((E, N), dtype=torch.int32, device=dev),
                          count=torch.zeros(E, dtype=torch.int32, device=dev),
                          dropped=torch.zeros(E, dtype=torch.int32, device=dev))
        self._out = {}

    # -- helpers ---------------------------------------------------------------------------------------------
    @property
    def dropped(self):
        """[n_envs] int32 device tensor: the notes of the last list of every env that did not fit max_notes."""
        return self.notes["dropped"]

    def n_samples(self, substeps: int, dt: Optional[float] = None) -> int:
        return n_samples(self.sample_rate, substeps, self.physics_timestep if dt is None else dt)

    def outputs(self, n_cap: int, cache: bool = True):
        """(wave float32 [E, n_cap], pcm int16 [E, n_cap]); cached per row length unless `cache` is False."""
        import torch
        if cache and n_cap in self._out:
            return self._out[n_cap]
        out = (torch.zeros((self.n_envs, n_cap), dtype=torch.float32, device=self.device),
               torch.zeros((self.n_envs, n_cap), dtype=torch.int16, device=self.device))
        if cache:
            self._out[n_cap] = out
        return out

    def _stream(self, hip_stream):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream if hip_stream is None else hip_stream

    def _notes_struct(self) -> Notes:
        return Notes(*[self.notes[k].data_ptr() for k in ("key", "t_on", "t_off", "velocity", "count", "dropped")])

    def _lengths(self, lengths, cap: int):
        """[E] int32 device tensor; lengths given on the host are checked against `cap` here."""
        import torch
        if not isinstance(lengths, torch.Tensor):
            host = np.asarray(lengths, np.int64).reshape(-1)
            if host.size and (host.min() < 0 or host.max() > cap):
                raise AudioError(f"lengths must lie in [0, {cap}], got up to {int(host.max())}")
            lengths = torch.as_tensor(host.astype(np.int32), device=self.device)
        if tuple(lengths.shape) != (self.n_envs,) or lengths.dtype != torch.int32 or not lengths.is_cuda:
            raise AudioError(f"lengths: expected {self.n_envs} int32 values")
        return lengths.contiguous()

    def _window(self, env_first, env_count):
        return int(env_first), int(self.n_envs - env_first if env_count is None else env_count)

    # -- the two calls -----------------------------------------------------------------------------------------
    def notes_args(self, trace, lengths, dt, env_first=0, env_count=None, hip_stream=None) -> NotesArgs:
        first, count = self._window(env_first, env_count)
        return _abi.fill(NotesArgs, trace=trace.data_ptr(), lengths=lengths.data_ptr(), trace_substeps=int(trace.shape[1]),
                         env_first=first, env_count=count, dt=float(dt), notes=self._notes_struct(),
                         hip_stream=self._stream(hip_stream))

    def synth_args(self, lengths, dt, substeps_cap, wave, pcm, env_first=0, env_count=None, hip_stream=None) -> SynthArgs:
        first, count = self._window(env_first, env_count)
        return _abi.fill(SynthArgs, notes=self._notes_struct(), lengths=lengths.data_ptr(), substeps_cap=int(substeps_cap),
                         n_cap=int(wave.shape[1]), env_first=first, env_count=count, dt=float(dt), wave=wave.data_ptr(),
                         pcm=None if pcm is None else pcm.data_ptr(), hip_stream=self._stream(hip_stream))

    def notes_raw(self, args: NotesArgs) -> int:
        """rp_audio_notes_from_trace with a caller-made argument block; returns the C return code."""
        return self._handle.call_raw("notes_from_trace", args)

    def synthesize_raw(self, args: SynthArgs) -> int:
        """rp_audio_synthesize with a caller-made argument block; returns the C return code."""
        return self._handle.call_raw("synthesize", args)

    def _check_trace(self, trace):
        import torch
        if (not isinstance(trace, torch.Tensor) or not trace.is_cuda or trace.dim() != 3 or trace.shape[0] != self.n_envs
                or trace.shape[2] != 4 or trace.element_size() != 4 or trace.is_floating_point() or not trace.is_contiguous()):
            raise AudioError(f"trace: expected a contiguous 32-bit integer device tensor [{self.n_envs}, T, 4]")

    def notes_from_trace(self, trace, lengths, dt=None, env_first=0, env_count=None, hip_stream=None):
        """Fills `notes` (and `dropped`) of the envs of the window from `trace` [E, T, 4]; returns `notes`."""
        self._check_trace(trace)
        lengths = self._lengths(lengths, int(trace.shape[1]))
        self._handle.call("notes_from_trace", self.notes_args(trace, lengths, self.physics_timestep if dt is None else dt,
                                                              env_first, env_count, hip_stream))
        return self.notes

    def synthesize_notes(self, lengths, substeps_cap, dt=None, pcm=True, env_first=0, env_count=None, hip_stream=None,
                         cache=True):
        """Synthesises the current `notes`; returns (wave, pcm or None), rows of n_samples(substeps_cap) samples."""
        dt = self.physics_timestep if dt is None else dt
        lengths = self._lengths(lengths, int(substeps_cap))
        wave, pcm_t = self.outputs(self.n_samples(substeps_cap, dt), cache)
        self._handle.call("synthesize", self.synth_args(lengths, dt, substeps_cap, wave, pcm_t if pcm else None, env_first,
                                                        env_count, hip_stream))
        return wave, (pcm_t if pcm else None)

    def synthesize_trace(self, trace, lengths, pcm=True, env_first=0, env_count=None, dt=None, hip_stream=None):
        """trace: device tensor [E, T, 4] (int32 / uint32; bit 88 = pedal), lengths: [E] substeps of every env (a
        device int32 tensor, or host values, which are checked).  Returns the device tensors (wave float32
        [E, n_cap], pcm int16 [E, n_cap] or None) with n_cap = n_samples(T); they are this object's cached buffers
        and are overwritten by the next call with the same T.  Envs outside the window keep their rows."""
        self._check_trace(trace)
        lengths = self._lengths(lengths, int(trace.shape[1]))
        self.notes_from_trace(trace, lengths, dt, env_first, env_count, hip_stream)
        return self.synthesize_notes(lengths, int(trace.shape[1]), dt, pcm, env_first, env_count, hip_stream)

    def set_notes(self, env: int, notes: Sequence[Note]) -> None:
        """Writes a host note list ((key, t_on, t_off, velocity), ordered by onset then key) as env `env`'s list;
        what does not fit max_notes is dropped and counted."""
        import torch
        keep = list(notes)[:self.max_notes]
        n = len(keep)
        if n:
            arr = np.asarray(keep, np.float64)
            for name, col, dt in (("key", 0, torch.int32), ("t_on", 1, torch.float64), ("t_off", 2, torch.float64),
                                  ("velocity", 3, torch.int32)):
                self.notes[name][env, :n] = torch.as_tensor(arr[:, col], device=self.device).to(dt)
        self.notes["count"][env] = n
        self.notes["dropped"][env] = len(notes) - n

    def get_samples(self, event_list: Sequence[midi_module.MidiMessage]) -> np.ndarray:
        """Synthesises a list of MIDI events (absolute times, MidiModule.get_all_midi_messages) into int16 samples,
        peak-normalised, with one second of tail after the last event: the reference's Synthesizer.get_samples.
        Uses env 0 of this object."""
        if len(event_list) == 0:
            raise ValueError("get_samples needs at least one event")
        end = float(event_list[-1].time)
        self.set_notes(0, notes_from_events(event_list, end))
        # (one "substep" as long as the episode: T dt is then the end time to the bit)
        T, dt = (1, end) if end > 0 else (0, 1.0)
        lengths = [T] + [0] * (self.n_envs - 1)
        _, pcm = self.synthesize_notes(lengths, 1, dt=dt, pcm=True, env_first=0, env_count=1, cache=False)
        return pcm[0, :n_samples(self.sample_rate, T, dt)].cpu().numpy()
